"""Frozen-backbone feature cache at 7B geometry (random-init weights, frozen, B=5): what a head-only step costs.

For V = 1000 (the reference's baseline experiment) and V = 2048 (configs[1]) one JSON line with
  * the uncached training step and validation step (wall ms per step: training_step + optimiser + scheduler);
  * the cached training step and validation step: GPU ms from event pairs around each step with the host queued ahead
    of the device (a spin kernel in front holds the stream, so the pair brackets the step's kernels back to back), and
    wall ms per step over --steps (>= 200) steps;
then one line with the item load time of the synthetic set, full item against ``features_only``, and the projected
wall time of the baseline schedule (10 epochs, 5 validation passes per epoch) with and without the cache for the given
clip counts (data loading not included).
Product library only (no VLB_LIB): python tools/bench_feature_cache.py [--steps 300]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300, help="timed cached steps (>= 200)")
    ap.add_argument("--uncached-steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=5)
    ap.add_argument("--targets", type=str, default="1000,2048")
    ap.add_argument("--items", type=int, default=4, help="items timed per load mode")
    ap.add_argument("--n-train", type=int, default=4000, help="training clips of the projected run")
    ap.add_argument("--n-val", type=int, default=800, help="validation clips of the projected run")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--val-passes", type=int, default=5, help="validation passes per epoch (val_check_interval 0.2)")
    return ap.parse_args()


def wall_ms(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def gpu_ms(fn, n):
    """Median device time of one step: a ~20 ms spin kernel holds the stream while the host enqueues the step, so the
    event pair measures the step's kernels without the host's launch gaps."""
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        torch.cuda._sleep(50_000_000)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    out.sort()
    return out[len(out) // 2]


def main():
    a = parse()
    if a.steps < 200:
        sys.exit("bench_feature_cache: --steps must be >= 200")
    warnings.simplefilter("ignore")
    from phantom_vlb_amd import _lib
    if not _lib.IS_PRODUCT_LIB:
        sys.exit("bench_feature_cache: VLB_LIB is set; only the in-tree product library is measured")
    from phantom_vlb_amd.datamodule import VLB_Dataset
    from phantom_vlb_amd.feature_cache import FeatureCache
    from phantom_vlb_amd.head import BrainHead
    from phantom_vlb_amd.litmodule import VLBLitModule, VLBLitModuleConfig
    from phantom_vlb_amd.synthetic import synthetic_batch

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    targets = [int(x) for x in a.targets.split(",")]
    B = a.batch
    cfg = VLBLitModuleConfig(model_path="none", freeze_backbone=True, use_lora=False, lora_r=None, lora_alpha=None,
                             lora_dropout=None, dropout_rate=0.1, num_target=targets[0], l2_lambda=1e-3, lr=1e-4,
                             betas=[0.9, 0.999], eps=1e-8, weight_decay=1e-2, lr_scheduler_name="CosineAnnealingLR",
                             last_epoch=-1, t_max=50000, geometry="7b", cache_features=True)
    m = VLBLitModule(cfg)
    m.configure_model()
    g = m.geometry
    results = []
    for V in targets:
        if V != m.head.V:                      # same frozen backbone, a fresh head of V targets
            m.config.num_target = V
            m.head = BrainHead(g.dim, V, cfg.l2_lambda, g.ln_eps, dev, seed=cfg.init_seed)
            m.flat = None
        opts, scheds = m.configure_optimizers()
        opt, sch = opts[0], scheds[0]["scheduler"]
        batch = synthetic_batch(g, B, seed=1234, device=dev)
        batch["language"], batch["padvals"] = batch["language"].cpu(), batch["padvals"].cpu()
        batch["timeseries"] = torch.randn(B, V, device=dev)
        plain = dict(batch)                    # no "index": the uncached step
        indexed = dict(batch, index=torch.arange(B, dtype=torch.int64))
        m.feature_caches.clear()
        m.feature_caches["train"] = FeatureCache("train", 64, g.dim, dev)
        m.feature_caches["val"] = FeatureCache("val", 64, g.dim, dev)

        def train_step(bt):
            m.training_step(bt)
            opt.step()
            sch.step()

        for _ in range(a.warmup):
            train_step(plain)
            m.validation_step(plain)
        unc_train = wall_ms(lambda: train_step(plain), a.uncached_steps)
        unc_val = wall_ms(lambda: m.validation_step(plain), a.uncached_steps)
        train_step(indexed)                    # fills the caches (an uncached step that also stores)
        m.validation_step(indexed)
        assert m.feature_caches["train"].complete() is False and m.feature_caches["train"].lookup(indexed["index"])
        for _ in range(20):
            train_step(indexed)
            m.validation_step(indexed)
        r = {"what": "feature cache, 7B frozen, random-init weights", "B": B, "V": V,
             "uncached_train_step_ms": round(unc_train, 2), "uncached_val_step_ms": round(unc_val, 2),
             "cached_train_step_gpu_ms": round(gpu_ms(lambda: train_step(indexed), 50), 4),
             "cached_val_step_gpu_ms": round(gpu_ms(lambda: m.validation_step(indexed), 50), 4),
             "cached_train_step_wall_ms": round(wall_ms(lambda: train_step(indexed), a.steps), 4),
             "cached_val_step_wall_ms": round(wall_ms(lambda: m.validation_step(indexed), a.steps), 4),
             "timed_steps": a.steps}
        print(json.dumps(r), flush=True)
        results.append(r)

    # ---- item load time on the synthetic set (7B geometry): full item against features_only
    ds = VLB_Dataset([(1234, a.items)], "7b", targets[0])

    def load_ms(features_only):
        ds.features_only = features_only
        t0 = time.perf_counter()
        for i in range(a.items):
            ds[i]
        return (time.perf_counter() - t0) * 1e3 / a.items
    full_ms, feat_ms = load_ms(False), load_ms(True)

    # ---- projected wall time of the baseline schedule (compute only, per target count)
    st, sv = math.ceil(a.n_train / B), math.ceil(a.n_val / B)
    proj = {}
    for r in results:
        without = a.epochs * st * r["uncached_train_step_ms"] + a.epochs * a.val_passes * sv * r["uncached_val_step_ms"]
        with_c = (st * r["uncached_train_step_ms"] + (a.epochs - 1) * st * r["cached_train_step_wall_ms"]
                  + sv * r["uncached_val_step_ms"] + (a.epochs * a.val_passes - 1) * sv * r["cached_val_step_wall_ms"])
        proj[str(r["V"])] = {"without_cache_s": round(without / 1e3, 1), "with_cache_s": round(with_c / 1e3, 1)}
    print(json.dumps({"what": "item load (synthetic set, 7B geometry) and projected baseline schedule",
                      "full_item_ms": round(full_ms, 2), "features_only_item_ms": round(feat_ms, 2), "items": a.items,
                      "projection": {"n_train": a.n_train, "n_val": a.n_val, "epochs": a.epochs, "val_passes_per_epoch":
                                     a.val_passes, "batch": B, "by_V": proj,
                                     "note": "step compute only (data loading excluded)"}}), flush=True)


if __name__ == "__main__":
    main()
