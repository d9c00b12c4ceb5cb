"""Merged LoRA adapters: achieved HBM GB/s of vlb_lora_merge at the 7B decoder shapes, the whole-model merge, and one
validation step on merged versus unmerged weights (7B geometry, LoRA r=16, B=3, synthetic batch).

  python tools/bench_lora_merge.py [--out profiles/lora_merge.txt] [--skip-model]

Warm-up, then the median of per-repetition HIP-event times on one stream.  Every repetition of a kernel row works on
its own W / Wm pair out of a ring larger than the 256 MiB Infinity Cache, so the figures are HBM figures.  The AdamW and
transpose rows are this repository's own HBM-bound yardsticks (tools/bench_hbm_kernels.py) timed the same way.
"""
import argparse
import os
import statistics
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phantom_vlb_amd import ops  # noqa: E402
from phantom_vlb_amd._lib import check, lib  # noqa: E402

BF = torch.bfloat16
dev = torch.device("cuda:0")
PEAK = 8000.0           # GB/s, HBM3E spec
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def median_ms(fns, warmup=3):
    """fns: one callable per timed repetition (the first ``warmup`` are also used to warm up)."""
    for f in fns[:warmup]:
        f()
    torch.cuda.synchronize()
    ts = []
    for f in fns:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def row(name, nbytes, ms):
    gbs = nbytes / ms / 1e6
    say(f"{name:44s} {nbytes / 1e6:9.1f} MB  {ms * 1e3:9.1f} us  {gbs:7.0f} GB/s  {gbs / PEAK * 100:5.1f}% of 8 TB/s")
    return gbs


def kernels():
    g = torch.Generator(device=dev).manual_seed(0)

    def rnd(*shape, std=0.02):
        return (torch.randn(*shape, device=dev, generator=g) * std).to(BF)
    say("# yardsticks (same method)")
    n = 65536 * 4096
    mst, grd, m1, v1 = (torch.zeros(n, device=dev) for _ in range(4))
    cp = torch.zeros(n, device=dev, dtype=BF)
    ss = torch.zeros(1, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    adam = row("adamw_step (268 M params, 30 B each)", n * 30, median_ms([lambda: check(lib.vlb_adamw_step(
        mst.data_ptr(), cp.data_ptr(), grd.data_ptr(), m1.data_ptr(), v1.data_ptr(), n, 1e-4, 0.9, 0.999, 1e-8, 1e-2, 1,
        ss.data_ptr(), 1.0, st), "adamw")] * 7))
    del mst, grd, m1, v1, cp
    xs = [rnd(28672, 4096) for _ in range(3)]
    row("transpose_bf16 [28672x4096]", 2 * xs[0].numel() * 2, median_ms([(lambda x=x: ops.transpose(x)) for x in xs * 3]))
    del xs
    torch.cuda.empty_cache()
    say()
    say("# vlb_lora_merge: 4 B of traffic per weight element (W read once, Wm written once)")
    shapes = (("q / o    [4096 x 4096]", 4096, 4096, False), ("k / v    [1024 x 4096]", 1024, 4096, False),
              ("gate+up  [2 x 14336 x 4096] interleaved", 14336, 4096, True), ("down     [4096 x 14336]", 4096, 14336, False))
    frac = {}
    for R in (16, 64):
        for name, N, K, il in shapes:
            rows = 2 * N if il else N
            copies = max(3, -(-600_000_000 // (rows * K * 2)))
            Ws = [rnd(rows, K) for _ in range(copies)]
            Wms = [torch.empty_like(w) for w in Ws]
            A, bts = rnd(2 * R, K), [rnd(R, N), rnd(R, N)]

            def one(i):
                if il:
                    ops.lora_merge(Ws[i], Wms[i], bts[0], A[:R], 2.0, ops.MERGE_GATE)
                    ops.lora_merge(Ws[i], Wms[i], bts[1], A[R:], 2.0, ops.MERGE_UP)
                else:
                    ops.lora_merge(Ws[i], Wms[i], bts[0], A[:R], 2.0)
            reps = [(lambda i=i: one(i)) for i in range(copies)]
            frac[(R, name)] = row(f"R={R:2d} {name}", rows * K * 4, median_ms(reps)) / adam
            del Ws, Wms
            torch.cuda.empty_cache()
    say()
    say("# fraction of the AdamW yardstick's achieved GB/s: " + ", ".join(f"R={R} {n.split()[0]} {v:.2f}" for (R, n), v in frac.items()))


def model():
    from phantom_vlb_amd.litmodule import VLBLitModule, VLBLitModuleConfig
    from phantom_vlb_amd.synthetic import synthetic_batch
    warnings.simplefilter("ignore")
    cfg = VLBLitModuleConfig(model_path="DAMO-NLP-SG/VideoLLaMA2-7B", freeze_backbone=False, use_lora=True, lora_r=16, lora_alpha=32,
                             lora_dropout=0.1, dropout_rate=0.1, num_target=2048, l2_lambda=1e-3, lr=1e-4, betas=[0.9, 0.999],
                             eps=1e-8, weight_decay=1e-2, lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=50000,
                             geometry="7b", merge_lora_for_eval=True)
    m = VLBLitModule(cfg)
    m.configure_model()
    m.configure_optimizers()
    g = m.geometry
    # fresh adapters have B = 0: give B values so that the merge is not the identity (timing does not depend on it)
    for n, t in m.lora.master.items():
        if "lora_B" in n:
            t[:m.lora.r].normal_(std=0.02)
    m.lora.refresh(from_master=True)
    batch = synthetic_batch(g, 3, seed=1234, device=dev)
    batch["language"], batch["padvals"] = batch["language"].cpu(), batch["padvals"].cpu()
    say()
    say(f"# 7B decoder ({g.layers} layers, LoRA r=16 on the seven linears), B=3 synthetic batch")

    def remerge():
        m.lora.version += 1
        m.lora.merge()
    t_merge = median_ms([remerge] * 5, warmup=1)
    nbytes = sum(t.numel() * 4 for lw in m.lora.merge() for k, t in lw.items() if k.startswith("w"))
    row(f"whole-model merge ({7 * g.layers} launches)", nbytes, t_merge)

    def val(merged):
        m.config.merge_lora_for_eval = merged
        return m.validation_step(batch)
    for merged in (True, False):
        val(merged)
    torch.cuda.synchronize()
    ts = {True: [], False: []}
    for _ in range(5):                                   # interleaved rounds, same process
        for merged in (True, False):
            ts[merged].append(median_ms([lambda: val(merged)] * 3, warmup=0))
    tm, tu = statistics.median(ts[True]), statistics.median(ts[False])
    say(f"validation step, unmerged (adapted decoder)      {tu:9.2f} ms   rounds: " + " ".join(f"{t:.2f}" for t in ts[False]))
    say(f"validation step, merged (frozen path)            {tm:9.2f} ms   rounds: " + " ".join(f"{t:.2f}" for t in ts[True]))
    say(f"saving per validation batch                      {tu - tm:9.2f} ms   ({(tu - tm) / tu * 100:.1f}%)")
    if tu > tm:
        say(f"one merge ({t_merge:.2f} ms) is paid back after {t_merge / (tu - tm):.1f} validation batches")
    a, b = val(True), val(False)
    say(f"merged vs unmerged: loss {float(a['loss']):.6f} / {float(b['loss']):.6f}, "
        f"max |pred diff| / max |pred| = {float((a['brain_preds'] - b['brain_preds']).abs().max() / b['brain_preds'].abs().max()):.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--skip-model", action="store_true", help="kernel rows only (no 7B module)")
    a = ap.parse_args()
    say(f"# tools/bench_lora_merge.py on {torch.cuda.get_device_name(0)}")
    kernels()
    if not a.skip_model:
        model()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
