"""``ridge_fit="closed_form"`` through the module and both runners (VLB_mini_synthetic and its multi-subject variant, mini
geometry, synthetic clips): when the fit runs, what it leaves in the masters and in AdamW's moments, the first loss after
it, and that the unset option is the parent commit's run bit for bit.

Bars: the first training mse after the solve is compared with the data term of J for the EMULATOR's solution (fp64 numpy,
tests/ridge_emul.py, bf16-rounded as the kernels read it) on that batch's own z, to the ridge stage's bars of
tests/head_emul.py - its loss bar plus its pred bar carried through the square, as in test_gpu_ridge_solve.py; per-subject
masters are within ``ridge_emul.master_bar`` (one fp32 ulp + E cond_2 2^-53 max|W|) of the emulator's solve over that subject's
clips alone.  tests/golden/ridge_fit_parent_run.json was recorded by the parent commit's own build running the command of
``test_unset_option_is_the_parent_commits_run`` on an MI355X."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import head_emul as HE
import ridge_emul as RE

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WN, BN = "ridge_layer.linear.weight", "ridge_layer.linear.bias"
LN = ("layer_norm1.weight", "layer_norm1.bias", "layer_norm2.weight", "layer_norm2.bias")


def _cfg(**kw):
    from phantom_vlb_amd.litmodule import VLBLitModuleConfig
    base = dict(model_path="none", freeze_backbone=True, use_lora=False, lora_r=None, lora_alpha=None, lora_dropout=None,
                dropout_rate=0.1, num_target=128, l2_lambda=1e-3, lr=1e-3, betas=[0.9, 0.999], eps=1e-8,
                weight_decay=1e-2, lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=50000, geometry="mini")
    base.update(kw)
    return VLBLitModuleConfig(**base)


def _dm(subjects=None):
    from phantom_vlb_amd.datamodule import VLBDataModule, VLBDataModuleConfig
    path = "synthetic:3x8" if subjects is None else "synthetic:3x4"          # the two YAMLs' stores
    return VLBDataModule(VLBDataModuleConfig(lazyload_path=path, subject="sub-99", seasons=["s1"], delay=3, window=3,
                                             random_state=1234, shuffle_val_data=False, batch_size=4, geometry="mini",
                                             num_target=128, subjects=subjects))


class _Rec:
    def __init__(self):
        self.rows = []

    def log_metrics(self, metrics, step):
        self.rows.append(dict(metrics))


def _moments(m, names):
    f = m.flat
    return {n: (f.m[o:o + k].clone(), f.v[o:o + k].clone()) for n, (o, k, _) in f.offsets.items() if n in names}


def _split_features(m, ds):
    """z (the device's bf16 features, as fp64), y (through bf16, as every step sees it) and the subject of every train clip"""
    cache = m.feature_caches["train"]
    was = ds.features_only
    ds.features_only = True
    items = [ds[i] for i in range(len(ds))]
    ds.features_only = was
    z = m.head.features_cached(cache, torch.arange(len(ds))).float().cpu().double().numpy().copy()
    y = torch.stack([it["timeseries"] for it in items]).to(torch.bfloat16).double().numpy()
    sub = np.array([int(it["subject"]) for it in items]) if "subject" in items[0] else None
    return z, y, sub


def _fit(epochs=2, subjects=None, **kw):
    """The built-in runner on the YAML's loop; every closed-form fit and every training step is recorded."""
    from phantom_vlb_amd.litmodule import VLBLitModule
    from phantom_vlb_amd.trainer import Trainer
    m = VLBLitModule(_cfg(subjects=subjects, **kw))
    m.configure_model()
    dm = _dm(subjects)
    fits, steps = [], []
    orig, ts = m.fit_ridge_closed_form, m.training_step

    def fit_spy(*a, **k):
        before = _moments(m, set(m.head.param_names))
        z, y, sub = _split_features(m, dm.datasets.train)
        out = orig(*a, **k)
        torch.cuda.synchronize()
        rec = dict(epoch=getattr(tr, "current_epoch", None), global_step=tr.global_step, steps_before=len(steps), out=out, z=z, y=y,
                   sub=sub, masters={n: t.clone() for n, t in m.head.master.items()},
                   compute={n: t.clone() for n, t in m.head.compute.items()}, moments_before=before,
                   moments_after=_moments(m, set(m.head.param_names)), logged={k2: v for k2, v in m.logged.items() if k2.startswith("ridge_fit/")})
        orig(*a, **k)                       # a direct call on the same cache: the same masters, bit for bit
        torch.cuda.synchronize()
        rec["direct"] = {n: t.clone() for n, t in m.head.master.items()}
        fits.append(rec)
        return out

    def step_spy(batch):
        cache = m.feature_caches.get("train")
        rec = dict(index=batch["index"].clone() if "index" in batch else None, cached=False)
        if m.config.ridge_fit and cache is not None and "index" in batch and cache.valid[batch["index"].numpy()].all():
            rec.update(cached=True, z=m.head.features_cached(cache, batch["index"]).float().cpu().double(),
                       W=m.head.compute[WN].float().cpu().double(), b=m.head.compute[BN].float().cpu().double(),
                       y=batch["timeseries"].to(torch.bfloat16).double().cpu())
        loss = ts(batch)
        rec["terms"] = m.head.loss_terms.double().cpu()
        steps.append(rec)
        return loss
    m.fit_ridge_closed_form, m.training_step = fit_spy, step_spy
    rec = _Rec()
    tr = Trainer(max_epochs=epochs, val_check_interval=0.5, log_every_n_steps=1, logger=rec)
    tr.fit(m, dm)
    torch.cuda.synchronize()
    return dict(module=m, dm=dm, fits=fits, steps=steps, rows=rec.rows,
                train=[r["train/brain_loss"] for r in rec.rows if "train/brain_loss" in r],
                val=[r["val/brain_loss"] for r in rec.rows if "val/brain_loss" in r])


@pytest.fixture(scope="module")
def runs(dev, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("ridge_fcache"))
    kw = dict(cache_features=True, ridge_fit="closed_form", dropout_rate=0.0, feature_cache_dir=d)
    cold = _fit(epochs=2, **kw)
    warm = _fit(epochs=1, **kw)                  # the cache persisted by `cold` loads: complete before the first step
    return cold, warm


def _check_fit_record(f, n_clips):
    assert [o["n"] for o in f["out"]] == [n_clips] and f["out"][0]["info"] == 0 and f["out"][0]["l2_lambda"] == 1e-3
    for n, t in f["masters"].items():
        assert torch.equal(f["direct"][n], t), f"{n}: a direct fit_ridge_closed_form call on the same cache gives other bits"
    for n in (WN, BN):
        assert not bool(f["moments_after"][n][0].any()) and not bool(f["moments_after"][n][1].any()), f"{n}: moments not zeroed"
        assert np.array_equal(f["compute"][n].float().cpu().numpy(), RE.rne_bf16(f["masters"][n].cpu().numpy()))
    for n in LN:
        assert torch.equal(f["moments_after"][n][0], f["moments_before"][n][0]) and torch.equal(f["moments_after"][n][1], f["moments_before"][n][1])
    lg = f["logged"]
    assert lg["ridge_fit/n"] == n_clips and lg["ridge_fit/l2_lambda"] == 1e-3
    assert lg["ridge_fit/train_mse_after"] < lg["ridge_fit/train_mse_before"]


def test_cold_cache_fits_once_at_the_end_of_the_first_epoch(runs):
    cold, _ = runs
    assert len(cold["fits"]) == 1
    f = cold["fits"][0]
    assert (f["epoch"], f["global_step"], f["steps_before"]) == (0, 4, 4)          # after epoch 1's four steps, before epoch 2's first
    _check_fit_record(f, 16)
    m = cold["module"]
    assert m.optimizer.step_count == 8                                                # the bias-correction count was left alone
    # AdamW had moved every tensor during epoch 1: the LN moments the fit left alone are not zero, the ridge ones were
    assert all(bool(f["moments_before"][n][0].any()) for n in LN + (WN, BN))
    assert [s["cached"] for s in cold["steps"]] == [False] * 4 + [True] * 4
    assert m.head._ridge is None                                                      # the sums are freed after the solve


def test_persisted_cache_fits_before_the_first_step(runs):
    cold, warm = runs
    assert len(warm["fits"]) == 1
    f = warm["fits"][0]
    assert (f["global_step"], f["steps_before"]) == (0, 0)
    _check_fit_record(f, 16)
    assert all(s["cached"] for s in warm["steps"]) and len(warm["steps"]) == 4
    assert not any(bool(f["moments_before"][n][0].any()) for n in LN)                 # no step yet: nothing to preserve, nothing set
    # the same cache, but the LN parameters of a fresh module (cold solved after four AdamW steps on them): other weights
    assert not torch.equal(f["masters"][WN], cold["fits"][0]["masters"][WN])


@pytest.mark.parametrize("which", ["cold", "warm"])
def test_first_mse_after_the_solve_is_the_emulators(runs, which):
    run = runs[0] if which == "cold" else runs[1]
    f = run["fits"][0]
    s = run["steps"][f["steps_before"]]                  # the first training step after the solve (dropout_rate = 0)
    assert s["cached"]
    sol = RE.solve(RE.sums(f["z"], f["y"], chunk=512), 1e-3)
    cond = RE.cond2(sol["A"])
    E = f["z"].shape[1]
    dW = np.abs(f["masters"][WN].cpu().numpy().astype(np.float64) - sol["W"].astype(np.float32).astype(np.float64))
    rW = float(np.max(dW / RE.master_bar(sol["W"], cond, E)))
    Wr = torch.from_numpy(RE.rne_bf16(sol["W"].astype(np.float32)).astype(np.float64))
    br = torch.from_numpy(RE.rne_bf16(sol["b"].astype(np.float32)).astype(np.float64))
    B, V = s["y"].shape
    ref = HE.ridge(s["z"], Wr, br, s["y"], 1e-3)
    bars = HE.ridge_bars(ref, B, E, V)
    d = (ref["pred"] - s["y"]).abs()
    bar = float(bars["loss"][0] + (2 * (d * bars["pred"]).sum() + (bars["pred"] ** 2).sum()) / (B * V))
    got, want = float(s["terms"][0]), float(ref["loss"][0])
    print(f"{which}: cond_2 {cond:.1f}, masters err / bar {rW:.3f}; first mse after the solve {got:.9f} vs emulator {want:.9f}: "
          f"err / bar {abs(got - want) / bar:.3e}; logged before / after {f['logged']}")
    assert rW <= 1
    assert abs(got - want) <= bar
    # N = 16 clips against E = 512 features: the fit interpolates up to the penalty, far below anything AdamW reached
    before = [float(x["terms"][0]) for x in run["steps"][:f["steps_before"]]]
    assert all(got < b for b in before)


def test_unset_option_is_the_parent_commits_run(dev):
    """ridge_fit=None: the losses and the head masters of the cached fit equal what the parent commit's build produced."""
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "ridge_fit_parent_run.json")))
    got = _fit(epochs=2, cache_features=True)
    assert got["fits"] == [] and "_ridge_fit_done" not in got["module"].__dict__
    assert getattr(got["module"].head, "_ridge", None) is None
    assert got["train"] == gold["train"], (got["train"], gold["train"])
    assert got["val"] == gold["val"], (got["val"], gold["val"])
    for n, t in got["module"].head.master.items():
        assert hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest() == gold["masters"][n], n
    assert not any(k.startswith("ridge_fit/") for r in got["rows"] for k in r) and not any(k.startswith("ridge_fit/") for k in got["module"].logged)


def test_multi_subject_solves_one_system_per_subject(dev):
    subjects = ["sub-01", "sub-02"]
    run = _fit(epochs=2, subjects=subjects, cache_features=True, ridge_fit="closed_form", dropout_rate=0.0)
    assert len(run["fits"]) == 1
    f = run["fits"][0]
    counts = [int((f["sub"] == g).sum()) for g in range(2)]
    assert [o["n"] for o in f["out"]] == counts == [8, 8] and [o["subject"] for o in f["out"]] == subjects
    assert all(o["info"] == 0 for o in f["out"])
    assert f["logged"]["ridge_fit/n"] == 16
    W = f["masters"][WN].cpu().numpy()
    assert W.shape == (2, 128, 512)
    for g in range(2):
        rows = np.nonzero(f["sub"] == g)[0]
        sol = RE.solve(RE.sums(f["z"][rows], f["y"][rows], chunk=512), 1e-3)
        bar = RE.master_bar(sol["W"], RE.cond2(sol["A"]), 512)
        own = float(np.max(np.abs(W[g].astype(np.float64) - sol["W"].astype(np.float32).astype(np.float64)) / bar))
        # ... and from no one else's: the other subject's clips alone, or all clips together, give weights far outside the bar
        other = RE.solve(RE.sums(np.delete(f["z"], rows, 0), np.delete(f["y"], rows, 0), chunk=512), 1e-3)
        both = RE.solve(RE.sums(f["z"], f["y"], chunk=512), 1e-3)
        far = [float(np.max(np.abs(W[g].astype(np.float64) - x["W"]) / bar)) for x in (other, both)]
        print(f"subject {g}: {len(rows)} clips, max |dW| / bar {own:.3f}; against the other subject's / everyone's fit {far}")
        assert own <= 1 and min(far) > 1
    for n in f["masters"]:
        assert torch.equal(f["direct"][n], f["masters"][n])


def test_lightning_hooks_run_the_fit_once(dev, tmp_path):
    """The module's Lightning hooks (on_train_epoch_start / _end) carry the fit too: tests/fake_lightning's automatic-optimisation
    loop, with the two epoch hooks Lightning calls around it, solves once at the end of the epoch that fills the cache and leaves
    the masters of a direct call."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import fake_lightning
    root = fake_lightning.write(tmp_path / "site")
    code = r'''
import torch
import lightning.pytorch as lp
from src.litmodule import VLBLitModule, VLBLitModuleConfig
from src.datamodule import VLBDataModule, VLBDataModuleConfig

class HookTrainer(lp.Trainer):
    """fake_lightning.Trainer.fit with trainer.datamodule set and the epoch hooks of Lightning's fit loop around each epoch"""
    def fit(self, model, datamodule=None, ckpt_path=None):
        self.datamodule, self.model = datamodule, model
        model.trainer = self
        model.configure_model()
        opts, scheds = model.configure_optimizers()
        opt, sched = opts[0], scheds[0]["scheduler"]
        self.optimizers, self.lr_schedulers = [opt], [sched]
        model.on_fit_start()
        model.train()
        loader = datamodule.train_dataloader()
        for epoch in range(self.max_epochs):
            self.current_epoch = epoch
            loader.sampler.set_epoch(epoch)
            model.on_train_epoch_start()
            for batch in loader:
                batch = model.transfer_batch_to_device(batch, model.device, 0)
                def closure():
                    with torch.autocast("cuda", dtype=torch.bfloat16, enabled="bf16" in str(self.precision)):
                        loss = model.training_step(batch)
                    opt.zero_grad()
                    loss.backward()
                    model.configure_gradient_clipping(opt, self.gradient_clip_val, None)
                    return loss
                self.losses.append(float(opt.step(closure=closure)))
                sched.step()
                self.global_step += 1
            model.on_train_epoch_end()

cfg = VLBLitModuleConfig(model_path="none", freeze_backbone=True, use_lora=False, lora_r=None, lora_alpha=None, lora_dropout=None,
                         dropout_rate=0.0, num_target=128, l2_lambda=1e-3, lr=1e-3, betas=[0.9, 0.999], eps=1e-8, weight_decay=1e-2,
                         lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=50000, geometry="mini", cache_features=True,
                         ridge_fit="closed_form")
dm = VLBDataModule(VLBDataModuleConfig(lazyload_path="synthetic:3x8", subject="sub-99", seasons=["s1"], delay=3, window=3,
                                       random_state=1234, shuffle_val_data=False, batch_size=4, geometry="mini", num_target=128))
m = VLBLitModule(cfg)
assert isinstance(m, lp.LightningModule)
calls, logged = [], {}
orig = m.fit_ridge_closed_form
def spy(*a, **k):
    out = orig(*a, **k)
    torch.cuda.synchronize()
    first = {n: t.clone() for n, t in m.head.master.items()}
    logged.update({k2: v for k2, v in tr.logged_metrics.items() if k2.startswith("ridge_fit/")})
    o, cnt, _ = m.flat.offsets["ridge_layer.linear.weight"]
    assert not bool(m.flat.m[o:o + cnt].any()) and not bool(m.flat.v[o:o + cnt].any())
    orig(*a, **k)
    torch.cuda.synchronize()
    assert all(torch.equal(m.head.master[n], t) for n, t in first.items())
    calls.append((tr.current_epoch, tr.global_step, out[0]["n"], out[0]["info"]))
    return out
m.fit_ridge_closed_form = spy
tr = HookTrainer(precision="bf16-mixed", gradient_clip_val=1, max_epochs=3)
tr.fit(model=m, datamodule=dm)
assert calls == [(0, 4, 16, 0)], calls
assert tr.global_step == 12 and m.optimizer.step_count == 12
assert logged["ridge_fit/n"] == 16.0 and logged["ridge_fit/train_mse_after"] < logged["ridge_fit/train_mse_before"], logged
print("RIDGE_LIGHTNING_OK", tr.losses)
'''
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, ROOT, os.path.join(ROOT, "oracle")]), VLB_TRAINER="lightning")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0 and "RIDGE_LIGHTNING_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
