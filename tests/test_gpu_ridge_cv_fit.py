"""``ridge_lambda_grid`` through the module and the built-in runner (VLB_mini_synthetic and its multi-subject variant, mini
geometry, synthetic clips): when the fit runs, that the chosen ``l2_lambda`` is the emulator's on the module's
own features, that it is what the head, the log and ``ridge_fit_result`` carry and what the next step's penalty uses, that the
masters are those of a direct fit with that value, and that a checkpoint restores it.

Bars: the scores against tests/ridge_cv_emul.py (each side solves for its own X: the end-to-end route, ``dx_bar`` included);
the chosen index only after the emulator's best score leads its runner-up by 100 score bars; the masters within
``ridge_emul.master_bar`` (one fp32 ulp + E cond_2 2^-53 max|W|: the fp32 roundings of two fp64 solutions of one system) of a
direct ``fit_ridge_closed_form(l2_lambda=best)``, whose sums are accumulated without folds; the l2 term of the next step
against best * sum(W_bf16^2) in fp64 to (V E + 4) 2^-24 relative (an fp32 sum of V E exact squares in any order, the
product with lambda, lambda's own fp32 rounding)."""
import numpy as np
import pytest
import torch

import ridge_cv_emul as CE
import ridge_emul as RE
import test_gpu_ridge_fit as RF

pytestmark = pytest.mark.gpu
WN, BN = RF.WN, RF.BN
GRID = [1e-4, 1e-2, 1.0]


def _fit(epochs=2, subjects=None, **kw):
    """The built-in runner on the YAML's loop; every closed-form fit and every training step is recorded."""
    from phantom_vlb_amd.litmodule import VLBLitModule
    from phantom_vlb_amd.trainer import Trainer
    m = VLBLitModule(RF._cfg(subjects=subjects, cache_features=True, ridge_fit="closed_form", dropout_rate=0.0, **kw))
    m.configure_model()
    dm = RF._dm(subjects)
    fits, steps = [], []
    orig, ts = m.fit_ridge_closed_form, m.training_step

    def fit_spy(*a, **k):
        z, y, sub = RF._split_features(m, dm.datasets.train)
        lam_before = m.head.l2_lambda
        out = orig(*a, **k)
        torch.cuda.synchronize()
        rec = dict(epoch=getattr(tr, "current_epoch", None), global_step=tr.global_step, steps_before=len(steps), out=out, z=z, y=y,
                   sub=sub, lam_before=lam_before, lam_after=m.head.l2_lambda, result=m.ridge_fit_result,
                   masters={n: t.clone() for n, t in m.head.master.items()},
                   logged={k2: v for k2, v in m.logged.items() if k2.startswith("ridge_fit/")})
        orig(*a, l2_lambda=m.head.l2_lambda, **k)          # a direct fit with the chosen value: no grid, no folds
        torch.cuda.synchronize()
        rec["direct"] = {n: t.clone() for n, t in m.head.master.items()}
        rec["direct_result"] = m.ridge_fit_result
        for n, t in rec["masters"].items():                # training goes on from the cross-validated fit's own masters
            m.head.master[n].copy_(t)
            m.head.compute[n].copy_(t)
        m.ridge_fit_result = rec["result"]
        fits.append(rec)
        return out

    def step_spy(batch):
        rec = dict(W=m.head.compute[WN].float().cpu().double(), lam=m.head.l2_lambda)
        loss = ts(batch)
        rec["terms"] = m.head.loss_terms.double().cpu()
        steps.append(rec)
        return loss
    m.fit_ridge_closed_form, m.training_step = fit_spy, step_spy
    rec = RF._Rec()
    tr = Trainer(max_epochs=epochs, val_check_interval=0.5, log_every_n_steps=1, logger=rec)
    tr.fit(m, dm)
    torch.cuda.synchronize()
    return dict(module=m, dm=dm, fits=fits, steps=steps, rows=rec.rows)


@pytest.mark.parametrize("subjects,folds,block", [(None, 2, 2), (None, 4, 2), (["sub-01", "sub-02"], 2, 2)])
def test_the_fit_chooses_the_emulators_lambda_and_everything_after_uses_it(dev, subjects, folds, block):
    run = _fit(epochs=2, subjects=subjects, ridge_lambda_grid=GRID, ridge_cv_folds=folds, ridge_cv_block=block, l2_lambda=3e-3)
    m = run["module"]
    # ---- once, at the moment the fit without a grid runs: after epoch 1's four steps, before epoch 2's first
    assert len(run["fits"]) == 1
    f = run["fits"][0]
    assert (f["epoch"], f["global_step"], f["steps_before"]) == (0, 4, 4)
    assert f["lam_before"] == 3e-3                          # the configured value holds until the fit; it is not in the grid
    cv = f["result"]
    H = 1 if subjects is None else len(subjects)
    # ---- the emulator on the module's own features
    emu = CE.cv(f["z"], f["y"], GRID, folds, block, chunk=512, sub=f["sub"], bars=True)
    assert emu["valid"].all(), "a target outside the first-order formula's validity: choose other inputs"
    serr = np.abs(np.array(cv["score"]) - emu["score"])
    order = np.argsort(emu["score"])[::-1]
    margin, sbar = float(emu["score"][order[0]] - emu["score"][order[1]]), float(emu["score_bar"].max())
    print(f"subjects={subjects} K={folds}: scores {cv['score']} vs emulator {emu['score'].tolist()}: err / bar "
          f"{np.max(serr / emu['score_bar']):.3e}; margin {margin:.2e} = {margin / sbar:.0f} score bars")
    assert np.all(serr <= emu["score_bar"])
    assert np.all(np.abs(np.array(cv["score_per_head"]) - emu["score_per_head"]) <= emu["score_bar"].max())
    assert margin >= 100 * sbar, "the inputs do not separate the best two grid points: choose another grid"
    best = GRID[emu["best_index"]]
    # ---- head, log, result and the solve agree with each other and with the emulator
    assert cv["best_index"] == emu["best_index"] and cv["best_lambda"] == best and cv["grid"] == GRID
    assert f["lam_after"] == best and m.head.l2_lambda == best
    assert [o["l2_lambda"] for o in f["out"]] == [best] * H and all(o["info"] == 0 for o in f["out"]) and cv["solve"] == f["out"]
    lg = f["logged"]
    assert lg["ridge_fit/l2_lambda"] == best and lg["ridge_fit/cv_best_index"] == emu["best_index"]
    assert lg["ridge_fit/cv_score"] == cv["score"][cv["best_index"]]
    assert [lg[f"ridge_fit/cv_score_{i}"] for i in range(len(GRID))] == cv["score"]
    assert tuple(cv["r"].shape) == (H, len(GRID), 128) and cv["infos"] == [[[0] * len(GRID)] * folds] * H
    # ---- the masters are those of a direct fit with that value (no grid: the fold-free sums)
    assert isinstance(f["direct_result"], list) and [o["l2_lambda"] for o in f["direct_result"]] == [best] * H
    E = f["z"].shape[1]
    Wc, Wd = (f[k][WN].cpu().numpy().astype(np.float64).reshape(H, 128, E) for k in ("masters", "direct"))
    for g in range(H):
        rows = np.arange(len(f["z"])) if f["sub"] is None else np.nonzero(f["sub"] == g)[0]
        sol = RE.solve(RE.sums(f["z"][rows], f["y"][rows], chunk=512), best)
        bar = RE.master_bar(sol["W"], RE.cond2(sol["A"]), E)
        print(f"  head {g}: max |W_cv - W_direct| / master_bar {np.max(np.abs(Wc[g] - Wd[g]) / bar):.3f}, "
              f"|W_cv - emulator| / bar {np.max(np.abs(Wc[g] - sol['W'].astype(np.float32).astype(np.float64)) / bar):.3f}")
        assert np.all(np.abs(Wc[g] - Wd[g]) <= bar)
        assert np.all(np.abs(Wc[g] - sol["W"].astype(np.float32).astype(np.float64)) <= bar)
    # ---- the next step's penalty is the chosen lambda's
    s = run["steps"][f["steps_before"]]
    want = best * float((s["W"] ** 2).sum())
    got = float(s["terms"][1])
    assert s["lam"] == best and abs(got - want) <= (s["W"].numel() + 4) * 2.0 ** -24 * want, (got, want)
    assert abs(got - want) < 0.1 * min(abs(got - want * x / best) for x in GRID + [3e-3] if x != best)
    # ---- a checkpoint carries the choice into a fresh module
    from phantom_vlb_amd.litmodule import VLBLitModule
    ck = {}
    m.on_save_checkpoint(ck)
    assert ck["vlb_ridge_l2_lambda"] == best
    m2 = VLBLitModule(RF._cfg(subjects=subjects, cache_features=True, ridge_fit="closed_form", ridge_lambda_grid=GRID, l2_lambda=3e-3))
    m2.on_load_checkpoint({k: v for k, v in ck.items() if k == "vlb_ridge_l2_lambda"})     # before the head exists ...
    m2.configure_model()
    assert m2.head.l2_lambda == best
    m2.head.l2_lambda = 3e-3
    m2.on_load_checkpoint(ck)                                                                # ... and after
    assert m2.head.l2_lambda == best


def test_integer_valued_sums_make_the_direct_fit_bit_identical(dev):
    """Folds' totals against the fold-free sums on integer features and targets: the same fp64 numbers, so ``ridge_solve`` with
    folds writes the masters of the fold-free path bit for bit."""
    from test_gpu_ridge_cv import _feed, _make
    head, cache, _, y, subject, K, block = _make("subjects", dev)
    gen = torch.Generator().manual_seed(3)
    yi = torch.randint(-4, 5, tuple(y.shape), generator=gen).float().to(dev)
    zi = torch.randint(-3, 4, (y.shape[0], head.E), generator=gen).to(torch.bfloat16).to(dev)
    head.features_cached = lambda cache_, ids: zi.index_select(0, torch.as_tensor(ids).to(dev)).contiguous()
    _feed(head, cache, yi, subject, K, block, chunk=37)
    head.ridge_solve(1e-2)
    with_folds = {n: head.master[n].clone() for n in (WN, BN)}
    totals = {n: torch.stack([head._ridge[n][g].sum(0) for g in range(3)]) for n in ("G", "C", "sz", "sy")}
    head.ridge_stats_end()
    head.ridge_stats_begin()
    for lo, hi in RE.chunks_of(y.shape[0], 64):
        head.ridge_stats_add(cache, torch.arange(lo, hi), yi[lo:hi], subject[lo:hi])
    assert all(torch.equal(head._ridge[n], totals[n]) for n in totals)
    head.ridge_solve(1e-2)
    torch.cuda.synchronize()
    assert all(torch.equal(head.master[n], t) for n, t in with_folds.items())
    head.ridge_stats_end()


def test_lightning_hooks_make_the_same_choice(dev, tmp_path):
    """The module's Lightning hooks carry the cross-validated fit too: tests/fake_lightning's automatic-optimisation loop with
    the two epoch hooks around each epoch fits once, at the end of the epoch that fills the cache, logs the new keys and
    chooses what the built-in runner chooses on the same clips."""
    import os
    import subprocess
    import sys
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
                         dropout_rate=0.0, num_target=128, l2_lambda=3e-3, lr=1e-3, betas=[0.9, 0.999], eps=1e-8, weight_decay=1e-2,
                         lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=50000, geometry="mini", cache_features=True,
                         ridge_fit="closed_form", ridge_lambda_grid=[1e-4, 1e-2, 1.0], ridge_cv_folds=2, ridge_cv_block=2)
dm = VLBDataModule(VLBDataModuleConfig(lazyload_path="synthetic:3x8", subject="sub-99", seasons=["s1"], delay=3, window=3,
                                       random_state=1234, shuffle_val_data=False, batch_size=4, geometry="mini", num_target=128))
m = VLBLitModule(cfg)
assert isinstance(m, lp.LightningModule)
calls, logged = [], {}
orig = m.fit_ridge_closed_form
def spy(*a, **k):
    out = orig(*a, **k)
    torch.cuda.synchronize()
    logged.update({k2: v for k2, v in tr.logged_metrics.items() if k2.startswith("ridge_fit/")})
    calls.append((tr.current_epoch, tr.global_step, out[0]["n"], out[0]["info"]))
    return out
m.fit_ridge_closed_form = spy
tr = HookTrainer(precision="bf16-mixed", gradient_clip_val=1, max_epochs=2)
tr.fit(model=m, datamodule=dm)
assert calls == [(0, 4, 16, 0)], calls
cv = m.ridge_fit_result
assert m.head.l2_lambda == cv["best_lambda"] == float(logged["ridge_fit/l2_lambda"]) and cv["best_lambda"] in cfg.ridge_lambda_grid
assert int(logged["ridge_fit/cv_best_index"]) == cv["best_index"] and float(logged["ridge_fit/cv_score"]) == cv["score"][cv["best_index"]]
assert all(float(logged["ridge_fit/cv_score_%d" % i]) == s for i, s in enumerate(cv["score"]))
ck = {}
m.on_save_checkpoint(ck)
assert ck["vlb_ridge_l2_lambda"] == cv["best_lambda"]
print("CV_LIGHTNING_OK", cv["best_index"], repr(cv["score"]))
'''
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, RF.ROOT, os.path.join(RF.ROOT, "oracle")]), VLB_TRAINER="lightning")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=RF.ROOT)
    assert r.returncode == 0 and "CV_LIGHTNING_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("CV_LIGHTNING_OK")][0]
    run = _fit(epochs=1, ridge_lambda_grid=GRID, ridge_cv_folds=2, ridge_cv_block=2, l2_lambda=3e-3)
    cv = run["fits"][0]["result"]
    # both runners fill the cache from the same clips; the LN parameters have taken four different AdamW paths (autocast,
    # clipping through Lightning), so only the choice - separated by a wide margin in the emulator - is compared
    assert int(line.split()[1]) == cv["best_index"]


def test_the_built_in_runner_sends_the_choice_to_its_loggers_and_its_checkpoints(dev, tmp_path):
    from phantom_vlb_amd.litmodule import VLBLitModule
    from phantom_vlb_amd.trainer import load_trainable_checkpoint, trainable_state
    run = _fit(epochs=2, ridge_lambda_grid=GRID, ridge_cv_folds=2, ridge_cv_block=2, l2_lambda=3e-3)
    m, cv = run["module"], run["fits"][0]["result"]
    rows = [r for r in run["rows"] if any(k.startswith("ridge_fit/") for k in r)]
    assert len(rows) == 1, rows                            # once, right after the fit
    assert rows[0]["ridge_fit/l2_lambda"] == cv["best_lambda"] and rows[0]["ridge_fit/cv_best_index"] == cv["best_index"]
    assert [rows[0][f"ridge_fit/cv_score_{i}"] for i in range(len(GRID))] == cv["score"]
    st = trainable_state(m, 8)
    assert st["ridge_l2_lambda"] == cv["best_lambda"]
    path = str(tmp_path / "last.ckpt")
    torch.save(st, path)
    m2 = VLBLitModule(RF._cfg(cache_features=True, ridge_fit="closed_form", ridge_lambda_grid=GRID, l2_lambda=3e-3))
    m2.configure_model()
    m2.configure_optimizers()
    assert m2.head.l2_lambda == 3e-3
    assert load_trainable_checkpoint(m2, path) == 8
    assert m2.head.l2_lambda == cv["best_lambda"]
    # without the grid neither the rows nor the checkpoint know about it
    plain = _fit(epochs=2)
    assert not any(k.startswith("ridge_fit/") for r in plain["rows"] for k in r)
    assert "ridge_l2_lambda" not in trainable_state(plain["module"], 8)
