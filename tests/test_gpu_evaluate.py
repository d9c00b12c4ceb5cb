"""The evaluation pass at module level: ``Trainer.test`` / ``test_step`` / ``TargetScores`` on the mini
geometry with synthetic data, against the existing ``LogValAccuracyCallback`` fed the same ``test_step`` outputs, under
per-subject heads, target masks, EMA evaluation weights and merged LoRA adapters; reproducibility of the ``.npz``; the CLI;
and that a test pass leaves the training state alone."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LORA = dict(use_lora=True, freeze_backbone=False, lora_r=16, lora_alpha=32, lora_dropout=0.1, dropout_rate=0.1)
ARRAYS = ("r", "r2", "mse", "n", "boot_mean", "boot_se", "p", "q", "avg", "kept", "blocks")


def _cfg(**kw):
    from phantom_vlb_amd.litmodule import VLBLitModuleConfig
    base = dict(model_path="none", freeze_backbone=True, use_lora=False, lora_r=None, lora_alpha=None, lora_dropout=None,
                dropout_rate=0.0, num_target=128, l2_lambda=1e-3, lr=1e-3, betas=[0.9, 0.999], eps=1e-8,
                weight_decay=1e-2, lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=50000, geometry="mini",
                score_block=4)
    base.update(kw)
    return VLBLitModuleConfig(**base)


def _dm(test="synthetic:2x6", batch_size=4, subjects=None, path="synthetic:3x4"):
    from phantom_vlb_amd.datamodule import VLBDataModule, VLBDataModuleConfig
    return VLBDataModule(VLBDataModuleConfig(lazyload_path=path, subject="sub-01", seasons=["s1"], delay=3, window=3,
                                             random_state=1234, shuffle_val_data=False, batch_size=batch_size, geometry="mini",
                                             num_target=128, subjects=subjects, test_lazyload_path=test))


def _module(**kw):
    from phantom_vlb_amd.litmodule import VLBLitModule
    m = VLBLitModule(_cfg(**kw))
    with pytest.warns(UserWarning, match="random-initialising"):
        m.configure_model()
    return m


class _Feed:
    """Hands every ``test_step`` output to a LogValAccuracyCallback (the yardstick) and keeps losses and predictions."""

    def __init__(self):
        from phantom_vlb_amd.utils import LogValAccuracyCallback
        self.cb, self.losses, self.preds = LogValAccuracyCallback(), [], []

    def on_test_epoch_start(self, trainer, module):
        self.cb.on_validation_epoch_start(trainer, module)

    def on_test_batch_end(self, trainer, module, out, batch, bi):
        self.cb.on_validation_batch_end(trainer, module, out, batch, bi)
        self.losses.append(float(out["loss"]))
        self.preds.append(out["brain_preds"].detach().cpu().clone())

    def on_test_epoch_end(self, trainer, module):
        self.cb.on_validation_epoch_end(trainer, module)


def _test_pass(m, dm=None, **kw):
    from phantom_vlb_amd.trainer import Trainer
    feed = _Feed()
    tr = Trainer(callbacks=[feed])
    metrics = tr.test(m, dm if dm is not None else _dm(), **kw)
    assert isinstance(metrics, list) and len(metrics) == 1
    return metrics[0], feed


def _against_callback(res_r, corr, kept=None):
    corr = corr.double().cpu().numpy()
    k = np.ones_like(corr, bool) if kept is None else kept
    assert np.isfinite(res_r[k]).all() and np.abs(res_r[k] - corr[k]).max() <= 1e-6, np.abs(res_r[k] - corr[k]).max()
    assert np.isnan(res_r[~k]).all() and np.isnan(corr[~k]).all()


@pytest.mark.parametrize("kind", ["frozen", "lora"])
def test_equals_the_validation_callback(dev, kind):
    m = _module(**(LORA if kind == "lora" else {}))
    metrics, feed = _test_pass(m)
    res = m.test_scores_result
    assert res["r"].shape == (1, 128) and (res["n"] == 12).all() and res["blocks"].tolist() == [3] and int(res["block"]) == 4
    _against_callback(res["r"][0], feed.cb.correlations)
    assert abs(metrics["test_corr_avg"] - float(feed.cb.correlations.double().mean())) <= 1e-6
    assert metrics["test_corr_avg"] == float(res["avg"][0, 0]) and metrics["test_r2_avg"] == float(res["avg"][0, 1])
    assert metrics["test/brain_mse"] == float(res["avg"][0, 2])
    assert len(feed.losses) == 3 and abs(metrics["test/brain_loss"] - sum(feed.losses) / 3) <= 1e-6 * abs(sum(feed.losses) / 3)
    assert np.isnan(res["p"]).all() and int(res["bootstrap"]) == 0            # no bootstrap was asked for
    # R^2 and mse against their definitions on the stored outputs
    p = torch.cat(feed.preds).double().numpy()
    y = torch.cat([b["timeseries"] for b in _dm().test_dataloader()]).to(torch.bfloat16).double().numpy()
    sse = ((p - y) ** 2).sum(0)
    # (sse from the moments, Tpp - 2 Tpy + Tyy, against the direct sum: 4 u (Tpp + 2 |Tpy| + Tyy) / sse, far below 1e-10 here)
    assert np.allclose(res["mse"][0], sse / 12, rtol=1e-10, atol=0)
    assert np.allclose(res["r2"][0], 1 - sse / ((y - y.mean(0)) ** 2).sum(0), rtol=0, atol=1e-10)


def test_multi_subject_equals_the_callback_per_subject(dev):
    subs = ["sub-01", "sub-02", "sub-03"]
    m = _module(subjects=subs)
    dm = _dm(test="synthetic:1x3", subjects=subs[:2] + ["sub-03"])
    # the third subject has no test clips: drop its files from the split
    keep = [i for i, g in enumerate(dm.datasets.test.subject_of) if g < 2]
    from phantom_vlb_amd.datamodule import VLB_Dataset
    dm.datasets.test = VLB_Dataset([dm.datasets.test.ds_paths[i] for i in keep], "mini", 128, subject_of=[dm.datasets.test.subject_of[i] for i in keep])
    metrics, feed = _test_pass(m, dm)
    res = m.test_scores_result
    assert res["r"].shape == (3, 128) and res["blocks"].tolist() == [1, 1, 0] and list(res["subjects"]) == subs
    corr = feed.cb.correlations
    for g in range(2):
        _against_callback(res["r"][g], corr[g])
        assert abs(metrics[f"test_corr_avg/{subs[g]}"] - float(corr[g].double().mean())) <= 1e-6
        assert (res["n"][g] == 3).all()
    assert np.isnan(res["r"][2]).all() and (res["n"][2] == 0).all() and "test_corr_avg/sub-03" not in metrics
    assert abs(metrics["test_corr_avg"] - (metrics["test_corr_avg/sub-01"] + metrics["test_corr_avg/sub-02"]) / 2) <= 1e-12
    assert abs(metrics["test_corr_avg"] - float(m.logged["val_corr_avg"])) <= 1e-6      # the callback's own mean over subjects


def test_target_mask(dev, tmp_path):
    w = np.ones(128, np.float32)
    w[[0, 5, 64, 127]] = 0
    np.save(tmp_path / "w.npy", w)
    m = _module(target_weights=str(tmp_path / "w.npy"))
    metrics, feed = _test_pass(m)
    res = m.test_scores_result
    kept = w > 0
    assert np.array_equal(res["kept"][0], kept)
    _against_callback(res["r"][0], feed.cb.correlations, kept)
    assert np.isnan(res["r2"][0, ~kept]).all() and np.isnan(res["mse"][0, ~kept]).all()
    assert abs(metrics["test_corr_avg"] - res["r"][0, kept].mean()) <= 1e-12
    assert abs(metrics["test_r2_avg"] - res["r2"][0, kept].mean()) <= 1e-9 * max(1.0, abs(metrics["test_r2_avg"]))
    assert abs(metrics["test_corr_avg"] - float(m.logged["val_corr_avg"])) <= 1e-6


def _fit(m, dm, **kw):
    from phantom_vlb_amd.trainer import Trainer
    tr = Trainer(max_epochs=1, val_check_interval=1.0, log_every_n_steps=1, **kw)
    tr.fit(m, dm)
    return tr


def test_ema_evaluation_weights(dev):
    """with ema_decay and ema_eval the scores are those of a module loaded with the averaged weights"""
    from phantom_vlb_amd.backbone import Weights
    from phantom_vlb_amd.litmodule import VLBLitModule, resolve_geometry
    kw = dict(LORA, ema_decay=0.9, ema_warmup=False)
    base = Weights.random_state_dict(resolve_geometry(_cfg(**kw)), dev, seed=1234)
    m = VLBLitModule(_cfg(**kw))
    m.configure_model(state_dict=dict(base))
    tr = _fit(m, _dm(batch_size=2))
    before = m.flat.compute.clone()
    metrics = tr.test(m, _dm())[0]
    assert torch.equal(m.flat.compute, before) and not m.__dict__.get("_ema_swapped", False)       # the last iterate is back
    avg = VLBLitModule(_cfg(**LORA))
    avg.configure_model(state_dict={**base, **m.trainable_state_dict(averaged=True)})
    want, _ = _test_pass(avg)
    raw = VLBLitModule(_cfg(**LORA))
    raw.configure_model(state_dict={**base, **m.trainable_state_dict()})
    last, _ = _test_pass(raw)
    for k in ("r", "r2", "mse"):
        assert np.array_equal(m.test_scores_result[k], avg.test_scores_result[k]), k
    assert metrics["test/brain_loss"] == want["test/brain_loss"] != last["test/brain_loss"]
    assert not np.array_equal(m.test_scores_result["r"], raw.test_scores_result["r"])


def test_merged_lora_path(dev):
    """merge_lora_for_eval: the test pass runs the merged decoder, as validation does"""
    m = _module(**dict(LORA, merge_lora_for_eval=True))
    calls, orig = [], m._merged_forward
    m._merged_forward = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    dm = _dm()
    metrics, feed = _test_pass(m, dm)
    assert len(calls) == 3
    want = torch.cat([m.validation_step(b)["brain_preds"].cpu() for b in dm.test_dataloader()])
    assert len(calls) == 6 and torch.equal(torch.cat(feed.preds), want)


def _arrays_equal(a, b):
    for k in ARRAYS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), k


def test_reproducible_bootstrap_and_predictions(dev, tmp_path):
    outs = []
    for i in range(2):
        m = _module(score_bootstrap=32, score_bootstrap_seed=5, score_save_predictions=True)
        metrics, feed = _test_pass(m)
        outs.append((m.test_scores.write(str(tmp_path / f"s{i}.npz")), m.test_scores_result, feed))
    a, b = np.load(outs[0][0]), np.load(outs[1][0])
    _arrays_equal(a, b)                                              # two runs: bit-identical files
    _arrays_equal(a, outs[0][1])                                     # and the file round-trips the result
    res = outs[0][1]
    assert res["blocks"].tolist() == [3] and int(res["bootstrap"]) == 32 and int(res["seed"]) == 5
    assert np.isfinite(res["boot_se"]).all() and (res["boot_se"] > 0).all() and np.isfinite(res["boot_mean"]).all()
    assert ((res["p"] >= 1 / 33) & (res["p"] <= 1)).all() and ((res["q"] >= res["p"]) & (res["q"] <= 1)).all()
    assert a["pred"].dtype == np.float32 and np.array_equal(a["pred"], torch.cat(outs[0][2].preds).numpy())
    assert a["index"].tolist() == list(range(12)) and a["subject"].tolist() == [0] * 12
    # one block only: the bootstrap has nothing to resample and says so
    one = _module(score_bootstrap=8, score_block=16)
    with pytest.warns(UserWarning, match="nothing to resample"):
        _test_pass(one)
    assert (one.test_scores_result["boot_se"] == 0).all()


def test_cli_reproduces_the_in_process_scores(dev, tmp_path):
    sys.path.insert(0, ROOT)
    import train
    from phantom_vlb_amd.config import instantiate, load_config
    ov = ["experiment=VLB_mini_synthetic", "subject=sub-98", f"output_dir={tmp_path}", "trainer.max_epochs=1",
          "litmodule.config.score_block=4", "litmodule.config.score_bootstrap=16"]
    cfg = load_config(os.path.join(ROOT, "config"), ov + ["evaluate=test"])
    assert train.check_evaluate_keys(cfg) == ("test", True, None)
    trainer = instantiate(cfg["trainer"], logger=[], callbacks=[])
    dm, m = instantiate(cfg["datamodule"]), instantiate(cfg["litmodule"])
    trainer.fit(model=m, datamodule=dm)
    ckpt = trainer.save_checkpoint(str(tmp_path))
    here = train.evaluate(trainer, m, dm, "test", str(tmp_path / "here.npz"))
    there = tmp_path / "there.npz"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), *ov, "evaluate=test", "fit=false", f"ckpt_path={ckpt}",
                        f"evaluate_out={there}"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    a, b = np.load(here), np.load(there)
    _arrays_equal(a, b)
    assert np.isfinite(b["r"]).all() and (b["n"] == 16).all() and b["blocks"].tolist() == [4] and np.isfinite(b["boot_se"]).all()
    # evaluate=val goes through the same TargetScores
    val = train.evaluate(trainer, m, dm, "val", str(tmp_path / "val.npz"))
    v = np.load(val)
    assert v["r"].shape == (1, 128) and (v["n"] == len(dm.datasets.val)).all() and not np.array_equal(v["r"], a["r"])


def test_a_test_pass_leaves_the_training_state_alone(dev):
    mods = []
    for with_test in (False, True):
        m = _module(**LORA)
        tr = _fit(m, _dm(batch_size=2))
        if with_test:
            tr.test(m, _dm())
        torch.cuda.synchronize()
        mods.append(m)
    a, b = mods
    for key in ("master", "m", "v", "compute"):
        assert torch.equal(getattr(a.flat, key), getattr(b.flat, key)), key
    assert a.rng_state() == b.rng_state() and a.optimizer.step_count == b.optimizer.step_count
    assert a.training == b.training
