"""litmodule.config.ema_decay through the optimiser, the module and the built-in runner, mini geometry.

The expected average is always tests/ema_emul.py's float32 restatement fed with the masters recorded after each optimiser
step; everything else is compared with torch.equal against a twin module without the average, or against a fresh module
loaded from ``trainable_state_dict(averaged=True)``."""
import os

import numpy as np
import pytest
import torch

import ema_emul as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
LORA = dict(use_lora=True, freeze_backbone=False, lora_r=16, lora_alpha=32, lora_dropout=0.1, dropout_rate=0.1)
RIDGE = ("ridge_layer.linear.weight", "ridge_layer.linear.bias")


def _cfg(**kw):
    from phantom_vlb_amd.litmodule import VLBLitModuleConfig
    base = dict(model_path="none", freeze_backbone=True, use_lora=False, lora_r=None, lora_alpha=None, lora_dropout=None,
                dropout_rate=0.0, num_target=128, l2_lambda=1e-3, lr=1e-3, betas=[0.9, 0.999], eps=1e-8,
                weight_decay=1e-2, lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=10, geometry="mini")
    base.update(kw)
    return VLBLitModuleConfig(**base)


_SHARED = {}


def _params_and_batches(n_micro=4, clips=2, seed=3):
    """LoRA initial weights and micro-batches, computed once and shared (never modified: configure_model copies)."""
    if "p" not in _SHARED:
        import vlb_oracle as O
        g = O.geometry_mini(lora_r=16, lora_alpha=32)
        _SHARED["p"] = O.round_bf16(O.init_params(g, seed=seed, lora=True, lora_b_std=0.02))
        whole = O.synthetic_batch(g, clips * n_micro, seed=seed + 1)
        _SHARED["micro"] = [{k: v[i * clips:(i + 1) * clips] for k, v in whole.items()} for i in range(n_micro)]
    return _SHARED["p"], _SHARED["micro"]


def _build(state_dict=None, k=None, **kw):
    from phantom_vlb_amd.litmodule import VLBLitModule
    p, _ = _params_and_batches()
    m = VLBLitModule(_cfg(**kw))
    m.configure_model(state_dict=p if state_dict is None else state_dict)
    opt, sch = m.configure_optimizers()
    if k is not None:
        m.accumulate_grad_batches = k
    return m, opt[0], sch[0]["scheduler"]


def _steps(m, opt, sch, batches, record=None):
    for b in batches:
        m.training_step(b)
        opt.step()
        sch.step()
        if record is not None:
            torch.cuda.synchronize()
            record.append(m.flat.master.cpu().numpy().copy())


def _emulate(start, masters, decays):
    ema = np.asarray(start, dtype=np.float32).copy()
    for p, d in zip(masters, decays):
        ema = E.ema_step(ema, p, d)
    return ema


def _same_state(a, b):
    for key in ("master", "m", "v", "compute"):
        assert torch.equal(getattr(a.flat, key), getattr(b.flat, key)), key


def _derived(m):
    """LoRA's derived layouts (A^T padded, block-diagonal padded B) of every layer and group, cloned."""
    return [blk[k].clone() for lay in m.lora.layers for blk in lay.values() for k in ("At", "Bpad")]


def _trained_pair(steps=3):
    """An EMA module and its twin without the average after the same ``steps`` steps (dropout on)."""
    _, micro = _params_and_batches()
    a, aopt, asch = _build(**dict(LORA, ema_decay=0.9, ema_warmup=False))
    b, bopt, bsch = _build(**LORA)
    _steps(a, aopt, asch, micro[:steps])
    _steps(b, bopt, bsch, micro[:steps])
    return (a, aopt, asch), (b, bopt, bsch)


# ------------------------------------------------------------------------------------------------ optimiser
def test_ema_does_not_perturb_training_and_equals_the_emulation(dev):
    _, micro = _params_and_batches()
    a, aopt, asch = _build(**dict(LORA, ema_decay=0.9, ema_warmup=False))
    b, bopt, bsch = _build(**LORA)
    assert aopt.ema is not None and aopt.ema.dtype == torch.float32 and aopt.ema.numel() == a.flat.numel
    assert aopt.ema.data_ptr() != a.flat.master.data_ptr() and torch.equal(aopt.ema, a.flat.master) and aopt.ema_updates == 0
    start = aopt.ema.cpu().numpy().copy()
    rec = []
    _steps(a, aopt, asch, micro[:4], rec)
    _steps(b, bopt, bsch, micro[:4])
    torch.cuda.synchronize()
    _same_state(a, b)
    assert aopt.ema_updates == aopt.step_count == 4 and aopt.ema_last_decay == 0.9
    want = _emulate(start, rec, [0.9] * 4)
    got = aopt.ema.cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())
    assert not np.array_equal(got, rec[-1])                      # an average, not a copy of the last iterate


def test_off_means_off(dev, tmp_path):
    from phantom_vlb_amd.trainer import TrainableCheckpoint, Trainer, trainable_state
    _, micro = _params_and_batches()
    m, opt, sch = _build(**LORA)
    assert opt.ema is None and opt.ema_updates == 0
    _steps(m, opt, sch, micro[:1])
    before = m.flat.compute.clone()
    with m.averaged_weights():                                   # a no-op
        assert torch.equal(m.flat.compute, before)
    tr = Trainer(max_epochs=1, limit_val_batches=1)
    tr.validate(m, [micro[0]])
    assert "_ema_stash" not in m.__dict__ and "ema/decay" not in m.logged
    st = trainable_state(m, 1)
    assert "ema" not in st and "ema_updates" not in st
    assert "ema" not in opt.state_dict()["vlb"]
    with pytest.raises(ValueError, match="ema_decay"):
        m.trainable_state_dict(averaged=True)
    TrainableCheckpoint(str(tmp_path)).save(m, str(tmp_path / "off.ckpt"), 1)
    assert "ema" not in torch.load(tmp_path / "off.ckpt", map_location="cpu", weights_only=False)


def test_warm_up_and_accumulation(dev):
    from phantom_vlb_amd.optim import ema_decay_at
    _, micro = _params_and_batches()
    m, opt, sch = _build(k=2, **dict(LORA, ema_decay=0.999))
    start = opt.ema.cpu().numpy().copy()
    rec, used = [], []
    for i, b in enumerate(micro[:4]):
        m.training_step(b)
        if i % 2 == 1:
            opt.step()
            sch.step()
            torch.cuda.synchronize()
            rec.append(m.flat.master.cpu().numpy().copy())
            used.append(opt.ema_last_decay)
        else:
            assert opt.ema_updates == i // 2                     # nothing moves inside a window
    assert opt.ema_updates == opt.step_count == 2
    assert used == [ema_decay_at(1, 0.999, True), ema_decay_at(2, 0.999, True)] == [2 / 11, 3 / 12]
    assert np.array_equal(opt.ema.cpu().numpy(), _emulate(start, rec, used))


class _Counting:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a):
        self.calls += 1
        return self.fn(*a)


def _count_adamw_calls(monkeypatch):
    from phantom_vlb_amd import optim
    counters = {}
    for name in ("vlb_adamw_step", "vlb_adamw_step_groups", "vlb_adamw_step_ema", "vlb_adamw_step_groups_ema", "vlb_adamw_step_g16",
                 "vlb_adamw_step_groups_g16"):
        counters[name] = _Counting(getattr(optim.lib, name))
        monkeypatch.setattr(optim.lib, name, counters[name])
    return counters


def test_entry_point_per_configuration_and_groups(dev, monkeypatch):
    """Which of the four fp32 entry points a step launches: exactly one, chosen by (groups, ema_decay); with two groups and
    the average, masters / moments / copies equal the grouped run without it and the average equals the emulation."""
    _, micro = _params_and_batches()
    counters = _count_adamw_calls(monkeypatch)
    groups = [{"params": ["*.lora_B.weight"], "lr_scale": 4}]
    runs = {}
    for label, kw, entry in (("plain", {}, "vlb_adamw_step"), ("ema", dict(ema_decay=0.9), "vlb_adamw_step_ema"),
                             ("groups", dict(optimizer_groups=groups), "vlb_adamw_step_groups"),
                             ("groups_ema", dict(optimizer_groups=groups, ema_decay=0.9), "vlb_adamw_step_groups_ema")):
        for c in counters.values():
            c.calls = 0
        m, opt, sch = _build(**dict(LORA, **kw))
        start = None if opt.ema is None else opt.ema.cpu().numpy().copy()
        rec = []
        _steps(m, opt, sch, micro[:3], rec)
        assert {n: c.calls for n, c in counters.items() if c.calls} == {entry: 3}, label
        runs[label] = (m, opt, start, rec)
    assert len(runs["groups_ema"][1].param_groups) == 2 and runs["groups_ema"][1].tables is not None
    _same_state(runs["groups"][0], runs["groups_ema"][0])
    _same_state(runs["plain"][0], runs["ema"][0])
    assert not torch.equal(runs["plain"][0].flat.master, runs["groups"][0].flat.master)
    from phantom_vlb_amd.optim import ema_decay_at
    for label in ("ema", "groups_ema"):
        m, opt, start, rec = runs[label]
        want = _emulate(start, rec, [ema_decay_at(t, 0.9, True) for t in (1, 2, 3)])
        assert np.array_equal(opt.ema.cpu().numpy(), want), label


def test_data_parallelism_is_refused(dev):
    from phantom_vlb_amd.parallel import attach_data_parallel
    m, opt, _ = _build(**dict(LORA, ema_decay=0.9))
    with pytest.raises(ValueError, match=r"ema_decay under data parallelism \(WORLD_SIZE > 1\) is not supported"):
        attach_data_parallel(m, opt)
    assert opt.shardeds == [None]
    n, o, _ = _build(**LORA)
    attach_data_parallel(n, o)                                   # without the average: attached as ever
    assert o.shardeds[0] is not None


# ------------------------------------------------------------------------------------------------ evaluating on the average
def test_swap_and_stash(dev):
    from phantom_vlb_amd.litmodule import VLBLitModule
    p, micro = _params_and_batches()
    (a, aopt, asch), (b, bopt, bsch) = _trained_pair(3)
    batch = micro[3]
    raw = a.validation_step(batch)["brain_preds"].clone()
    assert torch.equal(raw, b.validation_step(batch)["brain_preds"])
    before_c, before_d, version = a.flat.compute.clone(), _derived(a), a.lora.version
    ema_before = aopt.ema.clone()
    with a.averaged_weights():
        assert torch.equal(a.flat.compute, aopt.ema.to(BF))      # everywhere, padding included
        assert a.lora.version > version
        inside = a.validation_step(batch)["brain_preds"].clone()
        with a.averaged_weights():                               # entered again inside itself: nothing happens
            assert torch.equal(a.flat.compute, aopt.ema.to(BF))
        assert torch.equal(a.flat.compute, aopt.ema.to(BF))
    assert a.__dict__["_ema_stash"].dtype == BF and a.__dict__["_ema_stash"].numel() == a.flat.numel
    sd = a.trainable_state_dict(averaged=True)
    raw_sd = a.trainable_state_dict()
    assert set(sd) == set(raw_sd) and all(sd[n].shape == raw_sd[n].shape for n in sd)
    g = a.geometry
    assert sd["model.layers.1.mlp.down_proj.lora_B.weight"].shape == (g.dim, 16)
    assert not torch.equal(sd["ridge_layer.linear.weight"], raw_sd["ridge_layer.linear.weight"])
    fresh = VLBLitModule(_cfg(**LORA))
    fresh.configure_model(state_dict={**p, **sd})
    assert torch.equal(inside, fresh.validation_step(batch)["brain_preds"])
    assert not torch.equal(inside, raw)

    def check_restored():
        assert torch.equal(a.flat.compute, before_c)
        assert all(torch.equal(x, y) for x, y in zip(_derived(a), before_d))
        assert torch.equal(aopt.ema, ema_before)
        assert torch.equal(a.validation_step(batch)["brain_preds"], raw)
    check_restored()
    with pytest.raises(RuntimeError, match="inside the context"):
        with a.averaged_weights():
            assert not torch.equal(a.flat.compute, before_c)
            raise RuntimeError("inside the context")
    check_restored()
    _same_state(a, b)
    _steps(a, aopt, asch, [batch])
    _steps(b, bopt, bsch, [batch])
    torch.cuda.synchronize()
    _same_state(a, b)                                            # the next training step matches the twin's bit for bit


def test_validation_epoch_hooks_swap_and_restore(dev):
    """The hooks a Lightning trainer calls around a validation epoch: the average inside, the last iterate back (and
    ``ema/decay`` logged) at its end; with ``ema_eval=False`` they leave the weights alone."""
    _, micro = _params_and_batches()
    for ema_eval in (True, False):
        m, opt, sch = _build(**dict(LORA, ema_decay=0.9, ema_warmup=False, ema_eval=ema_eval))
        _steps(m, opt, sch, micro[:2])
        before = m.flat.compute.clone()
        m.on_validation_epoch_start()
        assert torch.equal(m.flat.compute, opt.ema.to(BF) if ema_eval else before)
        assert torch.equal(m.flat.compute, before) != ema_eval
        m.on_validation_epoch_end()
        assert torch.equal(m.flat.compute, before) and m.logged["ema/decay"] == 0.9
        assert not m.__dict__.get("_ema_swapped", False)
        m.on_validation_epoch_end()                              # a second call finds nothing to leave
        assert torch.equal(m.flat.compute, before)


def test_merged_weights_are_those_of_the_averaged_adapters(dev):
    from phantom_vlb_amd.litmodule import VLBLitModule
    p, micro = _params_and_batches()
    kw = dict(LORA, merge_lora_for_eval=True)
    a, aopt, asch = _build(**dict(kw, ema_decay=0.9, ema_warmup=False))
    _steps(a, aopt, asch, micro[:3])
    keys = [k for k in a.lora.merge()[0] if k.startswith("w")]

    def merged(m):
        return [lw[k].clone() for lw in m._merged_layers() for k in keys]

    def loaded(sd):
        f = VLBLitModule(_cfg(**kw))
        f.configure_model(state_dict={**p, **sd})
        return f
    raw = merged(a)
    want_raw = merged(loaded(a.trainable_state_dict()))
    want_avg = merged(loaded(a.trainable_state_dict(averaged=True)))
    assert all(torch.equal(x, y) for x, y in zip(raw, want_raw))
    with a.averaged_weights():
        inside = merged(a)
        pred_in = a.validation_step(micro[3])["brain_preds"].clone()          # eval mode: the merged decoder
    assert all(torch.equal(x, y) for x, y in zip(inside, want_avg))
    assert any(not torch.equal(x, y) for x, y in zip(inside, raw))
    assert all(torch.equal(x, y) for x, y in zip(merged(a), raw))           # outside: the raw adapters again
    assert not torch.equal(pred_in, a.validation_step(micro[3])["brain_preds"])
    # merged_state_dict (ema_eval defaults to true) exports the averaged adapters and head, and leaves the raw ones in force
    msd = a.merged_state_dict()
    avg_sd = a.trainable_state_dict(averaged=True)
    assert torch.equal(msd["ridge_layer.linear.weight"], avg_sd["ridge_layer.linear.weight"])
    fm = loaded(avg_sd).merged_state_dict()
    assert all(torch.equal(msd[k], fm[k]) for k in msd if k.startswith("model.layers."))
    assert all(torch.equal(x, y) for x, y in zip(merged(a), raw))


# ------------------------------------------------------------------------------------------------ checkpoints
def test_resume(dev, tmp_path):
    from phantom_vlb_amd.trainer import TrainableCheckpoint, load_trainable_checkpoint
    _, micro = _params_and_batches()
    kw = dict(LORA, ema_decay=0.999)
    a, aopt, asch = _build(**kw)
    _steps(a, aopt, asch, micro[:4])
    b, bopt, bsch = _build(**kw)
    _steps(b, bopt, bsch, micro[:3])
    path = str(tmp_path / "three.ckpt")
    TrainableCheckpoint(str(tmp_path)).save(b, path, 3)
    st = torch.load(path, map_location="cpu", weights_only=False)
    assert st["ema_updates"] == 3 and st["ema"].dtype == torch.float32 and torch.equal(st["ema"], bopt.ema.cpu())
    c, copt, csch = _build(**kw)
    assert load_trainable_checkpoint(c, path) == 3
    assert copt.ema_updates == 3 and torch.equal(copt.ema, bopt.ema)
    _steps(c, copt, csch, micro[3:4])
    torch.cuda.synchronize()
    _same_state(a, c)
    assert torch.equal(aopt.ema, copt.ema) and copt.ema_updates == aopt.ema_updates == 4
    # VlbAdamW.state_dict() / load_state_dict() carry the same two entries
    osd = bopt.state_dict()
    assert osd["vlb"]["ema_updates"] == 3 and torch.equal(osd["vlb"]["ema"], bopt.ema.cpu())
    d, dopt, _ = _build(**kw)
    d.load_trainable_state_dict(b.trainable_state_dict())
    dopt.load_state_dict(osd)
    assert dopt.ema_updates == 3 and torch.equal(dopt.ema, bopt.ema)
    # a checkpoint written without the average starts it from the restored masters
    e, eopt, esch = _build(**LORA)
    _steps(e, eopt, esch, micro[:2])
    old = str(tmp_path / "plain.ckpt")
    TrainableCheckpoint(str(tmp_path)).save(e, old, 2)
    f, fopt, _ = _build(**kw)
    assert load_trainable_checkpoint(f, old) == 2
    assert fopt.ema_updates == 0 and torch.equal(fopt.ema, f.flat.master) and torch.equal(f.flat.master, e.flat.master)
    assert fopt.step_count == 2


# ------------------------------------------------------------------------------------------------ runner
class _Rec:
    def __init__(self):
        self.rows = []

    def log_metrics(self, metrics, step):
        self.rows.append(dict(metrics))


def _dm(path="synthetic:3x4", batch_size=2):
    from phantom_vlb_amd.datamodule import VLBDataModule, VLBDataModuleConfig
    return VLBDataModule(VLBDataModuleConfig(lazyload_path=path, subject="sub-01", seasons=["s1"], delay=3, window=3,
                                             random_state=1234, shuffle_val_data=False, batch_size=batch_size, geometry="mini",
                                             num_target=128))


def test_closed_form_fit_restarts_the_average_of_the_ridge_tensors(dev):
    from phantom_vlb_amd.litmodule import VLBLitModule
    from phantom_vlb_amd.trainer import Trainer
    m = VLBLitModule(_cfg(cache_features=True, ridge_fit="closed_form", ema_decay=0.9, ema_warmup=False))
    m.configure_model()
    orig, seen = m.fit_ridge_closed_form, []

    def spy(*a, **k):
        seen.append(m.optimizer.ema.clone())
        out = orig(*a, **k)
        seen.append(m.optimizer.ema.clone())
        return out
    m.fit_ridge_closed_form = spy
    Trainer(max_epochs=1, val_check_interval=1.0).fit(m, _dm())
    torch.cuda.synchronize()
    assert len(seen) == 2 and m.optimizer.ema_updates == m.optimizer.step_count > 0
    before, after = seen
    for n, (o, k, _) in m.flat.offsets.items():
        if n in RIDGE:
            assert torch.equal(after[o:o + k], m.flat.master[o:o + k]), n           # the fit was the last thing to touch them
            assert not torch.equal(after[o:o + k], before[o:o + k]), n
        else:
            assert torch.equal(after[o:o + k], before[o:o + k]), n                  # the LayerNorms' average is not the fit's business
            assert not torch.equal(after[o:o + k], m.flat.master[o:o + k]), n


def test_trainer_validates_on_the_average_and_checkpoints_it(dev, tmp_path):
    from phantom_vlb_amd.litmodule import VLBLitModule
    from phantom_vlb_amd.optim import ema_decay_at
    from phantom_vlb_amd.trainer import TrainableCheckpoint, Trainer
    m = VLBLitModule(_cfg(ema_decay=0.999))
    rec, dm = _Rec(), _dm()
    tr = Trainer(max_epochs=1, val_check_interval=1.0, log_every_n_steps=1, logger=rec,
                 callbacks=[TrainableCheckpoint(str(tmp_path), filename="best")])
    tr.fit(m, dm)
    opt = m.optimizer
    assert tr.global_step == opt.ema_updates > 0
    rows = [r for r in rec.rows if "val/brain_loss" in r]
    assert len(rows) == 1 and rows[0]["ema/decay"] == ema_decay_at(opt.ema_updates, 0.999, True) == m.logged["ema/decay"]
    assert "_ema_stash" in m.__dict__ and not m.__dict__["_ema_swapped"]

    def val_loss():
        tot, n = None, 0
        for batch in dm.val_dataloader():
            loss = m.validation_step(batch)["loss"].detach().double()
            tot, n = loss if tot is None else tot + loss, n + 1
        return float(tot) / n
    raw = val_loss()
    with m.averaged_weights():
        averaged = val_loss()
    assert rows[0]["val/brain_loss"] == averaged and averaged != raw
    st = torch.load(tmp_path / "last.ckpt", map_location="cpu", weights_only=False)
    assert torch.equal(st["ema"], opt.ema.cpu()) and st["ema_updates"] == opt.ema_updates
    assert torch.equal(st["state_dict"]["ridge_layer.linear.weight"], m.head.master["ridge_layer.linear.weight"].cpu())   # raw masters
    # ema_eval=False: the same run validates on the last iterate
    m2 = VLBLitModule(_cfg(ema_decay=0.999, ema_eval=False))
    rec2 = _Rec()
    Trainer(max_epochs=1, val_check_interval=1.0, log_every_n_steps=1, logger=rec2).fit(m2, _dm())
    assert torch.equal(m2.flat.master, m.flat.master) and torch.equal(m2.optimizer.ema, opt.ema)
    assert [r for r in rec2.rows if "val/brain_loss" in r][0]["val/brain_loss"] == raw
