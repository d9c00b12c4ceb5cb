"""litmodule.config.optimizer_groups through the module, mini geometry.

The expected state after an optimiser step is computed by the kernels the grouped step stands in for: ONE parent launch
(vlb_adamw_step, or vlb_adamw_step_g16 on bf16 gradients) PER TENSOR on clones of the state snapshotted before the step, with
the tensor's learning rate and weight decay derived here from its name and from the scheduler's recurrence - never read back
from the optimiser - and the clip norm recomputed from the snapshotted gradient.  Everything is compared with torch.equal."""
import math
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
LR, WD, T_MAX = 1e-3, 1e-2, 10

EXAMPLE = [{"params": ["layer_norm*", "*.bias"], "lr_scale": 10, "weight_decay": 0},
           {"params": ["ridge_layer.*", "layer_mix.weight"], "lr_scale": 10},
           {"params": ["*.lora_B.weight"], "lr_scale": 4}]
FULL_GROUPS = [{"params": ["backbone.mm_projector.*"], "lr_scale": 0.1},
               {"params": ["layer_norm*", "*.bias"], "lr_scale": 10, "weight_decay": 0}]
LORA = dict(use_lora=True, freeze_backbone=False, lora_r=16, lora_alpha=32, lora_dropout=0.0)
FULL = dict(freeze_backbone=False, use_lora=False)


def example_rule(name):
    """(lr_scale, weight_decay) of a tensor under EXAMPLE, spelled out by hand: the first matching entry wins."""
    if name.startswith("layer_norm") or name.endswith(".bias"):
        return 10.0, 0.0
    if name.startswith("ridge_layer.") or name == "layer_mix.weight":
        return 10.0, WD
    if name.endswith(".lora_B.weight"):
        return 4.0, WD
    return 1.0, WD


def full_rule(name):
    if name.startswith("backbone.mm_projector."):
        return 0.1, WD
    if name.startswith("layer_norm") or name.endswith(".bias"):
        return 10.0, 0.0
    return 1.0, WD


def cosine_lrs(base, steps, t_max=T_MAX):
    """torch's CosineAnnealingLR (eta_min 0) as it computes it: the recurrence on the group's current lr, in doubles.
    -> the lr in force at optimiser steps 1 .. steps (the scheduler is stepped after each)."""
    out, lr = [], base
    for t in range(steps):
        if t > 0:
            lr = (1 + math.cos(math.pi * t / t_max)) / (1 + math.cos(math.pi * (t - 1) / t_max)) * (lr - 0.0) + 0.0
        out.append(lr)
    return out


def _cfg(**kw):
    from phantom_vlb_amd.litmodule import VLBLitModuleConfig
    base = dict(model_path="none", freeze_backbone=True, use_lora=False, lora_r=None, lora_alpha=None, lora_dropout=None,
                dropout_rate=0.0, num_target=128, l2_lambda=1e-3, lr=LR, betas=[0.9, 0.999], eps=1e-8,
                weight_decay=WD, lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=T_MAX, geometry="mini")
    base.update(kw)
    return VLBLitModuleConfig(**base)


_SHARED = {}


def _params_and_batches(lora, n_micro=1, clips=2, seed=3):
    """Initial weights and micro-batches, computed once per flavour and shared (never modified: configure_model copies)."""
    key = (lora, n_micro)
    if key not in _SHARED:
        import vlb_oracle as O
        g = O.geometry_mini(lora_r=16, lora_alpha=32) if lora else O.geometry_mini()
        p = O.round_bf16(O.init_params(g, seed=seed, lora=lora, lora_b_std=0.02) if lora else O.init_params(g, seed=seed))
        whole = O.synthetic_batch(g, clips * n_micro, seed=seed + 1)
        _SHARED[key] = (p, [{k: v[i * clips:(i + 1) * clips] for k, v in whole.items()} for i in range(n_micro)])
    return _SHARED[key]


def _build(p, k=None, **kw):
    from phantom_vlb_amd.litmodule import VLBLitModule
    m = VLBLitModule(_cfg(**kw))
    m.configure_model(state_dict=p)
    opt, sch = m.configure_optimizers()
    if k is not None:
        m.accumulate_grad_batches = k
    return m, opt[0], sch[0]["scheduler"]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sumsq(grads):
    """The clip norm's sum of squares over the stores' gradients, in store order, as VlbAdamW.step() computes it."""
    from phantom_vlb_amd._lib import check, lib
    dev = grads[0].device
    ss = torch.zeros(1, dtype=torch.float32, device=dev)
    ws = torch.zeros(max(lib.vlb_sumsq_ws_floats(), 1024), dtype=torch.float32, device=dev)
    for g in grads:
        fn = lib.vlb_grad_sumsq_bf16 if g.dtype == BF else lib.vlb_grad_sumsq
        check(fn(g.data_ptr(), g.numel(), ss.data_ptr(), ws.data_ptr(), _stream()), "sumsq")
    return ss


def _per_tensor_parent(offsets, prefix, snap, rule, base_lr_at_step, step, sumsq):
    """One parent launch per tensor on clones of ``snap`` (master, compute, grad, m, v of one store) -> the expected buffers."""
    from phantom_vlb_amd._lib import check, lib
    want = {k: t.clone() for k, t in snap.items()}
    bf = want["grad"].dtype == BF
    fn = lib.vlb_adamw_step_g16 if bf else lib.vlb_adamw_step
    for n, (o, k, _) in offsets.items():
        scale, wd = rule(prefix + n)
        cnt = (k + 7) // 8 * 8 if bf else k          # (the bf16-gradient kernel takes whole 8-element units: the tensor's zero pad)
        check(fn(want["master"].data_ptr() + 4 * o, want["compute"].data_ptr() + 2 * o, want["grad"].data_ptr() + (2 if bf else 4) * o,
                 want["m"].data_ptr() + 4 * o, want["v"].data_ptr() + 4 * o, cnt, base_lr_at_step(scale), 0.9, 0.999, 1e-8, wd, step,
                 sumsq.data_ptr(), 1.0, _stream()), "parent adamw")
    return want


def _stores(m):
    return [m.flat] + ([m.full.flat] if m.full is not None else [])


def _run_and_check(kw, rule, steps=3, k=None):
    lora = bool(kw.get("use_lora"))
    p, micro = _params_and_batches(lora, k or 1)
    m, opt, sch = _build(p, k, **kw)
    rates = {}                                       # lr_scale -> the scheduler's curve for base lr LR * lr_scale
    for step in range(1, steps + 1):
        for b in micro:
            m.training_step(b)
        snaps, grads = [], []
        for i, f in enumerate(_stores(m)):
            g = opt.window_gradient(i) if k else f.grad
            assert g.dtype == (torch.float32 if k or i == 0 else BF)
            snaps.append({"master": f.master.clone(), "compute": f.compute.clone(), "grad": g.clone(), "m": f.m.clone(), "v": f.v.clone()})
            grads.append(snaps[-1]["grad"])
        opt.step()
        sumsq = _sumsq(grads)
        assert torch.equal(sumsq, opt.sumsq) and float(sumsq) > 0

        def lr_at(scale, step=step):
            if scale not in rates:
                rates[scale] = cosine_lrs(LR * scale, steps)
            return rates[scale][step - 1]
        for i, f in enumerate(_stores(m)):
            want = _per_tensor_parent(f.offsets, "backbone." if i else "", snaps[i], rule, lr_at, step, sumsq)
            torch.cuda.synchronize()
            for key, have in (("master", f.master), ("m", f.m), ("v", f.v), ("compute", f.compute)):
                assert torch.equal(have, want[key]), (step, i, key, int((have != want[key]).sum()))
            assert not torch.equal(f.master, snaps[i]["master"])
        sch.step()
    return m, opt


def test_lora_and_head_with_the_example_configuration(dev):
    m, opt = _run_and_check(dict(LORA, optimizer_groups=EXAMPLE), example_rule)
    assert len(opt.param_groups) == 4 and opt.group_names[0] == "default" and opt.tables is not None and len(opt.tables) == 1
    assert [g["weight_decay"] for g in opt.param_groups] == [WD, 0.0, WD, WD]
    # every group was driven by the one scheduler: the configured ratios hold after three steps
    base = opt.param_groups[0]["lr"]
    assert base < LR and [g["lr"] / base for g in opt.param_groups] == pytest.approx([1.0, 10.0, 10.0, 4.0], rel=1e-12)
    bounds, group_of = opt.tables[0]
    assert bounds.is_cuda and bounds.dtype == torch.int64 and group_of.dtype == torch.int32 and int(bounds[-1]) == m.flat.numel
    assert sorted(set(group_of.tolist())) == [0, 1, 2, 3]
    assert sum(len(g["params"]) for g in opt.param_groups) == len(opt.names)


def test_full_finetune_connector_rate_bf16_gradients(dev):
    m, opt = _run_and_check(dict(FULL, optimizer_groups=FULL_GROUPS), full_rule)
    assert len(opt.param_groups) == 3 and len(opt.tables) == 2 and m.full.flat.grad.dtype == BF
    assert sorted(set(opt.tables[1][1].tolist())) == [0, 1]                # the backbone store: the connector and the rest


def test_accumulate_grad_batches_2_reads_the_fp32_accumulators(dev):
    _run_and_check(dict(FULL, optimizer_groups=FULL_GROUPS), full_rule, steps=2, k=2)


class _Counting:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a):
        self.calls += 1
        return self.fn(*a)


def _count_grouped_calls(monkeypatch):
    from phantom_vlb_amd import optim
    counters = {}
    for name in ("vlb_adamw_step_groups", "vlb_adamw_step_groups_g16", "vlb_adamw_step", "vlb_adamw_step_g16"):
        counters[name] = _Counting(getattr(optim.lib, name))
        monkeypatch.setattr(optim.lib, name, counters[name])
    return counters


def test_unit_scales_equal_the_ungrouped_path_and_unset_never_reaches_the_grouped_kernel(dev, monkeypatch):
    p, micro = _params_and_batches(True)
    counters = _count_grouped_calls(monkeypatch)
    masters = {}
    for label, groups in (("unset", None), ("unit", [{"params": ["ridge_layer.*"]}, {"params": ["*.lora_B.weight"], "lr_scale": 1}])):
        for c in counters.values():
            c.calls = 0
        m, opt, sch = _build(p, **dict(LORA, optimizer_groups=groups))
        for _ in range(3):
            m.training_step(micro[0])
            opt.step()
            sch.step()
        torch.cuda.synchronize()
        masters[label] = m.flat.master.clone()
        grouped = counters["vlb_adamw_step_groups"].calls + counters["vlb_adamw_step_groups_g16"].calls
        if groups is None:
            assert len(opt.param_groups) == 1 and opt.tables is None and opt.group_names == ["default"]
            assert grouped == 0 and counters["vlb_adamw_step"].calls == 3
        else:
            assert len(opt.param_groups) == 3 and grouped == 3 and counters["vlb_adamw_step"].calls == 0
    assert torch.equal(masters["unset"], masters["unit"])


def test_resume_restores_every_groups_rate(dev, tmp_path):
    from phantom_vlb_amd.trainer import TrainableCheckpoint, load_trainable_checkpoint
    p, micro = _params_and_batches(True)
    kw = dict(LORA, optimizer_groups=EXAMPLE)

    def steps(m, opt, sch, n):
        for _ in range(n):
            m.training_step(micro[0])
            opt.step()
            sch.step()

    a, aopt, asch = _build(p, **kw)
    steps(a, aopt, asch, 4)
    b, bopt, bsch = _build(p, **kw)
    steps(b, bopt, bsch, 2)
    path = str(tmp_path / "two.ckpt")
    TrainableCheckpoint(str(tmp_path)).save(b, path, 2)
    st = torch.load(path, map_location="cpu", weights_only=False)
    assert st["lrs"] == [g["lr"] for g in bopt.param_groups] and st["lr"] == st["lrs"][0] and len(st["lrs"]) == 4
    assert st["group_names"] == bopt.group_names and st["group_names"][0] == "default"
    c, copt, csch = _build(p, **kw)
    assert load_trainable_checkpoint(c, path) == 2
    assert [g["lr"] for g in copt.param_groups] == st["lrs"]
    steps(c, copt, csch, 2)
    torch.cuda.synchronize()
    for key in ("master", "m", "v", "compute"):
        assert torch.equal(getattr(a.flat, key), getattr(c.flat, key)), key
    assert [g["lr"] for g in copt.param_groups] == [g["lr"] for g in aopt.param_groups]
    assert copt.step_count == aopt.step_count == 4
    # another group count: refused, before anything is loaded
    d, dopt, _ = _build(p, **LORA)
    before = d.flat.master.clone()
    with pytest.raises(ValueError, match="4 optimiser group"):
        load_trainable_checkpoint(d, path)
    assert torch.equal(d.flat.master, before)
    # a checkpoint from before optimizer_groups (no `lrs`): one group - loads into a one-group optimiser, not into four
    del st["lrs"], st["group_names"]
    for key in ("base_lrs", "_last_lr"):
        st["lr_scheduler"][key] = st["lr_scheduler"][key][:1]
    old = str(tmp_path / "old.ckpt")
    torch.save(st, old)
    assert load_trainable_checkpoint(d, old) == 2 and dopt.param_groups[0]["lr"] == st["lr"] and dopt.step_count == 2
    e, _, _ = _build(p, **kw)
    with pytest.raises(ValueError, match="1 optimiser group"):
        load_trainable_checkpoint(e, old)


def test_learning_rate_logging_names(dev):
    from phantom_vlb_amd.trainer import lr_logs
    p, _ = _params_and_batches(True)
    _, opt, _ = _build(p, **dict(LORA, optimizer_groups=EXAMPLE))
    logs = lr_logs(opt, "lr-AdamW")
    assert logs["lr-AdamW"] == LR and [logs[f"lr-AdamW/pg{k}"] for k in (1, 2, 3, 4)] == [LR, LR * 10.0, LR * 10.0, LR * 4.0]
    _, one, _ = _build(p, **LORA)
    assert lr_logs(one, "lr") == {"lr": LR}


def test_unknown_name_is_refused_by_configure_optimizers(dev):
    from phantom_vlb_amd.litmodule import VLBLitModule
    p, _ = _params_and_batches(False)
    m = VLBLitModule(_cfg(optimizer_groups=[{"params": ["*.lora_B.weight"], "lr_scale": 4}]))       # no LoRA in this module
    m.configure_model(state_dict=p)
    with pytest.raises(ValueError, match=r"optimizer_groups\[0\].*ridge_layer.linear.weight"):
        m.configure_optimizers()


# ------------------------------------------------------------------------------------------------ data parallelism
def _dp_worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    for q in (ROOT, os.path.join(ROOT, "oracle")):
        if q not in sys.path:
            sys.path.insert(0, q)
    import vlb_oracle as O
    from phantom_vlb_amd.parallel import attach_data_parallel
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        g = O.geometry_mini(lora_r=16, lora_alpha=32)
        p = O.round_bf16(O.init_params(g, seed=3, lora=True, lora_b_std=0.02))
        whole = O.synthetic_batch(g, 4, seed=4)
        m, opt, _ = _build(p, **dict(LORA, optimizer_groups=EXAMPLE))
        st = attach_data_parallel(m, opt)
        assert st.active and st.numel * 2 == m.flat.numel and int(opt.tables[0][0][-1]) == st.numel
        mine = {k: v[rank * 2:rank * 2 + 2] for k, v in whole.items()}
        ok = True
        for step in (1, 2):
            snap = {k: st.gather_full(k).clone() for k in ("master", "m", "v")}
            snap["compute"] = m.flat.compute.clone()
            m.training_step(mine)
            opt.step()
            snap["grad"] = st.gather_full("grad").clone()          # the reduce-scattered gradient the step read (AdamW leaves it alone)
            sumsq = _sumsq([st.grad])                                # this rank's slices ...
            dist.all_reduce(sumsq)                                   # ... summed over the ranks, as the step does
            assert torch.equal(sumsq, opt.sumsq)
            want = _per_tensor_parent(m.flat.offsets, "", snap, example_rule, lambda scale: LR * scale, step, sumsq)
            after = st.gather_full("master")
            torch.cuda.synchronize()
            ok = ok and torch.equal(after, want["master"]) and torch.equal(st.gather_full("m"), want["m"]) \
                and torch.equal(st.gather_full("v"), want["v"]) and torch.equal(m.flat.compute, want["compute"])
        ret[rank] = {"ok": bool(ok), "master": after.cpu(), "ranges": int(opt.tables[0][1].numel())}
    finally:
        dist.destroy_process_group()


def test_two_ranks_update_their_slices_with_the_groups_rates(dev):
    import random
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_dp_worker, args=(2, 29600 + random.randint(0, 2000), ret), nprocs=2, join=True)
    assert ret[0]["ok"] and ret[1]["ok"]
    assert torch.equal(ret[0]["master"], ret[1]["master"])
    assert ret[0]["ranges"] > 4 and ret[1]["ranges"] > 4
