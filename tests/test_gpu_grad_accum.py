"""Gradient accumulation (accumulate_grad_batches = k) on the GPU: the two accumulate kernels (equalities: an fp32 sum has
one correctly rounded answer), the module's window against hand-summed k = 1 gradients (bit for bit: 1/k is a power of two
for k in {2, 4}), one window against the oracle and against the single step on the concatenated batch, and both runners.
Mini geometry throughout; the whole file runs in about 35 s on one MI355X."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


def _cfg(**kw):
    from phantom_vlb_amd.litmodule import VLBLitModuleConfig
    base = dict(model_path="none", freeze_backbone=True, use_lora=False, lora_r=None, lora_alpha=None, lora_dropout=None,
                dropout_rate=0.0, num_target=128, l2_lambda=1e-3, lr=1e-3, betas=[0.9, 0.999], eps=1e-8,
                weight_decay=1e-2, lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=50000, geometry="mini")
    base.update(kw)
    return VLBLitModuleConfig(**base)


LORA = dict(use_lora=True, freeze_backbone=False, lora_r=16, lora_alpha=32, lora_dropout=0.0)
LORA_DROP = dict(LORA, lora_dropout=0.1, dropout_rate=0.1)
FULL = dict(freeze_backbone=False, use_lora=False)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _accum(acc, g, off, n, first, sumsq=None, ws=None):
    from phantom_vlb_amd._lib import check, lib
    fn = lib.vlb_grad_accum_bf16 if g.dtype == BF else lib.vlb_grad_accum
    check(fn(acc.data_ptr() + 4 * off, g.data_ptr() + g.element_size() * off, n, int(first),
             None if sumsq is None else sumsq.data_ptr(), None if ws is None else ws.data_ptr(), _stream()), "vlb_grad_accum")


def _mini_flat_numel():
    from phantom_vlb_amd.litmodule import VLBLitModule
    m = VLBLitModule(_cfg(**LORA))
    m.configure_model()
    m.configure_optimizers()
    return m.flat.numel


# ---------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_accumulate_kernels_are_exact(dev, dtype):
    """first=1 copies, first=0 is torch's fp32 `acc + g`, bit for bit, for every n and on an offset sub-range whose
    surroundings stay untouched; the fused sum of squares equals vlb_grad_sumsq on the resulting accumulator bit for bit."""
    from phantom_vlb_amd._lib import check, lib
    gen = torch.Generator(device=dev).manual_seed(11)
    ws = torch.zeros(max(lib.vlb_sumsq_ws_floats(), 1024), device=dev)
    sizes = [1, 7, 8, 1000003, _mini_flat_numel()]
    cases = [(0, n) for n in sizes] + [(8, 1), (4096 + 24, 7), (8 * 1001, 100003), (64, 5 * 1024 * 1024 + 3)]
    for off, n in cases:
        total = off + n + 40
        g = (torch.randn(total, device=dev, generator=gen) * 3).to(dtype)
        a0 = torch.randn(total, device=dev, generator=gen)
        for fused in (False, True):
            for first in (1, 0):
                acc = a0.clone()
                ss = torch.zeros(1, device=dev)
                _accum(acc, g, off, n, first, ss if fused else None, ws if fused else None)
                want = a0.clone()
                want[off:off + n] = g[off:off + n].float() if first else a0[off:off + n] + g[off:off + n].float()
                assert torch.equal(acc, want), (dtype, off, n, first, fused)
                if fused:
                    ref = torch.zeros(1, device=dev)
                    check(lib.vlb_grad_sumsq(want.data_ptr() + 4 * off, n, ref.data_ptr(), ws.data_ptr(), _stream()), "sumsq")
                    assert torch.equal(ss, ref), (dtype, off, n, first, float(ss), float(ref))
                    _accum(acc, g, off, n, 0, ss, ws)                     # sumsq[0] is ADDED to, like vlb_grad_sumsq does
                    check(lib.vlb_grad_sumsq(acc.data_ptr() + 4 * off, n, ref.data_ptr(), ws.data_ptr(), _stream()), "sumsq")
                    assert torch.equal(ss, ref)


# ---------------------------------------------------------------------------------------------------- module, exact
def _build(p, k=None, **kw):
    from phantom_vlb_amd.litmodule import VLBLitModule
    m = VLBLitModule(_cfg(**kw))
    m.configure_model(state_dict=p)
    opt, _ = m.configure_optimizers()
    if k is not None:
        m.accumulate_grad_batches = k
    return m, opt[0]


def _params_and_batches(kw, n_micro, clips=2, seed=3):
    import vlb_oracle as O
    lora = bool(kw.get("use_lora"))
    g = O.geometry_mini(lora_r=16, lora_alpha=32) if lora else O.geometry_mini()
    p = O.round_bf16(O.init_params(g, seed=seed, lora=lora, lora_b_std=0.02) if lora else O.init_params(g, seed=seed))
    whole = O.synthetic_batch(g, clips * n_micro, seed=seed + 1)
    micro = [{key: v[i * clips:(i + 1) * clips] for key, v in whole.items()} for i in range(n_micro)]
    return g, p, whole, micro


def _stores(m):
    return [m.flat] + ([m.full.flat] if m.full is not None else [])


def _prime_cache(m, micro):
    """Feature-cache case: every clip's features are stored by one uncached pass, so the steps under test run cached."""
    from phantom_vlb_amd.feature_cache import FeatureCache
    m.feature_caches["train"] = FeatureCache("train", sum(len(b["index"]) for b in micro), m.geometry.dim, m.device)
    for b in micro:
        m.training_step(b)
        assert not m._cached_step
    m.optimizer.step()                    # (closes the priming window of the accumulating module; both modules take it alike)


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("case", ["frozen", "lora_dropout", "cached", "full"])
def test_window_equals_hand_summed_micro_batch_gradients(dev, case, k):
    """A k = 1 module over the k micro-batches, one training_step at a time (g_1 .. g_k), and a second module from the same
    weights over the same micro-batches as ONE window: its accumulator is ((g_1/k + g_2/k) + ...) summed in fp32 in
    micro-batch order, bit for bit; after opt.step() its masters are those of a k = 1 optimiser handed that gradient; and the
    window run twice gives the same bits."""
    from phantom_vlb_amd._lib import check, lib
    kw = {"frozen": dict(dropout_rate=0.1), "lora_dropout": LORA_DROP, "cached": dict(dropout_rate=0.1, cache_features=True),
          "full": dict(FULL, dropout_rate=0.1)}[case]
    g, p, whole, micro = _params_and_batches(kw, k)
    if case == "cached":
        for i, b in enumerate(micro):
            b["index"] = torch.arange(2 * i, 2 * i + 2)

    def window():
        m, opt = _build(p, k, **kw)
        if case == "cached":
            # prime with k = 1 semantics on both modules alike: one uncached pass, no accumulation involved
            m.accumulate_grad_batches = 1
            _prime_cache(m, micro)
            m.accumulate_grad_batches = k
        for b in micro:
            m.training_step(b)
            assert case != "cached" or m._cached_step
        return m, opt

    a, aopt = _build(p, 1, **kw)
    if case == "cached":
        _prime_cache(a, micro)
    start = [(f.master.clone(), f.m.clone(), f.v.clone()) for f in _stores(a)]
    gs = []
    for b in micro:
        a.training_step(b)
        assert case != "cached" or a._cached_step
        gs.append([f.grad.float().clone() for f in _stores(a)])
    assert aopt.accum == [None] * len(aopt.flats)
    want = []
    for i in range(len(_stores(a))):
        acc = gs[0][i] / k
        for j in range(1, k):
            acc = acc + gs[j][i] / k
        want.append(acc)

    b_, bopt = window()
    assert a.rng_state() == b_.rng_state()
    for i, w in enumerate(want):
        got = bopt.accum[i]
        assert got is not None and got.dtype == torch.float32
        diff = (got - w).abs().max()
        print(f"{case} k={k} store {i}: max |acc - hand sum| = {float(diff):.3e} of max {float(w.abs().max()):.3e}")
        assert torch.equal(got, w), (case, k, i, float(diff))
    # .grad of a trainable is what the optimiser will consume: the accumulator, once the window is complete
    n0, p0 = b_.trainable_named_parameters()[0]
    o, cnt, shp = b_.flat.offsets[n0]
    assert p0.grad.data_ptr() == bopt.accum[0][o:o + cnt].data_ptr()
    bopt.step()
    # reference update: the k = 1 optimiser's own launches (clip norm over all stores, then AdamW per store) on `want`
    if case != "full":
        a.flat.grad.copy_(want[0])
        aopt.step()
        ref_masters = [a.flat.master]
    else:
        ss = torch.zeros(1, device=dev)
        ref_masters = []
        for w in want:
            check(lib.vlb_grad_sumsq(w.data_ptr(), w.numel(), ss.data_ptr(), aopt.sumsq_ws.data_ptr(), _stream()), "sumsq")
        for (ms, m1, v1), w in zip(start, want):
            check(lib.vlb_adamw_step(ms.data_ptr(), None, w.data_ptr(), m1.data_ptr(), v1.data_ptr(), w.numel(), 1e-3, 0.9, 0.999,
                                     1e-8, 1e-2, 1, ss.data_ptr(), 1.0, _stream()), "adamw")
            ref_masters.append(ms)
    for f, ref in zip(_stores(b_), ref_masters):
        assert torch.equal(f.master, ref)
        assert torch.equal(f.compute, ref.to(BF))
    assert bopt.step_count == (2 if case == "cached" else 1) and bopt.window_gradient(0) is None      # (cached: + the priming step)
    c_, copt = window()
    copt.step()
    for fb, fc in zip(_stores(b_), _stores(c_)):
        assert torch.equal(fb.master, fc.master) and torch.equal(copt.accum[0], bopt.accum[0])


# ---------------------------------------------------------------------------------------------------- module, oracle
def _oracle_flat_grad(m, p, whole, g, lora):
    """The oracle's autograd gradient of the whole batch, laid out like the module's flat store."""
    import vlb_oracle as O
    names = O.trainable_names(p, not lora, lora)
    pr = {n: (v.clone().requires_grad_(True) if n in names else v) for n, v in p.items()}
    loss, _ = O.training_loss(pr, whole, g)
    loss.backward()
    ref = torch.zeros(m.flat.numel)
    for n, (o, cnt, shp) in m.flat.offsets.items():
        gr = pr[n].grad
        if "lora_B" in n:
            gr = gr.t()                   # the kernels keep B transposed ([r, out])
        ref[o:o + cnt] = gr.reshape(-1)
    return ref


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("lora", [False, True])
def test_window_tracks_oracle_and_single_step_on_the_whole_batch(dev, lora, k):
    """One window of k micro-batches of 2 clips against (a) the oracle's autograd on the 2k-clip batch and (b) this
    package's single step on it, dropout off, under tests/test_gpu_data_parallel.py's bars for "bf16 activations, different
    batch split": gradient max-error / max < 2e-2 frozen, < 4e-2 LoRA; masters after one AdamW step within 2.5e-3."""
    kw = LORA if lora else {}
    g, p, whole, micro = _params_and_batches(kw, k)
    m, opt = _build(p, k, **kw)
    for b in micro:
        m.training_step(b)
    acc = opt.accum[0].clone()
    opt.step()
    s, sopt = _build(p, 1, **kw)
    s.training_step(whole)
    g_single = s.flat.grad.clone()
    sopt.step()
    torch.cuda.synchronize()
    ref = _oracle_flat_grad(m, p, whole, g, lora)
    err_oracle = float((acc.cpu() - ref).abs().max() / ref.abs().max())
    err_single = float((acc - g_single).abs().max() / g_single.abs().max())
    perr = float((m.flat.master - s.flat.master).abs().max())
    print(f"lora={lora} k={k}: grad err vs oracle {err_oracle:.3e}, vs single step {err_single:.3e}, masters {perr:.3e}")
    bar = 4e-2 if lora else 2e-2
    assert err_oracle < bar, err_oracle
    assert err_single < bar, err_single
    assert perr < 2.5e-3, perr


# ---------------------------------------------------------------------------------------------------- runners
def _dm(spec="synthetic:3x4", batch_size=2):
    from phantom_vlb_amd.datamodule import VLBDataModule, VLBDataModuleConfig
    return VLBDataModule(VLBDataModuleConfig(lazyload_path=spec, subject="sub-01", seasons=["s1"], delay=3, window=3,
                                             random_state=1234, shuffle_val_data=False, batch_size=batch_size, geometry="mini",
                                             num_target=128))


def _train_batches(m, dm, epochs):
    """The batches Trainer.fit feeds, in its order (sampler re-seeded per epoch), staged like its prefetcher stages them."""
    loader = dm.train_dataloader()
    for epoch in range(epochs):
        if hasattr(loader.sampler, "set_epoch"):
            loader.sampler.set_epoch(epoch)
        for b in loader:
            yield m.transfer_batch_to_device(b, m.device)


def test_builtin_runner_counts_optimiser_steps_and_matches_a_hand_loop(dev):
    """8 batches at k = 2: global_step, the scheduler, the AdamW step count are 4, the dropout counters 8; the masters are
    those of a hand-driven loop of training_step x2 + step."""
    from phantom_vlb_amd.litmodule import VLBLitModule
    from phantom_vlb_amd.trainer import Trainer
    dm = _dm()
    n = len(dm.train_dataloader())
    assert n >= 2 and n % 2 == 0, n          # whole windows per epoch, so the hand loop below needs no epoch bookkeeping
    epochs = -(-8 // n)
    a = VLBLitModule(_cfg(**LORA_DROP))
    ta = Trainer(max_epochs=epochs, max_steps=4, val_check_interval=1.0, log_every_n_steps=1, accumulate_grad_batches=2)
    ta.fit(a, dm)
    assert ta.global_step == 4 and a.scheduler.last_epoch == 4 and a.optimizer.step_count == 4
    assert a.rng_state() == {"head_step": 8, "lora_step": 8}
    b = VLBLitModule(_cfg(**LORA_DROP))
    b.configure_model()
    opts, scheds = b.configure_optimizers()
    b.accumulate_grad_batches = 2
    for i, batch in enumerate(_train_batches(b, _dm(), epochs)):
        if i == 8:
            break
        b.training_step(batch)
        if i % 2 == 1:
            opts[0].step()
            scheds[0]["scheduler"].step()
    assert torch.equal(a.flat.master, b.flat.master) and torch.equal(a.flat.compute, b.flat.compute)


def test_resume_is_exact_with_validation_falling_due_mid_window(dev, tmp_path):
    """4 optimiser steps straight == 2 steps, checkpoint, fit(ckpt_path=) for 2 more - both dropouts on, k = 2, and a
    val_check_interval that falls due on the FIRST micro-batch of a window: validation and the checkpoint wait for the
    window boundary, so the checkpoint holds whole optimiser steps only and the resumed run lands on the same bits."""
    from phantom_vlb_amd.litmodule import VLBLitModule
    from phantom_vlb_amd.trainer import TrainableCheckpoint, Trainer
    dm = _dm()
    n = len(dm.train_dataloader())
    assert n >= 4, n
    kw = dict(max_epochs=4, val_check_interval=3, log_every_n_steps=1, accumulate_grad_batches=2)     # due after batch 3: mid-window
    a = VLBLitModule(_cfg(**LORA_DROP))
    Trainer(max_steps=4, **kw).fit(a, _dm())
    b = VLBLitModule(_cfg(**LORA_DROP))
    tb = Trainer(max_steps=2, callbacks=[TrainableCheckpoint(str(tmp_path), filename="best")], **kw)
    tb.fit(b, _dm())
    st = torch.load(tmp_path / "last.ckpt", map_location="cpu", weights_only=False)
    assert st["global_step"] == 2 and st["opt_step"] == 2 and st["lr_scheduler"]["last_epoch"] == 2
    assert st["rng"] == {"head_step": 4, "lora_step": 4}            # written after batch 4 (the boundary), not after batch 3
    assert not any("accum" in key for key in st)
    c = VLBLitModule(_cfg(**LORA_DROP))
    tc = Trainer(max_steps=4, **kw)
    tc.fit(c, _dm(), ckpt_path=str(tmp_path / "last.ckpt"))
    assert tc.global_step == 4 and c.optimizer.step_count == 4
    assert torch.equal(a.flat.master, c.flat.master) and torch.equal(a.flat.compute, c.flat.compute)
    assert torch.equal(a.flat.m, c.flat.m) and torch.equal(a.flat.v, c.flat.v)


def test_k1_is_the_unchanged_path(dev):
    """accumulate_grad_batches = 1: three steps through the runner equal a loop that never touches the new code (training_step
    with no runner attached, the optimiser's step), bit for bit, and the optimiser holds no accumulator."""
    from phantom_vlb_amd.litmodule import VLBLitModule
    from phantom_vlb_amd.trainer import Trainer
    a = VLBLitModule(_cfg(**LORA_DROP))
    Trainer(max_epochs=3, max_steps=3, val_check_interval=1.0, accumulate_grad_batches=1).fit(a, _dm())
    assert a.optimizer.accum == [None] and a.optimizer.step_count == 3
    b = VLBLitModule(_cfg(**LORA_DROP))
    b.configure_model()
    opts, scheds = b.configure_optimizers()
    for i, batch in enumerate(_train_batches(b, _dm(), 3)):
        if i == 3:
            break
        b.training_step(batch)
        opts[0].step()
        scheds[0]["scheduler"].step()
    assert opts[0].accum == [None]
    assert torch.equal(a.flat.master, b.flat.master) and torch.equal(a.flat.compute, b.flat.compute)


LIGHTNING_ORDER = r'''
import torch
import lightning.pytorch as lp
from src.litmodule import VLBLitModule, VLBLitModuleConfig
from src.datamodule import VLBDataModule, VLBDataModuleConfig
from phantom_vlb_amd import trainer as T

K = 2

def cfg():
    return VLBLitModuleConfig(model_path="none", freeze_backbone=False, use_lora=True, lora_r=16, lora_alpha=32, lora_dropout=0.1,
                              dropout_rate=0.1, num_target=128, l2_lambda=1e-3, lr=1e-3, betas=[0.9, 0.999], eps=1e-8, weight_decay=1e-2,
                              lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=50000, geometry="mini")

def dm():
    return VLBDataModule(VLBDataModuleConfig(lazyload_path="synthetic:3x4", subject="sub-01", seasons=["s1"], delay=3, window=3,
                                             random_state=1234, shuffle_val_data=False, batch_size=2, geometry="mini", num_target=128))

def drive(model, datamodule, trainer, max_steps, divisor):
    """Lightning 2.x automatic optimisation under accumulate_grad_batches = K for one optimiser: every batch runs the closure
    { training_step -> zero_grad ONLY when the batch opens a window -> (loss / K).backward() }; batches that do not close a
    window call the closure alone, the closing one hands it to optimizer.step(closure) (gradient clipping configured inside),
    then the scheduler steps and global_step counts."""
    assert isinstance(model, lp.LightningModule)
    model.trainer = trainer
    model.configure_model()
    opts, scheds = model.configure_optimizers()
    opt, sched = opts[0], scheds[0]["scheduler"]
    model.on_fit_start()
    model.train()
    loader = datamodule.train_dataloader()
    n = len(loader)
    for epoch in range(trainer.max_epochs):
        if hasattr(loader.sampler, "set_epoch"):
            loader.sampler.set_epoch(epoch)
        for batch_idx, batch in enumerate(loader):
            batch = model.transfer_batch_to_device(batch, model.device, 0)
            opens = batch_idx % K == 0
            closes = (batch_idx + 1) % K == 0 or batch_idx + 1 == n

            def closure():
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    loss = model.training_step(batch)
                if opens:
                    opt.zero_grad()
                (loss / divisor).backward()
                if closes:
                    model.configure_gradient_clipping(opt, trainer.gradient_clip_val, None)
                return loss
            if not closes:
                closure()
                continue
            opt.step(closure=closure)
            sched.step()
            trainer.global_step += 1
            if trainer.global_step >= max_steps:
                return

a = VLBLitModule(cfg())
ta = lp.Trainer(precision="bf16-mixed", gradient_clip_val=1, max_epochs=4, accumulate_grad_batches=K)
drive(a, dm(), ta, 4, K)
assert ta.global_step == 4 and a.optimizer.step_count == 4 and a.rng_state() == {"head_step": 8, "lora_step": 8}
b = VLBLitModule(cfg())
tb = T.Trainer(precision="bf16-mixed", gradient_clip_val=1, max_epochs=4, max_steps=4, val_check_interval=1.0, accumulate_grad_batches=K)
tb.fit(b, dm())
assert tb.global_step == 4
assert torch.equal(a.flat.master, b.flat.master) and torch.equal(a.flat.compute, b.flat.compute), "parameters differ"
# an upstream gradient other than 1/K (here: the loss not divided at all) is refused, not silently stepped
c = VLBLitModule(cfg())
try:
    drive(c, dm(), lp.Trainer(precision="bf16-mixed", gradient_clip_val=1, max_epochs=1, accumulate_grad_batches=K), 1, 1)
    raise SystemExit("an undivided loss was accepted under accumulate_grad_batches = 2")
except ValueError as e:
    assert "upstream gradient" in str(e), e
print("ACCUM_BRIDGE_OK")
'''


def test_lightning_accumulation_order_matches_the_builtin_runner(dev, tmp_path):
    """Lightning's accumulation sequence - zero_grad only when a window opens, (loss / k).backward() every batch,
    optimizer.step(closure) only on the closing batch - leaves the masters the built-in runner leaves, bit for bit, with both
    dropouts on; `on_fit_start` accepts k = 2; a loss that arrives with an upstream gradient other than 1/k raises."""
    import subprocess
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import fake_lightning
    root = fake_lightning.write(tmp_path / "site")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, ROOT, os.path.join(ROOT, "oracle")]))
    r = subprocess.run([sys.executable, "-c", LIGHTNING_ORDER], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0 and "ACCUM_BRIDGE_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---------------------------------------------------------------------------------------------------- two ranks
class _CountingComm:
    """TorchComm with every reduce-scatter call logged next to the number of training_steps begun so far."""

    def __init__(self, inner, clock):
        self.inner, self.clock, self.calls = inner, clock, []
        self.world, self.rank = inner.world, inner.rank

    def reduce_scatter(self, out, inp):
        self.calls.append(self.clock[0])
        return self.inner.reduce_scatter(out, inp)

    def all_gather(self, out, inp):
        return self.inner.all_gather(out, inp)

    def all_reduce_scalar(self, t):
        return self.inner.all_reduce_scalar(t)


def _worker(rank, world, port, lora, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    for p_ in (ROOT, os.path.join(ROOT, "oracle")):
        if p_ not in sys.path:
            sys.path.insert(0, p_)
    from phantom_vlb_amd.parallel import TorchComm, attach_data_parallel
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        kw = LORA if lora else {}
        g, p, whole, _ = _params_and_batches(kw, 1, clips=4)
        m, opt = _build(p, 2, **kw)
        clock = [0]
        comm = _CountingComm(TorchComm(), clock)
        st = attach_data_parallel(m, opt, comm=comm)
        assert st.active and m.world_size == 2
        for j in range(2):                      # rank r's window: clips 2r, 2r + 1, one per micro-batch
            clock[0] = j + 1
            m.training_step({key: v[2 * rank + j:2 * rank + j + 1] for key, v in whole.items()})
        calls_before_step = list(comm.calls)
        opt.step()
        g_dp = st.gather_full("grad")
        st.gather_masters()
        torch.cuda.synchronize()
        out = {"master": m.flat.master.cpu(), "compute": m.flat.compute.float().cpu(), "calls": calls_before_step,
               "segments": len(st.segments), "all_calls": list(comm.calls)}
        if rank == 0:
            ref, ropt = _build(p, 1, **kw)
            ref.training_step(whole)
            g_ref = ref.flat.grad.clone()
            ropt.step()
            torch.cuda.synchronize()
            out["err"] = float((g_dp - g_ref).abs().max() / g_ref.abs().max())
            out["perr"] = float((m.flat.master - ref.flat.master).abs().max())
        ret[rank] = out
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("lora", [False, True])
def test_two_ranks_accumulate_locally_and_reduce_once(dev, lora):
    """2 ranks x k = 2 x 1 clip against the single-process 4-clip step (test_gpu_data_parallel.py's harness and bars); both
    ranks end on the same bits; no reduce-scatter is started before the window's last micro-batch, and each segment is
    reduced exactly once per optimiser step."""
    import random
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(2, 31700 + random.randint(0, 2000), lora, ret), nprocs=2, join=True)
    print(f"lora={lora}: grad err {ret[0]['err']:.3e}, masters {ret[0]['perr']:.3e}, reduce-scatter calls at {ret[0]['all_calls']}")
    assert ret[0]["err"] < (4e-2 if lora else 2e-2), ret[0]["err"]
    assert ret[0]["perr"] < 2.5e-3, ret[0]["perr"]
    assert torch.equal(ret[0]["master"], ret[1]["master"]) and torch.equal(ret[0]["compute"], ret[1]["compute"])
    for r in (0, 1):
        assert all(c == 2 for c in ret[r]["all_calls"]), ret[r]["all_calls"]          # none during micro-batch 1
        assert len(ret[r]["all_calls"]) == ret[r]["segments"]
        if lora:
            assert len(ret[r]["calls"]) >= ret[r]["segments"] - 1                    # the layer segments went out under backward


def _worker_full(rank, world, port, full_shard, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    for p_ in (ROOT, os.path.join(ROOT, "oracle")):
        if p_ not in sys.path:
            sys.path.insert(0, p_)
    from phantom_vlb_amd.parallel import attach_data_parallel, sync_module_states
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        g, p, whole, _ = _params_and_batches(FULL, 1, clips=2)
        m, opt = _build(p, 2, **FULL)
        attach_data_parallel(m, opt, full_shard=full_shard)
        sync_module_states(m)
        try:
            m.training_step({key: v[rank:rank + 1] for key, v in whole.items()})
            ret[rank] = "accepted"
        except ValueError as e:
            ret[rank] = str(e)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("full_shard", [True, False])
def test_full_finetune_under_data_parallelism_refuses_accumulation(dev, full_shard):
    import random
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker_full, args=(2, 31700 + random.randint(0, 2000), full_shard, ret), nprocs=2, join=True)
    for r in (0, 1):
        assert "accumulate_grad_batches=2" in ret[r] and "data parallelism" in ret[r], ret[r]
        assert ("FULL_SHARD" if full_shard else "SHARD_GRAD_OP") in ret[r]
