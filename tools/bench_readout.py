"""Cost of ``readout_layers`` on the 7B LoRA step (bench.py's flagship shapes: r=16, 3 clips, V=2048, both dropouts on).

    python tools/bench_readout.py [rounds]        # default 5 rounds

One process, ONE set of frozen weights shared by every variant (each has its own head, adapters, flat store and
optimiser): the option unset, and the tap lists [32], [16], [8,16,24,32].  Rounds are interleaved - every round runs every
variant: one untimed step, then 3 timed ones (training_step + optimiser step + scheduler; wall clock around
torch.cuda.synchronize()).  Per variant: the median over rounds, min, max and the spread (max - min) of the per-round means,
and the difference to the unset option's median, to be read against that run's own spread.
Then the accumulate-mode d hidden kernel alone at rows = 5861, E = 4096 in tools/bench_hbm_kernels.py's style (HIP events,
algorithmic bytes of the live rows: hidden read once + dx read and written)."""
import os
import statistics
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = (("unset", None), ("[32]", [32]), ("[16]", [16]), ("[8,16,24,32]", [8, 16, 24, 32]))


def build(taps, shared):
    """A 7B LoRA module; every module after the first takes the first one's frozen weights (random init, same seed) instead
    of building 28 GB of its own."""
    from phantom_vlb_amd import litmodule as LM
    cfg = LM.VLBLitModuleConfig(
        model_path="DAMO-NLP-SG/VideoLLaMA2-7B", freeze_backbone=False, use_lora=True, lora_r=16, lora_alpha=32, lora_dropout=0.1,
        dropout_rate=0.1, num_target=2048, l2_lambda=1e-3, lr=1e-4, betas=[0.9, 0.999], eps=1e-8, weight_decay=1e-2,
        lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=50000, geometry="7b", pack_tokens=True, readout_layers=taps)
    m = LM.VLBLitModule(cfg)
    if shared is None:
        m.configure_model()
    else:
        real = LM.Weights
        LM.Weights = lambda *a, **k: shared           # configure_model's one Weights(...) call
        try:
            m.configure_model(state_dict={})
        finally:
            LM.Weights = real
    opt, sch = m.configure_optimizers()
    return m, opt[0], sch[0]["scheduler"]


def step_table(rounds):
    from phantom_vlb_amd.synthetic import synthetic_batch
    dev = torch.device("cuda:0")
    mods = {}
    for name, taps in VARIANTS:
        mods[name] = build(taps, None if not mods else mods["unset"][0].backbone.w)
    batch = synthetic_batch(mods["unset"][0].geometry, 3, seed=1234, device=dev)
    batch["language"], batch["padvals"] = batch["language"].cpu(), batch["padvals"].cpu()

    def step(name):
        m, opt, sch = mods[name]
        m.training_step(batch)
        opt.step()
        sch.step()

    means = {name: [] for name, _ in VARIANTS}
    for _ in range(rounds):
        for name, _ in VARIANTS:
            step(name)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                step(name)
            torch.cuda.synchronize()
            means[name].append((time.perf_counter() - t0) / 3 * 1e3)
    base = statistics.median(means["unset"])
    print(f"LoRA 7B step, 3 clips, {rounds} interleaved rounds x 3 steps, ms per step")
    print(f"{'readout_layers':16s} {'median':>9s} {'min':>9s} {'max':>9s} {'spread':>8s} {'vs unset':>10s}")
    for name, _ in VARIANTS:
        v = means[name]
        med = statistics.median(v)
        print(f"{name:16s} {med:9.2f} {min(v):9.2f} {max(v):9.2f} {max(v) - min(v):8.2f} {med - base:+10.2f}", flush=True)


def accumulate_kernel():
    from phantom_vlb_amd._lib import check, lib
    from phantom_vlb_amd.ops import RowLayout, _stream
    dev = torch.device("cuda:0")
    B, S, E, lens = 3, 2048, 4096, [1990, 1953, 1918]
    rows = sum(lens)
    assert rows == 5861
    lay = RowLayout(B, S, lens, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    wm = torch.rand(B, S, device=dev, generator=g) + 0.01
    wm[:, :700] = 0                                        # prompt / instruction span
    for b, n in enumerate(lens):
        wm[b, n:] = 0
    live = int((wm != 0).sum())
    stats = torch.zeros(B, S, 2, device=dev)
    stats[..., 1] = 1.0
    draw = torch.randn(B, E, device=dev, generator=g) * 1e-3
    # 8 (hidden, dx) pairs in rotation, 96 MB each pair: a pair is out of the 256 MB last-level cache when its turn comes again
    bufs = [(torch.randn(rows, E, device=dev, generator=g).bfloat16(), torch.zeros(rows, E, device=dev, dtype=torch.bfloat16)) for _ in range(8)]
    turn = [0]

    def run(accumulate):
        x, dx = bufs[turn[0] % len(bufs)]
        turn[0] += 1
        check(lib.vlb_head_dhidden(x.data_ptr(), wm.data_ptr(), stats.data_ptr(), draw.data_ptr(), dx.data_ptr(), B, S, E,
                                   lay.cu.data_ptr(), rows, accumulate, _stream()), "vlb_head_dhidden")

    def timeit(fn, reps=24):
        for _ in range(8):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def row(name, nbytes, ms):
        print(f"{name:44s} {nbytes / 1e6:8.1f} MB  {ms * 1e3:8.1f} us  {nbytes / ms / 1e6:7.0f} GB/s  {nbytes / ms / 1e6 / 8000 * 100:5.1f}% of 8 TB/s", flush=True)
    print(f"d hidden kernels, rows = {rows}, E = {E}, {live} live rows")
    t_w = min(timeit(lambda: run(0)) for _ in range(3))
    row("head_dhidden write (live: r hidden, w dx; dead: w)", live * E * 2 + rows * E * 2, t_w)
    t_a = min(timeit(lambda: run(1)) for _ in range(3))
    row("head_dhidden accumulate (live rows: r hidden, rw dx)", 3 * live * E * 2, t_a)


if __name__ == "__main__":
    warnings.simplefilter("ignore")
    if "--kernel-only" not in sys.argv:
        step_table(int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 5)
    accumulate_kernel()
