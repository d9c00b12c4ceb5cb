"""The EMA entries of the fused clip + AdamW step (vlb_adamw_step_ema / vlb_adamw_step_groups_ema) against the
same steps without the average, on the same buffers.  All four launch instantiations of ONE kernel (csrc/adamw.hip), with and
without the average, so both pairs are like for like and should sit on the byte ratio.  (Before the kernels were unified
vlb_adamw_step was a separate 4-byte-lane kernel and the ungrouped pair came out below it: profiles/adamw_ema_kernels.txt.)

  python tools/bench_adamw_ema.py [repetitions >= 20]

The 7B LoRA r=16 flat store (50.6 M elements, flat.FlatTrainables' layout with its padding), fp32 gradients:
* vlb_adamw_step against vlb_adamw_step_ema;
* vlb_adamw_step_groups against vlb_adamw_step_groups_ema, with the range table the README's example optimizer_groups gives.
The two entries of a pair alternate in one process; every launch is timed on its own with device events; the medians over the
repetitions (after three warm-up rounds) and their ratio are printed.  30 B move per element without the average, 38 B with
it (one more fp32 read and write): by bytes the expected ratio is 38 / 30 = 1.27.
"""
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_adamw_groups import EXAMPLE, lora7b_store, timed  # noqa: E402
from phantom_vlb_amd._lib import check, lib  # noqa: E402
from phantom_vlb_amd.optim_groups import assign_groups, group_ranges, group_specs, normalize_optimizer_groups  # noqa: E402

BF = torch.bfloat16
dev = torch.device("cuda:0")
DECAY = 0.999


def pair(label, n, table, reps):
    gen = torch.Generator(device=dev).manual_seed(0)
    mst = torch.randn(n, device=dev, generator=gen)
    grd = torch.randn(n, device=dev, generator=gen)
    m1 = torch.zeros(n, device=dev)
    v1 = torch.zeros(n, device=dev)
    ema = mst.clone()
    cp = torch.zeros(n, device=dev, dtype=BF)
    ss = torch.full((1,), 4.0, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    state = (mst.data_ptr(), cp.data_ptr(), grd.data_ptr(), m1.data_ptr(), v1.data_ptr())
    if table is None:
        names = ("vlb_adamw_step", "vlb_adamw_step_ema")
        rates = (1e-4, 0.9, 0.999, 1e-8, 1e-2, 1, ss.data_ptr(), 1.0)

        def parent():
            check(lib.vlb_adamw_step(*state, n, *rates, st), names[0])

        def with_ema():
            check(lib.vlb_adamw_step_ema(*state, ema.data_ptr(), n, *rates, DECAY, st), names[1])
    else:
        names = ("vlb_adamw_step_groups", "vlb_adamw_step_groups_ema")
        bounds, group_of, lrs, wds = table
        G = len(lrs)
        bounds, group_of = bounds.to(dev), group_of.to(dev)
        tab = (bounds.data_ptr(), group_of.data_ptr(), group_of.numel(), (ctypes.c_float * G)(*lrs), (ctypes.c_float * G)(*wds), G,
               0.9, 0.999, 1e-8, 1, ss.data_ptr(), 1.0)

        def parent():
            check(lib.vlb_adamw_step_groups(*state, n, *tab, st), names[0])

        def with_ema():
            check(lib.vlb_adamw_step_groups_ema(*state, ema.data_ptr(), n, *tab, DECAY, st), names[1])

    for _ in range(3):
        parent()
        with_ema()
    torch.cuda.synchronize()
    tp, te = [], []
    for _ in range(reps):
        tp.append(timed(parent))
        te.append(timed(with_ema))
    mp_, me = statistics.median(tp), statistics.median(te)
    print(f"{label}: n = {n / 1e6:.1f} M, {reps} repetitions each, interleaved", flush=True)
    print(f"  {names[0]:28s} median {mp_ * 1e3:9.1f} us  {n * 30 / mp_ / 1e6:7.0f} GB/s")
    print(f"  {names[1]:28s} median {me * 1e3:9.1f} us  {n * 38 / me / 1e6:7.0f} GB/s")
    print(f"  with EMA / parent = {me / mp_:.3f}   (by bytes: {38 / 30:.3f})", flush=True)


def main():
    reps = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 25
    entries = normalize_optimizer_groups(EXAMPLE)
    specs = group_specs(entries, 1e-4, 1e-2)
    offs, numel = lora7b_store()
    assert numel == 50_561_280, numel
    bounds, group_of = group_ranges(offs, numel, assign_groups(list(offs), entries))
    pair("one group, 7B LoRA r=16 store", numel, None, reps)
    pair("example optimizer_groups, 7B LoRA r=16 store", numel,
         (bounds, group_of, [s["lr"] for s in specs], [s["weight_decay"] for s in specs]), reps)


if __name__ == "__main__":
    main()
