#!/usr/bin/env python
"""Times of the closed-form ridge fit under target weights on one GPU:

* accumulate: vlb_ridge_gram_accumulate_masked + vlb_ridge_sumsq_accumulate_masked beside the unmasked pair at n = 512,
  E = 4096, V = 2048 with half of the targets masked; the two alternate call by call and the medians are compared;
* whole fit: ridge_cv + ridge_solve on synthetic fold sums, unweighted, with a mask (D = 1 level) and with three levels (D = 3).

Medians of ``--reps`` (default 9; the whole fit: at most 3); wall = host clock around the call ending in a synchronise, GPU =
device events.

    python tools/bench_ridge_wfit.py [--reps 9] [--skip-fit]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phantom_vlb_amd._lib import check, lib          # noqa: E402
from phantom_vlb_amd.head import BrainHead           # noqa: E402

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, a.elapsed_time(b)


def timed_pair(fa, fb, reps):
    """fa and fb alternate call by call -> ((wall, GPU) medians of fa, of fb)"""
    for f in (fa, fb):
        f()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(once(fa))
        tb.append(once(fb))
    med = lambda t: tuple(statistics.median(x[i] for x in t) for i in range(2))
    return med(ta), med(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--skip-fit", action="store_true")
    args = ap.parse_args()
    dev = "cuda"
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator().manual_seed(0)

    n, E, V = 512, 4096, 2048
    z = (torch.randn(n, E, generator=gen) + 0.5).to(BF16).to(dev)
    y = torch.randn(n, V, generator=gen).to(dev)
    keep = (torch.arange(V) % 2 == 0).float().to(dev)                          # half of the targets masked
    G, C = torch.zeros(E, E, dtype=F64, device=dev), torch.zeros(V, E, dtype=F64, device=dev)
    sz, sy, syy = torch.zeros(E, dtype=F64, device=dev), torch.zeros(V, dtype=F64, device=dev), torch.zeros(V, dtype=F64, device=dev)

    def plain():
        check(lib.vlb_ridge_gram_accumulate(z.data_ptr(), y.data_ptr(), V, G.data_ptr(), C.data_ptr(), sz.data_ptr(), sy.data_ptr(),
                                            n, E, V, st), "gram")
        check(lib.vlb_ridge_sumsq_accumulate(y.data_ptr(), V, syy.data_ptr(), n, V, st), "sumsq")

    def masked():
        check(lib.vlb_ridge_gram_accumulate_masked(z.data_ptr(), y.data_ptr(), V, keep.data_ptr(), G.data_ptr(), C.data_ptr(),
                                                   sz.data_ptr(), sy.data_ptr(), n, E, V, st), "gram masked")
        check(lib.vlb_ridge_sumsq_accumulate_masked(y.data_ptr(), V, keep.data_ptr(), syy.data_ptr(), n, V, st), "sumsq masked")
    (pw, pg), (mw, mg) = timed_pair(plain, masked, args.reps)
    print(f"accumulate n={n} E={E} V={V}, half masked, alternating, medians of {args.reps}: unmasked {pw:.3f} / {pg:.3f} ms, "
          f"masked {mw:.3f} / {mg:.3f} ms (wall / GPU); masked / unmasked GPU {mg / pg:.3f}")
    del G, C, z, y
    if args.skip_fit:
        return

    # the whole fit on synthetic fold sums: E = 4096, V = 1000, K = 5, L = 10, n_k = 640 (tools/bench_ridge_rows.py's)
    E, V, K, L, nk = 4096, 1000, 5, 10, 640
    g_list = [10.0 ** (p / 2) for p in range(-10, -10 + L)]
    zs = [(torch.randn(nk, E, generator=gen) + 0.5).to(BF16).to(dev) for _ in range(K)]
    sd = torch.logspace(-0.5, 1.5, V)
    mix = torch.randn(64, V, generator=gen)
    ys = [(zk[:, :64].float().cpu() @ mix + sd * torch.randn(nk, V, generator=gen)).to(dev) for zk in zs]
    half = (torch.arange(V) % 2 == 0).float()
    three = half * torch.tensor([0.5, 1.0, 2.0])[torch.arange(V) // 2 % 3]
    reps = min(args.reps, 3)
    for name, tw in (("unweighted", None), ("mask, D = 1", half), ("three levels, D = 3", three)):
        head = BrainHead(E, V, 1e-3, 1e-5, dev)
        head.set_target_weights(None if tw is None else tw.to(dev))
        head.ridge_stats_begin(folds=K, block=nk, weighted=True)
        s = head._ridge
        for k in range(K):
            if tw is None:
                check(lib.vlb_ridge_gram_accumulate(zs[k].data_ptr(), ys[k].data_ptr(), V, s["G"][0, k].data_ptr(), s["C"][0, k].data_ptr(),
                                                    s["sz"][0, k].data_ptr(), s["sy"][0, k].data_ptr(), nk, E, V, st), "gram")
                check(lib.vlb_ridge_sumsq_accumulate(ys[k].data_ptr(), V, s["syy"][0, k].data_ptr(), nk, V, st), "sumsq")
            else:
                kp = s["tw"][0].data_ptr()
                check(lib.vlb_ridge_gram_accumulate_masked(zs[k].data_ptr(), ys[k].data_ptr(), V, kp, s["G"][0, k].data_ptr(),
                                                           s["C"][0, k].data_ptr(), s["sz"][0, k].data_ptr(), s["sy"][0, k].data_ptr(), nk,
                                                           E, V, st), "gram masked")
                check(lib.vlb_ridge_sumsq_accumulate_masked(ys[k].data_ptr(), V, kp, s["syy"][0, k].data_ptr(), nk, V, st), "sumsq masked")
            s["n_fold"][0][k] += nk
            s["n"][0] += nk

        def fit():
            cv = head.ridge_cv(g_list)
            head.ridge_solve(cv["best_lambda"])
        t = [once(fit)[0] for _ in range(reps + 1)][1:]
        print(f"ridge_cv + ridge_solve E={E} V={V} K={K} L={L}, {name}: {statistics.median(t):.0f} ms wall (median of {reps})")
        head.ridge_stats_end()
        del head, s


if __name__ == "__main__":
    main()
