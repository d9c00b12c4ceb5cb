#!/usr/bin/env python
"""Times of the per-target l2_lambda machinery on one GPU: vlb_ridge_cv_select, vlb_head_l2_rows_fwd / _bwd and
the whole per-target fit (ridge_cv(per_target=True) + ridge_solve_rows) beside ridge_cv + ridge_solve, on synthetic sums.
Medians of ``--reps`` (default 9); wall = host clock around the call ending in a synchronise, GPU = device events.

    python tools/bench_ridge_rows.py [--reps 9] [--skip-fit]
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

F64, F32, BF16, I32 = torch.float64, torch.float32, torch.bfloat16, torch.int32


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    wall, gpu = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        gpu.append(a.elapsed_time(b))
    return statistics.median(wall), statistics.median(gpu)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--skip-fit", action="store_true")
    args = ap.parse_args()
    dev = "cuda"
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator().manual_seed(0)

    K, L, V = 5, 10, 1000
    table = torch.rand(K, L, V, generator=gen, dtype=F64).to(dev)
    grid = torch.tensor([10.0 ** (p / 2) for p in range(-12, -12 + L)], dtype=F64, device=dev)
    ok = torch.ones(L, dtype=I32, device=dev)
    rmean, choice, rbest = torch.empty(L, V, dtype=F64, device=dev), torch.empty(V, dtype=I32, device=dev), torch.empty(V, dtype=F64, device=dev)
    w, g = timed(lambda: check(lib.vlb_ridge_cv_select(table.data_ptr(), grid.data_ptr(), ok.data_ptr(), rmean.data_ptr(), choice.data_ptr(),
                                                       rbest.data_ptr(), K, L, V, st), "vlb_ridge_cv_select"), args.reps)
    print(f"vlb_ridge_cv_select K={K} L={L} V={V}: {w:.3f} / {g:.3f} ms (wall / GPU)")

    for R, E in ((1000, 4096), (65536, 4096)):
        W = (torch.randn(R, E, generator=gen) / 64).to(BF16).to(dev)
        lam = (10.0 ** (torch.rand(R, generator=gen) * 4 - 4)).float().to(dev)
        d = torch.zeros(R, E, dtype=F32, device=dev)
        ws = torch.empty(lib.vlb_head_l2_rows_ws_doubles(R), dtype=F64, device=dev)
        terms = torch.zeros(3, dtype=F32, device=dev)
        w, g = timed(lambda: check(lib.vlb_head_l2_rows_fwd(W.data_ptr(), lam.data_ptr(), ws.data_ptr(), terms.data_ptr(), R, E, st),
                                   "vlb_head_l2_rows_fwd"), args.reps)
        mb = R * E * 2 / 1e6
        print(f"vlb_head_l2_rows_fwd R={R} E={E} ({mb:.0f} MB of W): {w:.3f} / {g:.3f} ms, {mb / g / 1e3:.2f} TB/s")
        w, g = timed(lambda: check(lib.vlb_head_l2_rows_bwd(W.data_ptr(), lam.data_ptr(), d.data_ptr(), R, E, 2.0, st),
                                   "vlb_head_l2_rows_bwd"), args.reps)
        print(f"vlb_head_l2_rows_bwd R={R} E={E} ({5 * mb:.0f} MB moved): {w:.3f} / {g:.3f} ms, {5 * mb / g / 1e3:.2f} TB/s")
        del W, lam, d
    if args.skip_fit:
        return

    # the whole fit on synthetic fold sums: E = 4096, V = 1000, K = 5, L = 10, n_k = 640
    E, V, K, L, nk = 4096, 1000, 5, 10, 640
    head = BrainHead(E, V, 1e-3, 1e-5, dev)
    head.ridge_stats_begin(folds=K, block=nk)
    s = head._ridge
    for k in range(K):
        z = (torch.randn(nk, E, generator=gen) + 0.5).to(BF16).to(dev)
        sd = torch.logspace(-0.5, 1.5, V)
        y = (z[:, :64].float().cpu() @ torch.randn(64, V, generator=gen) + sd * torch.randn(nk, V, generator=gen)).to(dev)
        check(lib.vlb_ridge_gram_accumulate(z.data_ptr(), y.data_ptr(), V, s["G"][0, k].data_ptr(), s["C"][0, k].data_ptr(),
                                            s["sz"][0, k].data_ptr(), s["sy"][0, k].data_ptr(), nk, E, V, st), "gram")
        check(lib.vlb_ridge_sumsq_accumulate(y.data_ptr(), V, s["syy"][0, k].data_ptr(), nk, V, st), "sumsq")
        s["n_fold"][0][k] += nk
        s["n"][0] += nk
    g_list = [10.0 ** (p / 2) for p in range(-10, -10 + L)]

    def global_fit():
        cv = head.ridge_cv(g_list)
        head.ridge_solve(cv["best_lambda"])

    def rows_fit():
        cv = head.ridge_cv(g_list, per_target=True)
        out = head.ridge_solve_rows(cv["choice"], g_list)
        rows_fit.counts = out[0]["lambda_counts"]
    reps = min(args.reps, 3)
    w, g = timed(global_fit, reps)
    print(f"ridge_cv + ridge_solve E={E} V={V} K={K} L={L}: {w:.0f} ms wall (median of {reps})")
    w, g = timed(rows_fit, reps)
    used = sum(1 for c in rows_fit.counts if c)
    print(f"ridge_cv(per_target=True) + ridge_solve_rows: {w:.0f} ms wall (median of {reps}); {used} of {L} grid points in use, counts "
          f"{rows_fit.counts}")


if __name__ == "__main__":
    main()
