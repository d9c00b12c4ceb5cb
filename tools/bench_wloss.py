#!/usr/bin/env python
"""Head forward + backward with and without per-target loss weights on one GPU: B = 3, S = 2048, E = 4096,
V = 2048 and 65536, every objective.  The two heads share their inputs and alternate call by call (``--reps`` pairs, default
21, after 3 warm-up pairs); medians; wall = host clock around forward + backward ending in a synchronise, GPU = device events.

    python tools/bench_wloss.py [--reps 21]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phantom_vlb_amd.head import BrainHead           # noqa: E402


def once(head, hidden, wmask, y):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    head.forward(hidden, wmask, y)
    head.backward(need_dhidden=True)
    b.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, S, E = 3, 2048, 4096
    gen = torch.Generator().manual_seed(0)
    hidden = torch.randn(B * S, E, generator=gen).to(torch.bfloat16).to(dev)
    wmask = torch.rand(B, S, generator=gen).to(dev)
    for V in (2048, 65536):
        y = torch.randn(B, V, generator=gen).to(dev)
        tw = torch.where(torch.rand(V, generator=gen) < 0.25, torch.zeros(V), 0.25 + torch.rand(V, generator=gen)).to(dev)
        for loss in ("mse", "cosine", "pearson"):
            plain, weighted = BrainHead(E, V, 1e-3, 1e-5, dev, loss=loss), BrainHead(E, V, 1e-3, 1e-5, dev, loss=loss)
            weighted.set_target_weights(tw)
            t = {"plain": [], "weighted": []}
            for r in range(args.reps + 3):
                for name, head in (("plain", plain), ("weighted", weighted)):
                    res = once(head, hidden, wmask, y)
                    if r >= 3:
                        t[name].append(res)
            med = {k: (statistics.median(x[0] for x in v), statistics.median(x[1] for x in v)) for k, v in t.items()}
            print(f"head fwd+bwd B={B} S={S} E={E} V={V} {loss}: unweighted {med['plain'][0]:.3f} / {med['plain'][1]:.3f} ms, "
                  f"weighted {med['weighted'][0]:.3f} / {med['weighted'][1]:.3f} ms (wall / GPU, medians of {args.reps} alternating)",
                  flush=True)
            del plain, weighted


if __name__ == "__main__":
    main()
