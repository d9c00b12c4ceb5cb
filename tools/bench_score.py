"""Timings of the held-out scoring kernels quoted in DESIGN §5.3.10 (one MI355X): the median of 20 hipEvent-timed launches
after warm-up, on seeded tensors.

  python tools/bench_score.py [out.json]

1. vlb_score_accumulate at B = 5, V = 65,536, H = 1, next to LogValAccuracyCallback.on_validation_batch_end (the torch path the
   sums replace) on the same tensors.
2. vlb_score_bootstrap at V = 65,536, nb = 157 (20,000 clips in blocks of 128), R = 1000, with the bytes it streams
   (R nb 5 8 V: every resample adds nb blocks of five fp64 sums per target) and the rate that implies; vlb_score_finish on the
   same slab for scale."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phantom_vlb_amd._lib import check, lib                         # noqa: E402
from phantom_vlb_amd.utils import LogValAccuracyCallback            # noqa: E402


def stream():
    return torch.cuda.current_stream().cuda_stream


def timed(fn, reps=20, warm=3):
    """(median, min, max) ms of ``reps`` launches, each between two events"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    assert torch.cuda.is_available(), "bench_score.py needs a GPU"
    dev = torch.device("cuda:0")
    out = {}
    B, V, nb = 5, 65536, 4
    g = torch.Generator(device="cpu").manual_seed(1)
    pred = torch.randn(B, V, generator=g).to(torch.bfloat16).float().to(dev)
    y = torch.randn(B, V, generator=g).to(torch.bfloat16).float().to(dev)
    sums = torch.zeros(nb, 5, V, dtype=torch.float64, device=dev)
    slot = torch.zeros(B, dtype=torch.int32, device=dev)
    out["accumulate_ms"] = timed(lambda: check(lib.vlb_score_accumulate(
        pred.data_ptr(), V, y.data_ptr(), V, slot.data_ptr(), None, sums.data_ptr(), B, V, nb, nb, stream()), "accumulate"))
    cb = LogValAccuracyCallback()
    cb.on_validation_epoch_start(None, None)
    outputs = {"brain_preds": pred, "brain_vals": y}
    out["callback_batch_end_ms"] = timed(lambda: cb.on_validation_batch_end(None, None, outputs, None, 0))
    print(json.dumps(out), flush=True)

    nb, R = 157, 1000
    slab = torch.randn(nb, 5, V, dtype=torch.float64, device=dev)
    slab[:, 2:4].abs_().add_(1.0).mul_(128.0)                      # second moments large enough for positive variances
    n_j = torch.full((nb,), 128.0, dtype=torch.float64, device=dev)
    draws = torch.from_numpy(np.random.RandomState(0).randint(0, nb, size=(R, nb)).astype(np.int32)).to(dev)
    res = torch.empty(3, V, dtype=torch.float64, device=dev)
    med = timed(lambda: check(lib.vlb_score_bootstrap(slab.data_ptr(), n_j.data_ptr(), nb, draws.data_ptr(), R, None,
                                                      res.data_ptr(), V, stream()), "bootstrap"), warm=2)
    streamed = R * nb * 5 * 8 * V
    out.update(bootstrap_ms=med, bootstrap_bytes=streamed, bootstrap_TB_per_s=streamed / (med[0] * 1e-3) / 1e12,
               bootstrap_finite=bool(torch.isfinite(res).all()))
    fin, avg = torch.empty(4, V, dtype=torch.float64, device=dev), torch.empty(3, dtype=torch.float64, device=dev)
    out["finish_ms"] = timed(lambda: check(lib.vlb_score_finish(slab.data_ptr(), n_j.data_ptr(), nb, None, fin.data_ptr(),
                                                                avg.data_ptr(), V, stream()), "finish"))
    print(json.dumps(out), flush=True)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        json.dump(out, open(sys.argv[1], "w"), indent=1)


if __name__ == "__main__":
    main()
