"""Cost of per-subject ridge heads (``subjects``): the head's tail, forward + backward, at E = 4096, B = 3.

    python tools/bench_multi_subject.py [out.txt]        # default profiles/multi_subject_head.txt

For V = 2048 and V = 65,536: the ungrouped tail (vlb_head_fwd_cached + vlb_head_bwd_cached, the parent's kernels: the
yardstick), the same single head through the grouped entries (G = 1: the new code's overhead), and G = 2 and G = 6 heads
with the three clips spread over the heads.  HIP events around 24 forward + backward pairs after 8 untimed ones, the best of
three such runs (tools/bench_hbm_kernels.py's style).  Bytes are what the tail must move per head, times G:
W bf16 read three times (forward, ridge_bwd_w, dz) and dW fp32 written once = 10 bytes per weight; the [B,E] / [B,V]
buffers are left out (< 1 %).  The same buffers are used every iteration: at V = 2048 one head's W (16 MB) stays in the
last-level cache between its three reads, as in profiles/r04_hbm_bound_kernels.txt's head rows."""
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

E, B = 4096, 3
PEAK_GBS = 8000.0


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


def make_head(dev, V, G, grouped):
    """A head with random bf16-valued parameters and a 3-row feature cache; -> fn() running one forward + backward of the tail"""
    from phantom_vlb_amd._lib import lib
    from phantom_vlb_amd.feature_cache import FeatureCache
    from phantom_vlb_amd.head import BrainHead
    names = [f"sub-{g + 1:02d}" for g in range(G)]
    # G = 1 through the grouped entries: a plain head switched to them by hand (BrainHead(subjects=...) itself needs two)
    gen = torch.Generator(device=dev).manual_seed(V + G)
    wshape = (G, V, E) if G > 1 else (V, E)
    sd = {"layer_norm1.weight": torch.ones(E, device=dev), "layer_norm1.bias": torch.zeros(E, device=dev),
          "layer_norm2.weight": torch.ones(E, device=dev), "layer_norm2.bias": torch.zeros(E, device=dev),
          "ridge_layer.linear.weight": (torch.rand(*wshape, device=dev, generator=gen) * 2 - 1) / 64,       # nn.Linear's bound, 1/sqrt(E)
          "ridge_layer.linear.bias": (torch.rand(*wshape[:-1], device=dev, generator=gen) * 2 - 1) / 64}
    head = BrainHead(E, V, 1e-3, 1e-5, dev, sd=sd, subjects=names if G > 1 else None)
    del sd
    if grouped and G == 1:
        head.G = 1
    cache = FeatureCache("train", B, E, dev)
    cache._alloc()
    cache.pooled.copy_(torch.randn(B, E, device=dev, generator=gen))
    cache.sumw.fill_(1.0)
    cache.valid[:] = True
    y = torch.randn(B, V, device=dev, generator=gen)
    idx = torch.arange(B)
    subject = [b % G for b in range(B)]
    head._buffers(B, 1)
    if grouped and G == 1:
        head.gws = torch.empty(lib.vlb_head_grouped_ws_floats(B, E, V, 1), dtype=torch.float32, device=dev)
        rows = torch.arange(B, dtype=torch.int32, device=dev)
        group = torch.zeros(B, dtype=torch.int32, device=dev)

        def fn():
            head._tail(cache.pooled, cache.sumw, rows, B, y, None, group)      # a group: the grouped entries, with G = 1
            head._backward_tail(1.0, 1.0)
    elif grouped:
        def fn():
            head.forward_cached(cache, idx, y, None, subject=subject)
            head.backward_cached()
    else:
        def fn():
            head.forward_cached(cache, idx, y, None)
            head.backward_cached()
    return head, fn


def main(out_path):
    dev = torch.device("cuda:0")
    lines = [f"head tail forward + backward, E = {E}, B = {B}: us per pair, GB/s against 10 bytes per weight (W read x3, dW fp32 written), x G",
             f"{'variant':40s} {'MB':>9s} {'us':>10s} {'GB/s':>8s} {'of 8 TB/s':>10s} {'vs':>28s}"]
    for V in (2048, 65536):
        base = {}
        for name, G, grouped in (("ungrouped (parent's kernels)", 1, False), ("G=1 through the grouped entries", 1, True),
                                 ("G=2", 2, True), ("G=6", 6, True)):
            head, fn = make_head(dev, V, G, grouped)
            ms = min(timeit(fn) for _ in range(3))
            nbytes = 10.0 * G * V * E
            note = ""
            if grouped and G == 1:
                note = f"{(ms / base['ungrouped'] - 1) * 100:+.1f}% vs ungrouped"
            elif grouped:
                note = f"{ms / (G * base['g1']):.2f} x (G x the G=1 time)"
            base["g1" if grouped and G == 1 else "ungrouped" if not grouped else f"g{G}"] = ms
            lines.append(f"V={V:<6d} {name:31s} {nbytes / 1e6:9.1f} {ms * 1e3:10.1f} {nbytes / ms / 1e6:8.0f} "
                         f"{nbytes / ms / 1e6 / PEAK_GBS * 100:9.1f}% {note:>28s}")
            print(lines[-1], flush=True)
            del head, fn
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    warnings.simplefilter("ignore")
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "multi_subject_head.txt"))
