"""Clip + AdamW with a range table (vlb_adamw_step_groups / _g16) against the same step without one, on the same
buffers.  Both entries of a pair launch instantiations of ONE kernel (csrc/adamw.hip), so the ratio is the price of the table:
its staging in LDS and the binary search per lane, on top of the same bytes and the same arithmetic.  (Before the kernels were
unified the ungrouped fp32 step was a separate 4-byte-lane kernel and the pair measured that difference too;
profiles/adamw_groups_kernels.txt keeps those numbers, profiles/adamw_unified_kernels.txt has today's against them.)

  python tools/bench_adamw_groups.py [repetitions >= 20]

* fp32 gradients: the 7B LoRA r=16 flat store (50.6 M elements, flat.FlatTrainables' layout with its padding) with the range
  table the README's example optimizer_groups gives it, against ONE vlb_adamw_step over the store;
* bf16 gradients: 268 M elements cut into 64 ranges over three groups, against ONE vlb_adamw_step_g16.
The two entries of a pair alternate in one process; every launch is timed on its own with device events; the medians over the
repetitions (after three warm-up rounds) and their ratio are printed.  30 B (fp32 g) / 28 B (bf16 g) move per element.
"""
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phantom_vlb_amd._lib import check, lib  # noqa: E402
from phantom_vlb_amd.flat import SEG_ALIGN  # noqa: E402
from phantom_vlb_amd.geometry import geometry_7b  # noqa: E402
from phantom_vlb_amd.lora import GROUPS  # noqa: E402
from phantom_vlb_amd.optim_groups import assign_groups, group_ranges, group_specs, normalize_optimizer_groups  # noqa: E402

BF = torch.bfloat16
dev = torch.device("cuda:0")
EXAMPLE = [{"params": ["layer_norm*", "*.bias"], "lr_scale": 10, "weight_decay": 0},
           {"params": ["ridge_layer.*", "layer_mix.weight"], "lr_scale": 10},
           {"params": ["*.lora_B.weight"], "lr_scale": 4}]


def lora7b_store(r=16):
    """flat.FlatTrainables' element order and padding for the 7B geometry: the head, then per layer and LoRA group the A
    matrices of its targets followed by their B matrices.  -> offsets, numel"""
    g = geometry_7b()
    inn = {"self_attn.q_proj": g.dim, "self_attn.k_proj": g.dim, "self_attn.v_proj": g.dim, "self_attn.o_proj": g.heads * g.head_dim,
           "mlp.gate_proj": g.dim, "mlp.up_proj": g.dim, "mlp.down_proj": g.ff}
    out = {"self_attn.q_proj": g.heads * g.head_dim, "self_attn.k_proj": g.kv_heads * g.head_dim, "self_attn.v_proj": g.kv_heads * g.head_dim,
           "self_attn.o_proj": g.dim, "mlp.gate_proj": g.ff, "mlp.up_proj": g.ff, "mlp.down_proj": g.dim}
    entries = [(n, g.dim, -1) for n in ("layer_norm1.weight", "layer_norm1.bias", "layer_norm2.weight", "layer_norm2.bias")]
    entries += [("ridge_layer.linear.weight", g.num_target * g.dim, -1), ("ridge_layer.linear.bias", g.num_target, -1)]
    for li in range(g.layers):
        for _, targets in GROUPS:
            entries += [(f"model.layers.{li}.{t}.lora_A.weight", r * inn[t], li) for t in targets]
            entries += [(f"model.layers.{li}.{t}.lora_B.weight", out[t] * r, li) for t in targets]
    offs, off = {}, 0
    for i, (n, k, seg) in enumerate(entries):
        offs[n] = (off, k)
        off += (k + 7) // 8 * 8
        if i + 1 == len(entries) or entries[i + 1][2] != seg:
            off = (off + SEG_ALIGN - 1) // SEG_ALIGN * SEG_ALIGN
    return offs, off


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def pair(label, n, gdtype, bounds, group_of, lrs, wds, reps):
    gen = torch.Generator(device=dev).manual_seed(0)
    mst = torch.randn(n, device=dev, generator=gen)
    grd = torch.randn(n, device=dev, generator=gen).to(gdtype)
    m1 = torch.zeros(n, device=dev)
    v1 = torch.zeros(n, device=dev)
    cp = torch.zeros(n, device=dev, dtype=BF)
    ss = torch.full((1,), 4.0, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    bf = gdtype == BF
    G = len(lrs)
    lr_arg, wd_arg = (ctypes.c_float * G)(*lrs), (ctypes.c_float * G)(*wds)
    bounds, group_of = bounds.to(dev), group_of.to(dev)
    parent_fn = lib.vlb_adamw_step_g16 if bf else lib.vlb_adamw_step
    groups_fn = lib.vlb_adamw_step_groups_g16 if bf else lib.vlb_adamw_step_groups

    def parent():
        check(parent_fn(mst.data_ptr(), cp.data_ptr(), grd.data_ptr(), m1.data_ptr(), v1.data_ptr(), n, lrs[0], 0.9, 0.999, 1e-8, wds[0],
                        1, ss.data_ptr(), 1.0, st), "parent")

    def grouped():
        check(groups_fn(mst.data_ptr(), cp.data_ptr(), grd.data_ptr(), m1.data_ptr(), v1.data_ptr(), n, bounds.data_ptr(),
                        group_of.data_ptr(), group_of.numel(), lr_arg, wd_arg, G, 0.9, 0.999, 1e-8, 1, ss.data_ptr(), 1.0, st), "grouped")

    for _ in range(3):
        parent()
        grouped()
    torch.cuda.synchronize()
    tp, tg = [], []
    for _ in range(reps):
        tp.append(timed(parent))
        tg.append(timed(grouped))
    mp_, mg = statistics.median(tp), statistics.median(tg)
    nbytes = n * (28 if bf else 30)
    print(f"{label}: n = {n / 1e6:.1f} M, {group_of.numel()} ranges, {G} groups, {reps} repetitions each, interleaved", flush=True)
    print(f"  {'vlb_adamw_step_g16' if bf else 'vlb_adamw_step':28s} median {mp_ * 1e3:9.1f} us  {nbytes / mp_ / 1e6:7.0f} GB/s")
    print(f"  {'vlb_adamw_step_groups_g16' if bf else 'vlb_adamw_step_groups':28s} median {mg * 1e3:9.1f} us  {nbytes / mg / 1e6:7.0f} GB/s")
    print(f"  grouped / parent = {mg / mp_:.3f}", flush=True)


def main():
    reps = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 25
    entries = normalize_optimizer_groups(EXAMPLE)
    specs = group_specs(entries, 1e-4, 1e-2)
    offs, numel = lora7b_store()
    assert numel == 50_561_280, numel
    bounds, group_of = group_ranges(offs, numel, assign_groups(list(offs), entries))
    pair("fp32 gradients, 7B LoRA r=16 store, example optimizer_groups", numel, torch.float32, bounds, group_of,
         [s["lr"] for s in specs], [s["weight_decay"] for s in specs], reps)
    n = 65536 * 4096
    cuts = torch.arange(65, dtype=torch.int64) * (n // 64)
    pair("bf16 gradients, 268 M elements", n, BF, cuts, (torch.arange(64) % 3).to(torch.int32), [1e-4, 1e-5, 4e-4], [1e-2, 1e-2, 0.0], reps)


if __name__ == "__main__":
    main()
