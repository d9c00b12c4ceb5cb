"""Shared by the bare-buffer clip+AdamW tests (test_gpu_adamw_groups.py, test_gpu_adamw_ema.py, test_gpu_adamw_bits.py,
test_cpu_adamw_bits.py) and by tools/record_adamw_bits.py.

Two things live here.  The helpers the first two files used to spell out twice (random states with guard elements, range
tables, rates).  And the RECORDED cases: inputs made by exact integer arithmetic only - the same bits on any machine and any
library version - and a runner that pushes them through the six public entry points, so that the recording tool and the test
that replays tests/golden/adamw_parent_bits.json cannot drift apart."""
import ctypes
import hashlib

import numpy as np
import torch

BF = torch.bfloat16
BETAS, EPS, MAX_NORM = (0.9, 0.999), 1e-8, 1.0
LR, WD = 1e-3, 1e-2
TAIL = 64               # guard elements behind every buffer


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ moved helpers
def _state(n, dev, seed, gdtype=torch.float32, ema=False):
    """p, m, v, g, the bf16 copy (and ema) of n elements plus TAIL guards, torch.randn in this order from one generator."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    r = lambda: torch.randn(n + TAIL, device=dev, generator=gen)            # noqa: E731
    st = {"p": r(), "m": r() * 0.1, "v": r().square() * 0.01, "g": r().to(gdtype), "pb": r().to(BF)}
    if ema:
        st["ema"] = r()
    return st


def _clone(st):
    return {k: t.clone() for k, t in st.items()}


def _random_bounds(n, n_ranges, seed):
    """n_ranges ranges of random multiple-of-8 lengths >= 8 that fill [0, n)."""
    gen = torch.Generator().manual_seed(seed)
    cuts = torch.randperm(n // 8 - 1, generator=gen)[:n_ranges - 1].add(1).sort().values * 8
    return [0] + cuts.tolist() + [n]


def _rates(G, tie_last_two=False):
    """G (lr, weight_decay) pairs: group 1 has weight_decay 0; ``tie_last_two``: with three or more, the last two are equal."""
    lrs = [1e-3 * (1 + 3 * k) for k in range(G)]
    wds = [1e-2 * (1 + k) for k in range(G)]
    if G >= 2:
        wds[1] = 0.0
    if tie_last_two and G >= 3:
        lrs[-1], wds[-1] = lrs[-2], wds[-2]
    return lrs, wds


def _table_args(bounds, group_of, lrs, wds):
    G = len(lrs)
    return bounds.data_ptr(), group_of.data_ptr(), group_of.numel(), (ctypes.c_float * G)(*lrs), (ctypes.c_float * G)(*wds), G


# ------------------------------------------------------------------------------------------------ recorded cases
ARRAYS = ("p", "m", "v", "g", "pb", "ema")          # array ids of the generator, in this order
OUTPUTS = {"p": "master", "m": "m", "v": "v", "pb": "bf16", "ema": "ema"}
_M32 = np.uint64(0xFFFFFFFF)


def _hash32(n, seed, array_id):
    """lowbias32 of (index * 0x9E3779B1 + key(seed, array)) for index 0 .. n - 1, in uint64 arithmetic masked to 32 bits."""
    key = np.uint64((seed * 0x85EBCA6B + array_id * 0xC2B2AE35 + 1) & 0xFFFFFFFF)
    x = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B1) + key) & _M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & _M32
    x ^= x >> np.uint64(16)
    return x


def _exact_f32(n, seed, array_id):
    """fp32 in [-2, 2) on a 2^-22 grid: the hash's top 24 bits minus 2^23 (exact in fp32) times a power of two."""
    k = (_hash32(n, seed, array_id) >> np.uint64(8)).astype(np.int64) - (1 << 23)
    return k.astype(np.float32) * np.float32(2.0 ** -22)


def _exact_bf16_bits(n, seed, array_id):
    """bf16 in [-2, 2) on a 2^-6 grid, as uint16 bit patterns: 8 significant bits, so the fp32 value's low half is zero."""
    k = (_hash32(n, seed, array_id) >> np.uint64(24)).astype(np.int64) - 128
    f = k.astype(np.float32) * np.float32(2.0 ** -6)
    bits = f.view(np.uint32)
    assert not (bits & np.uint32(0xFFFF)).any()
    return (bits >> np.uint32(16)).astype(np.uint16)


BLOCK_EDGES = ([0, 8, 8 * 1029, 8 * 1031], [0, 1, 0])            # bounds, group of every range
_SHAPES3 = (("n8", 8), ("n8x1031", 8 * 1031), ("n8x196613", 8 * (3 * 2 ** 16 + 5)))


def recorded_cases():
    """-> list of dicts: name, entry, n, seed; ``shift`` (every pointer advanced by one element), ``table``, ``decay``."""
    cases = []
    for entry in ("vlb_adamw_step", "vlb_adamw_step_g16"):
        cases += [dict(name=f"{entry}/{tag}", entry=entry, n=n) for tag, n in _SHAPES3]
    # vlb_adamw_step's contract beyond the vectorised path: any n, pointers aligned to their element only
    cases += [dict(name="vlb_adamw_step/n1", entry="vlb_adamw_step", n=1),
              dict(name="vlb_adamw_step/n8x129+3", entry="vlb_adamw_step", n=8 * 129 + 3),
              dict(name="vlb_adamw_step/n8x1031_shifted_one_element", entry="vlb_adamw_step", n=8 * 1031, shift=1)]
    for entry in ("vlb_adamw_step_groups", "vlb_adamw_step_groups_g16"):
        cases.append(dict(name=f"{entry}/block_edges", entry=entry, n=8 * 1031, table=BLOCK_EDGES))
    cases.append(dict(name="vlb_adamw_step_ema/n8x1031_d0.5", entry="vlb_adamw_step_ema", n=8 * 1031, decay=0.5))
    cases.append(dict(name="vlb_adamw_step_groups_ema/block_edges_d0.5", entry="vlb_adamw_step_groups_ema", n=8 * 1031, table=BLOCK_EDGES,
                      decay=0.5))
    for seed, c in enumerate(cases):
        c.update(seed=seed, shift=c.get("shift", 0), table=c.get("table"), decay=c.get("decay"))
    return cases


# (sum of squares for the clip, step, write the bf16 copy): clip active / inactive, bias correction at step 1 / 7
RECORDED_VARIANTS = [(ss, step, pb) for ss in (1e4, 1e-2) for step in (1, 7) for pb in (True, False)]


def variant_name(ss, step, with_pb):
    return f"sumsq{ss:g}_step{step}_{'bf16copy' if with_pb else 'nocopy'}"


def exact_inputs(case):
    """The case's input arrays (n + TAIL elements each) as numpy: fp32, and uint16 bit patterns for the bf16 ones.
    v is a float32 square times a float32 constant, both IEEE-exact operations in numpy."""
    n, seed = case["n"] + TAIL, case["seed"]
    g16 = case["entry"].endswith("_g16")
    x = _exact_f32(n, seed, 2)
    arrays = {"p": _exact_f32(n, seed, 0), "m": _exact_f32(n, seed, 1) * np.float32(0.125), "v": (x * x) * np.float32(0.01),
              "g": _exact_bf16_bits(n, seed, 3) if g16 else _exact_f32(n, seed, 3), "pb": _exact_bf16_bits(n, seed, 4)}
    if case["decay"] is not None:
        arrays["ema"] = _exact_f32(n, seed, 5)
    return arrays


def digest(arrays, keys=None):
    h = hashlib.sha256()
    for k in (keys or [a for a in ARRAYS if a in arrays]):
        h.update(np.ascontiguousarray(arrays[k]).tobytes())
    return h.hexdigest()


def _to_device(a, dev, shift):
    """numpy array -> device tensor whose data pointer is `shift` elements behind an allocation's start."""
    t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)
    buf = torch.empty(shift + t.numel(), dtype=t.dtype, device=dev)
    buf[shift:].copy_(t)
    out = buf[shift:]
    return out.view(BF) if a.dtype == np.uint16 else out


def run_recorded(case, variant, arrays, dev):
    """One call of the case's entry point on fresh device copies of ``arrays``.  -> {array: numpy} after the call (bf16 as
    uint16 bit patterns), every array n + TAIL long."""
    from phantom_vlb_amd._lib import check, lib
    ss, step, with_pb = variant
    n = case["n"]
    st = {k: _to_device(a, dev, case["shift"]) for k, a in arrays.items()}
    sumsq = torch.tensor([ss], dtype=torch.float32, device=dev)
    head = [st["p"].data_ptr(), st["pb"].data_ptr() if with_pb else None, st["g"].data_ptr(), st["m"].data_ptr(), st["v"].data_ptr()]
    if case["decay"] is not None:
        head.append(st["ema"].data_ptr())
    tail = [sumsq.data_ptr(), MAX_NORM] + ([case["decay"]] if case["decay"] is not None else []) + [_stream()]
    if case["table"] is not None:
        bounds = torch.tensor(case["table"][0], dtype=torch.int64, device=dev)
        group_of = torch.tensor(case["table"][1], dtype=torch.int32, device=dev)
        mid = [*_table_args(bounds, group_of, *_rates(2)), BETAS[0], BETAS[1], EPS, step]
    else:
        mid = [LR, BETAS[0], BETAS[1], EPS, WD, step]
    check(getattr(lib, case["entry"])(*head, n, *mid, *tail), case["entry"])
    torch.cuda.synchronize()
    return {k: (t.view(torch.int16).cpu().numpy().view(np.uint16) if t.dtype == BF else t.cpu().numpy()) for k, t in st.items()}
