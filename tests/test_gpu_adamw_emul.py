"""All six clip+AdamW entry points (csrc/adamw.hip) against the host restatement tests/adamw_emul.py - torch.equal on master,
both moments, the bf16 copy and ema, at shapes, steps, rates, clip states and values that tests/golden/adamw_parent_bits.json
does not hold - and, at the shapes that take the capped grid-stride loop past its first trip, the WHOLE array against float64
AdamW under the derived bars (adamw_emul.ref_step / bars).  The restatement reproduces the recorded GPU bits on the CPU
(test_cpu_adamw_emul.py), so neither side of a comparison here is the kernel itself.  Last: the two kernels that feed the clip,
vlb_grad_sumsq / vlb_grad_sumsq_bf16, against a true sum of squares.

Bare buffers with TAIL guard elements behind each; bf16 and float32 are compared as bit patterns, a NaN the restatement expects
must be a NaN; the guards and the gradient must come back unchanged."""
import numpy as np
import pytest
import torch

import adamw_emul as A
import ema_emul as E
import exact_ints
from adamw_cases import BF, TAIL, _clone, _random_bounds, _rates, _state, _stream, _table_args

pytestmark = pytest.mark.gpu
F32 = np.float32
HYPER = [(1e-3, .9, .999, 1e-8, 1e-2), (3.7e-5, .95, .98, 1e-6, 0.0), (1e-4, 0.0, .5, 1e-8, .1)]      # lr, b1, b2, eps, wd
STEPS = (1, 2, 3, 7, 100, 1000, 50000, 10 ** 6)
# entry -> (bf16 gradients, range table, ema)
ENTRIES = {"vlb_adamw_step": (False, False, False), "vlb_adamw_step_g16": (True, False, False),
           "vlb_adamw_step_groups": (False, True, False), "vlb_adamw_step_groups_g16": (True, True, False),
           "vlb_adamw_step_ema": (False, False, True), "vlb_adamw_step_groups_ema": (False, True, True)}
TABLES = {"ranges300_G3_lds": (300, 3), "ranges700_G5_global": (700, 5)}


# ------------------------------------------------------------------------------------------------ helpers
def _launch(entry, st, n, *, hp, step, sumsq, max_norm=1.0, with_pb=True, table=None, d=None):
    """One call.  ``sumsq``: a device float32[1] or None (null pointer).  ``table``: (bounds, group_of, lrs, wds), device int64 /
    int32 tensors and lists - replaces hp's lr / wd for the table entries."""
    from phantom_vlb_amd._lib import check, lib
    _, has_table, has_ema = ENTRIES[entry]
    lr, b1, b2, eps, wd = hp
    head = [st["p"].data_ptr(), st["pb"].data_ptr() if with_pb else None, st["g"].data_ptr(), st["m"].data_ptr(), st["v"].data_ptr()]
    if has_ema:
        head.append(st["ema"].data_ptr())
    mid = [*_table_args(*table), b1, b2, eps, step] if has_table else [lr, b1, b2, eps, wd, step]
    tail = [sumsq.data_ptr() if sumsq is not None else None, max_norm] + ([d] if has_ema else []) + [_stream()]
    check(getattr(lib, entry)(*head, n, *mid, *tail), entry)


def _np(t):
    """device tensor -> numpy; bf16 as uint16 bit patterns."""
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if t.dtype == BF else t.cpu().numpy()


def _f32(a):
    """float32 values of a host gradient array (bf16 bit patterns are widened, exactly)."""
    return (a.astype(np.uint32) << np.uint32(16)).view(F32) if a.dtype == np.uint16 else a


def _expect(h, *, g16, hp, step, ss, max_norm=1.0, group=None, rates=None, d=None):
    """The restatement on host arrays h = {p, m, v, g[, ema]} -> {p, m, v, pb (bit patterns)[, ema]}.  ``ss``: the float32 sumsq
    word's value or None; ``group`` / ``rates``: every element's group and (lrs, wds) for the table entries."""
    lr, b1, b2, eps, wd = hp
    if group is not None:
        p2, m2, v2, pb = A.emul_groups(h["p"], h["m"], h["v"], _f32(h["g"]), group, *rates, g16=g16, b1=b1, b2=b2, eps=eps, step=step,
                                       sumsq=ss, max_norm=max_norm)
    else:
        p2, m2, v2, pb = A.emul_step(h["p"], h["m"], h["v"], _f32(h["g"]), g16=g16,
                                     scalars=A.host_scalars(lr, b1, b2, eps, wd, step, ss, max_norm))
    out = {"p": p2, "m": m2, "v": v2, "pb": pb}
    if d is not None:
        out["ema"] = E.ema_step(h["ema"], p2, d)
    return out


def _same_bits(got, want, tag):
    """float32 arrays / uint16 bf16 patterns: NaN where a NaN is expected, the same bits everywhere else."""
    if want.dtype == np.uint16:
        nan_w, nan_g = A.bf16_is_nan(want), A.bf16_is_nan(got)
    else:
        assert got.dtype == want.dtype == F32
        nan_w, nan_g = np.isnan(want), np.isnan(got)
        got, want = got.view(np.uint32), want.view(np.uint32)
    assert np.array_equal(nan_g, nan_w), (tag, "NaN at", np.flatnonzero(nan_g != nan_w)[:8].tolist())
    bad = (got != want) & ~nan_w
    assert not bad.any(), (tag, int(bad.sum()), "first at", np.flatnonzero(bad)[:8].tolist())


def _run_and_check(dev, entry, st0, n, *, hp, step, ss, max_norm=1.0, with_pb=True, table=None, d=None, tag=()):
    """Launch on a copy of st0 and hold every array to the restatement.  ``ss``: float or None.  -> (kernel's arrays, expected)."""
    g16, has_table, has_ema = ENTRIES[entry]
    got = _preserving_clone(st0)
    sumsq = None if ss is None else torch.tensor([ss], dtype=torch.float32, device=dev)
    dtab = None
    if has_table:
        bounds, groups, lrs, wds = table
        dtab = (torch.tensor(bounds, dtype=torch.int64, device=dev), torch.tensor(groups, dtype=torch.int32, device=dev), lrs, wds)
    _launch(entry, got, n, hp=hp, step=step, sumsq=sumsq, max_norm=max_norm, with_pb=with_pb, table=dtab, d=d if has_ema else None)
    torch.cuda.synchronize()
    h0 = {k: _np(t) for k, t in st0.items()}
    hg = {k: _np(t) for k, t in got.items()}
    group = A.group_of_elements(table[0], table[1], np.arange(n)) if has_table else None
    exp = _expect({k: a[:n] for k, a in h0.items()}, g16=g16, hp=hp, step=step, ss=None if ss is None else float(F32(ss)), max_norm=max_norm,
                  group=group, rates=table[2:] if has_table else None, d=d if has_ema else None)
    tag = (entry, n, hp, step, ss, max_norm, with_pb, d) + tuple(tag)
    for k in hg:
        assert np.array_equal(hg[k][n:].view(np.uint8), h0[k][n:].view(np.uint8)), (tag, k, "wrote behind the end")
    assert np.array_equal(hg["g"].view(np.uint8), h0["g"].view(np.uint8)), (tag, "the gradient was written")
    for k in ("p", "m", "v") + (("ema",) if has_ema else ()):
        _same_bits(hg[k][:n], exp[k], tag + (k,))
    if with_pb:
        _same_bits(hg["pb"][:n], exp["pb"], tag + ("pb",))
    else:
        assert np.array_equal(hg["pb"], h0["pb"]), (tag, "bf16 copy written without its pointer")
    return hg, exp


def _preserving_clone(st):
    """_clone that keeps every array's offset from its allocation's start (a shifted view stays shifted)."""
    out = {}
    for k, t in st.items():
        off = t.storage_offset()
        buf = torch.empty(off + t.numel(), dtype=t.dtype, device=t.device)
        buf[off:].copy_(t)
        out[k] = buf[off:]
    return out


def _table(n, name):
    n_ranges, G = TABLES[name]
    n_ranges = min(n_ranges, n // 8)
    bounds = _random_bounds(n, n_ranges, 11 + G) if n_ranges > 1 else [0, n]
    assert bounds[0] == 0 and bounds[-1] == n and all(b % 8 == 0 for b in bounds) and len(bounds) == n_ranges + 1
    lrs, wds = _rates(G)
    assert G < 2 or wds[1] == 0.0
    return bounds, [r % G for r in range(n_ranges)], lrs, wds


# ------------------------------------------------------------------------------------------------ a) entry x path
@pytest.mark.parametrize("n", [8, 8 * 1031, 8 * 196613])
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_every_entry_equals_the_restatement(dev, entry, n):
    """Step 3 / 2 (no digest holds them), clip active / inactive, with / without the bf16 pointer; table entries with the LDS
    table (300 ranges, 3 groups) and the global one (700 ranges, 5 groups), group 1 with weight_decay 0."""
    g16, has_table, has_ema = ENTRIES[entry]
    st0 = _state(n, dev, seed=n % 1000 + 17, gdtype=BF if g16 else torch.float32, ema=has_ema)
    for name in (TABLES if has_table else [None]):
        table = _table(n, name) if has_table else None
        for ss, step, with_pb, d in ((1e4, 3, True, 0.999), (1e-2, 2, False, 0.5)):
            hg, _ = _run_and_check(dev, entry, st0, n, hp=HYPER[0], step=step, ss=ss, with_pb=with_pb, table=table, d=d, tag=(name,))
            assert not np.array_equal(hg["p"][:n], _np(st0["p"])[:n])


@pytest.mark.parametrize("case", ["n1", "n8x129+3", "n8x1031_shifted_one_element"])
def test_one_element_per_lane_path_equals_the_restatement(dev, case):
    """vlb_adamw_step alone serves any n and pointers aligned to their element only (W = 1)."""
    n, shift = {"n1": (1, 0), "n8x129+3": (8 * 129 + 3, 0), "n8x1031_shifted_one_element": (8 * 1031, 1)}[case]
    st0 = {k: t[shift:] for k, t in _state(n + shift, dev, seed=n % 1000 + 3).items()}
    assert all(t.numel() == n + TAIL for t in st0.values())
    if shift:
        assert st0["p"].data_ptr() % 16 == 4 and st0["pb"].data_ptr() % 8 == 2
    for ss, step, with_pb in ((1e4, 3, True), (1e-2, 2, False)):
        _run_and_check(dev, "vlb_adamw_step", st0, n, hp=HYPER[0], step=step, ss=ss, with_pb=with_pb)


# ------------------------------------------------------------------------------------------------ b) rates and steps
HP_ENTRIES = ("vlb_adamw_step", "vlb_adamw_step_g16", "vlb_adamw_step_groups_ema")
N_MID = 8 * 1031


def _mid_table(hp):
    """A three-range, two-group table around hp: group 0 is hp's own pair."""
    return [0, 8, 8 * 1029, N_MID], [0, 1, 0], [hp[0], 4 * hp[0]], [hp[4], 0.5 * hp[4]]


@pytest.mark.parametrize("hp", HYPER, ids=["hp0", "hp1_wd0", "hp2_b1_0"])
@pytest.mark.parametrize("entry", HP_ENTRIES)
def test_hyperparameters_and_steps_the_digests_do_not_hold(dev, entry, hp):
    g16, has_table, has_ema = ENTRIES[entry]
    st0 = _state(N_MID, dev, seed=29, gdtype=BF if g16 else torch.float32, ema=has_ema)
    for i, step in enumerate(STEPS):
        _run_and_check(dev, entry, st0, N_MID, hp=hp, step=step, ss=(1e4, 1e-2)[i % 2], with_pb=i % 3 != 2, table=_mid_table(hp), d=0.999)


@pytest.mark.parametrize("entry", HP_ENTRIES)
def test_lr_zero_and_a_scheduler_lr(dev, entry):
    g16, has_table, has_ema = ENTRIES[entry]
    st0 = _state(N_MID, dev, seed=31, gdtype=BF if g16 else torch.float32, ema=has_ema)
    # lr = 0: decay = fma(-0, wd, 1) = 1 and q = 0, so the masters come out as decay * p = p exactly while the moments move
    hp = (0.0,) + HYPER[0][1:]
    table = ([0, 8, 8 * 1029, N_MID], [0, 1, 0], [0.0, 0.0], [1e-2, 0.0])
    hg, exp = _run_and_check(dev, entry, st0, N_MID, hp=hp, step=5, ss=1e4, table=table, d=0.5)
    p0 = _np(st0["p"])[:N_MID]
    assert float(A.host_scalars(*hp, 5)["decay"]) == 1.0 and np.array_equal(hg["p"][:N_MID].view(np.uint32), p0.view(np.uint32))
    assert (hg["m"][:N_MID] != _np(st0["m"])[:N_MID]).mean() > 0.99 and (hg["v"][:N_MID] != _np(st0["v"])[:N_MID]).mean() > 0.99
    # the lr CosineAnnealingLR hands the optimiser at its 137th step of 1000
    w = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([w], lr=HYPER[0][0])
    sch = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=1000)
    for _ in range(137):
        opt.step(), sch.step()
    lr = opt.param_groups[0]["lr"]
    assert 0.9e-3 < lr < 1e-3 and float(F32(lr)) != lr
    hp = (lr,) + HYPER[0][1:]
    _run_and_check(dev, entry, st0, N_MID, hp=hp, step=138, ss=1e-2, table=_mid_table(hp), d=0.999)


# ------------------------------------------------------------------------------------------------ c) the clip's edges
@pytest.mark.parametrize("entry", ["vlb_adamw_step", "vlb_adamw_step_g16"])
def test_clip_edges(dev, entry):
    g16 = ENTRIES[entry][0]
    st0 = _state(N_MID, dev, seed=37, gdtype=BF if g16 else torch.float32)
    hp, n = HYPER[0], N_MID
    one = A.host_scalars(*hp, 3, 1.0, 1.0)["clip"]
    assert one < 1 and float(one) == float(F32(1) / (F32(1) + F32(1e-6)))           # the norm equals max_norm: still clipped
    unclipped = _run_and_check(dev, entry, st0, n, hp=hp, step=3, ss=None)[0]      # sumsq pointer null
    for ss, max_norm, clipped in ((1e4, 0.0, False), (1e4, -1.0, False), (0.0, 1.0, False), (1.0, 1.0, True), (1e4, 1.0, True)):
        hg, _ = _run_and_check(dev, entry, st0, n, hp=hp, step=3, ss=ss, max_norm=max_norm)
        assert np.array_equal(hg["m"], unclipped["m"]) == (not clipped), (ss, max_norm)
    # sumsq = +inf: clip = 0, a finite gradient contributes +-0 (m' = b1 m, v' = b2 v), an infinite one NaN in its own element only
    st = _clone(st0)
    st["g"][5] = float("inf")
    st["g"][n - 2] = float("-inf")
    hg, exp = _run_and_check(dev, entry, st, n, hp=hp, step=3, ss=float("inf"))
    assert float(A.host_scalars(*hp, 3, float("inf"), 1.0)["clip"]) == 0.0
    nan = np.zeros(n, bool)
    nan[[5, n - 2]] = True
    m0, v0 = _np(st0["m"])[:n], _np(st0["v"])[:n]
    for k in ("p", "m", "v"):
        assert np.array_equal(np.isnan(hg[k][:n]), nan), k
    assert A.bf16_is_nan(hg["pb"][:n]).tolist() == nan.tolist()
    assert np.array_equal(hg["m"][:n][~nan], (F32(hp[1]) * m0)[~nan]) and np.array_equal(hg["v"][:n][~nan], (F32(hp[2]) * v0)[~nan])


# ------------------------------------------------------------------------------------------------ d) special values
SPECIAL_ENTRIES = ("vlb_adamw_step", "vlb_adamw_step_g16", "vlb_adamw_step_ema")


@pytest.mark.parametrize("entry", SPECIAL_ENTRIES)
def test_special_values(dev, entry):
    g16, _, has_ema = ENTRIES[entry]
    n = 64
    st0 = _state(n, dev, seed=41, gdtype=BF if g16 else torch.float32, ema=has_ema)
    for i in (8, 9):                                     # g = m = v = 0 with p = +0 / -0 ...
        for k in "gmv":
            st0[k][i] = 0.0
    st0["p"][8], st0["p"][9] = 0.0, -0.0
    for k in "gmv":                                      # ... and with an ordinary p: q = 0, p' = decay * p
        st0[k][10] = 0.0
    st0["v"][16] = 0.0                                   # v = 0 with g != 0
    st0["p"][17], st0["p"][18] = 0.0, -0.0               # p = +-0 with an ordinary update
    st0["g"][24], st0["g"][25] = 1e30, -1e30             # huge |g|, clip off: gi^2 overflows, v' = inf, q = 0
    st0["g"][5] = float("nan")                           # one NaN gradient: 4, 6 and 7 share its 4-vector
    hp = HYPER[0]
    hg, exp = _run_and_check(dev, entry, st0, n, hp=hp, step=3, ss=None, d=0.5)
    p0 = _np(st0["p"])[:n]
    decay = A.host_scalars(*hp, 3)["decay"]
    assert hg["p"][8] == 0 and not np.signbit(hg["p"][8]) and hg["p"][9] == 0 and np.signbit(hg["p"][9])
    assert hg["p"][10] == decay * p0[10] and hg["m"][10] == 0 and hg["v"][10] == 0
    assert np.isinf(hg["v"][24]) and np.isinf(hg["v"][25]) and hg["p"][24] == decay * p0[24] and hg["p"][25] == decay * p0[25]
    nan = np.arange(n) == 5
    for k in ("p", "m", "v") + (("ema",) if has_ema else ()):
        assert np.array_equal(np.isnan(hg[k][:n]), nan), k
    assert np.array_equal(A.bf16_is_nan(hg["pb"][:n]), nan)
    assert np.isfinite(exp["p"][[4, 6, 7]]).all()


@pytest.mark.parametrize("entry", SPECIAL_ENTRIES)
def test_denormal_operands(dev, entry):
    """g between 1e-23 and 1e-19 (ob2 * gi^2 runs from below the smallest subnormal up through the subnormal range), subnormal v
    and, in a quarter of the elements, subnormal m.  Bit-equal to the restatement: the library is built without a
    flush-to-zero option, the kernels' code objects preserve float32 denormals (float_denorm_mode_32 = 3, no mode switch
    inside), the division goes through v_div_scale / v_div_fixup and the square root scales an argument below 2^-96 by 2^32
    before v_sqrt_f32 and corrects the last bit by two fused residuals - all of which keep subnormals IEEE."""
    g16, _, has_ema = ENTRIES[entry]
    n = 8 * 129
    st0 = _state(n, dev, seed=43, gdtype=BF if g16 else torch.float32, ema=has_ema)
    gen = torch.Generator(device=dev).manual_seed(44)
    r = lambda: torch.randn(n + TAIL, device=dev, generator=gen)                    # noqa: E731
    st0["g"] = (r() * 10 ** (torch.rand(n + TAIL, device=dev, generator=gen) * 4 - 23)).to(st0["g"].dtype)
    st0["v"] = r().abs() * 1e-40
    st0["m"] = torch.where(torch.arange(n + TAIL, device=dev) % 4 == 0, r() * 1e-40, r() * 1e-23)
    tiny = 2.0 ** -126
    assert bool(((st0["v"] > 0) & (st0["v"] < tiny)).float().mean() > 0.9) and bool(((st0["m"] != 0) & (st0["m"].abs() < tiny)).any())
    for ss in (None, 1e4):
        hg, exp = _run_and_check(dev, entry, st0, n, hp=HYPER[0], step=3, ss=ss, d=0.5)
        sub = (exp["v"] > 0) & (exp["v"] < tiny)
        assert sub.mean() > 0.5 and (exp["v"][sub] != _np(st0["v"])[:n][sub]).any()


# ------------------------------------------------------------------------------------------------ e) the capped loop
# W = 4: lanes = n / 4, nb = min(ceil(lanes / 512), 32768) workgroups, one trip = 2 chunks of 256 * nb lanes; the cap binds
# from n = 2^26.  W = 1: from n = 2^24.
SHAPE_A = 8 * (2 ** 23 + 2 ** 10 + 3)          # the second trip's first chunk only, ragged
SHAPE_B = 2 ** 26 + 2 ** 25 + 8 * 1031         # the second trip's first chunk full, its second chunk ragged
SHAPE_C = 2 ** 27 + 40                         # a third trip begins after a full second one
SHAPE_W1 = 2 ** 24 + 2 ** 23 + 3               # W = 1 (n % 8 = 3): second trip, second chunk ragged
LOOP_CASES = [("B", e) for e in ENTRIES] + [(s, e) for s in ("A", "C") for e in ("vlb_adamw_step", "vlb_adamw_step_g16")] + \
             [("W1", "vlb_adamw_step")]
_WORST = {}


def _subsample(n, chunk, seed):
    """First and last 4096 elements, 4096 on both sides of every multiple of ``chunk``, 2^20 seeded random indices."""
    parts = [np.arange(min(4096, n)), np.arange(max(0, n - 4096), n)]
    for b in range(chunk, n, chunk):
        parts.append(np.arange(b - 4096, min(b + 4096, n)))
    parts.append(np.random.default_rng(seed).integers(0, n, 2 ** 20))
    return np.unique(np.concatenate(parts))


@pytest.mark.parametrize("shape,entry", LOOP_CASES, ids=[f"{s}-{e}" for s, e in LOOP_CASES])
def test_capped_grid_stride_loop(dev, shape, entry):
    """Every element of m', v', p' on the device against float64 AdamW under the derived bars (one .item()), ema under three
    roundings, the bf16 copy as the rounding of the kernel's own master; and a subsample - both ends, both sides of every chunk
    boundary, 2^20 random elements - on the host, bit for bit against the restatement (the update is element-wise)."""
    n = {"A": SHAPE_A, "B": SHAPE_B, "C": SHAPE_C, "W1": SHAPE_W1}[shape]
    g16, has_table, has_ema = ENTRIES[entry]
    W = 1 if shape == "W1" else 4
    lanes = n // W
    nb = min((lanes + 511) // 512, 32768)
    chunk = 256 * nb * W
    assert nb == 32768 and n > 2 * chunk and (n % 8 == 0) == (W == 4)
    trips, rest = divmod(n, 2 * chunk)
    assert {"A": (1, True), "B": (1, False), "C": (2, True), "W1": (1, False)}[shape] == (trips, 0 < rest < chunk)
    hp, step, ss, d = HYPER[0], 3, 1e4, 0.999
    st0 = _state(n, dev, seed=n % 1000 + 5, gdtype=BF if g16 else torch.float32, ema=has_ema)
    got = _clone(st0)
    sumsq = torch.tensor([ss], dtype=torch.float32, device=dev)
    table = dtab = None
    if has_table:
        n_ranges, G = (300, 3) if entry == "vlb_adamw_step_groups" else (700, 5) if g16 else (12, 3)
        lrs, wds = _rates(G)
        table = (_random_bounds(n, n_ranges, 5), [r % G for r in range(n_ranges)], lrs, wds)
        dtab = (torch.tensor(table[0], dtype=torch.int64, device=dev), torch.tensor(table[1], dtype=torch.int32, device=dev), lrs, wds)
        lr_dev = torch.tensor([float(F32(x)) for x in lrs], dtype=torch.float64, device=dev)
        wd_dev = torch.tensor([float(F32(x)) for x in wds], dtype=torch.float64, device=dev)
    _launch(entry, got, n, hp=hp, step=step, sumsq=sumsq, with_pb=True, table=dtab, d=d if has_ema else None)
    torch.cuda.synchronize()

    # the whole array, on the device
    worst = torch.zeros((), dtype=torch.float64, device=dev)
    outside = torch.zeros((), dtype=torch.int64, device=dev)
    d32, omd = (float(x) for x in E.decay_pair(d))
    for s in range(0, n, 2 ** 24):
        e = min(n, s + 2 ** 24)
        lr, wd = hp[0], hp[4]
        if has_table:
            grp = dtab[1][torch.searchsorted(dtab[0], torch.arange(s, e, device=dev), right=True) - 1].long()
            lr, wd = lr_dev[grp], wd_dev[grp]
        R = A.ref_step(*(st0[k][s:e] for k in "pmvg"), lr=lr, b1=hp[1], b2=hp[2], eps=hp[3], wd=wd, step=step, sumsq=ss, max_norm=1.0)
        w, o = A.worst_ratio(tuple(got[k][s:e] for k in "pmv"), R, A.bars(R))
        worst, outside = torch.maximum(worst, w), outside + o
        outside += (got["pb"][s:e] != got["p"][s:e].to(BF)).sum()
        if has_ema:
            ref = d32 * st0["ema"][s:e].double() + omd * got["p"][s:e].double()
            bar = 3 * A.U * torch.maximum(st0["ema"][s:e].abs(), got["p"][s:e].abs()).double()
            outside += (~((got["ema"][s:e].double() - ref).abs() <= bar)).sum()
        del R, w, o
    for k in got:
        outside += (got[k][n:].view(torch.uint8) != st0[k][n:].view(torch.uint8)).sum()
    outside += (got["g"].view(torch.uint8) != st0["g"].view(torch.uint8)).sum()
    worst, outside = float(worst), int(outside)
    _WORST[(shape, entry)] = worst
    print(f"capped loop {shape} {entry}: n = {n}, worst |kernel - fp64| / bar over the whole array = {worst:.3f}, outside = {outside}")
    assert outside == 0 and worst <= 1.0, (shape, entry, worst, outside)

    # the subsample, on the host
    idx = _subsample(n, chunk, seed=n % 97)
    assert idx[0] == 0 and idx[-1] == n - 1 and np.isin([chunk - 1, chunk, 2 * chunk - 1, 2 * chunk], idx).all() and idx.size > 2 ** 19
    didx = torch.from_numpy(idx).to(dev)
    h0 = {k: _np(t[didx]) for k, t in st0.items()}
    hg = {k: _np(t[didx]) for k, t in got.items()}
    del st0, got
    exp = _expect(h0, g16=g16, hp=hp, step=step, ss=float(F32(ss)), group=A.group_of_elements(table[0], table[1], idx) if has_table else None,
                  rates=table[2:] if has_table else None, d=d if has_ema else None)
    for k in ("p", "m", "v", "pb") + (("ema",) if has_ema else ()):
        _same_bits(hg[k], exp[k], (shape, entry, k))


# ------------------------------------------------------------------------------------------------ f) the clip's norm
SUMSQ_N = [1, 7, 1024, 1025, 8 * 1031, 2 ** 20, 2 ** 20 + 8, 3 * 2 ** 20 + 8 * 5]


def _sumsq(g, prior, dev):
    """sumsq[0] after the call, as a float32 numpy scalar; the kernels ADD into it."""
    from phantom_vlb_amd._lib import check, lib
    bf = g.dtype == BF
    out = torch.full((1 + TAIL,), float(prior), dtype=torch.float32, device=dev)
    ws = torch.zeros(lib.vlb_sumsq_ws_floats() + TAIL, dtype=torch.float32, device=dev)
    fn = lib.vlb_grad_sumsq_bf16 if bf else lib.vlb_grad_sumsq
    check(fn(g.data_ptr(), g.numel(), out.data_ptr(), ws.data_ptr(), _stream()), "vlb_grad_sumsq")
    torch.cuda.synchronize()
    assert bool((out[1:] == float(prior)).all()) and bool((ws[lib.vlb_sumsq_ws_floats():] == 0).all())
    return out[:1].cpu().numpy()[0]


def _chain(n, bf):
    """Longest per-thread chain of additions: the fp32 kernel's thread sums ceil(n / (256 nb)) squares with nb = min(ceil(n / 1024),
    1024); the bf16 kernel's eight per trip over n / 8 vectors with nb = min(ceil(n8 / 256), 1024)."""
    if bf:
        n8 = n // 8
        nb = min((n8 + 255) // 256, 1024)
        return 8 * -(-n8 // (256 * nb))
    nb = min((n + 1023) // 1024, 1024)
    return -(-n // (256 * nb))


@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
def test_grad_sumsq_is_exact_on_ternary_gradients(dev, bf):
    """Gradients in {-1, 0, +1}: every partial sum is an integer below 2^24, exact in any order and under any contraction, so
    the result is the number of non-zeros plus what sumsq[0] held - as a float32 bit pattern.  n = 2^20, 2^20 + 8 and
    3 * 2^20 + 40 reach the 1024-workgroup cap and the second and third trip of the per-thread loop."""
    sizes = [n for n in SUMSQ_N if not bf or n % 8 == 0]
    assert len(sizes) == (5 if bf else 8)
    for n in sizes:
        g = exact_ints.ternary(n, seed=n % 1000 + 1, device=dev, dtype=BF if bf else torch.float32)
        count = int((g != 0).sum())
        assert count < 2 ** 24 - 5 and (n < 8 or 0 < count < n)
        for prior in (0, 5):
            got = _sumsq(g, prior, dev)
            assert got.dtype == F32 and got.view(np.uint32) == F32(count + prior).view(np.uint32), (n, prior, float(got), count + prior)
    # one element less in the reference (or in the gradient) must show: the check can see a single dropped element
    nz = int(torch.nonzero(g != 0)[len(g) // 3])
    assert float(got) != float(count - 1 + 5)
    g[nz] = 0
    assert float(_sumsq(g, 5, dev)) == float(count - 1 + 5)
    g[nz] = 2                                                      # 2^2: one element's weight, not its presence
    assert float(_sumsq(g, 0, dev)) == float(count - 1 + 4)


@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
def test_grad_sumsq_on_gaussian_gradients(dev, bf):
    """Against the float64 sum of the squares of the same float32 / bf16 values, under (L + 26) u S / (1 - (L + 26) u), L the
    longest per-thread chain (_chain).  All terms are positive, so the relative error of the total is at most the number of
    roundings on the longest path of one square to the result: its product (1; 0 where the compiler contracts it into the
    addition), the thread's chain (<= L additions), the wave's xor butterfly (6), the fold of the four waves' sums (4), then in the
    final kernel the thread's chain over at most 1024 / 256 partials (4), its butterfly (6), its fold (4) and the addition into
    sumsq[0] (1): L + 26 roundings of at most u each."""
    worst = 0.0
    for n in [n for n in SUMSQ_N if not bf or n % 8 == 0]:
        gen = torch.Generator(device=dev).manual_seed(n % 1000 + 2)
        g = torch.randn(n, device=dev, generator=gen).to(BF if bf else torch.float32)
        true = float(g.double().square().sum())
        got = float(_sumsq(g, 0, dev))
        k = (_chain(n, bf) + 26) * A.U
        bar = k / (1 - k) * true
        assert abs(got - true) <= bar, (n, got, true, abs(got - true) / bar)
        worst = max(worst, abs(got - true) / bar)
    print(f"grad_sumsq {'bf16' if bf else 'fp32'}: worst |kernel - fp64| / bar = {worst:.3f}")
