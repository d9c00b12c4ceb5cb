"""tests/adamw_emul.py without a GPU: the float32 restatement of the clip+AdamW step against bits a GPU produced
(tests/golden/adamw_parent_bits.json), the float64 reference against torch.optim.AdamW, and the derived bars between the two -
which must contain the restatement everywhere on the grid and must reject every wrong optimiser listed below.
test_gpu_adamw_emul.py then holds the kernels to the restatement bit for bit."""
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import adamw_cases as C
import adamw_emul as A
import ema_emul as E

F32 = np.float32
U = A.U
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adamw_parent_bits.json")
HYPER = [(1e-3, .9, .999, 1e-8, 1e-2), (3.7e-5, .95, .98, 1e-6, 0.0), (1e-4, 0.0, .5, 1e-8, .1)]      # lr, b1, b2, eps, wd
STEPS = (1, 2, 3, 7, 100, 1000, 50000, 10 ** 6)
CLIPS = {"active": 1e4, "inactive": 1e-2, "absent": None}                                              # sumsq; max_norm = 1
N = 4096


# ------------------------------------------------------------------------------------------------ fma32
def _round_f32(x: Fraction) -> float:
    """x rounded ONCE to float32 (nearest, ties to even; subnormals; overflow to inf), in rational arithmetic."""
    if x == 0:
        return 0.0
    sign, x = (-1.0 if x < 0 else 1.0), abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    assert Fraction(2) ** e <= x < Fraction(2) ** (e + 1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    k = x / quantum
    n = k.numerator // k.denominator
    rem = k - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    val = n * quantum
    return sign * (math.inf if val >= Fraction(2) ** 128 else float(val))


def _operands(rng, n):
    mant = lambda: rng.integers(2 ** 23, 2 ** 24, n).astype(np.float64) * rng.choice([-1.0, 1.0], n)        # noqa: E731
    a = (mant() * 2.0 ** rng.integers(-60, 20, n)).astype(F32)
    b = (mant() * 2.0 ** rng.integers(-60, 20, n)).astype(F32)
    c = (mant() * 2.0 ** rng.integers(-60, 20, n)).astype(F32)
    k = n // 4
    with np.errstate(all="ignore"):
        c[:k] = -(a[:k] * b[:k])                                     # cancellation: the result IS the product's rounding error
        c[k:2 * k] = (a[k:2 * k] * b[k:2 * k]) * F32(2.0 ** 24)      # the product sits at the sum's rounding position
        a[2 * k:3 * k] = (mant()[:k] * 2.0 ** -100).astype(F32)      # subnormal results (and a subnormal addend)
        b[2 * k:3 * k] = (mant()[:k] * 2.0 ** rng.integers(-84, -78, k)).astype(F32)
        c[2 * k:3 * k] = (mant()[:k] * 2.0 ** -160).astype(F32)
    return a, b, c


def test_fma32_is_an_exactly_rounded_fma():
    a, b, c = _operands(np.random.default_rng(0), 4000)
    got = A.fma32(a, b, c)
    assert got.dtype == F32
    want = np.array([_round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)], dtype=np.float64)
    assert np.isfinite(want).sum() > 3500 and (np.abs(want[np.isfinite(want)]) < 2.0 ** -126).sum() > 300
    assert np.array_equal(got.astype(np.float64), want)
    with np.errstate(all="ignore"):
        separate = (a * b + c).astype(np.float64)
    assert (separate != want).sum() > 500                            # the operands can tell an fma from a product and a sum


def test_fma32_on_double_rounding_ties():
    """a * b + c whose float64 sum lands EXACTLY on a float32 tie while the exact value lies 2^-63 to one side of it: rounding
    the float64 sum to float32 goes to the even neighbour, the fma must go to the near one.  Both sides, both signs."""
    x, y, c = F32(2.0 ** -23 * (1 + 2.0 ** -20)), F32(1 - 2.0 ** -20), F32(2 + 2.0 ** -22)
    cases = [(x, y, c, c),            # 2 + 2^-22 + 2^-23 - 2^-63: below the tie, the odd neighbour below is right
             (-x, y, c, c),           # 2 + 2^-23 + 2^-63: above the tie, the odd neighbour above is right
             (-x, y, -c, -c), (x, y, -c, -c)]
    for a, b, cc, want in cases:
        exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(cc))
        s64 = float(a) * float(b) + float(cc)
        tie = Fraction(s64)
        assert exact != tie and abs(exact - tie) == Fraction(2) ** -63 and _round_f32(tie) != float(want)
        assert _round_f32(exact) == float(want)
        assert float(F32(s64)) != float(want)                         # the double rounding really goes wrong here
        got = A.fma32(a, b, cc)
        assert got.dtype == F32 and float(got) == float(want), (a, b, cc, float(got), float(want))
    assert float(A.fma32(F32(0.0), F32(3.0), F32(-0.0))) == 0.0 and not np.signbit(A.fma32(F32(0.0), F32(3.0), F32(-0.0)))
    assert np.signbit(A.fma32(F32(-0.0), F32(3.0), F32(-0.0)))
    assert np.isnan(A.fma32(F32(np.inf), F32(0.0), F32(1.0))) and A.fma32(F32(np.inf), F32(1.0), F32(1.0)) == np.inf


def test_bf16_bits_rounds_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -2.5, 3.4e38, np.inf, 0.0, -0.0], dtype=F32)
    want = [0x3F80, 0x3F80, 0x3F82, 0x3F81, 0xC020, 0x7F80, 0x7F80, 0x0000, 0x8000]
    assert A.bf16_bits(x).tolist() == want
    t = torch.randn(10000, generator=torch.Generator().manual_seed(0)) * 10 ** torch.linspace(-30, 30, 10000)
    assert np.array_equal(A.bf16_bits(t.numpy()), t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    assert A.bf16_is_nan(A.bf16_bits(np.array([np.nan, -np.nan, 1.0], dtype=F32))).tolist() == [True, True, False]


# ------------------------------------------------------------------------------------------------ the recorded bits
def _widen(bits):
    return (bits.astype(np.uint32) << np.uint32(16)).view(F32)


def test_restatement_reproduces_every_recorded_digest():
    """13 cases x 8 variants, every output array: 432 digests a GPU produced, none skipped."""
    with open(GOLDEN) as f:
        recorded = json.load(f)["cases"]
    cases = C.recorded_cases()
    assert len(cases) == 13 and len(C.RECORDED_VARIANTS) == 8
    checked = 0
    for case in cases:
        n, g16 = case["n"], case["entry"].endswith("_g16")
        a = {k: x[:n] for k, x in C.exact_inputs(case).items()}
        g = _widen(a["g"]) if g16 else a["g"]
        for ss, step, with_pb in C.RECORDED_VARIANTS:
            kw = dict(b1=C.BETAS[0], b2=C.BETAS[1], eps=C.EPS, step=step, sumsq=ss, max_norm=C.MAX_NORM)
            if case["table"] is not None:
                bounds, groups = case["table"]
                grp = A.group_of_elements(bounds, groups, np.arange(n))
                p2, m2, v2, pb = A.emul_groups(a["p"], a["m"], a["v"], g, grp, *C._rates(2), g16=g16, **kw)
            else:
                p2, m2, v2, pb = A.emul_step(a["p"], a["m"], a["v"], g, g16=g16,
                                             scalars=A.host_scalars(C.LR, kw["b1"], kw["b2"], C.EPS, C.WD, step, ss, C.MAX_NORM))
            out = {"p": p2, "m": m2, "v": v2, "pb": pb if with_pb else a["pb"]}
            if case["decay"] is not None:
                out["ema"] = E.ema_step(a["ema"], p2, case["decay"])
            want = recorded[case["name"]]["outputs"][C.variant_name(ss, step, with_pb)]
            assert sorted(want) == sorted(C.OUTPUTS[k] for k in out)
            for k, x in out.items():
                assert C.digest({k: x}) == want[C.OUTPUTS[k]], (case["name"], C.variant_name(ss, step, with_pb), k)
                checked += 1
    assert checked == 432


# ------------------------------------------------------------------------------------------------ ref_step is AdamW
def _torch_adamw(groups, step, b1, b2, eps, max_norm=None):
    """groups: list of (p, m, v, g, lr, wd) float64 tensors / floats -> list of (p', m', v') from torch.optim.AdamW."""
    params = [torch.nn.Parameter(p.clone()) for p, *_ in groups]
    opt = torch.optim.AdamW([dict(params=[q], lr=lr, weight_decay=wd) for q, (_, _, _, _, lr, wd) in zip(params, groups)],
                            betas=(b1, b2), eps=eps, foreach=False)
    for q, (_, m, v, g, _, _) in zip(params, groups):
        q.grad = g.clone()
        opt.state[q] = dict(step=torch.tensor(float(step - 1)), exp_avg=m.clone(), exp_avg_sq=v.clone())
    if max_norm is not None:
        torch.nn.utils.clip_grad_norm_(params, max_norm=max_norm, foreach=False)
    opt.step()
    return [(q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"]) for q in params]


def _fp64_state(k, gen):
    """p, m, v, g in float64 with m, g and -p of one (random) sign per element, so that neither m' = b1 m + (1 - b1) g nor
    p' = decay p - q cancels: 1e-12 relative per element is then a statement about the formulas, not about conditioning
    (torch forms m' as a lerp; where the two terms cancel to 1e-4 of their size, two correct float64 formulas differ by more)."""
    r = lambda: torch.randn(k, dtype=torch.float64, generator=gen)                 # noqa: E731
    sign = torch.where(r() < 0, -1.0, 1.0).double()
    return -sign * r().abs(), sign * r().abs() * 0.1, r().square() * 0.01, sign * r().abs()


def _close(a, b, what):
    assert bool(((a - b).abs() <= 1e-12 * b.abs()).all()), (what, float(((a - b).abs() / b.abs()).max()))


@pytest.mark.parametrize("step", [1, 7, 1000])
@pytest.mark.parametrize("hp", HYPER, ids=["hp0", "hp1", "hp2"])
def test_ref_step_is_torch_adamw(hp, step):
    lr, b1, b2, eps, wd = (float(F32(x)) for x in hp)
    gen = torch.Generator().manual_seed(step)
    p, m, v, g = _fp64_state(1000, gen)
    assert bool((p < 0).any()) and bool((p > 0).any())
    (tp, tm, tv), = _torch_adamw([(p, m, v, g, lr, wd)], step, b1, b2, eps)
    R = A.ref_step(p, m, v, g, lr=lr, b1=b1, b2=b2, eps=eps, wd=wd, step=step)
    _close(R["p"], tp, "p"), _close(R["m"], tm, "m"), _close(R["v"], tv, "v")


def test_ref_step_is_torch_adamw_with_two_groups_and_the_clip():
    """Two ranges with their own (lr, weight_decay) and torch's clip_grad_norm_(max_norm = 1) over both; the gradients are
    scaled so that their true sum of squares is a float32 value (ref_step takes the float32 sumsq word)."""
    lrs, wds = ([float(F32(x)) for x in xs] for xs in C._rates(2))
    b1, b2, eps = float(F32(0.9)), float(F32(0.999)), float(F32(1e-8))
    gen = torch.Generator().manual_seed(3)
    sizes = (600, 400)
    st = [_fp64_state(k, gen) for k in sizes]
    true = sum(float(g.square().sum()) for *_, g in st)
    ss = float(F32(true))
    st = [(p, m, v, g * math.sqrt(ss / true)) for p, m, v, g in st]
    assert abs(sum(float(g.square().sum()) for *_, g in st) / ss - 1) < 1e-14 and ss > 100
    want = _torch_adamw([(*s, lr, wd) for s, lr, wd in zip(st, lrs, wds)], 7, b1, b2, eps, max_norm=1.0)
    cat = [torch.cat([s[i] for s in st]) for i in range(4)]
    per = lambda xs: torch.cat([torch.full((k,), x, dtype=torch.float64) for k, x in zip(sizes, xs)])       # noqa: E731
    R = A.ref_step(*cat, lr=per(lrs), b1=b1, b2=b2, eps=eps, wd=per(wds), step=7, sumsq=ss, max_norm=1.0)
    assert R["clip_ratio"] < 0.1
    for i, key in enumerate("pmv"):
        _close(R[key], torch.cat([w[i] for w in want]), key)
    Rn = A.ref_step(*cat, lr=per(lrs[::-1]), b1=b1, b2=b2, eps=eps, wd=per(wds[::-1]), step=7, sumsq=ss, max_norm=1.0)
    assert not bool(((Rn["p"] - R["p"]).abs() <= 1e-12 * R["p"].abs()).any())


# ------------------------------------------------------------------------------------------------ containment
def _regime(name, n, seed, g16):
    rng = np.random.default_rng(seed)
    r = lambda: rng.standard_normal(n)                                              # noqa: E731
    if name == "unit":
        p, m, v, g = r(), r() * 0.1, r() ** 2 * 0.01, r()
    elif name == "wide":
        dec = lambda: 10.0 ** rng.uniform(-6, 3, n)                                 # noqa: E731
        p, m, v, g = r() * dec(), r() * dec(), (r() * dec()) ** 2, r() * dec()
    elif name == "late":
        p, m, v, g = r(), r() * 1e-7, r() ** 2 * 1e-14, r() * 1e-7
    else:
        raise KeyError(name)
    p, m, v, g = (x.astype(F32) for x in (p, m, v, g))
    if g16:
        g = _widen(A.bf16_bits(g))
    return p, m, v, g


def _both(st, hp, step, sumsq, g16, mutation=None, ref_hp=None):
    """-> the restatement's (p', m', v') as tensors, ref_step's dict (of ``ref_hp`` / ``mutation`` when given), the bars of the
    UNMUTATED reference."""
    lr, b1, b2, eps, wd = hp
    p2, m2, v2, _ = A.emul_step(*st, g16=g16, scalars=A.host_scalars(lr, b1, b2, eps, wd, step, sumsq, 1.0))
    t = [torch.from_numpy(x) for x in st]
    R = A.ref_step(*t, lr=lr, b1=b1, b2=b2, eps=eps, wd=wd, step=step, sumsq=sumsq, max_norm=1.0)
    B = A.bars(R)
    if mutation is not None or ref_hp is not None:
        lr, b1, b2, eps, wd = ref_hp or hp
        R = A.ref_step(*t, lr=lr, b1=b1, b2=b2, eps=eps, wd=wd, step=step, sumsq=sumsq, max_norm=1.0, mutation=mutation)
    return tuple(torch.from_numpy(x) for x in (p2, m2, v2)), R, B


@pytest.mark.parametrize("g16", [False, True], ids=["fp32grad", "bf16grad"])
@pytest.mark.parametrize("regime", ["unit", "wide", "late"])
def test_restatement_lies_within_the_bars_of_fp64_adamw(regime, g16):
    st = _regime(regime, N, 11, g16)
    worst = 0.0
    for hp in HYPER:
        for step in STEPS:
            for clip, ss in CLIPS.items():
                got, R, B = _both(st, hp, step, ss, g16)
                w, outside = A.worst_ratio(got, R, B)
                assert int(outside) == 0 and float(w) <= 1.0, (regime, g16, hp, step, clip, float(w), int(outside))
                assert (clip == "active") == (R["clip_ratio"] is not None and R["clip_ratio"] < 1)
                worst = max(worst, float(w))
    print(f"containment {regime} {'bf16' if g16 else 'fp32'} gradients: worst |emul - ref| / bar = {worst:.3f}")
    assert 0.05 < worst <= 1.0                      # (a bar a hundred times too wide would say nothing)


@pytest.mark.parametrize("d", [0.0, 0.5, 0.999])
def test_ema_line_lies_within_three_roundings(d):
    worst = 0.0
    for regime in ("unit", "wide", "late"):
        p, m, v, g = _regime(regime, N, 5, False)
        ema = _regime(regime, N, 6, False)[0]
        p2 = A.emul_step(p, m, v, g, g16=False, scalars=A.host_scalars(*HYPER[0], 7, 1e4, 1.0))[0]
        got = E.ema_step(ema, p2, d).astype(np.float64)
        ref = E.ema_step_ref(ema.astype(np.float64), p2, d)
        bar = 3 * U * np.maximum(np.abs(ema), np.abs(p2)).astype(np.float64)
        assert (np.abs(got - ref) <= bar).all()
        worst = max(worst, float((np.abs(got - ref) / bar).max()))
    print(f"ema d = {d}: worst ratio {worst:.3f}")


# ------------------------------------------------------------------------------------------------ sensitivity
def _share_outside(got, R, B):
    """Share of elements with m', v' or p' outside its bar around R."""
    bad = torch.zeros(got[0].shape, dtype=torch.bool)
    for x, key, bar in ((got[1], "m", B[0]), (got[2], "v", B[1]), (got[0], "p", B[2])):
        bad |= ~((x.double() - R[key]).abs() <= bar)
    return float(bad.double().mean())


NEIGHBOUR = tuple(zip(*C._rates(3)))[1]              # group 1 of three: (4e-3, 0.0) next to group 0's (1e-3, 1e-2)
SENSITIVITY = [("no_bc1", 7, "unit"), ("no_bc2", 7, "unit"), ("step_plus_1", 7, "unit"), ("step_plus_1", 1000, "unit"),
               ("eps_in_sqrt", 7, "late"), ("l2_decay", 7, "unit"), ("clip_by_sumsq", 7, "unit"), ("unclipped_moments", 7, "unit"),
               ("neighbour_group", 7, "unit")]


@pytest.mark.parametrize("mutation,step,regime", SENSITIVITY, ids=[f"{m}-step{s}-{r}" for m, s, r in SENSITIVITY])
def test_bars_reject_a_wrong_optimiser(mutation, step, regime):
    """The unmutated restatement against the unmutated bars laid around a WRONG reference: more than a quarter of the elements
    must fall outside, for both gradient types (clip active: sumsq = 1e4, max_norm = 1)."""
    for g16 in (False, True):
        st = _regime(regime, N, 23, g16)
        hp = HYPER[0]
        if mutation == "neighbour_group":
            got, R, B = _both(st, hp, step, 1e4, g16, ref_hp=(NEIGHBOUR[0], *hp[1:4], NEIGHBOUR[1]))
        else:
            got, R, B = _both(st, hp, step, 1e4, g16, mutation=mutation)
        assert _share_outside(got, *_both(st, hp, step, 1e4, g16)[1:]) == 0.0
        share = _share_outside(got, R, B)
        print(f"mutation {mutation} step {step} {regime} {'bf16' if g16 else 'fp32'}: share outside {share:.3f}")
        assert share > 0.25, (mutation, step, regime, g16, share)


# ------------------------------------------------------------------------------------------------ trajectory
def test_teacher_forced_trajectory_of_twelve_steps():
    """Twelve consecutive steps of the restatement with fresh gradients, the true clip norm and a cosine lr; at EVERY step
    ref_step is fed the restatement's own float32 state, so each comparison is one step wide and the bars apply.  (Free-running
    float32 and float64 trajectories drift apart through 1 / (sqrt(v) + eps) without a derivable bound: not compared.)"""
    for g16 in (False, True):
        p, m, v, _ = _regime("unit", N, 31, g16)
        w = torch.nn.Parameter(torch.zeros(1))
        opt = torch.optim.SGD([w], lr=1e-3)
        sch = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=12)
        rng = np.random.default_rng(32)
        worst, lrs = 0.0, []
        for step in range(1, 13):
            lr = opt.param_groups[0]["lr"]
            lrs.append(lr)
            g = rng.standard_normal(N).astype(F32)
            if g16:
                g = _widen(A.bf16_bits(g))
            ss = float(F32(float((g.astype(np.float64) ** 2).sum())))
            _, b1, b2, eps, wd = HYPER[0]
            p2, m2, v2, _ = A.emul_step(p, m, v, g, g16=g16, scalars=A.host_scalars(lr, b1, b2, eps, wd, step, ss, 1.0))
            R = A.ref_step(*(torch.from_numpy(x) for x in (p, m, v, g)), lr=lr, b1=b1, b2=b2, eps=eps, wd=wd, step=step, sumsq=ss,
                           max_norm=1.0)
            wr, outside = A.worst_ratio(tuple(torch.from_numpy(x) for x in (p2, m2, v2)), R, A.bars(R))
            assert int(outside) == 0 and float(wr) <= 1.0, (g16, step, float(wr))
            worst = max(worst, float(wr))
            assert not np.array_equal(p2, p)
            p, m, v = p2, m2, v2
            opt.step(), sch.step()
        assert len(set(lrs)) == 12 and lrs[0] == 1e-3 and lrs[-1] < 1e-4
        print(f"teacher-forced trajectory {'bf16' if g16 else 'fp32'} gradients: worst ratio {worst:.3f}")
