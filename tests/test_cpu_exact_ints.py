"""tests/exact_ints.py can detect what it claims to detect (no GPU): the 256 cap holds for every K the GPU file uses, one
changed operand element or mask bit changes a reference bit, each planted reference-side bug makes assert_bits_equal
raise, and the fp32-matmul reference of the large shapes equals the fp64 one.  For the fractional grid of
tests/test_gpu_gemm_epilogues.py: the scale rule and the 90 % condition hold for every (K, K2) used there, a correct fp32
epilogue stays within ulp_bar of the fp64 reference, and each planted epilogue bug leaves it."""
import numpy as np
import pytest
import torch

import exact_ints as E
import test_gpu_exact_contractions as G
import test_gpu_gemm_epilogues as P

BF = torch.bfloat16
# every (K, K2) a bf16-output case of either GPU file contracts over; cases without a bias only lower the magnitudes, and a
# grid case is its integer case times a power of two (its [gate | up] is checked bit for bit under the same cap)
ALL_K_K2 = sorted(set(G.ALL_K_K2) | set(P.INT_K_K2) | set(P.GRID_K_K2))


def _bf(ref64):
    """What a correct kernel returns for the exact value ``ref64``."""
    return ref64.float().to(BF)


def _sum_pmf(K):
    """Exact distribution of a sum of K products of two independent ternary operands (value -1 / 0 / +1 with probability
    2/9, 5/9, 2/9) on the support -K..K."""
    n = 2 * K + 1
    p = np.zeros(n)
    p[0], p[1], p[n - 1] = 5 / 9, 2 / 9, 2 / 9
    return np.fft.fftshift(np.fft.irfft(np.fft.rfft(p) ** K, n))


@pytest.mark.parametrize("Ktot", sorted({k + k2 for k, k2 in ALL_K_K2}))
def test_cap_holds_analytically(Ktot):
    """P(|sum of K + K2 ternary products| + 8 > 256) <= 1 %: bias and residual add at most 4 each."""
    pmf = _sum_pmf(Ktot)
    s = np.arange(-Ktot, Ktot + 1)
    frac = float(pmf[np.abs(s) + 8 > E.CAP].sum())
    assert frac <= E.CAP_FRACTION, (Ktot, frac)
    if Ktot == 14400:
        assert 0.0005 < frac < 0.003          # sigma = 80: about 0.15 % (two-sided tail beyond 3.1 sigma)


@pytest.mark.parametrize("K,K2", list(dict.fromkeys(sorted(ALL_K_K2, key=lambda t: (t[0] + t[1], t[1]))[-3:] + [(4096, 64)])))
def test_cap_holds_on_generated_data(K, K2):
    """The generators themselves (not only the model of them): plain form with bias and residual, and the masked-pair form
    with 1/(1-p) = 2, at the largest K of the GPU file."""
    M, N = 96, 96
    a, w = E.ternary((M, K), 1), E.ternary((N, K), 2)
    a2, w2 = (E.ternary((M, K2), 3), E.ternary((N, K2), 4)) if K2 else (None, None)
    ref = E.exact_ref(a, w, a2, w2, bias=E.bias_ints(N, 5), residual=E.residual_ints(M, N, 6))
    assert E.cap_fraction(ref) <= E.CAP_FRACTION
    E.assert_bits_equal(_bf(ref), ref)
    u, at = E.ternary((M, 64), 7), E.ternary((N, 64), 8)
    refm = E.exact_ref(a, w, u, at, keep=E.keep_mask(9, M, N, 0.5), pair_scale=2.0)
    assert E.cap_fraction(refm) <= E.CAP_FRACTION
    assert bool((refm == refm.round()).all())


def test_generators_are_seeded_uniform_and_in_range():
    t = E.ternary((400, 300), 11)
    assert torch.equal(t, E.ternary((400, 300), 11)) and not torch.equal(t, E.ternary((400, 300), 12))
    assert t.dtype == BF and set(t.unique().tolist()) == {-1.0, 0.0, 1.0}
    for v in (-1.0, 0.0, 1.0):
        assert abs(float((t == v).float().mean()) - 1 / 3) < 0.01          # sigma = 1.4e-3
    assert set(E.bias_ints(4000, 1).unique().tolist()) == set(float(i) for i in range(-4, 5))
    assert set(E.residual_ints(70, 60, 2).unique().tolist()) == set(float(i) for i in range(-4, 5))
    assert set(E.gate_up_ints(70, 60, 3).unique().tolist()) == set(float(i) for i in range(-3, 4))


def test_mask_restatements_agree_and_p_half_is_exact():
    """The torch-integer mask of the large shapes is the numpy one; at p = 0.5 the threshold is 32768 and about half is kept."""
    for seed, M, K in ((0x1234ABCD, 300, 256), (7, 5, 4096), (0xFFFFFFFF, 129, 130)):
        ref = E.keep_mask(seed, M, K, 0.5)
        assert torch.equal(E.keep_mask_device(seed, M, K, 0.5, "cpu"), ref)
        rows = [0, M - 1, M // 2]
        assert np.array_equal(E.keep_mask_rows(seed, rows, K, 0.5), ref.numpy()[rows])
    assert abs(float(E.keep_mask(3, 512, 512, 0.5).float().mean()) - 0.5) < 0.005
    assert min(65535, int(0.5 * 65536 + 0.5)) == 32768


def _case(M=300, N=80, K=136, K2=24, seed=0):
    a, w = E.ternary((M, K), seed + 1), E.ternary((N, K), seed + 2)
    a2, w2 = E.ternary((M, K2), seed + 3), E.ternary((N, K2), seed + 4)
    return a, w, a2, w2, E.bias_ints(N, seed + 5), E.residual_ints(M, N, seed + 6)


def _other(v):
    """A different ternary value."""
    return 1.0 if float(v) != 1.0 else -1.0


@pytest.mark.parametrize("where", ["k_tail", "m_tail", "k2_column"])
def test_single_operand_element_changes_a_reference_bit(where):
    a, w, a2, w2, bias, res = _case()
    base = _bf(E.exact_ref(a, w, a2, w2, bias, res))
    a, a2 = a.clone(), a2.clone()
    if where == "k_tail":
        a[17, -1] = _other(a[17, -1])
    elif where == "m_tail":
        a[-1, 40] = _other(a[-1, 40])
    else:
        a2[123, -1] = _other(a2[123, -1])
    moved = _bf(E.exact_ref(a, w, a2, w2, bias, res))
    assert not torch.equal(moved, base)
    assert float((moved.float() - base.float()).abs().max()) >= 1.0
    with pytest.raises(AssertionError, match="not bit-equal"):
        E.assert_bits_equal(base, E.exact_ref(a, w, a2, w2, bias, res))


def test_single_mask_bit_changes_a_reference_bit():
    M, N, K = 300, 256, 128
    a, w, u, at = E.ternary((M, K), 1), E.ternary((N, K), 2), E.ternary((M, 64), 3), E.ternary((N, 64), 4)
    keep = E.keep_mask(77, M, N, 0.5)
    pair = u.double() @ at.double().t()
    m, n = [int(v) for v in (pair != 0).nonzero()[-1]]               # a position where the pair is non-zero
    base = E.exact_ref(a, w, u, at, keep=keep, pair_scale=2.0)
    flipped = keep.clone()
    flipped[m, n] = ~flipped[m, n]
    moved = E.exact_ref(a, w, u, at, keep=flipped, pair_scale=2.0)
    assert abs(float(moved[m, n] - base[m, n])) >= 2.0
    with pytest.raises(AssertionError, match="not bit-equal"):
        E.assert_bits_equal(_bf(moved), base)


def test_gate_up_and_residual_generators_reach_the_reference():
    a, w, a2, w2, bias, res = _case()
    base = E.exact_ref(a, w, a2, w2, bias, res)
    res2 = res.clone(); res2[-1, -1] += 1
    bias2 = bias.clone(); bias2[0] += 1
    assert not torch.equal(_bf(E.exact_ref(a, w, a2, w2, bias, res2)), _bf(base))
    assert not torch.equal(_bf(E.exact_ref(a, w, a2, w2, bias2, res)), _bf(base))


PLANTED = ["k_slab_dropped", "pair_dropped_from_tile0", "w_blocks_swapped", "mask_shifted", "splitk_slab_twice"]


@pytest.mark.parametrize("bug", PLANTED)
def test_planted_reference_side_bugs_are_caught(bug):
    """Each is what a subtly wrong kernel would return; assert_bits_equal must raise against the true reference."""
    M, N, K = 600, 256, 192
    a, w, u, at = E.ternary((M, K), 1), E.ternary((N, K), 2), E.ternary((M, 64), 3), E.ternary((N, 64), 4)
    bias, res = E.bias_ints(N, 5), E.residual_ints(M, N, 6)
    masked = bug == "mask_shifted"
    keep = E.keep_mask(5, M, N, 0.5) if masked else None
    ps = 2.0 if masked else 1.0
    true = E.exact_ref(a, w, u, at, None if masked else bias, None if masked else res, keep=keep, pair_scale=ps)
    E.assert_bits_equal(_bf(true), true)                                   # the correct kernel passes
    if bug == "k_slab_dropped":
        wrong = E.exact_ref(a[:, :K - 8], w[:, :K - 8], u, at, bias, res)
    elif bug == "pair_dropped_from_tile0":
        u0 = u.clone(); u0[256:] = 0                                       # tile0 = 1
        wrong = E.exact_ref(a, w, u0, at, bias, res)
    elif bug == "w_blocks_swapped":
        w1, at1 = w.clone(), at.clone()
        w1[16:32], w1[32:48] = w[32:48], w[16:32]
        at1[16:32], at1[32:48] = at[32:48], at[16:32]
        wrong = E.exact_ref(a, w1, u, at1, None, res) + bias.double()[None, :]       # the products moved, the epilogue did not
    elif bug == "mask_shifted":
        wrong = E.exact_ref(a, w, u, at, keep=torch.roll(keep, 1, dims=1), pair_scale=2.0)
    else:
        wrong = true + a[:, 64:128].double() @ w[:, 64:128].double().t()
    with pytest.raises(AssertionError, match="not bit-equal") as info:
        E.assert_bits_equal(_bf(wrong), true)
    assert "256x256 tile" in str(info.value) and "got" in str(info.value)
    if bug == "pair_dropped_from_tile0":
        assert "tile (1, 0)" in str(info.value)                            # located: nothing wrong above row 256


def test_fp32_output_form_and_its_range_guard():
    g, x = E.ternary((700, 16), 1), E.ternary((700, 776), 2)
    ref = g.double().t() @ x.double()
    E.assert_bits_equal(ref.float(), ref)
    off = ref.float().clone(); off[3, 775] += 1
    with pytest.raises(AssertionError, match="not bit-equal"):
        E.assert_bits_equal(off, ref)
    with pytest.raises(AssertionError, match="refused"):
        E.assert_bits_equal((ref * 2.0 ** 20).float(), ref * 2.0 ** 20)


def test_the_cap_refuses_a_case_that_rounding_could_hide():
    a, w = E.small_ints((64, 512), -8, 8, 1), E.small_ints((64, 512), -8, 8, 2)          # sigma ~ 600
    ref = E.exact_ref(a, w)
    with pytest.raises(AssertionError, match="case refused"):
        E.assert_bits_equal(_bf(ref), ref)
    hidden = ref + ((ref.abs() > 1024) & (ref % 8 == 0))                   # a +1 error that bf16 rounding swallows (ulp 8 there)
    assert bool((_bf(hidden) == _bf(ref)).all()) and bool((hidden != ref).any())


def test_fp32_matmul_reference_equals_fp64_at_a_mid_shape():
    M, N, K, K2 = 700, 512, 4096, 64
    a, w, a2, w2 = E.ternary((M, K), 1), E.ternary((N, K), 2), E.ternary((M, K2), 3), E.ternary((N, K2), 4)
    bias = E.bias_ints(N, 5)
    pre32 = E.device_pre(a, w, a2, w2, bias)
    assert pre32.dtype == torch.float32
    assert torch.equal(pre32.double(), E.exact_pre(a, w, a2, w2, bias))
    E.confirm_rows(pre32, a, w, a2, w2, bias)
    keep = E.keep_mask_device(21, M, N, 0.5, "cpu")
    prem = E.device_pre(a, w, a2, w2, keep=keep, pair_scale=2.0)
    assert torch.equal(prem.double(), E.exact_pre(a, w, a2, w2, keep=E.keep_mask(21, M, N, 0.5), pair_scale=2.0))
    E.confirm_rows(prem, a, w, a2, w2, keep_seed=21, keep_p=0.5, pair_scale=2.0)
    broken = pre32.clone(); broken[255, 100] += 1                          # confirm_rows looks at tile-boundary rows
    with pytest.raises(AssertionError, match="differs from CPU fp64"):
        E.confirm_rows(broken, a, w, a2, w2, bias)


def test_row_subsample_contents():
    for M in (1, 77, 300, 5861):
        rows = E.row_subsample(M)
        assert rows[0] == 0 and rows[-1] == M - 1 and rows == sorted(set(rows))
        for t in (192, 256):
            for b in range(t, M, t):
                assert b - 1 in rows and b in rows
        assert len(rows) <= 2 + 2 * (M // 192 + M // 256) + 32


def test_ulp_bar_accepts_one_rounding_and_rejects_two_ulps():
    x = torch.arange(-260, 261, dtype=torch.float64)[None, :].repeat(9, 1)
    res = E.residual_ints(9, x.shape[1], 1).double()
    ref = E.ACTS["silu"](x) + res
    got = _bf(E.ACTS["silu"](x.float()).double() + res)                    # fp32 activation, one bf16 rounding
    E.assert_within_ulp(got, ref, x)
    ulp = 2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -120))) - 7)
    with pytest.raises(AssertionError, match="outside the ulp bar"):
        E.assert_within_ulp(_bf(ref + 2 * ulp * (x == 37)), ref, x)
    with pytest.raises(AssertionError, match="outside the ulp bar"):
        E.assert_within_ulp(_bf(E.ACTS["silu"](x + (x == -3)) + res), ref, x)       # pre-activation off by one


# ------------------------------------------------------------------ the fractional grid (tests/test_gpu_gemm_epilogues.py)
GRID_K_K2 = sorted(set(P.GRID_K_K2) | {(64, 0), (128, 0), (4096, 0), (4096, 64), (14336, 64)})
ACT32 = {                                                                  # the kernels' activations restated in fp32 torch
    "quick_gelu": lambda v: v * torch.sigmoid(1.702 * v),
    "gelu": lambda v: 0.5 * v * (1 + torch.erf(v * 0.70710678118654752)),
    "silu": lambda v: v * torch.sigmoid(v),
    "gelu_tanh": lambda v: 0.5 * v * (1 + torch.tanh(0.7978845608028654 * (v + 0.044715 * v ** 3))),
}
_grid_cache = {}


def _grid(K, K2, M=256, N=256):
    """(a, w, a2, w2, bias, res, exact fp64 pre-activation with the bias) - generated once per (K, K2), never modified."""
    if (K, K2) not in _grid_cache:
        ops_in = E.grid_operands(M, N, K, K2, 100 + K + 3 * K2)
        _grid_cache[(K, K2)] = (*ops_in, E.exact_pre(*ops_in[:5]))
    return _grid_cache[(K, K2)]


def _epilogue32(pre64, bias, res, act, with_bias, with_res):
    """(what a correct kernel returns, the fp64 reference, the exact pre-activation): bias add, activation and residual add
    in fp32 on the exact accumulator, one rounding to bf16."""
    x = pre64 if with_bias else pre64 - bias.double()[None, :]
    v = (pre64 - bias.double()[None, :]).float()                           # the accumulator: exact in fp32
    assert torch.equal(v.double(), pre64 - bias.double()[None, :])
    if with_bias:
        v = v + bias.float()[None, :]
    v = ACT32[act](v)
    ref = E.ACTS["gelu" if act == "gelu_tanh" else act](x)
    if with_res:
        v, ref = v + res.float(), ref + res.double()
    return v.to(BF), ref, x


@pytest.mark.parametrize("K,K2", GRID_K_K2)
def test_grid_scale_rule_share_and_fp32_exactness(K, K2):
    s = E.grid_scale(K, K2)
    sd = (4 * (K + K2) / 9) ** 0.5
    assert s == 2.0 ** round(np.log2(s)) and s * sd <= E.GRID_SD < 2 * s * sd
    a, w, a2, w2, bias, res, pre = _grid(K, K2)
    assert (a2 is None) == (K2 == 0)
    assert set(a.unique().tolist()) == {-1.0, 0.0, 1.0} and set(w.unique().tolist()) == {-s, 0.0, s}
    assert set(bias.unique().tolist()) <= {i / 8 for i in range(-8, 9)} and set(res.unique().tolist()) == {i / 8 for i in range(-32, 33)}
    nb = pre - bias.double()[None, :]
    for x in (pre, nb):
        E.assert_grid_case(x)
        assert E.grid_share(x) >= 0.99                                     # sd <= 1.4 (+ a bias of sd 0.6): |x| <= 4 is 2.6 sigma
    assert 0.45 * E.GRID_SD < float(nb.std()) < 1.1 * E.GRID_SD
    assert bool((nb / s == (nb / s).round()).all()) and E.cap_fraction(nb / s) <= E.CAP_FRACTION
    pre32 = E.device_pre(a, w, a2, w2, bias)                               # torch's fp32 matmul, any blocking
    assert pre32.dtype == torch.float32 and torch.equal(pre32.double(), pre)
    E.confirm_rows(pre32, a, w, a2, w2, bias)


def test_grid_scale_table():
    assert [E.grid_scale(k) for k in (64, 128, 4096, 4160, 14400)] == [1 / 4, 1 / 8, 1 / 32, 1 / 32, 1 / 64]
    assert E.grid_scale(4096, 64) == E.grid_scale(4160) and E.grid_scale(72) == 1 / 8 and E.grid_scale(1) == 2.0


def test_grid_condition_refuses_saturated_pre_activations():
    a, w = E.ternary((64, 4096), 1), E.ternary((64, 4096), 2)              # integer operands: sd 43
    with pytest.raises(AssertionError, match="case refused"):
        E.assert_grid_case(E.exact_pre(a, w))
    x = torch.zeros(10, 10, dtype=torch.float64)
    x.view(-1)[:10] = 5.0
    E.assert_grid_case(x)                                                  # exactly 90 % inside
    x.view(-1)[10] = -4.125
    with pytest.raises(AssertionError, match="case refused"):
        E.assert_grid_case(x)


@pytest.mark.parametrize("with_bias,with_res", P.PRESENCES)
@pytest.mark.parametrize("act", P.ACT_NAMES)
@pytest.mark.parametrize("K,K2", GRID_K_K2)
def test_correct_fp32_epilogue_is_within_the_bar_on_the_grid(K, K2, act, with_bias, with_res):
    """The bar is held by the reference alone: worst |err| / bar is about 0.995 (a bf16 tie next to a power of two)."""
    a, w, a2, w2, bias, res, pre = _grid(K, K2)
    got, ref, x = _epilogue32(pre, bias, res, act, with_bias, with_res)
    E.assert_within_ulp(got, ref, x)


GRID_PLANTED = ["residual_dropped", "bias_dropped", "quick_gelu_for_silu", "gelu_for_quick_gelu", "tanh_gelu_for_erf_gelu",
                "residual_row_shifted", "fragment_from_neighbour"]


@pytest.mark.parametrize("K,K2", [(128, 0), (4096, 64)])
@pytest.mark.parametrize("bug", GRID_PLANTED)
def test_planted_epilogue_bugs_leave_the_bar(bug, K, K2):
    """Each is what a subtly wrong epilogue would return on the grid; at least one element must leave the bar."""
    a, w, a2, w2, bias, res, pre = _grid(K, K2)
    act = {"gelu_for_quick_gelu": "quick_gelu", "tanh_gelu_for_erf_gelu": "gelu"}.get(bug, "silu")
    true, ref, x = _epilogue32(pre, bias, res, act, True, True)
    E.assert_within_ulp(true, ref, x)                                      # the correct epilogue passes
    if bug == "residual_dropped":
        wrong = _epilogue32(pre, bias, res, act, True, False)[0]
    elif bug == "bias_dropped":
        wrong = _epilogue32(pre, bias, res, act, False, True)[0]
    elif bug == "quick_gelu_for_silu":
        wrong = _epilogue32(pre, bias, res, "quick_gelu", True, True)[0]
    elif bug == "gelu_for_quick_gelu":
        wrong = _epilogue32(pre, bias, res, "gelu", True, True)[0]
    elif bug == "tanh_gelu_for_erf_gelu":
        wrong = _epilogue32(pre, bias, res, "gelu_tanh", True, True)[0]
    elif bug == "residual_row_shifted":
        wrong = _epilogue32(pre, bias, torch.roll(res, 1, dims=0), act, True, True)[0]
    else:
        wrong = true.clone()
        wrong[:, 16:32] = true[:, 32:48]
    with pytest.raises(AssertionError, match="outside the ulp bar") as info:
        E.assert_within_ulp(wrong, ref, x)
    assert "256x256 tile" in str(info.value)
    if bug == "fragment_from_neighbour":
        assert "tile cols 16..31" in str(info.value)


def test_planted_residual_only_bugs_are_not_bit_equal():
    """EPI_RESIDUAL on the integer operands: the residual read 16 columns off, or dropped on the last rows only."""
    a, w, a2, w2, bias, res = _case(M=300, N=256)
    pre = E.exact_pre(a, w, a2, w2)
    true = pre + res.double()
    E.assert_bits_equal(_bf(true), true)
    shifted = res.double().clone()
    shifted[:, 16:32] = res.double()[:, 0:16]                              # rp for rp + 16
    tail = res.double().clone()
    tail[256:] = 0                                                         # dropped on the tail tile
    for wrong in (pre + shifted, pre + tail, pre):
        with pytest.raises(AssertionError, match="not bit-equal"):
            E.assert_bits_equal(_bf(wrong), true)


def test_ulp_bar_gain_defaults_to_the_plain_bar():
    ref, x = torch.linspace(-5, 5, 41, dtype=torch.float64)[None, :], torch.linspace(-9, 9, 41, dtype=torch.float64)[None, :]
    assert torch.equal(E.ulp_bar(ref, x), E.ulp_bar(ref, x, 1.0))
    assert torch.equal(E.ulp_bar(ref, x), 2.0 ** -8 * ref.abs() + 2.0 ** -20 * (1 + x.abs()))
    assert torch.equal(E.ulp_bar(0 * ref, x, 3.0), 3.0 * E.ulp_bar(0 * ref, x))          # only the activation term scales
    assert torch.equal(E.ulp_bar(ref, 0 * x, 1 + x.abs()), E.ulp_bar(ref, x))


@pytest.mark.parametrize("K,K2", sorted({(c[3], c[4]) for c in P.SWIGLU_GRID}))
def test_swiglu_product_on_the_grid_passes_and_planted_bugs_fail(K, K2):
    """h = silu(gate) * up in fp32 with one rounding stays within the bar with gain max(1, |up|); up taken from the
    neighbouring fragment, or a sigmoid for the SiLU, leaves it."""
    M, ff, s = 256, 128, E.grid_scale(K, K2)
    a, t = E.ternary((M, K), 1), E.ternary((M, K2), 2)
    w, b = (E.ternary((2 * ff, K), 3).float() * s).to(BF), (E.ternary((2 * ff, K2), 4).float() * s).to(BF)
    pre = E.exact_pre(a, w, t, b)
    assert torch.equal(E.device_pre(a, w, t, b).double(), pre) and torch.equal(_bf(pre).double(), pre)
    g, u = pre[:, :ff], pre[:, ff:]
    E.assert_grid_case(g)
    ref, gain = E.ACTS["silu"](g) * u, u.abs().clamp_min(1.0)
    g32, u32 = g.float(), u.float()
    E.assert_within_ulp((ACT32["silu"](g32) * u32).to(BF), ref, g, gain)
    for wrong in (ACT32["silu"](g32) * torch.roll(u32, 16, dims=1), torch.sigmoid(g32) * u32):
        with pytest.raises(AssertionError, match="outside the ulp bar"):
            E.assert_within_ulp(wrong.to(BF), ref, g, gain)


def test_swiglu_backward_on_the_grid_passes_and_planted_bugs_fail():
    """[d gate | d up] in fp32 as the kernel spells it, one rounding each: within the bar with ulp_bar's gains at gate / up
    on multiples of 1/8 in [-4, 4]; the SiLU derivative without its g (1 - s) term, or gate and up swapped, leaves it."""
    M, ff = 300, 256
    gu = E.grid_gate_up(M, 2 * ff, 5)
    assert set(gu.unique().tolist()) == {i / 8 for i in range(-32, 33)}
    dh = E.exact_pre(E.ternary((M, 4096), 1), E.ternary((ff, 4096), 2), E.ternary((M, 64), 3), E.ternary((ff, 64), 4),
                     keep=E.keep_mask(9, M, ff, 0.5), pair_scale=2.0)
    g, up = gu[:, :ff].double(), gu[:, ff:].double()
    sg = torch.sigmoid(g)
    ref = torch.cat([dh * up * sg * (1 + g * (1 - sg)), dh * g * sg], 1)
    x = torch.cat([dh, dh], 1)
    gain = torch.cat([(1 + g.abs()) * up.abs().clamp_min(1.0), 1 + g.abs()], 1)
    v, g32, u32 = dh.float(), g.float(), up.float()
    s32 = torch.sigmoid(g32)
    got = torch.cat([(v * u32 * (s32 * (1 + g32 * (1 - s32)))).to(BF), (v * (g32 * s32)).to(BF)], 1)
    E.assert_within_ulp(got, ref, x, gain)
    no_term = torch.cat([(v * u32 * s32).to(BF), (v * (g32 * s32)).to(BF)], 1)
    swapped = torch.cat([(v * g32 * (s32 * (1 + g32 * (1 - s32)))).to(BF), (v * (u32 * s32)).to(BF)], 1)
    for wrong in (no_term, swapped):
        with pytest.raises(AssertionError, match="outside the ulp bar"):
            E.assert_within_ulp(wrong, ref, x, gain)
