"""tests/mx_emul.py proved without a GPU: the shared-exponent rule exhaustively over every finite bf16 magnitude against
exact rationals (and against the two other spellings the project has: log2 in double, and the kernels' fp32
frexpf(amax / 448.f)), the element rule against torch's CPU cast on the whole pivot sweep, the round trip through every
finite code, the cap conditions that make the sweep worth sending to the GPU, and three deliberate mutations of the rule
(truncation, floor, no clamp) that these same checks must reject."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import mx_emul as mx

AMAX_BITS = np.arange(0x7F80, dtype=np.uint16)              # every finite non-negative bf16 pattern: 32640


def _rational_rule(bits, lo=-127):
    """ceil(log2(amax / 448)) clamped to [lo, 127] in exact rationals: the smallest E with 2^E >= amax / 448."""
    out = np.empty(len(bits), dtype=np.int64)
    for i, b in enumerate(bits):
        b = int(b)
        ex, m = b >> 7, b & 0x7F
        if b == 0:
            out[i] = lo
            continue
        r = Fraction(m + (128 if ex else 0)) * Fraction(2) ** (max(ex, 1) - 134) / 448
        E = r.numerator.bit_length() - r.denominator.bit_length()       # 2^(E-1) < r < 2^(E+1)
        while Fraction(2) ** E < r:
            E += 1
        while Fraction(2) ** (E - 1) >= r:
            E -= 1
        out[i] = min(127, max(lo, E))
    return out


RATIONAL = _rational_rule(AMAX_BITS)


def _scale_rule_mismatches(shared_exp):
    return int((shared_exp(mx.bf16_to_f64(AMAX_BITS)) != RATIONAL).sum())


def _element_rule_mismatches(e4m3_rne):
    """Against torch's CPU cast to float8_e4m3fn on the scaled values of the whole sweep (exact in fp32: at most 8
    significant bits, magnitudes in [2^-27, 448]); only the sign of zero may differ."""
    bits = mx.pivot_sweep()
    s = mx.pivot_sweep_ref()[1]
    x = mx.bf16_to_f64(bits).reshape(-1, mx.BLOCK)
    y = np.ldexp(x, 127 - s.reshape(-1, 1).astype(np.int64))
    y32 = y.astype(np.float32)
    assert bool((y32.astype(np.float64) == y).all())
    want = torch.from_numpy(y32).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    return int((~mx.same_codes(e4m3_rne(y), want)).sum()), y.size


def test_bf16_patterns_round_trip_through_fp64():
    bits = np.arange(1 << 16, dtype=np.uint16)
    finite = (bits >> 7) & 0xFF != 0xFF
    v = mx.bf16_to_f64(bits)
    as32 = (bits[finite].astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    assert bool((v[finite] == as32).all()) and bool((np.signbit(v) == (bits >> 15 == 1)).all())
    assert bool(np.isinf(v[[0x7F80, 0xFF80]]).all()) and bool(np.isnan(v[~finite & ((bits & 0x7F) != 0)]).all())
    assert bool((mx.f64_to_bf16_bits(v[finite]) == bits[finite]).all())


def test_shared_exponent_exhaustive_against_exact_rationals_and_the_other_spellings():
    amax = mx.bf16_to_f64(AMAX_BITS)
    E = mx.shared_exp(amax)
    assert len(AMAX_BITS) == 32640 and _scale_rule_mismatches(mx.shared_exp) == 0
    # the log2-in-double rule of the older torch restatement
    pos = amax > 0
    log2_rule = np.full(len(amax), -127, dtype=np.int64)
    log2_rule[pos] = np.clip(np.ceil(np.log2(amax[pos] / 448.0)), -127, 127).astype(np.int64)
    assert bool((log2_rule == E).all())
    # the kernels' arithmetic in fp32 with denormals kept: frexpf(amax / 448.f), f == 0.5f -> e - 1
    f, e = np.frexp(amax.astype(np.float32) / np.float32(448.0))
    assert f.dtype == np.float32
    fp32_rule = np.where(pos, np.clip(np.where(f == np.float32(0.5), e - 1, e), -127, 127), -127)
    assert bool((fp32_rule == E).all())
    byte = E + 127
    assert int(byte.min()) == 0 and int(byte.max()) == 247 and set(byte.tolist()) == set(range(248))
    clamped = np.nonzero(pos & (byte == 0))[0]
    assert len(clamped) == 1120 and int(clamped[-1]) == 1120            # patterns 1..1120; the next one gets byte 1
    assert float(np.ldexp(amax[1120], 127)) == 448.0 and int(byte[1121]) == 1
    # a flushed quotient (fp32 denormals off) would have said 127 for the smallest inputs: the emulator does not depend on it
    assert float(amax[1]) / 448.0 < 2.0 ** -126 and int(byte[1]) == 0


def test_element_rule_equals_the_cpu_cast_on_the_whole_sweep():
    bad, n = _element_rule_mismatches(mx.e4m3_rne)
    print(f"element rule: {bad} mismatches in {n} elements")
    assert bad == 0 and n > 5_000_000


def test_every_code_round_trips():
    """quantize(dequant(b, s)) == (b, s) for every finite code, at scale bytes from the subnormal bf16 range to the top."""
    others = mx.FINITE_CODES[mx.FINITE_CODES != 0x7E]
    assert len(mx.FINITE_CODES) == 254 and len(others) == 253
    nb = -(-len(others) // 31)
    codes = np.zeros((nb, 32), dtype=np.uint8)
    fill = np.zeros(nb * 31, dtype=np.uint8); fill[:len(others)] = others
    at = np.arange(nb) * 5 % 32
    cols = np.arange(32)[None, :]
    codes[cols == at[:, None]] = 0x7E                       # 448 in every block: the block's scale byte is forced
    codes[cols != at[:, None]] = fill
    table = mx.E4M3_TABLE[mx.FINITE_CODES]
    assert bool(np.isfinite(table).all()) and len(set(np.abs(table).tolist())) == 127 and bool(np.isnan(mx.E4M3_TABLE[[0x7F, 0xFF]]).all())
    for sb in (3, 10, 126, 127, 128, 200, 246):
        s = np.full((nb, 1), sb, dtype=np.uint8)
        v = mx.dequant(codes, s)
        q2, s2, v2 = mx.quantize(mx.f64_to_bf16_bits(v))
        assert bool((s2 == s).all()) and bool((q2 == codes).all()) and bool((v2 == v).all()), sb


def test_sweep_layout_and_cap_conditions():
    bits = mx.pivot_sweep()
    q, s, deq, ties = mx.pivot_sweep_ref()
    assert bits.shape[1] == 256 and bits.shape[0] % 64 == 0 and not bits.flags.writeable
    blocks = bits.reshape(-1, 32)
    mag = (blocks & 0x7FFF).astype(np.int64)
    amax_at = mag.argmax(1)
    live = mag.max(1) > 0
    # pivots: every exponent field x PIVOT_M occurs as a block maximum, at every block position
    pivots = set(mag.max(1)[live].tolist())
    assert pivots == {(ex << 7) | m for ex in range(255) for m in mx.PIVOT_M} - {0}
    assert set(amax_at[live].tolist()) == set(range(32)) and bool((~live).any())
    # |v| <= pivot and within 20 binades of it
    assert bool((mag.max(1)[:, None] - mag <= 128 * mx.BINADES_BELOW)[mag > 0].all())
    zero_share = float(((q & 0x7F) == 0).mean())
    n_ties = int(ties.sum())
    print(f"sweep: {bits.size} elements, zero bytes {100 * zero_share:.1f} %, ties {n_ties}, codes {len(set(q.reshape(-1).tolist()) - {0x80, 0x00}) + 2}, "
          f"scale bytes {len(set(s.reshape(-1).tolist()))}")
    assert zero_share <= 0.15
    assert n_ties >= 100_000
    assert set(q.reshape(-1).tolist()) == set(mx.FINITE_CODES.tolist())
    assert set(s.reshape(-1).tolist()) == set(range(248))
    # the reference itself: every block's largest element lands in [224, 448] unless the clamp holds it lower
    top = np.abs(np.ldexp(deq.reshape(-1, 32), 127 - s.reshape(-1, 1).astype(np.int64))).max(1)
    assert bool(((top >= 224) & (top <= 448))[s.reshape(-1) > 0].all()) and bool((top <= 448).all())
    # the 1-in-4 subsample keeps every significand and the edge binades
    sub = mx.pivot_sweep(mx.sweep_exponents(subsample=True))
    sm = (sub.reshape(-1, 32) & 0x7FFF).max(1)
    assert {int(p) >> 7 for p in sm if p} >= {0, 1, 8, 9, 254} and {int(p) & 0x7F for p in sm if p} == set(mx.PIVOT_M)
    assert sub.shape[0] * 3 < bits.shape[0]


@pytest.mark.parametrize("name", ["truncation", "floor", "no clamp"])
def test_mutations_of_the_rule_are_rejected(name):
    """The checks above, re-run on a deliberately wrong emulator, must each report mismatches."""
    if name == "truncation":
        bad, _ = _element_rule_mismatches(lambda y: mx.e4m3_rne(y, rint=np.trunc))
        assert bad > 100_000                                # every tie that rounds up, and everything above half a step
    elif name == "floor":
        assert _scale_rule_mismatches(lambda a: mx.shared_exp(a, ceil=False)) > 30_000      # all but the exact powers
    else:
        assert _scale_rule_mismatches(lambda a: mx.shared_exp(a, lo=-(1 << 20))) == 1120 - 128 + 1   # zero, and amax <= 448 2^-128
        q, s, _ = mx.quantize(np.full((1, 32), 0x0001, dtype=np.uint16))
        assert int(s[0, 0]) == 0 and int(q[0, 0]) == mx.e4m3_rne(np.ldexp(1.0, -133 + 127))
