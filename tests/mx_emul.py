"""Test-only helper: the MX-fp8 quantisation rule (OCP microscaling: e4m3 elements, one E8M0 scale per 32 consecutive
elements) restated exactly on the host - numpy, integers and fp64 only; no fp8 dtype, no log2.

A bf16 value is an 8-bit significand times a power of two, every scaling below is by a power of two, and every
intermediate has at most 8 significant bits inside fp64's exponent range: ``ldexp`` in fp64 IS the real value, whatever
the fp32 denormal mode of the device whose kernels are compared with this file (gemm_fp8.hip, common.hpp, ops.hip).

  * ``bf16_to_f64`` / ``f64_to_bf16_bits``: bit patterns (uint16) <-> exact fp64 values
  * ``shared_exp(amax)``: ceil(log2(amax / 448)) clamped to [-127, 127]; -127 for 0 (scale byte = E + 127)
  * ``e4m3_rne(y)``: |y| <= 448 -> e4m3 byte, round-to-nearest-even (step 2^(e-3); 2^-9 below 2^-6)
  * ``quantize(bits)`` -> (bytes, scale bytes, dequantised fp64), blocks of 32 along the last axis
  * ``dequant(bytes, scales)``: all 256 codes from a table (0x7F / 0xFF are NaN) times 2^(scale - 127)
  * ``pivot_sweep()``: the shared input of the CPU and GPU tests - every bf16 binade, four significands each, as a block
    maximum, surrounded by every bf16 pattern of the 20 binades below it
"""
from __future__ import annotations

import functools

import numpy as np

BLOCK = 32
PIVOT_M = (0x00, 0x60, 0x61, 0x7F)      # 1.0, 1.75 (= 448 * 2^k exactly), one ulp above it, the largest significand
BINADES_BELOW = 20
ROW = 256                               # columns of the sweep's 2-D form (8 blocks a row)
ROW_MULTIPLE = 64                       # rows padded to a multiple of this (zero blocks)


# ------------------------------------------------------------------ bf16 bit patterns <-> exact fp64
def bf16_to_f64(bits):
    """uint16 bf16 patterns -> fp64, from the fields (no float32 detour, so no denormal mode enters)."""
    b = np.asarray(bits).astype(np.int64)
    ex, m = (b >> 7) & 0xFF, b & 0x7F
    mag = np.ldexp((m + np.where(ex > 0, 128, 0)).astype(np.float64), np.maximum(ex, 1) - 134)
    mag = np.where(ex == 255, np.where(m == 0, np.inf, np.nan), mag)
    return np.where((b >> 15) & 1 == 1, -mag, mag)


def f64_to_bf16_bits(v):
    """fp64 values that bf16 holds exactly (asserted) -> uint16 patterns."""
    v = np.asarray(v, dtype=np.float64)
    m, e = np.frexp(np.abs(v))                              # |v| = m 2^e, m in [0.5, 1)
    ex = np.clip(e + 126, 0, 254)                           # biased exponent field; 0: subnormal
    sig = np.ldexp(np.abs(v), 134 - np.maximum(ex, 1))      # the 8-bit significand as an integer
    assert bool((sig == np.rint(sig)).all()) and bool((sig < 256).all()), "not a bf16 value"
    sig = sig.astype(np.int64)
    ex = np.where(sig == 0, 0, ex)
    bits = (ex << 7) + np.where(ex > 0, sig - 128, sig)
    return (bits | np.where(np.signbit(v), 0x8000, 0)).astype(np.uint16)


# ------------------------------------------------------------------ the rule
def shared_exp(amax, ceil=True, lo=-127):
    """ceil(log2(amax / 448)) clamped to [lo, 127], and ``lo`` for amax == 0 (int64).  With amax = f 2^e (frexp, f in [0.5, 1))
    and 448 = 0.875 * 2^9: amax / 448 = (f / 0.875) 2^(e - 9) with f / 0.875 in [4/7, 8/7), so the ceiling is e - 9 for
    f <= 0.875 and e - 8 above - comparisons of exact fp64 values.  (``ceil`` / ``lo`` exist for the mutation tests only.)"""
    amax = np.asarray(amax, dtype=np.float64)
    assert bool(np.isfinite(amax).all()) and bool((amax >= 0).all())
    f, e = np.frexp(amax)
    e = e.astype(np.int64)
    if ceil:
        E = np.where(f <= 0.875, e - 9, e - 8)
    else:
        E = np.where(f < 0.875, e - 10, e - 9)              # floor(log2(amax / 448))
    E = np.where(amax > 0, E, -(1 << 20))
    return np.clip(E, lo, 127)


def e4m3_rne(y, rint=np.rint, return_ties=False):
    """fp64 |y| <= 448 -> OCP e4m3 bytes (uint8): the grid step is 2^(e-3) for |y| in [2^e, 2^(e+1)), e >= -6, and 2^-9 below
    2^-6; ``rint`` (round-half-even) to that grid, then re-encoded.  ``return_ties``: also the mask of exact ties."""
    y = np.asarray(y, dtype=np.float64)
    a = np.abs(y)
    assert bool((a <= 448).all()), "e4m3_rne: |y| must not exceed 448"
    _, e = np.frexp(a)
    eu = np.where(a > 0, np.maximum(e.astype(np.int64) - 1, -6), -6)     # a = 1.m 2^eu, subnormals share -6
    t = np.ldexp(a, 3 - eu)                                 # in [8, 16) for normals, [0, 8) below 2^-6: exact
    q = rint(t).astype(np.int64)                            # 0..16; 16 is the next binade's 8
    code = ((eu + 7) << 3) + q - 8                          # exponent field eu + 7, q - 8 mantissa bits; q < 8 only at eu == -6
    out = (code | np.where(np.signbit(y), 0x80, 0)).astype(np.uint8)
    if return_ties:
        return out, (t - np.floor(t)) == 0.5
    return out


_mag = np.arange(128)
_E4M3 = np.ldexp(((_mag & 7) + np.where(_mag >> 3 > 0, 8, 0)).astype(np.float64), np.maximum(_mag >> 3, 1) - 10)
_E4M3[0x7F] = np.nan
E4M3_TABLE = np.concatenate([_E4M3, -_E4M3])               # the value of every byte; 0x7F and 0xFF are NaN
FINITE_CODES = np.array([b for b in range(256) if b & 0x7F != 0x7F], dtype=np.uint8)


def dequant(q, s):
    """(bytes [..., K], scale bytes [..., K/32]) -> fp64 [..., K]."""
    q, s = np.asarray(q), np.asarray(s)
    v = E4M3_TABLE[q].reshape(*s.shape, BLOCK)
    return np.ldexp(v, (s.astype(np.int64) - 127)[..., None]).reshape(q.shape)


def quantize(bits, shared_exp=shared_exp, e4m3_rne=e4m3_rne, return_ties=False):
    """bf16 patterns [..., K] (finite) -> (e4m3 bytes [..., K], scale bytes [..., K/32], dequantised fp64 [..., K])."""
    bits = np.asarray(bits)
    assert bits.shape[-1] % BLOCK == 0
    x = bf16_to_f64(bits).reshape(*bits.shape[:-1], bits.shape[-1] // BLOCK, BLOCK)
    assert bool(np.isfinite(x).all()), "quantize: finite inputs only"
    E = shared_exp(np.abs(x).max(-1))
    y = np.ldexp(x, -E[..., None])
    q, ties = e4m3_rne(y, return_ties=True)
    q = q.reshape(bits.shape)
    s = (E + 127).astype(np.uint8)
    if return_ties:
        return q, s, dequant(q, s), ties.reshape(bits.shape)
    return q, s, dequant(q, s)


def same_codes(a, b):
    """Element-wise equality of e4m3 bytes with 0x00 and 0x80 (the same value) taken as equal."""
    a, b = np.asarray(a), np.asarray(b)
    return (a == b) | (((a & 0x7F) == 0) & ((b & 0x7F) == 0))


# ------------------------------------------------------------------ the shared input
def sweep_exponents(subsample=False, lo=0, hi=254):
    """Exponent fields of the sweep's pivots: all of lo..hi, or the 1-in-4 subsample that keeps 0, 1, 8, 9 and 254 (zero
    and subnormal inputs, both sides of the shared-exponent clamp, the largest binade)."""
    ex = [e for e in range(lo, hi + 1) if not subsample or e % 4 == 0 or e in (0, 1, 8, 9, 254)]
    return tuple(ex)


@functools.lru_cache(maxsize=None)
def pivot_sweep(exps=None):
    """uint16 [rows, 256] (read-only): for every pivot pattern (ex << 7) | m, ex in ``exps`` (default 0..254), m in PIVOT_M,
    blocks of 32 that hold the pivot at a position cycling through 0..31 (every lane of a four-lane reduction gets the
    maximum) and 31 of the patterns below it: every magnitude of the 20 binades under the pivot (2560 patterns, fewer next
    to zero), both signs, in order, so |v| <= pivot throughout; the last block of a pivot is filled up with zeros.  Rows are
    padded with zero blocks to a multiple of 64."""
    exps = sweep_exponents() if exps is None else exps
    blocks = []
    pos = 0
    for ex in exps:
        for m in PIVOT_M:
            p = (ex << 7) | m
            mags = np.arange(max(0, p - 128 * BINADES_BELOW), p, dtype=np.int64)
            vals = np.stack([mags, mags | 0x8000], axis=1).reshape(-1)      # +v, -v, ascending magnitude
            nb = max(1, -(-len(vals) // (BLOCK - 1)))
            fill = np.zeros(nb * (BLOCK - 1), dtype=np.int64)
            fill[:len(vals)] = vals
            fill = fill.reshape(nb, BLOCK - 1)
            blk = np.empty((nb, BLOCK), dtype=np.int64)
            at = (pos + np.arange(nb)) % BLOCK
            pos += nb
            cols = np.arange(BLOCK)[None, :]
            blk[cols == at[:, None]] = p
            blk[cols != at[:, None]] = fill.reshape(-1)
            blocks.append(blk)
    flat = np.concatenate(blocks).reshape(-1)
    per = ROW * ROW_MULTIPLE
    out = np.zeros(-(-len(flat) // per) * per, dtype=np.uint16)
    out[:len(flat)] = flat
    out = out.reshape(-1, ROW)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def pivot_sweep_ref(exps=None):
    """quantize(pivot_sweep(exps)) with the tie mask, computed once and shared (read-only)."""
    ref = quantize(pivot_sweep(exps), return_ties=True)
    for a in ref:
        a.setflags(write=False)
    return ref
