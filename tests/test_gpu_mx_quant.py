"""The five bf16 -> MX-fp8 quantisers and the MX-fp8 GEMM's decode against tests/mx_emul.py, bit for bit (-m gpu).  Every
comparison is with the host emulator (proved in test_cpu_mx_emul.py), never with another kernel; 0x00 and 0x80, the same
value, are the only element the comparison discounts.

What each test pins:

  vlb_quantize_mxfp8 (the inline frexpf rule of quantize_mxfp8_kernel, v_cvt_pk_fp8_f32)
    * test_every_amax_to_scale_byte: the scale byte of all 32640 finite amax values - the 448 2^k boundary (f == 0.5f),
      the clamp at -127, bf16-subnormal amax (an fp32-subnormal quotient), the top binade - and the element at the maximum
    * test_pivot_sweep_rowwise: round-half-even ties (241 k of them), the e4m3 subnormal range, flushes to zero, every
      finite code and every scale byte 0..247, the block maximum at each of the 32 positions
    * test_non_finite_inputs
  vlb_transpose_quantize_mxfp8 (mx_shared_exp / mx_pack4 through tq_quantize_pair, tq_stage_and_store)
    * test_every_amax_to_scale_byte, test_pivot_sweep_transposed_and_dual: the same rule through the second spelling
    * test_transpose_layout_edges: ragged R (1..200), the scalar column tail (C % 8 != 0), C < one tile and two tiles,
      Rpad / 32 not a multiple of 4 (byte-wise scale store, nb < 4 last tile), a whole tile of padding rows (bytes 0,
      scale byte 0), a scale base one byte off 4-byte alignment, ldq > Rpad, ldx > C, nothing written outside
    * test_non_finite_inputs
  vlb_quantize_dual_mxfp8 (both outputs)
    * test_every_amax_to_scale_byte, test_pivot_sweep_transposed_and_dual, test_dual_layout_edges, test_non_finite_inputs
  vlb_rmsnorm_fwd_mxfp8, vlb_swiglu_fwd_mxfp8 (mx_quantize_lane8: the four-lane amax reduction, the lane-0 scale store)
    * test_fused_producers: the emulator applied to the device's own bf16 output (no assumption about rsqrt / silu),
      outputs over more than 200 binades, all-zero blocks, the maximum in each of the four lanes; one-block rows (dim 32),
      a partly filled wave (dim 96), the 8-pass kernel (dim 4096); plus the equality with the separate kernels
    * test_non_finite_inputs
  vlb_gemm_mxfp8 (the decode inside v_mfma_scale_f32_16x16x128_f8f6f4)
    * test_quantise_then_gemm_reads_out_every_code: every finite code x scale bytes 19..220 through the MFMA against an
      identity, forward (row-wise quantiser) and wgrad (transposed quantiser on both operands, padded K)
    * test_gemm_wide_scales_bit_exact: scale bytes 27..227 that differ per K block and per operand but cancel in the
      product - a scale byte taken from the wrong K block or the wrong operand moves the result by a power of two - on
      the 256-row tile, the 192-row tile and the re-cut halves
    * test_non_finite_inputs: a non-finite operand row gives a non-finite output row and disturbs no other row

Non-finite contract: a NaN or Inf input never becomes a finite fp8 value - its byte is 0x7F or
0xFF; the scale byte and the finite neighbours of its block are unspecified; every other block is unaffected.
"""
import numpy as np
import pytest
import torch

import exact_ints as E
import mx_emul as mx
from test_gpu_exact_contractions import MXFP8

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
FILL = 0x55


def _bf(bits, dev):
    """uint16 patterns (numpy) -> bf16 tensor on the device."""
    return torch.from_numpy(np.array(bits, dtype=np.uint16).view(np.int16)).view(BF).to(dev)      # a copy: the sweep is read-only


def _bits(t):
    """bf16 tensor -> uint16 patterns (numpy)."""
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _np(t):
    return t.cpu().numpy()


def _assert_equals_emulator(q, s, ref_q, ref_s, what):
    q, s = _np(q), _np(s)
    assert q.shape == ref_q.shape and s.shape == ref_s.shape, (what, q.shape, ref_q.shape, s.shape, ref_s.shape)
    bad_s = s != ref_s
    assert not bad_s.any(), f"{what}: {int(bad_s.sum())} scale bytes differ; first at {tuple(np.argwhere(bad_s)[0])}: " \
                            f"got {int(s[bad_s][0])} want {int(ref_s[bad_s][0])}"
    bad = ~mx.same_codes(q, ref_q)
    assert not bad.any(), f"{what}: {int(bad.sum())} bytes differ; first at {tuple(np.argwhere(bad)[0])}: " \
                          f"got {int(q[bad][0]):#04x} want {int(ref_q[bad][0]):#04x}"


def _transposed_ref(bits, Rpad):
    """The emulator on x^T with rows R..Rpad-1 of x taken as zero: (q [C, Rpad], s [C, Rpad/32], deq)."""
    R, C = bits.shape
    xt = np.zeros((C, Rpad), dtype=np.uint16)
    xt[:, :R] = bits.T
    return mx.quantize(xt)


def _run_transposed(ops, x, Rpad):
    C = x.shape[1]
    q = torch.full((C, Rpad), FILL, dtype=torch.uint8, device=x.device)
    s = torch.full((C, Rpad // 32), FILL, dtype=torch.uint8, device=x.device)
    return ops.transpose_quantize_mxfp8(x, q, s, Rpad)


def _run_dual(ops, x, Rpad):
    R, C = x.shape
    dev = x.device
    q = torch.full((R, C), FILL, dtype=torch.uint8, device=dev); s = torch.full((R, C // 32), FILL, dtype=torch.uint8, device=dev)
    qt = torch.full((C, Rpad), FILL, dtype=torch.uint8, device=dev); st = torch.full((C, Rpad // 32), FILL, dtype=torch.uint8, device=dev)
    return ops.quantize_dual_mxfp8(x, q, s, qt, st, Rpad)


# ------------------------------------------------------------------ a. every amax -> scale byte
def test_every_amax_to_scale_byte(dev):
    """One block per finite non-negative bf16 value, the value at a rotating position, the rest zero."""
    from phantom_vlb_amd import ops
    n = 0x7F80
    blocks = np.zeros((n, 32), dtype=np.uint16)
    blocks[np.arange(n), np.arange(n) % 32] = np.arange(n, dtype=np.uint16)
    bits = blocks.reshape(n // 8, 256)                                  # [4080, 256]
    ref_q, ref_s, _ = mx.quantize(bits)
    assert set(ref_s.reshape(-1).tolist()) == set(range(248))
    x = _bf(bits, dev)
    _assert_equals_emulator(*ops.quantize_mxfp8(x), ref_q, ref_s, "quantize")
    # the transposed arrangement: x^T [256, 4080] -> q [4080, 256], the same blocks
    xt = x.t().contiguous()
    _assert_equals_emulator(*_run_transposed(ops, xt, 256), ref_q, ref_s, "transpose_quantize")
    # dual, x as it is: the row-wise output sees the blocks, the transposed one their columns (several values a block)
    q, s, qt, st = _run_dual(ops, x, n // 8 + 16)
    _assert_equals_emulator(q, s, ref_q, ref_s, "dual row-wise")
    _assert_equals_emulator(qt, st, *_transposed_ref(bits, n // 8 + 16)[:2], "dual transposed (columns)")
    # dual on the transposed arrangement (C padded to 4096 with zero columns): the transposed output sees the blocks
    bits_t = np.zeros((256, 4096), dtype=np.uint16)
    bits_t[:, :n // 8] = bits.T
    q, s, qt, st = _run_dual(ops, _bf(bits_t, dev), 256)
    _assert_equals_emulator(qt[:n // 8], st[:n // 8], ref_q, ref_s, "dual transposed")
    assert not bool(qt[n // 8:].any()) and not bool(st[n // 8:].any())
    _assert_equals_emulator(q, s, *mx.quantize(bits_t)[:2], "dual row-wise (rows of x^T)")


# ------------------------------------------------------------------ b. the pivot sweep
def test_pivot_sweep_rowwise(dev):
    from phantom_vlb_amd import ops
    bits = mx.pivot_sweep()
    ref_q, ref_s, _, _ = mx.pivot_sweep_ref()
    _assert_equals_emulator(*ops.quantize_mxfp8(_bf(bits, dev)), ref_q, ref_s, "quantize")


def test_pivot_sweep_transposed_and_dual(dev):
    from phantom_vlb_amd import ops
    exps = mx.sweep_exponents(subsample=True)
    bits = mx.pivot_sweep(exps)
    ref_q, ref_s, _, _ = mx.pivot_sweep_ref(exps)
    rows = bits.shape[0]
    assert rows % 64 == 0
    x = _bf(bits, dev)
    xt = x.t().contiguous()                                             # [256, rows]: its transposed quantisation is the sweep's
    _assert_equals_emulator(*_run_transposed(ops, xt, 256), ref_q, ref_s, "transpose_quantize")
    q, s, qt, st = _run_dual(ops, xt, 256)
    _assert_equals_emulator(qt, st, ref_q, ref_s, "dual transposed")
    _assert_equals_emulator(q, s, *mx.quantize(np.ascontiguousarray(bits.T))[:2], "dual row-wise (rows of x^T)")
    q, s, qt, st = _run_dual(ops, x, rows)
    _assert_equals_emulator(q, s, ref_q, ref_s, "dual row-wise")
    _assert_equals_emulator(qt, st, *_transposed_ref(bits, rows)[:2], "dual transposed (columns)")


# ------------------------------------------------------------------ c. layout edges
EDGE_R = (1, 31, 32, 33, 127, 128, 129, 200)


def _rpads(R):
    r32, r128 = -(-R // 32) * 32, -(-R // 128) * 128
    return tuple(dict.fromkeys((r32, r128, r32 + 128)))                 # the last: a whole tile of padding rows


def _edge_values(R, C, salt):
    """[R, C] patterns whose columns are the leading R elements of sweep rows: blocks along R are the sweep's own."""
    sw = mx.pivot_sweep(mx.sweep_exponents(subsample=True))
    rows = (np.arange(C) * 97 + 1013 * salt + 40) % sw.shape[0]
    return np.ascontiguousarray(sw[rows, :R].T)


def _framed_input(bits, dev):
    """x [R, C] as a strided view (ldx > C, one guard row above and below, 8 guard columns left) of a buffer of 0x5555."""
    R, C = bits.shape
    ldx = -(-C // 8) * 8 + 16
    buf = torch.full((R + 2, ldx), FILL * 0x0101, dtype=torch.int16, device=dev)
    x = buf.view(BF)[1:R + 1, 8:8 + C]
    x.copy_(_bf(bits, dev))
    return x


def _framed_out(rows, cols, ld, lead, dev):
    """uint8 [rows, cols] view with row stride ld and `lead` bytes in front, inside a 0x55 buffer; returns (view, buffer)."""
    buf = torch.full((lead + (rows + 1) * ld + 64,), FILL, dtype=torch.uint8, device=dev)
    return buf[lead:].as_strided((rows, cols), (ld, 1)), buf


def _assert_frame_untouched(view, buf, what):
    """Every byte of buf outside view still holds 0x55."""
    chk = buf.clone()
    chk[view.data_ptr() - buf.data_ptr():].as_strided(view.shape, view.stride()).fill_(FILL)
    assert bool((chk == FILL).all()), f"{what}: {int((chk != FILL).sum())} bytes written outside the output"


def _scale_layouts(nblk):
    """(lds, lead): contiguous and aligned; 4-byte multiple stride on a base one byte off alignment; odd stride."""
    return ((nblk, 16), (-(-nblk // 4) * 4 + 4, 17), (nblk + 3 - nblk % 2, 16))


@pytest.mark.parametrize("R", EDGE_R)
def test_transpose_layout_edges(dev, R):
    from phantom_vlb_amd import ops
    for C in (4, 64, 72, 128, 136, 200):
        bits = _edge_values(R, C, R)
        x = _framed_input(bits, dev)
        for Rpad in _rpads(R):
            ref_q, ref_s, _ = _transposed_ref(bits, Rpad)
            if Rpad - R >= 128:
                assert not ref_q[:, -128:].any() and not ref_s[:, -4:].any()
            for il, (lds, lead) in enumerate(_scale_layouts(Rpad // 32)):
                q, qbuf = _framed_out(C, Rpad, Rpad + 16 * (1 + il), 32, dev)
                s, sbuf = _framed_out(C, Rpad // 32, lds, lead, dev)
                assert q.data_ptr() % 16 == 0 and s.data_ptr() % 4 == lead % 4
                ops.transpose_quantize_mxfp8(x, q, s, Rpad)
                what = f"R={R} C={C} Rpad={Rpad} lds={lds} lead={lead}"
                _assert_equals_emulator(q, s, ref_q, ref_s, what)
                _assert_frame_untouched(q, qbuf, what + " q")
                _assert_frame_untouched(s, sbuf, what + " s")


@pytest.mark.parametrize("R", EDGE_R)
def test_dual_layout_edges(dev, R):
    from phantom_vlb_amd import ops
    for C in (64, 128, 192):
        bits = _edge_values(R, C, R + 7)
        x = _framed_input(bits, dev)
        row_q, row_s, _ = mx.quantize(bits)
        for Rpad in _rpads(R):
            ref_q, ref_s, _ = _transposed_ref(bits, Rpad)
            for il, (lds, lead) in enumerate(_scale_layouts(Rpad // 32)):
                q, qbuf = _framed_out(R, C, C + 16 * (1 + il), 16, dev)
                s, sbuf = _framed_out(R, C // 32, C // 32 + 1 + il, 1 + il, dev)
                qt, qtbuf = _framed_out(C, Rpad, Rpad + 16 * (1 + il), 32, dev)
                st, stbuf = _framed_out(C, Rpad // 32, lds, lead, dev)
                ops.quantize_dual_mxfp8(x, q, s, qt, st, Rpad)
                what = f"R={R} C={C} Rpad={Rpad} lds={lds} lead={lead}"
                _assert_equals_emulator(q, s, row_q, row_s, what + " row-wise")
                _assert_equals_emulator(qt, st, ref_q, ref_s, what + " transposed")
                for v, b, n in ((q, qbuf, "q"), (s, sbuf, "s"), (qt, qtbuf, "qt"), (st, stbuf, "st")):
                    _assert_frame_untouched(v, b, f"{what} {n}")


# ------------------------------------------------------------------ d. fused producers
FUSED_SHAPES = [(rows, dim) for rows in (1, 77) for dim in (32, 64, 96, 4096)]


def _block_exponents(rows, nblk, lo, hi, seed):
    """An exponent per (row, block), spread over lo..hi; and which blocks are zeroed."""
    rng = np.random.RandomState(seed)
    e = lo + (np.arange(rows * nblk) * 37 % (hi - lo + 1)).reshape(rows, nblk)
    zero = rng.rand(rows, nblk) < 0.1
    return e, zero


def _peaked(rows, dim, seed):
    """Magnitudes in [1, 2) with one element of every block raised 64-fold, at position (7 row + 11 block) % 32: the block
    maximum visits every lane of the four that share a block."""
    rng = np.random.RandomState(seed)
    v = 1 + rng.randint(0, 128, size=(rows, dim // 32, 32)) / 128.0
    r, b = np.meshgrid(np.arange(rows), np.arange(dim // 32), indexing="ij")
    at = (7 * r + 11 * b) % 32
    np.put_along_axis(v, at[..., None], 64 * np.take_along_axis(v, at[..., None], 2), 2)
    return v


def _spread(y_bits):
    """(binades spanned by the non-zero outputs, number of all-zero blocks, lanes (of four) that held a block maximum)."""
    mag = (y_bits.reshape(-1, 32) & 0x7FFF).astype(np.int64)
    assert bool((mag < 0x7F80).all()), "non-finite producer output"
    live = mag.max(1) > 0
    ex = mag[mag > 0] >> 7
    lanes = set((mag[live].argmax(1) // 8).tolist())
    return (int(ex.max() - ex.min()) + 1 if len(ex) else 0), int((~live).sum()), lanes


def _check_fused(producer, y, q, s, y0, stats):
    from phantom_vlb_amd import ops
    yb = _bits(y)
    stats.append(yb.reshape(-1))
    ref_q, ref_s, _ = mx.quantize(yb)
    _assert_equals_emulator(q, s, ref_q, ref_s, f"{producer} {tuple(y.shape)}")
    q0, s0 = ops.quantize_mxfp8(y0)
    assert torch.equal(y, y0) and torch.equal(q, q0) and torch.equal(s, s0), (producer, tuple(y.shape))


def _assert_spread(producer, stats, shape=None):
    binades, zero_blocks, lanes = _spread(np.concatenate(stats) if shape is None else stats[-1])
    print(f"{producer} {shape or 'all shapes'}: {binades} binades, {zero_blocks} all-zero blocks, lanes {sorted(lanes)}")
    assert binades >= 200 and zero_blocks > 0 and lanes == {0, 1, 2, 3}, (producer, shape, binades, zero_blocks, lanes)


def test_fused_producers(dev):
    """y = w * bf16(x * rstd) with rows of x scaled 2^0 .. 2^-100 (below sqrt(eps) the row scale survives the norm) and a
    weight exponent per block; h = silu(gate) * up with |gate| in [0.5, 2] and an exponent per (row, block) in `up`.  The
    spread (>= 200 binades, all-zero blocks, the maximum in each of the four lanes) is asserted on the device's output -
    over all eight shapes together, and on each 77-row 4096-column case alone; a 32-column row is a single block."""
    from phantom_vlb_amd import ops
    stats = []
    for rows, dim in FUSED_SHAPES:
        nblk = dim // 32
        rng = np.random.RandomState(rows * 131 + dim)
        row_e = -(np.arange(rows) * 100 // max(rows - 1, 1)) if rows > 1 else np.array([-(dim // 32 % 50)])
        xv = _peaked(rows, dim, rows + dim) * rng.choice([-1.0, 1.0], size=(rows, nblk, 32))
        xv = np.ldexp(xv, row_e[:, None, None])
        if rows > 3:
            xv[3] = 0                                                   # a row of zeros: rstd = 1/sqrt(eps), y = 0
        w_e, w_zero = _block_exponents(1, nblk, -20, 100, dim)
        wv = np.ldexp(1 + rng.randint(0, 128, size=(nblk, 32)) / 128.0, w_e[0][:, None])
        wv[w_zero[0] & (np.arange(nblk) > 0)] = 0
        x = _bf(mx.f64_to_bf16_bits(xv.reshape(rows, dim)), dev)
        w = _bf(mx.f64_to_bf16_bits(wv.reshape(dim)), dev)
        y, q, s = ops.rmsnorm_mxfp8(x, w, 1e-5)
        _check_fused("rmsnorm_mxfp8", y, q, s, ops.rmsnorm(x, w, 1e-5), stats)
        if (rows, dim) == (77, 4096):
            _assert_spread("rmsnorm_mxfp8", stats, (rows, dim))
    _assert_spread("rmsnorm_mxfp8", stats)
    stats = []
    for rows, ff in FUSED_SHAPES:
        nblk = ff // 32
        rng = np.random.RandomState(rows * 137 + ff)
        gate = rng.choice([-1.0, 1.0], size=(rows, ff)) * (0.5 + rng.randint(0, 193, size=(rows, ff)) / 128.0)
        u_e, u_zero = _block_exponents(rows, nblk, -105, 105, ff + rows)
        up = np.ldexp(_peaked(rows, ff, rows + ff + 1) * rng.choice([-1.0, 1.0], size=(rows, nblk, 32)), u_e[..., None])
        up[u_zero & (np.arange(rows * nblk).reshape(rows, nblk) > 0)] = 0
        gu = _bf(mx.f64_to_bf16_bits(np.concatenate([gate, up.reshape(rows, ff)], axis=1)), dev)
        h, q, s = ops.swiglu_mxfp8(gu)
        _check_fused("swiglu_mxfp8", h, q, s, ops.swiglu(gu), stats)
        if (rows, ff) == (77, 4096):
            _assert_spread("swiglu_mxfp8", stats, (rows, ff))
    _assert_spread("swiglu_mxfp8", stats)


# ------------------------------------------------------------------ e. quantise -> GEMM read-out
def _exact_bf16_image(deq):
    """fp64 values of at most 4 significant bits (asserted) -> the bf16 tensor that holds them exactly."""
    f32 = deq.astype(np.float32)
    assert bool((f32.astype(np.float64) == deq).all())
    raw = f32.view(np.uint32)
    assert bool(((raw & 0xFFFFF) == 0).all()), "more than 4 significant bits"
    assert bool((((raw >> 23) & 0xFF) > 0)[deq != 0].all()), "an fp32-subnormal product"
    return torch.from_numpy((raw >> 16).astype(np.uint16).view(np.int16)).view(BF)


def _assert_same_values(out, want, what):
    """bf16 tensors equal as values (+0 == -0; any NaN fails)."""
    out, want = out.float().cpu(), want.float().cpu()
    bad = ~(out == want)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} entries differ; first at {tuple(bad.nonzero()[0].tolist())}: " \
                                f"got {float(out[bad][0])!r} want {float(want[bad][0])!r}"


def test_quantise_then_gemm_reads_out_every_code(dev):
    from phantom_vlb_amd import ops
    exps = mx.sweep_exponents(lo=27, hi=227)                            # pivots in [2^-100, 2^100]
    bits = mx.pivot_sweep(exps)
    ref_q, ref_s, deq, _ = mx.pivot_sweep_ref(exps)
    assert set(ref_q.reshape(-1).tolist()) == set(mx.FINITE_CODES.tolist()) and set(ref_s.reshape(-1).tolist()) >= set(range(19, 221))
    eye = torch.eye(256, dtype=BF, device=dev)
    wq, sw = ops.quantize_mxfp8(eye)
    on = torch.eye(256, dtype=torch.bool, device=dev)
    blk_on = on.view(256, 8, 32).any(-1)
    assert bool((wq[on] == 0x78).all()) and bool((wq[~on] == 0).all()) and bool((sw[blk_on] == 119).all()) and bool((sw[~blk_on] == 0).all())
    # forward: dequant(A) . I
    aq, sa = ops.quantize_mxfp8(_bf(bits, dev))
    _assert_equals_emulator(aq, sa, ref_q, ref_s, "quantize")
    _assert_same_values(ops.gemm_mxfp8(aq, sa, wq, sw), _exact_bf16_image(deq), "forward read-out")
    # wgrad: dy^T . x over R = 200 rows padded to 256, both operands from the transposed quantiser
    R, Rpad = 200, 256
    dy_bits = np.ascontiguousarray(bits[np.arange(R) * (bits.shape[0] // R)])
    dq_ref, ds_ref, d_deq = _transposed_ref(dy_bits, Rpad)
    xd = torch.zeros(R, 256, dtype=BF, device=dev)
    xd[torch.arange(R), torch.arange(R)] = 1
    dq, ds = _run_transposed(ops, _bf(dy_bits, dev), Rpad)
    xq, xs = _run_transposed(ops, xd, Rpad)
    _assert_equals_emulator(dq, ds, dq_ref, ds_ref, "transpose_quantize(dy)")
    assert bool((xq[:R, :R][on[:R, :R]] == 0x78).all()) and int((xq != 0).sum()) == R and int((xs == 119).sum()) == R and int((xs != 0).sum()) == R
    out = ops.gemm_mxfp8(dq, ds, xq, xs)
    _assert_same_values(out[:, :R], _exact_bf16_image(d_deq[:, :R]), "wgrad read-out")
    assert not bool(out[:, R:].any()) and not bool(d_deq[:, R:].any())


# ------------------------------------------------------------------ f. GEMM with wide scales
CODES = (0x00, 0x38, 0xB8)                                              # 0, +1, -1
D_RANGE = 80                                                            # |d_kb| <= 80: scale bytes 27..227


def _wide_operand(rows, K, seed, dev, d, sign):
    """Codes for 0 / +-1, scale byte row_exp[row] + sign * d[kb] with row_exp in 127 +- 20; one block in eight all-zero
    with scale byte 0.  Returns (q, s, integer values with the zeroed blocks applied [rows, K], row_exp - 127)."""
    v = E.small_ints((rows, K), -1, 1, seed, dev, dtype=torch.int64)
    row_e = E.small_ints((rows, 1), 107, 147, seed + 1, dev, dtype=torch.int64)
    dead = E.small_ints((rows, K // 32), 0, 7, seed + 2, dev, dtype=torch.int64) == 0
    v = (v.view(rows, K // 32, 32) * (~dead)[..., None]).view(rows, K)
    q = torch.tensor(CODES, dtype=torch.uint8, device=dev)[v % 3]
    s = torch.where(dead, torch.zeros_like(row_e), row_e + sign * d[None, :]).to(torch.uint8)
    return q.contiguous(), s.contiguous(), v.float(), (row_e - 127).double()


@pytest.mark.parametrize("M,N,K", MXFP8, ids=["x".join(map(str, c)) for c in MXFP8])
def test_gemm_wide_scales_bit_exact(dev, M, N, K):
    """sa[m, kb] = a_m + d_kb and sw[n, kb] = w_n - d_kb: every block product carries 2^(a_m + w_n - 254), so the exact
    result is (an integer of magnitude <= K) * 2^(a_m + w_n - 254) and the output its bf16 round-to-nearest-even."""
    from phantom_vlb_amd import ops
    seed = 5000 + M + 2 * N + 3 * K
    d = E.small_ints((K // 32,), -D_RANGE, D_RANGE, seed, dev, dtype=torch.int64)
    if K // 32 >= 2:
        d[0], d[-1] = D_RANGE, -D_RANGE
    aq, sa, av, ae = _wide_operand(M, K, seed + 10, dev, d, +1)
    wq, sw, wv, we = _wide_operand(N, K, seed + 20, dev, d, -1)
    assert 27 <= int(sa[sa > 0].min()) and int(sa.max()) <= 227 and 27 <= int(sw[sw > 0].min()) and int(sw.max()) <= 227
    ints = av @ wv.t()                                                  # integers of magnitude <= K: exact in fp32
    rows = torch.as_tensor(E.row_subsample(M, seed), device=dev)
    assert torch.equal(ints[rows].double().cpu(), av[rows].double().cpu() @ wv.double().cpu().t())
    exact = ints.double() * torch.exp2(ae) * torch.exp2(we).t()
    out = torch.full((M, N), 7.0, dtype=BF, device=dev)
    E.assert_bits_equal(ops.gemm_mxfp8(aq, sa, wq, sw, out=out), exact, cap=False)


# ------------------------------------------------------------------ g. non-finite inputs
NAN, PINF, NINF = 0x7FC0, 0x7F80, 0xFF80


def _non_finite_case():
    """(finite patterns [64, 256], the same with NaN / +Inf / -Inf put in, [(row, col)] of those)."""
    sw = mx.pivot_sweep(mx.sweep_exponents(lo=120, hi=134))
    base = np.ascontiguousarray(sw[np.arange(64) * (sw.shape[0] // 64)])
    mag = (base & 0x7FFF).astype(np.int64)
    spots = [(3, 5, NAN), (10, 40, PINF), (20, 100, NINF), (21, 255, NAN), (40, 0, PINF)]
    for row, blk, pat in ((30, 2, NAN), (31, 5, PINF), (33, 7, NINF)):  # at the position that sets the block's amax
        spots.append((row, blk * 32 + int(mag[row, blk * 32:blk * 32 + 32].argmax()), pat))
    bad = base.copy()
    for r, c, pat in spots:
        bad[r, c] = pat
    return base, bad, [(r, c) for r, c, _ in spots]


def _assert_non_finite_rule(q, s, ref_q, ref_s, hit, what):
    """hit: bool [rows, K] of the non-finite inputs.  Their bytes are NaN codes; every block without one equals the emulator."""
    q, s = _np(q), _np(s)
    assert bool(((q[hit] & 0x7F) == 0x7F).all()), f"{what}: non-finite inputs became {[hex(b) for b in q[hit]]}"
    clean = ~hit.reshape(hit.shape[0], -1, 32).any(-1)
    assert bool((s[clean] == ref_s[clean]).all()), what
    assert bool(mx.same_codes(q, ref_q).reshape(hit.shape[0], -1, 32)[clean].all()), what


def test_non_finite_inputs(dev):
    from phantom_vlb_amd import ops
    base, bad, spots = _non_finite_case()
    hit = np.zeros(base.shape, dtype=bool)
    for r, c in spots:
        hit[r, c] = True
    ref_q, ref_s, _ = mx.quantize(base)
    x = _bf(bad, dev)
    q, s = ops.quantize_mxfp8(x)
    _assert_non_finite_rule(q, s, ref_q, ref_s, hit, "quantize")
    xt = x.t().contiguous()
    _assert_non_finite_rule(*_run_transposed(ops, xt, 256), ref_q, ref_s, hit, "transpose_quantize")
    dq, ds, dqt, dst = _run_dual(ops, xt, 256)
    _assert_non_finite_rule(dqt, dst, ref_q, ref_s, hit, "dual transposed")
    _assert_non_finite_rule(dq, ds, *mx.quantize(np.ascontiguousarray(base.T))[:2], np.ascontiguousarray(hit.T), "dual row-wise")
    # the fused producers: wherever their own bf16 output is non-finite
    w = torch.ones(256, dtype=BF, device=dev)
    gu = torch.cat([torch.ones(64, 256, dtype=BF, device=dev), x], dim=1)
    for name, (y, fq, fs) in (("rmsnorm_mxfp8", ops.rmsnorm_mxfp8(x, w, 1e-5)), ("swiglu_mxfp8", ops.swiglu_mxfp8(gu))):
        yb = _bits(y)
        y_hit = (yb & 0x7F80) == 0x7F80
        assert bool(y_hit[hit].all()), name
        y_ref = mx.quantize(np.where(y_hit, 0, yb).astype(np.uint16))
        _assert_non_finite_rule(fq, fs, y_ref[0], y_ref[1], y_hit, name)
    # the GEMM: rows with a non-finite element come out non-finite, every other row keeps the bits of the all-finite run
    wq, sw = ops.quantize_mxfp8(_bf(np.ascontiguousarray(mx.pivot_sweep(mx.sweep_exponents(lo=126, hi=128))[:256]), dev))
    good = ops.gemm_mxfp8(*ops.quantize_mxfp8(_bf(base, dev)), wq, sw)
    out = ops.gemm_mxfp8(q, s, wq, sw)
    rows_hit = torch.from_numpy(hit.any(1)).to(dev)
    assert bool(torch.isfinite(good).all())
    assert not bool(torch.isfinite(out[rows_hit]).any()), "a non-finite operand row gave finite outputs"
    assert torch.equal(out[~rows_hit].view(torch.int16), good[~rows_hit].view(torch.int16))
