"""fp64 restatement of the kernels that index a 2-D or 3-D neighbourhood (csrc/ops.hip, csrc/train.hip, csrc/gemm.hip), ONE
OPERATION AT A TIME, with derived per-element error bars, inputs, an fp32 restatement in the kernels' own operation order,
a restatement of the launchers' grid sizes, and planted bugs.  The shared pieces come from tests/rows_emul.py.

Arithmetic operations (-> ``(ref, bar)`` with ``*_reach`` entries, as rows_emul's stages): dwconv3x3, dwconv3x3_dx (the data
gradient: the same kernel on reversed taps), dwconv3x3_bwd_w, se_pool, se_scale, se_bwd_gate, se_bwd_x, vit_assemble.
Bit-exact operations (-> ``{name: int16 bit patterns}``, no bar): patchify (torch's fp32 -> bf16 round-to-nearest-even), and
the pure copies drop_cls, im2col3d, col2im3d, transpose, transpose_pad, splice_embed (dense layout).

Layouts: planes are channels-last [N, H, W, C]; the depthwise taps are [9, C], tap = (dy + 1) * 3 + (dx + 1) with
y[h, w] = sum x[h + dy, w + dx] * k[tap]; im2col3d's columns are [B * T2 * H2 * W2, 8, C], tap = (kt * 2 + kh) * 2 + kw.

The references are plain index arithmetic (gather indices and a validity mask per tap), so that the per-output sum|terms|
of a bar comes out of the same loop as the value; test_cpu_stencil_emul ties them to torch.nn.functional in fp64.

Bars: the rule of rows_emul.  An fp32 sum of terms gets c * 2^-24 * sum|terms| + 2^-22 * |ref|, c = the longest chain of
additions one output goes through + 2 (each ``c_*`` says which loop it counts); a product of two bf16 values is exact in
fp32; a division gets 1 + RCP units of 2^-24 (a correctly rounded one needs 1: the rest is slack, not a licence); sigmoid_f
gets rows_emul.sigmoid_err; a bf16 output adds half a bf16 ulp.  Nothing is fitted to a measurement."""
from __future__ import annotations

import functools

import numpy as np
import torch

from rows_emul import (BF16, F32, F64, HB, R, RCP, TINY, U, _bf, _gen, _np, bf16_out, cdiv, colpart_reduce32, f32, f64, outside, ratio,  # noqa: F401
                       ratios, rbf, reach, row_exp, sigmoid32, sigmoid_err)

I16, I64 = torch.int16, torch.int64
K_MAX_BLOCKS = 256 * 8          # ops.hip: kMaxBlocks, the grid cap of grid_for
LDS_LIMIT = 160 * 1024          # ops.hip: vlb_dwconv3x3 refuses a plane above it
GATE_EDGES = (0.0, -0.0, 20.0, -20.0, 88.5, -88.5, 90.0, -90.0)        # as rows_emul._swiglu_inputs


def sid(shape):
    return "x".join(str(int(v)) for v in shape)


# ---------------------------------------------------------------------------------------------------- launch geometry
def _stride(total):
    """a grid-stride kernel launched through grid_for(total, 256)"""
    blocks = max(1, min(cdiv(total, 256), K_MAX_BLOCKS))
    return dict(items=total, blocks=blocks, second_trip=total > blocks * 256)


def launch(op, shape):
    """what the launcher of ``op`` does at ``shape``: a restatement of the grid arithmetic in ops.hip / train.hip / gemm.hip
    (held to the source text by test_cpu_stencil_emul).  blocks_x: blockIdx.x extent; last_active: channel octets the last
    blockIdx.x block has work for; slabs: partial slabs colpart_reduce_kernel adds; lds: dynamic LDS bytes; second_trip:
    whether a thread of the capped grid walks its grid-stride loop twice."""
    if op in ("dwconv3x3", "dwconv3x3_dx"):
        N, H, W, C = shape
        lds = H * W * 64
        return dict(blocks_x=C // 32, blocks_y=N, lds=lds, above_64k=lds > 64 * 1024, refused=lds > LDS_LIMIT, position_trips=cdiv(H * W, 64))
    if op == "dwconv3x3_bwd_w":
        N, H, W, C = shape
        bx, rb = (C // 8 + 255) // 256, (9 * C + 31) // 32
        return dict(blocks_x=bx, last_active=C // 8 - (bx - 1) * 256, slabs=N * H, reduce_blocks=rb, reduce_last_active=9 * C - (rb - 1) * 32)
    if op == "se_pool":
        N, HW, C = shape
        bx = (C // 8 + 63) // 64
        return dict(blocks_x=bx, last_active=C // 8 - (bx - 1) * 64, idle_row_groups=max(0, 4 - HW))
    if op == "se_bwd_gate":
        N, HW, C = shape
        bx = (C // 8 + 255) // 256
        return dict(blocks_x=bx, last_active=C // 8 - (bx - 1) * 256)
    if op == "se_scale":
        N, HW, C = shape
        return _stride(N * HW * (C // 8))
    if op in ("se_bwd_x", "se_bwd_x_nopool"):
        N, HW, C = shape
        return dict(items=N * HW * (C // 8), blocks=cdiv(N * HW * (C // 8), 256), second_trip=False)       # blocks_for: no cap, no loop
    if op == "im2col3d":
        B, T, H, W, C = shape
        T2, H2, W2 = T // 2 + 1, H // 2 + 1, W // 2 + 1
        return dict(_stride(B * T2 * H2 * W2 * 8 * (C // 8)), out=(T2, H2, W2), trailing_pad=(T % 2 == 0, H % 2 == 0, W % 2 == 0))
    if op in ("col2im3d", "col2im3d_of_im2col"):
        B, T, H, W, C = shape
        total = B * T * H * W * (C // 8)
        return dict(items=total, blocks=cdiv(total, 256), second_trip=False, out=(T // 2 + 1, H // 2 + 1, W // 2 + 1),
                    trailing_pad=(T % 2 == 0, H % 2 == 0, W % 2 == 0))
    if op == "patchify":
        N, H, W, P, Kpad = shape
        return dict(_stride(N * (H // P) * (W // P) * (Kpad // 8)), K=3 * P * P, straddle=(3 * P * P) % 8 != 0)
    if op == "vit_assemble":
        N, G, D = shape
        return _stride(N * (G + 1) * (D // 8))
    if op == "drop_cls":
        N, G, D = shape
        return _stride(N * G * (D // 8))
    if op == "transpose_pad":
        Rr, C, ld_in, Rpad = shape
        return dict(grid=((C + 63) // 64, (Rpad + 63) // 64), scalar_tail=C % 8 != 0, pad_octets=(Rpad - cdiv(Rr, 8) * 8) // 8)
    if op == "transpose":
        Rr, C = shape
        return dict(grid=((C + 31) // 32, (Rr + 31) // 32))
    if op == "splice_embed":
        B, L, Nv, D = shape
        return dict(grid=((L - 1 + Nv + 15) // 16, B), last_rows=(L - 1 + Nv) - ((L - 1 + Nv + 15) // 16 - 1) * 16)
    raise KeyError(op)


# What a shape is there for, as LITERALS (not computed): test_cpu_stencil_emul and the GPU tests assert that ``launch`` says
# the same.  A case lists only the entries it is there for.
CASES = {
    # (N, H, W, C).  lds = H * W * 64 bytes; the plane loop ``for p`` takes position_trips trips of 64 positions
    "dwconv3x3": [((1, 1, 1, 32), dict(blocks_x=1, lds=64, position_trips=1)),
                  ((2, 1, 5, 32), dict(blocks_x=1, lds=320)),
                  ((2, 5, 1, 64), dict(blocks_x=2, lds=320)),
                  ((3, 5, 7, 96), dict(blocks_x=3, lds=2240, position_trips=1)),
                  ((1, 7, 5, 32), dict(blocks_x=1, lds=2240)),
                  ((2, 13, 13, 64), dict(blocks_x=2, lds=10816, position_trips=3)),
                  ((1, 24, 24, 32), dict(blocks_x=1, lds=36864, above_64k=False)),
                  ((1, 33, 32, 32), dict(blocks_x=1, lds=67584, above_64k=True, refused=False)),       # the reservation above 64 KB
                  ((1, 41, 63, 32), dict(lds=165312, refused=True))],                                   # 2583 positions: VlbError
    # (N, H, W, C).  blockIdx.x blocks of 256 octets; N * H slabs; colpart_reduce_kernel over 9 * C columns in blocks of 32
    "dwconv3x3_bwd_w": [((1, 1, 1, 8), dict(blocks_x=1, last_active=1, slabs=1, reduce_blocks=3, reduce_last_active=8)),
                        ((2, 7, 5, 8), dict(blocks_x=1, slabs=14)),
                        ((3, 5, 7, 72), dict(blocks_x=1, last_active=9, slabs=15, reduce_blocks=21, reduce_last_active=8)),       # 9 * C = 648
                        ((3, 6, 6, 64), dict(blocks_x=1, slabs=18, reduce_blocks=18, reduce_last_active=32)),
                        ((1, 3, 4, 2056), dict(blocks_x=2, last_active=1, slabs=3, reduce_blocks=579, reduce_last_active=8)),
                        ((9, 2, 3, 8), dict(blocks_x=1, slabs=18))],                                    # 18 slabs over 8 groups: 3, 3, 2 x 6
    # (N, HW, C).  blockIdx.x blocks of 64 octets x 4 row groups
    "se_pool": [((1, 1, 8), dict(blocks_x=1, last_active=1, idle_row_groups=3)),
                ((2, 3, 8), dict(blocks_x=1, idle_row_groups=1)),
                ((3, 35, 520), dict(blocks_x=2, last_active=1, idle_row_groups=0)),
                ((2, 169, 96), dict(blocks_x=1, last_active=12))],
    "se_bwd_gate": [((1, 1, 8), dict(blocks_x=1, last_active=1)),
                    ((3, 35, 2056), dict(blocks_x=2, last_active=1)),
                    ((2, 169, 96), dict(blocks_x=1, last_active=12))],
    "se_scale": [((1, 1, 8), dict(items=1, blocks=1, second_trip=False)),
                 ((3, 35, 520), dict(items=6825, blocks=27, second_trip=False)),
                 ((1, 1025, 4096), dict(items=524800, blocks=2048, second_trip=True))],                 # 512 items take a second trip
    "se_bwd_x": [((1, 1, 8), dict(blocks=1)), ((3, 35, 520), dict(blocks=27))],
    # (B, T, H, W, C)
    "im2col3d": [((1, 1, 1, 1, 8), dict(out=(1, 1, 1), trailing_pad=(False, False, False), second_trip=False)),
                 ((2, 3, 5, 4, 16), dict(out=(2, 3, 3), trailing_pad=(False, False, True))),
                 ((1, 4, 6, 7, 8), dict(out=(3, 4, 4), trailing_pad=(True, True, False))),
                 ((2, 8, 6, 6, 32), dict(out=(5, 4, 4), trailing_pad=(True, True, True), items=5120)),
                 ((1, 12, 24, 24, 8), dict(out=(7, 13, 13), items=9464, second_trip=False)),
                 ((1, 4, 14, 15, 4096), dict(out=(3, 8, 8), items=786432, blocks=2048, second_trip=True))],
    "col2im3d": [((1, 1, 1, 1, 8), dict(out=(1, 1, 1))),
                 ((2, 3, 5, 4, 16), dict(out=(2, 3, 3), trailing_pad=(False, False, True))),
                 ((1, 4, 6, 7, 8), dict(out=(3, 4, 4), trailing_pad=(True, True, False))),
                 ((2, 8, 6, 6, 32), dict(out=(5, 4, 4), blocks=9)),
                 ((1, 12, 24, 24, 8), dict(out=(7, 13, 13), blocks=27))],
    # (N, H, W, P, Kpad)
    "patchify": [((3, 4, 6, 2, 16), dict(K=12, straddle=True, items=36)),
                 ((1, 14, 14, 14, 592), dict(K=588, straddle=True, items=74)),
                 ((2, 28, 42, 14, 640), dict(K=588, items=960, second_trip=False)),
                 ((1, 1024, 1026, 2, 16), dict(K=12, items=525312, blocks=2048, second_trip=True))],
    # (N, G, D)
    "vit_assemble": [((1, 1, 8), dict(items=2)), ((3, 5, 24), dict(items=54)), ((2, 36, 128), dict(items=1184)),
                     ((1, 1024, 4096), dict(items=524800, blocks=2048, second_trip=True))],
    "drop_cls": [((1, 1, 8), dict(items=1)), ((3, 5, 24), dict(items=45)), ((2, 36, 128), dict(items=1152)),
                 ((1, 1025, 4096), dict(items=524800, blocks=2048, second_trip=True))],
    # (R, C, ld_in, Rpad); ld_out = Rpad + 8
    "transpose_pad": [((1, 1, 8, 8), dict(grid=(1, 1), scalar_tail=True)),
                      ((5, 13, 16, 8), dict(grid=(1, 1), scalar_tail=True, pad_octets=0)),
                      ((65, 67, 72, 72), dict(grid=(2, 2), scalar_tail=True, pad_octets=0)),
                      ((100, 77, 80, 128), dict(grid=(2, 2), scalar_tail=True, pad_octets=3)),          # rows 104 .. 127: whole octets of padding
                      ((64, 64, 64, 64), dict(grid=(1, 1), scalar_tail=False, pad_octets=0))],
    # (R, C)
    "transpose": [((1, 1), dict(grid=(1, 1))), ((33, 7), dict(grid=(1, 2))), ((31, 33), dict(grid=(2, 1))), ((300, 520), dict(grid=(17, 10)))],
    # (B, L, Nv, D): S = L - 1 + Nv = 19, two blocks of 16 rows per clip, the last with 3
    "splice_embed": [((3, 11, 9, 8), dict(grid=(2, 3), last_rows=3)), ((3, 11, 9, 264), dict(grid=(2, 3), last_rows=3))],
}
CASES["dwconv3x3_dx"] = [c for c in CASES["dwconv3x3"] if not c[1].get("refused")]
CASES["se_bwd_x_nopool"] = CASES["se_bwd_x"]
CASES["col2im3d_of_im2col"] = CASES["col2im3d"]
ARITH_OPS = ("dwconv3x3", "dwconv3x3_dx", "dwconv3x3_bwd_w", "se_pool", "se_scale", "se_bwd_gate", "se_bwd_x", "se_bwd_x_nopool", "vit_assemble")
BIT_OPS = ("patchify", "drop_cls", "im2col3d", "col2im3d", "col2im3d_of_im2col", "transpose", "transpose_pad", "splice_embed")


def shapes(op, runnable=True):
    """the shapes of an operation (without the one the launcher must refuse, unless asked)"""
    return [s for s, e in CASES[op] if not (runnable and e.get("refused"))]


# ---------------------------------------------------------------------------------------------------- inputs
CORNER = 2.0 ** 12          # one corner element per plane, far above the 2^-10 .. 2^6 of the rest


def _pos_scale(n):
    return torch.tensor([2.0 ** row_exp(p) for p in range(n)])


def _plane_inputs(shape):
    """x, dy [N * H * W, C] and w9 [9, C].  Every position carries its own scale 2^row_exp(p) (p counts through all images),
    so neighbours differ by up to 2^16 and a shifted, mirrored or transposed read lands on a value of another size; the
    TOP-RIGHT element of every x plane and the BOTTOM-LEFT of every dy plane is CORNER-sized: both move under a transpose
    and under either mirror, onto outputs whose bar is tiny.  Channels 8 .. 15 of x are zero (where C >= 16)."""
    N, H, W, C = shape
    g = _gen(N * 1000 + H, W, C, 11)
    sc = _pos_scale(N * H * W).reshape(N, H, W, 1)
    x = torch.randn(N, H, W, C, generator=g) * sc
    dy = torch.randn(N, H, W, C, generator=g) * torch.tensor([2.0 ** ((3 * p) % 5 - 2) for p in range(N * H * W)]).reshape(N, H, W, 1)
    x[:, 0, W - 1] = CORNER * (1 + torch.rand(N, C, generator=g))
    dy[:, H - 1, 0] = -CORNER * (1 + torch.rand(N, C, generator=g))
    if C >= 16:
        x[..., 8:16] = 0
    w9 = torch.randn(9, C, generator=g) * 0.3
    return dict(x=x.reshape(-1, C).to(BF16), dy=dy.reshape(-1, C).to(BF16), w9=w9.to(BF16))


def _se_inputs(shape):
    """x, dy [N * HW, C], gate logits s and dpool [N, C].  Per-position scales as the planes'; the LAST position of every image
    carries the largest scale (2^6), so that a dropped last row cannot hide below the sum's own rounding; channels 8 .. 15
    of x are zero (where C >= 16); s[0, :8] holds the gate edges."""
    N, HW, C = shape
    g = _gen(N, HW, C, 12)
    sc = _pos_scale(N * HW).reshape(N, HW, 1).clone()
    sc[:, HW - 1] = 2.0 ** 6
    x = torch.randn(N, HW, C, generator=g) * sc
    if C >= 16:
        x[..., 8:16] = 0
    dy = torch.randn(N, HW, C, generator=g) * torch.tensor([2.0 ** ((3 * p) % 5 - 2) for p in range(N * HW)]).reshape(N, HW, 1)
    s = torch.randn(N, C, generator=g) * 3
    s[0, :8] = torch.tensor(GATE_EDGES)
    dpool = torch.randn(N, C, generator=g) * 4
    return dict(x=x.reshape(-1, C).to(BF16), dy=dy.reshape(-1, C).to(BF16), s=s.to(BF16), dpool=dpool.to(BF16))


def _vit_inputs(shape):
    N, G, D = shape
    g = _gen(N, G, D, 13)
    pe = torch.randn(N * G, D, generator=g) * _pos_scale(N * G)[:, None]
    return dict(pe=pe.to(BF16), cls=torch.randn(D, generator=g).to(BF16), pos=(torch.randn(G + 1, D, generator=g) * 0.5).to(BF16))


SPECIAL_BITS = (0x8000, 0x0000, 0x0001, 0x8001, 0x007F, 0x0080, 0x7F80, 0xFF80, 0x7FC0, 0x7F81, 0xFFFF, 0x7FFF, 0xFFC1, 0x7F7F)
#               -0      +0      denormals (smallest, largest), smallest normal, +-inf, quiet / signalling NaN payloads, largest finite


def bits(shape, *key):
    """int16 tensor drawn from all 65536 bf16 bit patterns; the first and the last elements are SPECIAL_BITS"""
    n = 1
    for v in shape:
        n *= v
    v = torch.randint(0, 65536, (n,), generator=_gen(*key))
    sp = torch.tensor(SPECIAL_BITS)
    k = min(n, len(SPECIAL_BITS))
    v[:k] = sp[:k]
    if n >= 2 * len(SPECIAL_BITS):
        v[-k:] = sp
    return (v - 65536 * (v >= 32768).long()).to(I16).reshape(shape)


def _f32_from_bits(b):
    """fp32 tensor holding the given 32-bit patterns"""
    v = torch.tensor(b, dtype=I64)
    return (v - 2 ** 32 * (v >= 2 ** 31).long()).to(torch.int32).view(F32)


# fp32 values whose rounding to bf16 is decided by the tie rule or by one bit: exactly halfway above a bf16 value with an even
# (0x3F80, 0xC0A0, 0x0080) and an odd (0x3F81, 0xC0A1, 0x7F7D) last bit, one fp32 ulp to either side of halfway, +-0, the
# smallest fp32 normal, and a value just below bf16's largest finite one
PATCHIFY_SPECIALS = (0x3F808000, 0x3F818000, 0xC0A08000, 0xC0A18000, 0x00808000, 0x7F7D8000, 0x3F808001, 0x3F817FFF, 0xBF808001,
                     0xBF817FFF, 0x00000000, 0x80000000, 0x00800000, 0x80800000, 0x7F7F7FFF, 0xFF7F7FFF)


def _patchify_inputs(shape):
    """vision [N, 3, H, W] fp32: per-pixel scales, and every 5th element one of PATCHIFY_SPECIALS (no denormals, no NaN / inf)"""
    N, H, W, P, Kpad = shape
    g = _gen(N, H, W, P)
    v = (torch.randn(N * 3 * H * W, generator=g) * torch.tensor([2.0 ** row_exp(p) for p in range(17)]).repeat(cdiv(N * 3 * H * W, 17))[: N * 3 * H * W])
    sp = _f32_from_bits(list(PATCHIFY_SPECIALS))
    at = torch.arange(0, v.numel(), 5)
    v[at] = sp[torch.arange(at.numel()) % sp.numel()]
    return dict(vis=v.reshape(N, 3, H, W).contiguous())


def _copy_inputs(op):
    def make(shape):
        if op == "drop_cls":
            N, G, D = shape
            return dict(tok=bits((N * (G + 1), D), N, G, D, 21))
        if op == "im2col3d":
            B, T, H, W, C = shape
            return dict(x=bits((B * T * H * W, C), B * 100 + T, H, W, C))
        if op == "col2im3d":
            B, T, H, W, C = shape
            return dict(dcols=bits((B * (T // 2 + 1) * (H // 2 + 1) * (W // 2 + 1), 8 * C), B * 100 + T, H, W, C + 1))
        if op == "transpose":
            return dict(x=bits(shape, shape[0], shape[1], 23))
        if op == "transpose_pad":
            Rr, C, ld_in, Rpad = shape
            return dict(x=bits((Rr, ld_in), Rr, C, ld_in, Rpad))
        if op == "splice_embed":
            return _splice_inputs(shape)
        raise KeyError(op)
    return make


SPLICE_VOCAB = 23


def _splice_inputs(shape):
    """ids [3, L]: clip 0 has its video token at position 0 (nothing to its left), clip 1 in the middle behind 2 left-padding
    ids (0), clip 2 at L - 1 behind 3 of them; every other id is a random word, id 0 among them never (so the key mask's zeros
    are the padding's).  The embedding table and the video tokens are random bit patterns."""
    from vlb_oracle import VIDEO_TOKEN_ID
    B, L, Nv, D = shape
    assert B == 3
    g = _gen(L, Nv, D, 24)
    ids = torch.randint(1, SPLICE_VOCAB, (B, L), generator=g)
    ids[1, :2] = 0
    ids[2, :3] = 0
    for b, pos in enumerate((0, L // 2, L - 1)):
        ids[b, pos] = VIDEO_TOKEN_ID
    return dict(ids=ids.to(I64), emb=bits((SPLICE_VOCAB, D), L, Nv, D, 25), vid=bits((B, Nv, D), L, Nv, D, 26), video_pos=(0, L // 2, L - 1))


_MAKERS = dict(plane=_plane_inputs, se=_se_inputs, vit=_vit_inputs, patchify=_patchify_inputs)
_KIND = dict(dwconv3x3="plane", dwconv3x3_dx="plane", dwconv3x3_bwd_w="plane", se_pool="se", se_scale="se", se_bwd_gate="se", se_bwd_x="se",
             se_bwd_x_nopool="se", vit_assemble="vit", patchify="patchify", col2im3d_of_im2col="im2col3d")


@functools.lru_cache(maxsize=None)
def _inputs(kind, shape):
    return (_MAKERS[kind] if kind in _MAKERS else _copy_inputs(kind))(shape)


def inputs_for(op, shape):
    """the inputs of ``op`` at ``shape``, made once and shared between the operations that read the same tensors (read-only)"""
    return _inputs(_KIND.get(op, op), tuple(shape))


# ---------------------------------------------------------------------------------------------------- chains
def c_dwconv():
    """dwconv3x3_kernel: one output adds at most 9 exact products (``for dy`` outer, ``for dx`` inner)"""
    return 9 + 2


def c_dww(N, H, W):
    """dwconv_dw_partial_kernel: a slab (n, h) adds W exact products per tap (``for w``); colpart_reduce_kernel with nb = N * H:
    a group adds ceil(nb / 8) partials (``for b``), the 8 groups add 7 more"""
    return W + cdiv(N * H, 8) + 7 + 2


def c_pool(HW):
    """se_pool_kernel: a thread adds ceil(HW / 4) rows (``for r``, r = rg, rg + 4, ...), the four row groups add 3 more"""
    return cdiv(HW, 4) + 3 + 2


def c_gate(HW):
    """se_bwd_gate_kernel: one thread adds the HW exact products of its channel in order (``for p``)"""
    return HW + 2


# ---------------------------------------------------------------------------------------------------- depthwise 3x3
def taps(H, W, bug=None):
    """[(tap row of w9, valid [H * W] bool, source position [H * W])] for every output position p, dy outer, dx inner"""
    p = torch.arange(H * W)
    hy, wx = (p // H, p % H) if bug == "hw_swapped" else (p // W, p % W)
    out = []
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            yy, xx = hy + dy, wx + dx
            if bug == "no_pad_bottom_right":                    # clamps where it should skip
                yy, xx = yy.clamp(max=H - 1), xx.clamp(max=W - 1)
            src = yy * W + xx
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            if bug == "border_wraps":                           # flat indexing without the xx test: column -1 is the previous row's last
                ok = (yy >= 0) & (yy < H) & (src >= 0) & (src < H * W)
            k = (dx + 1) * 3 + (dy + 1) if bug == "tap_transposed" else (dy + 1) * 3 + (dx + 1)
            out.append((k, ok, src.clamp(0, H * W - 1)))
    return out


def dwconv3x3(x, w9, N, H, W, C, bug=None, key="y"):
    """dwconv3x3_kernel.  x [N * H * W, C], w9 [9, C] -> y [N * H * W, C]"""
    x, w = f64(x).reshape(N, H * W, C), f64(w9).reshape(9, C)
    y, mag = torch.zeros_like(x), torch.zeros_like(x)
    for k, ok, src in taps(H, W, bug):
        t = x[:, src] * ok[None, :, None] * w[k]
        y, mag = y + t, mag + t.abs()
    y, mag = y.reshape(-1, C), mag.reshape(-1, C)
    b32 = c_dwconv() * U * mag + R * y.abs()
    return {key: y}, {key: bf16_out(y, b32), key + "_reach": reach(y, b32)}


def dwconv3x3_dx(dy, w9, N, H, W, C, bug=None):
    """the data gradient as FullFT._block_bwd takes it: dwconv3x3_kernel on dy with the taps reversed (flip of [9, C] along
    the tap axis), which is the transpose of dwconv3x3(., w9)"""
    return dwconv3x3(dy, w9 if bug == "dw_flip_missing" else torch.flip(w9, dims=[0]), N, H, W, C, bug=bug, key="dx")


def dwconv3x3_bwd_w(x, dy, N, H, W, C, bug=None):
    """dwconv_dw_partial_kernel + colpart_reduce_kernel.  -> dw [9, C], dw[tap] = sum_p dy[p] * x[p + tap]"""
    x, g = f64(x).reshape(N, H * W, C), f64(dy).reshape(N, H * W, C)
    dw, mag = torch.zeros(9, C, dtype=F64), torch.zeros(9, C, dtype=F64)
    for k, ok, src in taps(H, W, bug):
        t = g * x[:, src] * ok[None, :, None]
        dw[k], mag[k] = t.sum((0, 1)), t.abs().sum((0, 1))
    if bug == "drop_last_octet" and C // 8 > 256:               # the second blockIdx.x loses its last octet
        dw[:, -8:] = 0
    b32 = c_dww(N, H, W) * U * mag + R * dw.abs()
    return dict(dw=dw), dict(dw=bf16_out(dw, b32), dw_reach=reach(dw, b32))


# ---------------------------------------------------------------------------------------------------- squeeze-excite
def se_pool(x, N, HW, C, bug=None):
    """se_pool_kernel.  x [N * HW, C] -> pooled [N, C] = mean over the HW positions"""
    x = f64(x).reshape(N, HW, C)
    rows = x[:, : HW - 1] if bug == "pool_drop_last_row" else x
    y = rows.sum(1) / (4 * cdiv(HW, 4) if bug == "pool_div_padded" else HW)
    if bug == "drop_last_octet" and C // 8 > 64:
        y[:, -8:] = 0
    b32 = c_pool(HW) * U * x.abs().sum(1) / HW + (1 + RCP) * U * y.abs() + R * y.abs()
    return dict(pooled=y), dict(pooled=bf16_out(y, b32), pooled_reach=reach(y, b32))


def se_scale(x, gate, N, HW, C, bug=None):
    """se_scale_kernel.  y[n, p, c] = x[n, p, c] * sigmoid_f(gate[n, c]): the gate's error and the product's rounding"""
    x, g = f64(x).reshape(N, HW, C), f64(gate).reshape(N, 1, C)
    s, e_s = sigmoid_err(g)
    y = (x * s).reshape(-1, C)
    b32 = (x.abs() * e_s).reshape(-1, C) + U * y.abs()
    return dict(y=y), dict(y=bf16_out(y, b32), y_reach=reach(y, b32))


def se_bwd_gate(x, dy, s, N, HW, C, bug=None):
    """se_bwd_gate_kernel.  ds[n, c] = (sum_p x * dy) * g * (1 - g), g = sigmoid_f(s): the chain over exact products, the gate's
    error through both factors (1 - g adds its own rounding), and the two products' roundings"""
    t = f64(x).reshape(N, HW, C) * f64(dy).reshape(N, HW, C)
    a, bar_a = t.sum(1), c_gate(HW) * U * t.abs().sum(1)
    g, e_g = sigmoid_err(f64(s))
    om = 1 - g
    e_om = e_g + U * om
    ds = a * g if bug == "gate_grad_no_1mg" else a * g * om
    if bug == "drop_last_octet" and C // 8 > 256:
        ds[:, -8:] = 0
    exact = a * g * om
    b32 = (a.abs() + bar_a) * (g + e_g) * (om + e_om) - exact.abs() + 2 * U * exact.abs() + R * exact.abs()
    return dict(ds=ds), dict(ds=bf16_out(ds, b32), ds_reach=reach(ds, b32))


def se_bwd_x(dy, s, dpool, N, HW, C, bug=None):
    """se_bwd_x_kernel.  dx = dy * sigmoid_f(s) + dpool / HW (dpool may be None): the gate's error, the product's rounding, the
    division, the addition"""
    d = f64(dy).reshape(N, HW, C)
    g, e_g = sigmoid_err(f64(s).reshape(N, 1, C))
    a = d * g
    b32 = d.abs() * e_g + U * a.abs()
    dx = a
    if dpool is not None:
        q = f64(dpool).reshape(N, 1, C) / (1 if bug == "dpool_not_divided" else HW)
        dx = a + q
        b32 = b32 + (1 + RCP) * U * q.abs() + U * dx.abs()
    dx, b32 = dx.reshape(-1, C), b32.reshape(-1, C)
    return dict(dx=dx), dict(dx=bf16_out(dx, b32), dx_reach=reach(dx, b32))


# ---------------------------------------------------------------------------------------------------- vision ingest
def vit_assemble(pe, cls, pos, N, G, D, bug=None):
    """vit_assemble_kernel.  tok[n, 0] = cls + pos[0], tok[n, t] = pe[n, t - 1] + pos[t]: one fp32 addition, as rows_emul.add"""
    a = torch.cat([f64(cls).reshape(1, 1, D).expand(N, 1, D), f64(pe).reshape(N, G, D)], 1)
    t = torch.arange(G + 1)
    if bug == "assemble_pos_off_by_one":
        t = (t - 1).clamp(min=0)
    y = (a + f64(pos)[t][None]).reshape(-1, D)
    return dict(tok=y), dict(tok=bf16_out(y, U * y.abs()), tok_reach=reach(y, U * y.abs()))


def patchify(vis, P, Kpad, bug=None):
    """patchify_kernel.  vis [N, 3, H, W] fp32 -> bit patterns of [N * (H / P) * (W / P), Kpad] bf16: column
    k = c * P * P + py * P + px of patch row (n, gy, gx) is torch's round-to-nearest-even of vis[n, c, gy P + py, gx P + px];
    columns 3 P P .. Kpad are +0"""
    N, _, H, W = vis.shape
    G, GH, K = W // P, H // P, 3 * P * P
    if bug == "hw_swapped":
        G, GH = GH, G
    prow, k = torch.arange(N * G * GH)[:, None], torch.arange(K)[None]
    gx, gy, n = prow % G, (prow // G) % GH, prow // (G * GH)
    if bug == "patchify_channel_minor":
        c, py, px = k % 3, (k // 3) // P, (k // 3) % P
    else:
        c, py, px = k // (P * P), (k // P) % P, k % P
    idx = ((n * 3 + c) * H + gy * P + py) * W + gx * P + px
    out = torch.zeros(N * G * GH, Kpad, dtype=BF16)
    out[:, :K] = vis.reshape(-1)[idx.clamp(max=vis.numel() - 1)].to(BF16)
    return dict(patches=out.view(I16))


def drop_cls(tok, N, G, D, bug=None):
    """drop_cls_kernel.  tok [N * (G + 1), D] -> [N * G, D] without every image's first token"""
    t = tok.reshape(N, G + 1, D)
    return dict(out=(t[:, :G] if bug == "drop_cls_keeps_cls" else t[:, 1:]).reshape(N * G, D).clone())


# ---------------------------------------------------------------------------------------------------- Conv3d k2 s2 p1 as a GEMM
def _im2col_index(T, H, W, bug=None):
    """-> source position [R, 8] within one clip's T * H * W, validity [R, 8]; R = T2 * H2 * W2 windows, row-major"""
    T2, H2, W2 = T // 2 + 1, H // 2 + 1, W // 2 + 1
    t2, h2, w2 = (v.reshape(-1) for v in torch.meshgrid(torch.arange(T2), torch.arange(H2), torch.arange(W2), indexing="ij"))
    src, ok = torch.zeros(t2.numel(), 8, dtype=I64), torch.zeros(t2.numel(), 8, dtype=torch.bool)
    for tap in range(8):
        kt, kh, kw = tap >> 2, (tap >> 1) & 1, tap & 1
        t, h, w = 2 * t2 - 1 + kt, 2 * h2 - 1 + kh, 2 * w2 - 1 + kw
        col = (kw * 2 + kh) * 2 + kt if bug == "im2col_tap_order" else tap
        ok[:, col] = (t >= 0) & (t < T) & (h >= 0) & (h < H) & (w >= 0) & (w < W)
        src[:, col] = ((t * H + h) * W + w).clamp(0, T * H * W - 1)
    return src, ok


def im2col3d(x, B, T, H, W, C, bug=None):
    """im2col3d_kernel.  x [B * T * H * W, C] -> cols [B * T2 * H2 * W2, 8 * C]; a tap outside the clip is +0.  (Any dtype:
    int16 bit patterns for the device comparison, fp64 for the adjoint identity.)"""
    src, ok = _im2col_index(T, H, W, bug)
    v = x.reshape(B, T * H * W, C)[:, src]                                  # [B, R, 8, C]
    return dict(cols=torch.where(ok[None, :, :, None], v, torch.zeros_like(v)).reshape(-1, 8 * C))


def col2im3d(dcols, B, T, H, W, C, bug=None):
    """col2im3d_kernel.  dcols [B * T2 * H2 * W2, 8 * C] -> dx [B * T * H * W, C]: element (t, h, w) sits in exactly one window,
    window ((t + 1) // 2, ...) at tap ((t + 1) & 1, ...); whatever the padding taps of dcols hold is ignored"""
    T2, H2, W2 = T // 2 + 1, H // 2 + 1, W // 2 + 1
    t, h, w = (v.reshape(-1) for v in torch.meshgrid(torch.arange(T), torch.arange(H), torch.arange(W), indexing="ij"))
    o = 0 if bug == "col2im_unpadded_coords" else 1
    win = (((t + o) // 2) * H2 + (h + o) // 2) * W2 + (w + o) // 2
    tap = (((t + 1) & 1) * 2 + ((h + 1) & 1)) * 2 + ((w + 1) & 1)
    return dict(dx=dcols.reshape(B, T2 * H2 * W2, 8, C)[:, win, tap].reshape(-1, C).clone())


def padding_taps(T, H, W):
    """[R, 8] bool: the taps of im2col3d's output that lie outside the clip"""
    return ~_im2col_index(T, H, W)[1]


# ---------------------------------------------------------------------------------------------------- transposes, splice
def transpose(x, bug=None):
    """transpose_kernel (gemm.hip).  [R, C] -> [C, R]"""
    return dict(out=x.t().contiguous())


def transpose_pad(x, Rr, C, Rpad, bug=None):
    """transpose_pad_kernel.  x [R, ld_in], its first C columns -> out [C, Rpad] = x^T with columns R .. Rpad +0"""
    out = torch.zeros(C, Rpad, dtype=x.dtype)
    out[:, :Rr] = x[:, :C].t()
    if bug == "transpose_pad_tail_dropped":                    # the columns the scalar tail reads
        out[C // 8 * 8:] = 0
    return dict(out=out)


def splice_embed(ids, emb, vid, bug=None):
    """splice_kernel, dense layout: embeddings and key mask of oracle/vlb_oracle.py::splice_multimodal.  emb and vid are
    int16 bit patterns: embedding lookup and concatenation move bits"""
    from vlb_oracle import splice_multimodal
    e, m = splice_multimodal(emb.view(BF16), ids, vid.view(BF16))
    return dict(embeds=e.reshape(-1, e.shape[-1]).contiguous().view(I16), key_mask=m.to(torch.uint8))


# ---------------------------------------------------------------------------------------------------- fp32 restatement
# The arithmetic kernels in numpy float32, in the kernels' order (no fma contraction: every sum rounds; the products of two
# bf16 values are exact either way).  A skipped tap is restated as adding +-0, which leaves an fp32 sum as it is.
def _taps_np(H, W):
    return [(k, ok.numpy().astype(np.float32), src.numpy()) for k, ok, src in taps(H, W)]


def emu_dwconv3x3(x, w9, N, H, W, C, key="y"):
    """tap order dy outer, dx inner"""
    x, w = _np(x).reshape(N, H * W, C), _np(w9)
    acc = np.zeros((N, H * W, C), dtype=f32)
    for k, ok, src in _taps_np(H, W):
        acc = acc + x[:, src] * ok[None, :, None] * w[k]
    return {key: _bf(acc.reshape(-1, C))}


def emu_dwconv3x3_dx(dy, w9, N, H, W, C):
    return emu_dwconv3x3(dy, torch.flip(w9, dims=[0]), N, H, W, C, key="dx")


def emu_dwconv3x3_bwd_w(x, dy, N, H, W, C):
    """slab (n, h): ``for w`` outer, the 9 taps inner; then colpart_reduce32 over the N * H slabs of 9 * C columns"""
    x, g = _np(x).reshape(N, H * W, C), _np(dy).reshape(N, H * W, C)
    part = np.zeros((N, H, 9, C), dtype=f32)
    tp = _taps_np(H, W)
    for w in range(W):
        p = np.arange(H) * W + w
        for k, ok, src in tp:
            part[:, :, k] = part[:, :, k] + g[:, p] * x[:, src[p]] * ok[p][None, :, None]
    return dict(dw=_bf(colpart_reduce32(part.reshape(N * H, 9 * C)).reshape(9, C)))


def emu_se_pool(x, N, HW, C):
    """row group rg walks r = rg, rg + 4, ...; ((g0 + g1) + g2) + g3; / HW"""
    x = _np(x).reshape(N, HW, C)
    grp = np.zeros((4, N, C), dtype=f32)
    for rg in range(4):
        for r in range(rg, HW, 4):
            grp[rg] = grp[rg] + x[:, r]
    return dict(pooled=_bf((((grp[0] + grp[1]) + grp[2]) + grp[3]) / f32(HW)))


def emu_se_scale(x, gate, N, HW, C):
    return dict(y=_bf((_np(x).reshape(N, HW, C) * sigmoid32(_np(gate))[:, None]).reshape(-1, C)))


def emu_se_bwd_gate(x, dy, s, N, HW, C):
    """``for p`` in order; acc * g * (1 - g) left to right"""
    x, d = _np(x).reshape(N, HW, C), _np(dy).reshape(N, HW, C)
    acc = np.zeros((N, C), dtype=f32)
    for p in range(HW):
        acc = acc + x[:, p] * d[:, p]
    g = sigmoid32(_np(s))
    return dict(ds=_bf(acc * g * (f32(1) - g)))


def emu_se_bwd_x(dy, s, dpool, N, HW, C):
    o = _np(dy).reshape(N, HW, C) * sigmoid32(_np(s))[:, None]
    o = o + ((_np(dpool) / f32(HW))[:, None] if dpool is not None else f32(0))
    return dict(dx=_bf(o.reshape(-1, C)))


def emu_vit_assemble(pe, cls, pos, N, G, D):
    a = np.concatenate([np.broadcast_to(_np(cls).reshape(1, 1, D), (N, 1, D)), _np(pe).reshape(N, G, D)], 1)
    return dict(tok=_bf((a + _np(pos)[None]).reshape(-1, D)))


# ---------------------------------------------------------------------------------------------------- one call per operation
def call(op, shape, emu=False, bug=None):
    """``op`` on the shared inputs of ``shape``: the fp64 stage (-> ref, bar), the fp32 restatement (emu: -> outputs), or, for
    the bit-exact operations, -> {name: bits}"""
    i = inputs_for(op, shape)
    kw = {} if emu else dict(bug=bug)
    if op in ("dwconv3x3", "dwconv3x3_dx", "dwconv3x3_bwd_w"):
        if op == "dwconv3x3":
            return (emu_dwconv3x3 if emu else dwconv3x3)(i["x"], i["w9"], *shape, **kw)
        if op == "dwconv3x3_dx":
            return (emu_dwconv3x3_dx if emu else dwconv3x3_dx)(i["dy"], i["w9"], *shape, **kw)
        return (emu_dwconv3x3_bwd_w if emu else dwconv3x3_bwd_w)(i["x"], i["dy"], *shape, **kw)
    if op == "se_pool":
        return (emu_se_pool if emu else se_pool)(i["x"], *shape, **kw)
    if op == "se_scale":
        return (emu_se_scale if emu else se_scale)(i["x"], i["s"], *shape, **kw)
    if op == "se_bwd_gate":
        return (emu_se_bwd_gate if emu else se_bwd_gate)(i["x"], i["dy"], i["s"], *shape, **kw)
    if op in ("se_bwd_x", "se_bwd_x_nopool"):
        return (emu_se_bwd_x if emu else se_bwd_x)(i["dy"], i["s"], i["dpool"] if op == "se_bwd_x" else None, *shape, **kw)
    if op == "vit_assemble":
        return (emu_vit_assemble if emu else vit_assemble)(i["pe"], i["cls"], i["pos"], *shape, **kw)
    assert not emu, op
    if op == "patchify":
        return patchify(i["vis"], shape[3], shape[4], bug=bug)
    if op == "drop_cls":
        return drop_cls(i["tok"], *shape, bug=bug)
    if op == "im2col3d":
        return im2col3d(i["x"], *shape, bug=bug)
    if op == "col2im3d":
        return col2im3d(i["dcols"], *shape, bug=bug)
    if op == "col2im3d_of_im2col":
        return col2im3d(im2col3d(i["x"], *shape)["cols"], *shape, bug=bug)
    if op == "transpose":
        return transpose(i["x"], bug=bug)
    if op == "transpose_pad":
        return transpose_pad(i["x"], shape[0], shape[1], shape[3], bug=bug)
    if op == "splice_embed":
        return splice_embed(i["ids"], i["emb"], i["vid"], bug=bug)
    raise KeyError(op)


# ---------------------------------------------------------------------------------------------------- planted bugs
# bug -> [(operation, shape)] at which at least one output must leave its bar or, for a bit-exact operation, change a bit
BUGS = {
    "hw_swapped": [("dwconv3x3", (2, 1, 5, 32)), ("dwconv3x3", (2, 5, 1, 64)), ("dwconv3x3", (3, 5, 7, 96)), ("dwconv3x3", (1, 7, 5, 32)),
                   ("dwconv3x3_dx", (3, 5, 7, 96)), ("dwconv3x3_bwd_w", (2, 7, 5, 8)), ("dwconv3x3_bwd_w", (3, 5, 7, 72)),
                   ("patchify", (3, 4, 6, 2, 16)), ("patchify", (2, 28, 42, 14, 640))],
    "tap_transposed": [("dwconv3x3", (3, 5, 7, 96)), ("dwconv3x3", (2, 13, 13, 64)), ("dwconv3x3", (1, 24, 24, 32)), ("dwconv3x3_dx", (1, 7, 5, 32)),
                       ("dwconv3x3_bwd_w", (3, 6, 6, 64)), ("dwconv3x3_bwd_w", (2, 7, 5, 8))],
    "no_pad_bottom_right": [("dwconv3x3", (2, 5, 1, 64)), ("dwconv3x3", (2, 1, 5, 32)), ("dwconv3x3", (3, 5, 7, 96)), ("dwconv3x3", (1, 24, 24, 32)),
                            ("dwconv3x3_dx", (2, 13, 13, 64)), ("dwconv3x3_bwd_w", (3, 6, 6, 64))],
    "border_wraps": [("dwconv3x3", (3, 5, 7, 96)), ("dwconv3x3", (1, 7, 5, 32)), ("dwconv3x3", (2, 13, 13, 64)), ("dwconv3x3", (1, 33, 32, 32)),
                     ("dwconv3x3_dx", (1, 24, 24, 32)), ("dwconv3x3_bwd_w", (3, 5, 7, 72))],
    "pool_div_padded": [("se_pool", (2, 3, 8)), ("se_pool", (3, 35, 520)), ("se_pool", (2, 169, 96))],
    "pool_drop_last_row": [("se_pool", (1, 1, 8)), ("se_pool", (2, 3, 8)), ("se_pool", (3, 35, 520)), ("se_pool", (2, 169, 96))],
    "drop_last_octet": [("se_pool", (3, 35, 520)), ("se_bwd_gate", (3, 35, 2056)), ("dwconv3x3_bwd_w", (1, 3, 4, 2056))],
    "gate_grad_no_1mg": [("se_bwd_gate", (1, 1, 8)), ("se_bwd_gate", (3, 35, 2056)), ("se_bwd_gate", (2, 169, 96))],
    "dpool_not_divided": [("se_bwd_x", (3, 35, 520))],
    "im2col_tap_order": [("im2col3d", (2, 3, 5, 4, 16)), ("im2col3d", (1, 4, 6, 7, 8)), ("im2col3d", (2, 8, 6, 6, 32))],
    "col2im_unpadded_coords": [("col2im3d", (2, 3, 5, 4, 16)), ("col2im3d", (1, 4, 6, 7, 8)), ("col2im3d_of_im2col", (2, 8, 6, 6, 32)),
                               ("col2im3d_of_im2col", (1, 12, 24, 24, 8))],
    "assemble_pos_off_by_one": [("vit_assemble", (1, 1, 8)), ("vit_assemble", (3, 5, 24)), ("vit_assemble", (2, 36, 128))],
    "drop_cls_keeps_cls": [("drop_cls", (1, 1, 8)), ("drop_cls", (3, 5, 24)), ("drop_cls", (2, 36, 128))],
    "patchify_channel_minor": [("patchify", (3, 4, 6, 2, 16)), ("patchify", (1, 14, 14, 14, 592)), ("patchify", (2, 28, 42, 14, 640))],
    "transpose_pad_tail_dropped": [("transpose_pad", (1, 1, 8, 8)), ("transpose_pad", (5, 13, 16, 8)), ("transpose_pad", (65, 67, 72, 72)),
                                   ("transpose_pad", (100, 77, 80, 128))],
    "dw_flip_missing": [("dwconv3x3_dx", (2, 1, 5, 32)), ("dwconv3x3_dx", (3, 5, 7, 96)), ("dwconv3x3_dx", (2, 13, 13, 64))],
}


def bits_differ(got, ref):
    """{name: number of elements whose bits differ} between two results of a bit-exact operation"""
    return {k: int((torch.as_tensor(got[k]) != ref[k]).sum()) if tuple(got[k].shape) == tuple(ref[k].shape) else ref[k].numel() for k in ref}
