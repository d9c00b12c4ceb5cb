"""fp64 restatement of the row and element-wise kernels (csrc/ops.hip, csrc/train.hip), ONE OPERATION AT A TIME, with
derived per-element error bars, inputs, an fp32 restatement in the kernels' own operation order, and planted bugs.

Operations: rmsnorm_fwd, rmsnorm_bwd, rmsnorm_bwd_dw, rmsnorm_bwd_full, layernorm_fwd, layernorm_bwd, rope, swiglu_fwd,
swiglu_bwd, act_fwd, act_bwd, colsum, embed_grad, add.  A stage function takes the kernel's bf16 inputs (converted to fp64
inside) and returns ``(ref, bar)``: the outputs in fp64 and, per output, the per-element bound on |device - ref|.

Bars (the rule of tests/head_emul.py; nothing is fitted to a measurement; tests print max(err / bar) and assert <= 1):
  * an fp32 sum of terms:  c * 2^-24 * sum|terms| + 2^-22 * |ref|,  c = the longest chain of additions one output goes
    through in that kernel + 2 (each ``c_*`` below says which loop or butterfly it counts); a term that is a product of
    more than two rounded factors adds its extra roundings to c.  The compiler may contract a*b+c into an fma: that only
    removes roundings, the bars assume none removed.
  * rsqrtf, __expf and the hardware reciprocal get a RELATIVE allowance, stated next to ``RSQ``, ``expf_rel`` and ``RCP``.
    v_rsq_f32, v_exp_f32 and v_rcp_f32 are specified to 1 ulp in the CDNA instruction set reference; 1 ulp = 2 * 2^-24
    relative.
  * a difference of rounded quantities (x - mean, a - b) gets the ABSOLUTE errors of its operands: no bar relies on a
    result being far from zero.
  * a bf16 output adds 2^-8 * |ref| (half a bf16 ulp) on top of the fp32 bar of the value before rounding.
  * where the kernel rounds an intermediate to bf16 on purpose (RMSNorm forward: w * bf16(x * rstd), the HF order) the
    reference rounds at the same place, and the bar carries |w| times the distance to the neighbouring bf16 value ONLY
    where the fp32 error of x * rstd can carry the intermediate across a rounding boundary: a flipped rounding is legal,
    anything more is not.  (Never more than one bf16 ulp of the intermediate times |w|.)
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
U = 2.0 ** -24          # fp32 unit roundoff
R = 2.0 ** -22          # relative slack on the reference's own magnitude
HB = 2.0 ** -8          # half a bf16 ulp, relative
TINY = 2.0 ** -126      # v_exp_f32 / v_rcp_f32 flush denormal results: an absolute floor where a value leaves fp32's normal range
RSQ = 8                 # in units of U, on top of the chain: the squares (1), / dim (1), + eps (1), rsqrtf (1 ulp = 2), slack 3
RCP = 2                 # in units of U: v_rcp_f32, 1 ulp
EPS_RMS, EPS_LN = 1e-5, 1e-6
ACT_NONE, ACT_QUICK_GELU, ACT_GELU, ACT_SILU = 0, 1, 2, 3
C_QUICK = 1.702                                     # the constants as mathematics; the kernels' fp32 roundings of them are
C_RSQRT2 = math.sqrt(0.5)                           # counted in the bars (one U each, where the constant is used)
C_PDF = 1.0 / math.sqrt(2.0 * math.pi)
BF16_MAX = float(torch.finfo(BF16).max)


def cdiv(a, b):
    return -(-a // b)


def f64(t):
    return t.to(F64)


def rbf(t):
    """fp64 -> the bf16 value an fp32 holding it rounds to, as fp64"""
    return t.to(F32).to(BF16).to(F64)


def reach(ref, bar32):
    """(lo, hi): where the fp32 value behind a bf16 output can lie.  Rounding is monotone, so the output itself lies in
    [bf16(lo), bf16(hi)]: ONE value wherever no rounding boundary is within bar32 of ref.  ``outside`` counts the elements
    that do not; it sees an fp32-sized error (which the half ulp in ``bf16_out`` hides) on every element that the error
    carries across a boundary, about |error| / ulp of them."""
    return ref - bar32 - TINY, ref + bar32 + TINY


def bf16_out(ref, bar32):
    """bar of a bf16 output whose fp32 value is within bar32 of ref (TINY: a result below fp32's normal range may be
    flushed to zero, depending on the denormal mode the conversion runs under)"""
    return HB * ref.abs() + (1 + HB) * bar32 + TINY


# ---------------------------------------------------------------------------------------------------- dispatch
def norm_rows_per_block(rows):
    """train.hip: norm_rows_per_block"""
    r = (rows + 255) // 256
    return 4 if r < 4 else (r + 3) // 4 * 4


def rms_full_rows_per_block(rows):
    """train.hip: rms_full_rows_per_block"""
    r = (rows + 1023) // 1024
    return 4 if r < 4 else (r + 3) // 4 * 4


def _ni4(dim):
    """the dim <= 512 / 1024 / 2048 / else ladder of vlb_rmsnorm_bwd_dw, vlb_rmsnorm_bwd_full, vlb_layernorm_bwd"""
    return 1 if dim <= 512 else 2 if dim <= 1024 else 4 if dim <= 2048 else 8


def paths(op, rows, dim):
    """(kernel instantiation, rows_per_block) the launcher of ``op`` takes at [rows, dim]: a restatement of the branch
    conditions in ops.hip / train.hip.  rows_per_block is 4 (one wave per row, 4 waves) where the launcher has no choice."""
    if op == "rmsnorm_fwd":
        return ("rmsnorm_fwd_cached_kernel<1>" if dim <= 512 else "rmsnorm_fwd_cached_kernel<8>" if dim <= 4096 else "rmsnorm_fwd_kernel"), 4
    if op == "rmsnorm_bwd":
        return ("rmsnorm_bwd_cached_kernel<1>" if dim <= 512 else "rmsnorm_bwd_kernel"), 4
    if op == "layernorm_fwd":
        return ("layernorm_fwd_cached_kernel<1>" if dim <= 512 else "layernorm_fwd_cached_kernel<2>" if dim <= 1024
                else "layernorm_fwd_cached_kernel<8>" if dim <= 4096 else "layernorm_fwd_kernel"), 4
    assert dim <= 4096, (op, dim)
    if op == "rmsnorm_bwd_dw":
        return f"rmsnorm_dw_partial_kernel<{_ni4(dim)}>", norm_rows_per_block(rows)
    if op == "rmsnorm_bwd_full":
        return f"rmsnorm_dw_partial_kernel<{_ni4(dim)}>", rms_full_rows_per_block(rows)
    if op == "layernorm_bwd":
        return f"layernorm_bwd_kernel<{_ni4(dim)}>", norm_rows_per_block(rows)
    if op == "colsum":
        return "colsum_partial_kernel", norm_rows_per_block(rows)
    raise KeyError(op)


NORM_OPS = ("rmsnorm_fwd", "rmsnorm_bwd", "layernorm_fwd", "rmsnorm_bwd_dw", "rmsnorm_bwd_full", "layernorm_bwd")
FWD_ONLY_DIMS = (4104, 6144)            # vlb_rmsnorm_bwd_dw / _full / vlb_layernorm_bwd refuse dim > 4096

# What a shape is there for, per operation, as LITERALS (not computed from dim): the tests assert that ``paths`` leads
# there.  Order: rmsnorm_fwd, rmsnorm_bwd, layernorm_fwd, then the NI of rmsnorm_dw_partial_kernel / layernorm_bwd_kernel.
_C1 = ("rmsnorm_fwd_cached_kernel<1>", "rmsnorm_bwd_cached_kernel<1>", "layernorm_fwd_cached_kernel<1>", 1)
_C2 = ("rmsnorm_fwd_cached_kernel<8>", "rmsnorm_bwd_kernel", "layernorm_fwd_cached_kernel<2>", 2)
_C4 = ("rmsnorm_fwd_cached_kernel<8>", "rmsnorm_bwd_kernel", "layernorm_fwd_cached_kernel<8>", 4)
_C8 = ("rmsnorm_fwd_cached_kernel<8>", "rmsnorm_bwd_kernel", "layernorm_fwd_cached_kernel<8>", 8)
_GEN = ("rmsnorm_fwd_kernel", "rmsnorm_bwd_kernel", "layernorm_fwd_kernel", None)
RUNGS = {8: _C1, 64: _C1, 264: _C1, 512: _C1, 520: _C2, 1024: _C2, 1032: _C4, 1160: _C4, 2048: _C4, 2056: _C8, 4096: _C8,
         4104: _GEN, 6144: _GEN}
# (rows, dim, rows_per_block of the norm_rows_per_block passes, of rmsnorm_bwd_full's pass)
_SHAPES = [(37, d, 4, 4) for d in (8, 264, 512, 520, 1024, 1032, 1160, 2048, 2056, 4096, 4104, 6144)]
_SHAPES += [(1, 8, 4, 4), (1, 520, 4, 4), (4, 520, 4, 4), (5, 520, 4, 4), (5, 1160, 4, 4), (4, 4096, 4, 4), (1, 6144, 4, 4)]
_SHAPES += [(1030, 64, 8, 4),        # norm_rows_per_block = 8: 129 blocks, the last with 6 rows; colpart's 8 groups get 17, 16 x 7
            (4101, 64, 20, 8)]       # rms_full_rows_per_block = 8 (513 blocks, the last with 5 rows)


def _norm_case(rows, dim, rpb, rpb_full):
    rf, rb, lf, ni = RUNGS[dim]
    expect = {"rmsnorm_fwd": (rf, 4), "rmsnorm_bwd": (rb, 4), "layernorm_fwd": (lf, 4)}
    if ni is not None:
        expect.update({"rmsnorm_bwd_dw": (f"rmsnorm_dw_partial_kernel<{ni}>", rpb),
                       "rmsnorm_bwd_full": (f"rmsnorm_dw_partial_kernel<{ni}>", rpb_full),
                       "layernorm_bwd": (f"layernorm_bwd_kernel<{ni}>", rpb)})
    if rows > 1000:                     # the long cases are there for the partial-sum passes only
        for op in ("rmsnorm_fwd", "rmsnorm_bwd", "layernorm_fwd"):
            del expect[op]
    return dict(id=f"{rows}x{dim}", rows=rows, dim=dim, expect=expect)


NORM_CASES = [_norm_case(*s) for s in _SHAPES]
ROPE_CASES = [dict(id=f"D{D}-h{h}-{'pos' if pos else 'seq'}-{'fwd' if sign > 0 else 'bwd'}", D=D, heads=h, pos=pos, sign=sign)
              for D in (16, 64, 128) for h in (1, 3) for pos in (False, True) for sign in (1, -1)]
SWIGLU_CASES = [dict(id=f"{r}x{ff}", rows=r, ff=ff) for ff in (8, 264) for r in (1, 70)]
ACT_CASES = [dict(id=n, act=a) for n, a in (("quick_gelu", ACT_QUICK_GELU), ("gelu", ACT_GELU), ("silu", ACT_SILU))]
# (1030, 2056) is left out for its size; 1030 rows (rows_per_block 8) run at dim 8 and 64, dim 2056 (two blockIdx.x) at 1 and 37 rows
COLSUM_CASES = [dict(id=f"{r}x{d}", rows=r, dim=d, ld=d + 24, expect=("colsum_partial_kernel", rpb))
                for r, d, rpb in ((1, 8, 4), (37, 8, 4), (1030, 8, 8), (1, 2056, 4), (37, 2056, 4), (1030, 64, 8))]
EMBED_CASES = [dict(id=f"D{D}", D=D, ld=D + 8) for D in (8, 2056)]
ADD_CASES = [dict(id=f"n{n}", n=n) for n in (8, 37 * 264)]
BY_ID = {("norm", c["id"]): c for c in NORM_CASES}
for _k, _cs in (("rope", ROPE_CASES), ("swiglu", SWIGLU_CASES), ("act", ACT_CASES), ("colsum", COLSUM_CASES),
                ("embed", EMBED_CASES), ("add", ADD_CASES)):
    BY_ID.update({(_k, c["id"]): c for c in _cs})


def norm_cases(op):
    return [c for c in NORM_CASES if op in c["expect"]]


# ---------------------------------------------------------------------------------------------------- inputs
KINDS = ("rand", "zero", "const", "single", "rand", "rand", "ulp", "rand")


def row_exp(r):
    """per-row scale exponent: -10 .. 6, all 17 values within any 17 consecutive rows"""
    return -10 + (5 * r) % 17


def _gen(*key):
    return torch.Generator().manual_seed(sum(int(k) * p for k, p in zip(key, (1000003, 10007, 101, 7))) % (2 ** 31))


def _norm_inputs(case):
    """x: zero-mean rows at scale 2^row_exp(r) (eps dominates the small ones), with (from 4 rows on, by r % 8) an all-zero
    row, a constant row, a row whose only non-zero element is its LAST one, and (xl only) a row of 100.5 * scale with one
    element one bf16 ulp (0.5 * scale) higher: mean / std = 201 sqrt(dim), where a one-pass variance loses everything.
    xl (LayerNorm's x): as x, and every "rand" row with even r sits on an offset of 64 times its standard deviation.  w = 1 + 0.1 randn with one entry exactly 0 and one negative."""
    rows, dim = case["rows"], case["dim"]
    g = _gen(rows, dim, 1)
    sc = torch.tensor([2.0 ** row_exp(r) for r in range(rows)])[:, None]
    x = torch.randn(rows, dim, generator=g) * sc
    xl = x.clone()
    for r in range(rows):
        kind = KINDS[r % 8] if rows >= 4 else "rand"
        s = float(sc[r])
        if kind == "zero":
            x[r] = 0
            xl[r] = 0
        elif kind == "const":
            x[r] = 3 * s
            xl[r] = 3 * s
        elif kind == "single":
            x[r] = 0
            x[r, dim - 1] = 1.5 * s
            xl[r] = x[r]
        elif kind == "ulp":
            xl[r] = 100.5 * s                       # (not a power of two: the squares' sum must not be exact in fp32)
            xl[r, dim // 2] = 101 * s
        elif r % 2 == 0:
            xl[r] += 64 * s
    w = 1 + 0.1 * torch.randn(dim, generator=g)
    w[dim // 3] = 0
    w[dim - 1] = -0.75
    b = 0.1 * torch.randn(dim, generator=g)
    dsc = torch.tensor([2.0 ** ((3 * r) % 5 - 2) for r in range(rows)])[:, None]
    dy = torch.randn(rows, dim, generator=g) * dsc
    dx_in = 0.5 * torch.randn(rows, dim, generator=g)
    res = torch.randn(rows, dim, generator=g)
    return {k: v.to(BF16) for k, v in dict(x=x, xl=xl, w=w, b=b, dy=dy, dx_in=dx_in, res=res).items()}


def rope_tables(S, D):
    """cos / sin [S, D/2] fp32, theta = 10000"""
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=F64) / D))
    ang = torch.arange(S, dtype=F64)[:, None] * inv[None, :]
    return ang.cos().to(F32), ang.sin().to(F32)


ROPE_B, ROPE_S = 2, 5
ROPE_POS = (3, 0, 4, 4, 1, 0, 2, 3, 3, 1)          # non-monotonic, repeating, and != r % S at r = 0, 1, 2, 3, 4, 6, 7, 8, 9


def _rope_inputs(case):
    D, heads = case["D"], case["heads"]
    rows, ld = ROPE_B * ROPE_S, heads * D + 64
    g = _gen(D, heads, 2)
    x = (torch.randn(rows, ld, generator=g) * torch.tensor([2.0 ** ((r * 3) % 7 - 3) for r in range(rows)])[:, None]).to(BF16)
    cos, sin = rope_tables(ROPE_S, D)
    return dict(x=x, cos=cos, sin=sin, pos=torch.tensor(ROPE_POS, dtype=torch.int32) if case["pos"] else None)


def act_grid():
    """4096 bf16 values: [-90, 90] evenly, [-8, 8] evenly, and the edges (+-0, the largest finite bf16, the smallest
    normal and a denormal bf16, the neighbourhood of fp32 expf's overflow at 88.7)"""
    edges = [0.0, -0.0, BF16_MAX, -BF16_MAX, 2.0 ** -126, -2.0 ** -126, 2.0 ** -130, -2.0 ** -130, 88.0, -88.0, 88.5, -88.5,
             89.0, -89.0, 1.0, -1.0]
    x = torch.cat([torch.linspace(-90, 90, 2040), torch.linspace(-8, 8, 2040), torch.tensor(edges)])
    return x.to(BF16)


def _act_inputs(case):
    x = act_grid()
    return dict(x=x, dy=(torch.randn(x.numel(), generator=_gen(case["act"], 3)) * 2).to(BF16))


def _swiglu_inputs(case):
    rows, ff = case["rows"], case["ff"]
    g = _gen(rows, ff, 4)
    gu = torch.randn(rows, 2 * ff, generator=g) * 3
    gu[0, :8] = torch.tensor([0.0, -0.0, 20.0, -20.0, 88.5, -88.5, 90.0, -90.0])       # gate edges
    return dict(gu=gu.to(BF16), dout=torch.randn(rows, ff, generator=g).to(BF16))


def _colsum_inputs(case):
    rows, ld = case["rows"], case["ld"]
    sc = torch.tensor([2.0 ** ((r * 3) % 7 - 3) for r in range(rows)])[:, None]
    return dict(x=(torch.randn(rows, ld, generator=_gen(rows, ld, 5)) * sc).to(BF16))


EMBED_ROWS, EMBED_VOCAB = 50, 12
EMBED_TOK = (3, 7, 9, 0)
EMBED_COUNTS = (1, 33, 3, 2)                        # one occurrence; 33: a long fp32 chain rounded once


def _embed_inputs(case):
    g = _gen(case["D"], 6)
    d = torch.randn(EMBED_ROWS, case["ld"], generator=g).to(BF16)
    order = torch.randperm(EMBED_ROWS, generator=g)[: sum(EMBED_COUNTS)]
    beg = [0]
    for n in EMBED_COUNTS:
        beg.append(beg[-1] + n)
    rows = torch.cat([order[beg[j]:beg[j + 1]].sort().values for j in range(len(EMBED_COUNTS))])   # ascending per job
    return dict(d=d, tok=torch.tensor(EMBED_TOK, dtype=torch.int32), beg=torch.tensor(beg, dtype=torch.int32), rows=rows.to(torch.int32))


def _add_inputs(case):
    g = _gen(case["n"], 7)
    n = case["n"]
    return dict(a=(torch.randn(n, generator=g) * 4).to(BF16), b=torch.randn(n, generator=g).to(BF16))


_MAKERS = dict(norm=_norm_inputs, rope=_rope_inputs, act=_act_inputs, swiglu=_swiglu_inputs, colsum=_colsum_inputs,
               embed=_embed_inputs, add=_add_inputs)


@functools.lru_cache(maxsize=None)
def inputs_for(kind, case_id):
    """the inputs of a named case, made once and shared (treat as read-only)"""
    return _MAKERS[kind](BY_ID[(kind, case_id)])


# ---------------------------------------------------------------------------------------------------- chains
def c_stat(dim):
    """a row statistic (rmsnorm / layernorm kernels, rmsnorm_dw_partial_kernel, layernorm_bwd_kernel): a lane adds 8 values
    per 512-column trip (the ``for c`` / ``for k`` loop; the zero padding of the register-cached forms adds exactly), then
    wave_sum's 6 butterfly levels"""
    return 8 * cdiv(dim, 512) + 6 + 2


def c_colpart(rows, rpb):
    """d gamma / d beta through rmsnorm_dw_partial_kernel or layernorm_bwd_kernel and colpart_reduce_kernel: a wave adds its
    rpb / 4 rows (``for row``), the 4 waves are added (3), a group adds ceil(nb / 8) partials (``for b``), 8 groups (7)"""
    nb = cdiv(rows, rpb)
    return rpb // 4 + 3 + cdiv(nb, 8) + 7 + 2


def c_colsum(rows, rpb):
    """colsum_partial_kernel walks the rpb rows of a block in order (``for r``), then colpart_reduce_kernel as above"""
    nb = cdiv(rows, rpb)
    return rpb + cdiv(nb, 8) + 7 + 2


# ---------------------------------------------------------------------------------------------------- RMSNorm
def _rms_stats(x, eps, bug):
    dim = x.shape[-1]
    cols = torch.ones(dim, dtype=F64)
    if bug == "drop_last8":
        cols[-8:] = 0
    ms = (x * x * cols).sum(-1, keepdim=True) / dim
    if bug == "eps_outside":
        rstd = 1.0 / (ms.sqrt() + eps)
    else:
        rstd = (ms + (0.1 * eps if bug == "eps_tenth" else eps)).rsqrt()
    # ss is a sum of non-negative terms: its relative error is c_stat * U, and rstd takes half of what the root's argument has
    return rstd, (c_stat(dim) + RSQ) * U + R


def rmsnorm_fwd(x, w, eps, bug=None):
    """rmsnorm_fwd_kernel / rmsnorm_fwd_cached_kernel<NI>.  -> y = w * bf16(x * rstd)"""
    x, w = f64(x), f64(w)
    rstd, rel = _rms_stats(x, eps, bug)
    t = x * rstd
    tb = rbf(t)
    d = (rel + U) * t.abs()                          # fp32 error of x * rstd: rstd's, and the product's rounding
    flip = torch.maximum((rbf(t - d) - tb).abs(), (rbf(t + d) - tb).abs())     # 0 unless a rounding boundary is within d
    y = w * tb                                       # exact in fp32: two 8-bit significands
    ylo, yhi = w * rbf(t - d), w * rbf(t + d)
    return dict(y=y), dict(y=bf16_out(y, w.abs() * flip), y_reach=(torch.minimum(ylo, yhi) - TINY, torch.maximum(ylo, yhi) + TINY))


def _rms_dx(x, w, dy, dx_in, eps, bug):
    dim = x.shape[-1]
    rstd, rel = _rms_stats(x, eps, bug)
    terms = x * dy * w
    dot = terms.sum(-1, keepdim=True)
    coef = dot * rstd ** 3 / (cdiv(dim, 512) * 512 if bug == "padded_width" else dim)
    a, b = rstd * w * dy, coef * x
    dx = a - b
    bar_dot = (c_stat(dim) + 1) * U * terms.abs().sum(-1, keepdim=True)        # + 1: x * dy * w is two roundings
    bar_coef = rstd ** 3 / dim * bar_dot + coef.abs() * (3 * rel + 4 * U)      # rstd^3: three factors, three products, / dim
    bar = a.abs() * (rel + 2 * U) + x.abs() * bar_coef + U * b.abs() + U * dx.abs()
    if dx_in is not None:
        dx = dx + f64(dx_in)
        bar = bar + U * dx.abs()
    return dx, bar + R * dx.abs(), rstd, rel


def rmsnorm_bwd(x, w, dy, eps, dx_in=None, bug=None):
    """rmsnorm_bwd_kernel / rmsnorm_bwd_cached_kernel<1>.  -> dx = rstd * w * dy - x * mean(w dy x) rstd^3 (+ dx_in).
    bar["dx_reach"]: see ``reach``."""
    dx, bar, _, _ = _rms_dx(f64(x), f64(w), f64(dy), dx_in, eps, bug)
    return dict(dx=dx), dict(dx=bf16_out(dx, bar), dx_reach=reach(dx, bar))


def _block_last_rows(rows, rpb):
    keep = torch.ones(rows, 1, dtype=F64)
    keep[rpb - 1::rpb] = 0
    keep[rows - 1] = 0
    return keep


def _rms_dw(x, dy, rstd, rel, rpb, bug):
    rows = x.shape[0]
    terms = dy * x * rstd
    if bug == "drop_block_last_row":
        terms = terms * _block_last_rows(rows, rpb)
    dw = terms.sum(0)
    # a term dy * x * rstd: two roundings and rstd's own error
    bar = ((c_colpart(rows, rpb) + 2) * U + rel) * terms.abs().sum(0) + R * dw.abs()
    return dw, bf16_out(dw, bar), reach(dw, bar)


def rmsnorm_bwd_dw(x, dy, eps, bug=None):
    """rmsnorm_dw_partial_kernel<NI> (w == nullptr) + colpart_reduce_kernel.  -> dw = sum_rows dy * x * rstd"""
    x, dy = f64(x), f64(dy)
    rstd, rel = _rms_stats(x, eps, bug)
    dw, bar, rch = _rms_dw(x, dy, rstd, rel, norm_rows_per_block(x.shape[0]), bug)
    return dict(dw=dw), dict(dw=bar, dw_reach=rch)


def rmsnorm_bwd_full(x, w, dy, eps, dx_in=None, bug=None):
    """rmsnorm_dw_partial_kernel<NI> with w + colpart_reduce_kernel (rms_full_rows_per_block).  -> dx, dw"""
    x, w, dy = f64(x), f64(w), f64(dy)
    dx, bar, rstd, rel = _rms_dx(x, w, dy, dx_in, eps, bug)
    dw, bar_dw, rch = _rms_dw(x, dy, rstd, rel, rms_full_rows_per_block(x.shape[0]), bug)
    return dict(dx=dx, dw=dw), dict(dx=bf16_out(dx, bar), dw=bar_dw, dx_reach=reach(dx, bar), dw_reach=rch)


# ---------------------------------------------------------------------------------------------------- activations
def expf_rel(a):
    """relative error of __expf(a) = v_exp_f32(a * log2(e)): the product's rounding and the constant's move the exponent by
    2 * U * |a| log2(e), i.e. the result by 2 |a| U relative; v_exp_f32 itself 1 ulp = 2 U"""
    return (2 * a.abs() + 2) * U


def sigmoid_err(a, a_err=0.0):
    """-> (s, |error| of sigmoid_f(a') = rcp(1 + __expf(-a'))) for |a' - a| <= a_err.  With e = e^-a: the sum 1 + e has
    relative error e * expf_rel / (1 + e) + U = (1 - s) * expf_rel + U, the reciprocal RCP more; the argument's error goes
    through s' = s (1 - s)."""
    s = torch.sigmoid(a)
    rel = (1 - s) * expf_rel(a) + (1 + RCP) * U
    return s, s * rel + s * (1 - s) * a_err + TINY


def _sig_grad(a, a_err, x_is_a=True):
    """-> (g, |error|) of s * (1 + a * (1 - s)), s = sigmoid_f(a): the SiLU' form shared by act_grad and swiglu_bwd_kernel"""
    s, e_s = sigmoid_err(a, a_err)
    om = 1 - s
    e_om = e_s + U * om
    t = a * om
    e_t = a.abs() * e_om + om * a_err + U * t.abs()
    p = 1 + t
    e_p = e_t + U * p.abs()
    g = s * p
    return g, p.abs() * e_s + s * e_p + U * g.abs()


E_ERF = 12 * U      # |error| of 1 + erff(x * C_RSQRT2): the argument's two roundings through erf' <= 2/sqrt(pi) with
#                     |a| e^(-a^2) <= 0.43 (< 2 U), erff 4 ulp of |erf| <= 1 (8 U), the addition (U), 1 U slack.  ABSOLUTE: the
#                     kernel forms 1 + erf, which cancels for x << 0, as torch's own fp32 gelu does


def act_val(x, act, bug=None):
    """-> (y, |error| of the fp32 value act_val / act_f computes) for an exact fp32 argument x"""
    if act == ACT_NONE:
        return x, torch.zeros_like(x)
    if act == ACT_SILU:
        s, e_s = sigmoid_err(x)
        return x * s, x.abs() * e_s + U * (x * s).abs()
    if act == ACT_QUICK_GELU:
        a = C_QUICK * x
        s, e_s = sigmoid_err(a, 2 * U * a.abs())                   # 1.702f and the product
        return x * s, x.abs() * e_s + U * (x * s).abs()
    if act == ACT_GELU:
        y = 0.5 * x * (1 + torch.erf(x * C_RSQRT2))
        return y, 0.5 * x.abs() * E_ERF + 2 * U * y.abs()
    raise KeyError(act)


def act_grad(x, act, bug=None):
    """-> (act'(x), |error| of the fp32 value act_grad computes) for an exact fp32 argument x"""
    if act == ACT_NONE:
        return torch.ones_like(x), torch.zeros_like(x)
    if act == ACT_SILU:
        if bug == "silu_grad_no_x":
            return torch.sigmoid(x), torch.zeros_like(x)
        return _sig_grad(x, 0.0)
    if act == ACT_QUICK_GELU:
        if bug == "quick_grad_1":
            s = torch.sigmoid(C_QUICK * x)
            return s * (1 + x * (1 - s)), torch.zeros_like(x)
        a = C_QUICK * x
        return _sig_grad(a, 2 * U * a.abs())
    if act == ACT_GELU:
        q = 0.5 * x * x
        pdf = x * C_PDF * torch.exp(-q)
        g = 0.5 * (1 + torch.erf(x * C_RSQRT2)) + pdf
        # -0.5f * x * x: one rounding of the exponent (q U relative in the result), __expf, two products and the constant
        e_pdf = pdf.abs() * (q * U + expf_rel(q) + 3 * U) + TINY * x.abs()
        return g, 0.5 * E_ERF + e_pdf + U * g.abs()
    raise KeyError(act)


SILU_D2_MAX = 0.5       # max |SiLU''| (at 0): how an error of the recomputed pre-activation reaches SiLU' in layernorm_bwd_kernel


def act_fwd(x, act, bug=None):
    """act_fwd_kernel"""
    y, e = act_val(f64(x), act, bug)
    return dict(y=y), dict(y=bf16_out(y, e), y_reach=reach(y, e))


def act_bwd(x, dy, act, bug=None):
    """act_bwd_kernel.  -> dx = dy * act'(x)"""
    dy = f64(dy)
    g, e = act_grad(f64(x), act, bug)
    dx = dy * g
    b32 = dy.abs() * e + U * dx.abs()
    return dict(dx=dx), dict(dx=bf16_out(dx, b32), dx_reach=reach(dx, b32))


def swiglu_fwd(gu, bug=None):
    """swiglu_fwd_kernel.  gu = [gate | up] -> silu(gate) * up"""
    gu = f64(gu)
    ff = gu.shape[1] // 2
    g, u = gu[:, :ff], gu[:, ff:]
    s, e = act_val(g, ACT_SILU)
    y = s * u
    b32 = u.abs() * e + U * y.abs()
    return dict(y=y), dict(y=bf16_out(y, b32), y_reach=reach(y, b32))


def swiglu_bwd(gu, dout, bug=None):
    """swiglu_bwd_kernel.  -> dgu = [dout * up * silu'(gate) | dout * silu(gate)]"""
    gu, d = f64(gu), f64(dout)
    ff = gu.shape[1] // 2
    g, u = gu[:, :ff], gu[:, ff:]
    si, e_si = act_val(g, ACT_SILU)
    gr, e_gr = act_grad(g, ACT_SILU, bug)
    du, dg = d * si, d * u * gr
    bar_du = d.abs() * e_si + U * du.abs()
    bar_dg = (d * u).abs() * e_gr + 2 * U * dg.abs()
    dgu, b32 = torch.cat([dg, du], 1), torch.cat([bar_dg, bar_du], 1)
    return dict(dgu=dgu), dict(dgu=bf16_out(dgu, b32), dgu_reach=reach(dgu, b32))


# ---------------------------------------------------------------------------------------------------- LayerNorm
def _ln_stats(x, eps, bug):
    """-> mean-free d, rstd, xhat and their bars.  mean: c_stat * U * mean|x|; d = x - mean: the mean's absolute error and
    the subtraction's rounding; var = mean(d^2): its own chain and what the d carry; rstd: half the root's argument's
    relative error (eps included in the argument: a constant row's noise is judged against eps, not against itself)"""
    dim = x.shape[-1]
    c = c_stat(dim)
    cols = torch.ones(dim, dtype=F64)
    if bug == "drop_last8":
        cols[-8:] = 0
    mean = (x * cols).sum(-1, keepdim=True) / dim
    d = x - mean
    if bug == "onepass_var32":
        x32 = x.to(F32)
        var = f64((x32 * x32).sum(-1, keepdim=True) / dim - (x32.sum(-1, keepdim=True) / dim) ** 2)
    else:
        var = (d * d * cols).sum(-1, keepdim=True) / dim
    if bug == "eps_outside":
        rstd = 1.0 / (var.sqrt() + eps)
    else:
        rstd = (var + (0.1 * eps if bug == "eps_tenth" else eps)).rsqrt()
    bar_d = c * U * x.abs().sum(-1, keepdim=True) / dim + U * mean.abs() + U * d.abs()
    bar_var = (c + 2) * U * var + (2 * (d.abs() * bar_d).sum(-1, keepdim=True) + (bar_d * bar_d).sum(-1, keepdim=True)) / dim
    rel = 0.5 * bar_var / (var + eps) + RSQ * U + R
    xh = d * rstd
    bar_xh = rstd * bar_d + (rel + U) * xh.abs()
    return d, rstd, rel, xh, bar_xh


def _ln_z(x, w, b, res, eps, bug):
    d, rstd, rel, xh, bar_xh = _ln_stats(x, eps, bug)
    z = xh * w + b
    bar_z = w.abs() * bar_xh + 2 * U * ((xh * w).abs() + b.abs())
    if res is not None and bug != "res_after_act":
        z = z + res
        bar_z = bar_z + U * z.abs()
    return z, bar_z, rstd, rel, xh, bar_xh


def layernorm_fwd(x, w, b, eps, res=None, act=ACT_NONE, bug=None):
    """layernorm_fwd_kernel / layernorm_fwd_cached_kernel<NI>.  -> y = act(LN(x; w, b) + res)"""
    x, w, b = f64(x), f64(w), f64(b)
    res = None if res is None else f64(res)
    z, bar_z, *_ = _ln_z(x, w, b, res, eps, bug)
    y, e = act_val(z, act)
    g, _ = act_grad(z, act)
    if bug == "res_after_act" and res is not None:
        y = y + res
    b32 = g.abs() * bar_z + e + R * y.abs()
    return dict(y=y), dict(y=bf16_out(y, b32), y_reach=reach(y, b32))


def layernorm_bwd(x, w, b, dy, eps, res=None, act=ACT_NONE, bug=None):
    """layernorm_bwd_kernel<NI> + 2 x colpart_reduce_kernel.  -> dx, dres (= dz, through the activation), dw, db"""
    assert act in (ACT_NONE, ACT_SILU)
    x, w, b, dy = f64(x), f64(w), f64(b), f64(dy)
    rows, dim = x.shape
    c = c_stat(dim)
    z, bar_z, rstd, rel, xh, bar_xh = _ln_z(x, w, b, None if res is None else f64(res), eps, bug)
    if act == ACT_NONE:
        dz, bar_dz = dy, torch.zeros_like(dy)
    else:
        g, e = act_grad(z, act, bug)
        dz = dy * g
        bar_dz = dy.abs() * (SILU_D2_MAX * bar_z + e) + U * dz.abs()
    gw = dz * w
    bar_gw = w.abs() * bar_dz + U * gw.abs()
    s1 = gw.sum(-1, keepdim=True) / dim
    s2 = (gw * xh).sum(-1, keepdim=True) / dim
    mean = lambda t: t.sum(-1, keepdim=True) / dim
    bar_s1 = (c + 1) * U * mean(gw.abs()) + mean(bar_gw)
    bar_s2 = (c + 2) * U * mean((gw * xh).abs()) + mean(bar_gw * xh.abs() + gw.abs() * bar_xh)
    inner = gw - s1 - xh * s2
    dx = rstd * inner
    bar_in = bar_gw + bar_s1 + xh.abs() * bar_s2 + s2.abs() * bar_xh + 2 * U * (gw.abs() + s1.abs() + (xh * s2).abs())
    bar_dx = rstd * bar_in + (rel + U) * dx.abs() + R * dx.abs()
    rpb = norm_rows_per_block(rows)
    tg, tb = dz * xh, dz
    if bug == "drop_block_last_row":
        keep = _block_last_rows(rows, rpb)
        tg, tb = tg * keep, tb * keep
    dw, db = tg.sum(0), tb.sum(0)
    cc = c_colpart(rows, rpb)
    bar_dw = cc * U * tg.abs().sum(0) + (bar_dz * xh.abs() + dz.abs() * bar_xh + U * tg.abs()).sum(0) + R * dw.abs()
    bar_db = cc * U * tb.abs().sum(0) + bar_dz.sum(0) + R * db.abs()
    ref = dict(dx=dx, dres=dz, dw=dw, db=db)
    bar = {}
    for k, b32 in (("dx", bar_dx), ("dres", bar_dz), ("dw", bar_dw), ("db", bar_db)):
        bar[k], bar[k + "_reach"] = bf16_out(ref[k], b32), reach(ref[k], b32)
    return ref, bar


def dres_vs_act_bwd_bar(y_pre, dy):
    """|dres - act_bwd(y_pre, dy, SiLU)|, y_pre = layernorm(..., act = NONE) of the same inputs: the bf16 rounding of the
    pre-activation (2^-8 |z|, and the forward's own fp32 error, below a tenth of that) through |SiLU''| <= 0.5, and the two
    bf16 roundings of the results"""
    y_pre, dy = f64(y_pre), f64(dy)
    g, e = act_grad(y_pre, ACT_SILU)
    return dy.abs() * (SILU_D2_MAX * 1.1 * HB * y_pre.abs() + 2 * e) + 2 * HB * (1 + HB) * (dy * g).abs()


# ---------------------------------------------------------------------------------------------------- RoPE, sums, add
def rope(x, cos, sin, S, heads, D, sign, pos=None, bug=None):
    """rope_kernel, on the first heads * D columns; the rest of a row is returned unchanged (and must stay bit-identical)"""
    x, cos, sin = f64(x), f64(cos), f64(sin)
    rows, half = x.shape[0], D // 2
    p = torch.arange(rows) % S if pos is None or bug == "rope_pos_mod" else pos.long()
    co, si = cos[p][:, None, :], sign * sin[p][:, None, :]
    v = x[:, : heads * D].reshape(rows, heads, D)
    a, b = v[..., :half], v[..., half:]
    oa = a * co - b * si
    ob = b * co + a * si * (-1 if bug == "rope_half_sign" else 1)
    mag = (a * co).abs() + (b * si).abs(), (b * co).abs() + (a * si).abs()
    out, bar, b32 = x.clone(), torch.zeros_like(x), torch.zeros_like(x)
    out[:, : heads * D] = torch.cat([oa, ob], -1).reshape(rows, heads * D)
    # two products and one addition: c = 1 + 2
    bar[:, : heads * D] = torch.cat([bf16_out(oa, 3 * U * mag[0]), bf16_out(ob, 3 * U * mag[1])], -1).reshape(rows, heads * D)
    b32[:, : heads * D] = 3 * U * torch.cat(mag, -1).reshape(rows, heads * D)
    return dict(x=out), dict(x=bar, x_reach=(out - b32, out + b32))            # (the untouched tail: exactly itself)


def colsum(x, dim, bug=None):
    """colsum_partial_kernel + colpart_reduce_kernel on the first dim columns of x [rows, ld]"""
    x = f64(x)[:, :dim]
    rows = x.shape[0]
    s = x.sum(0)
    b32 = c_colsum(rows, norm_rows_per_block(rows)) * U * x.abs().sum(0) + R * s.abs()
    return dict(out=s), dict(out=bf16_out(s, b32), out_reach=reach(s, b32))


def embed_grad(d, tok, beg, rows, D, vocab, bug=None):
    """embed_grad_kernel.  -> dE [vocab, D] with NaN in the rows no job names (they must stay untouched); a job's sum is one
    chain of its n occurrences (``for o``): c = n + 2"""
    d = f64(d)[:, :D]
    out = torch.full((vocab, D), float("nan"), dtype=F64)
    bar, b32 = torch.zeros(vocab, D, dtype=F64), torch.zeros(vocab, D, dtype=F64)
    for j, t in enumerate(tok.tolist()):
        sel = d[rows[int(beg[j]):int(beg[j + 1])].long()]
        out[t] = sel.sum(0)
        b32[t] = (sel.shape[0] + 2) * U * sel.abs().sum(0)
        bar[t] = bf16_out(out[t], b32[t])
    return dict(dE=out), dict(dE=bar, dE_reach=reach(out, b32))


def add(a, b, bug=None):
    """add_kernel: one fp32 addition, one bf16 rounding"""
    y = f64(a) + f64(b)
    return dict(y=y), dict(y=bf16_out(y, U * y.abs()), y_reach=reach(y, U * y.abs()))


# ---------------------------------------------------------------------------------------------------- fp32 restatement
# The kernels' arithmetic in numpy float32, in the kernels' order per lane, per wave butterfly and per partial slab (no
# fma contraction: every product and sum rounds).  It shows on the CPU that honest fp32 meets the bars.
f32 = np.float32


def _np(t):
    return t.to(F32).numpy()


def _bf(a):
    """numpy float32 -> rounded to bf16, as float32"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(BF16).to(F32).numpy()


def wave_sum32(terms):
    """[rows, dim] -> [rows, 1]: lane l adds columns 8l + 512k + i (k outer, i inner), then v += shfl_xor(v, o), o = 32 .. 1"""
    rows, dim = terms.shape
    nt = cdiv(dim, 512)
    pad = np.zeros((rows, nt * 512), dtype=f32)
    pad[:, :dim] = terms
    t = pad.reshape(rows, nt, 64, 8)
    acc = np.zeros((rows, 64), dtype=f32)
    for k in range(nt):
        for i in range(8):
            acc = acc + t[:, k, :, i]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ o]
    return acc[:, :1]


def colpart32(terms, rpb):
    """[rows, dim] -> [dim]: wave w of a block adds rows w, w + 4, ... of the block's rpb; ((w0 + w1) + w2) + w3; then
    colpart_reduce_kernel: group g adds partials g, g + 8, ...; the 8 groups in order"""
    rows, dim = terms.shape
    nb = cdiv(rows, rpb)
    pad = np.zeros((nb * rpb, dim), dtype=f32)
    pad[:rows] = terms
    t = pad.reshape(nb, rpb // 4, 4, dim)
    w = np.zeros((nb, 4, dim), dtype=f32)
    for j in range(rpb // 4):
        w = w + t[:, j]
    return colpart_reduce32(((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3])


def colpart_reduce32(part):
    nb, dim = part.shape
    pad = np.zeros((cdiv(nb, 8) * 8, dim), dtype=f32)
    pad[:nb] = part
    p = pad.reshape(-1, 8, dim)
    grp = np.zeros((8, dim), dtype=f32)
    for j in range(p.shape[0]):
        grp = grp + p[j]
    t = grp[0]
    for k in range(1, 8):
        t = t + grp[k]
    return t


def _rstd32(ss, dim, eps):
    return (f32(1) / np.sqrt(ss / f32(dim) + f32(eps))).astype(f32)


def sigmoid32(x):
    with np.errstate(over="ignore"):
        return (f32(1) / (f32(1) + np.exp(-x, dtype=f32))).astype(f32)


def act_val32(x, act):
    if act == ACT_SILU:
        return x * sigmoid32(x)
    if act == ACT_QUICK_GELU:
        with np.errstate(over="ignore"):
            return x * sigmoid32(f32(1.702) * x)
    if act == ACT_GELU:
        erf = torch.erf(torch.from_numpy(x * f32(0.70710678118654752))).numpy()
        return f32(0.5) * x * (f32(1) + erf)
    return x


def act_grad32(x, act):
    with np.errstate(over="ignore", invalid="ignore"):
        if act == ACT_SILU:
            s = sigmoid32(x)
            return s * (f32(1) + x * (f32(1) - s))
        if act == ACT_QUICK_GELU:
            a = quick_arg32(x)
            s = sigmoid32(a)
            return s * (f32(1) + a * (f32(1) - s))
        if act == ACT_GELU:
            erf = torch.erf(torch.from_numpy(x * f32(0.70710678118654752))).numpy()
            return f32(0.5) * (f32(1) + erf) + x * f32(0.3989422804014327) * np.exp(f32(-0.5) * x * x, dtype=f32)
    return np.ones_like(x)


def quick_arg32(x):
    """1.702f * x as act_grad forms it: past +-3e38 (where the product overflows) the finite stand-in"""
    with np.errstate(over="ignore"):
        t = f32(1.702) * x
    return np.where(np.abs(t) > f32(3.0e38), np.copysign(f32(3.0e38), t), t).astype(f32)


def emu_rmsnorm_fwd(x, w, eps):
    x, w = _np(x), _np(w)
    rstd = _rstd32(wave_sum32(x * x), x.shape[1], eps)
    return dict(y=_bf(w * _bf(x * rstd)))


def _emu_rms_dx(x, w, dy, dx_in, eps):
    dim = x.shape[1]
    rstd = _rstd32(wave_sum32(x * x), dim, eps)
    coef = wave_sum32(x * dy * w) * rstd * rstd * rstd / f32(dim)
    o = rstd * w * dy - coef * x
    if dx_in is not None:
        o = o + _np(dx_in)
    return _bf(o), rstd


def emu_rmsnorm_bwd(x, w, dy, eps, dx_in=None):
    return dict(dx=_emu_rms_dx(_np(x), _np(w), _np(dy), dx_in, eps)[0])


def emu_rmsnorm_bwd_dw(x, dy, eps):
    x, dy = _np(x), _np(dy)
    rstd = _rstd32(wave_sum32(x * x), x.shape[1], eps)
    return dict(dw=_bf(colpart32(dy * x * rstd, norm_rows_per_block(x.shape[0]))))


def emu_rmsnorm_bwd_full(x, w, dy, eps, dx_in=None):
    x, w, dy = _np(x), _np(w), _np(dy)
    dx, rstd = _emu_rms_dx(x, w, dy, dx_in, eps)
    return dict(dx=dx, dw=_bf(colpart32(dy * x * rstd, rms_full_rows_per_block(x.shape[0]))))


def _emu_ln_stats(x, eps):
    dim = x.shape[1]
    mean = wave_sum32(x) / f32(dim)
    d = x - mean
    return d, _rstd32(wave_sum32(d * d), dim, eps)


def emu_layernorm_fwd(x, w, b, eps, res=None, act=ACT_NONE):
    x, w, b = _np(x), _np(w), _np(b)
    d, rstd = _emu_ln_stats(x, eps)
    v = d * rstd * w + b
    if res is not None:
        v = v + _np(res)
    return dict(y=_bf(act_val32(v, act)))


def emu_layernorm_bwd(x, w, b, dy, eps, res=None, act=ACT_NONE):
    x, w, b, dz = _np(x), _np(w), _np(b), _np(dy)
    rows, dim = x.shape
    d, rstd = _emu_ln_stats(x, eps)
    xh = d * rstd
    if act != ACT_NONE:
        z = xh * w + b
        if res is not None:
            z = z + _np(res)
        dz = dz * act_grad32(z, act)
    s1 = wave_sum32(dz * w) / f32(dim)
    s2 = wave_sum32(dz * w * xh) / f32(dim)
    dx = rstd * (dz * w - s1 - xh * s2)
    rpb = norm_rows_per_block(rows)
    return dict(dx=_bf(dx), dres=_bf(dz), dw=_bf(colpart32(dz * xh, rpb)), db=_bf(colpart32(dz, rpb)))


def emu_rope(x, cos, sin, S, heads, D, sign, pos=None):
    out = _np(x).copy()
    rows, half = out.shape[0], D // 2
    p = np.arange(rows) % S if pos is None else pos.numpy()
    co, si = cos.numpy()[p][:, None, :], f32(sign) * sin.numpy()[p][:, None, :]
    v = out[:, : heads * D].reshape(rows, heads, D)
    a, b = v[..., :half], v[..., half:]
    out[:, : heads * D] = np.concatenate([_bf(a * co - b * si), _bf(b * co + a * si)], -1).reshape(rows, heads * D)
    return dict(x=out)


def emu_swiglu_fwd(gu):
    gu = _np(gu)
    ff = gu.shape[1] // 2
    return dict(y=_bf(act_val32(gu[:, :ff], ACT_SILU) * gu[:, ff:]))


def emu_swiglu_bwd(gu, dout):
    gu, d = _np(gu), _np(dout)
    ff = gu.shape[1] // 2
    g, u = gu[:, :ff], gu[:, ff:]
    sg = sigmoid32(g)
    return dict(dgu=np.concatenate([_bf(d * u * (sg * (f32(1) + g * (f32(1) - sg)))), _bf(d * (g * sg))], 1))


def emu_act_fwd(x, act):
    return dict(y=_bf(act_val32(_np(x), act)))


def emu_act_bwd(x, dy, act):
    return dict(dx=_bf(_np(dy) * act_grad32(_np(x), act)))


def emu_colsum(x, dim):
    x = _np(x)[:, :dim]
    rows = x.shape[0]
    rpb = norm_rows_per_block(rows)
    nb = cdiv(rows, rpb)
    pad = np.zeros((nb * rpb, dim), dtype=f32)
    pad[:rows] = x
    t = pad.reshape(nb, rpb, dim)
    acc = np.zeros((nb, dim), dtype=f32)
    for r in range(rpb):
        acc = acc + t[:, r]
    return dict(out=_bf(colpart_reduce32(acc)))


def emu_embed_grad(d, tok, beg, rows, D, vocab):
    d = _np(d)[:, :D]
    out = np.full((vocab, D), np.nan, dtype=f32)
    for j, t in enumerate(tok.tolist()):
        acc = np.zeros(D, dtype=f32)
        for o in range(int(beg[j]), int(beg[j + 1])):
            acc = acc + d[int(rows[o])]
        out[t] = _bf(acc)
    return dict(dE=out)


def emu_add(a, b):
    return dict(y=_bf(_np(a) + _np(b)))


# ---------------------------------------------------------------------------------------------------- variants
def norm_variants(op):
    """the argument combinations of one norm operation: [(label, kwargs)]"""
    if op in ("rmsnorm_fwd", "rmsnorm_bwd_dw"):
        return [("", {})]
    if op in ("rmsnorm_bwd", "rmsnorm_bwd_full"):
        return [("plain", dict(dx_in=False)), ("dx_in", dict(dx_in=True))]
    if op == "layernorm_fwd":
        return [(f"act{a}{'+res' if r else ''}", dict(act=a, res=r)) for a in (0, 1, 2, 3) for r in (False, True)]
    if op == "layernorm_bwd":
        return [(f"act{a}{'+res' if r else ''}", dict(act=a, res=r)) for a in (ACT_NONE, ACT_SILU) for r in (False, True)]
    raise KeyError(op)


def norm_call(op, inp, kw, emu=False, bug=None):
    """one norm operation on the inputs of a case: the fp64 stage (-> ref, bar) or the fp32 restatement (-> outputs)"""
    x, xl, w, b, dy = inp["x"], inp["xl"], inp["w"], inp["b"], inp["dy"]
    dxi = inp["dx_in"] if kw.get("dx_in") else None
    res = inp["res"] if kw.get("res") else None
    extra = {} if emu else dict(bug=bug)
    if op == "rmsnorm_fwd":
        return (emu_rmsnorm_fwd if emu else rmsnorm_fwd)(x, w, EPS_RMS, **extra)
    if op == "rmsnorm_bwd":
        return (emu_rmsnorm_bwd if emu else rmsnorm_bwd)(x, w, dy, EPS_RMS, dx_in=dxi, **extra)
    if op == "rmsnorm_bwd_dw":
        return (emu_rmsnorm_bwd_dw if emu else rmsnorm_bwd_dw)(x, dy, EPS_RMS, **extra)
    if op == "rmsnorm_bwd_full":
        return (emu_rmsnorm_bwd_full if emu else rmsnorm_bwd_full)(x, w, dy, EPS_RMS, dx_in=dxi, **extra)
    if op == "layernorm_fwd":
        return (emu_layernorm_fwd if emu else layernorm_fwd)(xl, w, b, EPS_LN, res=res, act=kw["act"], **extra)
    if op == "layernorm_bwd":
        return (emu_layernorm_bwd if emu else layernorm_bwd)(xl, w, b, dy, EPS_LN, res=res, act=kw["act"], **extra)
    raise KeyError(op)


# ---------------------------------------------------------------------------------------------------- planted bugs
# bug -> [(operation, variant kwargs, case id)] at which at least one output must leave its bar
_SILU_RES = dict(act=ACT_SILU, res=True)
BUGS = {
    "eps_outside": [("rmsnorm_fwd", {}, "37x520"), ("rmsnorm_bwd", dict(dx_in=False), "5x1160"), ("layernorm_fwd", dict(act=0, res=False), "37x4104"),
                    ("layernorm_bwd", dict(act=0, res=False), "37x264")],
    "eps_tenth": [("rmsnorm_fwd", {}, "37x6144"), ("rmsnorm_bwd_dw", {}, "37x8"), ("rmsnorm_bwd_full", dict(dx_in=True), "37x2056"),
                  ("layernorm_fwd", dict(act=3, res=True), "37x1024"), ("layernorm_bwd", _SILU_RES, "1030x64")],
    "onepass_var32": [("layernorm_fwd", dict(act=0, res=False), "37x512"), ("layernorm_fwd", dict(act=0, res=False), "37x6144"),
                      ("layernorm_bwd", dict(act=0, res=False), "37x4096")],
    "drop_last8": [("rmsnorm_fwd", {}, "37x4104"), ("rmsnorm_fwd", {}, "4x520"), ("rmsnorm_bwd", dict(dx_in=True), "37x1032"),
                   ("rmsnorm_bwd_dw", {}, "37x2056"), ("rmsnorm_bwd_full", dict(dx_in=False), "4x4096"),
                   ("layernorm_fwd", dict(act=0, res=True), "37x4104"), ("layernorm_bwd", _SILU_RES, "37x1160")],
    "drop_block_last_row": [("rmsnorm_bwd_dw", {}, "37x264"), ("rmsnorm_bwd_dw", {}, "1030x64"), ("rmsnorm_bwd_full", dict(dx_in=False), "4101x64"),
                            ("layernorm_bwd", _SILU_RES, "1030x64"), ("layernorm_bwd", dict(act=0, res=False), "5x520")],
    "padded_width": [("rmsnorm_bwd", dict(dx_in=False), "37x264"), ("rmsnorm_bwd", dict(dx_in=True), "37x4104"),
                     ("rmsnorm_bwd_full", dict(dx_in=False), "37x1160"), ("rmsnorm_bwd_full", dict(dx_in=True), "37x2056")],
    "rope_half_sign": [("rope", None, "D16-h1-seq-fwd"), ("rope", None, "D128-h3-pos-bwd")],
    "rope_pos_mod": [("rope", None, "D16-h3-pos-fwd"), ("rope", None, "D64-h1-pos-bwd")],
    "silu_grad_no_x": [("act_bwd", None, "silu"), ("swiglu_bwd", None, "1x8"), ("swiglu_bwd", None, "70x264"), ("layernorm_bwd", _SILU_RES, "37x520")],
    "res_after_act": [("layernorm_fwd", dict(act=3, res=True), "37x264"), ("layernorm_fwd", dict(act=1, res=True), "1x6144"),
                      ("layernorm_fwd", dict(act=2, res=True), "37x2048")],
    "quick_grad_1": [("act_bwd", None, "quick_gelu")],
}


# ---------------------------------------------------------------------------------------------------- the check
def ratio(got, ref, bar):
    """max |got - ref| / bar (0 where both agree exactly, NaN in ref = "must be NaN in got", inf for any other NaN)"""
    got = torch.as_tensor(got).to(F64)
    both_nan = torch.isnan(ref) & torch.isnan(got)
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bar.clamp_min(1e-300))
    r = torch.where(both_nan, torch.zeros_like(r), r)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


def outside(got, ref, bar):
    """{output: number of elements outside [bf16(lo), bf16(hi)]} (see ``reach``; NaN in ref: not judged here)"""
    out = {}
    for k in ref:
        lo, hi = bar[k + "_reach"]
        g = torch.as_tensor(got[k]).to(F64)
        out[k] = int((~((g >= rbf(lo)) & (g <= rbf(hi))) & ~torch.isnan(ref[k])).sum())
    return out


def ratios(got, ref, bar):
    """{output: max(err / bar)} over every output of one stage"""
    return {k: ratio(got[k], ref[k], bar[k]) for k in ref}
