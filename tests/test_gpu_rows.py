"""The norm, RoPE, SwiGLU, activation, column-sum, embedding-gradient and add kernels (csrc/ops.hip, csrc/train.hip), one
operation at a time, per element against the fp64 restatement of tests/rows_emul.py.

Every output lies in a buffer pre-filled with NaN with guard rows before and behind it (and guard columns where the
operation takes a row stride): after the call the written region holds no NaN and the guard is bit-untouched.  Each case
names, as literals, the kernel instantiation and rows_per_block it is there for, and fails if rows_emul.paths, a Python
restatement of the launchers' branch conditions (held to the source text by test_cpu_rows_emul), does not lead there.
Bars: rows_emul.py; test_cpu_rows_emul.py shows on the CPU that honest fp32 meets them and that eleven planted bugs do not.
Run with -s to see max(err / bar) per operation, case and output."""
import pytest
import torch

import rows_emul as E

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
G = 2                     # guard rows on either side of an output


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Out:
    """[rows, cols] bf16 output inside a NaN-filled [G + rows + G, ld] buffer"""

    def __init__(self, dev, rows, cols, ld=None, fill=None):
        ld = cols if ld is None else ld
        self.full = torch.full((G + rows + G, ld), float("nan"), dtype=BF, device=dev)
        if fill is not None:
            self.full[G:G + rows] = fill.to(dev)
        self.view = self.full[G:G + rows, :cols] if ld != cols else self.full[G:G + rows]
        self.inside = torch.zeros(G + rows + G, ld, dtype=torch.bool, device=dev)
        self.inside[G:G + rows, :cols] = True
        self.before = self.full.clone()

    @property
    def vec(self):
        assert self.view.shape[0] == 1
        return self.view[0]

    def host(self, written=None):
        """-> the written region on the host, after checking that it is finite and that nothing else changed"""
        torch.cuda.synchronize()
        inside = self.inside if written is None else written
        assert bool(torch.isfinite(self.full[inside].float()).all()), "NaN / inf in the written region"
        assert torch.equal(self.full.view(torch.int16)[~inside], self.before.view(torch.int16)[~inside]), "guard region touched"
        return self.view.float().cpu()


def _report(what, got, ref, bar):
    """max(err / bar) per output <= 1, and every element within the bf16 values its fp32 bar can reach (rows_emul.reach)"""
    r, out = E.ratios(got, ref, bar), E.outside(got, ref, bar)
    print(what, {k: round(v, 3) for k, v in r.items()}, "outside:", out)
    assert all(v <= 1.0 for v in r.values()), (what, r)
    assert not any(out.values()), (what, out)


def _expect(op, c):
    assert E.paths(op, c["rows"], c["dim"]) == c["expect"][op], (op, c["id"])


def _dev_inputs(dev, kind, cid):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in E.inputs_for(kind, cid).items()}


def _ids(cases):
    return [c["id"] for c in cases]


# ---------------------------------------------------------------------------------------------------- launches
def _rmsnorm_bwd_dw(d, out):
    from phantom_vlb_amd import ops
    ops.rmsnorm_bwd_dw(d["x"], d["dy"], E.EPS_RMS, out.vec)


def _rmsnorm_bwd_full(d, dx_in, dx, dw):
    """vlb_rmsnorm_bwd_full on caller-owned outputs (ops.rmsnorm_bwd_full allocates dx itself)"""
    from phantom_vlb_amd._lib import check, lib
    rows, dim = d["x"].shape
    ws = torch.empty(int(lib.vlb_rmsnorm_bwd_full_ws_floats(rows, dim)), dtype=torch.float32, device=d["x"].device)
    check(lib.vlb_rmsnorm_bwd_full(d["x"].data_ptr(), d["w"].data_ptr(), d["dy"].data_ptr(), None if dx_in is None else dx_in.data_ptr(),
                                   dx.view.data_ptr(), dw.vec.data_ptr(), ws.data_ptr(), rows, dim, E.EPS_RMS, _stream()), "vlb_rmsnorm_bwd_full")


def _layernorm_bwd(d, res, act, dx, dres, dw, db):
    from phantom_vlb_amd._lib import check, lib
    rows, dim = d["xl"].shape
    ws = torch.empty(int(lib.vlb_norm_bwd_ws_floats(rows, dim)), dtype=torch.float32, device=d["xl"].device)
    check(lib.vlb_layernorm_bwd(d["xl"].data_ptr(), d["w"].data_ptr(), d["b"].data_ptr(), None if res is None else res.data_ptr(),
                                d["dy"].data_ptr(), dx.view.data_ptr(), dres.view.data_ptr(), dw.vec.data_ptr(), db.vec.data_ptr(),
                                ws.data_ptr(), rows, dim, E.EPS_LN, act, _stream()), "vlb_layernorm_bwd")


def _run_norm(dev, op, c, d, kw):
    """one launch of a norm operation into guarded outputs -> {name: host tensor}"""
    from phantom_vlb_amd import ops
    rows, dim = c["rows"], c["dim"]
    dxi = d["dx_in"] if kw.get("dx_in") else None
    res = d["res"] if kw.get("res") else None
    if op == "rmsnorm_fwd":
        y = Out(dev, rows, dim)
        ops.rmsnorm(d["x"], d["w"], E.EPS_RMS, out=y.view)
        return dict(y=y.host())
    if op == "rmsnorm_bwd":
        dx = Out(dev, rows, dim)
        ops.rmsnorm_bwd(d["x"], d["w"], d["dy"], E.EPS_RMS, dx_in=dxi, out=dx.view)
        return dict(dx=dx.host())
    if op == "rmsnorm_bwd_dw":
        dw = Out(dev, 1, dim, ld=dim + 8)
        _rmsnorm_bwd_dw(d, dw)
        return dict(dw=dw.host()[0])
    if op == "rmsnorm_bwd_full":
        dx, dw = Out(dev, rows, dim), Out(dev, 1, dim, ld=dim + 8)
        _rmsnorm_bwd_full(d, dxi, dx, dw)
        return dict(dx=dx.host(), dw=dw.host()[0])
    if op == "layernorm_fwd":
        y = Out(dev, rows, dim)
        ops.layernorm(d["xl"], d["w"], d["b"], E.EPS_LN, residual=res, act=kw["act"], out=y.view)
        return dict(y=y.host())
    if op == "layernorm_bwd":
        dx, dres, dw, db = Out(dev, rows, dim), Out(dev, rows, dim), Out(dev, 1, dim, ld=dim + 8), Out(dev, 1, dim, ld=dim + 8)
        _layernorm_bwd(d, res, kw["act"], dx, dres, dw, db)
        return dict(dx=dx.host(), dres=dres.host(), dw=dw.host()[0], db=db.host()[0])
    raise KeyError(op)


def _norm_test(dev, op, cid):
    c = E.BY_ID[("norm", cid)]
    _expect(op, c)
    d = _dev_inputs(dev, "norm", cid)
    for label, kw in E.norm_variants(op):
        got = _run_norm(dev, op, c, d, kw)
        ref, bar = E.norm_call(op, E.inputs_for("norm", cid), kw)
        _report(f"{op} {cid} {label} {c['expect'][op]}", got, ref, bar)


# ---------------------------------------------------------------------------------------------------- the norms
@pytest.mark.parametrize("cid", _ids(E.norm_cases("rmsnorm_fwd")))
def test_rmsnorm_fwd(dev, cid):
    _norm_test(dev, "rmsnorm_fwd", cid)


@pytest.mark.parametrize("cid", _ids(E.norm_cases("rmsnorm_bwd")))
def test_rmsnorm_bwd(dev, cid):
    _norm_test(dev, "rmsnorm_bwd", cid)


@pytest.mark.parametrize("cid", _ids(E.norm_cases("rmsnorm_bwd_dw")))
def test_rmsnorm_bwd_dw(dev, cid):
    _norm_test(dev, "rmsnorm_bwd_dw", cid)


@pytest.mark.parametrize("cid", _ids(E.norm_cases("rmsnorm_bwd_full")))
def test_rmsnorm_bwd_full(dev, cid):
    _norm_test(dev, "rmsnorm_bwd_full", cid)


@pytest.mark.parametrize("cid", _ids(E.norm_cases("layernorm_fwd")))
def test_layernorm_fwd(dev, cid):
    _norm_test(dev, "layernorm_fwd", cid)


@pytest.mark.parametrize("cid", _ids(E.norm_cases("layernorm_bwd")))
def test_layernorm_bwd(dev, cid):
    _norm_test(dev, "layernorm_bwd", cid)


# ---------------------------------------------------------------------------------------------------- RoPE
@pytest.mark.parametrize("cid", _ids(E.ROPE_CASES))
def test_rope(dev, cid):
    from phantom_vlb_amd import ops
    c, inp = E.BY_ID[("rope", cid)], E.inputs_for("rope", cid)
    D, h, rows = c["D"], c["heads"], E.ROPE_B * E.ROPE_S
    ld = inp["x"].shape[1]
    assert ld == h * D + 64
    x = Out(dev, rows, ld, fill=inp["x"])
    written = torch.zeros_like(x.inside)
    written[G:G + rows, : h * D] = True                    # the tail of every row is part of the guard: bit-identical
    pos = None if inp["pos"] is None else inp["pos"].to(dev)
    ops.rope_(x.view, inp["cos"].to(dev), inp["sin"].to(dev), E.ROPE_B, E.ROPE_S, h, D, sign=c["sign"], pos=pos)
    got = x.host(written)
    ref, bar = E.rope(inp["x"], inp["cos"], inp["sin"], E.ROPE_S, h, D, c["sign"], pos=inp["pos"])
    _report(f"rope {cid}", dict(x=got), ref, bar)


# ---------------------------------------------------------------------------------------------------- SwiGLU, activations, add
@pytest.mark.parametrize("cid", _ids(E.SWIGLU_CASES))
def test_swiglu_fwd_bwd(dev, cid):
    from phantom_vlb_amd import ops
    c, inp, d = E.BY_ID[("swiglu", cid)], E.inputs_for("swiglu", cid), _dev_inputs(dev, "swiglu", cid)
    y, dgu = Out(dev, c["rows"], c["ff"]), Out(dev, c["rows"], 2 * c["ff"])
    ops.swiglu(d["gu"], out=y.view)
    ops.swiglu_bwd(d["gu"], d["dout"], out=dgu.view)
    ref, bar = E.swiglu_fwd(inp["gu"])
    _report(f"swiglu_fwd {cid}", dict(y=y.host()), ref, bar)
    ref, bar = E.swiglu_bwd(inp["gu"], inp["dout"])
    _report(f"swiglu_bwd {cid}", dict(dgu=dgu.host()), ref, bar)


@pytest.mark.parametrize("cid", _ids(E.ACT_CASES))
def test_act_fwd_bwd(dev, cid):
    from phantom_vlb_amd import ops
    c, inp, d = E.BY_ID[("act", cid)], E.inputs_for("act", cid), _dev_inputs(dev, "act", cid)
    n = inp["x"].numel()
    y, dx = Out(dev, 1, n, ld=n + 8), Out(dev, 1, n, ld=n + 8)
    ops.act_fwd(d["x"], c["act"], out=y.vec)
    ops.act_bwd(d["x"], d["dy"], c["act"], out=dx.vec)
    ref, bar = E.act_fwd(inp["x"], c["act"])
    _report(f"act_fwd {cid}", dict(y=y.host()[0]), ref, bar)
    ref, bar = E.act_bwd(inp["x"], inp["dy"], c["act"])
    _report(f"act_bwd {cid}", dict(dx=dx.host()[0]), ref, bar)


@pytest.mark.parametrize("cid", _ids(E.ADD_CASES))
def test_add(dev, cid):
    from phantom_vlb_amd import ops
    inp, d = E.inputs_for("add", cid), _dev_inputs(dev, "add", cid)
    n = inp["a"].numel()
    y = Out(dev, 1, n, ld=n + 8)
    ops.add(d["a"], d["b"], out=y.vec)
    ref, bar = E.add(inp["a"], inp["b"])
    _report(f"add {cid}", dict(y=y.host()[0]), ref, bar)


# ---------------------------------------------------------------------------------------------------- column sums, embedding gradient
def _colsum(dev, c, d):
    from phantom_vlb_amd import ops
    out = Out(dev, 1, c["dim"], ld=c["dim"] + 8)
    ops.colsum(d["x"][:, : c["dim"]], out.vec)             # a column slice: ld > dim
    return out.host()[0]


@pytest.mark.parametrize("cid", _ids(E.COLSUM_CASES))
def test_colsum(dev, cid):
    c = E.BY_ID[("colsum", cid)]
    assert E.paths("colsum", c["rows"], c["dim"]) == c["expect"]
    ref, bar = E.colsum(E.inputs_for("colsum", cid)["x"], c["dim"])
    _report(f"colsum {cid} {c['expect']}", dict(out=_colsum(dev, c, _dev_inputs(dev, "colsum", cid))), ref, bar)


def _embed_grad(dev, c, d):
    from phantom_vlb_amd import ops
    dE = Out(dev, E.EMBED_VOCAB, c["D"])
    named = torch.zeros_like(dE.inside)
    named[G + d["tok"].long()] = True                      # the rows no job names belong to the guard
    ops.embed_grad(d["d"][:, : c["D"]], d["tok"], d["beg"], d["rows"], dE.view, c["D"])
    dE.host(named)
    return dE.view.float().cpu()


@pytest.mark.parametrize("cid", _ids(E.EMBED_CASES))
def test_embed_grad(dev, cid):
    c, inp = E.BY_ID[("embed", cid)], E.inputs_for("embed", cid)
    got = _embed_grad(dev, c, _dev_inputs(dev, "embed", cid))
    ref, bar = E.embed_grad(inp["d"], inp["tok"], inp["beg"], inp["rows"], c["D"], E.EMBED_VOCAB)
    _report(f"embed_grad {cid}", dict(dE=got), ref, bar)


# ---------------------------------------------------------------------------------------------------- determinism
def test_fixed_order_reductions_repeat_bit_for_bit(dev):
    """train.hip's header: "fixed-order two-stage reduction".  129 partial slabs, uneven colpart groups, twice."""
    cid = "1030x64"
    c, d = E.BY_ID[("norm", cid)], _dev_inputs(dev, "norm", cid)
    for op, kw in (("rmsnorm_bwd_dw", {}), ("rmsnorm_bwd_full", dict(dx_in=True)), ("layernorm_bwd", dict(act=E.ACT_SILU, res=True))):
        a, b = _run_norm(dev, op, c, d, kw), _run_norm(dev, op, c, d, kw)
        for k in a:
            assert torch.equal(a[k], b[k]), (op, k)
    cc = E.BY_ID[("colsum", cid)]
    dc = _dev_inputs(dev, "colsum", cid)
    assert torch.equal(_colsum(dev, cc, dc), _colsum(dev, cc, dc))
    for ce in E.EMBED_CASES:
        de = _dev_inputs(dev, "embed", ce["id"])
        a, b = _embed_grad(dev, ce, de), _embed_grad(dev, ce, de)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), ce["id"]          # (NaN rows included: compare bits)


# ---------------------------------------------------------------------------------------------------- one thing, two ways
@pytest.mark.parametrize("cid", _ids(E.norm_cases("rmsnorm_bwd_full")))
def test_rmsnorm_bwd_full_against_the_separate_kernels(dev, cid):
    """dx: rmsnorm_dw_partial_kernel<NI> evaluates ``rstd * w * dy - coef * x (+ dx_in)`` from the same per-lane sums in the
    same order as rmsnorm_bwd_kernel / rmsnorm_bwd_cached_kernel<1>; the source promises no more (the compiler is free to
    contract the products and sums into fmas differently per kernel).  Both fp32 values lie within the fp32 bar of the fp64
    reference, so both bf16 results lie in [bf16(lo), bf16(hi)] (rows_emul.reach): wherever no rounding boundary is
    within reach that is ONE value and the two outputs have the same bits; elsewhere they differ by at most that span.
    d gamma: with w and without, the partial pass is the same kernel instantiation, so the same bits where both launchers
    take the same rows_per_block (the same slabs); where they do not, the partials are grouped differently, each is held
    to its own fp64 bar, and the two differ by at most the sum of the bars."""
    c, d = E.BY_ID[("norm", cid)], _dev_inputs(dev, "norm", cid)
    inp = E.inputs_for("norm", cid)
    for label, kw in E.norm_variants("rmsnorm_bwd_full"):
        full = _run_norm(dev, "rmsnorm_bwd_full", c, d, kw)
        sep = _run_norm(dev, "rmsnorm_bwd", c, d, kw)
        ref, bar = E.norm_call("rmsnorm_bwd", inp, kw)
        lo, hi = (E.rbf(t) for t in bar["dx_reach"])
        differ = full["dx"] != sep["dx"]
        print(f"rmsnorm_bwd_full vs rmsnorm_bwd {cid} {label}: {int(differ.sum())} of {differ.numel()} dx elements differ, "
              f"{int((lo != hi).sum())} lie at a rounding boundary")
        for got in (full["dx"].double(), sep["dx"].double()):
            assert bool(((got >= lo) & (got <= hi)).all())
        assert not bool((differ & (lo == hi)).any())
    dw_full = _run_norm(dev, "rmsnorm_bwd_full", c, d, dict(dx_in=False))["dw"]
    dw_sep = _run_norm(dev, "rmsnorm_bwd_dw", c, d, {})["dw"]
    if c["expect"]["rmsnorm_bwd_full"][1] == c["expect"]["rmsnorm_bwd_dw"][1]:
        assert torch.equal(dw_full, dw_sep)
    else:
        _, bar_f = E.norm_call("rmsnorm_bwd_full", inp, dict(dx_in=False))
        _, bar_s = E.norm_call("rmsnorm_bwd_dw", inp, {})
        r = E.ratio(dw_full, dw_sep.double(), bar_f["dw"] + bar_s["dw"])
        print(f"rmsnorm_bwd_full vs rmsnorm_bwd_dw {cid}: d gamma {r:.3f} of the two bars")
        assert r <= 1.0


@pytest.mark.parametrize("cid", ["37x264", "37x520", "5x1160", "37x2056", "1030x64"])
def test_layernorm_bwd_dres_against_act_bwd(dev, cid):
    """d residual is dz = dy * act'(z).  Without an activation it is dy, bit for bit.  With SiLU the kernel recomputes z in
    fp32 "exactly as the forward kernel forms it (no intermediate rounding)", so act_bwd on the forward's bf16-rounded
    pre-activation differs by that rounding through SiLU'' and no more (rows_emul.dres_vs_act_bwd_bar)."""
    from phantom_vlb_amd import ops
    c, d = E.BY_ID[("norm", cid)], _dev_inputs(dev, "norm", cid)
    plain = _run_norm(dev, "layernorm_bwd", c, d, dict(act=E.ACT_NONE, res=True))
    assert torch.equal(plain["dres"], d["dy"].float().cpu())
    silu = _run_norm(dev, "layernorm_bwd", c, d, dict(act=E.ACT_SILU, res=True))
    y_pre = ops.layernorm(d["xl"], d["w"], d["b"], E.EPS_LN, residual=d["res"], act=E.ACT_NONE)
    two = ops.act_bwd(y_pre, d["dy"], E.ACT_SILU).float().cpu()
    r = E.ratio(silu["dres"], two.double(), E.dres_vs_act_bwd_bar(y_pre.float().cpu(), d["dy"].float().cpu()))
    print(f"layernorm_bwd dres vs act_bwd {cid}: {r:.3f}")
    assert r <= 1.0
