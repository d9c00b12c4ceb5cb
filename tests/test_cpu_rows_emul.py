"""The row kernels' fp64 reference (tests/rows_emul.py) checked on the CPU: every stage function is the operation (an
independently written fp64 formulation: torch.nn.functional forward, autograd backward, 1e-12), an fp32 restatement of each
kernel's arithmetic in the kernel's own order stays inside every bar at every GPU case, every planted bug leaves a bar, and
``paths`` restates branch conditions that are still in the source."""
import pathlib
import re

import pytest
import torch
import torch.nn.functional as F

import rows_emul as E

F64 = torch.float64
TOL = 1e-12


def _close_rows(a, ref, what):
    """per row: max |a - ref| <= 1e-12 * max |ref| (a row of zeros must be zeros)"""
    err, mag = (a - ref).abs().amax(-1), ref.abs().amax(-1)
    assert bool((err <= TOL * mag).all()), (what, float((err / mag.clamp_min(1e-300)).max()))


def _close_el(a, ref, mag, what):
    err = (a - ref).abs()
    assert bool((err <= TOL * (ref.abs() + mag)).all()), (what, float((err / (ref.abs() + mag).clamp_min(1e-300)).max()))


def _act64(z, act):
    return {0: lambda t: t, 1: lambda t: t * torch.sigmoid(E.C_QUICK * t), 2: F.gelu, 3: F.silu}[act](z)


# ---------------------------------------------------------------------------------------------------- against torch fp64
@pytest.mark.parametrize("cid", ["37x8", "5x520", "37x264", "5x1160"])
def test_rmsnorm_stages_equal_fp64_autograd(cid):
    inp = E.inputs_for("norm", cid)
    x, w, dy, dxi = (inp[k].to(F64) for k in ("x", "w", "dy", "dx_in"))
    dim = x.shape[1]
    ref, _ = E.rmsnorm_fwd(x, w, E.EPS_RMS)
    _close_rows(ref["y"], w * E.rbf(F.rms_norm(x, (dim,), None, E.EPS_RMS)), "rmsnorm_fwd")
    xs, ws = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    F.rms_norm(xs, (dim,), ws, E.EPS_RMS).backward(dy)
    _close_rows(E.rmsnorm_bwd(x, w, dy, E.EPS_RMS)[0]["dx"], xs.grad, "rmsnorm_bwd")
    _close_rows(E.rmsnorm_bwd(x, w, dy, E.EPS_RMS, dx_in=dxi)[0]["dx"], xs.grad + dxi, "rmsnorm_bwd + dx_in")
    _close_rows(E.rmsnorm_bwd_dw(x, dy, E.EPS_RMS)[0]["dw"], ws.grad, "rmsnorm_bwd_dw")
    full, _ = E.rmsnorm_bwd_full(x, w, dy, E.EPS_RMS, dx_in=dxi)
    _close_rows(full["dx"], xs.grad + dxi, "rmsnorm_bwd_full dx")
    _close_rows(full["dw"], ws.grad, "rmsnorm_bwd_full dw")


@pytest.mark.parametrize("cid", ["37x8", "5x520", "37x264"])
@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("res", [False, True])
def test_layernorm_stages_equal_fp64_autograd(cid, act, res):
    inp = E.inputs_for("norm", cid)
    x, w, b, dy = (inp[k].to(F64) for k in ("xl", "w", "b", "dy"))
    dim = x.shape[1]
    xs, ws, bs = (t.clone().requires_grad_(True) for t in (x, w, b))
    rs = inp["res"].to(F64).requires_grad_(True) if res else None
    z = F.layer_norm(xs, (dim,), ws, bs, E.EPS_LN)
    y = _act64(z + rs if res else z, act)
    _close_rows(E.layernorm_fwd(x, w, b, E.EPS_LN, res=inp["res"] if res else None, act=act)[0]["y"], y.detach(), "layernorm_fwd")
    if act in (E.ACT_NONE, E.ACT_SILU):
        y.backward(dy)
        ref, _ = E.layernorm_bwd(x, w, b, dy, E.EPS_LN, res=inp["res"] if res else None, act=act)
        _close_rows(ref["dx"], xs.grad, "layernorm_bwd dx")
        _close_rows(ref["dw"], ws.grad, "layernorm_bwd dw")
        _close_rows(ref["db"], bs.grad, "layernorm_bwd db")
        if res:
            _close_rows(ref["dres"], rs.grad, "layernorm_bwd dres")


@pytest.mark.parametrize("act", [1, 2, 3])
def test_activation_stages_equal_fp64_autograd(act):
    inp = E.inputs_for("act", {1: "quick_gelu", 2: "gelu", 3: "silu"}[act])
    x, dy = inp["x"].to(F64), inp["dy"].to(F64)
    xs = x.clone().requires_grad_(True)
    y = _act64(xs, act)
    y.backward(dy)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(xs.grad).all())          # the formula survives the whole grid in fp64
    _close_el(E.act_fwd(x, act)[0]["y"], y.detach(), x.abs(), "act_fwd")      # 1 + erf cancels: absolute in |x|
    _close_el(E.act_bwd(x, dy, act)[0]["dx"], xs.grad, dy.abs(), "act_bwd")


@pytest.mark.parametrize("cid", [c["id"] for c in E.SWIGLU_CASES])
def test_swiglu_stages_equal_fp64_autograd(cid):
    inp = E.inputs_for("swiglu", cid)
    gu, d = inp["gu"].to(F64).requires_grad_(True), inp["dout"].to(F64)
    ff = gu.shape[1] // 2
    y = F.silu(gu[:, :ff]) * gu[:, ff:]
    y.backward(d)
    _close_el(E.swiglu_fwd(inp["gu"])[0]["y"], y.detach(), 0.0, "swiglu_fwd")
    _close_el(E.swiglu_bwd(inp["gu"], inp["dout"])[0]["dgu"], gu.grad, torch.cat([(d * gu[:, ff:]).abs(), d.abs()], 1).detach(), "swiglu_bwd")


@pytest.mark.parametrize("cid", [c["id"] for c in E.ROPE_CASES])
def test_rope_stage_is_a_complex_rotation(cid):
    c, inp = E.BY_ID[("rope", cid)], E.inputs_for("rope", cid)
    D, h, rows = c["D"], c["heads"], E.ROPE_B * E.ROPE_S
    ref, _ = E.rope(inp["x"], inp["cos"], inp["sin"], E.ROPE_S, h, D, c["sign"], pos=inp["pos"])
    x = inp["x"].to(F64)
    p = torch.tensor(E.ROPE_POS) if c["pos"] else torch.arange(rows) % E.ROPE_S
    rot = torch.complex(inp["cos"].to(F64), c["sign"] * inp["sin"].to(F64))[p][:, None, :]
    v = x[:, : h * D].reshape(rows, h, D)
    out = torch.complex(v[..., : D // 2], v[..., D // 2:]) * rot
    _close_el(ref["x"][:, : h * D], torch.cat([out.real, out.imag], -1).reshape(rows, h * D), 0.0, "rope")
    assert torch.equal(ref["x"][:, h * D:], x[:, h * D:])
    if c["pos"]:
        assert sum(int(a != r % E.ROPE_S) for r, a in enumerate(E.ROPE_POS)) >= 8 and len(set(E.ROPE_POS)) < rows
        assert any(a > b for a, b in zip(E.ROPE_POS, E.ROPE_POS[1:]))


def test_sum_stages_equal_torch():
    for c in E.COLSUM_CASES:
        x = E.inputs_for("colsum", c["id"])["x"]
        _close_el(E.colsum(x, c["dim"])[0]["out"], x.to(F64)[:, : c["dim"]].sum(0), 0.0, "colsum")
    for c in E.EMBED_CASES:
        inp = E.inputs_for("embed", c["id"])
        ref = E.embed_grad(inp["d"], inp["tok"], inp["beg"], inp["rows"], c["D"], E.EMBED_VOCAB)[0]["dE"]
        counts = (inp["beg"][1:] - inp["beg"][:-1]).long()
        exp = torch.zeros(E.EMBED_VOCAB, c["D"], dtype=F64).index_add_(0, torch.repeat_interleave(inp["tok"].long(), counts),
                                                                       inp["d"].to(F64)[inp["rows"].long(), : c["D"]])
        named = inp["tok"].long()
        _close_el(ref[named], exp[named], 0.0, "embed_grad")
        rest = [t for t in range(E.EMBED_VOCAB) if t not in named.tolist()]
        assert bool(torch.isnan(ref[rest]).all()) and sorted(counts.tolist()) == [1, 2, 3, 33]
        assert len(set(inp["rows"].tolist())) == int(counts.sum())
    for c in E.ADD_CASES:
        inp = E.inputs_for("add", c["id"])
        assert torch.equal(E.add(inp["a"], inp["b"])[0]["y"], inp["a"].double() + inp["b"].double())


# ---------------------------------------------------------------------------------------------------- cases and dispatch
def test_cases_name_every_rung_and_rows_per_block():
    seen = {op: set() for op in E.NORM_OPS}
    trips = {op: {} for op in E.NORM_OPS}
    for c in E.NORM_CASES:
        assert c["rows"] * c["dim"] <= 4200 * 64 and c["dim"] % 8 == 0
        for op, lit in c["expect"].items():
            assert E.paths(op, c["rows"], c["dim"]) == lit, (c["id"], op)
            seen[op].add(lit)
            trips[op].setdefault(lit[0], set()).add(c["dim"] % 512 == 0)
    assert {k for k, _ in seen["rmsnorm_fwd"]} == {"rmsnorm_fwd_cached_kernel<1>", "rmsnorm_fwd_cached_kernel<8>", "rmsnorm_fwd_kernel"}
    assert {k for k, _ in seen["rmsnorm_bwd"]} == {"rmsnorm_bwd_cached_kernel<1>", "rmsnorm_bwd_kernel"}
    assert {k for k, _ in seen["layernorm_fwd"]} == {"layernorm_fwd_cached_kernel<1>", "layernorm_fwd_cached_kernel<2>",
                                                    "layernorm_fwd_cached_kernel<8>", "layernorm_fwd_kernel"}
    for op, kern in (("rmsnorm_bwd_dw", "rmsnorm_dw_partial_kernel"), ("rmsnorm_bwd_full", "rmsnorm_dw_partial_kernel"),
                     ("layernorm_bwd", "layernorm_bwd_kernel")):
        assert {k for k, _ in seen[op]} == {f"{kern}<{ni}>" for ni in (1, 2, 4, 8)}
        assert {r for _, r in seen[op]} >= {4, 8}
    for op in E.NORM_OPS:                       # every rung with a full last trip and with one only some lanes take
        for kern, full in trips[op].items():
            assert full == {True, False}, (op, kern)
    assert {c["rows"] for c in E.NORM_CASES} >= {1, 4, 5, 37, 1030, 4101}
    for c in E.COLSUM_CASES:
        assert E.paths("colsum", c["rows"], c["dim"]) == c["expect"] and c["ld"] > c["dim"]
    assert {c["expect"][1] for c in E.COLSUM_CASES} == {4, 8}
    assert E.norm_rows_per_block(1030) == 8 and -(-1030 // 8) == 129 and 1030 - 128 * 8 == 6
    assert E.rms_full_rows_per_block(4101) == 8 and E.norm_rows_per_block(4101) == 20


def test_inputs_hold_the_rows_the_bars_are_for():
    inp = E.inputs_for("norm", "37x520")
    x, xl, w = inp["x"].double(), inp["xl"].double(), inp["w"].double()
    assert bool((x[1] == 0).all()) and bool((x[2] == x[2, 0]).all()) and float(x[2, 0]) != 0
    assert int((x[3] != 0).sum()) == 1 and float(x[3, -1]) != 0
    ms = (x * x).mean(-1)
    assert float(ms[ms > 0].min()) < 0.2 * E.EPS_RMS and float(ms.max()) > 1e4 * E.EPS_RMS        # eps dominates / is negligible
    r = xl.mean(-1).abs() / xl.std(-1, unbiased=False).clamp_min(1e-300)
    assert int(((r > 50) & (r < 80)).sum()) >= 8                                                  # mean = 64 x std
    assert float(r[6]) > 200 * 520 ** 0.5 and len(set(xl[6].tolist())) == 2                      # 100.5 s with one element an ulp up
    assert int((w == 0).sum()) == 1 and int((w < 0).sum()) >= 1
    g = E.act_grid().double()
    assert g.numel() % 8 == 0 and float(g.max()) == E.BF16_MAX and float(g.min()) == -E.BF16_MAX
    z = g[g == 0]
    assert set(torch.signbit(z).tolist()) == {True, False}


def test_paths_restate_the_launchers():
    """``paths`` is a restatement in Python; the library does not say which kernel it launched.  What can be held fast is
    the source: the branch conditions it copies are still the ones ops.hip and train.hip branch on."""
    csrc = pathlib.Path(__file__).resolve().parent.parent / "phantom_vlb_amd" / "csrc"
    ops, train = (re.sub(r"\s+", " ", (csrc / n).read_text()) for n in ("ops.hip", "train.hip"))
    for cond in ("if (dim <= 512) hipLaunchKernelGGL(rmsnorm_fwd_cached_kernel<1>, VLB_RN_ARGS); "
                 "else if (dim <= 4096) hipLaunchKernelGGL(rmsnorm_fwd_cached_kernel<8>, VLB_RN_ARGS); "
                 "else hipLaunchKernelGGL(rmsnorm_fwd_kernel, VLB_RN_ARGS);",
                 "if (dim <= 512) hipLaunchKernelGGL(rmsnorm_bwd_cached_kernel<1>, VLB_RB_ARGS); "
                 "else hipLaunchKernelGGL(rmsnorm_bwd_kernel, VLB_RB_ARGS);",
                 "if (dim <= 512) hipLaunchKernelGGL(layernorm_fwd_cached_kernel<1>, VLB_LN_ARGS); "
                 "else if (dim <= 1024) hipLaunchKernelGGL(layernorm_fwd_cached_kernel<2>, VLB_LN_ARGS); "
                 "else if (dim <= 4096) hipLaunchKernelGGL(layernorm_fwd_cached_kernel<8>, VLB_LN_ARGS); "
                 "else hipLaunchKernelGGL(layernorm_fwd_kernel, VLB_LN_ARGS);",
                 "dim3((rows + 3) / 4), dim3(256), 0, as_stream(stream)"):
        assert cond in ops, cond
    for cond in ("static inline int norm_rows_per_block(int rows) { int r = (rows + 255) / 256; return r < 4 ? 4 : (r + 3) / 4 * 4; }",
                 "static inline int rms_full_rows_per_block(int rows) { int r = (rows + 1023) / 1024; return r < 4 ? 4 : (r + 3) / 4 * 4; }",
                 "if (dim <= 512) VLB_RDW(1); else if (dim <= 1024) VLB_RDW(2); else if (dim <= 2048) VLB_RDW(4); else VLB_RDW(8);",
                 "if (dim <= 512) VLB_RBF(1); else if (dim <= 1024) VLB_RBF(2); else if (dim <= 2048) VLB_RBF(4); else VLB_RBF(8);",
                 "if (dim <= 512) VLB_LNB(1); else if (dim <= 1024) VLB_LNB(2); else if (dim <= 2048) VLB_LNB(4); else VLB_LNB(8);",
                 "const int rpb = rms_full_rows_per_block(rows), nb = (rows + rpb - 1) / rpb;",
                 "hipLaunchKernelGGL(colsum_partial_kernel, dim3((dim / 8 + 255) / 256, nb), dim3(256), 0, st, (const bf16*)x, ld, ws, rows, dim, rpb);"):
        assert cond in train, cond
    assert train.count("const int rpb = norm_rows_per_block(rows), nb = (rows + rpb - 1) / rpb;") == 3      # dw, layernorm_bwd, colsum
    assert train.count("dim % 8 == 0 && dim <= 4096") == 3                                                  # what FWD_ONLY_DIMS is about
    assert E.paths("rmsnorm_fwd", 3, 4096)[0] == "rmsnorm_fwd_cached_kernel<8>" and E.paths("rmsnorm_fwd", 3, 4104)[0] == "rmsnorm_fwd_kernel"
    assert E.paths("layernorm_bwd", 1030, 2056) == ("layernorm_bwd_kernel<8>", 8)


# ---------------------------------------------------------------------------------------------------- bars accept fp32
def _report(what, got, ref, bar):
    r, out = E.ratios(got, ref, bar), E.outside(got, ref, bar)
    print(what, {k: round(v, 3) for k, v in r.items()}, "outside:", out)
    assert all(v <= 1.0 for v in r.values()), (what, r)
    assert not any(out.values()), (what, out)


@pytest.mark.parametrize("op,cid", [(op, c["id"]) for op in E.NORM_OPS for c in E.norm_cases(op)])
def test_bars_accept_the_fp32_restatement_norms(op, cid):
    inp = E.inputs_for("norm", cid)
    for label, kw in E.norm_variants(op):
        ref, bar = E.norm_call(op, inp, kw)
        _report(f"{op} {cid} {label}", E.norm_call(op, inp, kw, emu=True), ref, bar)


def other_call(op, cid, emu=False, bug=None):
    """the operations that are not norms, on a named case: the fp64 stage (-> ref, bar) or the fp32 restatement"""
    extra = {} if emu else dict(bug=bug)
    if op == "rope":
        c, i = E.BY_ID[("rope", cid)], E.inputs_for("rope", cid)
        return (E.emu_rope if emu else E.rope)(i["x"], i["cos"], i["sin"], E.ROPE_S, c["heads"], c["D"], c["sign"], pos=i["pos"], **extra)
    if op in ("swiglu_fwd", "swiglu_bwd"):
        i = E.inputs_for("swiglu", cid)
        if op == "swiglu_fwd":
            return (E.emu_swiglu_fwd if emu else E.swiglu_fwd)(i["gu"], **extra)
        return (E.emu_swiglu_bwd if emu else E.swiglu_bwd)(i["gu"], i["dout"], **extra)
    if op in ("act_fwd", "act_bwd"):
        c, i = E.BY_ID[("act", cid)], E.inputs_for("act", cid)
        if op == "act_fwd":
            return (E.emu_act_fwd if emu else E.act_fwd)(i["x"], c["act"], **extra)
        return (E.emu_act_bwd if emu else E.act_bwd)(i["x"], i["dy"], c["act"], **extra)
    if op == "colsum":
        c = E.BY_ID[("colsum", cid)]
        return (E.emu_colsum if emu else E.colsum)(E.inputs_for("colsum", cid)["x"], c["dim"], **extra)
    if op == "embed_grad":
        c, i = E.BY_ID[("embed", cid)], E.inputs_for("embed", cid)
        return (E.emu_embed_grad if emu else E.embed_grad)(i["d"], i["tok"], i["beg"], i["rows"], c["D"], E.EMBED_VOCAB, **extra)
    if op == "add":
        i = E.inputs_for("add", cid)
        return (E.emu_add if emu else E.add)(i["a"], i["b"], **extra)
    raise KeyError(op)


OTHERS = ([("rope", c["id"]) for c in E.ROPE_CASES] + [(op, c["id"]) for op in ("swiglu_fwd", "swiglu_bwd") for c in E.SWIGLU_CASES]
          + [(op, c["id"]) for op in ("act_fwd", "act_bwd") for c in E.ACT_CASES] + [("colsum", c["id"]) for c in E.COLSUM_CASES]
          + [("embed_grad", c["id"]) for c in E.EMBED_CASES] + [("add", c["id"]) for c in E.ADD_CASES])


@pytest.mark.parametrize("op,cid", OTHERS)
def test_bars_accept_the_fp32_restatement_others(op, cid):
    ref, bar = other_call(op, cid)
    _report(f"{op} {cid}", other_call(op, cid, emu=True), ref, bar)


# ---------------------------------------------------------------------------------------------------- bars reject bugs
def test_every_planted_bug_is_listed():
    assert set(E.BUGS) == {"eps_outside", "eps_tenth", "onepass_var32", "drop_last8", "drop_block_last_row", "padded_width",
                           "rope_half_sign", "rope_pos_mod", "silu_grad_no_x", "res_after_act", "quick_grad_1"}


@pytest.mark.parametrize("bug,op,kw,cid", [(b, op, kw, cid) for b, sites in E.BUGS.items() for op, kw, cid in sites])
def test_bars_reject_planted_bug(bug, op, kw, cid):
    """the fp64 stage with the bug planted, rounded to bf16 as a device would write it, against the honest stage's bars"""
    if kw is None:
        (ref, bar), (bad, _) = other_call(op, cid), other_call(op, cid, bug=bug)
    else:
        inp = E.inputs_for("norm", cid)
        (ref, bar), (bad, _) = E.norm_call(op, inp, kw), E.norm_call(op, inp, kw, bug=bug)
    bad = {k: E.rbf(v) for k, v in bad.items()}
    r = E.ratios(bad, ref, bar)
    print(bug, op, cid, {k: round(v, 2) for k, v in r.items()}, "outside:", E.outside(bad, ref, bar))
    assert max(r.values()) > 1.0, (bug, op, cid, r)
