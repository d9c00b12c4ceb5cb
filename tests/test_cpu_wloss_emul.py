"""Per-target loss weights and masks of the brain head on the CPU: the fp64 restatement of tests/wloss_emul.py is the
Definition (fp64 torch autograd), it has the properties the feature promises (a 0/1 mask is the objective on the kept
columns, unit weights are the unweighted objective, scale invariance, exact zeros and no arithmetic at masked targets),
its bars accept an honest fp32 computation at every shape the GPU tests use and reject every planted bug, and the number
formats leave room under the end-to-end bars."""
import pytest
import torch
import torch.nn.functional as F

import head_emul as H
import head_loss_emul as L
import wloss_emul as W

F64 = torch.float64


# ---------------------------------------------------------------------------------------------------- against autograd
def _definition(p, y, w, loss, loss_scale):
    """the Definition through fp64 autograd.  cosine / pearson: c_b is F.cosine_similarity of sqrt(w) u and sqrt(w) t, which
    carries the clamp and autograd's convention under it"""
    p = p.clone().requires_grad_(True)
    keep = w > 0
    ys = torch.where(keep, y, torch.zeros((), dtype=F64))
    Wb = w.sum(1, keepdim=True)
    if loss == "mse":
        val = ((w * (p - ys) ** 2).sum(1, keepdim=True) / Wb).mean()
    else:
        mu_p, mu_y = ((w * p).sum(1, keepdim=True) / Wb, (w * ys).sum(1, keepdim=True) / Wb) if loss == "pearson" else (0.0, 0.0)
        sw = w.sqrt()
        val = 1 - F.cosine_similarity(sw * (p - mu_p), sw * (ys - mu_y), dim=-1).mean()
    (loss_scale * val).backward()
    return val.detach(), p.grad


def _draw(B, V, seed, kind="plain"):
    gen = torch.Generator().manual_seed(seed)
    p, y = torch.randn(B, V, generator=gen, dtype=F64), torch.randn(B, V, generator=gen, dtype=F64)
    w = torch.stack([W.make_weights(V, seed + b) for b in range(B)]).double()
    if kind == "offset":
        p, y = p + 50, y + 50
    if kind == "zero_target":
        y[0] = 0
    return p, y, w


def _objective(p, y, w, loss, scale=1.0):
    rs = W.rowstat(p, y, w, loss)
    lo = W.loss_terms(rs["m"], rs["c"], torch.zeros((), dtype=F64), loss)
    return lo["loss"][0], W.dpred(p, y, w, rs, loss, scale)[0]


@pytest.mark.parametrize("loss", W.LOSSES)
@pytest.mark.parametrize("kind,V,scale", [("plain", 7, 1.0), ("plain", 300, 0.125), ("offset", 33, 1.0), ("zero_target", 7, 0.5),
                                          ("plain", 2, 0.25)])
def test_emulation_equals_fp64_autograd_of_the_definition(loss, kind, V, scale):
    p, y, w = _draw(3, V, 11 + V, kind)
    val, dp = _objective(p, y, w, loss, scale)
    ref_val, ref_dp = _definition(p, y, w, loss, scale)
    assert torch.isfinite(dp).all() and torch.isfinite(val)
    assert abs(float(val - ref_val)) <= 1e-12, float(val - ref_val)
    assert float((dp - ref_dp).abs().max()) <= 1e-12 * max(1.0, float(ref_dp.abs().max()))


# ---------------------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize("loss", W.LOSSES)
def test_a_mask_is_the_objective_on_the_kept_columns(loss):
    p, y, w = _draw(4, 37, 5)
    w = (w > 0.9).double()
    w[:, :2] = 1
    val, dp = _objective(p, y, w, loss)
    for b in range(4):                       # each clip keeps its own columns here; the reference takes them one clip at a time
        keep = w[b] > 0
        pk, yk = p[b:b + 1, keep].clone().requires_grad_(True), y[b:b + 1, keep]
        if loss == "mse":
            ref = F.mse_loss(pk, yk)
        elif loss == "cosine":
            ref = 1 - F.cosine_similarity(pk, yk, dim=-1).mean()
        else:
            ref = 1 - F.cosine_similarity(pk - pk.mean(-1, keepdim=True), yk - yk.mean(-1, keepdim=True), dim=-1).mean()
        (ref / 4).backward()
        rs = W.rowstat(p[b:b + 1], y[b:b + 1], w[b:b + 1], loss)
        got = rs["m"][0] if loss == "mse" else 1 - rs["c"][0]
        assert abs(float(got - ref.detach())) <= 1e-12
        assert float((dp[b, keep] - pk.grad[0]).abs().max()) <= 1e-12 and bool((dp[b, ~keep] == 0).all())
    assert torch.isfinite(val)


@pytest.mark.parametrize("loss", W.LOSSES)
def test_unit_weights_are_the_unweighted_objective(loss):
    p, y, _ = _draw(3, 33, 9)
    w = torch.ones(3, 33, dtype=F64)
    val, dp = _objective(p, y, w, loss, 0.5)
    if loss == "mse":                        # head_emul's: mean over B*V, d pred = gscale (pred - y)
        ref_val, ref_dp = ((p - y) ** 2).mean(), 0.5 * 2.0 / (3 * 33) * (p - y)
    else:
        ref_val, ref_dp = L.objective(p, y, loss, loss_scale=0.5)
    assert abs(float(val - ref_val)) <= 1e-13 and float((dp - ref_dp).abs().max()) <= 1e-13


@pytest.mark.parametrize("loss", W.LOSSES)
def test_scaling_the_weights_changes_nothing(loss):
    p, y, w = _draw(3, 33, 21)
    val, dp = _objective(p, y, w, loss)
    val4, dp4 = _objective(p, y, 4.0 * w, loss)         # a power of two: not one bit
    assert torch.equal(val, val4) and torch.equal(dp, dp4)
    val3, dp3 = _objective(p, y, 3.7 * w, loss)
    assert abs(float(val - val3)) <= 1e-13 and float((dp - dp3).abs().max()) <= 1e-13


@pytest.mark.parametrize("loss", W.LOSSES)
def test_masked_targets_enter_no_arithmetic(loss):
    p, y, w = _draw(3, 33, 31)
    out = []
    for fill in (0.0, float("nan"), float("inf")):
        yy = torch.where(w > 0, y, torch.full((), fill, dtype=F64))
        out.append(_objective(p, yy, w, loss))
    for val, dp in out[1:]:
        assert torch.equal(val, out[0][0]) and torch.equal(dp, out[0][1])
    assert bool((out[0][1][w == 0] == 0).all()) and bool(torch.isfinite(out[0][1]).all())


# ---------------------------------------------------------------------------------------------------- cases
def test_cases_cover_the_issue():
    ids = [c["id"] for c in W.CASES]
    assert len(set(ids)) == len(ids) and not set(ids) & (set(H.BY_ID) | set(L.BY_ID))
    for c in W.CASES:
        assert set(c["expect"]) <= H.dispatch(c["B"], c["E"]), c["id"]
        assert "pearson" not in c["losses"] or c["V"] >= 2
    assert {c["V"] for c in W.CASES} >= {1, 2, 5, 17, 300, 1030} and {c["B"] for c in W.CASES} >= {1, 8, 9, 17}
    assert {c["E"] for c in W.CASES} == {128, 264} and any(c["lens"] for c in W.CASES)
    assert any(c["S"] == 33 and c["zero_clip"] for c in W.CASES)
    reached = set().union(*(H.dispatch(c["B"], c["E"]) for c in W.CASES))
    assert {"ridge_fwd_kernel", "ridge_fwd_mfma_kernel<1>", "ridge_bwd_z_kernel", "wgrad_mfma_kernel", "ridge_bwd_w:b0_passes=1",
            "ridge_bwd_w:b0_passes=2"} <= reached
    g3 = [c for c in W.CASES if c["G"] == 3]
    assert {c["B"] <= 16 for c in g3} == {True, False}
    for c in g3:
        assert set(c["group"]) == {0, 2} and len(c["group"]) == c["B"]              # head 1 is absent
        tw = W.inputs_for(c["id"], "mse")["tw"]
        assert tw.shape == (3, c["V"]) and not torch.equal(tw[0], tw[2])
    tw = W.inputs_for("w-V17", "mse")["tw"][0]
    assert {int(i) % 4 for i in torch.nonzero(tw == 0).flatten()} == {0, 1, 2, 3}   # a zero at each alignment position
    assert bool((tw == 1).any()) and bool(((tw != 0) & (tw != 1) & (tw != tw.round())).any())
    for cid, loss in W.PAIRS:
        assert int((W.inputs_for(cid, loss)["tw"] > 0).sum(1).min()) >= (2 if loss == "pearson" else 1)


# ---------------------------------------------------------------------------------------------------- bars accept fp32
@pytest.mark.parametrize("cid,loss", W.PAIRS)
def test_bars_accept_an_honest_fp32_computation(cid, loss):
    """every stage in plain fp32 torch (torch's summation order, not the kernels'), chained as on the device, stays
    within its bar when judged the way the GPU test judges the kernels"""
    inp = W.inputs_for(cid, loss)
    bufs = W.run(inp, dt=H.F32, device_like=True)
    ratios = {**W.check_stages(bufs, inp), **W.check_rest(bufs, inp)}
    print(cid, loss, {k: round(v, 3) for k, v in H.by_stage(ratios).items()})
    assert all(v <= 1.0 for v in ratios.values()), {k: v for k, v in ratios.items() if not v <= 1.0}
    e2e = W.end_to_end(bufs, inp)
    assert all(v < H.E2E_BARS[k] for k, v in e2e.items()), e2e


@pytest.mark.parametrize("cid,loss", W.PAIRS)
def test_number_formats_leave_room_under_the_end_to_end_bars(cid, loss):
    dev = W.format_deviation(W.inputs_for(cid, loss))
    print(cid, loss, {k: f"{v:.1e}" for k, v in dev.items()})
    assert all(v <= H.E2E_FORMAT_SHARE * H.E2E_BARS[k] for k, v in dev.items()), dev
    for n in range(W.RESEED.get((cid, loss), 0)):
        dev = W.format_deviation(W.make_inputs(W.BY_ID[cid], loss, reseed=n))
        assert any(v > H.E2E_FORMAT_SHARE * H.E2E_BARS[k] for k, v in dev.items()), (cid, loss, n)


# ---------------------------------------------------------------------------------------------------- bars reject bugs
BUG_CASES = {
    "dpred_no_w": (("w-V17", "mse"), ("w-V300", "cosine"), ("w-G3", "pearson"), ("w-V1030", "pearson")),
    "div_by_V": (("w-V17", "mse"), ("w-V300", "mse"), ("w-G3-B17", "mse")),
    "unweighted_means": (("w-V17", "pearson"), ("w-V300", "pearson"), ("w-V1030", "pearson")),
    "wrong_head": (("w-G3", "mse"), ("w-G3", "cosine"), ("w-G3-B17", "pearson")),
    "mul_zero": (("w-V17", "mse"), ("w-V5", "cosine"), ("w-G3", "pearson")),
    "drop_tail": (("w-V17", "mse"), ("w-V1030", "cosine"), ("w-V5", "pearson")),
}


def test_every_planted_bug_has_cases():
    assert set(BUG_CASES) == set(W.BUGS)


def nan_targets(inp):
    """inp["y"] with NaN wherever the clip's head gives the target weight 0"""
    return torch.where(W.clip_weights(inp) > 0, inp["y"], torch.full((), float("nan")))


@pytest.mark.parametrize("bug,cid,loss", [(b, c, k) for b, cs in BUG_CASES.items() for c, k in cs])
def test_bars_reject_planted_bug(bug, cid, loss):
    inp = W.inputs_for(cid, loss)
    y = nan_targets(inp) if bug == "mul_zero" else None
    if y is not None:                        # the select keeps every figure finite and inside the bars ...
        clean = W.check_stages(W.run(inp, dt=H.F32, device_like=True, y=y), inp, y=y)
        assert all(v <= 1.0 for v in clean.values()), clean
    bufs = W.run(inp, dt=H.F32, device_like=True, bug=bug, y=y)
    worst = H.by_stage(W.check_stages(bufs, inp, (W.BUGS[bug],), y=y))
    print(bug, cid, loss, worst)
    assert worst[W.BUGS[bug]] > 1.0, (bug, cid, loss, worst)
