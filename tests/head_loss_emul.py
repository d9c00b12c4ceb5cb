"""fp64 restatement of the brain head's correlation objectives (``loss="cosine"`` / ``"pearson"``), one kernel at a time,
with derived bars, cases and planted bugs.  The companion of tests/head_emul.py (imported as ``H``: the staged fp64 head,
its inputs and its bar constants), for the kernels head.hip adds:

  rowstat      head_rowstat_kernel        pred, y -> mu_p, mu_y, sum u^2, sum t^2, sum u t, c_b      (BrainHead.rowstat)
  loss         loss_finalize_corr_kernel  c_b, the ridge forward's partials -> loss_terms, loss_aux
  ridge_bwd_w  ridge_bwd_w_kernel<true>   d pred from (rowstat, loss_scale) -> dW, dbias   (head_loss_coef_kernel rides along)
  dz           dpred_t_kernel<true> + skinny wgrad + head_dz_from16, or ridge_bwd_z_kernel<true> + head_dz_reduce

Per clip:  u = p - mu_p, t = y - mu_y (mu = 0 for cosine), nu = max(|u|, 1e-8), nt = max(|t|, 1e-8), c = <u,t>/(nu nt),
data term = 1 - mean_b c_b;  d pred = a u + b t,  b = -s/(B nu nt),  a = s c/(B nu |u|) (0 where |u| = 0): s c/(B nu^2)
wherever the norm is not clamped, and under the clamp what fp64 autograd through F.cosine_similarity gives (it clamps the
norm's value under no_grad and differentiates the norm itself).

Bars follow head_emul's rule, c * 2^-24 * sum|terms| + 2^-22 * |ref|, c read from the kernels' addition chains:

  rowstat.  A thread adds at most one head element, 4 per f32x4 over ceil(nvec/1024) <= ceil(V/4096) vectors and one tail
    element into one accumulator; block_sum adds 6 wave levels and 16 wave partials:  C_RS = 4*ceil(V/4096) + 2 + 6 + 16 + 2.
    The centred sums are judged with the DEVICE's own means (as head_emul judges pooled_raw with the device's own stats):
    u = p - mu is then one rounding, u*u or u*t two more -> C_RS + 3.  c_b is judged from the device's own three sums:
    two sqrtf, the clamp, a product and a division, all correctly rounded -> 8 * 2^-24 relative.
  loss.  The sum over clips runs in double; 1 - mean is rounded once to fp32 -> 2 * 2^-24 on 1 + |mean c| (the terms of
    the difference).  loss_terms[1] is asked bit-equal to what the plain forward wrote; aux[0] gets head_emul's MSE bar.
  d pred.  The coefficients go through sqrtf, the clamp, nu*|u|, s/B, a product and a division (6 roundings each), the
    centred operand through one subtraction, then a product and the final addition:  C_DP = 9 on |a u| + |b t|, the two
    terms d pred is the (cancelling) sum of - never on |d pred| itself.
  ridge_bwd_w.  head_emul's chain with C_DP in place of the 2 roundings of gscale*(pred - y).
  dz.  B > 16: head_emul's chain with C_DP.  B <= 16: d pred is rounded to bf16 for the MFMA; its fp32 value is not
    reproduced bit for bit here (a*u + b*t may or may not be contracted into an fma), so the reference keeps d pred
    unrounded and the bar carries half a bf16 ulp of every d pred, 2^-8 * (|d pred| @ |W|), head_emul's rule for bf16 values.

Nothing is fitted to a measurement.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import head_emul as H

F64, F32, BF16 = H.F64, H.F32, H.BF16
U, R, HB = H.U, H.R, H.HB
CLAMP = 1e-8
LOSSES = ("cosine", "pearson")
C_DP = 9
STAGES = ("rowstat", "loss", "ridge_bwd_w", "dz")
REST = ("pool", "ln2", "ridge", "ln2_bwd", "dhidden")         # head_emul's stages the objective does not change


# ---------------------------------------------------------------------------------------------------- cases
# Re-drawn cases (head_emul.RESEED's rule): (case id, loss) -> the first draw whose bf16 roundings alone stay within
# E2E_FORMAT_SHARE of every end-to-end bar; test_cpu_head_loss asserts that and that no earlier draw does.
RESEED = {("loss-B16", "cosine"): 1, ("loss-V2", "cosine"): 3, ("loss-packed", "cosine"): 1, ("loss-packed", "pearson"): 1,
          ("loss-offset50", "cosine"): 1}


def _case(id, E, S, B, V, losses=LOSSES, zero_target=False, offset=0.0, **kw):
    c = H._case(id, E, S, B, V, **kw)
    c.update(losses=tuple(losses), zero_target=zero_target, offset=offset)
    return c


_SK, _BIG = H._SKINNY, H._BIG
CASES = []
# clip counts: both dz routes, one to three b0 passes of ridge_bwd_w_kernel; E = 1024 (MFMA ridge forward), V = 17 (rows of
# pred start 1, 2, 3 elements off a 16-byte boundary)
for _B, _passes, _path in ((1, 1, _SK), (3, 1, _SK), (8, 1, _SK), (9, 2, _SK), (16, 2, _SK), (17, 3, _BIG)):
    CASES.append(_case(f"loss-B{_B}", 1024, 33, _B, 17, expect=(f"ridge_bwd_w:b0_passes={_passes}",) + _path))
# scalar ridge forward (E = 264), both dz routes
CASES.append(_case("loss-E264", 264, 33, 3, 17, expect=("ridge_fwd_kernel",) + _SK))
CASES.append(_case("loss-E264-B17-V300", 264, 33, 17, 300, expect=_BIG))
# target counts
CASES.append(_case("loss-V1", 1024, 33, 3, 1, losses=("cosine",), expect=_SK))
CASES.append(_case("loss-V2", 1024, 33, 3, 2, expect=_SK))
CASES.append(_case("loss-V2-B17", 1024, 33, 17, 2, expect=_BIG))
CASES.append(_case("loss-V300", 1024, 33, 3, 300, expect=_SK))
CASES.append(_case("loss-V32784", 264, 33, 2, 32784, expect=("ridge_fwd_kernel",) + _SK))
# dropout and both scales != 1, on either dz route
CASES.append(_case("loss-scales", 1024, 33, 9, 17, drop=True, scales=(0.25, 0.5), expect=("ridge_bwd_w:b0_passes=2",) + _SK))
CASES.append(_case("loss-scales-B17", 1024, 33, 17, 17, drop=True, scales=(0.25, 0.5), expect=_BIG))
CASES.append(_case("loss-packed", 1024, 70, 3, 17, lens=(70, 1, 37), expect=_SK))
CASES.append(_case("loss-zero-target", 1024, 33, 3, 17, zero_target=True, expect=_SK))
# predictions and targets on a common offset of 50 with unit spread: what a one-pass or uncentred implementation fails
CASES.append(_case("loss-offset50", 1024, 33, 3, 300, offset=50.0, expect=_SK))
BY_ID = {c["id"]: c for c in CASES}
PAIRS = [(c["id"], k) for c in CASES for k in c["losses"]]


def make_inputs(case, loss, reseed=None):
    n = RESEED.get((case["id"], loss), 0) if reseed is None else reseed
    inp = H.make_inputs(dict(case, reseed=n))
    inp["loss"] = loss
    if case["zero_target"]:
        inp["y"][1] = 0
    if case["offset"]:
        p = inp["params"]
        p["ridge_layer.linear.bias"] = (p["ridge_layer.linear.bias"] + case["offset"]).to(BF16).float()
        inp["y"] = inp["y"] + case["offset"]
    return inp


@functools.lru_cache(maxsize=None)
def inputs_for(case_id, loss):
    """the inputs of a named case, made once and shared (treat as read-only)"""
    return make_inputs(BY_ID[case_id], loss)


# ---------------------------------------------------------------------------------------------------- the objective
BUGS = {"no_centre": "rowstat", "centre_p_only": "rowstat", "unclamped": "rowstat", "no_inv_b": "loss",
        "no_inv_b_grad": "ridge_bwd_w", "drop_a": "ridge_bwd_w", "sign_b": "ridge_bwd_w", "scale_twice": "ridge_bwd_w"}
DZ_BUGS = ("drop_a", "sign_b", "scale_twice", "no_inv_b_grad")      # the same bugs seen by the dz stage


def rowstat(pred, y, loss, mu=None, dt=F64, bug=None):
    """head_rowstat_kernel.  -> mu_p, mu_y, suu, stt, sut, c [B].  ``mu`` = (mu_p, mu_y) to centre with (the device's own)."""
    p, yy = pred.to(dt), y.to(dt)
    V = p.shape[1]
    zero = torch.zeros(p.shape[0], dtype=dt)
    centre = loss == "pearson" and bug != "no_centre"
    mu_p = p.sum(1) / V if centre else zero
    mu_y = yy.sum(1) / V if centre and bug != "centre_p_only" else zero
    mp, my = (mu_p, mu_y) if mu is None else (mu[0].to(dt), mu[1].to(dt))
    u, t = p - mp[:, None], yy - my[:, None]
    suu, stt, sut = (u * u).sum(1), (t * t).sum(1), (u * t).sum(1)
    out = dict(mu_p=mu_p, mu_y=mu_y, suu=suu, stt=stt, sut=sut, mag_p=p.abs().sum(1) / V, mag_y=yy.abs().sum(1) / V,
               mag_ut=(u * t).abs().sum(1))
    out["c"] = corr_from_sums(suu, stt, sut, bug=bug)
    return out


def corr_from_sums(suu, stt, sut, bug=None):
    if bug == "unclamped":
        return sut / (suu.sqrt() * stt.sqrt())
    return sut / (suu.sqrt().clamp_min(CLAMP) * stt.sqrt().clamp_min(CLAMP))


def rowstat_chain(V):
    return 4 * H.cdiv(V, 4096) + 2 + 6 + 16 + 2


def rowstat_bars(ref, V):
    c = rowstat_chain(V)
    return dict(mu_p=c * U * ref["mag_p"] + R * ref["mu_p"].abs(), mu_y=c * U * ref["mag_y"] + R * ref["mu_y"].abs(),
                suu=((c + 3) * U + R) * ref["suu"], stt=((c + 3) * U + R) * ref["stt"],
                sut=(c + 3) * U * ref["mag_ut"] + R * ref["sut"].abs())


def coefficients(suu, stt, c, B, loss_scale, bug=None):
    """head_loss_coef_kernel -> a_b, b_b"""
    ru = suu.sqrt()
    nu, nt = ru.clamp_min(CLAMP), stt.sqrt().clamp_min(CLAMP)
    s = loss_scale * loss_scale if bug == "scale_twice" else loss_scale
    sb = s if bug == "no_inv_b_grad" else s / B
    a = torch.where(ru > 0, sb * c / (nu * ru).clamp_min(1e-300), torch.zeros_like(c))
    b = -sb / (nu * nt)
    if bug == "drop_a":
        a = torch.zeros_like(a)
    if bug == "sign_b":
        b = -b
    return a, b


def dpred(pred, y, rs, loss_scale, dt=F64, bug=None):
    """d pred [B,V] from row statistics ``rs`` (mu_p, mu_y, suu, stt, c), and |a u| + |b t|, the magnitude its error scales with"""
    p, yy = pred.to(dt), y.to(dt)
    a, b = coefficients(rs["suu"].to(dt), rs["stt"].to(dt), rs["c"].to(dt), p.shape[0], loss_scale, bug=bug)
    u, t = p - rs["mu_p"].to(dt)[:, None], yy - rs["mu_y"].to(dt)[:, None]
    au, bt = a[:, None] * u, b[:, None] * t
    return au + bt, au.abs() + bt.abs()


def objective(pred, y, loss, loss_scale=1.0, dt=F64):
    """-> (data term 1 - mean_b c_b, d(loss_scale * data term)/d pred): the closed form the kernels implement"""
    rs = rowstat(pred, y, loss, dt=dt)
    dp, _ = dpred(pred, y, rs, loss_scale, dt=dt)
    return 1 - rs["c"].sum() / pred.shape[0], dp


def loss_terms(c, l2, mse, bug=None):
    """loss_finalize_corr_kernel: c [B] (the device's own), l2 and mse from head_emul.ridge"""
    B = c.numel()
    mean = c.to(F64).sum() / (1 if bug == "no_inv_b" else B)
    data = 1 - mean
    return dict(loss=torch.stack([data, l2, data + l2]), aux=torch.stack([mse, mean]), mean=mean)


def loss_bars(ref, ridge_bar):
    """``ridge_bar``: head_emul.ridge_bars(...)["loss"] = bars of (mse, l2, .)"""
    bar_d = 2 * U * (1 + ref["mean"].abs()) + R * ref["loss"][0].abs()
    return dict(loss=torch.stack([bar_d, ridge_bar[1], bar_d + ridge_bar[1] + R * ref["loss"][2].abs()]),
                aux=torch.stack([ridge_bar[0], 2 * U * ref["mean"].abs() + R * ref["mean"].abs()]))


def ridge_bwd_w(dp, mag_dp, z, W, l2coef, dt=F64):
    z, W = z.to(dt), W.to(dt)
    seed = l2coef * W
    return dict(dW=seed + dp.t() @ z, dbias=dp.sum(0), mag_dW=seed.abs() + mag_dp.t() @ z.abs(), mag_dbias=mag_dp.sum(0))


def ridge_bwd_w_bars(ref, B):
    c_dW = B + 1 + 2 + C_DP
    c_db = B + H.cdiv(B, 8) + 2 + C_DP
    return dict(dW=c_dW * U * ref["mag_dW"] + R * ref["dW"].abs(), dbias=c_db * U * ref["mag_dbias"] + R * ref["dbias"].abs())


def dz(dp, mag_dp, W, keep, dt=F64):
    W = W.to(dt)
    k = torch.ones(dp.shape[0], W.shape[1], dtype=dt) if keep is None else keep.to(dt)
    return dict(dz=(dp @ W) * k, mag=(mag_dp @ W.abs()) * k, mag_round=(dp.abs() @ W.abs()) * k)


def dz_bars(ref, B, V):
    if B <= 16:
        sp = H.wgrad_splits(V)
        c = H.cdiv(V, sp) + sp + 2 + 1
        # d pred's own fp32 error (C_DP on |a u| + |b t|) and its rounding to bf16 (half an ulp of every d pred)
        return dict(dz=(c * U * ref["mag_round"] + C_DP * U * ref["mag"] + HB * ref["mag_round"]) + R * ref["dz"].abs())
    c = H.cdiv(H.cdiv(V, 32), 4) + 3 + 32 + 2 + 1 + C_DP
    return dict(dz=c * U * ref["mag"] + R * ref["dz"].abs())


# ---------------------------------------------------------------------------------------------------- the chain
def run(inp, dt=F64, device_like=False, bug=None):
    """head_emul.run with the correlation objective in place of the MSE: every buffer ``BrainHead`` holds after a forward
    and a backward, plus rowstat's columns and loss_aux.  dt / device_like as there."""
    loss, p, B, V = inp["loss"], inp["params"], inp["case"]["B"], inp["case"]["V"]
    W, g1, g2 = p["ridge_layer.linear.weight"], p["layer_norm1.weight"], p["layer_norm2.weight"]
    po = H.pool(inp["hidden"], inp["wmask"], inp["eps"], dt=dt)
    l2o = H.ln2(po["pooled_raw"], po["sumw"], g1, p["layer_norm1.bias"], g2, p["layer_norm2.bias"], inp["keep"], inp["eps"], dt=dt)
    z = l2o["z"].to(BF16).to(dt) if device_like else l2o["z"]
    lam = float(np.float32(inp["lam"])) if device_like else inp["lam"]
    ro = H.ridge(z, W, p["ridge_layer.linear.bias"], inp["y"], lam, dt=dt)
    rs = rowstat(ro["pred"], inp["y"], loss, dt=dt, bug=bug)
    lo = loss_terms(rs["c"], ro["loss"][1].to(F64), ro["loss"][0].to(F64), bug=bug)
    if device_like:
        l2coef, s = H.host_scales(B, V, inp["lam"], inp["loss_scale"], inp["l2_scale"])[1], float(np.float32(inp["loss_scale"]))
    else:
        l2coef, s = inp["l2_scale"] * 2.0 * inp["lam"], inp["loss_scale"]
    dp, mag = dpred(ro["pred"], inp["y"], rs, s, dt=dt, bug=bug)
    wo = ridge_bwd_w(dp, mag, z, W, l2coef, dt=dt)
    dpz = dp.to(BF16).to(dt) if device_like and B <= 16 else dp
    do = dz(dpz, mag, W, inp["keep"], dt=dt)
    bo = H.ln2_bwd(do["dz"], g2, l2o["zhat"], l2o["ln2_rstd"], g1, po["pooled_raw"], po["sumw"], dt=dt)
    ho = H.dhidden(inp["hidden"], inp["wmask"], po["mu"], po["rstd"], bo["dpooled"], dt=dt)
    dh = ho["dh"].to(BF16).to(dt) if device_like else ho["dh"]
    out = dict(mu=po["mu"], rstd=po["rstd"], pooled_raw=po["pooled_raw"], sumw=po["sumw"], zhat=l2o["zhat"],
               ln2_rstd=l2o["ln2_rstd"], z=z, pred=ro["pred"], loss_terms=lo["loss"].to(dt), loss_aux=lo["aux"].to(dt),
               dW=wo["dW"], dbias=wo["dbias"], dz=do["dz"], dpooled=bo["dpooled"], dg2=bo["dg2"], db2=bo["db2"], dg1=bo["dg1"],
               db1=bo["db1"], dh=dh)
    out.update({k: rs[k].to(dt) for k in ("mu_p", "mu_y", "suu", "stt", "sut", "c")})
    return out


def whole(inp):
    """the head with this objective as mathematics: fp64, nothing rounded"""
    return run(inp, dt=F64, device_like=False)


def rowstat_columns(rowstat_buf):
    """BrainHead.rowstat [B,8] -> the named columns ``run`` returns"""
    return {k: rowstat_buf[:, i].contiguous() for i, k in enumerate(("mu_p", "mu_y", "suu", "stt", "sut", "c"))}


# ---------------------------------------------------------------------------------------------------- the check
def check_stages(bufs, inp, stages=STAGES):
    """Each new kernel's outputs in ``bufs`` (named as in ``run``) against its fp64 restatement fed with bufs' own upstream
    buffers.  -> {"stage.output": max(err / bar)}"""
    c, p, loss = inp["case"], inp["params"], inp["loss"]
    B, E, V = c["B"], c["E"], c["V"]
    W = p["ridge_layer.linear.weight"]
    l2coef, s = H.host_scales(B, V, inp["lam"], inp["loss_scale"], inp["l2_scale"])[1], float(np.float32(inp["loss_scale"]))
    out = {}
    if "rowstat" in stages:
        ref = rowstat(bufs["pred"], inp["y"], loss)                                           # the means: from pred and y
        bars = rowstat_bars(ref, V)
        for n in ("mu_p", "mu_y"):
            out[f"rowstat.{n}"] = H.ratio(bufs[n], ref[n], bars[n])
        ref = rowstat(bufs["pred"], inp["y"], loss, mu=(bufs["mu_p"], bufs["mu_y"]))           # the sums: with the device's means
        bars = rowstat_bars(ref, V)
        for n in ("suu", "stt", "sut"):
            out[f"rowstat.{n}"] = H.ratio(bufs[n], ref[n], bars[n])
        cref = corr_from_sums(bufs["suu"].to(F64), bufs["stt"].to(F64), bufs["sut"].to(F64))  # c: from the device's sums
        out["rowstat.c"] = H.ratio(bufs["c"], cref, 8 * U * cref.abs())
    if "loss" in stages:
        rr = H.ridge(bufs["z"], W, p["ridge_layer.linear.bias"], inp["y"], float(np.float32(inp["lam"])), pred_for_loss=bufs["pred"])
        ref = loss_terms(bufs["c"], rr["loss"][1], rr["loss"][0])
        bars = loss_bars(ref, H.ridge_bars(rr, B, E, V)["loss"])
        out["loss.loss_terms"] = H.ratio(bufs["loss_terms"], ref["loss"], bars["loss"])
        out["loss.loss_aux"] = H.ratio(bufs["loss_aux"], ref["aux"], bars["aux"])
    if "ridge_bwd_w" in stages or "dz" in stages:
        dp, mag = dpred(bufs["pred"], inp["y"], bufs, s)
    if "ridge_bwd_w" in stages:
        ref = ridge_bwd_w(dp, mag, bufs["z"], W, l2coef)
        bars = ridge_bwd_w_bars(ref, B)
        for n in ("dW", "dbias"):
            out[f"ridge_bwd_w.{n}"] = H.ratio(bufs[n], ref[n], bars[n])
    if "dz" in stages:
        ref = dz(dp, mag, W, inp["keep"])
        out["dz.dz"] = H.ratio(bufs["dz"], ref["dz"], dz_bars(ref, B, V)["dz"])
    return out


def check_rest(bufs, inp):
    """head_emul's own checks of the stages the objective leaves alone; its ridge stage is shown the MSE the device kept
    in loss_aux[0] in the place of loss_terms[0]"""
    mse, l2 = bufs["loss_aux"][0].to(F32), bufs["loss_terms"][1].to(F32)
    return H.check_stages(dict(bufs, loss_terms=torch.stack([mse, l2, mse + l2])), inp, REST)


def flat(inp):
    """True where the data term does not depend on the prediction at all: the cosine of two numbers (V = 1) and the Pearson
    correlation of two points (V = 2) are +-1 whatever the numbers.  d pred is then zero as mathematics (the kernels' a u
    and b t cancel to rounding), so is every gradient but the l2 term's, and an error RELATIVE to such a gradient says
    nothing: those cases are held to the end-to-end bars on pred, the loss and dW (the l2 gradient) only.  The stage checks,
    whose bars scale with |a u| + |b t|, apply to them in full."""
    return (inp["loss"], inp["case"]["V"]) in (("cosine", 1), ("pearson", 2))


def _e2e(bufs, inp):
    out = H._e2e_errors(bufs, whole(inp))
    return {k: v for k, v in out.items() if k in ("pred", "l2", "total", "dW")} if flat(inp) else out


def end_to_end(bufs, inp):
    """-> {name: max|got - ref| / max|ref|} against ``whole(inp)``, each held to head_emul.E2E_BARS"""
    return _e2e(bufs, inp)


def format_deviation(inp):
    """the same figures for fp64 arithmetic with only the bf16 roundings (and fp32 scales) of the device"""
    return _e2e(run(inp, dt=F64, device_like=True), inp)
