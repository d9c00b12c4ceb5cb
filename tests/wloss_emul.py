"""fp64 restatement of the brain head's per-target loss weights and masks (``BrainHead.set_target_weights``, DESIGN
§5.3.8), one new kernel at a time, with derived bars, cases and planted bugs.  The companion of tests/head_emul.py (``H``:
the staged fp64 head, its inputs and bar constants) and tests/head_loss_emul.py (``L``: the unweighted correlation
objectives), for the stages head.hip adds:

  rowstat   head_wrowstat_kernel    pred, y, tw[group[b]] -> wstat = {mu_p, mu_y, S_uu, S_tt, S_ut, c_b, W_b, m_b}
  loss      wloss_finalize_kernel   wstat, the ridge forward's sum W^2 partials -> loss_terms, loss_aux
  dpred     head_wdpred_kernel      wstat, pred, y, tw, loss_scale -> d pred [B,V]
  ridge_bwd_w, dz                   the DP_BUF forms of ridge_bwd_w_kernel and of the two dz routes: d pred is read, not derived

Definition, clip b of head g = group[b], w_v = tw[g,v], W_b = sum w:
  mse:  m_b = sum w (p-y)^2 / W_b, data term mean_b m_b;   d pred = s 2 w (p-y) / (B W_b)
  cosine / pearson:  u = p - mu_p, t = y - mu_y, mu = sum w (.) / W_b (0 for cosine), S_uu = sum w u^2, S_tt = sum w t^2,
    S_ut = sum w u t, c_b = S_ut / (max(sqrt S_uu, 1e-8) max(sqrt S_tt, 1e-8)), data term 1 - mean_b c_b;
    d pred = w (a u + b t), a and b as head_loss_emul.coefficients on the weighted sums.
Where w = 0 neither p nor y enters (a select): NaN there changes nothing, and d pred is exactly 0.

Bars follow head_emul's rule, c * 2^-24 * sum|terms| + 2^-22 * |ref|, c read from the kernels' chains:

  rowstat.  The row walk is head_rowstat_kernel's: C = L.rowstat_chain(V) additions into one accumulator and through
    block_sum.  W_b: the terms are w themselves -> C.  The means sp / sw: every term w*p is one rounding (C + 1 on
    sum|w p| / W), the divisor carries C more and the division one, both relative to |mu| <= sum|w p| / W -> 2C + 3.
    The centred sums are judged with the DEVICE's own means: u = p - mu is one rounding and enters twice (or u and t once
    each), w*u*u two products -> C + 4.  m_b = sm / sw: d = p - y enters twice, two products (C + 4), the divisor C, the
    division 1 -> 2C + 5, relative.  c_b from the device's own three sums: 8 * 2^-24 relative (head_loss_emul).
  loss.  Clips are summed in double; the data term is rounded once to fp32 -> 2 * 2^-24 on its terms.  loss_terms[1] gets
    head_emul's l2 bar here (the GPU test asks for the plain forward's bits).
  dpred.  From the device's own wstat.  mse: B*W_b, the division, cm*w, p - y, the product -> 5 on |d pred|.  cosine /
    pearson: head_loss_emul's C_DP = 9 on |a u| + |b t|, and the product with w -> 10 on w (|a u| + |b t|).
  ridge_bwd_w, dz.  From the device's own d pred, so head_emul's chains WITHOUT the roundings of forming d pred:
    dW: B + 1 + 2;  dbias: B + ceil(B/8) + 2;  dz, B <= 16: d pred rounded to bf16 exactly as dpred_t_kernel rounds the
    buffer, ceil(GV/splits) + splits + 2 + 1;  B > 16: ceil(ceil(V/32)/4) + 3 + 32 + 2 + 1.

Nothing is fitted to a measurement.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import head_emul as H
import head_loss_emul as L

F64, F32, BF16 = H.F64, H.F32, H.BF16
U, R, HB = H.U, H.R, H.HB
LOSSES = ("mse", "cosine", "pearson")
STAGES = ("rowstat", "loss", "dpred", "ridge_bwd_w", "dz")
REST = ("pool", "ln2", "ln2_bwd", "dhidden")          # head_emul's stages neither the weights nor the heads change
C_DP_MSE, C_DP_CORR = 5, L.C_DP + 1


# ---------------------------------------------------------------------------------------------------- cases
def _case(id, E, S, B, V, losses=LOSSES, G=0, group=None, **kw):
    c = H._case(id, E, S, B, V, **kw)
    c.update(losses=tuple(losses), G=G, group=None if group is None else tuple(group))
    return c


_SK, _BIG = H._SKINNY, H._BIG
CASES = [
    # V = 1: one target (no pearson); B = 1.  E = 128: the MFMA ridge forward
    _case("w-V1", 128, 33, 1, 1, losses=("mse", "cosine"), expect=("ridge_fwd_mfma_kernel<1>", "ridge_bwd_w:b0_passes=1") + _SK),
    _case("w-V2", 128, 33, 8, 2, expect=("ridge_bwd_w:b0_passes=1",) + _SK),
    # V = 5, 17: rows of pred / y / tw that start 1, 2, 3 elements off a 16-byte boundary.  E = 264: the scalar ridge forward
    _case("w-V5", 264, 33, 9, 5, expect=("ridge_fwd_kernel", "ridge_bwd_w:b0_passes=2") + _SK),
    _case("w-V17", 128, 33, 17, 17, expect=("ridge_bwd_w:b0_passes=3",) + _BIG),
    _case("w-V300", 264, 33, 17, 300, drop=True, scales=(0.25, 0.5), expect=_BIG),
    # V = 1030: past one 1024-thread stride of scalars; an all-zero clip; dropout and both scales != 1
    _case("w-V1030", 128, 33, 3, 1030, zero_clip=True, drop=True, scales=(0.25, 0.5), expect=_SK),
    _case("w-packed", 128, 70, 3, 17, lens=(70, 1, 37), expect=_SK),
    # three heads with their own weight rows, head 1 absent from the batch; both dz routes
    _case("w-G3", 128, 33, 9, 17, G=3, group=(0, 2, 0, 2, 2, 0, 0, 2, 0), expect=_SK),
    _case("w-G3-B17", 264, 33, 17, 5, G=3, group=(2, 0) * 8 + (2,), expect=_BIG),
]
BY_ID = {c["id"]: c for c in CASES}
PAIRS = [(c["id"], k) for c in CASES for k in c["losses"]]


def make_weights(V, seed):
    """[V]: zeros, ones and non-integers; a zero at each position of a 4-element group (0, 5, 10, 15) where V allows; the
    last two targets positive (pearson needs two)"""
    gen = torch.Generator().manual_seed(seed)
    r = torch.rand(V, generator=gen)
    w = torch.where(r < 0.25, torch.zeros(V), torch.where(r < 0.5, torch.ones(V), 0.25 + 1.5 * torch.rand(V, generator=gen)))
    for i in (0, 5, 10, 15):
        if i < V - 2:
            w[i] = 0
    w[-1] = 0.75
    if V >= 2:
        w[-2] = 1.0
    return w.float()


# Re-drawn cases (head_emul.RESEED's rule): (case id, loss) -> the first draw whose bf16 roundings alone stay within
# E2E_FORMAT_SHARE of every end-to-end bar; test_cpu_wloss_emul asserts that and that no earlier draw does.
RESEED = {("w-V2", "mse"): 1}


def make_inputs(case, loss, reseed=None):
    inp = H.make_inputs(dict(case, reseed=RESEED.get((case["id"], loss), 0) if reseed is None else reseed))
    E, B, V, G = case["E"], case["B"], case["V"], case["G"]
    inp["loss"] = loss
    Hh = max(1, G)
    inp["tw"] = torch.stack([make_weights(V, 100 * V + g) for g in range(Hh)])
    inp["group"] = None if not G else torch.tensor(case["group"], dtype=torch.int64)
    if G:                       # heads 1.. drawn like head 0; stacked [G*V, E] / [G*V]
        gen = torch.Generator().manual_seed(977 * V + E)
        p = inp["params"]
        Ws = [p["ridge_layer.linear.weight"]] + [(torch.randn(V, E, generator=gen) / math.sqrt(E)).to(BF16).float() for _ in range(G - 1)]
        bs = [p["ridge_layer.linear.bias"]] + [(0.1 * torch.randn(V, generator=gen)).to(BF16).float() for _ in range(G - 1)]
        p["ridge_layer.linear.weight"], p["ridge_layer.linear.bias"] = torch.cat(Ws), torch.cat(bs)
    return inp


@functools.lru_cache(maxsize=None)
def inputs_for(case_id, loss):
    """the inputs of a named case, made once and shared (treat as read-only)"""
    return make_inputs(BY_ID[case_id], loss)


def clip_weights(inp, bug=None):
    """w [B,V]: the weight row of every clip's head"""
    tw, g = inp["tw"], inp["group"]
    B = inp["case"]["B"]
    if g is None:
        return tw[0].expand(B, -1)
    if bug == "wrong_head":
        g = (g + 1) % tw.shape[0]
    return tw[g]


# ---------------------------------------------------------------------------------------------------- the new stages
BUGS = {"dpred_no_w": "dpred", "div_by_V": "rowstat", "unweighted_means": "rowstat", "wrong_head": "rowstat",
        "mul_zero": "rowstat", "drop_tail": "rowstat"}


def rowstat(pred, y, w, loss, mu=None, dt=F64, bug=None):
    """head_wrowstat_kernel.  -> mu_p, mu_y, suu, stt, sut, c, W, m [B] (+ magnitudes).  ``mu`` = (mu_p, mu_y) to centre with."""
    w = w.to(dt)
    keep = w > 0
    zero = torch.zeros((), dtype=dt)
    if bug == "mul_zero":
        p, yy = pred.to(dt), y.to(dt)                         # w * NaN = NaN
    else:
        p, yy = torch.where(keep, pred.to(dt), zero), torch.where(keep, y.to(dt), zero)
    if bug == "drop_tail":
        w = w.clone()
        w[:, -1] = 0
    V = p.shape[1]
    Wb = w.sum(1)
    zb = torch.zeros(p.shape[0], dtype=dt)
    if loss == "pearson":
        mu_p, mu_y = ((p.sum(1) / V, yy.sum(1) / V) if bug == "unweighted_means" else ((w * p).sum(1) / Wb, (w * yy).sum(1) / Wb))
    else:
        mu_p, mu_y = zb, zb
    mp, my = (mu_p, mu_y) if mu is None else (mu[0].to(dt), mu[1].to(dt))
    d = p - yy
    sm = (w * d * d).sum(1)
    out = dict(mu_p=mu_p, mu_y=mu_y, W=Wb, m=sm / (V if bug == "div_by_V" else Wb), mag_p=(w * p).abs().sum(1) / Wb,
               mag_y=(w * yy).abs().sum(1) / Wb)
    if loss == "mse":
        out.update(suu=zb, stt=zb, sut=zb, c=zb, mag_ut=zb)
        return out
    u, t = torch.where(keep, p - mp[:, None], zero), torch.where(keep, yy - my[:, None], zero)
    out.update(suu=(w * u * u).sum(1), stt=(w * t * t).sum(1), sut=(w * u * t).sum(1), mag_ut=(w * u * t).abs().sum(1))
    out["c"] = L.corr_from_sums(out["suu"], out["stt"], out["sut"])
    return out


def rowstat_bars(ref, V):
    c = L.rowstat_chain(V)
    return dict(W=(c * U + R) * ref["W"], m=((2 * c + 5) * U + R) * ref["m"],
                mu_p=(2 * c + 3) * U * ref["mag_p"] + R * ref["mu_p"].abs(), mu_y=(2 * c + 3) * U * ref["mag_y"] + R * ref["mu_y"].abs(),
                suu=((c + 4) * U + R) * ref["suu"], stt=((c + 4) * U + R) * ref["stt"],
                sut=(c + 4) * U * ref["mag_ut"] + R * ref["sut"].abs())


def loss_terms(m, c, l2, loss):
    """wloss_finalize_kernel: m, c [B] (the device's own), l2 from head_emul.ridge"""
    B = m.numel()
    ms, cs = m.to(F64).sum() / B, c.to(F64).sum() / B
    data = ms if loss == "mse" else 1 - cs
    return dict(loss=torch.stack([data, l2, data + l2]), aux=torch.stack([ms, cs]), terms=ms.abs() if loss == "mse" else 1 + cs.abs())


def loss_bars(ref, l2_bar):
    bar_d = 2 * U * ref["terms"] + R * ref["loss"][0].abs()
    return dict(loss=torch.stack([bar_d, l2_bar, bar_d + l2_bar + R * ref["loss"][2].abs()]),
                aux=(2 * U + R) * ref["aux"].abs())


def dpred(pred, y, w, rs, loss, loss_scale, dt=F64, bug=None):
    """head_wdpred_kernel from row statistics ``rs`` -> (d pred [B,V], the magnitude its error scales with).  Exactly 0 at w = 0."""
    w = w.to(dt)
    keep = w > 0
    zero = torch.zeros((), dtype=dt)
    p, yy = torch.where(keep, pred.to(dt), zero), torch.where(keep, y.to(dt), zero)
    B, V = p.shape
    wf = torch.where(keep, torch.ones((), dtype=dt), zero) if bug == "dpred_no_w" else w
    if loss == "mse":
        den = V if bug == "div_by_V" else rs["W"].to(dt)[:, None]
        dp = loss_scale * 2.0 * wf * (p - yy) / (B * den)
        return dp, dp.abs()
    a, b = L.coefficients(rs["suu"].to(dt), rs["stt"].to(dt), rs["c"].to(dt), B, loss_scale)
    u = torch.where(keep, p - rs["mu_p"].to(dt)[:, None], zero)
    t = torch.where(keep, yy - rs["mu_y"].to(dt)[:, None], zero)
    au, bt = a[:, None] * u, b[:, None] * t
    return wf * (au + bt), wf * (au.abs() + bt.abs())


def dpred_bar(dp, mag, loss):
    return (C_DP_MSE if loss == "mse" else C_DP_CORR) * U * mag + R * dp.abs()


def _heads(inp):
    """(group [B] int64, number of heads, V): one head -> all zero"""
    c = inp["case"]
    g = torch.zeros(c["B"], dtype=torch.int64) if inp["group"] is None else inp["group"]
    return g, max(1, c["G"]), c["V"]


def ridge_pred(z, W, bias, inp, dt=F64):
    """the (grouped) ridge forward: pred[b] = W[g_b] z[b] + bias[g_b]; l2 over every head; -> pred, its magnitude, l2"""
    g, Hh, V = _heads(inp)
    z, W3, b2 = z.to(dt), W.to(dt).view(Hh, V, -1), bias.to(dt).view(Hh, V)
    pred = torch.einsum("be,bve->bv", z, W3[g]) + b2[g]
    mag = torch.einsum("be,bve->bv", z.abs(), W3[g].abs()) + b2[g].abs()
    return pred, mag, (W.to(dt) ** 2).sum()


def ridge_bwd_w(dp, z, W, l2coef, inp, dt=F64):
    """DP_BUF ridge_bwd_w_kernel: dW [H*V,E] = l2coef W + sum_{b of the head} dp[b,v] z[b], dbias [H*V]"""
    g, Hh, V = _heads(inp)
    dp, z, W = dp.to(dt), z.to(dt), W.to(dt)
    onehot = torch.nn.functional.one_hot(g, Hh).to(dt)                    # [B,H]
    dpe = (onehot[:, :, None] * dp[:, None, :]).reshape(dp.shape[0], Hh * V)      # [B, H*V]: dp in the clip's head, 0 elsewhere
    seed = l2coef * W
    return dict(dW=seed + dpe.t() @ z, dbias=dpe.sum(0), mag_dW=seed.abs() + dpe.abs().t() @ z.abs(), mag_dbias=dpe.abs().sum(0))


def ridge_bwd_w_bars(ref, B):
    return dict(dW=(B + 1 + 2) * U * ref["mag_dW"] + R * ref["dW"].abs(),
                dbias=(B + H.cdiv(B, 8) + 2) * U * ref["mag_dbias"] + R * ref["dbias"].abs())


def dz(dp, W, keep, inp, round_dp_bf16, dt=F64):
    g, Hh, V = _heads(inp)
    dp = dp.to(BF16).to(dt) if round_dp_bf16 else dp.to(dt)
    W3 = W.to(dt).view(Hh, V, -1)
    k = torch.ones(dp.shape[0], W3.shape[2], dtype=dt) if keep is None else keep.to(dt)
    return dict(dz=torch.einsum("bv,bve->be", dp, W3[g]) * k, mag=torch.einsum("bv,bve->be", dp.abs(), W3[g].abs()) * k)


def dz_bars(ref, B, V, Hh):
    if B <= 16:
        sp = H.wgrad_splits(Hh * V)
        c = H.cdiv(Hh * V, sp) + sp + 2 + 1
    else:
        c = H.cdiv(H.cdiv(V, 32), 4) + 3 + 32 + 2 + 1
    return dict(dz=c * U * ref["mag"] + R * ref["dz"].abs())


WSTAT = ("mu_p", "mu_y", "suu", "stt", "sut", "c", "W", "m")


def wstat_columns(buf):
    """BrainHead.wstat [B,8] -> the named columns ``run`` returns"""
    return {k: buf[:, i].contiguous() for i, k in enumerate(WSTAT)}


# ---------------------------------------------------------------------------------------------------- the chain
def run(inp, dt=F64, device_like=False, bug=None, y=None):
    """head_emul.run with the weighted objective (and, with G, the stacked heads): every buffer ``BrainHead`` holds after a
    forward and a backward, plus wstat's columns, loss_aux and dpred.  ``y``: targets to use instead of inp["y"]."""
    loss, p, c = inp["loss"], inp["params"], inp["case"]
    B = c["B"]
    y = inp["y"] if y is None else y
    W, g1, g2 = p["ridge_layer.linear.weight"], p["layer_norm1.weight"], p["layer_norm2.weight"]
    w = clip_weights(inp, bug=bug)
    po = H.pool(inp["hidden"], inp["wmask"], inp["eps"], dt=dt)
    l2o = H.ln2(po["pooled_raw"], po["sumw"], g1, p["layer_norm1.bias"], g2, p["layer_norm2.bias"], inp["keep"], inp["eps"], dt=dt)
    z = l2o["z"].to(BF16).to(dt) if device_like else l2o["z"]
    lam = float(np.float32(inp["lam"])) if device_like else inp["lam"]
    pred, _, w2 = ridge_pred(z, W, p["ridge_layer.linear.bias"], inp, dt=dt)
    rs = rowstat(pred, y, w, loss, dt=dt, bug=bug)
    lo = loss_terms(rs["m"], rs["c"], (lam * w2).to(F64), loss)
    if device_like:
        l2coef, s = H.host_scales(B, c["V"], inp["lam"], inp["loss_scale"], inp["l2_scale"])[1], float(np.float32(inp["loss_scale"]))
    else:
        l2coef, s = inp["l2_scale"] * 2.0 * inp["lam"], inp["loss_scale"]
    dp, _ = dpred(pred, y, w, rs, loss, s, dt=dt, bug=bug)
    wo = ridge_bwd_w(dp, z, W, l2coef, inp, dt=dt)
    do = dz(dp, W, inp["keep"], inp, device_like and B <= 16, dt=dt)
    bo = H.ln2_bwd(do["dz"], g2, l2o["zhat"], l2o["ln2_rstd"], g1, po["pooled_raw"], po["sumw"], dt=dt)
    ho = H.dhidden(inp["hidden"], inp["wmask"], po["mu"], po["rstd"], bo["dpooled"], dt=dt)
    dh = ho["dh"].to(BF16).to(dt) if device_like else ho["dh"]
    out = dict(mu=po["mu"], rstd=po["rstd"], pooled_raw=po["pooled_raw"], sumw=po["sumw"], zhat=l2o["zhat"],
               ln2_rstd=l2o["ln2_rstd"], z=z, pred=pred, loss_terms=lo["loss"].to(dt), loss_aux=lo["aux"].to(dt), dpred=dp,
               dW=wo["dW"], dbias=wo["dbias"], dz=do["dz"], dpooled=bo["dpooled"], dg2=bo["dg2"], db2=bo["db2"], dg1=bo["dg1"],
               db1=bo["db1"], dh=dh)
    out.update({k: rs[k].to(dt) for k in WSTAT})
    return out


def whole(inp):
    """the head with the weighted objective as mathematics: fp64, nothing rounded"""
    return run(inp, dt=F64, device_like=False)


# ---------------------------------------------------------------------------------------------------- the check
def check_stages(bufs, inp, stages=STAGES, y=None):
    """Each new stage's outputs in ``bufs`` (named as in ``run``) against its fp64 restatement fed with bufs' own upstream
    buffers.  -> {"stage.output": max(err / bar)}.  ``y``: the targets the step was given, if not inp["y"]."""
    inp = inp if y is None else dict(inp, y=y)
    c, p, loss = inp["case"], inp["params"], inp["loss"]
    B, E, V = c["B"], c["E"], c["V"]
    W = p["ridge_layer.linear.weight"]
    w = clip_weights(inp)
    l2coef, s = H.host_scales(B, V, inp["lam"], inp["loss_scale"], inp["l2_scale"])[1], float(np.float32(inp["loss_scale"]))
    out = {}
    if "rowstat" in stages:
        ref = rowstat(bufs["pred"], inp["y"], w, loss)                                        # W, m, the means: from pred and y
        bars = rowstat_bars(ref, V)
        for n in ("W", "m") + (("mu_p", "mu_y") if loss == "pearson" else ()):
            out[f"rowstat.{n}"] = H.ratio(bufs[n], ref[n], bars[n])
        if loss != "mse":
            ref = rowstat(bufs["pred"], inp["y"], w, loss, mu=(bufs["mu_p"], bufs["mu_y"]))   # the sums: with the device's means
            bars = rowstat_bars(ref, V)
            for n in ("suu", "stt", "sut"):
                out[f"rowstat.{n}"] = H.ratio(bufs[n], ref[n], bars[n])
            cref = L.corr_from_sums(bufs["suu"].to(F64), bufs["stt"].to(F64), bufs["sut"].to(F64))
            out["rowstat.c"] = H.ratio(bufs["c"], cref, 8 * U * cref.abs())
        zeros = ("mu_p", "mu_y") if loss == "cosine" else ("mu_p", "mu_y", "suu", "stt", "sut", "c") if loss == "mse" else ()
        if any(bool((bufs[n] != 0).any()) for n in zeros):
            out["rowstat.zeros"] = float("inf")
    if "loss" in stages:
        _, _, w2 = ridge_pred(bufs["z"], W, p["ridge_layer.linear.bias"], inp)
        lam = float(np.float32(inp["lam"]))
        l2 = (lam * w2).to(F64)
        l2_bar = H.ridge_bars(dict(pred=l2, mag_pred=l2, loss=torch.stack([0 * l2, l2, l2])), B, E, W.shape[0])["loss"][1]   # head_emul's l2 bar
        ref = loss_terms(bufs["m"], bufs["c"], lam * w2, loss)
        bars = loss_bars(ref, l2_bar)
        out["loss.loss_terms"] = H.ratio(bufs["loss_terms"], ref["loss"], bars["loss"])
        out["loss.loss_aux"] = H.ratio(bufs["loss_aux"], ref["aux"], bars["aux"])
    if "dpred" in stages:
        dp, mag = dpred(bufs["pred"], inp["y"], w, bufs, loss, s)
        out["dpred.dpred"] = H.ratio(bufs["dpred"], dp, dpred_bar(dp, mag, loss))
        if bool((bufs["dpred"][w == 0] != 0).any()):
            out["dpred.masked"] = float("inf")                 # exactly 0 where w = 0
    if "ridge_bwd_w" in stages:
        ref = ridge_bwd_w(bufs["dpred"], bufs["z"], W, l2coef, inp)
        bars = ridge_bwd_w_bars(ref, B)
        for n in ("dW", "dbias"):
            out[f"ridge_bwd_w.{n}"] = H.ratio(bufs[n].reshape(ref[n].shape), ref[n], bars[n])
    if "dz" in stages:
        ref = dz(bufs["dpred"], W, inp["keep"], inp, B <= 16)
        out["dz.dz"] = H.ratio(bufs["dz"], ref["dz"], dz_bars(ref, B, V, max(1, c["G"]))["dz"])
    return out


def check_rest(bufs, inp):
    """the stages the weights leave alone: head_emul's own checks of pool, LN2 and the LN backward / d hidden, and the
    (grouped) ridge prediction at head_emul's ridge bar"""
    c, p = inp["case"], inp["params"]
    out = H.check_stages(bufs, inp, REST)
    pred, mag, _ = ridge_pred(bufs["z"], p["ridge_layer.linear.weight"], p["ridge_layer.linear.bias"], inp)
    bar = H.ridge_bars(dict(pred=pred, mag_pred=mag, loss=torch.ones(3, dtype=F64)), c["B"], c["E"], c["V"])["pred"]
    out["ridge.pred"] = H.ratio(bufs["pred"], pred, bar)
    return out


def flat(inp):
    """as head_loss_emul.flat, on the targets that count: with one positive weight (cosine) or two (pearson) per clip the
    data term is +-1 whatever the prediction, d pred is zero as mathematics and a relative error of a gradient says nothing"""
    npos = int((inp["tw"] > 0).sum(1).min())
    return (inp["loss"] == "cosine" and npos <= 1) or (inp["loss"] == "pearson" and npos <= 2)


def end_to_end(bufs, inp):
    """-> {name: max|got - ref| / max|ref|} against ``whole(inp)``, each held to head_emul.E2E_BARS"""
    ref = whole(inp)
    b = dict(bufs, dW=bufs["dW"].reshape(ref["dW"].shape), dbias=bufs["dbias"].reshape(ref["dbias"].shape))
    out = H._e2e_errors(b, ref)
    return {k: v for k, v in out.items() if k in ("pred", "l2", "total", "dW")} if flat(inp) else out


def format_deviation(inp):
    """the same figures for fp64 arithmetic with only the bf16 roundings (and fp32 scales) of the device"""
    return end_to_end(run(inp, dt=F64, device_like=True), inp)
