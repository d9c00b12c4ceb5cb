"""fp64 restatement of the GROUPED tail of the brain head (per-subject ridge heads on one trunk), one
kernel at a time, with derived bars, cases, planted bugs and a restatement of the grouped planner.  The companion of
tests/head_emul.py (``H``: the staged fp64 head) and tests/head_loss_emul.py (``L``: the correlation objectives), for the
kernels vlb_head_fwd_grouped / vlb_head_bwd_grouped launch:

  ln2          head_ln2_kernel                      unchanged, shared by all heads                        (H.ln2)
  ridge        ridge_fwd_mfma_kernel<KS,grouped> / ridge_fwd_kernel<grouped> + loss_finalize[_corr]_kernel
  rowstat/loss head_rowstat_kernel, loss_finalize_corr_kernel on the [B,V] rows (cosine / pearson only)   (L.rowstat ...)
  ridge_bwd_w  ridge_bwd_w_kernel<CORR,grouped>     dW [G,V,E], dbias [G,V]
  dz           dpred_t_kernel<CORR,grouped> + skinny wgrad over all G*V rows + head_dz_from16, or
               ridge_bwd_z_kernel<CORR,grouped> + head_dz_reduce
  ln2_bwd      head_ln2_bwd_kernel + head_param_grads_kernel, unchanged                                   (H.ln2_bwd)

Semantics.  W [G,V,E], bias [G,V], group[b] in [0,G):  pred[b] = W[group[b]] z[b] + bias[group[b]];  the data term is the
ungrouped one over the [B,V] batch;  l2 = lam * sum over ALL G heads of |W_g|^2;  d pred is formed with the whole batch's B;
dW[g] = l2coef W[g] + sum_{b in g} dp[b]^T z[b],  dbias[g] = sum_{b in g} dp[b],  dz[b] = keep * dp[b] W[group[b]].
A stage here runs the ungrouped stage function of H / L once per head on that head's clips and puts the pieces together.

Bars: head_emul's rule, c * 2^-24 * sum|terms| + 2^-22 * |ref|, each c read from the grouped kernel's addition chain:

  ridge, MFMA form.  One output is KSTEPS MFMAs of 32 products, 3 K-quarters and the bias, as ungrouped:
      c_pred = 32*KSTEPS + 3 + 1 + 2.
    A persistent block takes tpb = ceil(G*tpg / min(G*tpg, 2048)) row tiles (tpg = ceil(V/16) tiles per head); per tile a lane
    adds at most 4 squared errors (only on the tiles of its clip's head: fewer, never more) and 8*KSTEPS squares of W:
      c_mse = 4*tpb + 6 + 3 + 2,   c_w2 = 8*KSTEPS*tpb + 6 + 3 + 2.
  ridge, scalar form.  A block is 16 rows of ONE head: lane 0 adds 4 rows x (clips of that head <= B) squared errors:
      c_pred = 8*ceil(E/512) + 6 + 1 + 2,   c_mse = 4*B + 3 + 2,   c_w2 = 8*ceil(E/512)*4 + 6 + 3 + 2.
  ridge_bwd_w.  Row (g, v) adds the n_g clips of head g onto the seed l2coef*W, clips of other heads are skipped:
      c_dW = n_g + 1 + 2 + c_dp,   c_db = n_g + ceil(B/8) + 2 + c_dp     (the read-modify-write per b0 pass stays)
    with c_dp = 2 (gscale*(pred - y)) or L.C_DP (correlation objectives).  n_g = 0: the bar is 2^-22 |l2coef W|; the GPU test
    asks the exact fp32 product on top.
  dz, B <= 16.  ONE skinny contraction over all G*V rows, sp = wgrad_splits(G*V) splits: a split's ceil(G*V/sp) rows go
    through the MFMA accumulator (the other heads' rows add exact zeros; they still count), then the splits, then keep:
      c_dz = ceil(G*V/sp) + sp + 2 + 1.
  dz, B > 16.  Clip b walks only the rows of its own head, V/32 per split over 4 waves, as ungrouped:
      c_dz = ceil(ceil(V/32)/4) + 3 + 32 + 2 + 1 + c_dp.
Nothing is fitted to a run; tests print max(err / bar) and assert <= 1.
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
STAGES = ("ln2", "ridge", "ridge_bwd_w", "dz", "ln2_bwd")
LOSS_STAGES = ("rowstat", "loss")
GROUPED_MAX_ROWS = 1 << 27


# ---------------------------------------------------------------------------------------------------- the planner
def grouped_fwd_parts(B, E, V, G):
    """ridge_fwd_parts of head.hip with G heads: (sum err^2, sum W^2) pairs the grouped ridge forward leaves, one per block"""
    ntiles = G * H.cdiv(V, 16)
    return min(ntiles, 2048) if H.mfma_ridge(B, E) else G * H.cdiv(V, 16)


def tile_of(t, V):
    """row tile t of the MFMA form -> (head, first row inside the head): a tile never spans two heads"""
    tpg = H.cdiv(V, 16)
    return t // tpg, 16 * (t % tpg)


def dispatch(B, E, G):
    """Kernels vlb_head_fwd_grouped + vlb_head_bwd_grouped run for (B, E): their branch conditions, restated"""
    k = {"feature_cache_gather_kernel", "head_ln2_kernel", "ridge_bwd_w_kernel<grouped>", f"ridge_bwd_w:b0_passes={H.cdiv(B, 8)}",
         "head_ln2_bwd_kernel", "head_param_grads_kernel"}
    k.add(f"ridge_fwd_mfma_kernel<{E // 128},grouped>" if B <= 16 and E % 128 == 0 and E <= 4096 else "ridge_fwd_kernel<grouped>")
    if B <= 16 and E % 8 == 0:
        k |= {"dpred_t_kernel<grouped>", "wgrad_mfma_kernel", "head_dz_from16_kernel"}
    else:
        k |= {"ridge_bwd_z_kernel<grouped>", "head_dz_reduce_kernel"}
    return k


# ---------------------------------------------------------------------------------------------------- cases
_SK = ("dpred_t_kernel<grouped>", "wgrad_mfma_kernel", "head_dz_from16_kernel")
_BIG = ("ridge_fwd_kernel<grouped>", "ridge_bwd_z_kernel<grouped>", "head_dz_reduce_kernel")


def _case(id, E, B, V, G, subjects, expect=(), **kw):
    c = H._case(id, E, 33, B, V, **kw)
    assert len(subjects) == B and all(0 <= g < G for g in subjects)
    c.update(G=G, subjects=tuple(subjects), expect=tuple(expect))
    return c


CASES = [
    _case("g3-B5", 512, 5, 40, 3, [2, 0, 2, 1, 0], expect=("ridge_fwd_mfma_kernel<4,grouped>",) + _SK),
    # two absent heads (0 and 2); V = 17: the last tile of every head has one live row
    _case("g4-absent", 512, 3, 17, 4, [3, 1, 3], expect=("ridge_fwd_mfma_kernel<4,grouped>",) + _SK),
    _case("g3-V5", 512, 4, 5, 3, [0, 1, 2, 1], expect=("ridge_fwd_mfma_kernel<4,grouped>",) + _SK),      # heads smaller than a tile
    _case("g2-B16", 1024, 16, 40, 2, [i % 2 for i in range(16)],
          expect=("ridge_fwd_mfma_kernel<8,grouped>", "ridge_bwd_w:b0_passes=2") + _SK),
    # the scalar forward and the grouped ridge_bwd_z, three b0 passes, dropout and both scales != 1; a head changes inside a pass
    _case("g3-B17", 1024, 17, 40, 3, [(2 * i + i // 5) % 3 for i in range(17)], drop=True, scales=(0.25, 0.5),
          expect=("ridge_bwd_w:b0_passes=3",) + _BIG),
    _case("g2-E264", 264, 2, 48, 2, [1, 0], expect=("ridge_fwd_kernel<grouped>",) + _SK),               # scalar forward, skinny dz
    _case("g2-E4096", 4096, 3, 33, 2, [1, 0, 1], expect=("ridge_fwd_mfma_kernel<32,grouped>",) + _SK),  # KSTEPS = 32
]
BY_ID = {c["id"]: c for c in CASES}
LOSS_CASES = ("g3-B5", "g3-B17")           # also run with loss = "cosine" and "pearson"
G1_CASES = [_case("g1-B5", 512, 5, 40, 1, [0] * 5), _case("g1-B17", 1024, 17, 40, 1, [0] * 17, drop=True, scales=(0.25, 0.5))]


def make_inputs(case, loss="mse"):
    """head_emul.make_inputs for the case, with (W, b) drawn per head: params['ridge_layer.linear.weight'] [G,V,E],
    ['ridge_layer.linear.bias'] [G,V] (bf16-valued), inp['group'] the head of every clip, inp['loss']."""
    inp = H.make_inputs(case)
    E, V, G = case["E"], case["V"], case["G"]
    gen = torch.Generator().manual_seed(424243 + E * 31 + V * 7 + G)
    W = torch.randn(G, V, E, generator=gen) / math.sqrt(E)
    b = 0.1 * torch.randn(G, V, generator=gen)
    inp["params"]["ridge_layer.linear.weight"] = W.to(BF16).float()
    inp["params"]["ridge_layer.linear.bias"] = b.to(BF16).float()
    inp["group"] = list(case["subjects"])
    inp["loss"] = loss
    return inp


@functools.lru_cache(maxsize=None)
def inputs_for(case_id, loss="mse"):
    """the inputs of a named case, made once and shared (treat as read-only)"""
    return make_inputs(BY_ID[case_id], loss)


def clips_of(group, G):
    """[G] index tensors: the clips of every head, ascending"""
    g = torch.as_tensor(group)
    return [torch.nonzero(g == k).flatten() for k in range(G)]


# ---------------------------------------------------------------------------------------------------- stages
BUGS = {  # planted bug -> the stage whose bar must reject it
    "route_next": "ridge",            # a clip contracted with head (g+1) % G
    "flat_tiles": "ridge",            # row tiles cut from the flat rows g*V + v: a tile that straddles two heads serves the first
    "l2_present_only": "ridge",       # the penalty over the heads that have a clip in the batch
    "gscale_group_count": "ridge_bwd_w",      # gscale formed with the head's clip count in place of B
    "absent_dbias": "ridge_bwd_w",    # a head without clips gets the batch's dbias instead of 0
}


def ridge(z, W, bias, y, group, lam, pred_for_loss=None, dt=F64, bug=None):
    """grouped ridge forward + loss_finalize_kernel -> pred [B,V], mag_pred, loss = (mse, l2, total); H.ridge per head"""
    G, V, E = W.shape
    B = z.shape[0]
    pred, mag = torch.zeros(B, V, dtype=dt), torch.zeros(B, V, dtype=dt)
    l2 = torch.zeros((), dtype=dt)
    for g, idx in enumerate(clips_of(group, G)):
        src = (g + 1) % G if bug == "route_next" else g
        r = H.ridge(z[idx], W[src], bias[src], y[idx], lam, dt=dt)
        pr = r["pred"]
        if bug == "flat_tiles":       # flat row g*V + v sits in tile (g*V + v) // 16, which serves the head of its first row
            rows = g * V + torch.arange(V)
            lost = (16 * (rows // 16)) // V != g
            pr = torch.where(lost[None, :], torch.zeros((), dtype=dt), pr)
        pred[idx], mag[idx] = pr, r["mag_pred"]
        if not (bug == "l2_present_only" and idx.numel() == 0):
            l2 = l2 + r["loss"][1]
    d = (pred if pred_for_loss is None else pred_for_loss.to(dt)) - y.to(dt)
    mse = (d * d).sum() / (B * V)
    return dict(pred=pred, mag_pred=mag, loss=torch.stack([mse, l2, mse + l2]))


def ridge_bars(ref, B, E, V, G):
    if H.mfma_ridge(B, E):
        ks, ntiles = E // 128, G * H.cdiv(V, 16)
        tpb = H.cdiv(ntiles, min(ntiles, 2048))
        c_pred = 32 * ks + 3 + 1 + 2
        c_mse = 4 * tpb + 6 + 3 + 2
        c_w2 = 8 * ks * tpb + 6 + 3 + 2
    else:
        nch = H.cdiv(E, 512)
        c_pred = 8 * nch + 6 + 1 + 2
        c_mse = 4 * B + 3 + 2
        c_w2 = 8 * nch * 4 + 6 + 3 + 2
    mse, l2, tot = ref["loss"]
    bar_mse, bar_l2 = ((c_mse + 2) * U + R) * mse, (c_w2 * U + R) * l2
    return dict(pred=c_pred * U * ref["mag_pred"] + R * ref["pred"].abs(), loss=torch.stack([bar_mse, bar_l2, bar_mse + bar_l2 + R * tot]))


def _dpred(pred, y, inp_loss, rs, B, V, gscale, s, dt, bug=None, n_g=None):
    """d pred [B,V] of the whole batch and the magnitude its error scales with; (c_dp roundings)"""
    if inp_loss == "mse":
        gs = gscale * B / n_g[:, None].clamp_min(1).to(dt) if bug == "gscale_group_count" else gscale
        dp = gs * (pred.to(dt) - y.to(dt))
        return dp, dp.abs()
    return L.dpred(pred, y, rs, s, dt=dt)


def ridge_bwd_w(dp, mag_dp, z, W, group, l2coef, dt=F64, bug=None):
    """ridge_bwd_w_kernel<grouped> -> dW [G,V,E], dbias [G,V] (+ their magnitudes, n_g): L.ridge_bwd_w per head"""
    G = W.shape[0]
    out = dict(dW=[], dbias=[], mag_dW=[], mag_dbias=[], n=[])
    for g, idx in enumerate(clips_of(group, G)):
        r = L.ridge_bwd_w(dp[idx].to(dt), mag_dp[idx].to(dt), z[idx], W[g], l2coef, dt=dt)
        if bug == "absent_dbias" and idx.numel() == 0:
            r["dbias"] = dp.to(dt).sum(0)
        for k in ("dW", "dbias", "mag_dW", "mag_dbias"):
            out[k].append(r[k])
        out["n"].append(idx.numel())
    return {k: torch.stack(v) if k != "n" else v for k, v in out.items()}


def ridge_bwd_w_bars(ref, B, c_dp):
    n = torch.tensor(ref["n"], dtype=F64)
    c_dW = (n + 1 + 2 + c_dp)[:, None, None]
    c_db = (n + H.cdiv(B, 8) + 2 + c_dp)[:, None]
    return dict(dW=c_dW * U * ref["mag_dW"] + R * ref["dW"].abs(), dbias=c_db * U * ref["mag_dbias"] + R * ref["dbias"].abs())


def dz(dp, mag_dp, W, keep, group, dt=F64):
    """dz [B,E] = keep * dp[b] W[group[b]] -> dz, mag (|a u|+|b t| through |W|), mag_round (|dp| through |W|): L.dz per head"""
    G, V, E = W.shape
    B = dp.shape[0]
    out = {k: torch.zeros(B, E, dtype=dt) for k in ("dz", "mag", "mag_round")}
    for g, idx in enumerate(clips_of(group, G)):
        r = L.dz(dp[idx].to(dt), mag_dp[idx].to(dt), W[g], None if keep is None else keep[idx], dt=dt)
        for k in out:
            out[k][idx] = r[k]
    return out


def dz_bars(ref, B, V, G, corr):
    if B <= 16:
        sp = H.wgrad_splits(G * V)
        c = H.cdiv(G * V, sp) + sp + 2 + 1
        if corr:       # L.dz_bars: d pred's own fp32 error and its rounding to bf16 ride on the bar
            return dict(dz=(c * U * ref["mag_round"] + L.C_DP * U * ref["mag"] + HB * ref["mag_round"]) + R * ref["dz"].abs())
        return dict(dz=c * U * ref["mag"] + R * ref["dz"].abs())
    c = H.cdiv(H.cdiv(V, 32), 4) + 3 + 32 + 2 + 1 + (L.C_DP if corr else 2)
    return dict(dz=c * U * ref["mag"] + R * ref["dz"].abs())


# ---------------------------------------------------------------------------------------------------- the chain
def _scales(inp, device_like):
    B, V = inp["case"]["B"], inp["case"]["V"]
    if device_like:
        gscale, l2coef = H.host_scales(B, V, inp["lam"], inp["loss_scale"], inp["l2_scale"])
        return gscale, l2coef, float(np.float32(inp["loss_scale"])), float(np.float32(inp["lam"]))
    return inp["loss_scale"] * 2.0 / (B * V), inp["l2_scale"] * 2.0 * inp["lam"], inp["loss_scale"], inp["lam"]


def run(inp, dt=F64, device_like=False, bug=None):
    """Pool (H.pool), then the grouped tail, every stage on its own output -> the buffers ``BrainHead(subjects=...)`` holds after
    a forward and a backward (dW [G,V,E], dbias [G,V]).  dt / device_like as in head_emul.run."""
    c, p, loss, group = inp["case"], inp["params"], inp["loss"], inp["group"]
    B, V, G = c["B"], c["V"], c["G"]
    W, bias, g1, g2 = p["ridge_layer.linear.weight"], p["ridge_layer.linear.bias"], p["layer_norm1.weight"], p["layer_norm2.weight"]
    gscale, l2coef, s, lam = _scales(inp, device_like)
    po = H.pool(inp["hidden"], inp["wmask"], inp["eps"], dt=dt)
    l2o = H.ln2(po["pooled_raw"], po["sumw"], g1, p["layer_norm1.bias"], g2, p["layer_norm2.bias"], inp["keep"], inp["eps"], dt=dt)
    z = l2o["z"].to(BF16).to(dt) if device_like else l2o["z"]
    ro = ridge(z, W, bias, inp["y"], group, lam, dt=dt, bug=bug)
    out = {}
    rs = None
    terms = ro["loss"]
    if loss != "mse":
        rs = L.rowstat(ro["pred"], inp["y"], loss, dt=dt)
        lo = L.loss_terms(rs["c"], ro["loss"][1].to(F64), ro["loss"][0].to(F64))
        terms = lo["loss"].to(dt)
        out["loss_aux"] = lo["aux"].to(dt)
        out.update({k: rs[k].to(dt) for k in ("mu_p", "mu_y", "suu", "stt", "sut", "c")})
    n_g = torch.tensor([int(sum(1 for x in group if x == k)) for k in range(G)])[torch.as_tensor(group)]
    dp, mag = _dpred(ro["pred"], inp["y"], loss, rs, B, V, gscale, s, dt, bug=bug, n_g=n_g)
    wo = ridge_bwd_w(dp, mag, z, W, group, l2coef, dt=dt, bug=bug)
    if device_like and B <= 16:
        dpz = (torch.tensor(gscale, dtype=F32) * (ro["pred"].to(F32) - inp["y"].to(F32))).to(BF16).to(dt) if loss == "mse" else dp.to(BF16).to(dt)
    else:
        dpz = dp
    do = dz(dpz, mag, W, inp["keep"], group, dt=dt)
    bo = H.ln2_bwd(do["dz"], g2, l2o["zhat"], l2o["ln2_rstd"], g1, po["pooled_raw"], po["sumw"], dt=dt)
    out.update(pooled_raw=po["pooled_raw"], sumw=po["sumw"], zhat=l2o["zhat"], ln2_rstd=l2o["ln2_rstd"], z=z, pred=ro["pred"],
               loss_terms=terms, dW=wo["dW"], dbias=wo["dbias"], dz=do["dz"], dpooled=bo["dpooled"], dg2=bo["dg2"], db2=bo["db2"],
               dg1=bo["dg1"], db1=bo["db1"])
    return out


# ---------------------------------------------------------------------------------------------------- the check
def check_stages(bufs, inp, stages=STAGES + LOSS_STAGES):
    """Every stage of ``bufs`` (host tensors named as in ``run``) against its fp64 restatement fed with bufs' OWN upstream
    buffers -> {"stage.output": max(err / bar)}.  rowstat / loss are judged only under a correlation objective."""
    c, p, loss, group = inp["case"], inp["params"], inp["loss"], inp["group"]
    B, E, V, G = c["B"], c["E"], c["V"], c["G"]
    W, bias, g1, g2 = p["ridge_layer.linear.weight"], p["ridge_layer.linear.bias"], p["layer_norm1.weight"], p["layer_norm2.weight"]
    gscale, l2coef, s, lam = _scales(inp, True)
    corr = loss != "mse"
    out = {}

    def put(stage, ref, bars, names):
        for n in names:
            out[f"{stage}.{n}"] = H.ratio(bufs[n], ref[n], bars[n])
    if "ln2" in stages:
        ref = H.ln2(bufs["pooled_raw"], bufs["sumw"], g1, p["layer_norm1.bias"], g2, p["layer_norm2.bias"], inp["keep"], inp["eps"])
        put("ln2", ref, H.ln2_bars(ref, E), ("zhat", "ln2_rstd", "z"))
    rr = None
    if "ridge" in stages or (corr and "loss" in stages):
        rr = ridge(bufs["z"], W, bias, inp["y"], group, lam, pred_for_loss=bufs["pred"])
        rbars = ridge_bars(rr, B, E, V, G)
    if "ridge" in stages:
        put("ridge", rr, rbars, ("pred",))
        if corr:            # the device kept the MSE in loss_aux[0]; loss_terms[0] belongs to the "loss" stage
            mse, l2 = bufs["loss_aux"][0].to(F32), bufs["loss_terms"][1].to(F32)
            out["ridge.loss_terms"] = H.ratio(torch.stack([mse, l2]), rr["loss"][:2], rbars["loss"][:2])
        else:
            out["ridge.loss_terms"] = H.ratio(bufs["loss_terms"], rr["loss"], rbars["loss"])
    if corr and "rowstat" in stages:
        ref = L.rowstat(bufs["pred"], inp["y"], loss)
        bars = L.rowstat_bars(ref, V)
        for n in ("mu_p", "mu_y"):
            out[f"rowstat.{n}"] = H.ratio(bufs[n], ref[n], bars[n])
        ref = L.rowstat(bufs["pred"], inp["y"], loss, mu=(bufs["mu_p"], bufs["mu_y"]))
        bars = L.rowstat_bars(ref, V)
        for n in ("suu", "stt", "sut"):
            out[f"rowstat.{n}"] = H.ratio(bufs[n], ref[n], bars[n])
        cref = L.corr_from_sums(bufs["suu"].to(F64), bufs["stt"].to(F64), bufs["sut"].to(F64))
        out["rowstat.c"] = H.ratio(bufs["c"], cref, 8 * U * cref.abs())
    if corr and "loss" in stages:
        ref = L.loss_terms(bufs["c"], rr["loss"][1], rr["loss"][0])
        bars = L.loss_bars(ref, rbars["loss"])
        out["loss.loss_terms"] = H.ratio(bufs["loss_terms"], ref["loss"], bars["loss"])
        out["loss.loss_aux"] = H.ratio(bufs["loss_aux"], ref["aux"], bars["aux"])
    if "ridge_bwd_w" in stages or "dz" in stages:
        dp, mag = _dpred(bufs["pred"], inp["y"], loss, bufs, B, V, gscale, s, F64)
    if "ridge_bwd_w" in stages:
        ref = ridge_bwd_w(dp, mag, bufs["z"], W, group, l2coef)
        put("ridge_bwd_w", ref, ridge_bwd_w_bars(ref, B, L.C_DP if corr else 2), ("dW", "dbias"))
    if "dz" in stages:
        if B <= 16 and not corr:        # dpred_t_kernel<grouped>'s own bf16 rounding of the fp32 d pred, as H.dz forms it
            dpz = (torch.tensor(gscale, dtype=F32) * (bufs["pred"].to(F32) - inp["y"].to(F32))).to(BF16).to(F64)
        else:
            dpz = dp
        ref = dz(dpz, mag if corr else dpz.abs(), W, inp["keep"], group)
        put("dz", ref, dz_bars(ref, B, V, G, corr), ("dz",))
    if "ln2_bwd" in stages:
        ref = H.ln2_bwd(bufs["dz"], g2, bufs["zhat"], bufs["ln2_rstd"], g1, bufs["pooled_raw"], bufs["sumw"])
        put("ln2_bwd", ref, H.ln2_bwd_bars(ref, B, E), ("dpooled", "dg2", "db2", "dg1", "db1"))
    return out


by_stage = H.by_stage


def single_head_inputs(inp, g):
    """the same batch for ONE head holding (W[g], b[g]): what an ungrouped BrainHead is built from"""
    p = dict(inp["params"])
    p["ridge_layer.linear.weight"] = inp["params"]["ridge_layer.linear.weight"][g].contiguous()
    p["ridge_layer.linear.bias"] = inp["params"]["ridge_layer.linear.bias"][g].contiguous()
    return dict(inp, params=p)
