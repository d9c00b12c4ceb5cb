"""fp64 restatement of the brain head, ONE KERNEL AT A TIME, with derived error bars, inputs and planted bugs.

The head (phantom_vlb_amd/csrc/head.hip) keeps every intermediate in an fp32 buffer on ``BrainHead``, so each kernel
can be checked alone: a stage function here takes what its kernel READS (the device's own upstream buffers, copied to
the host) and returns what the kernel WRITES, in fp64.  The only error left between the two is that one kernel's fp32
accumulation, which is 3-4 orders of magnitude below the bf16 rounding of ``z`` that dominates an end-to-end bar.

Stages (kernels):   pool (head_pool_kernel + head_reduce_kernel), ln2 (head_ln2_kernel), ridge (ridge_fwd_kernel /
ridge_fwd_mfma_kernel + loss_finalize_kernel), ridge_bwd_w (ridge_bwd_w_kernel), dz (dpred_t + skinny wgrad +
head_dz_from16, or ridge_bwd_z + head_dz_reduce), ln2_bwd (head_ln2_bwd_kernel + head_param_grads_kernel), dhidden
(head_dhidden_kernel).  ``run(..., dt=F64)`` chains them with all rounding off: the head as mathematics (``whole``).

Bars.  For an fp32 result that is a sum of terms:   bar = c * 2^-24 * sum|terms| + 2^-22 * |ref|,   sum|terms| from the
fp64 reference, c = the longest chain of additions one output goes through in that kernel (read from the code, spelled
out next to each ``c_*`` below) + 2.  Where a term is itself a product of more than two rounded factors the extra
roundings are added to c (said where it happens); that makes some c larger than the plain chain, never smaller.
Results that go through rsqrtf get a RELATIVE bar with c + 8.  A difference of rounded quantities (x - mean) gets the
absolute errors of its operands, so that a bar never relies on the result being far from zero.  bf16 outputs (z, dh)
get 2^-8 |ref| (half a bf16 ulp) on top of the fp32 bar of the value before rounding.  Nothing here is fitted to a
measurement; tests print max(err / bar) and assert <= 1.
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

EPS, LAMBDA = 1e-5, 1e-3
STAGES = ("pool", "ln2", "ridge", "ridge_bwd_w", "dz", "ln2_bwd", "dhidden")


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------- dispatch
def pool_ni(E):
    """template argument of head_pool_kernel (vlb_head_fwd)"""
    ni = cdiv(E, 512)
    return 1 if ni <= 1 else 2 if ni <= 2 else 4 if ni <= 4 else 8 if ni <= 8 else 16


def wgrad_splits(V):
    """vlb_wgrad_splits"""
    return 32 if V >= 4096 else max(1, cdiv(V, 256))


def mfma_ridge(B, E):
    return B <= 16 and E % 128 == 0 and E <= 4096


def dispatch(B, E):
    """Kernels a head step of (B, E) runs: the branch conditions of vlb_head_fwd / head_fwd_tail / head_bwd_params."""
    k = {f"head_pool_kernel<{pool_ni(E)}>", "head_reduce_kernel", "head_ln2_kernel", "loss_finalize_kernel",
         "ridge_bwd_w_kernel", f"ridge_bwd_w:b0_passes={cdiv(B, 8)}", "head_ln2_bwd_kernel", "head_param_grads_kernel",
         "head_dhidden_kernel"}
    k.add(f"ridge_fwd_mfma_kernel<{E // 128}>" if mfma_ridge(B, E) else "ridge_fwd_kernel")
    if B <= 16 and E % 8 == 0:
        k |= {"dpred_t_kernel", "wgrad_mfma_kernel", "head_dz_from16_kernel"}
    else:
        k |= {"ridge_bwd_z_kernel", "head_dz_reduce_kernel"}
    return k


# ---------------------------------------------------------------------------------------------------- cases
# Cases whose seeded inputs are drawn again (the seed moves by 7919 * n): with the first draw the bf16 roundings alone
# put the head more than E2E_FORMAT_SHARE of an end-to-end bar away from the head as mathematics (see "end to end" below;
# a property of the inputs and the number formats, computed in fp64 without the code under test).  n is the first that
# does not.
RESEED = {"pool-E512": 1, "pool-E520": 3, "pool-E1024": 1, "pool-E2568": 1, "pool-E4104": 2, "tok-S31": 1, "tok-S128": 1,
          "clips-B1": 1, "clips-B16": 1, "targets-V5": 2, "targets-V300": 1}


def _case(id, E, S, B, V, mask="lead", drop=False, scales=(1.0, 1.0), lens=None, zero_clip=False, expect=(), stages=STAGES):
    return dict(id=id, E=E, S=S, B=B, V=V, mask=mask, drop=drop, scales=scales, lens=lens, zero_clip=zero_clip,
                expect=tuple(expect), stages=tuple(stages), reseed=RESEED.get(id, 0))


# What a case is there for is written out per case, as literals, NOT computed from (B, E): the tests assert
# expect <= dispatch(B, E), so a slip in ``dispatch`` or in a case's shape fails.  Both sides are restatements in Python:
# the library does not report which kernels it launched, so a planner change in head.hip is caught only through
# test_cpu_head_emul.test_dispatch_restates_the_planner, which looks for the branch conditions in the source text.
_BIG = ("ridge_fwd_kernel", "ridge_bwd_z_kernel", "head_dz_reduce_kernel")
_SKINNY = ("dpred_t_kernel", "wgrad_mfma_kernel", "head_dz_from16_kernel")

CASES = []
# pool instantiations and column guards: B=2, S=70 (a 6-token tail block), V=48
for _E, _pool, _fwd in ((264, "head_pool_kernel<1>", "ridge_fwd_kernel"),
                          (512, "head_pool_kernel<1>", "ridge_fwd_mfma_kernel<4>"),
                          (520, "head_pool_kernel<2>", "ridge_fwd_kernel"),
                          (1024, "head_pool_kernel<2>", "ridge_fwd_mfma_kernel<8>"),
                          (1536, "head_pool_kernel<4>", "ridge_fwd_mfma_kernel<12>"),
                          (2048, "head_pool_kernel<4>", "ridge_fwd_mfma_kernel<16>"),
                          (2568, "head_pool_kernel<8>", "ridge_fwd_kernel"),
                          (4096, "head_pool_kernel<8>", "ridge_fwd_mfma_kernel<32>"),
                          (4104, "head_pool_kernel<16>", "ridge_fwd_kernel"),
                          (8192, "head_pool_kernel<16>", "ridge_fwd_kernel")):
    CASES.append(_case(f"pool-E{_E}", _E, 70, 2, 48, expect=(_pool, _fwd) + _SKINNY))
# token edges: E=512, V=48, B=3, one clip all zero.  S=128: every live subset; the others: a dead leading span of S//3
# tokens (none at S=1, where the all-zero clip is the only dead token)
for _S in (1, 31, 32, 33, 128):
    CASES.append(_case(f"tok-S{_S}", 512, _S, 3, 48, mask="subsets" if _S == 128 else "lead", zero_clip=True,
                       expect=("head_pool_kernel<1>", "ridge_fwd_mfma_kernel<4>")))
# clip-count edges: E=1024, V=40, S=33.  ridge_bwd_w_kernel takes 8 clips per b0 pass: 1, 1, 2, 2, 3 (8+8+1), 4 (8+8+8+1)
for _B, _passes, _path in ((1, "ridge_bwd_w:b0_passes=1", ("ridge_fwd_mfma_kernel<8>",) + _SKINNY),
                           (8, "ridge_bwd_w:b0_passes=1", ("ridge_fwd_mfma_kernel<8>",) + _SKINNY),
                           (9, "ridge_bwd_w:b0_passes=2", ("ridge_fwd_mfma_kernel<8>",) + _SKINNY),
                           (16, "ridge_bwd_w:b0_passes=2", ("ridge_fwd_mfma_kernel<8>",) + _SKINNY),
                           (17, "ridge_bwd_w:b0_passes=3", _BIG),
                           (25, "ridge_bwd_w:b0_passes=4", _BIG)):
    CASES.append(_case(f"clips-B{_B}", 1024, 33, _B, 40, expect=(_passes,) + _path))
CASES.append(_case("clips-B17-drop", 1024, 33, 17, 40, drop=True, expect=("ridge_bwd_w:b0_passes=3",) + _BIG))
# target-count edges: E=512, B=3, S=33
for _V in (1, 5, 16, 17, 300):
    CASES.append(_case(f"targets-V{_V}", 512, 33, 3, _V, expect=("ridge_fwd_mfma_kernel<4>",) + _SKINNY))
CASES.append(_case("targets-V32784", 128, 32, 2, 32784, expect=("ridge_fwd_mfma_kernel<1>",) + _SKINNY))
for _V in (5, 300):
    CASES.append(_case(f"targets-B17-V{_V}", 512, 33, 17, _V, expect=_BIG))
# scales and dropout on one MFMA-path shape and one B=17 shape
CASES.append(_case("scales-mfma", 1024, 33, 9, 40, drop=True, scales=(0.25, 0.5),
                   expect=("ridge_fwd_mfma_kernel<8>", "ridge_bwd_w:b0_passes=2") + _SKINNY))
CASES.append(_case("scales-B17", 1024, 33, 17, 40, drop=True, scales=(0.25, 0.5), expect=_BIG))
# packed layout: each clip's dead leading span is a third of ITS length, so the one-row clip keeps its one token live
CASES.append(_case("packed", 1536, 70, 3, 48, lens=(70, 1, 37), expect=("head_pool_kernel<4>", "ridge_fwd_mfma_kernel<12>")))
# every ridge_fwd_mfma_kernel<KSTEPS>: ridge and dz only (KSTEPS is the sweep variable itself)
KSWEEP = [_case(f"ksteps-{_k}", 128 * _k, 32, 4, 33, stages=("ridge", "dz"),
                expect=(f"ridge_fwd_mfma_kernel<{_k}>",) + _SKINNY) for _k in range(1, 33)]
BY_ID = {c["id"]: c for c in CASES + KSWEEP}


# ---------------------------------------------------------------------------------------------------- inputs
def subsets_mask_live(S=128):
    """[S] bool: for S = 128 the four tokens of a wave, 32*blk + wave + 8q, take all 16 live/dead patterns across the
    32 (block, wave) slots (slot k = 8*blk + wave gets pattern k % 16, bit q = token q live)."""
    assert S == 128
    live = torch.zeros(S, dtype=torch.bool)
    for blk in range(4):
        for wave in range(8):
            pat = (8 * blk + wave) % 16
            for q in range(4):
                live[32 * blk + wave + 8 * q] = bool((pat >> q) & 1)
    return live


def wave_patterns(live_row):
    """the set of 4-bit live patterns the (block, wave) slots of one clip's mask row show"""
    S = live_row.numel()
    out = set()
    for blk in range(cdiv(S, 32)):
        for wave in range(8):
            out.add(sum(int(32 * blk + wave + 8 * q < S and bool(live_row[32 * blk + wave + 8 * q])) << q for q in range(4)))
    return out


def hrf_like_weights(B, S, gen):
    """both signs, in the Glover HRF's range (peak ~ +0.12, undershoot ~ -0.03)"""
    w = torch.rand(B, S, generator=gen) * 0.115 + 0.005
    neg = (torch.arange(S) + torch.arange(B)[:, None]) % 5 == 2        # every fifth token in the undershoot
    return torch.where(neg, -0.25 * w, w)


def make_mask(kind, B, S, gen, zero_clip=False, lens=None):
    w = hrf_like_weights(B, S, gen)
    if kind == "subsets":
        base = subsets_mask_live(S)
        w = torch.where(base, w, torch.zeros(()))            # every clip: all 16 patterns (the weights differ per clip)
    else:
        for b in range(B):                                   # dead leading span (prompt / instruction): a third of the clip
            n = S if lens is None else lens[b]
            w[b, : n // 3] = 0
            w[b, n:] = 0
        if S > 4:
            w[0, S // 2] = 0
    if B > 1:
        w[B - 1] *= 2.0 ** -5                                # a faint clip: pooled variance small enough for LN2's eps to matter
    if zero_clip and B > 1:
        w[1] = 0
    return w


def keep_scale(B, E, p, gen):
    """values in {0, 1/(1-p)}"""
    return (torch.rand(B, E, generator=gen) > p).float() / (1.0 - p)


@functools.lru_cache(maxsize=None)
def inputs_for(case_id):
    """the inputs of a named case, made once and shared (treat as read-only)"""
    return make_inputs(BY_ID[case_id])


def make_inputs(case, seed=None):
    """Seeded CPU tensors for a case.  hidden is bf16 [B,S,E] with a per-channel offset and two outlier channels of
    magnitude ~50 (as Mistral hidden states have) and one live token scaled by 2^-6 (a row whose variance is small
    enough for eps to matter).  Parameters are bf16-valued with non-trivial LN affines."""
    E, S, B, V = case["E"], case["S"], case["B"], case["V"]
    gen = torch.Generator().manual_seed((E * 1000003 + S * 10007 + B * 101 + V + 7919 * case["reseed"]) % (2 ** 31) if seed is None else seed)
    off = 0.5 * torch.randn(E, generator=gen)
    hidden = torch.randn(B, S, E, generator=gen) * 1.5 + off
    hidden[..., 3 % E] += 50.0
    hidden[..., (5 * E // 8) | 1] -= 45.0
    wmask = make_mask(case["mask"], B, S, gen, case["zero_clip"], case["lens"])
    live0 = torch.nonzero(wmask[0] != 0).flatten()
    if live0.numel():
        hidden[0, int(live0[0])] *= 2.0 ** -6
    params = {"layer_norm1.weight": 1 + 0.1 * torch.randn(E, generator=gen), "layer_norm1.bias": 0.1 * torch.randn(E, generator=gen),
              "layer_norm2.weight": 1 + 0.1 * torch.randn(E, generator=gen), "layer_norm2.bias": 0.1 * torch.randn(E, generator=gen),
              "ridge_layer.linear.weight": torch.randn(V, E, generator=gen) / math.sqrt(E),
              "ridge_layer.linear.bias": 0.1 * torch.randn(V, generator=gen)}
    params = {k: v.to(BF16).float() for k, v in params.items()}
    y = torch.randn(B, V, generator=gen)
    keep = keep_scale(B, E, 0.1, gen) if case["drop"] else None
    return dict(case=case, hidden=hidden.to(BF16), wmask=wmask, params=params, y=y, keep=keep, eps=EPS, lam=LAMBDA,
                loss_scale=case["scales"][0], l2_scale=case["scales"][1])


def host_scales(B, V, lam, loss_scale, l2_scale, swap=False):
    """(gscale, l2coef) as head_bwd_params forms them, in fp32 and in its order of operations"""
    f = np.float32
    if swap:
        loss_scale, l2_scale = l2_scale, loss_scale
    gscale = f(loss_scale) * f(2.0) / (f(B) * f(V))
    l2coef = f(l2_scale) * f(2.0) * f(lam)
    return float(gscale), float(l2coef)


# ---------------------------------------------------------------------------------------------------- stages
def pool(hidden, wmask, eps, stats=None, dt=F64, bug=None):
    """head_pool_kernel + head_reduce_kernel.  -> mu, rstd [B,S] (meaningful at live tokens), pooled_raw [B,E], sumw [B].
    ``stats`` = (mu, rstd) to pool with (the device's own, so that pooled_raw is judged on its accumulation alone)."""
    x, w = hidden.to(dt), wmask.to(dt).clone()
    E = x.shape[-1]
    cols = torch.ones(E, dtype=dt)
    if bug == "drop_chunk":
        cols[8:16] = 0
    mu = (x * cols).sum(-1) / E
    d = x - mu[..., None]
    var = (d * d * cols).sum(-1) / E
    rstd = (var + (0.0 if bug == "pool_no_eps" else eps)).rsqrt()
    if bug == "drop_token":
        b, s = [int(v) for v in torch.nonzero(w != 0)[-1]]
        w[b, s] = 0
    mu_u, rstd_u = (mu, rstd) if stats is None else (stats[0].to(dt), stats[1].to(dt))
    terms = (w * rstd_u)[..., None] * (x - mu_u[..., None]) * cols
    return dict(mu=mu, rstd=rstd, pooled_raw=terms.sum(1), sumw=w.sum(1),
                mag_mu=x.abs().sum(-1) / E, mag_raw=terms.abs().sum(1), mag_sumw=w.abs().sum(1))


def pool_bars(ref, E, S):
    ni, nblk = pool_ni(E), cdiv(S, 32)
    c_stat = 8 * ni + 6 + 2                   # a lane adds 8*NI values, wave_sum adds 6 levels
    c_acc = 4 + 3 + nblk + 2 + 1              # 4 tokens per wave, 3 tree levels, nblk slabs; the term w*rstd*(x-mu) is 3 roundings
    return dict(mu=c_stat * U * ref["mag_mu"] + R * ref["mu"].abs(),
                rstd=((c_stat + 8) * U + R) * ref["rstd"],
                pooled_raw=c_acc * U * ref["mag_raw"] + R * ref["pooled_raw"].abs(),
                sumw=(4 + 3 + nblk + 2) * U * ref["mag_sumw"] + R * ref["sumw"].abs())


def ln2(pooled_raw, sumw, g1, b1, g2, b2, keep, eps, dt=F64, bug=None):
    """head_ln2_kernel.  -> zhat [B,E], ln2_rstd [B], z [B,E] UNROUNDED (the bar carries the bf16 rounding)."""
    raw, sw = pooled_raw.to(dt), sumw.to(dt)[:, None]
    g1, b1, g2, b2 = (t.to(dt) for t in (g1, b1, g2, b2))
    E = raw.shape[-1]
    aff = torch.zeros_like(raw) if bug == "no_b1" else b1 * sw
    pv = g1 * raw + aff
    mag_pv = (g1 * raw).abs() + aff.abs()
    mean = pv.sum(-1, keepdim=True) / E
    d = pv - mean
    var = (d * d).sum(-1) / E
    rstd = (var + (0.0 if bug == "ln2_no_eps" else eps)).rsqrt()
    zhat = d * rstd[:, None]
    z = zhat * g2 + b2
    k = torch.ones_like(z) if keep is None or bug == "fwd_no_keep" else keep.to(dt)
    return dict(zhat=zhat, ln2_rstd=rstd, z=z * k, mag_pv=mag_pv, d=d, keep=k, g2=g2, b2=b2)


def ln2_bars(ref, E):
    c = cdiv(E, 1024) + 6 + 16 + 2            # block_sum: ceil(E/1024) per thread, 6 wave levels, 16 wave partials
    mag_pv, d, rstd, zhat = ref["mag_pv"], ref["d"], ref["ln2_rstd"][:, None], ref["zhat"]
    bar_d = 3 * U * mag_pv + c * U * mag_pv.sum(-1, keepdim=True) / E + U * d.abs()       # pv: 3 roundings; the mean; the subtraction
    # var = mean(d^2): each d carries pv's rounding, 2*sum|d|*3U*mag_pv / sum d^2 relative; rstd takes half of it
    rel_rstd = (c + 8) * U + R + 3 * U * (d.abs() * mag_pv).sum(-1, keepdim=True) / (d * d).sum(-1, keepdim=True).clamp_min(1e-300)
    bar_zhat = rstd * bar_d + (rel_rstd + U + R) * zhat.abs()
    bar_zz = (ref["g2"].abs() * bar_zhat + 2 * U * ((zhat * ref["g2"]).abs() + ref["b2"].abs())) * ref["keep"] + U * ref["z"].abs()
    return dict(zhat=bar_zhat, ln2_rstd=rel_rstd[:, 0] * ref["ln2_rstd"], z=HB * ref["z"].abs() + bar_zz)


def ridge(z, W, bias, y, lam, pred_for_loss=None, dt=F64, bug=None):
    """ridge forward + loss_finalize_kernel.  -> pred [B,V], loss = (mse, l2, total).  The squared error is taken from
    ``pred_for_loss`` (the device's own pred: the kernel squares what it wrote) when that is given."""
    z, W, bias, y = z.to(dt), W.to(dt), bias.to(dt), y.to(dt)
    B, E = z.shape
    if bug == "lose_quarter":
        z = z.clone()
        z[:, E // 4: E // 2] = 0
    pred = z @ W.t() + bias
    mag = z.abs() @ W.abs().t() + bias.abs()
    d = (pred if pred_for_loss is None else pred_for_loss.to(dt)) - y
    mse = (d * d).sum() / (B * W.shape[0])
    l2 = lam * (W * W).sum()
    return dict(pred=pred, mag_pred=mag, loss=torch.stack([mse, l2, mse + l2]))


def ridge_bars(ref, B, E, V):
    if mfma_ridge(B, E):
        ks, ntiles = E // 128, cdiv(V, 16)
        tpb = cdiv(ntiles, min(ntiles, 2048))          # row tiles a persistent block takes
        c_pred = 32 * ks + 3 + 1 + 2                   # KSTEPS MFMAs of 32 products, 3 K-quarters, the bias
        c_mse = 4 * tpb + 6 + 3 + 2                    # 4 rows per lane and tile, wave_sum, 4 waves
        c_w2 = 8 * ks * tpb + 6 + 3 + 2
    else:
        nch = cdiv(E, 512)
        c_pred = 8 * nch + 6 + 1 + 2                   # 8 products per 512-column step, wave_sum, the bias
        c_mse = 4 * B + 3 + 2                          # lane 0: 4 rows x B clips; 4 waves
        c_w2 = 8 * nch * 4 + 6 + 3 + 2
    mse, l2, tot = ref["loss"]
    # the per-block partials are fp32, the sum over blocks fp64; d = pred - y and its square are two roundings (the + 2);
    # 1/(B*V) is formed in fp32 (2U more)
    bar_mse, bar_l2 = ((c_mse + 2) * U + R) * mse, (c_w2 * U + R) * l2
    return dict(pred=c_pred * U * ref["mag_pred"] + R * ref["pred"].abs(), loss=torch.stack([bar_mse, bar_l2, bar_mse + bar_l2 + R * tot]))


def ridge_bwd_w(pred, y, z, W, gscale, l2coef, dt=F64, bug=None):
    """ridge_bwd_w_kernel.  -> dW [V,E] = l2coef*W + sum_b dp[b,v] z[b,e], dbias [V] = sum_b dp[b,v]."""
    pred, y, z, W = pred.to(dt), y.to(dt), z.to(dt), W.to(dt)
    dp = gscale * (pred - y)
    seed = torch.zeros_like(W) if bug == "no_l2_seed" else l2coef * W
    dpb = dp[:8] if bug == "dbias_first8" else dp
    return dict(dW=seed + dp.t() @ z, dbias=dpb.sum(0), mag_dW=seed.abs() + dp.abs().t() @ z.abs(), mag_dbias=dp.abs().sum(0))


def ridge_bwd_w_bars(ref, B):
    c_dW = B + 1 + 2 + 2                      # B terms onto the seed; dp = gscale*(pred-y) brings two more roundings than a plain product
    c_db = B + cdiv(B, 8) + 2 + 2             # 8 per pass plus the read-modify-write per pass
    return dict(dW=c_dW * U * ref["mag_dW"] + R * ref["dW"].abs(), dbias=c_db * U * ref["mag_dbias"] + R * ref["dbias"].abs())


def dz(pred, y, W, keep, gscale, round_dp_bf16, dt=F64, bug=None):
    """dz [B,E] = keep * sum_v dp[b,v] W[v,e].  B <= 16 (``round_dp_bf16``): dp is rounded to bf16 for the MFMA
    (dpred_t_kernel; formed in fp32 exactly as there); B > 16 (ridge_bwd_z_kernel): it is not."""
    W = W.to(dt)
    if round_dp_bf16 and bug != "dz_unrounded":
        dp = (torch.tensor(gscale, dtype=F32) * (pred.to(F32) - y.to(F32))).to(BF16).to(dt)
    else:
        dp = gscale * (pred.to(dt) - y.to(dt))
    k = torch.ones(pred.shape[0], W.shape[1], dtype=dt) if keep is None or bug == "dz_no_keep" else keep.to(dt)
    return dict(dz=(dp @ W) * k, mag=(dp.abs() @ W.abs()) * k)


def dz_bars(ref, B, V):
    if B <= 16:
        sp = wgrad_splits(V)
        c = cdiv(V, sp) + sp + 2 + 1          # a split's rows through the MFMA accumulator, the splits, keep
    else:
        c = cdiv(cdiv(V, 32), 4) + 3 + 32 + 2 + 3     # rows per wave, 4 waves, 32 splits; dp (2 more roundings) and keep
    return dict(dz=c * U * ref["mag"] + R * ref["dz"].abs())


def ln2_bwd(dz_, g2, zhat, ln2_rstd, g1, pooled_raw, sumw, dt=F64):
    """head_ln2_bwd_kernel + head_param_grads_kernel.  -> dpooled = d loss / d pooled_raw (dp * g1), dg2, db2, dg1, db1."""
    dz_, g2, zhat, g1, raw = (t.to(dt) for t in (dz_, g2, zhat, g1, pooled_raw))
    rstd, sw = ln2_rstd.to(dt)[:, None], sumw.to(dt)[:, None]
    E = dz_.shape[-1]
    g = dz_ * g2
    m1 = g.sum(-1, keepdim=True) / E
    m2 = (g * zhat).sum(-1, keepdim=True) / E
    dp = rstd * (g - m1 - zhat * m2)
    return dict(dpooled=dp * g1, dg2=(dz_ * zhat).sum(0), db2=dz_.sum(0), dg1=(dp * raw).sum(0), db1=(dp * sw).sum(0),
                g=g, m1=m1, m2=m2, zhat=zhat, rstd=rstd, dp=dp, g1=g1, raw=raw, sw=sw, dz=dz_)


def _ln_bwd_bar(g, m1, m2, xh, rstd, dp, c, k):
    """|error| of rstd*(g - m1 - xh*m2): the two block / wave means at chain c, the operands' own roundings (k)"""
    E = g.shape[-1]
    mg, mgx = g.abs().sum(-1, keepdim=True) / E, (g * xh).abs().sum(-1, keepdim=True) / E
    return rstd * U * (c * (mg + xh.abs() * mgx) + k * (g.abs() + m1.abs() + (xh * m2).abs())) + R * dp.abs()


def ln2_bwd_bars(ref, B, E):
    c = cdiv(E, 1024) + 6 + 16 + 2 + 1        # block_sum; g*zhat is a product of a product
    bar_dp = _ln_bwd_bar(ref["g"], ref["m1"], ref["m2"], ref["zhat"], ref["rstd"], ref["dp"], c, 4)
    cb = B + 2                                # head_param_grads_kernel: B terms in order
    dz_, dp = ref["dz"], ref["dp"]
    return dict(dpooled=ref["g1"].abs() * bar_dp + U * ref["dpooled"].abs(),
                dg2=cb * U * (dz_ * ref["zhat"]).abs().sum(0) + R * ref["dg2"].abs(),
                db2=cb * U * dz_.abs().sum(0) + R * ref["db2"].abs(),
                # the kernel multiplies its own dp (off by bar_dp) with pooled_raw / sumw
                dg1=(bar_dp * ref["raw"].abs()).sum(0) + cb * U * (dp * ref["raw"]).abs().sum(0) + R * ref["dg1"].abs(),
                db1=(bar_dp * ref["sw"].abs()).sum(0) + cb * U * (dp * ref["sw"]).abs().sum(0) + R * ref["db1"].abs())


def dhidden(hidden, wmask, mu, rstd, draw, dt=F64, bug=None):
    """head_dhidden_kernel.  -> dh [B,S,E] UNROUNDED; zero-weight rows are exactly 0."""
    x, w, mu, rstd, u = hidden.to(dt), wmask.to(dt)[..., None], mu.to(dt)[..., None], rstd.to(dt)[..., None], draw.to(dt)[:, None, :]
    E = x.shape[-1]
    xh = (x - mu) * rstd
    g = w * u
    m1 = g.sum(-1, keepdim=True) / E
    m2 = (g * xh).sum(-1, keepdim=True) / E
    dh = rstd * (g - m1 - ((x - mu) if bug == "m2_no_rstd" else xh) * m2)
    live = (wmask != 0)[..., None]
    return dict(dh=torch.where(live, dh, torch.zeros((), dtype=dt)), g=g * live, m1=m1 * live, m2=m2 * live, xh=xh * live,
                rstd=rstd * live)


def dhidden_bars(ref, E):
    c = 8 * cdiv(E, 512) + 6 + 2 + 2          # 8 per 512-column step, wave_sum; g*(x-mu)*rstd is three products deep
    bar32 = _ln_bwd_bar(ref["g"], ref["m1"], ref["m2"], ref["xh"], ref["rstd"], ref["dh"], c, 6)
    return dict(dh=HB * ref["dh"].abs() + bar32)


# ---------------------------------------------------------------------------------------------------- the chain
POOL_BUGS = ("drop_token", "drop_chunk", "pool_no_eps")
BUGS = {  # planted bug -> the stage whose bar must reject it
    "drop_token": "pool", "drop_chunk": "pool", "pool_no_eps": "pool", "ln2_no_eps": "ln2", "no_b1": "ln2",
    "fwd_no_keep": "ln2", "dz_no_keep": "dz", "lose_quarter": "ridge", "dbias_first8": "ridge_bwd_w",
    "no_l2_seed": "ridge_bwd_w", "swap_scales": "ridge_bwd_w", "dz_unrounded": "dz", "m2_no_rstd": "dhidden"}


def run(inp, dt=F64, device_like=False, bug=None):
    """All stages chained on their own outputs -> the buffers ``BrainHead`` holds after forward + backward.
    ``device_like``: z, dh (and dp on the B <= 16 path) rounded to bf16 and the scales formed in fp32, as the kernels do.
    dt = F64 with device_like off is the head as mathematics; dt = F32 is an honest fp32 computation in torch's own
    summation order (pairwise / vectorised, not the kernels' order)."""
    p, B, V = inp["params"], inp["case"]["B"], inp["case"]["V"]
    W, g1, g2 = p["ridge_layer.linear.weight"], p["layer_norm1.weight"], p["layer_norm2.weight"]
    po = pool(inp["hidden"], inp["wmask"], inp["eps"], dt=dt, bug=bug)
    l2o = ln2(po["pooled_raw"], po["sumw"], g1, p["layer_norm1.bias"], g2, p["layer_norm2.bias"], inp["keep"], inp["eps"], dt=dt, bug=bug)
    z = l2o["z"].to(BF16).to(dt) if device_like else l2o["z"]
    lam = float(np.float32(inp["lam"])) if device_like else inp["lam"]
    ro = ridge(z, W, p["ridge_layer.linear.bias"], inp["y"], lam, dt=dt, bug=bug)
    if device_like:
        gscale, l2coef = host_scales(B, V, inp["lam"], inp["loss_scale"], inp["l2_scale"], swap=bug == "swap_scales")
    else:
        gscale, l2coef = inp["loss_scale"] * 2.0 / (B * V), inp["l2_scale"] * 2.0 * inp["lam"]
    wo = ridge_bwd_w(ro["pred"], inp["y"], z, W, gscale, l2coef, dt=dt, bug=bug)
    do = dz(ro["pred"], inp["y"], W, inp["keep"], gscale, device_like and B <= 16, dt=dt, bug=bug)
    bo = ln2_bwd(do["dz"], g2, l2o["zhat"], l2o["ln2_rstd"], g1, po["pooled_raw"], po["sumw"], dt=dt)
    ho = dhidden(inp["hidden"], inp["wmask"], po["mu"], po["rstd"], bo["dpooled"], dt=dt, bug=bug)
    dh = ho["dh"].to(BF16).to(dt) if device_like else ho["dh"]
    return dict(mu=po["mu"], rstd=po["rstd"], pooled_raw=po["pooled_raw"], sumw=po["sumw"], zhat=l2o["zhat"],
                ln2_rstd=l2o["ln2_rstd"], z=z, pred=ro["pred"], loss_terms=ro["loss"], dW=wo["dW"], dbias=wo["dbias"],
                dz=do["dz"], dpooled=bo["dpooled"], dg2=bo["dg2"], db2=bo["db2"], dg1=bo["dg1"], db1=bo["db1"], dh=dh)


def whole(inp):
    """the head as mathematics: fp64, nothing rounded"""
    return run(inp, dt=F64, device_like=False)


GRAD_KEYS = {"layer_norm1.weight": "dg1", "layer_norm1.bias": "db1", "layer_norm2.weight": "dg2", "layer_norm2.bias": "db2",
             "ridge_layer.linear.weight": "dW", "ridge_layer.linear.bias": "dbias"}


# ---------------------------------------------------------------------------------------------------- the check
def ratio(got, ref, bar):
    """max |got - ref| / bar (0 where both vanish, inf where only the bar does, inf for a NaN)"""
    err = (got.to(F64) - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bar.clamp_min(1e-300))
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


def check_stages(bufs, inp, stages=STAGES):
    """Every stage of ``bufs`` (the buffers of one forward + backward, host tensors named as in ``run``) against its
    fp64 restatement FED WITH bufs' OWN upstream buffers.  -> {"stage.output": max(err / bar)}."""
    c, p = inp["case"], inp["params"]
    B, S, E, V = c["B"], c["S"], c["E"], c["V"]
    W, g1, g2 = p["ridge_layer.linear.weight"], p["layer_norm1.weight"], p["layer_norm2.weight"]
    live = inp["wmask"] != 0
    zero = torch.zeros((), dtype=F64)
    mu_d, rstd_d = torch.where(live, bufs["mu"].to(F64), zero), torch.where(live, bufs["rstd"].to(F64), zero)
    gscale, l2coef = host_scales(B, V, inp["lam"], inp["loss_scale"], inp["l2_scale"])
    out = {}

    def put(stage, ref, bars, names):
        for n in names:
            out[f"{stage}.{n}"] = ratio(bufs[n], ref[n], bars[n])
    if "pool" in stages:
        ref = pool(inp["hidden"], inp["wmask"], inp["eps"], stats=(mu_d, rstd_d))
        bars = pool_bars(ref, E, S)
        out["pool.mu"] = ratio(bufs["mu"][live], ref["mu"][live], bars["mu"][live])
        out["pool.rstd"] = ratio(bufs["rstd"][live], ref["rstd"][live], bars["rstd"][live])
        put("pool", ref, bars, ("pooled_raw", "sumw"))
    if "ln2" in stages:
        ref = ln2(bufs["pooled_raw"], bufs["sumw"], g1, p["layer_norm1.bias"], g2, p["layer_norm2.bias"], inp["keep"], inp["eps"])
        put("ln2", ref, ln2_bars(ref, E), ("zhat", "ln2_rstd", "z"))
    if "ridge" in stages:
        ref = ridge(bufs["z"], W, p["ridge_layer.linear.bias"], inp["y"], float(np.float32(inp["lam"])), pred_for_loss=bufs["pred"])
        bars = ridge_bars(ref, B, E, V)
        put("ridge", ref, bars, ("pred",))
        out["ridge.loss_terms"] = ratio(bufs["loss_terms"], ref["loss"], bars["loss"])
    if "ridge_bwd_w" in stages:
        ref = ridge_bwd_w(bufs["pred"], inp["y"], bufs["z"], W, gscale, l2coef)
        put("ridge_bwd_w", ref, ridge_bwd_w_bars(ref, B), ("dW", "dbias"))
    if "dz" in stages:
        ref = dz(bufs["pred"], inp["y"], W, inp["keep"], gscale, B <= 16)
        put("dz", ref, dz_bars(ref, B, V), ("dz",))
    if "ln2_bwd" in stages:
        ref = ln2_bwd(bufs["dz"], g2, bufs["zhat"], bufs["ln2_rstd"], g1, bufs["pooled_raw"], bufs["sumw"])
        put("ln2_bwd", ref, ln2_bwd_bars(ref, B, E), ("dpooled", "dg2", "db2", "dg1", "db1"))
    if "dhidden" in stages:
        ref = dhidden(inp["hidden"], inp["wmask"], mu_d, rstd_d, bufs["dpooled"])
        put("dhidden", ref, dhidden_bars(ref, E), ("dh",))
        dead = bufs["dh"][~live]
        if dead.numel() and bool((dead != 0).any()):
            out["dhidden.dh"] = float("inf")               # zero-weight rows are exactly 0
    return out


def by_stage(ratios):
    """{"stage.output": r} -> {"stage": max r}"""
    out = {}
    for k, v in ratios.items():
        s = k.split(".")[0]
        out[s] = max(out.get(s, 0.0), v)
    return out


# ---------------------------------------------------------------------------------------------------- end to end
# The bars test_head_fwd_bwd holds the whole head to (max-norm relative error), unchanged, against ``whole``.  They see
# only gross errors; what they add to the stage checks is that two stages cannot be wrong in compensating ways.  Most of
# such a bar is used up by the number formats alone: the bf16 roundings of z, d pred and d hidden move the results of an
# otherwise exact fp64 computation (``format_deviation``: no code under test involved) by several 1e-3, and with outlier
# channels the largest entry of d layer_norm1.weight is a cancellation residual of LN2's backward that they can move by
# more than 1e-2.  The bar is not widened for that; the INPUTS are chosen (``RESEED``) so that the format deviation stays
# within E2E_FORMAT_SHARE of every bar at every case, which test_cpu_head_emul asserts.  The rest of the bar is for the
# device's fp32 accumulation and the bf16 roundings it flips, 2^-15 of the format deviation per rounding.
E2E_BARS = dict(pred=6e-3, l2=1e-5, total=2e-3, dg1=1e-2, db1=1e-2, dg2=1e-2, db2=1e-2, dW=1e-2, dbias=1e-2, dh=1.5e-2)
E2E_FORMAT_SHARE = 0.7


def _e2e_errors(bufs, ref):
    def rel(a, r):
        return float((a.to(F64) - r).abs().max() / (r.abs().max() + 1e-12))
    out = {k: rel(bufs[k], ref[k]) for k in ("pred", "dg1", "db1", "dg2", "db2", "dW", "dbias", "dh")}
    out["l2"] = rel(bufs["loss_terms"][1], ref["loss_terms"][1])
    out["total"] = rel(bufs["loss_terms"][2], ref["loss_terms"][2])
    return out


def end_to_end(bufs, inp):
    """-> {name: max|got - ref| / max|ref|} of one forward + backward against ``whole(inp)``; each is held to E2E_BARS"""
    return _e2e_errors(bufs, whole(inp))


def format_deviation(inp):
    """the same figures for fp64 arithmetic with only the bf16 roundings (and fp32 scales) of the device"""
    return _e2e_errors(run(inp, dt=F64, device_like=True), whole(inp))
