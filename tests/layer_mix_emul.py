"""fp64 restatement of the three stages ``readout_layers`` adds to the brain head, with derived error bars, seeded inputs
and planted bugs (the head's other stages: head_emul.py, whose rule for bars is followed here).

Stages (kernels of phantom_vlb_amd/csrc/head.hip):
  mix_fwd   head_mix_fwd_kernel                        alpha = softmax(a),  pooled = sum_k alpha_k P_k
  mix_bwd   head_mix_bwd_kernel + head_mix_da_kernel   draw_stack[k] = alpha_k draw,  d_a_k = alpha_k (dal_k - sum_j alpha_j dal_j),
                                                       dal_k = <draw, P_k>
  dhidden   head_dhidden_kernel (write)                dx = value on live rows, 0 on rows with w = 0
            head_dhidden_acc_kernel (accumulate)       dx = bf16(float(dx) + value) on live rows, other rows untouched

Bars, after the rule at the top of head_emul.py: an fp32 sum of terms gets c * 2^-24 * sum|terms| + 2^-22 * |ref| with c =
the longest chain of additions read from the kernel + 2, more where a term is itself several roundings deep (said where);
a result through a transcendental gets a relative bar with c + 8; a difference of rounded quantities gets the absolute
errors of its operands; a bf16 output adds 2^-8 |ref|.  Accumulate mode: the bar of the value (fp32) plus half a bf16 ulp of
the sum (plus the fp32 add itself).  Nothing is fitted to a measurement.
"""
from __future__ import annotations

import torch

import head_emul as H
from head_emul import BF16, F32, F64, HB, R, U, cdiv

MIX_CHUNK = 1024          # elements of [B,E] per block of head_mix_bwd_kernel
EPS = H.EPS


# ---------------------------------------------------------------------------------------------------- inputs
def mix_inputs(K, B, E, seed=0):
    """P_stack fp32 [K,B,E] (pooled vectors: a per-layer scale and offset, so the layers differ in more than noise), draw
    fp32 [B,E], logits a: bf16-valued, spread about 2 (alpha far from uniform), in no particular order."""
    gen = torch.Generator().manual_seed(1000 * K + 100 * B + E + 7919 * seed)
    scale = 1.0 + 0.5 * torch.arange(K, dtype=F32)[:, None, None]
    P = torch.randn(K, B, E, generator=gen) * scale + 0.3 * torch.randn(K, 1, E, generator=gen)
    draw = torch.randn(B, E, generator=gen) * 1e-2
    a = None
    if K > 1:
        a = (torch.linspace(-1.0, 1.0, K)[torch.randperm(K, generator=gen)] + 0.05 * torch.randn(K, generator=gen)).to(BF16).float()
    return dict(P=P, draw=draw, a=a, K=K, B=B, E=E)


def dh_inputs(E=512, B=3, S=33, lens=None, seed=0):
    """hidden bf16 [B,S,E] of TWO taps (head_emul.make_inputs' statistics: per-channel offset, outlier channels), an HRF-like
    mask with a dead leading span, clip 1 all zero (and nothing past ``lens`` when the rows are packed), draw [B,E] for
    each tap, and a seeded bf16 dx the accumulate mode adds into."""
    case = H._case(f"dh-E{E}", E, S, B, 8, zero_clip=True, lens=lens)
    one = H.make_inputs(case, seed=4242 + seed)
    two = H.make_inputs(case, seed=977 + seed)
    gen = torch.Generator().manual_seed(31 + seed)
    draw = torch.randn(2, B, E, generator=gen) * 1e-2
    dx0 = (torch.randn(B, S, E, generator=gen) * 3e-3).to(BF16)
    return dict(hidden=(one["hidden"], two["hidden"] * 0.5), wmask=one["wmask"], draw=draw, dx0=dx0, eps=EPS, lens=lens, E=E, B=B, S=S)


def pack_rows(t, lens):
    """dense [B,S,...] -> packed [sum(lens),...] (clip b's first lens[b] rows)"""
    return torch.cat([t[b, :n] for b, n in enumerate(lens)], 0)


def unpack_rows(t, lens, S, fill):
    """packed [rows,...] -> dense [B,S,...]; rows past a clip's length take ``fill``'s"""
    out, r = fill.clone(), 0
    for b, n in enumerate(lens):
        out[b, :n] = t[r:r + n]
        r += n
    return out


# ---------------------------------------------------------------------------------------------------- stages
def softmax(a, K, dt=F64):
    return torch.ones(1, dtype=dt) if a is None else torch.softmax(a.to(dt), 0)


def mix_fwd(P, a, dt=F64, bug=None):
    K = P.shape[0]
    alpha = softmax(a, K, dt)
    used = alpha.clone()
    if bug == "swap_alpha":
        used[0], used[1] = alpha[1], alpha[0]
    terms = used[:, None, None] * P.to(dt)
    return dict(alpha=alpha, pooled=terms.sum(0), mag=terms.abs().sum(0))


def mix_fwd_bars(ref, P, a):
    """alpha: K exps summed in order (chain K), the quotient and the product; the arguments a_k - max are differences of
    bf16 values rounded once: 2^-24 (max - min) absolute in the exponent, in numerator and denominator -> twice that,
    relative.  pooled: K - 1 additions of terms alpha_k P_k (one product each: + 1), and alpha's own bar carried by |P_k|."""
    K = P.shape[0]
    if a is None:
        return dict(alpha=torch.zeros(1, dtype=F64), pooled=torch.zeros_like(ref["pooled"]))     # 1.0f * P: exact
    spread = float(a.max() - a.min())
    bar_alpha = ref["alpha"] * ((K + 2 + 8) * U + 2 * U * spread + R)
    bar_pooled = (K - 1 + 1 + 2) * U * ref["mag"] + (bar_alpha[:, None, None] * P.to(F64).abs()).sum(0) + R * ref["pooled"].abs()
    return dict(alpha=bar_alpha, pooled=bar_pooled)


def mix_bwd(P, draw, alpha, dt=F64, bug=None):
    """alpha: what the forward left (the device's own fp32 vector, or mix_fwd's)."""
    P, d, al = P.to(dt), draw.to(dt), alpha.to(dt)
    prod = d[None] * P
    dal = prod.sum((1, 2))
    dot = (al * dal).sum()
    d_a = al * (dal - (0.0 if bug == "no_jacobian_sum" else dot))
    return dict(d_a=d_a, draw_stack=al[:, None, None] * d[None], dal=dal, dot=dot, mag_dal=prod.abs().sum((1, 2)),
                mag_dot=(al * dal).abs().sum())


def mix_bwd_bars(ref, alpha, B, E):
    """dal_k: a thread's 4 products (4), wave_sum (6), 4 waves (4), nblk slabs.  d_a_k = alpha_k (dal_k - dot): dot is a
    chain of K products of rounded dal; the difference carries the absolute errors of dal_k and of dot; two more roundings
    (the difference, the product).  draw_stack: one product."""
    K = alpha.numel()
    al = alpha.to(F64)
    nblk = cdiv(B * E, MIX_CHUNK)
    bar_dal = (4 + 6 + 4 + nblk + 2) * U * ref["mag_dal"] + R * ref["dal"].abs()
    bar_dot = (al * bar_dal).sum() + (K + 1 + 2) * U * ref["mag_dot"]
    bar_da = al * (bar_dal + bar_dot + 2 * U * (ref["dal"].abs() + ref["dot"].abs())) + R * ref["d_a"].abs()
    return dict(d_a=bar_da, draw_stack=(1 + 2) * U * ref["draw_stack"].abs() + R * ref["draw_stack"].abs())


def stats_of(hidden, eps, dt=F64):
    x = hidden.to(dt)
    mu = x.mean(-1)
    return mu, (((x - mu[..., None]) ** 2).mean(-1) + eps).rsqrt()


def dhidden_write(hidden, wmask, mu, rstd, draw, dt=F64):
    """head_dhidden_kernel: head_emul.dhidden (value on live rows, exactly 0 elsewhere), unrounded."""
    return H.dhidden(hidden, wmask, mu, rstd, draw, dt=dt)


def dhidden_write_bars(ref, E):
    return H.dhidden_bars(ref, E)["dh"]


def dhidden_acc(dx0, hidden, wmask, mu, rstd, draw, dt=F64, bug=None):
    """head_dhidden_acc_kernel, unrounded: dx0 + value on live rows; rows with w = 0 keep dx0's bits.
    bugs: ``overwrite`` (the value alone), ``touch_dead`` (zero-weight rows zeroed, as write mode does)."""
    ref = H.dhidden(hidden, wmask, mu, rstd, draw, dt=dt)
    live = (wmask != 0)[..., None]
    base = dx0.to(dt)
    summed = ref["dh"] if bug == "overwrite" else base + ref["dh"]
    dead = torch.zeros_like(base) if bug == "touch_dead" else base
    return dict(ref, dx=torch.where(live, summed, dead), live=live)


def dhidden_acc_bars(ref, E):
    """the fp32 bar of the value, the fp32 add, half a bf16 ulp of the sum; nothing on rows that are not written"""
    bar32 = H.dhidden_bars(ref, E)["dh"] - HB * ref["dh"].abs()
    return torch.where(ref["live"], bar32 + (U + HB) * ref["dx"].abs(), torch.zeros((), dtype=F64))


BUGS = ("swap_alpha", "no_jacobian_sum", "overwrite", "touch_dead", "wrong_tap_stats")
ratio = H.ratio
