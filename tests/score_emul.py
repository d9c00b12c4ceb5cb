"""Host restatement of the held-out scoring kernels (phantom_vlb_amd/csrc/score.hip): numpy fp64 with explicit
loops in the kernels' summation order, one IEEE operation per kernel operation (the kernels are compiled without contraction).
Elementwise numpy over the target axis performs, per target, exactly the scalar operation a thread performs.

Also the error bars the GPU tests hold the finisher and the bootstrap to.  With u = 2^-53 (half an ulp: the relative error of
one correctly rounded fp64 operation) every bar below counts rounded operations in score.hip's ``score_r`` /
``score_finish_kernel`` / ``score_bootstrap_kernel`` for both sides: the host's (numpy: correctly rounded, u each) and the
device's (+, -, * correctly rounded, u each; a division or square root is allowed one full ulp, 2u).  The block totals
themselves (pure additions in one order) carry no bar: both sides add the same numbers in the same order."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -53
NT = 256          # threads of score_avg_kernel's one block
RT = 8            # resamples per register tile of score_bootstrap_kernel (does not change any sum's order)


def bf16_round(x):
    """fp32 array -> the nearest bf16 value (ties to even), as fp32: what real ``pred`` / ``y`` hold"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def accumulate(sums, pred, y, slot, keep, nb):
    """vlb_score_accumulate: sums fp64 [n_slots,5,V] in place; pred / y fp32 [B,V]; slot ints [B]; keep fp32 [H,V] or None"""
    V = sums.shape[2]
    for b in range(len(slot)):
        s = int(slot[b])
        if s < 0 or s >= sums.shape[0]:
            continue
        k = np.ones(V, bool) if keep is None else keep[s // nb] > 0
        p = np.where(k, pred[b, :V].astype(np.float64), 0.0)
        t = np.where(k, y[b, :V].astype(np.float64), 0.0)
        sums[s, 0] += p
        sums[s, 1] += t
        sums[s, 2] += p * p
        sums[s, 3] += t * t
        sums[s, 4] += p * t
    return sums


def totals(sums_h, n_j, order):
    """T [5,V] and n from the blocks listed in ``order``, added one after the other from zero"""
    t = np.zeros(sums_h.shape[1:], np.float64)
    n = np.float64(0.0)
    for j in order:
        n = n + np.float64(n_j[j])
        t = t + sums_h[j]
    return t, n


def score_r(t, n):
    """score.hip ``score_r``: (r, cov, vp, vy) per target"""
    with np.errstate(all="ignore"):
        cov = t[4] - t[0] * t[1] / n
        vp = t[2] - t[0] * t[0] / n
        vy = t[3] - t[1] * t[1] / n
        ok = (vp > 0) & (vy > 0)
        r = np.where(ok, cov / np.sqrt(np.where(ok, vp * vy, 1.0)), 0.0)
    return np.clip(r, -1.0, 1.0), cov, vp, vy


def finish(sums_h, n_j, keep_h=None):
    """vlb_score_finish -> out fp64 [4,V], avg fp64 [3]"""
    nb, _, V = sums_h.shape
    t, n = totals(sums_h, n_j, range(nb))
    kept = np.ones(V, bool) if keep_h is None else keep_h > 0
    r, _, _, vy = score_r(t, n)
    with np.errstate(all="ignore"):
        sse = t[2] - 2.0 * t[4] + t[3]
        r2 = np.where(vy > 0, 1.0 - sse / np.where(vy > 0, vy, 1.0), 0.0)
        mse = sse / n
    out = np.stack([r, r2, mse, np.full(V, n)])
    out[:3, ~kept] = np.nan
    part = np.zeros((4, NT), np.float64)            # score_avg_kernel: thread t over v = t, t + NT, ..., then the partials in order
    for lo in range(0, V, NT):
        w = min(NT, V - lo)
        k = kept[lo:lo + w]
        part[3, :w] += np.where(k, 1.0, 0.0)
        for c in range(3):
            part[c, :w] += np.where(k, out[c, lo:lo + w], 0.0)
    a = np.zeros(4, np.float64)
    for i in range(NT):
        a += part[:, i]
    with np.errstate(all="ignore"):
        avg = a[:3] / a[3]
    return out, avg


def bootstrap(sums_h, n_j, draws, keep_h=None):
    """vlb_score_bootstrap -> out fp64 [3,V], the resampled r* [R,V] and each resample's (cov, vp, vy, T, n) for the bars"""
    nb, _, V = sums_h.shape
    R = draws.shape[0]
    kept = np.ones(V, bool) if keep_h is None else keep_h > 0
    rs, parts = np.zeros((R, V), np.float64), []
    s1, s2, le0 = np.zeros(V), np.zeros(V), np.zeros(V)
    for rho in range(R):
        t, n = totals(sums_h, n_j, [int(j) for j in draws[rho]])
        r, cov, vp, vy = score_r(t, n)
        rs[rho] = r
        parts.append((cov, vp, vy, t, n))
        d = r - rs[0]
        s1 = s1 + d
        s2 = s2 + d * d
        le0 = le0 + (r <= 0)
    Rd = np.float64(R)
    var = (s2 - s1 * s1 / Rd) / (Rd - 1.0)
    out = np.stack([rs[0] + s1 / Rd, np.sqrt(np.where(var > 0, var, 0.0)), (1.0 + le0) / (Rd + 1.0)])
    out[:, ~kept] = np.nan
    return out, rs, parts


# ---------------------------------------------------------------------------------------------------- error bars
K_CENTER = 7      # d = a - b c / n: host mul, div, sub (3u) + device mul (u), div (2u), sub (u); relative to |a| + |b c / n|
K_RATIO = 8       # cov / sqrt(vp vy): host mul, sqrt, div (3u) + device mul (u), sqrt (2u), div (2u); relative to |r|
K_SSE = 4         # (Tpp - 2 Tpy) + Tyy: two additions per side (2 Tpy is exact); relative to |Tpp| + 2 |Tpy| + |Tyy|
K_DIV = 3         # one division: host u + device 2u
K_SUB = 2         # one subtraction or addition per side


def center_bar(a, b, c, n):
    """bar of d = a - b c / n between the two sides: K_CENTER u (|a| + |b c / n|)"""
    return K_CENTER * U * (np.abs(a) + np.abs(b * c / n))


def r_bar(t, n, cov, vp, vy):
    """bar of r: the three centred moments' bars through cov / sqrt(vp vy) to first order, plus the quotient's own rounding.
    Where a variance is not clearly positive on both sides (vp or vy <= its bar) the branch may differ: the bar is 2, the range
    of r - unless the variance is exactly 0 with a zero bar (a constant column: both sides take the r = 0 branch)."""
    bc, bp, by = center_bar(t[4], t[0], t[1], n), center_bar(t[2], t[0], t[0], n), center_bar(t[3], t[1], t[1], n)
    with np.errstate(all="ignore"):
        sure = (vp > 2 * bp) & (vy > 2 * by)
        den = np.sqrt(np.where(sure, vp * vy, 1.0))
        r = cov / den
        # second-order terms are below 1/4 of the first-order ones under `sure`: the factor 1.25 covers them
        bar = 1.25 * (bc / den + np.abs(r) * 0.5 * (bp / np.where(sure, vp, 1.0) + by / np.where(sure, vy, 1.0))) + K_RATIO * U * np.abs(r)
    exact_zero = ((vp == 0) | (vy == 0)) & (vp >= 0) & (vy >= 0)
    return np.where(sure, bar, np.where(exact_zero, 0.0, 2.0))


def finish_bars(sums_h, n_j):
    """bars [3,V] of vlb_score_finish's r, R^2 and mse against ``finish``"""
    nb = sums_h.shape[0]
    t, n = totals(sums_h, n_j, range(nb))
    _, cov, vp, vy = score_r(t, n)
    by = center_bar(t[3], t[1], t[1], n)
    with np.errstate(all="ignore"):
        sse = t[2] - 2.0 * t[4] + t[3]
        bsse = K_SSE * U * (np.abs(t[2]) + 2 * np.abs(t[4]) + np.abs(t[3]))
        sure = vy > 2 * by
        vys = np.where(sure, vy, 1.0)
        q = sse / vys
        bq = 1.25 * (bsse / vys + np.abs(q) * by / vys) + K_DIV * U * np.abs(q)
        br2 = np.where(sure, bq + K_SUB * U * np.abs(1.0 - q), np.where(vy == 0, 0.0, np.inf))
        bmse = bsse / n + K_DIV * U * np.abs(sse / n)
    return np.stack([r_bar(t, n, cov, vp, vy), br2, bmse])


def bootstrap_bars(rs, parts):
    """bars [2,V] of vlb_score_bootstrap's mean and sd against ``bootstrap`` (the p-value's count is compared exactly)"""
    R = rs.shape[0]
    e = np.stack([r_bar(t, n, cov, vp, vy) for cov, vp, vy, t, n in parts])          # [R,V]: each r*'s bar
    d = rs - rs[0]
    ed = e + e[0] + K_SUB * U * np.abs(d)                                               # each d's
    sabs, s1, s2 = np.abs(d).sum(0), d.sum(0), (d * d).sum(0)
    es1 = ed.sum(0) + K_SUB * R * U * sabs                                             # R additions per side, each <= u sum|d|
    bmean = e[0] + es1 / R + (K_DIV + K_SUB) * U * (np.abs(s1) / R + np.abs(rs[0]))
    es2 = (2 * np.abs(d) * ed + ed * ed).sum(0) + K_SUB * (R + 1) * U * s2              # the squares' and the additions' rounding
    q = s1 * s1 / R
    eq = 2 * np.abs(s1) * es1 / R + es1 * es1 / R + (K_DIV + K_SUB) * U * q
    var = np.maximum((s2 - q) / (R - 1), 0.0)
    evar = (es2 + eq + K_SUB * U * (s2 + q)) / (R - 1) + K_DIV * U * var
    sd = np.sqrt(var)
    with np.errstate(all="ignore"):
        bsd = np.where(evar > 0, evar / np.maximum(sd, np.sqrt(evar)), 0.0) + 3 * U * sd      # |sqrt a - sqrt b| <= |a - b| / max(sqrt a, sqrt|a - b|)
    return np.stack([bmean, bsd])


# ---------------------------------------------------------------------------------------------------- seeded cases
def make_case(seed, n_clips, V, block, rho=0.5, const_y=(), const_p=(), masked=()):
    """One head's raw (p, y) fp32 [n,V] (bf16-valued, correlated with coefficient about ``rho``) -> dict with the per-block sums.
    const_y / const_p: targets whose y / prediction is one constant; masked: targets with keep = 0."""
    rng = np.random.RandomState(seed)
    y = rng.randn(n_clips, V)
    p = rho * y + np.sqrt(max(0.0, 1 - rho * rho)) * rng.randn(n_clips, V) + 0.25
    y[:, list(const_y)] = 0.75
    p[:, list(const_p)] = -1.5
    p, y = bf16_round(p.astype(np.float32)), bf16_round(y.astype(np.float32))
    nb = -(-n_clips // block)
    slot = np.arange(n_clips) // block
    keep = None
    if len(masked):
        keep = np.ones((1, V), np.float32)
        keep[0, list(masked)] = 0.0
    sums = accumulate(np.zeros((nb, 5, V), np.float64), p, y, slot, keep, nb)
    n_j = np.bincount(slot, minlength=nb).astype(np.float64)
    return dict(p=p, y=y, slot=slot, nb=nb, sums=sums, n_j=n_j, keep=keep, block=block)
