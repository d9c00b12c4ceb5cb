"""fp64 numpy restatement of the blocked K-fold cross-validation of ``l2_lambda`` (BrainHead.ridge_cv, the vlb_ridge_cv_*
entries of phantom_vlb_amd/csrc/ridge_solve.hip), its error bars and planted bugs.  Built on ridge_emul's
``sums`` / ``solve``.

Per head, clip m (its rank among the clips that head has received, in walk order) belongs to fold ``(m // block) % K``.  The
sums are kept per fold, S_k = (G_k, C_k, sz_k, sy_k, syy_k, n_k); fold k's training sums are T_k = sum_{j != k} S_j (ascending
j) and are solved as ridge_emul solves any sums (N = N - n_k, ridge term lam (N - n_k) V).  The held-out Pearson correlation
of target v needs S_k and the solution X [V,E] only (r does not depend on the bias):

    Gc = G_k - sz_k sz_k^T / n_k      Rc = C_k - sy_k sz_k^T / n_k      vy_v = syy_k[v] - sy_k[v]^2 / n_k
    cov_v = X[v,:] . Rc[v,:]          vp_v = X[v,:] Gc X[v,:]^T
    r_v = cov_v / sqrt(vp_v vy_v) clipped to [-1, 1];  0 unless vp_v > 0 and vy_v > 0

The score of a grid point is the mean over heads and folds of the mean over targets of r; the largest wins, an exact tie goes
to the larger lambda, a grid point with a failed solve is left out.

Bars - none is fitted to what the device returns (u = 2^-53):
* per element of Gc (Rc alike): forming it, 5 u (|G| + |sz||sz|^T / n) as in §5.3.5; the two fp64 accumulations of G_k
  (device, emulator; any order), n 2^-52 sum_k |a_k b_k| (``ridge_emul.gram_bar``); and the same for sz (sy) carried through
  the outer product, (dsz |sz|^T + |sz| dsz^T) / n with dsz = n 2^-52 sum |z|.
* vy: 5 u (syy + sy^2 / n) + n 2^-52 sum y^2 + 2 |sy| dsy / n.
* vp: |dvp| <= gamma_{2E+c} |x|^T |Gc| |x|  (E products and E - 1 additions per element of x Gc, then E more of each against
  x; any order) + |x|^T dGc |x|;  cov: |dcov| <= gamma_{E+c} |x| . |Rc_v| + |x| . dRc_v;  c = 4 covers the product vp vy, the
  square root, the division and 1 / n.  ``score`` evaluates vp and cov in extended precision (x87 long double, 64-bit
  significand) where numpy has it, so the emulator's own rounding is 2^-11 of the bar and the one-sided bound is what two
  computations differ by; without it the two gamma terms are doubled.
* r, to first order:  |dr| <= |dcov| / sqrt(vp vy) + |r| (|dvp| / (2 vp) + |dvy| / (2 vy)), valid where vp and vy exceed their
  own bars by 10^3 (``valid``; the tests assert it for every target, none is left out).
* when device and emulator each solve for their own X (the end-to-end tests), the two backward-stable solutions of the same
  system differ by |dX| <= (2 solve_bar + dR + |X| dA) |A^-1| to first order (``dx_bar``; dA, dR: the training system's own
  forming and accumulation bars), which enters through |dvp| += 2 |dX| |Gc| |x| and |dcov| += |dX| . |Rc_v|.
* a score (a mean of r over V targets, K folds, H heads, summed in any order on either side): the mean of the r bars plus
  (V + K + H) 2^-52.
"""
from __future__ import annotations

import numpy as np

import ridge_emul as RE

U64 = RE.U64
BUGS = ("leak", "ridge_n_total", "no_fold_centring", "interleaved", "cov_uncentred", "argmax_first_fold")
C_DOT = 4
EXT = np.finfo(np.longdouble).nmant >= 63
_F = 1.0 if EXT else 2.0


# ---------------------------------------------------------------------------------------------------- folds
def fold_of(m, K: int, block: int, bug: str | None = None):
    m = np.asarray(m, np.int64)
    return m % K if bug == "interleaved" else (m // block) % K


def assign(n: int, K: int, block: int, sub=None, chunk: int = 512, bug: str | None = None):
    """The fold of each of n clips walked in index order, ``chunk`` at a time, as ``ridge_stats_add`` decides it: a chunk is
    partitioned by head (``sub``: one head index per clip; None: one head) and each head counts its own clips."""
    sub = np.zeros(n, np.int64) if sub is None else np.asarray(sub, np.int64)
    seen: dict[int, int] = {}
    fold = np.empty(n, np.int64)
    for lo, hi in RE.chunks_of(n, chunk):
        for g in np.unique(sub[lo:hi]):
            rows = lo + np.nonzero(sub[lo:hi] == g)[0]
            m0 = seen.get(int(g), 0)
            fold[rows] = fold_of(m0 + np.arange(len(rows)), K, block, bug)
            seen[int(g)] = m0 + len(rows)
    return fold


def fold_sums(z, y, fold, K: int, chunk: int = 512) -> list:
    """z [N,E], y [N,V] of ONE head in walk order, fold [N] -> K dicts (G, C, sz, sy, syy, n, rows), fp64, accumulated over
    chunks of ``chunk`` rows in index order, each chunk partitioned by fold."""
    z, y = np.asarray(z, np.float64), np.asarray(y, np.float64)
    N, E = z.shape
    V = y.shape[1]
    S = [dict(G=np.zeros((E, E)), C=np.zeros((V, E)), sz=np.zeros(E), sy=np.zeros(V), syy=np.zeros(V), n=0) for _ in range(K)]
    for lo, hi in RE.chunks_of(N, chunk):
        for k in range(K):
            rows = lo + np.nonzero(fold[lo:hi] == k)[0]
            if not len(rows):
                continue
            zz, yy, s = z[rows], y[rows], S[k]
            s["G"] += zz.T @ zz
            s["C"] += yy.T @ zz
            s["sz"] += zz.sum(0)
            s["sy"] += yy.sum(0)
            s["syy"] += (yy * yy).sum(0)
            s["n"] += len(rows)
    for k in range(K):
        S[k]["rows"] = np.nonzero(np.asarray(fold) == k)[0]
    return S


def sum_except(S: list, skip: int, bug: str | None = None) -> dict:
    """T = sum_{j != skip} S_j in ascending j (skip = -1: the totals)"""
    keep = [j for j in range(len(S)) if j != skip or bug == "leak"]
    T = {key: np.zeros_like(S[0][key]) for key in ("G", "C", "sz", "sy", "syy")}
    for j in keep:
        for key in T:
            T[key] = T[key] + S[j][key]
    T["n"] = sum(S[j]["n"] for j in keep)
    T["rows"] = np.sort(np.concatenate([S[j]["rows"] for j in keep]))
    return T


def solve_fold(S: list, k: int, lam: float, bug: str | None = None) -> dict:
    T = sum_except(S, k, bug)
    if bug == "ridge_n_total":              # the ridge term lam N V of the whole split on N - n_k clips
        lam = lam * sum(s["n"] for s in S) / T["n"]
    sol = RE.solve(T, lam)
    sol["T"] = T
    return sol


# ---------------------------------------------------------------------------------------------------- held-out moments, r
def moments(Sk: dict, bug: str | None = None):
    n = Sk["n"]
    if bug == "no_fold_centring":
        return Sk["G"].copy(), Sk["C"].copy(), Sk["syy"].copy()
    Gc = Sk["G"] - np.outer(Sk["sz"], Sk["sz"]) / n
    Rc = Sk["C"].copy() if bug == "cov_uncentred" else Sk["C"] - np.outer(Sk["sy"], Sk["sz"]) / n
    return Gc, Rc, Sk["syy"] - Sk["sy"] ** 2 / n


def score(X, Gc, Rc, vy) -> dict:
    """-> r [V], cov, vp (fp64; the two dot products in extended precision where numpy has it)"""
    ld = np.longdouble if EXT else np.float64
    Xl = np.asarray(X, ld)
    vp = np.asarray(((Xl @ np.asarray(Gc, ld)) * Xl).sum(1), np.float64)
    cov = np.asarray((Xl * np.asarray(Rc, ld)).sum(1), np.float64)
    ok = (vp > 0) & (vy > 0)
    r = np.zeros_like(vp)
    r[ok] = np.clip(cov[ok] / np.sqrt(vp[ok] * vy[ok]), -1.0, 1.0)
    return dict(r=r, cov=cov, vp=vp)


def explicit_r(z, y, W, b):
    """the two-pass Pearson correlation of the prediction z W^T + b against y, per target (in extended precision where numpy
    has it: its own rounding is then 2^-11 of an fp64 evaluation's)"""
    ld = np.longdouble if EXT else np.float64
    z, y, W, b = (np.asarray(a, ld) for a in (z, y, W, b))
    p = z @ W.T + b
    pc, yc = p - p.mean(0), y - y.mean(0)
    return np.asarray((pc * yc).sum(0) / np.sqrt((pc * pc).sum(0) * (yc * yc).sum(0)), np.float64)


# ---------------------------------------------------------------------------------------------------- bars
def moment_bars(zk, yk, Sk: dict):
    """(dGc [E,E], dRc [V,E], dvy [V]) for the fold whose rows are zk [n,E], yk [n,V]"""
    zk, yk = np.abs(np.asarray(zk, np.float64)), np.abs(np.asarray(yk, np.float64))
    n = Sk["n"]
    asz, asy = np.abs(Sk["sz"]), np.abs(Sk["sy"])
    dsz, dsy = n * 2.0 ** -52 * zk.sum(0), n * 2.0 ** -52 * yk.sum(0)
    dGc = 5 * U64 * (np.abs(Sk["G"]) + np.outer(asz, asz) / n) + RE.gram_bar(zk, zk) + (np.outer(dsz, asz) + np.outer(asz, dsz)) / n
    dRc = 5 * U64 * (np.abs(Sk["C"]) + np.outer(asy, asz) / n) + RE.gram_bar(yk, zk) + (np.outer(dsy, asz) + np.outer(asy, dsz)) / n
    dvy = 5 * U64 * (Sk["syy"] + asy ** 2 / n) + n * 2.0 ** -52 * (yk * yk).sum(0) + 2 * asy * dsy / n
    return dGc, dRc, dvy


def r_bar(X, Gc, Rc, vy, dGc, dRc, dvy, dX=None) -> dict:
    """The first-order bar on r for the solution X [V,E]; ``dX``: a bar on the difference of the two X that are scored."""
    E = X.shape[1]
    ax, aG, aR = np.abs(X), np.abs(Gc), np.abs(Rc)
    s = score(X, Gc, Rc, vy)
    dvp = _F * RE.gamma(2 * E + C_DOT) * ((ax @ aG) * ax).sum(1) + ((ax @ dGc) * ax).sum(1)
    dcov = _F * RE.gamma(E + C_DOT) * (ax * aR).sum(1) + (ax * dRc).sum(1)
    if dX is not None:
        dvp = dvp + 2 * ((dX @ aG) * ax).sum(1)
        dcov = dcov + (dX * aR).sum(1)
    vp, r = s["vp"], s["r"]
    valid = (vp > 1e3 * dvp) & (vy > 1e3 * dvy)
    with np.errstate(divide="ignore", invalid="ignore"):
        dr = dcov / np.sqrt(vp * vy) + np.abs(r) * (dvp / (2 * vp) + dvy / (2 * vy))
    return dict(dr=dr, dvp=dvp, dcov=dcov, valid=valid, **s)


def system_bars(z_tr, y_tr, sol: dict, lam: float):
    """(dA [E,E], dR [V,E]): forming and accumulation bars of the training system of ``sol`` (rows z_tr, y_tr)"""
    z_tr, y_tr = np.abs(np.asarray(z_tr, np.float64)), np.abs(np.asarray(y_tr, np.float64))
    T = sol["T"]
    n, V, E = T["n"], y_tr.shape[1], z_tr.shape[1]
    asz, asy = np.abs(T["sz"]), np.abs(T["sy"])
    dsz, dsy = n * 2.0 ** -52 * z_tr.sum(0), n * 2.0 ** -52 * y_tr.sum(0)
    dA = 5 * U64 * (np.abs(T["G"]) + np.outer(asz, asz) / n + lam * n * V * np.eye(E)) + RE.gram_bar(z_tr, z_tr) \
        + (np.outer(dsz, asz) + np.outer(asz, dsz)) / n
    dR = 5 * U64 * (np.abs(T["C"]) + np.outer(asy, asz) / n) + RE.gram_bar(y_tr, z_tr) + (np.outer(dsy, asz) + np.outer(asy, dsz)) / n
    return dA, dR


def dx_bar(sol: dict, dA, dR):
    """|X_device - X_emulator| to first order: two backward-stable solutions (ridge_emul.solve_bar each) of two systems that
    differ by at most (dA, dR)"""
    Ainv = np.abs(np.linalg.inv(sol["A"]))
    return (2 * RE.solve_bar(sol["L"], sol["W"]) + dR + np.abs(sol["W"]) @ dA) @ Ainv


# ---------------------------------------------------------------------------------------------------- selection, the whole CV
def select(means, grid, ok=None, bug: str | None = None) -> dict:
    """means [H,K,L] (target-mean r per head, fold, grid point) -> score [L], score_per_head [H,L], best_index"""
    means = np.asarray(means, np.float64)
    L = means.shape[2]
    ok = [True] * L if ok is None else list(ok)
    per_head = means.mean(1)
    sc = per_head.mean(0)
    decide = means[:, :1].mean(1).mean(0) if bug == "argmax_first_fold" else sc
    cand = [i for i in range(L) if ok[i]]
    if not cand:
        raise ValueError("every grid point is excluded")
    best = max(cand, key=lambda i: (decide[i], grid[i]))
    return dict(score=sc, score_per_head=per_head, best_index=best, best_lambda=grid[best])


def cv(z, y, grid, K: int, block: int, chunk: int = 512, sub=None, bug: str | None = None, bars: bool = False,
       own_x: bool = True) -> dict:
    """The whole cross-validation of z [N,E], y [N,V] (walk order; ``sub``: head per clip).  -> r [H,K,L,V], means [H,K,L],
    score, score_per_head, best_index, best_lambda, fold [N], S (per head: the fold sums), X [H][K][L]; with ``bars`` also
    r_bar [H,K,L,V], valid [H,K,L,V] and score_bar [L] (``own_x``: the device solves for its own X, ``dx_bar`` is included)."""
    z, y = np.asarray(z, np.float64), np.asarray(y, np.float64)
    N, E = z.shape
    V, L = y.shape[1], len(grid)
    sub_ = np.zeros(N, np.int64) if sub is None else np.asarray(sub, np.int64)
    H = int(sub_.max()) + 1
    fold = assign(N, K, block, sub, chunk, bug)
    r = np.full((H, K, L, V), np.nan)
    rb, valid = np.full((H, K, L, V), np.nan), np.zeros((H, K, L, V), bool)
    S_all, X_all = [], []
    for g in range(H):
        rows_g = np.nonzero(sub_ == g)[0]
        zg, yg = z[rows_g], y[rows_g]
        # the head's clips reach it in chunks of the walk; their partition into folds does not depend on that chunking
        S = fold_sums(zg, yg, fold[rows_g], K, chunk)
        S_all.append(S)
        X_all.append([])
        for k in range(K):
            Gc, Rc, vy = moments(S[k], bug)
            if bars:
                dGc, dRc, dvy = moment_bars(zg[S[k]["rows"]], yg[S[k]["rows"]], S[k])
            X_all[g].append([])
            for i, lam in enumerate(grid):
                sol = solve_fold(S, k, lam, bug)
                X_all[g][k].append(sol["W"])
                r[g, k, i] = score(sol["W"], Gc, Rc, vy)["r"]
                if bars:
                    dX = None
                    if own_x:
                        tr = sol["T"]["rows"]
                        dX = dx_bar(sol, *system_bars(zg[tr], yg[tr], sol, lam))
                    b = r_bar(sol["W"], Gc, Rc, vy, dGc, dRc, dvy, dX)
                    rb[g, k, i], valid[g, k, i] = b["dr"], b["valid"]
    means = r.mean(-1)
    out = dict(r=r, means=means, fold=fold, S=S_all, X=X_all, grid=list(grid), **select(means, list(grid), bug=bug))
    if bars:
        out.update(r_bar=rb, valid=valid, score_bar=rb.mean((0, 1, 3)) + (V + K + H) * 2.0 ** -52)
    return out
