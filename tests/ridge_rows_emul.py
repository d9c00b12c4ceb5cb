"""fp64 numpy restatement of the per-target choice of ``l2_lambda`` (BrainHead.ridge_cv(per_target=True), ridge_solve_rows,
set_l2_lambda_rows; vlb_ridge_cv_select / vlb_ridge_solve_rows of csrc/ridge_solve.hip and vlb_head_l2_rows_fwd / _bwd of
csrc/head.hip), its error bars and planted bugs.  Built on ridge_cv_emul (the table of held-out r) and
ridge_emul (the solve).

The objective with one penalty per target decouples per row of W:

    J(W, b) = 1/(N V) sum_n ||W z_n + b - y_n||^2 + sum_v lam_v ||W_v||^2
    (Zc^T Zc + lam_v N V I) W_v^T = Zc^T Yc_v,   b = ybar - W zbar

so row v of the minimiser is row v of ridge_emul.solve with the scalar lam_v.

``select_rows`` does, per target, the operations vlb_ridge_cv_select does, in its order (s = 0; s += r[k] for ascending k;
s / K; a strict ``>`` against the best so far, an exact tie decided by the grid VALUE; an excluded point never compared), so
the device's three outputs are compared with ``torch.equal``.

Bars - none is fitted to what the device returns:
* ``rmean_bar``: rmean[i,v] is the mean over K folds of r values that each carry ridge_cv_emul's bar ``r_bar``; summed in any
  order on either side:  r_bar.mean(folds) + K 2^-52.
* the choice: where a target's best rmean leads its runner-up by more than 2 bars no device within its bars can choose
  another point; the tests ask for 100 (``margins``).
* ``l2_bar``: the device squares bf16 values in fp32 (exact: 16 significant bits), sums E of them per row in fp64, multiplies
  by the row's lambda (one product), sums the R rows in fp64 and rounds once to fp32; the emulator sums in extended
  precision:  ((E + R + 2) 2^-52 + 2^-24) l2  (every term is >= 0, so the sums' relative error is the bound itself).
* ``grad_bar``: d = g + (coef lam_r) w in fp32, fused or not: one rounding of the product coef lam_r, one of the sum (and one
  of the product with w when it is not fused):  2^-23 (|g| + |coef lam_r w|) per element.
"""
from __future__ import annotations

import numpy as np

import ridge_cv_emul as CE
import ridge_emul as RE

BUGS = ("tie_smaller", "argmax_by_index", "first_fold", "max_over_folds", "excluded_wins", "choice_shifted", "l2_mean_lambda",
        "grad_first_lambda")
LD = np.longdouble if CE.EXT else np.float64


# ---------------------------------------------------------------------------------------------------- the recipe
def planted_rows(N=300, E=96, V=40, seed=5, rho=0.0, mean=0.5, noise=(0.3, 40.0), dens=(0.03, 0.8)):
    """test_cpu_ridge_cv_emul.planted with a noise sd per target (geomspace over ``noise``, permuted) and a weight density per
    target (geomspace over ``dens``): z bf16-valued [N,E], y fp32-valued [N,V].  The draws come in ``planted``'s order; the
    permutation is drawn after the weights, before the offsets and the noise."""
    rng = np.random.default_rng(seed)

    def ar1(n, m):
        e = rng.standard_normal((n, m))
        for t in range(1, n):
            e[t] = rho * e[t - 1] + np.sqrt(1 - rho * rho) * e[t]
        return e
    z = RE.rne_bf16((ar1(N, E) + mean).astype(np.float32)).astype(np.float64)
    W = rng.standard_normal((V, E)) * (rng.random((V, E)) < np.geomspace(dens[0], dens[1], V)[:, None])
    sd = np.geomspace(noise[0], noise[1], V)[rng.permutation(V)]
    y = (z @ W.T + rng.uniform(-2, 2, V) + sd * ar1(N, V)).astype(np.float32).astype(np.float64)
    return z, y


# ---------------------------------------------------------------------------------------------------- selection
def fold_mean(r):
    """r [K,L,V] -> rmean [L,V]: (sum over k ascending, from 0) / K, the device's operations"""
    r = np.asarray(r, np.float64)
    s = np.zeros(r.shape[1:])
    for k in range(r.shape[0]):
        s = s + r[k]
    return s / float(r.shape[0])


def select_rows(r, grid, ok=None, bug: str | None = None) -> dict:
    """r [K,L,V] (one head's held-out r), grid [L] (any order), ok [L] -> rmean [L,V], choice [V] (int32), rbest [V].
    No allowed point: choice -1, rbest NaN."""
    r = np.asarray(r, np.float64)
    K, L, V = r.shape
    ok = [True] * L if ok is None else [bool(o) for o in ok]
    rmean = fold_mean(r)
    decide = rmean
    if bug == "first_fold":
        decide = r[0]
    if bug == "max_over_folds":
        decide = r.max(0)
    choice, rbest = np.full(V, -1, np.int32), np.full(V, np.nan)
    for v in range(V):
        best, db, gb = -1, np.nan, 0.0
        for i in range(L):
            if not ok[i] and bug != "excluded_wins":
                continue
            m = decide[i, v]
            key = float(i) if bug == "argmax_by_index" else float(grid[i])
            tie = key < gb if bug == "tie_smaller" else key > gb
            if best < 0 or m > db or (m == db and tie):
                best, db, gb = i, m, key
        choice[v] = best
        if best >= 0:
            rbest[v] = rmean[best, v]
    return dict(rmean=rmean, choice=choice, rbest=rbest)


def rmean_bar(r_bar):
    """r_bar [K,L,V] (ridge_cv_emul's) -> the bar of rmean [L,V]"""
    r_bar = np.asarray(r_bar, np.float64)
    return r_bar.mean(0) + r_bar.shape[0] * 2.0 ** -52


def margins(rmean, bar, ok=None):
    """per target: (best - runner-up) / max(their two bars) over the allowed grid points; [V] (inf with one allowed point)"""
    rmean, bar = np.asarray(rmean, np.float64), np.asarray(bar, np.float64)
    L, V = rmean.shape
    cand = [i for i in range(L) if ok is None or ok[i]]
    out = np.full(V, np.inf)
    for v in range(V):
        order = sorted(cand, key=lambda i: rmean[i, v], reverse=True)
        if len(order) > 1:
            a, b = order[0], order[1]
            out[v] = (rmean[a, v] - rmean[b, v]) / max(bar[a, v], bar[b, v])
    return out


def counts(choice, L):
    return np.bincount(np.asarray(choice, np.int64), minlength=L)


# ---------------------------------------------------------------------------------------------------- the solve, row by row
def solve_rows(sums: dict, grid, choice, bug: str | None = None) -> dict:
    """-> W [V,E], b [V] (fp64): row v from ridge_emul.solve(sums, grid[choice[v]]); ``sols``: the solve per used grid point"""
    choice = np.asarray(choice, np.int64)
    L = len(grid)
    V, E = sums["C"].shape
    take = (choice + 1) % L if bug == "choice_shifted" else choice
    W, b, sols = np.zeros((V, E)), np.zeros(V), {}
    for i in sorted(set(take.tolist())):
        sols[i] = RE.solve(sums, grid[i])
        rows = take == i
        W[rows], b[rows] = sols[i]["W"][rows], sols[i]["b"][rows]
    return dict(W=W, b=b, sols=sols)


def objective_rows(W, b, z, y, lam):
    """(data term, penalty, J) of the objective with lam [V] in fp64"""
    W, b, z, y, lam = (np.asarray(a, np.float64) for a in (W, b, z, y, lam))
    N, V = y.shape
    d = z @ W.T + b - y
    data, pen = float((d * d).sum() / (N * V)), float((lam * (W * W).sum(1)).sum())
    return data, pen, data + pen


def gradient_rows(W, b, z, y, lam):
    """ridge_emul.gradient with lam [V]: dJ/dW, dJ/db and the magnitudes of the terms they are made of"""
    W, b, z, y, lam = (np.asarray(a, np.float64) for a in (W, b, z, y, lam))
    N, V = y.shape
    d = z @ W.T + b - y
    dW = 2.0 / (N * V) * d.T @ z + 2.0 * lam[:, None] * W
    db = 2.0 / (N * V) * d.sum(0)
    mag_d = np.abs(z) @ np.abs(W).T + np.abs(b) + np.abs(y)
    mag_W = 2.0 / (N * V) * mag_d.T @ np.abs(z) + 2.0 * lam[:, None] * np.abs(W)
    mag_b = 2.0 / (N * V) * mag_d.sum(0)
    return dW, db, mag_W, mag_b


def lstsq_row(z, y, v, lam_v):
    """row v of the minimiser through ``numpy.linalg.lstsq`` on its own augmented system (the ridge term is lam_v N V with V
    the number of targets of the whole head)"""
    z, y = np.asarray(z, np.float64), np.asarray(y, np.float64)
    N, E = z.shape
    V = y.shape[1]
    zbar, ybar = z.mean(0), y[:, v].mean()
    M = np.concatenate([z - zbar, np.sqrt(lam_v * N * V) * np.eye(E)], 0)
    t = np.concatenate([y[:, v] - ybar, np.zeros(E)], 0)
    w = np.linalg.lstsq(M, t, rcond=None)[0]
    return w, ybar - w @ zbar


# ---------------------------------------------------------------------------------------------------- the penalty on the step
def l2_rows(W_bf16, lam, bug: str | None = None) -> float:
    """sum_r lam[r] sum_e W[r,e]^2 in extended precision (W: the bf16 compute copy's values, [R,E])"""
    W, lam = np.asarray(W_bf16, LD), np.asarray(lam, LD).reshape(-1)
    W = W.reshape(lam.shape[0], -1)
    if bug == "l2_mean_lambda":
        lam = np.full_like(lam, lam.mean())
    return float((lam * (W * W).sum(1)).sum())


def l2_rows_grad(W_bf16, lam, coef: float, bug: str | None = None):
    """coef lam[r] W[r,e] in fp64, [R,E] (coef = l2_scale * 2)"""
    lam = np.asarray(lam, np.float64).reshape(-1)
    W = np.asarray(W_bf16, np.float64).reshape(lam.shape[0], -1)
    if bug == "grad_first_lambda":
        lam = np.full_like(lam, lam[0])
    return float(coef) * lam[:, None] * W


def l2_bar(R: int, E: int, l2: float) -> float:
    return ((E + R + 2) * 2.0 ** -52 + 2.0 ** -24) * abs(l2)


def grad_bar(g, term):
    return 2.0 ** -23 * (np.abs(np.asarray(g, np.float64)) + np.abs(np.asarray(term, np.float64)))


# ---------------------------------------------------------------------------------------------------- the whole fit
def fit(z, y, grid, K: int, block: int, chunk: int = 512, sub=None, bug: str | None = None, bars: bool = False, ok=None,
        cv: dict | None = None) -> dict:
    """ridge_cv_emul.cv, then per head the selection and the row-wise solve of the head's totals.  -> cv (CE.cv's dict),
    rmean [H,L,V], choice [H,V], rbest [H,V], lambda_rows [H,V], lambda_counts [H,L], score_per_target, W [H,V,E], b [H,V];
    with ``bars`` also rmean_bar [H,L,V] and margins [H,V]."""
    cv = CE.cv(z, y, grid, K, block, chunk=chunk, sub=sub, bars=bars) if cv is None else cv
    H, L = cv["r"].shape[0], len(grid)
    sel = [select_rows(cv["r"][g], grid, ok, bug) for g in range(H)]
    out = dict(cv=cv, rmean=np.stack([s["rmean"] for s in sel]), choice=np.stack([s["choice"] for s in sel]),
               rbest=np.stack([s["rbest"] for s in sel]))
    out["lambda_rows"] = np.asarray(grid, np.float64)[out["choice"]]
    out["lambda_counts"] = np.stack([counts(c, L) for c in out["choice"]])
    out["score_per_target"] = float(out["rbest"].mean())
    sols = [solve_rows(CE.sum_except(cv["S"][g], -1), grid, out["choice"][g], bug) for g in range(H)]
    out["W"], out["b"] = np.stack([s["W"] for s in sols]), np.stack([s["b"] for s in sols])
    if bars:
        out["rmean_bar"] = np.stack([rmean_bar(cv["r_bar"][g]) for g in range(H)])
        out["margins"] = np.stack([margins(out["rmean"][g], out["rmean_bar"][g], ok) for g in range(H)])
    return out
