"""fp64 numpy restatement of the closed-form ridge fit and its cross-validation under target weights (BrainHead's
``ridge_stats_begin(weighted=True)`` path; vlb_ridge_gram_accumulate_masked / vlb_ridge_sumsq_accumulate_masked /
vlb_ridge_cv_score_rows of csrc/ridge_solve.hip) and its planted bugs.  Built on ridge_emul (sums, solve),
ridge_cv_emul (folds, held-out r, bars) and ridge_rows_emul (selection, margins); their bars are reused unwidened.

Per head, with w the fp32 weight row, Ws = sum_v w_v and N that head's clips, the weighted objective of §5.3.8 plus the penalty

    J(W, b) = (1/N) sum_n sum_v w_v (W_v z_n + b_v - y_nv)^2 / Ws + sum_v lam_v ||W_v||^2

decouples per target: for w_v > 0 row v is row v of ridge_emul.solve with lam_v Ws / (V w_v); for w_v = 0 the data term does
not see the row, the penalty puts W_v = 0 and b_v (free) is written as 0.  The distinct positive fp32 weights of a row are its
levels, ascending; ``scale[d] = Ws / (V w_d)`` with Ws the exactly rounded sum (math.fsum), so a constant row has scale 1.0.

* the sums read y through a select (``np.where(w > 0, y, 0)``): a NaN / Inf in a masked column reaches nothing, the masked
  rows of C and entries of sy, syy are +0;
* the held-out table is NaN at masked targets; a (head, fold, grid point) mean, and with it every score, is the plain mean over
  the kept targets; the per-target choice is made for kept targets only (masked: -1, rbest NaN, lambda_rows = best_lambda);
* ``solve_rows_w``: a kept target's code is choice * D + level; every used (grid point, level) is solved once.

Bars: a kept row at level d IS ridge_emul's / ridge_cv_emul's computation on the selected y with lam scale[d], so
``ridge_emul.master_bar`` and ``ridge_cv_emul.r_bar`` / ``dx_bar`` / ``system_bars`` apply to it as they stand; a mean over K'
kept targets carries the mean of their bars plus (K' + K + H) 2^-52 (any summation order on either side).
"""
from __future__ import annotations

import math

import numpy as np

import ridge_cv_emul as CE
import ridge_emul as RE
import ridge_rows_emul as RR

BUGS = ("no_ws_over_v", "w_inverted", "mask_product", "masked_unsolved", "mean_all_v", "swap_levels", "count_masked")
MAX_LEVELS = 8
UNSOLVED = 0.5          # what "masked_unsolved" leaves in a masked row: whatever the scratch held


# ---------------------------------------------------------------------------------------------------- levels, sums
def levels(w, bug: str | None = None) -> dict:
    """w [V] (fp32 values) -> lvl [V] (-1: masked), scale [D] (fp64), vals [D], keep [V] bool"""
    w32 = np.asarray(w, np.float32)
    row = [float(x) for x in w32]
    vals = sorted({x for x in row if x > 0})
    if len(vals) > MAX_LEVELS:
        raise ValueError(f"{len(vals)} levels")
    rank = {x: d for d, x in enumerate(vals)}
    V, ws = len(row), math.fsum(row)
    scale = [ws / (V * x) for x in vals]
    if bug == "no_ws_over_v":
        scale = [1.0 / x for x in vals]
    if bug == "w_inverted":
        scale = [ws * x / V for x in vals]
    if bug == "swap_levels" and len(vals) > 1:
        scale[0], scale[1] = scale[1], scale[0]
    return dict(lvl=np.array([rank[x] if x > 0 else -1 for x in row], np.int64), scale=scale, vals=vals, keep=w32 > 0)


def select_y(y, w, bug: str | None = None):
    y = np.asarray(y, np.float64)
    keep = np.asarray(w, np.float32) > 0
    if bug == "mask_product":
        with np.errstate(invalid="ignore"):
            return y * keep.astype(np.float64)
    return np.where(keep[None, :], y, 0.0)


def sums_w(z, y, w, chunk: int = 512, bug: str | None = None) -> dict:
    return RE.sums(z, select_y(y, w, bug), chunk=chunk)


def fold_sums_w(z, y, w, fold, K: int, chunk: int = 512, bug: str | None = None) -> list:
    return CE.fold_sums(z, select_y(y, w, bug), fold, K, chunk)


# ---------------------------------------------------------------------------------------------------- the solve, level by level
def solve_w(s: dict, lam, w, bug: str | None = None) -> dict:
    """-> W [V,E], b [V] (fp64; masked rows exactly 0), sols {d: ridge_emul.solve's dict}, lv (levels' dict).  ``lam``: a
    scalar, or [V] (one penalty per row: each distinct (lam_v, level) pair is solved once)."""
    lv = levels(w, bug)
    V, E = s["C"].shape
    lam_v = np.broadcast_to(np.asarray(lam, np.float64), (V,))
    W, b, sols = np.zeros((V, E)), np.zeros(V), {}
    if bug == "masked_unsolved":
        W[:], b[:] = UNSOLVED, UNSOLVED
    for d, sc in enumerate(lv["scale"]):
        for lm in sorted(set(lam_v[lv["lvl"] == d].tolist())):
            sol = RE.solve(s, lm * sc)
            rows = (lv["lvl"] == d) & (lam_v == lm)
            W[rows], b[rows] = sol["W"][rows], sol["b"][rows]
            sols[(d, lm)] = sol
    return dict(W=W, b=b, sols=sols, lv=lv)


def solve_rows_w(s: dict, grid, choice, w, bug: str | None = None) -> dict:
    """the combined-code row solve: kept target v has code choice[v] * D + lvl[v]; each used code is solved once with
    grid[i] scale[d]; -1 is taken at masked targets only"""
    lv = levels(w, bug)
    choice = np.asarray(choice, np.int64)
    L, D = len(grid), len(lv["scale"])
    if np.any(lv["keep"] & ((choice < 0) | (choice >= L))):
        raise ValueError("-1 (or an index outside the grid) at a kept target")
    code = np.where(lv["keep"], choice * D + lv["lvl"], -1)
    V, E = s["C"].shape
    W, b, used = np.zeros((V, E)), np.zeros(V), []
    for c in sorted(set(code[code >= 0].tolist())):
        i, d = divmod(c, D)
        sol = RE.solve(s, grid[i] * lv["scale"][d])
        rows = code == c
        W[rows], b[rows] = sol["W"][rows], sol["b"][rows]
        used.append((i, d))
    return dict(W=W, b=b, code=code, used=used, lv=lv)


# ---------------------------------------------------------------------------------------------------- cross-validation
def cv_w(z, y, w, grid, K: int, block: int, chunk: int = 512, sub=None, bug: str | None = None, bars: bool = False) -> dict:
    """ridge_cv_emul.cv under weights w [H,V] (or [V]): r [H,K,L,V] (NaN at masked targets), means [H,K,L] over the kept
    targets, score, score_per_head, best_index, best_lambda, fold, S, keep [H,V]; with ``bars`` r_bar, valid (True at masked
    targets: nothing is claimed there) and score_bar [L]."""
    z, y = np.asarray(z, np.float64), np.asarray(y, np.float64)
    N, E = z.shape
    V, L = y.shape[1], len(grid)
    sub_ = np.zeros(N, np.int64) if sub is None else np.asarray(sub, np.int64)
    H = int(sub_.max()) + 1
    w = np.broadcast_to(np.asarray(w, np.float32).reshape(-1, V), (H, V))
    fold = CE.assign(N, K, block, sub, chunk)
    r, rb = np.full((H, K, L, V), np.nan), np.full((H, K, L, V), np.nan)
    valid = np.ones((H, K, L, V), bool)
    S_all, lvs = [], []
    for g in range(H):
        rows_g = np.nonzero(sub_ == g)[0]
        zg, yg = z[rows_g], select_y(y[rows_g], w[g], bug)
        lv = levels(w[g], bug)
        lvs.append(lv)
        S = CE.fold_sums(zg, yg, fold[rows_g], K, chunk)
        S_all.append(S)
        for k in range(K):
            Gc, Rc, vy = CE.moments(S[k])
            if bars:
                dGc, dRc, dvy = CE.moment_bars(zg[S[k]["rows"]], yg[S[k]["rows"]], S[k])
            for i, lam in enumerate(grid):
                for d, sc in enumerate(lv["scale"]):
                    mine = lv["lvl"] == d
                    sol = CE.solve_fold(S, k, lam * sc)
                    with np.errstate(invalid="ignore", divide="ignore"):
                        r[g, k, i, mine] = CE.score(sol["W"], Gc, Rc, vy)["r"][mine]
                        if bars:
                            tr = sol["T"]["rows"]
                            dX = CE.dx_bar(sol, *CE.system_bars(zg[tr], yg[tr], sol, lam * sc))
                            bb = CE.r_bar(sol["W"], Gc, Rc, vy, dGc, dRc, dvy, dX)
                            rb[g, k, i, mine], valid[g, k, i, mine] = bb["dr"][mine], bb["valid"][mine]
    keep = np.stack([lv["keep"] for lv in lvs])
    if bug == "mean_all_v":
        means = np.nansum(r, -1) / V
    else:
        # (all kept: ridge_cv_emul's own expression, so a constant row reproduces its means bit for bit)
        means = np.stack([r[g].mean(-1) if keep[g].all() else r[g][..., keep[g]].mean(-1) for g in range(H)])
    out = dict(r=r, means=means, fold=fold, S=S_all, grid=list(grid), keep=keep, lv=lvs, **CE.select(means, list(grid)))
    if bars:
        kb = np.stack([rb[g][..., keep[g]].mean(-1) for g in range(H)])            # [H,K,L]
        out.update(r_bar=rb, valid=valid, means_bar=kb + V * 2.0 ** -52, score_bar=kb.mean((0, 1)) + (V + K + H) * 2.0 ** -52)
    return out


def fit_w(z, y, w, grid, K: int, block: int, chunk: int = 512, sub=None, bug: str | None = None, bars: bool = False,
          cv: dict | None = None) -> dict:
    """cv_w, then per head the per-target selection over kept targets and the combined-code row solve of the head's totals:
    rmean [H,L,V], choice [H,V] (-1 masked), rbest [H,V] (NaN masked), lambda_rows [H,V] (best_lambda where masked),
    lambda_counts [H,L] (kept targets), score_per_target, W [H,V,E], b [H,V]; with ``bars`` rmean_bar and margins (inf masked)."""
    cv = cv_w(z, y, w, grid, K, block, chunk=chunk, sub=sub, bug=bug, bars=bars) if cv is None else cv
    H, L = cv["r"].shape[0], len(grid)
    keep = cv["keep"]
    sel = [RR.select_rows(cv["r"][g], grid) for g in range(H)]
    raw = np.stack([s["choice"] for s in sel])
    choice = np.where(keep, raw, -1).astype(np.int32)
    rbest = np.where(keep, np.stack([s["rbest"] for s in sel]), np.nan)
    out = dict(cv=cv, rmean=np.stack([s["rmean"] for s in sel]), choice=choice, rbest=rbest)
    out["lambda_rows"] = np.where(keep, np.asarray(grid, np.float64)[np.maximum(choice, 0)], cv["best_lambda"])
    counted = raw if bug == "count_masked" else choice
    out["lambda_counts"] = np.stack([np.bincount(c[c >= 0], minlength=L) for c in counted])
    out["score_per_target"] = float(rbest[keep].mean())
    wq = np.broadcast_to(np.asarray(w, np.float32).reshape(-1, keep.shape[1]), keep.shape)
    sols = [solve_rows_w(CE.sum_except(cv["S"][g], -1), grid, choice[g], wq[g], bug) for g in range(H)]
    out["W"], out["b"] = np.stack([s["W"] for s in sols]), np.stack([s["b"] for s in sols])
    if bars:
        out["rmean_bar"] = np.stack([RR.rmean_bar(cv["r_bar"][g]) for g in range(H)])
        m = np.full(keep.shape, np.inf)
        for g in range(H):
            kk = np.nonzero(keep[g])[0]
            m[g, kk] = RR.margins(out["rmean"][g][:, kk], out["rmean_bar"][g][:, kk])
        out["margins"] = m
    return out


# ---------------------------------------------------------------------------------------------------- the objective
def objective_w(W, b, z, y, w, lam):
    """J of one head in fp64: (1/N) sum_n sum_v w_v (.)^2 / Ws + sum_v lam_v ||W_v||^2 (masked y never enters)"""
    W, b, z = (np.asarray(a, np.float64) for a in (W, b, z))
    w = np.asarray(w, np.float32).astype(np.float64)
    lam_v = np.broadcast_to(np.asarray(lam, np.float64), w.shape)
    d = z @ W.T + b - select_y(y, w)
    return float(((d * d) * w).sum() / (len(z) * w.sum()) + (lam_v * (W * W).sum(1)).sum())
