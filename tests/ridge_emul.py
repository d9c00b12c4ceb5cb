"""fp64 numpy restatement of the closed-form ridge fit (phantom_vlb_amd/csrc/ridge_solve.hip), its error
bars and planted bugs.

The objective (``loss="mse"``, LN parameters fixed, dropout off; z bf16 [N,E] as head_ln2_kernel writes it, y fp32 [N,V]):

    J(W, b) = 1/(N V) sum_n ||W z_n + b - y_n||^2 + lam ||W||_F^2
    (Zc^T Zc + lam N V I) W^T = Zc^T Yc,   b = ybar - W zbar            (Zc, Yc column-centred; b not penalised)

``sums`` accumulates G = Z^T Z, C = Y^T Z, sz, sy chunk by chunk as the device does; ``solve`` centres, factors with
``numpy.linalg.cholesky``, substitutes and forms the bias.  ``bug=`` plants one mistake in either.

Bars - none is fitted to what the device returns:
* exact sums: z integer in [-3,3] (exact in bf16), y integer in [-4,4]: every partial sum is an integer below
  N * 16 << 2^53, so any summation order gives the same fp64 number: ``torch.equal``.
* ``gram_bar``: a sum of n exact products accumulated in fp64 in ANY order is within gamma_{n-1} sum|a_k b_k| of the exact
  sum (Higham, Accuracy and Stability, §4.2); two such sums (device, emulator) differ by at most twice that, and
  2 gamma_{n-1} <= n 2^-52 for n 2^-53 << 1:   n * 2^-52 * sum_k |a_k b_k|   per element.
* ``chol_bar``: |A - L L^T| <= gamma_{n+1} |L| |L|^T elementwise (Thm 10.3), u = 2^-53, any summation order.
* ``solve_bar``: the computed x solves (A + dA) x = r with |dA| <= gamma_{3n+1} |L| |L|^T (Thm 10.4), so
  |r - A x| <= gamma_{3n+1} |L| |L|^T |x| elementwise.
* ``master_bar``: the device's fp32 weight against float32(emulator's): both fp64 solutions carry a forward error of
  order cond_2(A) u, so their fp32 roundings differ by at most one fp32 ulp wherever that error is below the ulp, plus the
  absolute floor E cond_2(A) 2^-53 max|W| for the entries so small that it is not.
"""
from __future__ import annotations

import numpy as np

U64 = 2.0 ** -53
BUGS = ("no_centring", "ridge_n", "ridge_on_bias", "c_transposed", "chunk_twice", "drop_last_chunk")


def gamma(k: int) -> float:
    return k * U64 / (1.0 - k * U64)


def chunks_of(n: int, chunk: int):
    return [(lo, min(lo + chunk, n)) for lo in range(0, n, chunk)]


def sums(z, y, chunk: int = 512, bug: str | None = None) -> dict:
    """z [N,E], y [N,V] (any float dtype holding bf16 / fp32 values) -> G [E,E], C [V,E], sz [E], sy [V], n; fp64,
    accumulated over chunks of ``chunk`` rows in index order."""
    z, y = np.asarray(z, np.float64), np.asarray(y, np.float64)
    N, E = z.shape
    V = y.shape[1]
    G, C, sz, sy, n = np.zeros((E, E)), np.zeros((V, E)), np.zeros(E), np.zeros(V), 0
    parts = chunks_of(N, chunk)
    if bug == "chunk_twice":
        parts = parts + parts[:1]
    if bug == "drop_last_chunk" and N % chunk:
        parts = parts[:-1]
    for lo, hi in parts:
        zz, yy = z[lo:hi], y[lo:hi]
        G += zz.T @ zz
        # the planted layout bug: z^T y [E,V] written into the [V,E] buffer as it lies in memory
        C += (zz.T @ yy).reshape(V, E) if bug == "c_transposed" else yy.T @ zz
        sz += zz.sum(0)
        sy += yy.sum(0)
        n += hi - lo
    return dict(G=G, C=C, sz=sz, sy=sy, n=n)


def system(s: dict, lam: float, bug: str | None = None):
    """The centred, regularised system A [E,E] and its right-hand sides R [V,E] (one per row)."""
    N, V, E = s["n"], s["C"].shape[0], s["G"].shape[0]
    sz, sy = s["sz"], s["sy"]
    if bug == "no_centring":
        A, R = s["G"].copy(), s["C"].copy()
    else:
        A, R = s["G"] - np.outer(sz, sz) / N, s["C"] - np.outer(sy, sz) / N
    A[np.diag_indices(E)] += lam * N * (1 if bug == "ridge_n" else V)
    return A, R


def solve(s: dict, lam: float, bug: str | None = None) -> dict:
    """-> W [V,E], b [V] (fp64), the system (A, R) and its factor L."""
    N, V = s["n"], s["C"].shape[0]
    if bug == "ridge_on_bias":
        # the penalty on (W, b): the augmented feature [z, 1] with an uncentred, fully regularised system
        E = s["G"].shape[0]
        Ga = np.block([[s["G"], s["sz"][:, None]], [s["sz"][None, :], np.array([[float(N)]])]])
        Ca = np.concatenate([s["C"], s["sy"][:, None]], 1)
        Wa = np.linalg.solve(Ga + lam * N * V * np.eye(E + 1), Ca.T).T
        return dict(W=Wa[:, :E], b=Wa[:, E])
    A, R = system(s, lam, bug)
    L = np.linalg.cholesky(A)
    X = np.linalg.solve(L.T, np.linalg.solve(L, R.T)).T
    b = s["sy"] / N - X @ s["sz"] / N
    return dict(W=X, b=b, A=A, R=R, L=L)


def objective(W, b, z, y, lam):
    """(data term, penalty, J) in fp64."""
    W, b, z, y = (np.asarray(a, np.float64) for a in (W, b, z, y))
    N, V = y.shape
    d = z @ W.T + b - y
    data, pen = float((d * d).sum() / (N * V)), float(lam * (W * W).sum())
    return data, pen, data + pen


def gradient(W, b, z, y, lam):
    """dJ/dW [V,E], dJ/db [V] and, for each, the sum of the magnitudes of the terms it is made of (what fp64 rounding of
    the evaluation itself can leave behind, relative to 2^-53)."""
    W, b, z, y = (np.asarray(a, np.float64) for a in (W, b, z, y))
    N, V = y.shape
    d = z @ W.T + b - y
    dW = 2.0 / (N * V) * d.T @ z + 2.0 * lam * W
    db = 2.0 / (N * V) * d.sum(0)
    mag_d = np.abs(z) @ np.abs(W).T + np.abs(b) + np.abs(y)
    mag_W = 2.0 / (N * V) * mag_d.T @ np.abs(z) + 2.0 * lam * np.abs(W)
    mag_b = 2.0 / (N * V) * mag_d.sum(0)
    return dW, db, mag_W, mag_b


def lstsq_solution(z, y, lam):
    """The same minimiser through ``numpy.linalg.lstsq`` on the augmented system
    min || [Zc; sqrt(lam N V) I] W^T - [Yc; 0] ||_F - no normal equations, no Cholesky."""
    z, y = np.asarray(z, np.float64), np.asarray(y, np.float64)
    N, E = z.shape
    V = y.shape[1]
    zbar, ybar = z.mean(0), y.mean(0)
    M = np.concatenate([z - zbar, np.sqrt(lam * N * V) * np.eye(E)], 0)
    T = np.concatenate([y - ybar, np.zeros((E, V))], 0)
    W = np.linalg.lstsq(M, T, rcond=None)[0].T
    return W, ybar - W @ zbar


# ---------------------------------------------------------------------------------------------------- bars
def gram_bar(a, b):
    """per element of a^T b (a [n,M], b [n,N]):  n * 2^-52 * sum_k |a_k| |b_k|"""
    a, b = np.abs(np.asarray(a, np.float64)), np.abs(np.asarray(b, np.float64))
    return a.shape[0] * 2.0 ** -52 * (a.T @ b)


def chol_bar(L):
    L = np.abs(np.tril(np.asarray(L, np.float64)))
    return gamma(L.shape[0] + 1) * (L @ L.T)


def solve_bar(L, X):
    """X [nrhs,n] (one solution per row) -> bar on R - X A  [nrhs,n]"""
    L = np.abs(np.tril(np.asarray(L, np.float64)))
    return gamma(3 * L.shape[0] + 1) * (np.abs(np.asarray(X, np.float64)) @ (L @ L.T))


def ulp32(x):
    x = np.abs(np.asarray(x, np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def master_bar(W_ref, cond: float, E: int):
    W32 = np.asarray(W_ref, np.float64).astype(np.float32)
    return ulp32(W32) + E * cond * U64 * float(np.abs(W_ref).max())


def rne_bf16(x32):
    """fp32 -> bf16 (round to nearest even) -> fp32, on the bit patterns"""
    u = np.asarray(x32, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def cond2(A) -> float:
    w = np.linalg.eigvalsh(np.asarray(A, np.float64))
    return float(w[-1] / w[0])
