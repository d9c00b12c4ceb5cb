"""The closed-form ridge fit on the GPU (csrc/ridge_solve.hip, BrainHead.ridge_*): every entry point against the fp64 numpy
emulator tests/ridge_emul.py.  Bars are derived there and in test_cpu_ridge_emul.py (none is fitted to the device's output):

* accumulate, integers: ``torch.equal`` (every partial sum is an integer far below 2^53).
* accumulate, Gaussian: n 2^-52 sum_k |a_k b_k| per element; two runs bit-identical (no atomics, fixed order).
* Cholesky: |A - L L^T| <= gamma_{n+1} |L| |L|^T (Higham Thm 10.3); solve: |R - X A| <= gamma_{3n+1} |X| |L| |L|^T (Thm 10.4).
* vlb_ridge_solve forms A = G - sz sz^T / N + rho I and R = C - sy sz^T / N itself, in fp64: a product, a scaling by the
  rounded 1/N, a subtraction (and the diagonal's addition) are at most 5 roundings of the magnitudes involved, so the system
  the device factored is within 5 * 2^-53 (|G| + |sz||sz|^T / N + rho I) of the emulator's (R likewise); that is added to
  the two bars above when they are applied to the emulator's A and R.
* full geometry, solution against the emulator: both satisfy Thm 10.4, so to first order each is within
  cond_2(A) * gamma_{3E+1} * || |L||L|^T ||_F / ||A||_2 of the exact solution in the 2-norm; the two differ by at most the
  sum:  c * E * cond_2(A) * 2^-53  with  c = 6 r * 1.01,  r = || |L||L|^T ||_F / ||A||_2 taken from the EMULATOR's factor
  (6 = 2 solutions * gamma_{3E+1} / (E 2^-53) rounded up; 1.01 for the second-order term, cond * 6 r E 2^-53 < 0.01 is asserted).
  cond_2(A) = (rho + lambda_max(Zc Zc^T)) / rho exactly, since N < E leaves rho as the smallest eigenvalue.
* whole head: masters within one fp32 ulp of float32(emulator) + E cond_2(A) 2^-53 max|W|; bf16 copies = RNE(masters);
  the split's mean loss_terms against J of the emulator's bf16-rounded solution, evaluated in fp64 on the same z, to the
  ridge stage's own bars of tests/head_emul.py (group_emul.py for per-subject heads): its loss bar, plus its pred bar carried
  through the square, (2 sum|d| bar_pred + sum bar_pred^2) / (B V).
"""
import numpy as np
import pytest
import torch

import group_emul as GE
import head_emul as HE
import ridge_emul as RE

pytestmark = pytest.mark.gpu
F64, BF16 = torch.float64, torch.bfloat16
U64 = RE.U64


def _st():
    return torch.cuda.current_stream().cuda_stream


def _state(E, V, dev):
    return dict(G=torch.zeros(E, E, dtype=F64, device=dev), C=torch.zeros(V, E, dtype=F64, device=dev),
                sz=torch.zeros(E, dtype=F64, device=dev), sy=torch.zeros(V, dtype=F64, device=dev))


def _add(s, z, y, lo=0, hi=None):
    from phantom_vlb_amd._lib import check, lib
    hi = z.shape[0] if hi is None else hi
    E, V = z.shape[1], y.shape[1]
    zz, yy = z[lo:hi], y[lo:hi]
    assert zz.is_contiguous() and yy.is_contiguous()
    check(lib.vlb_ridge_gram_accumulate(zz.data_ptr(), yy.data_ptr(), V, s["G"].data_ptr(), s["C"].data_ptr(), s["sz"].data_ptr(),
                                        s["sy"].data_ptr(), hi - lo, E, V, _st()), "vlb_ridge_gram_accumulate")


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("G", "C", "sz", "sy"))


def _host(s):
    return {k: v.cpu().numpy() for k, v in s.items()}


# ---------------------------------------------------------------------------------------------------- accumulate
@pytest.mark.parametrize("n,E,V", [(1, 16, 1), (37, 96, 5), (64, 64, 64), (65, 130, 33), (513, 256, 100)])
def test_accumulate_integers_exactly(dev, n, E, V):
    rng = np.random.default_rng(n * 1000 + E)
    zi, yi = rng.integers(-3, 4, (n, E)), rng.integers(-4, 5, (n, V))
    z = torch.from_numpy(zi.astype(np.float32)).to(dev, BF16)
    y = torch.from_numpy(yi.astype(np.float32)).to(dev)
    ref = RE.sums(zi, yi, chunk=n)
    s = _state(E, V, dev)
    _add(s, z, y)
    torch.cuda.synchronize()
    got = _host(s)
    for k in ("G", "C", "sz", "sy"):
        assert np.array_equal(got[k], ref[k]), f"{k} differs: max |d| {np.abs(got[k] - ref[k]).max()}"
    # a second call adds to a non-zero state
    _add(s, z, y)
    torch.cuda.synchronize()
    got = _host(s)
    for k in ("G", "C", "sz", "sy"):
        assert np.array_equal(got[k], 2 * ref[k]), f"{k}: the second call did not accumulate"
    if n == 513:
        for cuts in ((0, 512, 513), (0, 200, 400, 513)):
            t = _state(E, V, dev)
            for lo, hi in zip(cuts, cuts[1:]):
                _add(t, z, y, lo, hi)
            torch.cuda.synchronize()
            assert all(np.array_equal(_host(t)[k], ref[k]) for k in ("G", "C", "sz", "sy")), cuts


@pytest.mark.parametrize("n,E,V", [(65, 130, 33), (513, 256, 100)])
def test_accumulate_gaussian_within_the_summation_bar_and_reproducible(dev, n, E, V):
    gen = torch.Generator(device="cpu").manual_seed(n + E)
    z = (torch.randn(n, E, generator=gen) * 1.5 + 0.25).to(BF16).to(dev)
    y = (torch.randn(n, V, generator=gen) * 2 - 0.5).to(dev)
    zh, yh = z.float().cpu().numpy().astype(np.float64), y.cpu().numpy().astype(np.float64)
    ref = RE.sums(zh, yh, chunk=n)
    runs = []
    for _ in range(2):
        s = _state(E, V, dev)
        _add(s, z, y)
        torch.cuda.synchronize()
        runs.append(s)
    assert _same(runs[0], runs[1]), "two runs differ: the summation order is not fixed"
    got = _host(runs[0])
    bars = dict(G=RE.gram_bar(zh, zh), C=RE.gram_bar(yh, zh), sz=n * 2.0 ** -52 * np.abs(zh).sum(0), sy=n * 2.0 ** -52 * np.abs(yh).sum(0))
    for k, bar in bars.items():
        ratio = float(np.max(np.abs(got[k] - ref[k]) / bar))
        print(f"n={n} E={E} V={V} {k}: max err / bar {ratio:.3e}")
        assert ratio <= 1, k


# ---------------------------------------------------------------------------------------------------- Cholesky, solve
def _spd(n, seed, c=0.5):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n + 3, n))
    return X.T @ X + c * np.eye(n)


def _chol(A_host, dev, lda=None, upper=None):
    """device factorisation of A_host; the strict upper triangle (and the pitch padding) handed over hold ``upper``"""
    from phantom_vlb_amd._lib import check, lib
    n = A_host.shape[0]
    lda = n if lda is None else lda
    buf = np.full((n, lda), -7.25 if upper is None else upper)
    buf[:, :n] = np.where(np.tril(np.ones((n, n), bool)), A_host, buf[:, :n])
    A = torch.from_numpy(buf).to(dev)
    info = torch.full((1,), 77, dtype=torch.int32, device=dev)          # the entry clears it
    check(lib.vlb_chol_f64(A.data_ptr(), n, lda, info.data_ptr(), _st()), "vlb_chol_f64")
    torch.cuda.synchronize()
    return A, info, buf


@pytest.mark.parametrize("n,lda", [(1, 1), (7, 7), (64, 64), (65, 65), (130, 130), (200, 200), (130, 133), (200, 208)])
def test_cholesky_meets_the_componentwise_bound_and_leaves_the_upper_triangle(dev, n, lda):
    A0 = _spd(n, n + lda)
    A, info, buf = _chol(A0, dev, lda)
    assert int(info) == 0
    out = A.cpu().numpy()
    up = ~np.tril(np.ones((n, lda), bool))
    assert np.array_equal(out[up], buf[up]), "bytes above the diagonal (or in the pitch padding) changed"
    L = np.tril(out[:, :n])
    assert np.all(np.diag(L) > 0)
    ratio = float(np.max(np.abs(A0 - L @ L.T) / RE.chol_bar(L)))
    print(f"n={n} lda={lda}: max |A - L L^T| / bar {ratio:.3e}")
    assert ratio <= 1


@pytest.mark.parametrize("n,p", [(7, 3), (200, 0), (200, 70), (200, 128), (200, 199)])
def test_cholesky_reports_the_first_bad_pivot_and_stops(dev, n, p):
    A0 = _spd(n, 11 * n + p)
    A0[p, p] = -1.0                      # leading minors 1..p stay positive; pivot p + 1 is -1 - sum L[p,:p]^2 < 0
    A, info, _ = _chol(A0, dev)
    assert int(info) == p + 1
    out = A.cpu().numpy()
    assert np.isfinite(out).all(), "the factorisation went on with a pivot that is not positive"
    # what was factored before the failure is right: the leading block of whole 64-blocks
    k = p // 64 * 64
    if k:
        L = np.tril(out[:k, :k])
        assert np.all(np.abs(A0[:k, :k] - L @ L.T) <= RE.chol_bar(L))


def test_cholesky_flags_nan(dev):
    for n, (i, j) in ((7, (5, 2)), (130, (100, 3)), (130, (129, 129))):
        A0 = _spd(n, n)
        A0[i, j] = A0[j, i] = np.nan
        assert int(_chol(A0, dev)[1]) != 0


@pytest.mark.parametrize("n,nrhs,ldx", [(1, 1, 1), (7, 5, 7), (65, 1, 65), (65, 100, 65), (130, 5, 131), (200, 100, 200), (200, 5, 200)])
def test_solve_meets_the_residual_bound(dev, n, nrhs, ldx):
    from phantom_vlb_amd._lib import check, lib
    A0 = _spd(n, 7 * n + nrhs)
    A, info, _ = _chol(A0, dev)
    assert int(info) == 0
    rng = np.random.default_rng(n + nrhs)
    R = rng.standard_normal((nrhs, n))
    buf = np.full((nrhs, ldx), 3.5)
    buf[:, :n] = R
    X = torch.from_numpy(buf).to(dev)
    check(lib.vlb_chol_solve_f64(A.data_ptr(), n, X.data_ptr(), n, nrhs, ldx, info.data_ptr(), _st()), "vlb_chol_solve_f64")
    torch.cuda.synchronize()
    out = X.cpu().numpy()
    assert np.all(out[:, n:] == 3.5), "the pitch padding was written"
    L, Xs = np.tril(A.cpu().numpy()), out[:, :n]
    ratio = float(np.max(np.abs(R - Xs @ A0) / RE.solve_bar(L, Xs)))
    print(f"n={n} nrhs={nrhs} ldx={ldx}: max |R - X A| / bar {ratio:.3e}")
    assert ratio <= 1
    # a failed factorisation's info makes the solve a no-op
    bad = torch.ones(1, dtype=torch.int32, device=dev)
    X2 = torch.from_numpy(buf).to(dev)
    check(lib.vlb_chol_solve_f64(A.data_ptr(), n, X2.data_ptr(), n, nrhs, ldx, bad.data_ptr(), _st()), "vlb_chol_solve_f64")
    torch.cuda.synchronize()
    assert np.array_equal(X2.cpu().numpy(), buf)


# ---------------------------------------------------------------------------------------------------- vlb_ridge_solve
def _ridge_solve(s, N, lam, E, V, dev):
    from phantom_vlb_amd._lib import check, lib
    A = torch.full((E, E), -7.25, dtype=F64, device=dev)
    X = torch.empty(V, E, dtype=F64, device=dev)
    W = torch.full((V, E), 9.0, dtype=torch.float32, device=dev)
    b = torch.full((V,), 9.0, dtype=torch.float32, device=dev)
    info = torch.full((1,), 77, dtype=torch.int32, device=dev)
    check(lib.vlb_ridge_solve(s["G"].data_ptr(), s["C"].data_ptr(), s["sz"].data_ptr(), s["sy"].data_ptr(), N, lam, A.data_ptr(),
                              X.data_ptr(), W.data_ptr(), b.data_ptr(), info.data_ptr(), E, V, _st()), "vlb_ridge_solve")
    torch.cuda.synchronize()
    return A, X, W, b, int(info)


def test_full_geometry_system(dev):
    """E = 4096, V = 32, N = 600 < E: the ridge term carries the conditioning."""
    E, V, N, lam = 4096, 32, 600, 1e-3
    gen = torch.Generator(device="cpu").manual_seed(4096)
    z = (torch.randn(N, E, generator=gen) * (0.5 + torch.rand(E, generator=gen)) + torch.randn(E, generator=gen)).to(BF16).to(dev)
    y = (torch.randn(N, V, generator=gen) + 0.3).to(dev)
    s = _state(E, V, dev)
    _add(s, z, y, 0, 512)
    _add(s, z, y, 512, N)
    before = {k: v.clone() for k, v in s.items()}
    A_ws, X_ws, W, b, info = _ridge_solve(s, N, lam, E, V, dev)
    assert info == 0 and _same(s, before), "the sums are read only"
    sh = _host(s)
    sh["n"] = N
    zh, yh = z.float().cpu().numpy().astype(np.float64), y.cpu().numpy().astype(np.float64)
    ref_s = RE.sums(zh, yh, chunk=512)
    assert all(np.all(np.abs(sh[k] - ref_s[k]) <= bar) for k, bar in (("G", RE.gram_bar(zh, zh)), ("C", RE.gram_bar(yh, zh))))
    rho = lam * N * V
    # the emulator on the DEVICE's sums: what is compared below is the system, the factor and the solve
    emu = RE.solve(sh, lam)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    A0, R0 = t(emu["A"]), t(emu["R"])
    form_A = 5 * U64 * (s["G"].abs() + torch.outer(s["sz"].abs(), s["sz"].abs()) / N + rho * torch.eye(E, dtype=F64, device=dev))
    form_R = 5 * U64 * (s["C"].abs() + torch.outer(s["sy"].abs(), s["sz"].abs()) / N)
    L = torch.tril(A_ws)
    LL = L.abs() @ L.abs().t()
    r_f = float(torch.max((A0 - L @ L.t()).abs() / (RE.gamma(E + 1) * LL + form_A)))
    # residual of the fp64 solution X_ws against the emulator's system
    res = (R0 - X_ws @ A0).abs()
    r_s = float(torch.max(res / (RE.gamma(3 * E + 1) * (X_ws.abs() @ LL) + form_R + X_ws.abs() @ form_A)))
    print(f"full geometry: factor err / bar {r_f:.3e}, residual / bar {r_s:.3e}")
    assert r_f <= 1 and r_s <= 1
    # the strict upper triangle holds the system as formed (never touched by the factorisation): the device's own A
    up = torch.triu(torch.ones(E, E, dtype=torch.bool, device=dev), 1)
    assert bool(((A_ws - A0).abs()[up] <= form_A[up]).all())
    # norm-wise against the emulator's solution
    zc = zh - zh.mean(0)
    lmax = float(np.linalg.eigvalsh(zc @ zc.T)[-1])

    def normwise(emu, X, rho):
        cond = (rho + lmax) / rho
        Le = t(np.abs(emu["L"]))
        r = float(torch.linalg.matrix_norm(Le @ Le.t())) / (rho + lmax)
        c = 6 * r * 1.01
        bar = c * E * cond * U64
        assert cond * 6 * r * E * U64 < 0.01
        rel = np.linalg.norm(X - emu["W"], axis=1) / np.linalg.norm(emu["W"], axis=1)
        print(f"full geometry rho {rho:.1f}: cond_2 {cond:.1f}, r {r:.2f}, c {c:.2f}, max rel err {rel.max():.3e}, bar {bar:.3e}")
        assert np.all(rel <= bar)
    Xh = X_ws.cpu().numpy()
    normwise(emu, Xh, rho)
    # W_out / b_out are the fp32 roundings of the fp64 solution and of the bias formed from it
    assert torch.equal(W, X_ws.float())
    b_ref = sh["sy"] / N - Xh @ sh["sz"] / N
    b_bar = (E + 4) * U64 * (np.abs(sh["sy"]) / N + np.abs(Xh) @ np.abs(sh["sz"]) / N) + RE.ulp32(b_ref)
    assert np.all(np.abs(b.cpu().numpy().astype(np.float64) - b_ref) <= b_bar)


# ---------------------------------------------------------------------------------------------------- the whole head
E_MINI, V_MINI, LAM = 512, 128, 1e-3
BATCH = 25


def _make(kind, dev):
    """head, cache, y [N,V], subject (host int64 [N] or None)"""
    from phantom_vlb_amd.feature_cache import FeatureCache
    from phantom_vlb_amd.head import LAYER_MIX, BrainHead
    gen = torch.Generator(device="cpu").manual_seed({"plain": 1, "taps": 2, "subjects": 3}[kind])
    kw, layers, N = {}, None, 700
    if kind == "taps":
        kw, layers = dict(readout_layers=[1, 2, 4]), 3
    if kind == "subjects":
        kw, N = dict(subjects=["s-a", "s-b", "s-c"]), 1200
    head = BrainHead(E_MINI, V_MINI, LAM, 1e-5, dev, seed=5, **kw)
    for n in ("layer_norm1.weight", "layer_norm1.bias", "layer_norm2.weight", "layer_norm2.bias"):
        head.master[n].add_(0.1 * torch.randn(E_MINI, generator=gen).to(dev))
        head.compute[n].copy_(head.master[n])
    if kind == "taps":
        head.master[LAYER_MIX].copy_(torch.tensor([0.5, -1.0, 1.25]))
        head.compute[LAYER_MIX].copy_(head.master[LAYER_MIX])
    cache = FeatureCache("train", N, E_MINI, dev, layers=layers)
    cache._alloc()
    cache.pooled.copy_((torch.randn(*cache.pooled.shape, generator=gen) * 3 + 0.5 * torch.randn(E_MINI, generator=gen)).to(dev))
    cache.sumw.copy_((0.5 + torch.rand(N, generator=gen)).to(dev))
    cache.valid[:] = True
    subject = None
    if kind == "subjects":            # unequal N: 700 / 300 / 200, the last two below E = 512
        subject = torch.cat([torch.zeros(700), torch.ones(300), torch.full((200,), 2)]).long()[torch.randperm(N, generator=gen)]
    # targets with a linear part in the features, through bf16 as every step sees them
    mix = torch.randn(E_MINI, V_MINI, generator=gen) / 40
    src = cache.pooled if layers is None else cache.pooled.mean(0)
    y = (src.cpu() @ mix + 0.7 * torch.randn(N, V_MINI, generator=gen) + 0.2).to(BF16).float().to(dev).contiguous()
    return head, cache, y, subject


def _split_loss(head, cache, y, subject):
    """mean loss_terms of the existing cached forward over the split in index order, and the device's z and pred"""
    N = y.shape[0]
    assert N % BATCH == 0
    terms, zs, preds = [], [], []
    for lo in range(0, N, BATCH):
        idx = torch.arange(lo, lo + BATCH)
        _, t = head.forward_cached(cache, idx, y[lo:lo + BATCH], None, None if subject is None else subject[lo:lo + BATCH])
        terms.append(t.double().cpu())
        zs.append(head.z[:BATCH].float().cpu().double())
        preds.append(head.pred[:BATCH].double().cpu())
    return torch.stack(terms).mean(0), torch.cat(zs), torch.cat(preds)


def _adamw_epoch(head, cache, y, subject):
    """one epoch of the project's clip + AdamW over every head parameter, batches in index order (the mini YAML's lr)"""
    from types import SimpleNamespace

    from phantom_vlb_amd.flat import FlatTrainables
    from phantom_vlb_amd.optim import VlbAdamW
    flat = FlatTrainables(SimpleNamespace(head=head, lora=None))
    opt = VlbAdamW([(n, torch.nn.Parameter(head.master[n])) for n in head.param_names], flat, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                   weight_decay=1e-2, max_norm=1.0)
    for lo in range(0, y.shape[0], BATCH):
        sub = None if subject is None else subject[lo:lo + BATCH]
        head.forward_cached(cache, torch.arange(lo, lo + BATCH), y[lo:lo + BATCH], None, sub)
        if head.K:
            head.backward_tapped()
        else:
            head.backward_cached()
        opt.step()


@pytest.mark.parametrize("kind", ["plain", "taps", "subjects"])
def test_whole_head(dev, kind):
    head, cache, y, subject = _make(kind, dev)
    N, E, V, H = y.shape[0], E_MINI, V_MINI, max(1, head.G)
    wn, bn = "ridge_layer.linear.weight", "ridge_layer.linear.bias"
    # ---- the features are forward_cached's, bit for bit
    for idx in (torch.tensor([5, 699, 0, 321, 17]), torch.randperm(N, generator=torch.Generator().manual_seed(9))[:37]):
        sub = None if subject is None else subject[idx]
        head.forward_cached(cache, idx, y[idx.to(dev)].contiguous(), None, sub)
        z_fwd = head.z[:idx.numel()].clone()
        head.z.fill_(float("nan"))
        z_new = head.features_cached(cache, idx)[:idx.numel()]
        torch.cuda.synchronize()
        assert torch.equal(z_new.view(torch.int16), z_fwd.view(torch.int16)), "vlb_head_features_cached: z differs from forward_cached's"
    loss_init, z_all, _ = _split_loss(head, cache, y, subject)
    # ---- accumulate (512-clip chunks, the last one partial), solve
    head.ridge_stats_begin()
    for lo in range(0, N, 512):
        idx = torch.arange(lo, min(lo + 512, N))
        head.ridge_stats_add(cache, idx, y[lo:lo + 512], None if subject is None else subject[idx])
    counts = [N] if subject is None else [int((subject == g).sum()) for g in range(H)]
    assert head._ridge["n"] == counts
    before = {n: t.clone() for n, t in head.master.items()}
    if kind == "subjects":       # l2_lambda = 0 with N < E: refused on the host, nothing written
        with pytest.raises(ValueError, match=r"head 1 \('s-b'\) has N = 300 <= E = 512"):
            head.ridge_solve(l2_lambda=0.0)
        assert all(torch.equal(head.master[n], t) for n, t in before.items())
    out = head.ridge_solve()
    torch.cuda.synchronize()
    assert [o["n"] for o in out] == counts and all(o["info"] == 0 and o["l2_lambda"] == LAM for o in out)
    for n in ("layer_norm1.weight", "layer_norm1.bias", "layer_norm2.weight", "layer_norm2.bias"):
        assert torch.equal(head.master[n], before[n])
    # ---- the emulator on the same z (the device's bf16 features) and y, per head
    zh, yh = z_all.numpy(), y.double().cpu().numpy()
    W_dev = head.master[wn].cpu().numpy().reshape(H, V, E)
    b_dev = head.master[bn].cpu().numpy().reshape(H, V)
    W_emu, b_emu = np.zeros((H, V, E)), np.zeros((H, V))
    for g in range(H):
        rows = np.arange(N) if subject is None else np.nonzero(subject.numpy() == g)[0]
        sol = RE.solve(RE.sums(zh[rows], yh[rows], chunk=512), LAM)
        cond = RE.cond2(sol["A"])
        W_emu[g], b_emu[g] = sol["W"], sol["b"]
        dW = np.abs(W_dev[g].astype(np.float64) - sol["W"].astype(np.float32).astype(np.float64))
        rW = float(np.max(dW / RE.master_bar(sol["W"], cond, E)))
        # the bias: the same bar with the weights' floor carried through zbar (b = ybar - W zbar)
        zbar = np.abs(zh[rows].mean(0))
        b_bar = RE.ulp32(sol["b"]) + E * cond * U64 * float(np.abs(sol["W"]).max()) * float(zbar.sum()) + (E + 4) * U64 * (
            np.abs(yh[rows].mean(0)) + np.abs(sol["W"]) @ zbar)
        rb = float(np.max(np.abs(b_dev[g].astype(np.float64) - sol["b"].astype(np.float32).astype(np.float64)) / b_bar))
        print(f"{kind} head {g}: N {len(rows)}, cond_2 {cond:.1f}, max |dW| / bar {rW:.3f}, max |db| / bar {rb:.3f}")
        assert rW <= 1 and rb <= 1
    if kind == "plain":          # the sums are only read: another lambda re-solves from them, and the first one comes back bit for bit
        first = head.master[wn].clone()
        assert head.ridge_solve(l2_lambda=10 * LAM)[0]["l2_lambda"] == 10 * LAM
        sol10 = RE.solve(RE.sums(zh, yh, chunk=512), 10 * LAM)
        d10 = np.abs(head.master[wn].cpu().numpy().astype(np.float64) - sol10["W"].astype(np.float32).astype(np.float64))
        assert np.all(d10 <= RE.master_bar(sol10["W"], RE.cond2(sol10["A"]), E)) and not torch.equal(head.master[wn], first)
        head.ridge_solve()
        assert torch.equal(head.master[wn], first)
    # ---- bf16 copies: round to nearest even of the masters
    for n in (wn, bn):
        want = RE.rne_bf16(head.master[n].cpu().numpy())
        assert np.array_equal(head.compute[n].float().cpu().numpy(), want), f"{n}: the bf16 copy is not RNE(master)"
    # ---- the split's loss against J of the emulator's bf16-rounded solution, in fp64 on the same z
    loss_fit, _, _ = _split_loss(head, cache, y, subject)
    Wr = torch.from_numpy(RE.rne_bf16(W_emu.astype(np.float32)).astype(np.float64))
    br = torch.from_numpy(RE.rne_bf16(b_emu.astype(np.float32)).astype(np.float64))
    ref_sum, bar_sum = torch.zeros(3, dtype=F64), torch.zeros(3, dtype=F64)
    for lo in range(0, N, BATCH):
        zb, yb = z_all[lo:lo + BATCH], y[lo:lo + BATCH].double().cpu()
        if subject is None:
            ref = HE.ridge(zb, Wr[0], br[0], yb, LAM)
            bars = HE.ridge_bars(ref, BATCH, E, V)
        else:
            ref = GE.ridge(zb, Wr, br, yb, subject[lo:lo + BATCH], LAM)
            bars = GE.ridge_bars(ref, BATCH, E, V, H)
        d = (ref["pred"] - yb).abs()
        carried = (2 * (d * bars["pred"]).sum() + (bars["pred"] ** 2).sum()) / (BATCH * V)
        ref_sum += ref["loss"]
        bar_sum += bars["loss"] + torch.stack([carried, torch.zeros((), dtype=F64), carried])
    nb = N // BATCH
    ref_mean, bar_mean = ref_sum / nb, bar_sum / nb
    # (equal batches: the mean over the batches of the per-batch data term IS the data term of J over the split)
    ratios = ((loss_fit - ref_mean).abs() / bar_mean).tolist()
    print(f"{kind}: loss (mse, l2, total) {loss_fit.tolist()} vs J {ref_mean.tolist()}: err / bar {ratios}; random init {loss_init.tolist()}")
    assert max(ratios) <= 1
    # ---- and it is the minimum: below the untouched random-init head, below one epoch of AdamW on the same data
    assert float(loss_fit[2]) < float(loss_init[2])
    other, cache2, y2, subject2 = _make(kind, dev)
    _adamw_epoch(other, cache2, y2, subject2)
    loss_adamw, _, _ = _split_loss(other, cache2, y2, subject2)
    print(f"{kind}: closed form {float(loss_fit[2]):.6f} < one AdamW epoch {float(loss_adamw[2]):.6f} < random init {float(loss_init[2]):.6f}")
    assert float(loss_fit[2]) < float(loss_adamw[2])
    head.ridge_stats_end()


def test_failed_solve_raises_and_leaves_the_parameters(dev):
    """l2_lambda = 0 with N < E is refused on the host; a NaN target is found on the device (info < 0) and ridge_solve raises
    naming the head and the column.  Neither leaves a trace in the masters or the bf16 copies."""
    head, cache, y, _ = _make("plain", dev)
    before = {n: (head.master[n].clone(), head.compute[n].clone()) for n in head.param_names}
    y = y.clone()
    y[3, 7] = float("nan")
    head.ridge_stats_begin()
    head.ridge_stats_add(cache, torch.arange(0, 400), y[:400])
    with pytest.raises(ValueError, match=r"N = 400 <= E = 512.*l2_lambda > 0"):
        head.ridge_solve(l2_lambda=0.0)
    # a NaN in y reaches C and sy, never the matrix the factorisation sees: vlb_ridge_solve looks at sy itself
    with pytest.raises(ValueError, match=r"the head: target column 7 holds a NaN or Inf \(info = -8"):
        head.ridge_solve()
    for n, (m, c) in before.items():
        assert torch.equal(head.master[n], m) and torch.equal(head.compute[n], c), n
