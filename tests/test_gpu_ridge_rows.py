"""One ``l2_lambda`` per target on the device: vlb_ridge_cv_select, vlb_ridge_solve_rows and the two per-row
penalty entries alone, then ``BrainHead.ridge_cv(per_target=True) / ridge_solve_rows / set_l2_lambda_rows`` on a plain head, a
head with three tapped layers and three per-subject heads, then the option through the module and both checkpoint routes,
against tests/ridge_rows_emul.py.

Bars (derived in ridge_rows_emul's docstring; none is fitted to what the device returns):
* the selection kernel does the emulator's fp64 operations in the emulator's order: ``torch.equal``, no tolerance.
* the row-masked solve runs vlb_ridge_solve's launches: every row ``torch.equal`` to the plain solve's row for its lambda.
* l2 term: ((E + R + 2) 2^-52 + 2^-24) l2;  its gradient: 2^-23 (|g| + |coef lam_r w|) per element; lam_r = 0: the bits of g.
* head level: device and emulator each hold an rmean within ``rmean_bar`` of the other's at every grid point, so the emulator's
  rmean at the device's choice is at least the emulator's best minus the two points' bars; where the emulator's margin exceeds
  that the choice is forced.  The share of (head, target) pairs with a margin below 100 bars is asserted (at most 1/8; none for
  the plain and the tapped head), as is the validity of ridge_cv_emul's first-order bars for every target.
* all lambdas equal: the scalar path's l2 term is an fp32 sum of R E exact squares in some order times lambda,
  (R E + 4) 2^-24 relative (as tests/test_gpu_ridge_cv_fit.py derives); its gradient seeds with l2coef W and adds the clips'
  terms in fp32: (B + 5) 2^-24 of the terms' magnitudes plus 2^-22 of the value (tests/head_emul.ridge_bwd_w_bars).
"""
import numpy as np
import pytest
import torch

import ridge_cv_emul as CE
import ridge_emul as RE
import ridge_rows_emul as RR
import test_gpu_ridge_fit as RF
from test_gpu_ridge_cv import E_MINI, GRID, V_HEAD, _feed, _st

pytestmark = pytest.mark.gpu
F64, F32, BF16, I32 = torch.float64, torch.float32, torch.bfloat16, torch.int32
WN, BN = RF.WN, RF.BN
SENT = -7.25


def _same(a, b):
    """equal where neither is NaN, NaN in the same places"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


# ---------------------------------------------------------------------------------------------------- 1: the selection kernel
def _select(dev, table, grid, ok):
    from phantom_vlb_amd._lib import check, lib
    K, L, V = table.shape
    t = torch.from_numpy(table).to(dev)
    g = torch.tensor(grid, dtype=F64, device=dev)
    o = torch.tensor([int(x) for x in ok], dtype=I32, device=dev)
    rmean = torch.full((L * V + 8,), SENT, dtype=F64, device=dev)
    choice = torch.full((V + 8,), -77, dtype=I32, device=dev)
    rbest = torch.full((V + 8,), SENT, dtype=F64, device=dev)
    check(lib.vlb_ridge_cv_select(t.data_ptr(), g.data_ptr(), o.data_ptr(), rmean.data_ptr(), choice.data_ptr(), rbest.data_ptr(),
                                  K, L, V, _st()), "vlb_ridge_cv_select")
    torch.cuda.synchronize()
    assert bool((rmean[L * V:] == SENT).all()) and bool((choice[V:] == -77).all()) and bool((rbest[V:] == SENT).all())
    return rmean[:L * V].view(L, V).cpu(), choice[:V].cpu(), rbest[:V].cpu()


@pytest.mark.parametrize("K,L,V", [(5, 7, 40), (2, 2, 1), (3, 10, 257), (1, 1, 1)])
def test_select_kernel_equals_the_emulator(dev, K, L, V):
    rng = np.random.default_rng(K * 100 + L)
    grid = (10.0 ** rng.permutation(np.linspace(-5, 0, L))).tolist()            # unsorted
    base = rng.uniform(-0.3, 0.9, (K, L, V))
    scenarios = []
    if L >= 5:          # everything at once: two pairs of duplicated columns, an excluded NaN column, an excluded column on top
        t = base.copy()
        t[:, 1], t[:, 4] = t[:, 0], t[:, 3]
        t[:, 2], t[:, L - 1] = np.nan, 5.0 + rng.uniform(0, 1, (K, V))
        ok = [1] * L
        ok[2] = ok[L - 1] = 0
        scenarios.append((t, ok))
    else:
        scenarios.append((base.copy(), [1] * L))
        if L == 2:
            t = base.copy()
            t[:, 1] = t[:, 0]
            scenarios.append((t, [1, 1]))                                       # an exact tie
            for fill in (np.nan, 5.0):
                t = base.copy()
                t[:, 0] = fill
                scenarios.append((t, [0, 1]))
    scenarios.append((base.copy(), [0] * L))                                     # nothing allowed: -1, NaN
    for t, ok in scenarios:
        rmean, choice, rbest = _select(dev, t, grid, ok)
        emu = RR.select_rows(t, grid, ok)
        assert torch.equal(choice, torch.from_numpy(emu["choice"])), (choice.tolist(), emu["choice"].tolist())
        assert _same(rmean, torch.from_numpy(emu["rmean"])) and _same(rbest, torch.from_numpy(emu["rbest"]))
        if any(ok):
            assert all(ok[c] for c in choice.tolist())
    if L >= 5:          # the duplicated pairs tie exactly: whoever chose one of a pair chose the larger lambda
        t, ok = scenarios[0]
        _, choice, _ = _select(dev, t, grid, ok)
        picked = set(choice.tolist())
        assert picked & {0, 1, 3, 4}, "no target chose a duplicated column: choose other inputs"
        for a, b in ((0, 1), (3, 4)):
            assert (b if grid[a] > grid[b] else a) not in picked


# ---------------------------------------------------------------------------------------------------- 2: the row-masked solve
def _sums(dev, E, V, N, seed):
    from phantom_vlb_amd._lib import check, lib
    gen = torch.Generator().manual_seed(seed)
    z = (torch.randn(N, E, generator=gen) + 0.5).to(BF16).to(dev)
    y = (torch.randn(N, V, generator=gen) * 2 + 0.3).to(dev)
    s = dict(G=torch.zeros(E, E, dtype=F64, device=dev), C=torch.zeros(V, E, dtype=F64, device=dev),
             sz=torch.zeros(E, dtype=F64, device=dev), sy=torch.zeros(V, dtype=F64, device=dev))
    check(lib.vlb_ridge_gram_accumulate(z.data_ptr(), y.data_ptr(), V, s["G"].data_ptr(), s["C"].data_ptr(), s["sz"].data_ptr(),
                                        s["sy"].data_ptr(), N, E, V, _st()), "vlb_ridge_gram_accumulate")
    return s


def _solve(dev, s, N, lam, E, V, choice=None, want=0, W=None, b=None):
    from phantom_vlb_amd._lib import check, lib
    A, X = torch.empty(E, E, dtype=F64, device=dev), torch.empty(V, E, dtype=F64, device=dev)
    W = torch.full((V, E), SENT, dtype=F32, device=dev) if W is None else W
    b = torch.full((V,), SENT, dtype=F32, device=dev) if b is None else b
    info = torch.full((1,), 77, dtype=I32, device=dev)
    args = (s["G"].data_ptr(), s["C"].data_ptr(), s["sz"].data_ptr(), s["sy"].data_ptr(), N, lam, A.data_ptr(), X.data_ptr(),
            W.data_ptr(), b.data_ptr(), info.data_ptr(), E, V)
    if choice is None:
        check(lib.vlb_ridge_solve(*args, _st()), "vlb_ridge_solve")
    else:
        check(lib.vlb_ridge_solve_rows(*args, choice.data_ptr(), want, _st()), "vlb_ridge_solve_rows")
    torch.cuda.synchronize()
    return W, b, int(info)


@pytest.mark.parametrize("E,V,N", [(200, 70, 37), (64, 64, 2), (1, 1, 2), (257, 5, 9)])
def test_solve_rows_writes_the_plain_solves_rows_and_nothing_else(dev, E, V, N):
    lams = [1e-2, 1e-1, 1.0]                                  # grid point 1 is chosen by no row
    s = _sums(dev, E, V, N, seed=E + V)
    gen = torch.Generator().manual_seed(V)
    choice_h = torch.randint(0, 2, (V,), generator=gen).to(I32) * 2
    if V > 1:
        choice_h[0], choice_h[-1] = 0, 2
    choice = choice_h.to(dev)
    plain = {}
    for i, lam in enumerate(lams):
        W, b, info = _solve(dev, s, N, lam, E, V)
        assert info == 0 and not bool((W == SENT).any()) and not bool((b == SENT).any())
        plain[i] = (W, b)
    # one call: exactly its rows are written, with the plain solve's bits
    W, b, info = _solve(dev, s, N, lams[0], E, V, choice, 0)
    mine = choice == 0
    assert info == 0
    assert torch.equal(W[mine], plain[0][0][mine]) and torch.equal(b[mine], plain[0][1][mine])
    assert bool((W[~mine] == SENT).all()) and bool((b[~mine] == SENT).all())
    # the unused grid point writes nothing; the other used one completes the result
    before = (W.clone(), b.clone())
    _, _, info = _solve(dev, s, N, lams[1], E, V, choice, 1, W, b)
    assert info == 0 and torch.equal(W, before[0]) and torch.equal(b, before[1])
    _, _, info = _solve(dev, s, N, lams[2], E, V, choice, 2, W, b)
    assert info == 0 and not bool((W == SENT).any()) and not bool((b == SENT).any())
    for v in range(V):
        i = int(choice_h[v])
        assert torch.equal(W[v], plain[i][0][v]) and torch.equal(b[v], plain[i][1][v]), v


def test_solve_rows_with_a_failed_factorisation_writes_nothing(dev):
    """test_gpu_ridge_cv's construction: N = 37 < E = 200 leaves the centred Gram matrix with rank 36 at most and a ridge term
    of 1e-30 N V is far below its rounding, so a pivot past the rank comes out non-positive.  Valid memory throughout."""
    E, V, N = 200, 70, 37
    s = _sums(dev, E, V, N, seed=3)
    choice = torch.zeros(V, dtype=I32, device=dev)
    W, b, info = _solve(dev, s, N, 1e-30, E, V, choice, 0)
    assert info > 0
    assert bool((W == SENT).all()) and bool((b == SENT).all())


# ---------------------------------------------------------------------------------------------------- 3: the l2 entries
def _l2_inputs(dev, R, E, seed):
    gen = torch.Generator().manual_seed(seed)
    W = (torch.randn(R, E, generator=gen) / E ** 0.5).to(BF16)
    lam = (10.0 ** (torch.rand(R, generator=gen) * 4 - 4)).float()
    if R > 1:
        lam[torch.randperm(R, generator=gen)[:max(1, R // 5)]] = 0.0
    g = torch.randn(R, E, generator=gen)
    return W, lam, g


def _l2_fwd(dev, W, lam, mse=0.37):
    from phantom_vlb_amd._lib import check, lib
    R, E = W.shape
    n = lib.vlb_head_l2_rows_ws_doubles(R)
    ws = torch.full((n + 8,), SENT, dtype=F64, device=dev)
    terms = torch.tensor([mse, SENT, SENT], dtype=F32, device=dev)
    check(lib.vlb_head_l2_rows_fwd(W.data_ptr(), lam.data_ptr(), ws.data_ptr(), terms.data_ptr(), R, E, _st()), "vlb_head_l2_rows_fwd")
    torch.cuda.synchronize()
    assert bool((ws[n:] == SENT).all()), "the workspace query is smaller than what the kernel writes"
    return terms.cpu()


def _l2_bwd(dev, W, lam, g, coef):
    from phantom_vlb_amd._lib import check, lib
    R, E = W.shape
    d = torch.cat([g.flatten(), torch.full((8,), SENT)]).to(dev)
    check(lib.vlb_head_l2_rows_bwd(W.data_ptr(), lam.data_ptr(), d.data_ptr(), R, E, coef, _st()), "vlb_head_l2_rows_bwd")
    torch.cuda.synchronize()
    assert bool((d[R * E:] == SENT).all())
    return d[:R * E].view(R, E).cpu()


@pytest.mark.parametrize("R,E", [(40, 96), (1, 8), (257, 4096), (3 * 24, 512)])
def test_l2_rows_entries_against_the_emulator(dev, R, E):
    W, lam, g = _l2_inputs(dev, R, E, seed=R + E)
    Wd, lamd = W.to(dev), lam.to(dev)
    Wn, lamn = W.float().numpy().astype(np.float64), lam.numpy()
    # ---- forward
    terms = _l2_fwd(dev, Wd, lamd)
    want = RR.l2_rows(Wn, lamn)
    err, bar = abs(float(terms[1].double()) - want), RR.l2_bar(R, E, want)
    print(f"R={R} E={E}: l2 {float(terms[1]):.6e}, err / bar {err / bar:.3f}")
    assert want > 0 and err <= bar
    assert terms[0].item() == np.float32(0.37) and torch.equal(terms[2], terms[0] + terms[1])
    assert torch.equal(_l2_fwd(dev, Wd, lamd).view(I32), terms.view(I32))                       # two runs, the same bits
    zero = _l2_fwd(dev, Wd, torch.zeros_like(lamd))
    assert float(zero[1]) == 0.0 and torch.equal(zero[2], zero[0])
    # ---- backward on top of a random gradient
    coef = 2.0 * 0.25
    d = _l2_bwd(dev, Wd, lamd, g, coef)
    term = RR.l2_rows_grad(Wn, lamn, coef)
    derr = np.abs(d.double().numpy() - (g.double().numpy() + term))
    gbar = RR.grad_bar(g.numpy(), term)
    live = lamn != 0
    print(f"R={R} E={E}: gradient max err / bar {np.max(derr[live] / gbar[live]):.3f}; {int((~live).sum())} rows with lambda 0")
    assert np.all(derr <= gbar)
    assert torch.equal(d[~torch.from_numpy(live)].view(I32), g[~torch.from_numpy(live)].view(I32))
    assert bool((d[torch.from_numpy(live)] != g[torch.from_numpy(live)]).any())
    assert torch.equal(_l2_bwd(dev, Wd, lamd, g, coef).view(I32), d.view(I32))


# ---------------------------------------------------------------------------------------------------- 4: head level
#           N               K  block  seed
KINDS = {"plain": ((300,), 5, 7, 11),
         "taps": ((300,), 4, 16, 12),
         "subjects": ((120, 60, 45), 3, 3, 13)}
NOISE = (0.2, 20.0)                     # the targets' noise sd: geomspace over two decades, permuted
_CACHE = {}


def _make(kind, dev):
    """test_gpu_ridge_cv._make with a noise sd per target; -> head, cache, z (host fp64), y (device), subject, K, block"""
    from phantom_vlb_amd.feature_cache import FeatureCache
    from phantom_vlb_amd.head import LAYER_MIX, BrainHead
    counts, K, block, seed = KINDS[kind]
    gen = torch.Generator(device="cpu").manual_seed(seed)
    N = sum(counts)
    kw, layers = {}, None
    if kind == "taps":
        kw, layers = dict(readout_layers=[1, 2, 4]), 3
    if kind == "subjects":
        kw = dict(subjects=["s-a", "s-b", "s-c"])
    head = BrainHead(E_MINI, V_HEAD, 1e-3, 1e-5, dev, seed=5, **kw)
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
    if kind == "subjects":
        subject = torch.cat([torch.full((c,), g) for g, c in enumerate(counts)]).long()[torch.randperm(N, generator=gen)]
    z = head.features_cached(cache, torch.arange(N))[:N].float().cpu().double()
    mix = torch.zeros(E_MINI, V_HEAD, dtype=F64)
    mix[:16] = torch.randn(16, V_HEAD, generator=gen, dtype=F64)
    sd = torch.from_numpy(np.geomspace(NOISE[0], NOISE[1], V_HEAD))[torch.randperm(V_HEAD, generator=gen)]
    y = (z @ mix + sd * torch.randn(N, V_HEAD, generator=gen, dtype=F64) + 0.2).float().to(BF16).float().to(dev).contiguous()
    return head, cache, z.numpy(), y, subject, K, block


def _fitted(kind, dev):
    """the head of ``kind`` with its folds fed, and the emulator's fit of the same clips (computed once per kind)"""
    if kind not in _CACHE:
        head, cache, z, y, subject, K, block = _make(kind, dev)
        sub = None if subject is None else subject.numpy()
        emu = RR.fit(z, y.double().cpu().numpy(), GRID, K, block, chunk=64, sub=sub, bars=True)
        _CACHE[kind] = dict(head=head, cache=cache, z=z, y=y, subject=subject, sub=sub, K=K, block=block, emu=emu,
                            start={n: t.clone() for n, t in head.master.items()})
    c = _CACHE[kind]
    head = c["head"]
    head.set_l2_lambda_rows(None)
    for n, t in c["start"].items():
        head.master[n].copy_(t)
        head.compute[n].copy_(t)
    return c


@pytest.mark.parametrize("kind", list(KINDS))
def test_whole_head_chooses_and_solves_per_target(dev, kind):
    c = _fitted(kind, dev)
    head, emu, z, sub = c["head"], c["emu"], c["z"], c["sub"]
    H, V, E, L = max(1, head.G), V_HEAD, E_MINI, len(GRID)
    _feed(head, c["cache"], c["y"], c["subject"], c["K"], c["block"])
    plain_cv = head.ridge_cv(GRID)
    cv = head.ridge_cv(GRID, per_target=True)
    torch.cuda.synchronize()
    assert all(torch.equal(head.master[n], t) for n, t in c["start"].items()), "ridge_cv wrote a parameter"
    # ---- what ridge_cv returned before is unchanged
    for k in ("grid", "score", "score_per_head", "best_index", "best_lambda", "infos"):
        assert cv[k] == plain_cv[k], k
    assert torch.equal(cv["r"], plain_cv["r"]) and set(cv) - set(plain_cv) == {"choice", "lambda_rows", "lambda_counts", "score_per_target"}
    # ---- the device's table passes the parent's bars
    ecv = emu["cv"]
    assert ecv["valid"].all(), "a target outside the first-order formula's validity: choose other inputs"
    table = head._ridge["cv_table"].cpu().numpy()
    assert np.all(np.abs(table - ecv["r"]) <= ecv["r_bar"])
    # ---- the condition on the inputs: the margins are wide for (nearly) every pair
    m, bar = emu["margins"], emu["rmean_bar"]
    thin = m < 100
    print(f"{kind}: {int(thin.sum())} of {m.size} (head, target) pairs below 100 bars, min margin {m.min():.0f}; emulator counts "
          f"{emu['lambda_counts'].tolist()}, global choice {ecv['best_index']}")
    assert thin.mean() <= 1 / 8, "the inputs do not separate the targets' best two grid points: choose other inputs"
    if kind != "subjects":
        assert not thin.any(), "the inputs do not separate the targets' best two grid points: choose other inputs"
    # ---- every (head, target): the emulator's rmean at the device's choice is its best, less the two points' bars
    choice = cv["choice"]
    assert choice.dtype == I32 and choice.is_cuda and tuple(choice.shape) == (H, V)
    ch = choice.cpu().numpy()
    rmean_dev = head._ridge["cv_rmean"].cpu().numpy()
    assert np.all(np.abs(rmean_dev - emu["rmean"]) <= bar)
    hh, vv = np.meshgrid(np.arange(H), np.arange(V), indexing="ij")
    at_dev, at_emu = emu["rmean"][hh, ch, vv], emu["rmean"][hh, emu["choice"], vv]
    assert np.all(at_dev >= at_emu - (bar[hh, ch, vv] + bar[hh, emu["choice"], vv]))
    assert np.array_equal(ch[~thin], emu["choice"][~thin])            # forced wherever the margin exceeds the two bars
    assert len(set(ch.flatten().tolist())) >= 3
    # ---- the rest of the dict
    lam_rows = cv["lambda_rows"]
    assert lam_rows.dtype == F32 and lam_rows.is_cuda and tuple(lam_rows.shape) == (H, V)
    assert torch.equal(lam_rows.cpu(), torch.tensor(GRID, dtype=F64).float()[torch.from_numpy(ch).long()])
    assert cv["lambda_counts"] == [np.bincount(ch[g], minlength=L).tolist() for g in range(H)]
    assert abs(cv["score_per_target"] - rmean_dev[hh, ch, vv].mean()) <= (H * V + 2) * 2.0 ** -52
    assert abs(cv["score_per_target"] - emu["score_per_target"]) <= bar.max() + (H * V + 2) * 2.0 ** -52
    # ---- ridge_solve_rows: every row has the bits of ridge_solve with its lambda, on the same sums
    rows_of = {}
    for i in sorted(set(ch.flatten().tolist())):
        head.ridge_solve(GRID[i])
        rows_of[i] = (head.master[WN].clone().view(H, V, E), head.master[BN].clone().view(H, V))
    for n, t in c["start"].items():
        head.master[n].copy_(t)
        head.compute[n].copy_(t)
    out = head.ridge_solve_rows(choice, GRID)
    torch.cuda.synchronize()
    assert [o["lambda_counts"] for o in out] == cv["lambda_counts"] and all(o["info"] == 0 and "l2_lambda" not in o for o in out)
    Wm, bm = head.master[WN].view(H, V, E), head.master[BN].view(H, V)
    yh = c["y"].double().cpu().numpy()
    for g in range(H):
        rows = np.arange(len(z)) if sub is None else np.nonzero(sub == g)[0]
        assert out[g]["n"] == len(rows)
        sums = RE.sums(z[rows], yh[rows], chunk=512)
        worst = 0.0
        for v in range(V):
            i = int(ch[g, v])
            assert torch.equal(Wm[g, v], rows_of[i][0][g, v]) and torch.equal(bm[g, v], rows_of[i][1][g, v]), (g, v)
        for i in sorted(set(ch[g].tolist())):
            sol = RE.solve(sums, GRID[i])
            mine = ch[g] == i
            dW = np.abs(Wm[g].cpu().numpy().astype(np.float64) - sol["W"].astype(np.float32).astype(np.float64))[mine]
            worst = max(worst, float(np.max(dW / RE.master_bar(sol["W"], RE.cond2(sol["A"]), E)[mine])))
        print(f"{kind} head {g}: max |dW| / master_bar {worst:.3f}")
        assert worst <= 1
    for n in (WN, BN):
        assert np.array_equal(head.compute[n].float().cpu().numpy(), RE.rne_bf16(head.master[n].cpu().numpy()))
    for n in c["start"]:
        if n not in (WN, BN):
            assert torch.equal(head.master[n], c["start"][n])
    head.ridge_stats_end()


def test_a_failed_solve_leaves_every_parameter(dev):
    """N = 300 < E = 512: with 1e-30 in the grid the totals' factorisation fails (test_gpu_ridge_cv's construction)"""
    c = _fitted("plain", dev)
    head = c["head"]
    _feed(head, c["cache"], c["y"], c["subject"], c["K"], c["block"])
    grid = [1e-30] + GRID[1:]
    choice = torch.ones(1, V_HEAD, dtype=I32, device=dev)
    choice[0, 5] = 0
    with pytest.raises(ValueError, match=r"the head, l2_lambda = 1e-30 \(grid point 0\): pivot \d+ of 512"):
        head.ridge_solve_rows(choice, grid)
    torch.cuda.synchronize()
    assert all(torch.equal(head.master[n], t) for n, t in c["start"].items())
    assert all(torch.equal(head.compute[n], c["start"][n].to(BF16)) for n in c["start"])
    head.ridge_stats_end()


# ---------------------------------------------------------------------------------------------------- 5: the step
def _calls(kind, c, dev):
    """name -> (forward, backward) for every path the head of ``kind`` has, on one batch of B = 4"""
    from phantom_vlb_amd import ops
    head, cache, y = c["head"], c["cache"], c["y"]
    B, S, E = 4, 24, E_MINI
    gen = torch.Generator().manual_seed(7)
    idx = torch.tensor([3, 17, 40, 8])
    yb = y[idx.to(dev)].contiguous()
    sub = None if c["subject"] is None else c["subject"][idx]
    lens = [24, 9, 17, 24]
    hidden = (torch.randn(B, S, E, generator=gen) * 2).to(BF16)
    wm = torch.rand(B, S, generator=gen) * 0.1
    for b_, n in enumerate(lens):
        wm[b_, max(n - 4, 0):] = 0
    packed = torch.cat([hidden[b_, :n] for b_, n in enumerate(lens)], 0).contiguous().to(dev)
    hd, wd = hidden.view(B * S, E).to(dev), wm.to(dev)
    calls = {}
    if kind == "taps":
        calls["cached"] = (lambda: head.forward_cached(cache, idx, yb), lambda s: head.backward_tapped(loss_scale=s, l2_scale=s))

        def tapped():
            head.begin(B, S)
            for i in range(3):
                head.tap(i, hd * (1 + 0.25 * i), wd)
            return head.forward_tapped(yb)
        calls["tapped"] = (tapped, lambda s: head.backward_tapped(loss_scale=s, l2_scale=s))
        return calls, B
    calls["plain" if sub is None else "grouped"] = (lambda: head.forward(hd, wd, yb, subject=sub),
                                                    lambda s: head.backward(True, loss_scale=s, l2_scale=s))
    calls["packed"] = (lambda: head.forward(packed, wd, yb, layout=ops.RowLayout(B, S, lens, device=dev), subject=sub),
                       lambda s: head.backward(True, loss_scale=s, l2_scale=s))
    calls["cached"] = (lambda: head.forward_cached(cache, idx, yb, subject=sub), lambda s: head.backward_cached(loss_scale=s, l2_scale=s))
    return calls, B


def _run(head, fwd, bwd, scale):
    _, terms = fwd()
    terms = terms.clone()
    bwd(scale)
    torch.cuda.synchronize()
    return terms.cpu(), {n: t.clone() for n, t in head.grads.items()}


def _clip_terms_magnitude(head, y, subject, scale):
    """sum_b |dp[b,v]| |z[b,e]| over the clips of each row's head, [R,E]: what the data term of d_ridge_w is made of
    (dp = loss_scale 2 / (B V) (pred - y); z: what the ridge layer read in the last forward, no dropout)"""
    B, V = y.shape
    dp = (scale * 2.0 / (B * V) * (head.pred.double() - y.double())).abs().cpu()
    z = head.z[:B].float().double().abs().cpu()
    H = max(1, head.G)
    out = torch.zeros(H, V, head.E, dtype=F64)
    for g in range(H):
        rows = torch.arange(B) if subject is None else torch.nonzero(subject == g).flatten()
        out[g] = dp[rows].t() @ z[rows]
    return out.view(H * V, head.E).numpy()


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_step_carries_the_penalty_per_row_on_every_path(dev, kind):
    c = _fitted(kind, dev)
    head = c["head"]
    H, V, E = max(1, head.G), V_HEAD, E_MINI
    R = H * V
    gen = torch.Generator().manual_seed(3)
    lam = (10.0 ** (torch.rand(R, generator=gen) * 4 - 4)).float()
    lam[torch.randperm(R, generator=gen)[:R // 6]] = 0.0
    lamd = lam.to(dev)
    Wn = head.compute[WN].float().cpu().numpy().astype(np.float64).reshape(R, E)
    want = RR.l2_rows(Wn, lam.numpy())
    scale = 0.5
    term = RR.l2_rows_grad(Wn, lam.numpy(), 2.0 * scale)
    calls, B = _calls(kind, c, dev)
    idx = torch.tensor([3, 17, 40, 8])                                   # _calls' batch
    yb, subb = c["y"][idx.to(dev)], None if c["subject"] is None else c["subject"][idx]
    for name, (fwd, bwd) in calls.items():
        was = head.l2_lambda
        head.l2_lambda = 0.0
        t0, g0 = _run(head, fwd, bwd, scale)
        head.l2_lambda = was
        assert float(t0[1]) == 0.0 and torch.equal(t0[2], t0[0])
        scalar, gs = _run(head, fwd, bwd, scale)                        # the scalar path, as it is without the vector
        head.set_l2_lambda_rows(lamd)
        t1, g1 = _run(head, fwd, bwd, scale)
        t1b, g1b = _run(head, fwd, bwd, scale)
        assert torch.equal(t1[0].view(I32), t0[0].view(I32)), name
        err, bar = abs(float(t1[1].double()) - want), RR.l2_bar(R, E, want)
        assert err <= bar, (name, err, bar)
        assert torch.equal(t1[2], t1[0] + t1[1])
        dW = g1[WN].double().cpu().numpy().reshape(R, E)
        dW0 = g0[WN].double().cpu().numpy().reshape(R, E)
        gbar = RR.grad_bar(dW0, term)
        assert np.all(np.abs(dW - (dW0 + term)) <= gbar), name
        assert torch.equal(g1[WN].view(R, E)[lam == 0], g0[WN].view(R, E)[lam == 0])
        for n in g0:
            if n != WN:
                assert torch.equal(g1[n], g0[n]), (name, n)
        assert torch.equal(t1b.view(I32), t1.view(I32)) and all(torch.equal(g1b[n], g1[n]) for n in g1)
        # ---- all lambdas equal: the scalar path at that lambda, to the sum of both paths' bars
        lam_s = head.l2_lambda
        head.set_l2_lambda_rows(torch.full((R,), lam_s, dtype=F32, device=dev))
        t2, g2 = _run(head, fwd, bwd, scale)
        l2_s = float(np.float32(lam_s)) * float((Wn * Wn).sum())
        assert abs(float(t2[1].double()) - float(scalar[1].double())) <= RR.l2_bar(R, E, l2_s) + (R * E + 4) * 2.0 ** -24 * l2_s
        assert torch.equal(t2[0], scalar[0])
        seed_s = 2.0 * scale * float(np.float32(lam_s)) * Wn
        mag = _clip_terms_magnitude(head, yb, subb, scale) + np.abs(seed_s)
        dWs, dW2 = (x[WN].double().cpu().numpy().reshape(R, E) for x in (gs, g2))
        sbar = (B + 5) * 2.0 ** -24 * mag + 2.0 ** -22 * np.abs(dWs)
        assert np.all(np.abs(dW2 - dWs) <= RR.grad_bar(dW0, seed_s) + sbar), name
        for n in g0:
            if n != WN:
                assert torch.equal(g2[n], gs[n]), (name, n)
        # ---- clearing the vector restores the scalar path's bits
        head.set_l2_lambda_rows(None)
        t3, g3 = _run(head, fwd, bwd, scale)
        assert torch.equal(t3.view(I32), scalar.view(I32)) and all(torch.equal(g3[n], gs[n]) for n in gs), name
        print(f"{kind}/{name}: l2 err / bar {err / bar:.3f}, dW err / bar {np.max(np.abs(dW - (dW0 + term))[lam.numpy() != 0] / gbar[lam.numpy() != 0]):.3f}")


def test_heads_of_the_correlation_objectives_refuse_the_vector(dev):
    from phantom_vlb_amd.head import BrainHead
    for loss in ("cosine", "pearson"):
        h = BrainHead(64, 8, 1e-3, 1e-5, dev, loss=loss)
        with pytest.raises(ValueError, match="mse"):
            h.set_l2_lambda_rows(torch.full((8,), 1e-3, device=dev))
        assert h.l2_lambda_rows is None
    h = BrainHead(64, 8, 1e-3, 1e-5, dev)
    for bad in (torch.full((7,), 1e-3, device=dev), torch.full((8,), -1e-3, device=dev), torch.full((8,), float("nan"), device=dev),
                torch.full((8,), 1e-3, device=dev, dtype=F64)):
        with pytest.raises(ValueError, match="set_l2_lambda_rows"):
            h.set_l2_lambda_rows(bad)


# ---------------------------------------------------------------------------------------------------- 6: through the module
MGRID = [1e-4, 1e-2, 1.0]


def _module_fit(subjects, epochs=2):
    from phantom_vlb_amd.litmodule import VLBLitModule
    from phantom_vlb_amd.trainer import Trainer
    m = VLBLitModule(RF._cfg(subjects=subjects, cache_features=True, ridge_fit="closed_form", dropout_rate=0.0, l2_lambda=3e-3,
                             ridge_lambda_grid=MGRID, ridge_cv_folds=2, ridge_cv_block=2, ridge_lambda_per_target=True))
    m.configure_model()
    dm = RF._dm(subjects)
    fits, steps = [], []
    orig, ts = m.fit_ridge_closed_form, m.training_step

    def fit_spy(*a, **k):
        out = orig(*a, **k)
        torch.cuda.synchronize()
        rec = dict(global_step=tr.global_step, steps_before=len(steps), out=out, result=m.ridge_fit_result,
                   masters={n: t.clone() for n, t in m.head.master.items()},
                   logged={k2: v for k2, v in m.logged.items() if k2.startswith("ridge_fit/")})
        # a twin head on the same cache and clips: ridge_cv(per_target=True) + ridge_solve_rows called directly
        from phantom_vlb_amd.head import BrainHead
        from phantom_vlb_amd.litmodule import check_batch_subjects
        h = m.head
        twin = BrainHead(h.E, h.V, 3e-3, h.eps, h.dev, sd={n: t.clone() for n, t in h.master.items()}, subjects=subjects)
        for n in RF.LN:                                     # the LN parameters as the fit saw them (the fit does not touch them)
            twin.compute[n].copy_(h.compute[n])
        ds, cache = dm.datasets.train, m.feature_caches["train"]
        was = ds.features_only
        ds.features_only = True
        items = [ds[i] for i in range(len(ds))]
        ds.features_only = was
        batch = {k2: torch.stack([torch.as_tensor(it[k2]) for it in items]) for k2 in items[0]}
        y = batch["timeseries"].to(h.dev, F32).to(BF16).float().contiguous()
        twin.ridge_stats_begin(folds=2, block=2)
        twin.ridge_stats_add(cache, batch["index"], y, check_batch_subjects(batch, subjects, len(items)))
        tcv = twin.ridge_cv(MGRID, per_target=True)
        twin.ridge_solve_rows(tcv["choice"], MGRID)
        torch.cuda.synchronize()
        rec["twin"] = {n: t.clone() for n, t in twin.master.items()}
        rec["twin_choice"] = tcv["choice"].clone()
        fits.append(rec)
        return out

    def step_spy(batch):
        rec = dict(W=m.head.compute[WN].float().cpu().double(), rows=None if m.head.l2_lambda_rows is None else m.head.l2_lambda_rows.cpu())
        loss = ts(batch)
        rec["terms"] = m.head.loss_terms.double().cpu()
        steps.append(rec)
        return loss
    m.fit_ridge_closed_form, m.training_step = fit_spy, step_spy
    log = RF._Rec()
    tr = Trainer(max_epochs=epochs, val_check_interval=0.5, log_every_n_steps=1, logger=log)
    tr.fit(m, dm)
    torch.cuda.synchronize()
    return dict(module=m, dm=dm, fits=fits, steps=steps, rows=log.rows)


def _val_loss(m, dm):
    ds = dm.datasets.val
    was = ds.features_only
    ds.features_only = False                                             # whole clips: every module runs the backbone on them
    try:
        batch = next(iter(dm.val_dataloader()))
    finally:
        ds.features_only = was
    batch = {k: v for k, v in batch.items() if k != "index"}            # ... and none looks into a cache
    out = m.validation_step(m.transfer_batch_to_device(batch, m.device, 0))
    torch.cuda.synchronize()
    return out["loss"].cpu(), m.head.loss_terms.cpu().clone()


@pytest.mark.parametrize("subjects", [None, ["sub-01", "sub-02"]])
def test_the_option_through_the_module_and_both_checkpoint_routes(dev, tmp_path, subjects):
    from phantom_vlb_amd.litmodule import VLBLitModule
    from phantom_vlb_amd.trainer import load_trainable_checkpoint, trainable_state
    run = _module_fit(subjects)
    m = run["module"]
    H, V, L = 1 if subjects is None else len(subjects), 128, len(MGRID)
    assert len(run["fits"]) == 1                            # once
    f = run["fits"][0]
    cv = f["result"]
    choice = cv["choice"].cpu().long()
    rows = torch.tensor(MGRID, dtype=F64).float()[choice].flatten()
    # ---- the head holds grid[choice]; the scalar keeps the global choice
    assert torch.equal(m.head.l2_lambda_rows.cpu(), rows) and m.head.l2_lambda == cv["best_lambda"] == MGRID[cv["best_index"]]
    assert torch.equal(cv["lambda_rows"].cpu().flatten(), rows)
    # ---- the masters are a direct ridge_cv(per_target=True) + ridge_solve_rows on a twin head, bit for bit
    assert torch.equal(f["twin_choice"], cv["choice"])
    for n in (WN, BN):
        assert torch.equal(f["masters"][n], f["twin"][n]), n
    # ---- the log
    lg = f["logged"]
    counts = [lg[f"ridge_fit/lambda_count_{i}"] for i in range(L)]
    assert sum(counts) == H * V and counts == [float(sum(r[i] for r in cv["lambda_counts"])) for i in range(L)]
    assert lg["ridge_fit/cv_score_per_target"] == cv["score_per_target"] and lg["ridge_fit/l2_lambda"] == cv["best_lambda"]
    assert lg["ridge_fit/cv_best_index"] == cv["best_index"] and lg["ridge_fit/cv_score"] == cv["score"][cv["best_index"]]
    assert [o["lambda_counts"] for o in f["out"]] == cv["lambda_counts"] and cv["solve"] == f["out"]
    sent = [r for r in run["rows"] if any(k.startswith("ridge_fit/") for k in r)]
    assert len(sent) == 1 and sent[0]["ridge_fit/cv_score_per_target"] == cv["score_per_target"]
    assert [sent[0][f"ridge_fit/lambda_count_{i}"] for i in range(L)] == counts
    # ---- the next training step's l2 term is the vector's
    s = run["steps"][f["steps_before"]]
    assert s["rows"] is not None and torch.equal(s["rows"], rows)
    assert all(st["rows"] is None for st in run["steps"][:f["steps_before"]])
    Wn = s["W"].numpy().reshape(H * V, -1)
    want = RR.l2_rows(Wn, rows.numpy())
    got = float(s["terms"][1])
    print(f"subjects={subjects}: counts {counts}, global choice {cv['best_index']}, next step l2 {got:.6e}, err / bar "
          f"{abs(got - want) / RR.l2_bar(H * V, Wn.shape[1], want):.3f}")
    assert abs(got - want) <= RR.l2_bar(H * V, Wn.shape[1], want)
    # ---- both checkpoint routes restore the vector bit for bit and reproduce the next validation loss bit for bit
    ref_loss, ref_terms = _val_loss(m, run["dm"])
    cfg = dict(subjects=subjects, cache_features=True, ridge_fit="closed_form", dropout_rate=0.0, l2_lambda=3e-3,
               ridge_lambda_grid=MGRID, ridge_cv_folds=2, ridge_cv_block=2, ridge_lambda_per_target=True)
    ck = {}
    m.on_save_checkpoint(ck)
    ck["state_dict"] = {k: v.clone() for k, v in m.state_dict().items()}
    assert torch.equal(ck["vlb_ridge_l2_lambda_rows"], rows) and ck["vlb_ridge_l2_lambda"] == cv["best_lambda"]
    m2 = VLBLitModule(RF._cfg(**cfg))
    m2.on_load_checkpoint({k: v for k, v in ck.items() if k.startswith("vlb_ridge")})         # before the head exists ...
    m2.configure_model()
    assert torch.equal(m2.head.l2_lambda_rows.cpu().view(I32), rows.view(I32)) and m2.head.l2_lambda == cv["best_lambda"]
    m2.head.set_l2_lambda_rows(None)
    m2.on_load_checkpoint(ck)                                                                    # ... and after
    m2.load_state_dict(ck["state_dict"])
    assert torch.equal(m2.head.l2_lambda_rows.cpu().view(I32), rows.view(I32))
    loss2, terms2 = _val_loss(m2, run["dm"])
    assert torch.equal(loss2.view(I32), ref_loss.view(I32)) and torch.equal(terms2.view(I32), ref_terms.view(I32))
    st = trainable_state(m, 8)
    assert torch.equal(st["ridge_l2_lambda_rows"], rows) and st["ridge_l2_lambda"] == cv["best_lambda"]
    path = str(tmp_path / "last.ckpt")
    torch.save(st, path)
    m3 = VLBLitModule(RF._cfg(**cfg))
    m3.configure_model()
    m3.configure_optimizers()
    assert m3.head.l2_lambda_rows is None
    assert load_trainable_checkpoint(m3, path) == 8
    assert torch.equal(m3.head.l2_lambda_rows.cpu().view(I32), rows.view(I32)) and m3.head.l2_lambda == cv["best_lambda"]
    loss3, terms3 = _val_loss(m3, run["dm"])
    assert torch.equal(loss3.view(I32), ref_loss.view(I32)) and torch.equal(terms3.view(I32), ref_terms.view(I32))


def test_an_explicit_lambda_skips_the_grid_and_clears_the_vector(dev):
    from phantom_vlb_amd.trainer import trainable_state
    run = _module_fit(None, epochs=2)
    m = run["module"]
    assert m.head.l2_lambda_rows is not None
    from phantom_vlb_amd.litmodule import VLBLitModule
    out = VLBLitModule.fit_ridge_closed_form(m, run["dm"].datasets.train, l2_lambda=1e-2)
    torch.cuda.synchronize()
    assert m.head.l2_lambda_rows is None and [o["l2_lambda"] for o in out] == [1e-2]
    ck = {}
    m.on_save_checkpoint(ck)
    assert "vlb_ridge_l2_lambda_rows" not in ck and "ridge_l2_lambda_rows" not in trainable_state(m, 8)
