"""Blocked K-fold cross-validation of ``l2_lambda`` on the device: the new entries of csrc/ridge_solve.hip
alone, then ``BrainHead.ridge_stats_begin(folds=...) / ridge_cv / ridge_solve`` on a plain head, a head with three tapped layers
and three per-subject heads, against tests/ridge_cv_emul.py.

Bars (derived in ridge_cv_emul's docstring; none is fitted to what the device returns):
* integer inputs (z in [-3,3], y in [-4,4]): every sum is an integer far below 2^53 - ``torch.equal`` under any chunking, any K.
* Gc, Rc, vy: forming (5 u (|G| + |sz||sz|^T / n)) plus the accumulation bars of the sums.
* r of the score kernel: the DEVICE's own X, read back, is scored by the emulator (extended precision), so the bar is the
  quadratic form's gamma_{2E+4} |x|^T|Gc||x|, the dot product's gamma_{E+4} |x|.|Rc_v|, the propagated moment bars and vy's,
  through the first-order formula - independent of cond(A).  Every target must be inside the formula's validity (asserted).
* head level: device and emulator each solve for their own X: ``dx_bar`` (2 solve_bar + the systems' forming bars, through
  |A^-1|) is added; the chosen index is compared only after the emulator's best score leads its runner-up by 100 score bars.
"""
import warnings

import numpy as np
import pytest
import torch

import ridge_cv_emul as CE
import ridge_emul as RE

pytestmark = pytest.mark.gpu
F64, BF16 = torch.float64, torch.bfloat16
WN, BN = "ridge_layer.linear.weight", "ridge_layer.linear.bias"
#        E    V   n_k
CASES = [(200, 70, 37),      # ragged tiles on both axes, a partial FK slice (200 = 12 * 16 + 8)
         (64, 64, 2),        # exact tiles
         (1, 1, 2),          # one target, one thread's column
         (257, 5, 9)]        # four column tiles plus one column: the multi-partial finish


def _st():
    return torch.cuda.current_stream().cuda_stream


def _fold_state(K, E, V, dev):
    return dict(G=torch.zeros(K, E, E, dtype=F64, device=dev), C=torch.zeros(K, V, E, dtype=F64, device=dev),
                sz=torch.zeros(K, E, dtype=F64, device=dev), sy=torch.zeros(K, V, dtype=F64, device=dev),
                syy=torch.zeros(K, V, dtype=F64, device=dev))


def _accumulate(s, k, z, y):
    """rows z bf16 [m,E], y fp32 [m,V] (device, contiguous) into fold k's sums"""
    from phantom_vlb_amd._lib import check, lib
    m, E, V = z.shape[0], z.shape[1], y.shape[1]
    check(lib.vlb_ridge_gram_accumulate(z.data_ptr(), y.data_ptr(), V, s["G"][k].data_ptr(), s["C"][k].data_ptr(),
                                        s["sz"][k].data_ptr(), s["sy"][k].data_ptr(), m, E, V, _st()), "vlb_ridge_gram_accumulate")
    check(lib.vlb_ridge_sumsq_accumulate(y.data_ptr(), V, s["syy"][k].data_ptr(), m, V, _st()), "vlb_ridge_sumsq_accumulate")


def _walk(s, z, y, fold, K, chunk):
    for lo, hi in RE.chunks_of(z.shape[0], chunk):
        for k in range(K):
            sel = torch.from_numpy(lo + np.nonzero(fold[lo:hi] == k)[0]).to(z.device)
            if sel.numel():
                _accumulate(s, k, z.index_select(0, sel).contiguous(), y.index_select(0, sel).contiguous())


def _sum_except(parts, skip):
    from phantom_vlb_amd._lib import check, lib
    K, numel = parts.shape[0], parts[0].numel()
    out = torch.full_like(parts[0], -7.25)
    check(lib.vlb_f64_sum_except(parts.data_ptr(), numel, K, skip, out.data_ptr(), numel, _st()), "vlb_f64_sum_except")
    return out


# ---------------------------------------------------------------------------------------------------- integer inputs: exact
@pytest.mark.parametrize("E,V,nk", CASES)
@pytest.mark.parametrize("K,block,chunk", [(2, 1, 5), (3, 4, 64), (5, 3, 7)])
def test_integer_sums_are_exact_under_any_chunking_and_any_k(dev, E, V, nk, K, block, chunk):
    rng = np.random.default_rng(E + 7 * K)
    N = K * nk + 1
    zi, yi = rng.integers(-3, 4, (N, E)), rng.integers(-4, 5, (N, V))
    z, y = torch.from_numpy(zi).to(dev, BF16), torch.from_numpy(yi).to(dev, torch.float32)
    fold = CE.assign(N, K, block, chunk=chunk)
    s = _fold_state(K, E, V, dev)
    _walk(s, z, y, fold, K, chunk)
    free = _fold_state(1, E, V, dev)                     # the fold-free path: one set of sums, all rows in one call
    _accumulate(free, 0, z, y)
    torch.cuda.synchronize()
    for k in range(K):
        rows = np.nonzero(fold == k)[0]
        want = dict(G=zi[rows].T @ zi[rows], C=yi[rows].T @ zi[rows], sz=zi[rows].sum(0), sy=yi[rows].sum(0), syy=(yi[rows] ** 2).sum(0))
        for name, w in want.items():
            assert torch.equal(s[name][k].cpu(), torch.from_numpy(w.astype(np.float64))), (name, k)
    for name in ("G", "C", "sz", "sy", "syy"):
        assert torch.equal(_sum_except(s[name], -1), free[name][0]), f"{name}: the folds' totals are not the fold-free sums"
        for skip in range(K):
            want = sum(s[name][j].cpu() for j in range(K) if j != skip)
            assert torch.equal(_sum_except(s[name], skip).cpu(), want), (name, skip)


# ---------------------------------------------------------------------------------------------------- Gaussian: centre, score
@pytest.mark.parametrize("E,V,nk", CASES)
def test_centre_and_score_kernels_against_the_emulator(dev, E, V, nk):
    from phantom_vlb_amd._lib import check, lib
    K, lam = 3, 1e-2
    rng = np.random.default_rng(100 + E)
    N = K * nk
    zh = torch.from_numpy(rng.standard_normal((N, E)) * rng.uniform(0.5, 1.5, E) + 0.5).to(BF16)
    Wt = rng.standard_normal((V, E)) / np.sqrt(E)
    yh = torch.from_numpy(zh.double().numpy() @ Wt.T + rng.uniform(-2, 2, V) + 0.5 * rng.standard_normal((N, V))).float()
    z, y = zh.to(dev), yh.to(dev)
    fold = CE.assign(N, K, nk, chunk=N)                  # K contiguous blocks of n_k clips
    s = _fold_state(K, E, V, dev)
    _walk(s, z, y, fold, K, 16)
    S = CE.fold_sums(zh.double().numpy(), yh.double().numpy(), fold, K, 16)
    zn, yn = zh.double().numpy(), yh.double().numpy()
    Gc, Rc, X = (torch.full(sh, -7.25, dtype=F64, device=dev) for sh in ((E, E), (V, E), (V, E)))
    vy = torch.full((V,), -7.25, dtype=F64, device=dev)
    A = torch.empty(E, E, dtype=F64, device=dev)
    W, b = torch.empty(V, E, dtype=torch.float32, device=dev), torch.empty(V, dtype=torch.float32, device=dev)
    nws = lib.vlb_ridge_cv_ws_doubles(E, V)
    assert nws == V * ((E + 63) // 64)
    ws = torch.full((nws + 8,), -7.25, dtype=F64, device=dev)
    worst = dict(Gc=0.0, Rc=0.0, vy=0.0, r=0.0)
    for k in range(K):
        T = [_sum_except(s[name], k) for name in ("G", "C", "sz", "sy")]
        check(lib.vlb_ridge_cv_center(s["G"][k].data_ptr(), s["C"][k].data_ptr(), s["sz"][k].data_ptr(), s["sy"][k].data_ptr(),
                                      s["syy"][k].data_ptr(), nk, Gc.data_ptr(), Rc.data_ptr(), vy.data_ptr(), E, V, _st()),
              "vlb_ridge_cv_center")
        info = torch.full((1,), 77, dtype=torch.int32, device=dev)
        check(lib.vlb_ridge_solve(T[0].data_ptr(), T[1].data_ptr(), T[2].data_ptr(), T[3].data_ptr(), N - nk, lam, A.data_ptr(),
                                  X.data_ptr(), W.data_ptr(), b.data_ptr(), info.data_ptr(), E, V, _st()), "vlb_ridge_solve")
        r = torch.full((V,), float("nan"), dtype=F64, device=dev)
        check(lib.vlb_ridge_cv_score(X.data_ptr(), Gc.data_ptr(), Rc.data_ptr(), vy.data_ptr(), ws.data_ptr(), r.data_ptr(),
                                     info.data_ptr(), E, V, _st()), "vlb_ridge_cv_score")
        torch.cuda.synchronize()
        assert int(info) == 0 and bool((ws[nws:] == -7.25).all()), "the workspace query is smaller than what the kernel writes"
        rows = S[k]["rows"]
        eG, eR, ev = CE.moments(S[k])
        dGc, dRc, dvy = CE.moment_bars(zn[rows], yn[rows], S[k])
        for name, got, want, bar in (("Gc", Gc, eG, dGc), ("Rc", Rc, eR, dRc), ("vy", vy, ev, dvy)):
            err = np.abs(got.cpu().numpy() - want)
            assert np.all(err <= bar), (name, k, float(np.max(err / bar)))
            worst[name] = max(worst[name], float(np.max(err / bar)))
        bars = CE.r_bar(X.cpu().numpy(), eG, eR, ev, dGc, dRc, dvy)          # the device's own X, scored by the emulator
        assert bars["valid"].all(), "a target outside the first-order formula's validity: choose other inputs"
        err = np.abs(r.cpu().numpy() - bars["r"])
        worst["r"] = max(worst["r"], float(np.max(err / bars["dr"])))
        assert np.all(err <= bars["dr"]), (k, float(np.max(err / bars["dr"])), float(err.max()))
        assert np.all(np.abs(r.cpu().numpy()) <= 1.0)
    print(f"E={E} V={V} n_k={nk}: max err / bar Gc {worst['Gc']:.3e}, Rc {worst['Rc']:.3e}, vy {worst['vy']:.3e}, r {worst['r']:.3e}")
    # a failed solve turns the scoring into a no-op: the NaN pre-fill stays
    info = torch.full((1,), 3, dtype=torch.int32, device=dev)
    r = torch.full((V,), float("nan"), dtype=F64, device=dev)
    check(lib.vlb_ridge_cv_score(X.data_ptr(), Gc.data_ptr(), Rc.data_ptr(), vy.data_ptr(), ws.data_ptr(), r.data_ptr(),
                                 info.data_ptr(), E, V, _st()), "vlb_ridge_cv_score")
    torch.cuda.synchronize()
    assert bool(torch.isnan(r).all())


# ---------------------------------------------------------------------------------------------------- head level
E_MINI, V_HEAD = 512, 24
GRID = [1e-3, 1e-2, 1e-1, 1.0]
#          N                 K  block  noise  seed
KINDS = {"plain": ((300,), 5, 7, 2.0, 11),
         "taps": ((300,), 4, 16, 2.0, 12),
         "subjects": ((90, 40, 30), 3, 3, 1.0, 13)}


def _make(kind, dev):
    """head, cache, z (the device's bf16 features of every clip, host fp64), y [N,V] (device, through bf16), subject"""
    from phantom_vlb_amd.feature_cache import FeatureCache
    from phantom_vlb_amd.head import LAYER_MIX, BrainHead
    counts, K, block, noise, seed = KINDS[kind]
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
    # targets: 16 features carry the signal, plus noise; through bf16 as every step sees them
    mix = torch.zeros(E_MINI, V_HEAD, dtype=F64)
    mix[:16] = torch.randn(16, V_HEAD, generator=gen, dtype=F64)
    y = (z @ mix + noise * torch.randn(N, V_HEAD, generator=gen, dtype=F64) + 0.2).float().to(BF16).float().to(dev).contiguous()
    return head, cache, z.numpy(), y, subject, K, block


def _feed(head, cache, y, subject, K, block, chunk=64):
    head.ridge_stats_begin(folds=K, block=block)
    for lo, hi in RE.chunks_of(y.shape[0], chunk):
        idx = torch.arange(lo, hi)
        head.ridge_stats_add(cache, idx, y[lo:hi], None if subject is None else subject[idx])


@pytest.mark.parametrize("kind", list(KINDS))
def test_whole_head(dev, kind):
    head, cache, z, y, subject, K, block = _make(kind, dev)
    H, V, E, L = max(1, head.G), V_HEAD, E_MINI, len(GRID)
    sub = None if subject is None else subject.numpy()
    before = {n: t.clone() for n, t in head.master.items()}
    _feed(head, cache, y, subject, K, block)
    emu = CE.cv(z, y.double().cpu().numpy(), GRID, K, block, chunk=64, sub=sub, bars=True)
    assert head._ridge["n_fold"] == [[s["n"] for s in S] for S in emu["S"]]
    cv = head.ridge_cv(GRID)
    torch.cuda.synchronize()
    assert all(torch.equal(head.master[n], t) for n, t in before.items()), "ridge_cv wrote a parameter"
    table = head._ridge["cv_table"].cpu().numpy()
    assert table.shape == (H, K, L, V) and cv["infos"] == [[[0] * L] * K] * H and cv["grid"] == GRID
    # ---- every r, every (head, fold, lambda) target mean and the scores, within the emulator's bars
    assert emu["valid"].all(), "a target outside the first-order formula's validity: choose other inputs"
    err = np.abs(table - emu["r"])
    assert np.all(err <= emu["r_bar"]), float(np.max(err / emu["r_bar"]))
    mbar = emu["r_bar"].mean(-1) + V * 2.0 ** -52
    merr = np.abs(table.mean(-1) - emu["means"])
    assert np.all(merr <= mbar)
    serr = np.abs(np.array(cv["score"]) - emu["score"])
    assert np.all(serr <= emu["score_bar"])
    assert np.all(np.abs(np.array(cv["score_per_head"]) - emu["score_per_head"]) <= emu["r_bar"].mean((1, 3)) + (V + K) * 2.0 ** -52)
    assert torch.equal(cv["r"], head._ridge["cv_table"].mean(1)) and tuple(cv["r"].shape) == (H, L, V)
    # ---- the choice, once the emulator's margin rules out luck (condition (b) of test_cpu_ridge_cv_emul.py)
    order = np.argsort(emu["score"])[::-1]
    margin, sbar = float(emu["score"][order[0]] - emu["score"][order[1]]), float(emu["score_bar"].max())
    print(f"{kind}: max r err / bar {np.max(err / emu['r_bar']):.3e}, score err / bar {np.max(serr / emu['score_bar']):.3e}; scores "
          f"{np.round(emu['score'], 5).tolist()}, best {emu['best_index']}, margin {margin:.2e} = {margin / sbar:.0f} score bars")
    assert margin >= 100 * sbar, "the inputs do not separate the best two grid points: choose other inputs"
    if kind == "plain":
        assert 0 < emu["best_index"] < L - 1
    assert cv["best_index"] == emu["best_index"] and cv["best_lambda"] == GRID[emu["best_index"]]
    # ---- the totals' solve with the chosen lambda: masters within master_bar of the emulator's
    out = head.ridge_solve(cv["best_lambda"])
    torch.cuda.synchronize()
    assert all(o["info"] == 0 and o["l2_lambda"] == cv["best_lambda"] for o in out)
    W_dev = head.master[WN].cpu().numpy().reshape(H, V, E)
    yh = y.double().cpu().numpy()
    for g in range(H):
        rows = np.arange(len(z)) if sub is None else np.nonzero(sub == g)[0]
        assert out[g]["n"] == len(rows)
        sol = RE.solve(RE.sums(z[rows], yh[rows], chunk=512), cv["best_lambda"])
        dW = np.abs(W_dev[g].astype(np.float64) - sol["W"].astype(np.float32).astype(np.float64))
        ratio = float(np.max(dW / RE.master_bar(sol["W"], RE.cond2(sol["A"]), E)))
        print(f"{kind} head {g}: N {len(rows)}, max |dW| / master_bar {ratio:.3f}")
        assert ratio <= 1
        assert np.array_equal(head.compute[WN].float().cpu().numpy().reshape(H, V, E)[g], RE.rne_bf16(W_dev[g]))
    head.ridge_stats_end()


def test_two_runs_give_the_same_bits(dev):
    head, cache, _, y, subject, K, block = _make("subjects", dev)
    tables, scores = [], []
    for _ in range(2):
        _feed(head, cache, y, subject, K, block, chunk=50)
        cv = head.ridge_cv(GRID)
        tables.append(head._ridge["cv_table"].clone())
        scores.append((cv["score"], cv["score_per_head"], cv["best_index"], cv["r"].clone()))
        head.ridge_stats_end()
    assert torch.equal(tables[0].view(torch.int64), tables[1].view(torch.int64))
    assert scores[0][:3] == scores[1][:3] and torch.equal(scores[0][3], scores[1][3])


def test_a_grid_point_whose_factorisation_fails_is_excluded_with_a_warning(dev):
    """1e-30 is a valid grid value, but with N_tr = 240 < E = 512 the centred Gram matrix has rank 239 at most and a ridge
    term of 1e-30 * 240 * 24 is far below its rounding: a pivot past the rank comes out non-positive and the factorisation
    reports it.  Valid memory throughout; the kernels after a failed factorisation are no-ops."""
    head, cache, z, y, subject, K, block = _make("plain", dev)
    grid = [1e-30] + GRID[1:]
    before = {n: t.clone() for n, t in head.master.items()}
    _feed(head, cache, y, subject, K, block)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        cv = head.ridge_cv(grid)
    torch.cuda.synchronize()
    msgs = [str(w.message) for w in rec if "ridge_cv" in str(w.message)]
    assert len(msgs) == 1 and "1e-30" in msgs[0] and "excluded" in msgs[0], msgs
    infos = np.array(cv["infos"])
    assert infos[:, :, 0].any() and not infos[:, :, 1:].any()
    table = head._ridge["cv_table"]
    for k in range(K):                                   # a failed (fold, lambda) keeps its NaN pre-fill
        assert bool(torch.isnan(table[0, k, 0]).all()) == bool(infos[0, k, 0])
    emu = CE.cv(z, y.double().cpu().numpy(), grid[1:], K, block, chunk=64)
    assert cv["best_index"] == emu["best_index"] + 1 and cv["best_lambda"] == grid[cv["best_index"]] and cv["best_lambda"] != 1e-30
    assert np.isnan(cv["score"][0]) and not np.isnan(cv["score"][1:]).any()
    assert all(torch.equal(head.master[n], t) for n, t in before.items())
    # every grid point failing raises and leaves the parameters
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match="every grid point"):
            head.ridge_cv([1e-30, 1e-31])
    assert all(torch.equal(head.master[n], t) for n, t in before.items())
    head.ridge_stats_end()


def test_a_fold_with_fewer_than_two_clips_raises_before_any_launch(dev):
    head, cache, _, y, subject, _, _ = _make("plain", dev)
    before = {n: t.clone() for n, t in head.master.items()}
    _feed(head, cache, y, subject, 5, 100)               # 300 clips in blocks of 100: folds 3 and 4 stay empty
    assert head._ridge["n_fold"] == [[100, 100, 100, 0, 0]]
    with pytest.raises(ValueError, match=r"the head: fold 3 of 5 holds 0 clip"):
        head.ridge_cv(GRID)
    assert "cv_table" not in head._ridge and "T" not in head._ridge           # nothing allocated, nothing launched
    assert all(torch.equal(head.master[n], t) for n, t in before.items())
    head.ridge_stats_end()
