"""The closed-form ridge fit and its cross-validation under target weights on the device: the two masked
accumulate entries and vlb_ridge_cv_score_rows alone, then ``BrainHead.ridge_stats_begin(weighted=True)`` and what follows it on
a plain head, a head with three tapped layers and three per-subject heads, then ``ridge_fit_weighted`` through the module,
against tests/ridge_wfit_emul.py.

Bars (none is fitted to what the device returns):
* the masked accumulate runs the unmasked entry's launches with a select on the staging path: G, sz and every kept row of C /
  entry of sy, syy are ``torch.equal`` to the unmasked entry's on the same inputs; masked ones are +0.0 bit for bit whatever y
  holds there.  Integer inputs (z in [-3,3], y in [-4,4]) make every sum exact, so two chunks equal the emulator's.
* vlb_ridge_cv_score_rows: the rows it writes are ``torch.equal`` to vlb_ridge_cv_score's, the others keep a sentinel.
* head level: a kept row at level d is the unweighted computation on the selected y with lambda scale[d], so
  ``ridge_emul.master_bar`` (W, b) and ridge_cv_emul's ``r_bar`` with ``dx_bar`` (the table) apply as they stand; a mean over
  the kept targets carries the mean of their bars plus (V + K + H) 2^-52.  Every kept row is also ``torch.equal`` to the plain
  vlb_ridge_solve's row at lambda scale[d] on the same sums.
* the choices: the global one is compared once the emulator's best score leads its runner-up by more than two score bars
  (asserted for every case); per target the forced-choice rule of test_gpu_ridge_rows, with at most 1/8 of the kept
  (head, target) pairs below 100 bars (asserted).
"""
import numpy as np
import pytest
import torch

import ridge_emul as RE
import ridge_wfit_emul as WF
import test_gpu_ridge_fit as RF
from test_gpu_ridge_cv import E_MINI, GRID, KINDS, V_HEAD, _make, _st

pytestmark = pytest.mark.gpu
F64, F32, BF16, I32 = torch.float64, torch.float32, torch.bfloat16, torch.int32
WN, BN = RF.WN, RF.BN
SENT = -7.25
FILLS = (0.0, float("nan"), float("inf"), float("-inf"))


# ---------------------------------------------------------------------------------------------------- 1: the masked accumulate
def _masks(V):
    one = np.zeros(V, bool)
    one[V // 2] = True
    edges = np.ones(V, bool)
    edges[[i for i in (0, 63, 64, 127) if i < V]] = False
    return {"all": np.ones(V, bool), "one": one, "tile-edges": edges, "alternating": np.arange(V) % 2 == 0}


def _accumulate(dev, z, yh, ldy, keep_h, rows=None, masked=True):
    """-> G, C, sz, sy, syy (host) of the rows ``rows`` (a list of chunks) of z bf16 [n,E] (device), yh fp32 [n,V] (host) laid
    out with pitch ldy; keep sits at an odd float offset of its allocation; every output carries a sentinel tail"""
    from phantom_vlb_amd._lib import check, lib
    n, E = z.shape
    V = yh.shape[1]
    buf = torch.full((n, ldy), SENT, dtype=F32)
    buf[:, :V] = yh
    y = buf.to(dev)
    kb = torch.full((V + 9,), float("nan"), dtype=F32)
    kb[1:V + 1] = torch.from_numpy(keep_h.astype(np.float32))
    kd = kb.to(dev)
    keep = kd[1:V + 1]
    assert keep.data_ptr() % 8 == 4
    sizes = dict(G=E * E, C=V * E, sz=E, sy=V, syy=V)
    out = {k: torch.cat([torch.zeros(m, dtype=F64), torch.full((8,), SENT, dtype=F64)]).to(dev) for k, m in sizes.items()}
    for lo, hi in rows or [(0, n)]:
        zz, yy = z[lo:hi], y[lo:hi]
        if masked:
            check(lib.vlb_ridge_gram_accumulate_masked(zz.data_ptr(), yy.data_ptr(), ldy, keep.data_ptr(), out["G"].data_ptr(),
                                                       out["C"].data_ptr(), out["sz"].data_ptr(), out["sy"].data_ptr(), hi - lo, E, V,
                                                       _st()), "vlb_ridge_gram_accumulate_masked")
            check(lib.vlb_ridge_sumsq_accumulate_masked(yy.data_ptr(), ldy, keep.data_ptr(), out["syy"].data_ptr(), hi - lo, V, _st()),
                  "vlb_ridge_sumsq_accumulate_masked")
        else:
            check(lib.vlb_ridge_gram_accumulate(zz.data_ptr(), yy.data_ptr(), ldy, out["G"].data_ptr(), out["C"].data_ptr(),
                                                out["sz"].data_ptr(), out["sy"].data_ptr(), hi - lo, E, V, _st()),
                  "vlb_ridge_gram_accumulate")
            check(lib.vlb_ridge_sumsq_accumulate(yy.data_ptr(), ldy, out["syy"].data_ptr(), hi - lo, V, _st()),
                  "vlb_ridge_sumsq_accumulate")
    torch.cuda.synchronize()
    for k, m in sizes.items():
        assert bool((out[k][m:] == SENT).all()), f"{k}: the tail was written"
    return {"G": out["G"][:E * E].view(E, E).cpu(), "C": out["C"][:V * E].view(V, E).cpu(), "sz": out["sz"][:E].cpu(),
            "sy": out["sy"][:V].cpu(), "syy": out["syy"][:V].cpu()}


@pytest.mark.parametrize("n,E,V", [(37, 70, 200), (1, 8, 1), (33, 64, 65)])
def test_masked_accumulate_keeps_the_kept_bits_and_zeroes_the_rest(dev, n, E, V):
    rng = np.random.default_rng(n + E + V)
    zi, yi = rng.integers(-3, 4, (n, E)), rng.integers(-4, 5, (n, V))
    z = torch.from_numpy(zi).to(dev, BF16)
    y0 = torch.from_numpy(yi).float()
    for ldy in (V, V + 1):                                 # V + 1: never a multiple of 4 with an aligned row -> the scalar staging path
        plain = _accumulate(dev, z, y0, ldy, np.ones(V, bool), masked=False)
        for name, keep in _masks(V).items():
            k = torch.from_numpy(keep)
            runs = []
            for fill in FILLS:
                yf = y0.clone()
                yf[:, ~k] = fill
                runs.append(_accumulate(dev, z, yf, ldy, keep))
            got = runs[0]
            assert torch.equal(got["G"], plain["G"]) and torch.equal(got["sz"], plain["sz"]), (name, ldy)
            for key in ("C", "sy", "syy"):
                assert torch.equal(got[key][k], plain[key][k]), (key, name, ldy)
                dead = got[key][~k]
                assert bool((dead == 0).all()) and not bool(torch.signbit(dead).any()), (key, name, ldy)
                for other in runs[1:]:                      # 0, NaN, +Inf, -Inf at the masked targets: the same bits
                    assert torch.equal(other[key].view(torch.int64), got[key].view(torch.int64)), (key, name, ldy)
            for other in runs[1:]:
                assert torch.equal(other["G"], got["G"]) and torch.equal(other["sz"], got["sz"])
        # a weight row, not a 0/1 one: any positive value keeps
        wrow = np.where(_masks(V)["alternating"], 0.25, 0.0)
        got = _accumulate(dev, z, y0, ldy, wrow)
        assert torch.equal(got["C"][::2], plain["C"][::2]) and not bool(got["C"][1::2].any())
        # two chunks accumulate as the emulator does (integers: every order gives the same fp64 number)
        if n > 1:
            keep = _masks(V)["tile-edges"]
            yn = y0.clone()
            yn[:, ~torch.from_numpy(keep)] = float("nan")
            cut = n // 2 + 1
            got = _accumulate(dev, z, yn, ldy, keep, rows=[(0, cut), (cut, n)])
            ysel = WF.select_y(yi.astype(np.float64), keep)
            emu = RE.sums(zi, ysel, chunk=cut)
            for key in ("G", "C", "sz", "sy"):
                assert torch.equal(got[key], torch.from_numpy(emu[key])), (key, ldy)
            assert torch.equal(got["syy"], torch.from_numpy((ysel * ysel).sum(0)))


# ---------------------------------------------------------------------------------------------------- 2: the row-select score
@pytest.mark.parametrize("V", [1, 65, 200])
def test_score_rows_writes_its_rows_with_the_plain_scores_bits(dev, V):
    from phantom_vlb_amd._lib import check, lib
    E = 70
    gen = torch.Generator().manual_seed(V)
    X = torch.randn(V, E, generator=gen, dtype=F64).to(dev)
    M = torch.randn(E + 5, E, generator=gen, dtype=F64)
    Gc, Rc = (M.t() @ M).to(dev), torch.randn(V, E, generator=gen, dtype=F64).to(dev)
    vy = (0.5 + torch.rand(V, generator=gen, dtype=F64)).to(dev)
    nws = lib.vlb_ridge_cv_ws_doubles(E, V)
    ws = torch.full((nws + 8,), SENT, dtype=F64, device=dev)
    info = torch.zeros(1, dtype=I32, device=dev)
    plain = torch.full((V + 8,), SENT, dtype=F64, device=dev)
    check(lib.vlb_ridge_cv_score(X.data_ptr(), Gc.data_ptr(), Rc.data_ptr(), vy.data_ptr(), ws.data_ptr(), plain.data_ptr(),
                                 info.data_ptr(), E, V, _st()), "vlb_ridge_cv_score")
    choice_h = torch.randint(-1, 3, (V,), generator=gen).to(I32)
    choice_h[0] = 1
    choice = choice_h.to(dev)
    got = torch.full((V + 8,), SENT, dtype=F64, device=dev)
    args = (X.data_ptr(), Gc.data_ptr(), Rc.data_ptr(), vy.data_ptr(), ws.data_ptr(), got.data_ptr())
    check(lib.vlb_ridge_cv_score_rows(*args, info.data_ptr(), E, V, choice.data_ptr(), 1, _st()), "vlb_ridge_cv_score_rows")
    torch.cuda.synchronize()
    mine = choice == 1
    assert bool((ws[nws:] == SENT).all()) and bool((got[V:] == SENT).all()) and bool((plain[:V] != SENT).all())
    assert torch.equal(got[:V][mine], plain[:V][mine]) and bool((got[:V][~mine] == SENT).all())
    for want in (0, 2):                                    # the other levels complete the vector; -1 is never written
        check(lib.vlb_ridge_cv_score_rows(*args, info.data_ptr(), E, V, choice.data_ptr(), want, _st()), "vlb_ridge_cv_score_rows")
    torch.cuda.synchronize()
    live = choice >= 0
    assert torch.equal(got[:V][live], plain[:V][live]) and bool((got[:V][~live] == SENT).all())
    # a failed solve's info: nothing is written
    bad = torch.full((1,), 3, dtype=I32, device=dev)
    got.fill_(SENT)
    check(lib.vlb_ridge_cv_score_rows(*args, bad.data_ptr(), E, V, choice.data_ptr(), 1, _st()), "vlb_ridge_cv_score_rows")
    torch.cuda.synchronize()
    assert bool((got == SENT).all())


# ---------------------------------------------------------------------------------------------------- 3: head level
#        head kind   weights
CASES = [("plain", "mask"), ("plain", "scaled"), ("plain", "levels"), ("taps", "levels"), ("subjects", "per-head")]
_CACHE = {}


def _weights(kind, wkind):
    """fp32 [H,V]: about half of the targets masked (target 0 kept, target 1 masked); per-head: another mask for every head"""
    H = len(KINDS[kind][0])
    rng = np.random.default_rng(7)
    rows = []
    for g in range(H):
        keep = rng.random(V_HEAD) < 0.55
        keep[:2] = True, False
        lv = rng.choice([0.5, 1.0, 2.0], V_HEAD) if wkind == "levels" else 0.3 if wkind == "scaled" else 1.0
        rows.append((keep * lv).astype(np.float32))
    return np.stack(rows)


def _feed(head, cache, y, subject, K, block, chunk=64, weighted=True):
    head.ridge_stats_begin(folds=K, block=block, weighted=weighted)
    for lo, hi in RE.chunks_of(y.shape[0], chunk):
        idx = torch.arange(lo, hi)
        head.ridge_stats_add(cache, idx, y[lo:hi], None if subject is None else subject[idx])


def _case(kind, wkind, dev):
    """the head of ``kind`` with the weights set and NaN planted in its masked targets, and the emulator's fit (made once)"""
    key = (kind, wkind)
    if key not in _CACHE:
        head, cache, z, y, subject, K, block = _make(kind, dev)
        w = _weights(kind, wkind)
        sub = None if subject is None else subject.numpy()
        yh = y.double().cpu().numpy()
        emu = WF.fit_w(z, yh, w, GRID, K, block, chunk=64, sub=sub, bars=True)
        wd = torch.from_numpy(w).to(dev)
        yn = y.clone()
        g_clip = torch.zeros(y.shape[0], dtype=torch.int64) if subject is None else subject
        yn[wd[g_clip.to(dev)] == 0] = float("nan")
        _CACHE[key] = dict(head=head, cache=cache, z=z, y=yn, yh=yh, subject=subject, sub=sub, K=K, block=block, w=w, wd=wd, emu=emu,
                           start={n: t.clone() for n, t in head.master.items()})
    c = _CACHE[key]
    c["head"].set_target_weights(c["wd"])
    for n, t in c["start"].items():
        c["head"].master[n].copy_(t)
        c["head"].compute[n].copy_(t)
    return c


def _plain_solve(dev, head, g, lam):
    """vlb_ridge_solve on head g's totals with l2_lambda = lam -> W [V,E], b [V]"""
    from phantom_vlb_amd._lib import check, lib
    E, V = head.E, head.V
    Gs, Cs, szs, sys_ = (t.clone() for t in head._head_totals(head._ridge, g))
    A, X = torch.empty(E, E, dtype=F64, device=dev), torch.empty(V, E, dtype=F64, device=dev)
    W, b = torch.full((V, E), SENT, dtype=F32, device=dev), torch.full((V,), SENT, dtype=F32, device=dev)
    info = torch.full((1,), 77, dtype=I32, device=dev)
    check(lib.vlb_ridge_solve(Gs.data_ptr(), Cs.data_ptr(), szs.data_ptr(), sys_.data_ptr(), head._ridge["n"][g], lam, A.data_ptr(),
                              X.data_ptr(), W.data_ptr(), b.data_ptr(), info.data_ptr(), E, V, _st()), "vlb_ridge_solve")
    torch.cuda.synchronize()
    assert int(info) == 0
    return W, b


@pytest.mark.parametrize("kind,wkind", CASES)
def test_whole_head_fits_and_cross_validates_under_weights(dev, kind, wkind):
    c = _case(kind, wkind, dev)
    head, emu, z, sub, w = c["head"], c["emu"], c["z"], c["sub"], c["w"]
    ecv = emu["cv"]
    H, V, E, L, K = max(1, head.G), V_HEAD, E_MINI, len(GRID), c["K"]
    keep = w > 0
    _feed(head, c["cache"], c["y"], c["subject"], K, c["block"])
    st = head._ridge
    assert st["scale"] == [lv["scale"] for lv in ecv["lv"]] and st["lvl"].cpu().tolist() == [lv["lvl"].tolist() for lv in ecv["lv"]]
    # ---- ridge_solve: the emulator's minimiser; masked rows exactly 0; kept rows the plain solve's at lambda scale
    lam = 1e-2
    out = head.ridge_solve(lam)
    torch.cuda.synchronize()
    Wm, bm = head.master[WN].view(H, V, E).clone(), head.master[BN].view(H, V).clone()
    assert [o["kept"] for o in out] == keep.sum(1).tolist() and [o["levels"] for o in out] == [len(s) for s in st["scale"]]
    assert all(o["info"] == 0 and o["l2_lambda"] == lam for o in out)
    for g in range(H):
        rows = np.arange(len(z)) if sub is None else np.nonzero(sub == g)[0]
        assert out[g]["n"] == len(rows)
        dead = torch.from_numpy(~keep[g]).to(dev)
        for t in (Wm[g][dead], bm[g][dead]):
            assert bool((t == 0).all()) and not bool(torch.signbit(t).any())
        sol = WF.solve_w(WF.sums_w(z[rows], c["yh"][rows], w[g], chunk=512), lam, w[g])
        worst = 0.0
        for (d, _), s in sol["sols"].items():
            mine = sol["lv"]["lvl"] == d
            dW = np.abs(Wm[g].cpu().numpy().astype(np.float64) - s["W"].astype(np.float32).astype(np.float64))[mine]
            worst = max(worst, float(np.max(dW / RE.master_bar(s["W"], RE.cond2(s["A"]), E)[mine])))
            db = np.abs(bm[g].cpu().numpy().astype(np.float64) - s["b"].astype(np.float32).astype(np.float64))[mine]
            worst = max(worst, float(np.max(db / RE.master_bar(s["b"], RE.cond2(s["A"]), E)[mine])))
            Wp, bp = _plain_solve(dev, head, g, lam * sol["lv"]["scale"][d])
            md = torch.from_numpy(mine).to(dev)
            assert torch.equal(Wm[g][md], Wp[md]) and torch.equal(bm[g][md], bp[md]), (g, d)
        print(f"{kind}/{wkind} head {g}: {int(keep[g].sum())} kept, {len(sol['lv']['scale'])} level(s), max |dW| / master_bar {worst:.3f}")
        assert worst <= 1
    for n in (WN, BN):
        assert np.array_equal(head.compute[n].float().cpu().numpy(), RE.rne_bf16(head.master[n].cpu().numpy()))
    for n, t in c["start"].items():
        head.master[n].copy_(t)
        head.compute[n].copy_(t)
    # ---- ridge_cv: the table within the emulator's bars at the kept targets, NaN at the masked ones
    plain_cv = head.ridge_cv(GRID)
    cv = head.ridge_cv(GRID, per_target=True)
    torch.cuda.synchronize()
    assert all(torch.equal(head.master[n], t) for n, t in c["start"].items()), "ridge_cv wrote a parameter"
    for k in ("grid", "score", "score_per_head", "best_index", "best_lambda", "infos"):
        assert cv[k] == plain_cv[k], k
    assert cv["infos"] == [[[0] * L] * K] * H
    assert ecv["valid"].all(), "a target outside the first-order formula's validity: choose other inputs"
    table = st["cv_table"].cpu().numpy()
    k4 = np.broadcast_to(keep[:, None, None, :], table.shape)
    assert np.isnan(table[~k4]).all() and np.isfinite(table[k4]).all()
    err = np.abs(table - ecv["r"])[k4]
    assert np.all(err <= ecv["r_bar"][k4]), float(np.max(err / ecv["r_bar"][k4]))
    serr = np.abs(np.array(cv["score"]) - ecv["score"])
    assert np.all(serr <= ecv["score_bar"])
    means_dev = np.stack([table[g][..., keep[g]].mean(-1) for g in range(H)])
    assert np.all(np.abs(np.array(cv["score_per_head"]) - means_dev.mean(1)) <= (V + K) * 2.0 ** -52)
    order = np.argsort(ecv["score"])[::-1]
    margin, sbar = float(ecv["score"][order[0]] - ecv["score"][order[1]]), float(ecv["score_bar"].max())
    print(f"{kind}/{wkind}: max r err / bar {np.max(err / ecv['r_bar'][k4]):.3e}, score err / bar {np.max(serr / ecv['score_bar']):.3e}; "
          f"scores {np.round(ecv['score'], 5).tolist()}, best {ecv['best_index']}, margin {margin / sbar:.0f} score bars")
    assert margin > 2 * sbar, "the inputs do not separate the best two grid points: choose other inputs"
    assert cv["best_index"] == ecv["best_index"] and cv["best_lambda"] == GRID[ecv["best_index"]]
    # ---- per target: the forced-choice rule over the kept targets; masked: -1, NaN, best_lambda
    m, bar = emu["margins"], emu["rmean_bar"]
    thin = (m < 100) & keep
    print(f"{kind}/{wkind}: {int(thin.sum())} of {int(keep.sum())} kept (head, target) pairs below 100 bars; emulator counts "
          f"{emu['lambda_counts'].tolist()}")
    assert thin.sum() <= keep.sum() / 8, "the inputs do not separate the targets' best two grid points: choose other inputs"
    choice = cv["choice"]
    assert choice.dtype == I32 and choice.is_cuda and tuple(choice.shape) == (H, V)
    ch = choice.cpu().numpy()
    assert (ch[~keep] == -1).all() and (ch[keep] >= 0).all()
    rmean_dev = st["cv_rmean"].cpu().numpy()
    k3 = np.broadcast_to(keep[:, None, :], rmean_dev.shape)
    assert np.all(np.abs(rmean_dev - emu["rmean"])[k3] <= bar[k3]) and np.isnan(rmean_dev[~k3]).all()
    hh, vv = np.nonzero(keep)
    at_dev, at_emu = emu["rmean"][hh, ch[hh, vv], vv], emu["rmean"][hh, emu["choice"][hh, vv], vv]
    assert np.all(at_dev >= at_emu - (bar[hh, ch[hh, vv], vv] + bar[hh, emu["choice"][hh, vv], vv]))
    forced = keep & ~thin
    assert np.array_equal(ch[forced], emu["choice"][forced])
    lam_rows = cv["lambda_rows"]
    assert lam_rows.dtype == F32 and lam_rows.is_cuda and tuple(lam_rows.shape) == (H, V)
    want_rows = np.where(keep, np.asarray(GRID)[np.maximum(ch, 0)], cv["best_lambda"]).astype(np.float32)
    assert np.array_equal(lam_rows.cpu().numpy(), want_rows)
    assert cv["lambda_counts"] == [np.bincount(ch[g][keep[g]], minlength=L).tolist() for g in range(H)]
    assert abs(cv["score_per_target"] - rmean_dev[hh, ch[hh, vv], vv].mean()) <= (keep.sum() + 2) * 2.0 ** -52
    assert abs(cv["score_per_target"] - emu["score_per_target"]) <= bar[k3].max() + (keep.sum() + 2) * 2.0 ** -52
    # ---- ridge_solve_rows: every kept row is the plain solve's at grid[choice] scale[level]; masked rows exactly 0
    sols = head.ridge_solve_rows(choice, GRID)
    torch.cuda.synchronize()
    assert [o["lambda_counts"] for o in sols] == cv["lambda_counts"] and all(o["info"] == 0 for o in sols)
    Wm, bm = head.master[WN].view(H, V, E), head.master[BN].view(H, V)
    for g in range(H):
        lvl, scale = ecv["lv"][g]["lvl"], ecv["lv"][g]["scale"]
        dead = torch.from_numpy(~keep[g]).to(dev)
        assert not bool(Wm[g][dead].any()) and not bool(bm[g][dead].any())
        for i, d in sorted({(int(ch[g, v]), int(lvl[v])) for v in np.nonzero(keep[g])[0]}):
            Wp, bp = _plain_solve(dev, head, g, GRID[i] * scale[d])
            md = torch.from_numpy((ch[g] == i) & (lvl == d)).to(dev)
            assert torch.equal(Wm[g][md], Wp[md]) and torch.equal(bm[g][md], bp[md]), (g, i, d)
    bad = choice.clone()
    bad[0, 0] = -1                                          # target 0 is kept in every head
    with pytest.raises(ValueError, match="masked targets only"):
        head.ridge_solve_rows(bad, GRID)
    head.ridge_stats_end()
    head.set_target_weights(None)


def test_a_constant_row_is_the_unweighted_fit_bit_for_bit(dev):
    head, cache, _, y, subject, K, block = _make("plain", dev)
    start = {n: t.clone() for n, t in head.master.items()}

    def run(weighted):
        for n, t in start.items():
            head.master[n].copy_(t)
            head.compute[n].copy_(t)
        head.set_target_weights(torch.full((V_HEAD,), 0.3, device=dev) if weighted else None)
        _feed(head, cache, y, subject, K, block, weighted=weighted)
        if weighted:
            assert head._ridge["scale"] == [[1.0]]
        cv = head.ridge_cv(GRID, per_target=True)
        table = head._ridge["cv_table"].clone()
        head.ridge_solve(cv["best_lambda"])
        one = (head.master[WN].clone(), head.master[BN].clone())
        head.ridge_solve_rows(cv["choice"], GRID)
        torch.cuda.synchronize()
        rows = (head.master[WN].clone(), head.master[BN].clone())
        head.ridge_stats_end()
        return cv, table, one, rows
    a, b = run(False), run(True)
    head.set_target_weights(None)
    assert torch.equal(a[1].view(torch.int64), b[1].view(torch.int64)) and torch.equal(a[0]["choice"], b[0]["choice"])
    assert a[0]["best_index"] == b[0]["best_index"] and a[0]["lambda_counts"] == b[0]["lambda_counts"]
    assert torch.equal(a[0]["lambda_rows"], b[0]["lambda_rows"])
    for x, yy in zip(a[2] + a[3], b[2] + b[3]):
        assert torch.equal(x.view(I32), yy.view(I32))


def test_two_weighted_runs_give_the_same_bits(dev):
    c = _case("subjects", "per-head", dev)
    head = c["head"]
    got = []
    for _ in range(2):
        _feed(head, c["cache"], c["y"], c["subject"], c["K"], c["block"], chunk=50)
        cv = head.ridge_cv(GRID, per_target=True)
        head.ridge_solve_rows(cv["choice"], GRID)
        torch.cuda.synchronize()
        got.append((head._ridge["cv_table"].clone(), cv["choice"].clone(), cv["score"], head.master[WN].clone(), head.master[BN].clone()))
        head.ridge_stats_end()
    head.set_target_weights(None)
    assert torch.equal(got[0][0].view(torch.int64), got[1][0].view(torch.int64)) and torch.equal(got[0][1], got[1][1])
    assert got[0][2] == got[1][2] and torch.equal(got[0][3], got[1][3]) and torch.equal(got[0][4], got[1][4])


# ---------------------------------------------------------------------------------------------------- 3b: the head's own optimum
@pytest.mark.parametrize("kind,wkind", [("plain", "mask"), ("taps", "levels")])          # two of CASES: their emulator fits exist
def test_the_weighted_fit_is_the_heads_own_optimum(dev, kind, wkind):
    """After a weighted ``ridge_solve`` the head's existing weighted backward, accumulated over all clips (no dropout,
    loss_scale = l2_scale = 1 / chunks), must vanish in d ridge weight and d ridge bias.  One head only: with ``subjects`` the
    step divides a head's data term by the clips of the whole batch, the closed form by that head's own, so the step's
    gradient is not this objective's.

    The bar, per element, summed over the chunks (host fp64), nothing fitted to what the device returns:
    * wloss_emul.ridge_bwd_w_bars on the device's own d pred (dW: B + 3 roundings, dbias: B + ceil(B/8) + 2);
    * through |z|: wloss_emul.dpred_bar on the device's own pred and row weight sum, (V + 2) 2^-24 |d pred| for that fp32 sum of
      V weights against the exact one, and head_emul.ridge_bars' pred bar times d(d pred)/d pred = loss_scale 2 w / (B Ws);
    * the written W: the kernels read bf16(master).  The exact gradient at (W*, b*) + d is H d with H the objective's Hessian,
      |H d| <= (2 w_v / (N Ws)) sum_n (|d W_v| . |z_n| + |d b_v|) |z_n| + 2 lambda |d W_v| (bias: without the last |z_n| and the
      penalty), and |d| <= one bf16 spacing step of the emulator's fp32 value - 2^(e-8) for |x| in [2^(e-1), 2^e), twice the
      half-ulp that ridge_emul.rne_bf16 leaves (asserted), which also covers a master in the next binade - plus
      ridge_emul.master_bar for the master itself.
    Masked rows: d bias exactly 0, dW the penalty's 2 lambda W = 0."""
    import head_emul as HE
    import wloss_emul as WL
    c = _case(kind, wkind, dev)
    head, z, w, cache = c["head"], c["z"], c["w"][0], c["cache"]
    N, V, E, lam, chunk = len(z), V_HEAD, E_MINI, 1e-2, 60
    keep = w > 0
    _feed(head, cache, c["y"], None, c["K"], c["block"])
    head.ridge_solve(lam)
    head.ridge_stats_end()
    was, head.l2_lambda = head.l2_lambda, lam
    Wbf, bbf = head.compute[WN].float().cpu().double(), head.compute[BN].float().cpu().double()
    parts = RE.chunks_of(N, chunk)
    s = 1.0 / len(parts)
    w64 = torch.from_numpy(w.astype(np.float64))
    Ws = float(w64.sum())
    ysel = torch.from_numpy(WF.select_y(c["yh"], w))
    tot = dict(dW=torch.zeros(V, E, dtype=F64), dbias=torch.zeros(V, dtype=F64))
    bar = dict(dW=torch.zeros(V, E, dtype=F64), dbias=torch.zeros(V, dtype=F64))
    for lo, hi in parts:
        B = hi - lo
        idx = torch.arange(lo, hi)
        head.forward_cached(cache, idx, c["y"][lo:hi].contiguous())
        (head.backward_tapped if head.K else head.backward_cached)(loss_scale=s, l2_scale=s)
        torch.cuda.synchronize()
        dW, db = head.grads[WN].double().cpu().view(V, E), head.grads[BN].double().cpu().view(V)
        zc = head.z[:B].float().cpu().double()
        assert torch.equal(zc, torch.from_numpy(z[lo:hi]))
        dp_dev, pred_dev = head.dpred[:B].double().cpu(), head.pred[:B].double().cpu()
        assert not bool(dp_dev[:, ~torch.from_numpy(keep)].any())
        seed = s * 2.0 * lam * Wbf
        ref = dict(dW=seed + dp_dev.t() @ zc, dbias=dp_dev.sum(0), mag_dW=seed.abs() + dp_dev.abs().t() @ zc.abs(),
                   mag_dbias=dp_dev.abs().sum(0))
        stage = WL.ridge_bwd_w_bars(ref, B)
        assert bool((dW - ref["dW"]).abs().le(stage["dW"]).all()) and bool((db - ref["dbias"]).abs().le(stage["dbias"]).all())
        rs = dict(W=WL.wstat_columns(head.wstat.detach().cpu())["W"][:B].double())
        wB = w64.expand(B, V)
        dpx, mag = WL.dpred(pred_dev, ysel[lo:hi], wB, rs, "mse", s)
        assert bool((dp_dev - dpx).abs().le(WL.dpred_bar(dpx, mag, "mse")).all())
        fwd = HE.ridge(zc, Wbf, bbf, ysel[lo:hi], lam)
        pbar = HE.ridge_bars(fwd, B, E, V)["pred"]
        assert bool((pred_dev - fwd["pred"]).abs().le(pbar).all())
        ddp = WL.dpred_bar(dpx, mag, "mse") + (V + 2) * HE.U * dpx.abs() + s * 2.0 * wB / (B * Ws) * pbar
        for key, got, through in (("dW", dW, ddp.t() @ zc.abs()), ("dbias", db, ddp.sum(0))):
            tot[key] += got
            bar[key] += stage[key] + through
    head.l2_lambda = was
    # ---- the written W: one bf16 spacing step of the emulator's value, plus master_bar
    sol = WF.solve_w(WF.sums_w(z, c["yh"], w, chunk=512), lam, w)

    def step(x, mb):
        x32 = np.asarray(x, np.float64).astype(np.float32)
        e = np.frexp(np.abs(x32.astype(np.float64)))[1]
        d = np.where(x32 != 0, 2.0 ** (e - 8.0), 0.0)
        assert np.all(np.abs(RE.rne_bf16(x32).astype(np.float64) - x32) <= d / 2)
        return torch.from_numpy(d + mb)
    mbW, mbb = np.zeros((V, E)), np.zeros(V)
    for (d, _), so in sol["sols"].items():
        mine = sol["lv"]["lvl"] == d
        cond = RE.cond2(so["A"])
        mbW[mine], mbb[mine] = RE.master_bar(so["W"], cond, E)[mine], RE.master_bar(so["b"], cond, E)[mine]
    dWt, dbt = step(sol["W"], mbW), step(sol["b"], mbb)
    za = torch.from_numpy(np.abs(z))
    coef = (2.0 * w64 / (N * Ws))[:, None]
    resid = dWt @ za.t() + dbt[:, None]                                       # [V,N]: |d pred| of every clip
    bar["dW"] += coef * (resid @ za) + 2.0 * lam * dWt
    bar["dbias"] += coef[:, 0] * resid.sum(1)
    # (W*, b*) itself: the emulator's fp64 solution leaves the gradient at rounding level (test_cpu_ridge_wfit_emul asserts it)
    for key in ("dW", "dbias"):
        ratio = float((tot[key].abs() / bar[key].clamp_min(1e-300)).max())
        print(f"{kind}/{wkind} {key}: max |sum| {float(tot[key].abs().max()):.3e}, max |sum| / bar {ratio:.3f}")
        assert bool(tot[key].abs().le(bar[key]).all()), key
    dead = torch.from_numpy(~keep)
    assert not bool(tot["dbias"][dead].any()) and not bool(tot["dW"][dead].any())
    head.set_target_weights(None)


# ---------------------------------------------------------------------------------------------------- 4: through the module
MGRID = [1e-4, 1e-2, 1.0]
SUBJECTS = ["sub-01", "sub-02"]


def _mask_files(tmp_path):
    rng = np.random.default_rng(3)
    masks = []
    for s in SUBJECTS:
        keep = rng.random(128) < 0.6
        keep[0] = True
        np.save(tmp_path / f"mask_{s}.npy", keep)
        masks.append(keep)
    return str(tmp_path / "mask_{subject}.npy"), np.stack(masks)


def _plant_nan(ds, masks):
    """NaN into the masked targets of every clip ``ds`` serves: each file's ``get`` goes through a wrapper"""
    for i, ent in ds.ds_files.items():
        f, g = ent["ds_file"], ds.subject_of[i]

        def get(k, mod, orig=f.get, g=g):
            a = orig(k, mod)
            if mod == "timeseries":
                a = np.array(a, dtype=np.float32)
                a[..., ~masks[g]] = np.nan
            return a
        f.get = get


def _cfg_kw(path, weighted=True):
    kw = dict(subjects=SUBJECTS, cache_features=True, ridge_fit="closed_form", dropout_rate=0.0, l2_lambda=3e-3, ridge_lambda_grid=MGRID,
              ridge_cv_folds=2, ridge_cv_block=2, ridge_lambda_per_target=True, target_weights=path)
    if weighted:
        kw["ridge_fit_weighted"] = True
    return kw


def test_the_option_through_the_module(dev, tmp_path):
    from phantom_vlb_amd.litmodule import VLBLitModule
    from phantom_vlb_amd.trainer import Trainer, load_trainable_checkpoint, trainable_state
    from phantom_vlb_amd.utils import LogValAccuracyCallback
    path, masks = _mask_files(tmp_path)
    with pytest.raises(ValueError, match="closed_form"):                   # the option unset: refused with the existing message
        RF._cfg(**_cfg_kw(path, weighted=False))
    m = VLBLitModule(RF._cfg(**_cfg_kw(path)))
    m.configure_model()
    dm = RF._dm(SUBJECTS)
    _plant_nan(dm.datasets.train, masks)
    _plant_nan(dm.datasets.val, masks)
    fits, steps = [], []
    orig, ts = m.fit_ridge_closed_form, m.training_step

    def fit_spy(*a, **k):
        out = orig(*a, **k)
        torch.cuda.synchronize()
        fits.append(dict(global_step=tr.global_step, steps_before=len(steps), out=out, result=m.ridge_fit_result,
                         masters={n: t.clone() for n, t in m.head.master.items()},
                         logged={k2: v for k2, v in m.logged.items() if k2.startswith("ridge_fit/")}))
        return out

    def step_spy(batch):
        steps.append(1)
        return ts(batch)
    m.fit_ridge_closed_form, m.training_step = fit_spy, step_spy
    log = RF._Rec()
    tr = Trainer(max_epochs=2, val_check_interval=0.5, log_every_n_steps=1, logger=log, callbacks=[LogValAccuracyCallback()])
    tr.fit(m, dm)
    torch.cuda.synchronize()
    assert len(fits) == 1                                   # once, at the step test_gpu_ridge_rows' run fits at
    f = fits[0]
    assert (f["global_step"], f["steps_before"]) == (4, 4)
    lg, cv = f["logged"], f["result"]
    H, V, L = len(SUBJECTS), 128, len(MGRID)
    assert lg["ridge_fit/kept_targets"] == float(masks.sum()) and lg["ridge_fit/weight_levels"] == float(H)
    assert np.isfinite(lg["ridge_fit/train_mse_before"]) and np.isfinite(lg["ridge_fit/train_mse_after"])
    assert lg["ridge_fit/train_mse_after"] < lg["ridge_fit/train_mse_before"]
    assert [o["lambda_counts"] for o in f["out"]] == cv["lambda_counts"]
    assert sum(lg[f"ridge_fit/lambda_count_{i}"] for i in range(L)) == float(masks.sum())
    ch = cv["choice"].cpu().numpy()
    assert (ch[~masks] == -1).all() and (ch[masks] >= 0).all()
    Wf, bf = f["masters"][WN].view(H, V, -1).cpu(), f["masters"][BN].view(H, V).cpu()
    dead = torch.from_numpy(~masks)
    assert not bool(Wf[dead].any()) and not bool(bf[dead].any()) and bool(torch.isfinite(Wf).all()) and bool(Wf[~dead].any())
    rows = torch.from_numpy(np.where(masks, np.asarray(MGRID)[np.maximum(ch, 0)], cv["best_lambda"]).astype(np.float32)).flatten()
    assert torch.equal(m.head.l2_lambda_rows.cpu(), rows) and m.head.l2_lambda == cv["best_lambda"]
    vals = [r["val_corr_avg"] for r in log.rows if "val_corr_avg" in r]
    assert vals and all(np.isfinite(v) for v in vals)
    assert all(np.isfinite(r["train/brain_loss"]) for r in log.rows if "train/brain_loss" in r)
    # ---- both checkpoint routes carry the weights and the penalty rows
    tw = torch.from_numpy(masks.astype(np.float32))
    ck = {}
    m.on_save_checkpoint(ck)
    assert torch.equal(ck["vlb_target_weights"], tw) and torch.equal(ck["vlb_ridge_l2_lambda_rows"], rows)
    assert ck["vlb_ridge_l2_lambda"] == cv["best_lambda"]
    m2 = VLBLitModule(RF._cfg(**_cfg_kw(path)))
    m2.on_load_checkpoint({k: v for k, v in ck.items() if k.startswith(("vlb_ridge", "vlb_target"))})     # before the head exists
    m2.configure_model()
    assert torch.equal(m2.head.tw.cpu(), tw) and torch.equal(m2.head.l2_lambda_rows.cpu(), rows)
    st = trainable_state(m, 8)
    p = str(tmp_path / "last.ckpt")
    torch.save(st, p)
    m3 = VLBLitModule(RF._cfg(**_cfg_kw(path)))
    m3.configure_model()
    m3.configure_optimizers()
    assert load_trainable_checkpoint(m3, p) == 8
    assert torch.equal(m3.head.tw.cpu(), tw) and torch.equal(m3.head.l2_lambda_rows.cpu(), rows)
    assert torch.equal(m3.head.master[WN].cpu(), m.head.master[WN].cpu())


# ---------------------------------------------------------------------------------------------------- 5: unweighted is untouched
NEW = ("vlb_ridge_gram_accumulate_masked", "vlb_ridge_sumsq_accumulate_masked", "vlb_ridge_cv_score_rows")


@pytest.mark.parametrize("kind", ["plain", "subjects"])
def test_an_unweighted_fit_never_enters_the_new_entry_points(dev, monkeypatch, kind):
    from phantom_vlb_amd import _lib

    def refuse(*a):
        raise AssertionError("an entry point of the weighted fit was called")
    for name in NEW:
        monkeypatch.setattr(_lib.lib, name, refuse)
    head, cache, _, y, subject, K, block = _make(kind, dev)
    assert head.tw is None
    for weighted in (False, True):                          # weighted=True without weights: today's calls
        _feed(head, cache, y, subject, K, block, weighted=weighted)
        assert "tw" not in head._ridge
        cv = head.ridge_cv(GRID, per_target=True)
        head.ridge_solve(cv["best_lambda"])
        head.ridge_solve_rows(cv["choice"], GRID)
        head.ridge_stats_end()
    torch.cuda.synchronize()
