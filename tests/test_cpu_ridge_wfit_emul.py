"""The weighted closed-form fit above the kernels, on the CPU: tests/ridge_wfit_emul.py is the weighted
objective's minimiser (fp64 autograd of the objective restated in torch), its bit properties, its planted bugs fall outside the
bars of ridge_emul / ridge_cv_emul, and the config field, the host checks and the three new entry points.

The gradient bar: the emulator's (W, b) comes from normal equations whose residual is of order cond(A) 2^-53 of the right-hand
side; 1e-9 of the gradient's scale at W = 0, b = 0 (where it is the right-hand side itself) leaves seven decades over 2^-53."""
import ctypes
import math
import pathlib
import re
import subprocess

import numpy as np
import pytest
import torch

import ridge_cv_emul as CE
import ridge_emul as RE
import ridge_rows_emul as RR
import ridge_wfit_emul as WF

ROOT = pathlib.Path(__file__).resolve().parent.parent
N, E, V = 150, 48, 20
GRID = [1e-3, 1e-2, 1e-1, 1.0]
K, BLOCK = 3, 5


def _weights(kind, V=V, seed=0):
    rng = np.random.default_rng(100 + seed)
    keep = rng.random(V) < 0.6
    keep[:2] = True, False
    if kind == "mask":
        return keep.astype(np.float32)
    if kind == "scaled":
        return (0.3 * keep).astype(np.float32)
    if kind == "levels":
        return (keep * rng.choice([0.5, 1.0, 2.0], V)).astype(np.float32)
    raise KeyError(kind)


def _data(seed=5, n=N, e=E, v=V):
    return RR.planted_rows(N=n, E=e, V=v, seed=seed)


def _with_nan(y, w, fill=np.nan):
    y = y.copy()
    y[:, np.asarray(w) == 0] = fill
    return y


# ---------------------------------------------------------------------------------------------------- 1: the objective
def _grad(W, b, z, y, w, lam):
    """fp64 autograd of J = (1/N) sum_n sum_v w_v (W_v z_n + b_v - y_nv)^2 / Ws + sum_v lam_v ||W_v||^2 at (W, b)"""
    Wt, bt = torch.tensor(W, dtype=torch.float64, requires_grad=True), torch.tensor(b, dtype=torch.float64, requires_grad=True)
    zt, wt = torch.tensor(z, dtype=torch.float64), torch.tensor(np.asarray(w, np.float32).astype(np.float64))
    yt = torch.tensor(np.where(np.asarray(w) > 0, y, 0.0), dtype=torch.float64)
    lt = torch.as_tensor(np.broadcast_to(np.asarray(lam, np.float64), wt.shape).copy())
    d = zt @ Wt.T + bt - yt
    J = ((d * d) * wt).sum() / (zt.shape[0] * wt.sum()) + (lt * (Wt * Wt).sum(1)).sum()
    J.backward()
    return Wt.grad.numpy(), bt.grad.numpy()


@pytest.mark.parametrize("kind", ["mask", "scaled", "levels", "rows"])
def test_the_emulator_minimises_the_weighted_objective(kind):
    z, y = _data()
    w = _weights("levels" if kind == "rows" else kind)
    lam = 10.0 ** np.random.default_rng(1).uniform(-3, 0, V) if kind == "rows" else 1e-2
    sol = WF.solve_w(WF.sums_w(z, _with_nan(y, w), w, chunk=64), lam, w)
    gW, gb = _grad(sol["W"], sol["b"], z, y, w, lam)
    g0W, g0b = _grad(np.zeros((V, E)), np.zeros(V), z, y, w, lam)
    scale = max(np.abs(g0W).max(), np.abs(g0b).max())
    print(f"{kind}: |grad| / scale {max(np.abs(gW).max(), np.abs(gb).max()) / scale:.2e}, levels {len(sol['lv']['scale'])}")
    assert max(np.abs(gW).max(), np.abs(gb).max()) <= 1e-9 * scale
    masked = w == 0
    assert masked.any() and not sol["W"][masked].any() and not sol["b"][masked].any()
    assert not np.signbit(sol["W"][masked]).any() and not np.signbit(sol["b"][masked]).any()
    assert np.abs(sol["W"][~masked]).min(1).max() > 0


def test_three_heads_with_their_own_masks_each_minimise_their_own_objective():
    z, y = _data(seed=6)
    sub = np.random.default_rng(2).integers(0, 3, N)
    for g in range(3):
        w = _weights(["mask", "scaled", "levels"][g], seed=g)
        rows = sub == g
        sol = WF.solve_w(WF.sums_w(z[rows], _with_nan(y[rows], w), w, chunk=32), 3e-2, w)
        gW, gb = _grad(sol["W"], sol["b"], z[rows], y[rows], w, 3e-2)
        g0W, g0b = _grad(np.zeros((V, E)), np.zeros(V), z[rows], y[rows], w, 3e-2)
        assert max(np.abs(gW).max(), np.abs(gb).max()) <= 1e-9 * max(np.abs(g0W).max(), np.abs(g0b).max()), g
        assert not sol["W"][w == 0].any() and not sol["b"][w == 0].any()


# ---------------------------------------------------------------------------------------------------- 2: bit properties
def test_a_constant_row_is_the_unweighted_emulator_bit_for_bit():
    z, y = _data()
    plain = RE.solve(RE.sums(z, y, chunk=64), 1e-2)
    pcv = CE.cv(z, y, GRID, K, BLOCK, chunk=64)
    for c in (1.0, 0.3):
        w = np.full(V, c, np.float32)
        assert WF.levels(w)["scale"] == [1.0]
        sol = WF.solve_w(WF.sums_w(z, y, w, chunk=64), 1e-2, w)
        assert np.array_equal(sol["W"], plain["W"]) and np.array_equal(sol["b"], plain["b"])
        cv = WF.cv_w(z, y, w, GRID, K, BLOCK, chunk=64)
        assert np.array_equal(cv["r"], pcv["r"]) and np.array_equal(cv["means"], pcv["means"])
        assert cv["best_index"] == pcv["best_index"]


@pytest.mark.parametrize("kind", ["mask", "scaled", "levels"])
def test_scaling_the_weights_by_four_changes_no_bit(kind):
    z, y = _data()
    w = _weights(kind)
    a, b = (WF.fit_w(z, y, ww, GRID, K, BLOCK, chunk=64) for ww in (w, 4 * w))
    assert WF.levels(w)["scale"] == WF.levels(4 * w)["scale"]
    for key in ("W", "b", "choice", "lambda_counts"):
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(a["cv"]["r"], b["cv"]["r"], equal_nan=True) and a["cv"]["score"].tolist() == b["cv"]["score"].tolist()


def test_a_mask_is_the_fit_of_the_kept_columns_alone():
    z, y = _data()
    w = _weights("mask")
    keep = w > 0
    assert WF.levels(w)["scale"] == [keep.sum() / V]
    sol = WF.solve_w(WF.sums_w(z, y, w, chunk=64), 1e-2, w)
    ref = RE.solve(RE.sums(z, y[:, keep], chunk=64), 1e-2)                   # a K'-target head with the same lambda
    bar = RE.master_bar(ref["W"], RE.cond2(ref["A"]), E)
    assert np.all(np.abs(sol["W"][keep] - ref["W"]) <= bar)
    assert np.all(np.abs(sol["b"][keep] - ref["b"]) <= RE.master_bar(ref["b"], RE.cond2(ref["A"]), E))


@pytest.mark.parametrize("kind", ["mask", "levels"])
def test_what_a_masked_target_holds_changes_no_bit(kind):
    z, y = _data()
    w = _weights(kind)
    fits = [WF.fit_w(z, _with_nan(y, w, fill), w, GRID, K, BLOCK, chunk=64) for fill in (0.0, np.nan, np.inf, -np.inf)]
    for f in fits[1:]:
        for key in ("W", "b", "choice", "lambda_rows", "lambda_counts"):
            assert np.array_equal(f[key], fits[0][key]), key
        assert np.array_equal(f["cv"]["r"], fits[0]["cv"]["r"], equal_nan=True)
        assert f["cv"]["score"].tolist() == fits[0]["cv"]["score"].tolist() and np.isfinite(f["cv"]["score"]).all()
    r = fits[1]["cv"]["r"]
    assert np.isnan(r[..., w == 0]).all() and np.isfinite(r[..., w > 0]).all()
    s = WF.sums_w(z, _with_nan(y, w), w, chunk=64)
    assert not s["C"][w == 0].any() and not s["sy"][w == 0].any() and not np.signbit(s["C"][w == 0]).any()


# ---------------------------------------------------------------------------------------------------- 3: planted bugs
def test_planted_bugs_fall_outside_the_bars():
    z, y = _data()
    w = _weights("levels")
    keep = w > 0
    yn = _with_nan(y, w)
    s = WF.sums_w(z, yn, w, chunk=64)
    good = WF.solve_w(s, 1e-2, w)
    bar = np.zeros((V, E))
    for (d, _), sol in good["sols"].items():
        rows = good["lv"]["lvl"] == d
        bar[rows] = RE.master_bar(sol["W"], RE.cond2(sol["A"]), E)[rows]

    def outside(W):
        return not np.all(np.abs(W - good["W"]) <= bar)
    assert not outside(WF.solve_w(WF.sums_w(z, yn, w, chunk=32), 1e-2, w)["W"])          # another chunking stays inside
    for bug in ("no_ws_over_v", "w_inverted", "swap_levels"):
        assert outside(WF.solve_w(s, 1e-2, w, bug=bug)["W"]), bug
    leaked = WF.sums_w(z, yn, w, chunk=64, bug="mask_product")              # NaN * 0: the masked sums, exactly +0 by the select,
    assert np.isnan(leaked["C"][~keep]).all() and np.isnan(leaked["sy"][~keep]).all()     # hold NaN (the solve reports the column)
    assert not s["C"][~keep].any() and not s["sy"][~keep].any()
    unsolved = WF.solve_w(s, 1e-2, w, bug="masked_unsolved")
    assert unsolved["W"][~keep].all() and np.array_equal(unsolved["W"][keep], good["W"][keep])
    cv = WF.cv_w(z, yn, w, GRID, K, BLOCK, chunk=64, bars=True)
    assert cv["valid"].all()
    bad = WF.cv_w(z, yn, w, GRID, K, BLOCK, chunk=64, bug="mean_all_v")
    assert np.all(np.abs(bad["score"] - cv["score"]) > cv["score_bar"])
    swapped = WF.cv_w(z, yn, w, GRID, K, BLOCK, chunk=64, bug="swap_levels")
    assert not np.all(np.abs(swapped["r"] - cv["r"])[..., keep] <= cv["r_bar"][..., keep])
    fit, counted = (WF.fit_w(z, yn, w, GRID, K, BLOCK, chunk=64, bug=b, cv=cv) for b in (None, "count_masked"))
    assert fit["lambda_counts"].sum() == keep.sum() and counted["lambda_counts"].sum() == V
    assert (fit["choice"][0][~keep] == -1).all() and (fit["choice"][0][keep] >= 0).all()
    assert np.isnan(fit["rbest"][0][~keep]).all() and np.all(fit["lambda_rows"][0][~keep] == cv["best_lambda"])
    with pytest.raises(ValueError, match="kept target"):
        WF.solve_rows_w(s, GRID, np.where(keep, -1, 0), w)


SEEDS = {"mask": 5, "scaled": 5, "levels": 5}


@pytest.mark.parametrize("kind", list(SEEDS))
def test_the_chosen_inputs_separate_the_choices(kind):
    """the condition the device test puts on its inputs, met by the emulator alone: the global choice leads by more than two
    score bars and at most 1/8 of the kept (head, target) pairs have a per-target margin below 100 bars"""
    z, y = _data(seed=SEEDS[kind])
    w = _weights(kind)
    fit = WF.fit_w(z, _with_nan(y, w), w, GRID, K, BLOCK, chunk=64, bars=True)
    cv = fit["cv"]
    order = np.argsort(cv["score"])[::-1]
    assert cv["score"][order[0]] - cv["score"][order[1]] > 2 * cv["score_bar"].max()
    thin = fit["margins"][cv["keep"]] < 100
    print(f"{kind}: {int(thin.sum())} of {thin.size} kept pairs below 100 bars; counts {fit['lambda_counts'].tolist()}")
    assert thin.mean() <= 1 / 8


# ---------------------------------------------------------------------------------------------------- 4: config, host checks
def _cfg(**kw):
    from phantom_vlb_amd.litmodule import VLBLitModuleConfig
    base = dict(model_path="none", freeze_backbone=True, use_lora=False, lora_r=None, lora_alpha=None, lora_dropout=None,
                dropout_rate=0.0, num_target=6, l2_lambda=1e-3, lr=1e-3, betas=[0.9, 0.999], eps=1e-8, weight_decay=1e-2,
                lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=100, geometry="mini")
    base.update(kw)
    return VLBLitModuleConfig(**base)


CF = dict(ridge_fit="closed_form", cache_features=True)


def test_the_config_field_validates_and_gates_the_pair():
    assert _cfg().ridge_fit_weighted is False and _cfg(**CF, ridge_fit_weighted=True).ridge_fit_weighted is True
    for bad in (1, 0, "true", None):
        with pytest.raises(ValueError, match="ridge_fit_weighted"):
            _cfg(**CF, ridge_fit_weighted=bad)
    with pytest.raises(ValueError, match="closed_form"):
        _cfg(ridge_fit_weighted=True)
    with pytest.raises(ValueError, match="ridge_fit_weighted"):                # off: the refusal stands and names the option
        _cfg(**CF, target_weights="w.npy")
    assert _cfg(**CF, ridge_fit_weighted=True, target_weights="w.npy").target_weights == "w.npy"


def test_the_field_is_reachable_from_the_command_line():
    from phantom_vlb_amd.config import instantiate, load_config
    over = ["experiment=VLB_mini_synthetic", "litmodule.config.cache_features=true", "litmodule.config.ridge_fit=closed_form"]
    cfg = load_config(str(ROOT / "config"), over + ["litmodule.config.ridge_fit_weighted=true"])
    assert instantiate(cfg["litmodule"]["config"]).ridge_fit_weighted is True
    assert instantiate(load_config(str(ROOT / "config"), over)["litmodule"]["config"]).ridge_fit_weighted is False
    for name in ("VLB_mini_synthetic.yaml", "VLB_vllama2_friends_baseline.yaml"):
        assert "ridge_fit_weighted" in (ROOT / "config" / "experiment" / name).read_text()


def test_the_module_takes_weights_only_with_the_option():
    from phantom_vlb_amd.litmodule import VLBLitModule
    w = torch.tensor([1.0, 0.0, 0.5, 2.0, 0.0, 1.0])
    off = VLBLitModule(_cfg(**CF))
    with pytest.raises(ValueError, match="ridge_fit_weighted"):
        off.set_target_weights(w)
    on = VLBLitModule(_cfg(**CF, ridge_fit_weighted=True))
    on.set_target_weights(w)
    assert on.target_weight_mask().tolist() == [[True, False, True, True, False, True]]
    on.set_target_weights(None)
    nine = torch.arange(1, 10, dtype=torch.float32)
    m9 = VLBLitModule(_cfg(**CF, ridge_fit_weighted=True, num_target=9))
    with pytest.raises(ValueError, match=r"the head holds 9 distinct positive weights.*at most 8"):
        m9.set_target_weights(nine)
    ms = VLBLitModule(_cfg(**CF, ridge_fit_weighted=True, num_target=9, subjects=["a", "b"]))
    with pytest.raises(ValueError, match=r"head 1 \('b'\) holds 9 distinct"):
        ms.set_target_weights(torch.stack([torch.ones(9), nine]))
    VLBLitModule(_cfg(num_target=9)).set_target_weights(nine)              # without the closed-form fit any weights go


def test_the_head_takes_weights_only_when_begun_weighted():
    from phantom_vlb_amd.head import BrainHead, target_weight_levels
    h = BrainHead(8, 4, 1e-3, 1e-5, "cpu")
    h.ridge_stats_begin(weighted=True)                                       # no weights set: today's stats
    assert "tw" not in h._ridge
    h.set_target_weights(torch.tensor([1.0, 0.0, 0.5, 0.0]))
    with pytest.raises(ValueError, match="target weights.*weighted=True"):
        h.ridge_stats_begin()
    with pytest.raises(ValueError, match="target weights"):
        h.ridge_stats_begin(folds=2, block=1, weighted=False)
    h.ridge_stats_begin(folds=2, block=1, weighted=True)
    st = h._ridge
    assert st["lvl"].tolist() == [[1, -1, 0, -1]] and st["kept"] == [2] and st["keep"].tolist() == [[True, False, True, False]]
    assert st["scale"] == [[1.5 / (4 * 0.5), 1.5 / (4 * 1.0)]]
    h.set_target_weights(torch.tensor([1.0, 1.0, 1.0, 1.0]))              # the stats keep the weights of their begin
    assert st["tw"].tolist() == [[1.0, 0.0, 0.5, 0.0]]
    # -1 at a kept target is refused before any launch
    st["n"] = [4]
    for bad in ([-1, -1, 0, -1], [0, -1, 2, -1], [0, -2, 0, -1]):
        with pytest.raises(ValueError, match="masked targets only"):
            h.ridge_solve_rows(torch.tensor([bad], dtype=torch.int32), [1e-2, 1e-1])
    h.ridge_stats_end()
    g = BrainHead(8, 9, 1e-3, 1e-5, "cpu", subjects=["a", "b"])
    g.set_target_weights(torch.stack([torch.ones(9), torch.arange(1, 10, dtype=torch.float32)]))
    with pytest.raises(ValueError, match=r"head 1 \('b'\) holds 9 distinct positive weights"):
        g.ridge_stats_begin(weighted=True)
    # the host's levels are the emulator's
    for kind in ("mask", "scaled", "levels"):
        w = _weights(kind)
        lv, emu = target_weight_levels(torch.from_numpy(w)[None]), WF.levels(w)
        assert lv["lvl"][0] == emu["lvl"].tolist() and lv["scale"][0] == emu["scale"] and lv["levels"] == [len(emu["scale"])]
    for c in (1.0, 0.3, 1e-3):
        assert target_weight_levels(torch.full((1, 1000), c))["scale"] == [[1.0]]
    w = torch.tensor([[0.1, 0.2, 0.7, 0.0]])
    assert target_weight_levels(w)["scale"][0][0] == math.fsum(w[0].tolist()) / (4 * float(w[0, 0]))


NEW = ("vlb_ridge_gram_accumulate_masked", "vlb_ridge_sumsq_accumulate_masked", "vlb_ridge_cv_score_rows")


def test_entry_points_are_declared_bound_and_exported():
    from phantom_vlb_amd import _lib
    header = (ROOT / "include" / "vlb.h").read_text()
    assert re.search(r"#define VLB_ABI_VERSION 2\b", header) and _lib.lib.vlb_abi_version() == 2
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()[-2] == "T"}
    want = {ctypes.c_void_p: "P", ctypes.c_int: "I", ctypes.c_float: "F"}
    flat = re.sub(r"\s+", " ", header)
    doc = re.search(r"/\*((?:(?!\*/).)*)\*/ int vlb_ridge_gram_accumulate_masked\(", flat)
    assert doc and "a select" in doc.group(1) and "+0.0" in doc.group(1)
    mapped = (ROOT / "phantom_vlb_amd" / "csrc" / "libvlb.map").read_text()
    for name in NEW:
        m = re.search(r"\bint " + name + r"\(([^)]*)\);", text)
        assert m, f"{name} is not declared in include/vlb.h"
        args = [a.strip() for a in m.group(1).split(",")]
        kinds = ["P" if "*" in a else "F" if a.startswith("float ") else "I" if a.startswith("int ") else "?" for a in args]
        assert kinds == [want[t] for t in _lib.SIGNATURES[name]], (name, kinds)
        assert name in exported and name in mapped
        assert re.search(name + r" \(src/utils\.py:59-73", doc.group(1)), f"{name} does not cite the reference"
    m = re.search(r"\bint vlb_ridge_solve\(([^)]*)\);", text)
    assert len(m.group(1).split(",")) == 14 == len(_lib.SIGNATURES["vlb_ridge_solve"])
    for old in ("vlb_ridge_gram_accumulate", "vlb_ridge_sumsq_accumulate", "vlb_ridge_cv_score", "vlb_ridge_solve_rows", "vlb_ridge_cv_select"):
        assert old in _lib.SIGNATURES and old in exported


def test_the_new_entries_refuse_bad_arguments_without_a_device():
    from phantom_vlb_amd._lib import lib
    p = 64                                                                      # never dereferenced: every call is refused first
    gram = lambda **k: lib.vlb_ridge_gram_accumulate_masked(*[{**dict(z=p, y=p, ldy=4, keep=p, G=p, C=p, sz=p, sy=p, n=2, E=3, V=4,
                                                                     st=None), **k}[a] for a in
                                                              ("z", "y", "ldy", "keep", "G", "C", "sz", "sy", "n", "E", "V", "st")])
    for bad in (dict(z=None), dict(y=None), dict(keep=None), dict(G=None), dict(C=None), dict(sz=None), dict(sy=None), dict(n=0),
                dict(E=0), dict(V=0), dict(ldy=3), dict(keep=p + 2)):
        assert gram(**bad) != 0, bad
        assert b"ridge_gram_accumulate_masked" in lib.vlb_last_error()
    sq = lambda y=p, ldy=4, keep=p, syy=p, n=2, V=4: lib.vlb_ridge_sumsq_accumulate_masked(y, ldy, keep, syy, n, V, None)
    for bad in (dict(y=None), dict(keep=None), dict(syy=None), dict(n=0), dict(V=0), dict(ldy=3), dict(keep=p + 1)):
        assert sq(**bad) != 0, bad
        assert b"ridge_sumsq_accumulate_masked" in lib.vlb_last_error()
    rows = lambda X=p, Gc=p, Rc=p, vy=p, ws=p, r=p, info=p, E=3, V=4, choice=p, want=0: lib.vlb_ridge_cv_score_rows(
        X, Gc, Rc, vy, ws, r, info, E, V, choice, want, None)
    for bad in (dict(X=None), dict(Gc=None), dict(Rc=None), dict(vy=None), dict(ws=None), dict(r=None), dict(info=None),
                dict(choice=None), dict(E=0), dict(V=0), dict(want=-1)):
        assert rows(**bad) != 0, bad
        assert b"ridge_cv_score_rows" in lib.vlb_last_error()
