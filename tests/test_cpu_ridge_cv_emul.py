"""Choosing ``l2_lambda`` by blocked K-fold cross-validation, host side: the fp64 emulator
(tests/ridge_cv_emul.py) proved against the explicit held-out correlation, the condition on the planted recipe that the GPU
tests rely on, its planted bugs, the fold assignment, the config refusals and the new ABI entries.  No GPU.

The planted recipe (``planted``, seed 5: a seed at which fold 0 alone would choose another grid point): N = 300 clips, E = 96
features of mean 0.5 (bf16 valued), V = 40 targets from weights that are 20 % dense plus noise of sd 6, K = 5 folds of blocks
of 12 clips, seven lambdas 1e-6 .. 1.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ridge_cv_emul as CE
import ridge_emul as RE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = [10.0 ** p for p in range(-6, 1)]
NEW_ENTRIES = {"vlb_ridge_sumsq_accumulate": 6, "vlb_f64_sum_except": 7, "vlb_ridge_cv_center": 12, "vlb_ridge_cv_score": 10}


def _bf16(x):
    return torch.from_numpy(np.asarray(x, np.float32)).to(torch.bfloat16).float().numpy().astype(np.float64)


def _ar1(rng, n, m, rho):
    e = rng.standard_normal((n, m))
    for t in range(1, n):
        e[t] = rho * e[t - 1] + np.sqrt(1 - rho * rho) * e[t]
    return e


def planted(N=300, E=96, V=40, seed=5, rho=0.0, noise=6.0, mean=0.5, dens=0.2):
    """z bf16-valued [N,E] (lag-1 autocorrelation ``rho``, in the noise of y too), y fp32-valued [N,V]"""
    rng = np.random.default_rng(seed)
    z = _bf16(_ar1(rng, N, E, rho) + mean)
    W = rng.standard_normal((V, E)) * (rng.random((V, E)) < dens)
    y = (z @ W.T + rng.uniform(-2, 2, V) + noise * _ar1(rng, N, V, rho)).astype(np.float32).astype(np.float64)
    return z, y


@pytest.fixture(scope="module")
def recipe():
    z, y = planted()
    return z, y, CE.cv(z, y, GRID, 5, 12, bars=True)


# ---------------------------------------------------------------------------------------------------- (a)
def test_moment_form_is_the_explicit_held_out_correlation(recipe):
    """r from the fold's moments = the two-pass Pearson r of Z_k X^T + b against Y_k, for every (fold, lambda, target); with
    b = 0 as well: the bias does not enter.  Bar: the moment form's own r bar for the same X on both sides (no dX) - the
    explicit form is evaluated in extended precision, so what separates the two is the fp64 forming of the fold's sums and
    moments, which that bar bounds; without extended precision the explicit form's own fp64 rounding (well conditioned:
    two-pass, centred) is allowed the same again."""
    z, y, c = recipe
    worst = worst_abs = 0.0
    for k in range(5):
        S, rows = c["S"][0], c["S"][0][k]["rows"]
        Gc, Rc, vy = CE.moments(S[k])
        dGc, dRc, dvy = CE.moment_bars(z[rows], y[rows], S[k])
        for i, lam in enumerate(GRID):
            sol = CE.solve_fold(S, k, lam)
            b = CE.r_bar(sol["W"], Gc, Rc, vy, dGc, dRc, dvy)
            assert b["valid"].all()
            bar = b["dr"] * (1 if CE.EXT else 2)
            for bias in (sol["b"], np.zeros_like(sol["b"])):
                d = np.abs(CE.explicit_r(z[rows], y[rows], sol["W"], bias) - c["r"][0, k, i])
                worst, worst_abs = max(worst, float(np.max(d / bar))), max(worst_abs, float(d.max()))
                assert np.all(d <= bar), (k, i, float(d.max()), float(bar.min()))
    print(f"moment form vs explicit r over 35 (fold, lambda) pairs: max err {worst_abs:.2e}, max err / bar {worst:.3e}")


# ---------------------------------------------------------------------------------------------------- (b)
def test_planted_recipe_has_an_interior_optimum_with_a_wide_margin(recipe):
    """The condition the GPU tests' argmax checks rest on: interior optimum, and the best score leads the runner-up by at
    least 100 x the score's bar - no device within its bars can choose another grid point."""
    _, _, c = recipe
    sc = c["score"]
    order = np.argsort(sc)[::-1]
    margin, bar = float(sc[order[0]] - sc[order[1]]), float(c["score_bar"].max())
    print(f"scores {np.round(sc, 5).tolist()}, best index {c['best_index']} (lambda {c['best_lambda']}), margin {margin:.3e}, "
          f"score bar {bar:.3e}")
    assert c["valid"].all()
    assert 0 < c["best_index"] < len(GRID) - 1 and c["best_index"] == order[0]
    assert margin >= 100 * bar


# ---------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("bug", CE.BUGS)
def test_every_planted_bug_changes_the_choice_or_an_r_beyond_its_bar(recipe, bug):
    z, y, c = recipe
    if bug == "interleaved":
        # neighbouring clips share their features' and their noise's past (lag-1 autocorrelation 0.9): dealing single clips
        # round-robin puts each held-out clip between two training clips and the score rises
        z, y = planted(seed=1, rho=0.9)
        c = CE.cv(z, y, GRID, 5, 12, bars=True)
    bad = CE.cv(z, y, GRID, 5, 12, bug=bug)
    dr = np.abs(bad["r"] - c["r"])
    moved, changed = bool(np.any(dr > c["r_bar"])), bad["best_index"] != c["best_index"]
    print(f"{bug}: best index {c['best_index']} -> {bad['best_index']}, max |dr| {dr.max():.3e} (bar {np.nanmax(c['r_bar']):.1e}), "
          f"best score {c['score'].max():.4f} -> {bad['score'].max():.4f}")
    assert moved or changed
    if bug == "argmax_first_fold":
        assert changed and not moved                  # the table is the same: only the decision differs
    if bug in ("leak", "interleaved"):
        assert bad["score"].max() > c["score"].max() + 100 * c["score_bar"].max()        # leaking inflates the score


def test_tie_goes_to_the_larger_lambda_and_excluded_points_do_not_win():
    means = np.array([[[0.5, 0.7, 0.7, 0.1], [0.5, 0.7, 0.7, 0.1]]])
    assert CE.select(means, [1e-3, 1e-2, 1e-1, 1.0])["best_index"] == 2
    assert CE.select(means, [1e-3, 1e-1, 1e-2, 1.0])["best_index"] == 1
    assert CE.select(means, [1e-3, 1e-2, 1e-1, 1.0], ok=[True, True, False, True])["best_index"] == 1
    with pytest.raises(ValueError):
        CE.select(means, [1e-3, 1e-2, 1e-1, 1.0], ok=[False] * 4)


# ---------------------------------------------------------------------------------------------------- (d)
def test_fold_assignment_ignores_the_chunking_and_is_per_head():
    n, K, block = 101, 4, 7
    one = CE.assign(n, K, block, chunk=n)
    assert np.array_equal(one, (np.arange(n) // block) % K)
    for chunk in (1, 5, 7, 64, 512):
        assert np.array_equal(CE.assign(n, K, block, chunk=chunk), one)
    sub = np.random.default_rng(0).integers(0, 3, n)
    ref = CE.assign(n, K, block, sub=sub, chunk=n)
    for g in range(3):
        rows = np.nonzero(sub == g)[0]
        assert np.array_equal(ref[rows], (np.arange(len(rows)) // block) % K)       # each head counts its own clips
    for chunk in (1, 5, 64):
        assert np.array_equal(CE.assign(n, K, block, sub=sub, chunk=chunk), ref)
    # integer sums: the folds' totals are the fold-free sums, any chunking
    rng = np.random.default_rng(1)
    z, y = rng.integers(-3, 4, (n, 12)).astype(np.float64), rng.integers(-4, 5, (n, 5)).astype(np.float64)
    whole = RE.sums(z, y, chunk=n)
    for chunk in (n, 9):
        S = CE.fold_sums(z, y, one, K, chunk)
        T = CE.sum_except(S, -1)
        assert all(np.array_equal(T[k], whole[k]) for k in ("G", "C", "sz", "sy")) and T["n"] == n
        assert np.array_equal(T["syy"], (y * y).sum(0))


def test_head_partitions_a_chunk_by_head_and_fold_on_the_host():
    """BrainHead.ridge_stats_add's own bookkeeping (no launch: features and kernels replaced by recorders)."""
    from phantom_vlb_amd import head as H
    h = H.BrainHead(8, 4, 1e-3, 1e-5, "cpu", subjects=["a", "b", "c"])
    h.ridge_stats_begin(folds=3, block=2)
    st = h._ridge
    assert tuple(st["G"].shape) == (3, 3, 8, 8) and tuple(st["syy"].shape) == (3, 3, 4) and st["G"].dtype == torch.float64
    seen = []
    h.features_cached = lambda cache, ids: (seen.append(ids.tolist()), torch.zeros(len(ids), 8, dtype=torch.bfloat16))[1]
    calls = []

    class _Lib:
        def __getattr__(self, name):
            if name == "vlb_ridge_gram_accumulate":
                return lambda *a: calls.append(("gram", a[7])) or 0
            if name == "vlb_ridge_sumsq_accumulate":
                return lambda *a: calls.append(("sumsq", a[3])) or 0
            raise AssertionError(f"{name} launched")
    H_lib, H_stream, H.lib, H._stream = H.lib, H._stream, _Lib(), lambda: None
    try:
        n = 23
        sub = np.random.default_rng(3).integers(0, 3, n)
        for lo, hi in RE.chunks_of(n, 5):
            h.ridge_stats_add(None, torch.arange(lo, hi), torch.zeros(hi - lo, 4), sub[lo:hi])
    finally:
        H.lib, H._stream = H_lib, H_stream
    want = CE.assign(n, 3, 2, sub=sub, chunk=5)
    for g in range(3):
        assert st["n"][g] == int((sub == g).sum())
        assert st["n_fold"][g] == [int(((sub == g) & (want == k)).sum()) for k in range(3)]
    assert sorted(i for ids in seen for i in ids) == list(range(n))
    for ids in seen:                                   # every launch: one head, one fold, index order
        assert len({(int(sub[i]), int(want[i])) for i in ids}) == 1 and ids == sorted(ids)
    assert [c[0] for c in calls] == ["gram", "sumsq"] * len(seen) and [c[1] for c in calls[::2]] == [len(ids) for ids in seen]
    # the errors that precede any launch
    st["n_fold"][1][2] = 1
    with pytest.raises(ValueError, match=r"head 1 \('b'\).*fold 2 of 3 holds 1 clip"):
        h.ridge_cv([1e-3, 1e-2])
    with pytest.raises(ValueError, match="positive"):
        h.ridge_cv([1e-3, 0.0])
    h.ridge_stats_end()
    h.ridge_stats_begin()
    with pytest.raises(RuntimeError, match="folds"):
        h.ridge_cv([1e-3, 1e-2])
    with pytest.raises(ValueError, match="folds >= 2"):
        h.ridge_stats_begin(folds=1, block=4)
    with pytest.raises(ValueError, match="block >= 1"):
        h.ridge_stats_begin(folds=2, block=0)


# ---------------------------------------------------------------------------------------------------- (e)
def _cfg(**kw):
    from phantom_vlb_amd.litmodule import VLBLitModuleConfig
    base = dict(model_path="none", freeze_backbone=True, use_lora=False, lora_r=None, lora_alpha=None, lora_dropout=None,
                dropout_rate=0.1, num_target=128, l2_lambda=1e-3, lr=1e-3, betas=[0.9, 0.999], eps=1e-8,
                weight_decay=1e-2, lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=50000, geometry="mini")
    base.update(kw)
    return VLBLitModuleConfig(**base)


def test_config_accepts_and_refuses():
    c = _cfg()
    assert c.ridge_lambda_grid is None and c.ridge_cv_folds == 5 and c.ridge_cv_block == 128
    on = dict(cache_features=True, ridge_fit="closed_form")
    c = _cfg(ridge_lambda_grid=[1e-4, 1e-2, 1], ridge_cv_folds=2, ridge_cv_block=1, **on)
    assert c.ridge_lambda_grid == [1e-4, 1e-2, 1.0] and all(isinstance(x, float) for x in c.ridge_lambda_grid)
    assert _cfg(ridge_lambda_grid=[5e-2, 7e-2], l2_lambda=1e-3, **on).l2_lambda == 1e-3       # need not be in the grid
    with pytest.raises(ValueError, match=r"ridge_lambda_grid.*ridge_fit='closed_form'"):
        _cfg(ridge_lambda_grid=[1e-3, 1e-2])
    with pytest.raises(ValueError, match=r"ridge_lambda_grid.*two or more distinct"):
        _cfg(ridge_lambda_grid=[1e-3], **on)
    with pytest.raises(ValueError, match=r"ridge_lambda_grid.*two or more distinct"):
        _cfg(ridge_lambda_grid=[1e-3, 1e-3], **on)
    with pytest.raises(ValueError, match=r"ridge_lambda_grid.*two or more distinct"):
        _cfg(ridge_lambda_grid=[], **on)
    for bad in (0.0, -1e-3, float("nan"), float("inf"), "x", True):
        with pytest.raises(ValueError, match=r"ridge_lambda_grid.*> 0"):
            _cfg(ridge_lambda_grid=[1e-3, bad], **on)
    with pytest.raises(ValueError, match=r"ridge_lambda_grid.*a list"):
        _cfg(ridge_lambda_grid=1e-3, **on)
    for bad in (1, 0, -3, 2.5, True):
        with pytest.raises(ValueError, match=r"ridge_cv_folds.*>= 2"):
            _cfg(ridge_cv_folds=bad)
    for bad in (0, -1, 1.5, False):
        with pytest.raises(ValueError, match=r"ridge_cv_block.*>= 1"):
            _cfg(ridge_cv_block=bad)


def test_yaml_plumbing_reaches_the_fields():
    from phantom_vlb_amd.config import instantiate, load_config
    cdir = os.path.join(ROOT, "config")
    plain = load_config(cdir, ["experiment=VLB_mini_synthetic"])
    assert "ridge_lambda_grid" not in plain["litmodule"]["config"]
    assert instantiate(plain["litmodule"]["config"]).ridge_lambda_grid is None
    cfg = load_config(cdir, ["experiment=VLB_mini_synthetic", "litmodule.config.cache_features=true",
                             "litmodule.config.ridge_fit=closed_form", "litmodule.config.ridge_lambda_grid=[1e-4,1e-3,1e-2]",
                             "litmodule.config.ridge_cv_block=2", "litmodule.config.ridge_cv_folds=2"])
    c = instantiate(cfg["litmodule"]["config"])
    assert c.ridge_lambda_grid == [1e-4, 1e-3, 1e-2] and (c.ridge_cv_folds, c.ridge_cv_block) == (2, 2)
    text = open(os.path.join(cdir, "experiment", "VLB_vllama2_friends_baseline.yaml")).read()
    assert all(k in text for k in ("ridge_lambda_grid", "ridge_cv_folds", "ridge_cv_block"))


def test_unset_grid_adds_nothing_and_the_checkpoint_carries_the_choice():
    from phantom_vlb_amd.head import BrainHead
    from phantom_vlb_amd.litmodule import VLBLitModule
    h = BrainHead(8, 4, 1e-3, 1e-5, "cpu")
    h.ridge_stats_begin()
    assert sorted(h._ridge) == ["C", "G", "n", "sy", "sz"] and tuple(h._ridge["G"].shape) == (1, 8, 8)     # as before the option
    m = VLBLitModule(_cfg(cache_features=True, ridge_fit="closed_form"))
    m.rng_state = lambda: {}
    ck = {}
    m.on_save_checkpoint(ck)
    assert "vlb_ridge_l2_lambda" not in ck
    m._ridge_cv_lambda = 1e-2
    m.on_save_checkpoint(ck)
    assert ck["vlb_ridge_l2_lambda"] == 1e-2
    m2 = VLBLitModule(_cfg(cache_features=True, ridge_fit="closed_form", ridge_lambda_grid=[1e-3, 1e-2]))
    m2.set_rng_state = lambda s: None
    m2.head = h
    m2.on_load_checkpoint(ck)
    assert h.l2_lambda == 1e-2 and m2._ridge_cv_lambda == 1e-2


# ---------------------------------------------------------------------------------------------------- (f)
def test_new_entries_are_declared_bound_and_exported():
    """header == SIGNATURES == nm -D for the new entries (parameter kinds in the same positions), each citing the reference's
    RidgeRegressionLayer; the workspace query returns int64_t; ABI version still 2."""
    from phantom_vlb_amd import _lib
    raw = open(os.path.join(ROOT, "include", "vlb.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()[-2] == "T"}
    want = {ctypes.c_void_p: "P", ctypes.c_int: "I", ctypes.c_float: "F", ctypes.c_double: "D", ctypes.c_int64: "L"}

    def kind(p):
        return "P" if "*" in p else "F" if p.startswith("float") else "D" if p.startswith("double") else \
            "L" if p.startswith("int64_t") else "I"
    for name, n in NEW_ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
        assert m, f"{name} is not declared in include/vlb.h"
        params = [p.strip() for p in m.group(1).split(",")]
        assert len(params) == len(_lib.SIGNATURES[name]) == n, name
        assert [kind(p) for p in params] == [want[t] for t in _lib.SIGNATURES[name]], name
        assert params[-1] == "void* stream", name
        assert name in exported and hasattr(_lib.lib, name), name
        assert getattr(_lib.lib, name).restype is ctypes.c_int
        assert re.search(name + r" \(src/utils\.py:59-73", raw), f"{name} does not cite the reference's layer"
    assert re.search(r"\bint64_t\s+vlb_ridge_cv_ws_doubles\s*\(int E, int V\)", text)
    assert _lib.SIGNATURES["vlb_ridge_cv_ws_doubles"] == [ctypes.c_int, ctypes.c_int]
    assert _lib.lib.vlb_ridge_cv_ws_doubles.restype is ctypes.c_int64 and "vlb_ridge_cv_ws_doubles" in exported
    assert raw.index("visibility push") < raw.index("int vlb_ridge_cv_score(") < raw.index("visibility pop")
    assert _lib.lib.vlb_abi_version() == 2 and "#define VLB_ABI_VERSION 2" in raw


def test_entries_refuse_bad_arguments_without_a_device():
    from phantom_vlb_amd._lib import lib
    one = ctypes.c_void_p(16)
    assert lib.vlb_ridge_cv_ws_doubles(200, 70) == 70 * 4 and lib.vlb_ridge_cv_ws_doubles(4096, 1000) == 64000
    assert lib.vlb_ridge_cv_ws_doubles(1, 1) == 1 and lib.vlb_ridge_cv_ws_doubles(0, 4) == 0 and lib.vlb_ridge_cv_ws_doubles(64, 64) == 64
    assert lib.vlb_ridge_sumsq_accumulate(one, 4, None, 1, 4, None) != 0
    assert lib.vlb_ridge_sumsq_accumulate(one, 3, one, 1, 4, None) != 0 and b"ldy=3" in lib.vlb_last_error()
    assert lib.vlb_ridge_sumsq_accumulate(one, 4, one, 0, 4, None) != 0 and b"n=0" in lib.vlb_last_error()
    assert lib.vlb_f64_sum_except(one, 8, 3, 3, one, 8, None) != 0 and b"skip=3" in lib.vlb_last_error()
    assert lib.vlb_f64_sum_except(one, 8, 3, -2, one, 8, None) != 0 and lib.vlb_f64_sum_except(one, 4, 3, 0, one, 8, None) != 0
    assert lib.vlb_f64_sum_except(one, 8, 0, -1, one, 8, None) != 0 and lib.vlb_f64_sum_except(None, 8, 3, 0, one, 8, None) != 0
    assert lib.vlb_ridge_cv_center(one, one, one, one, one, 0, one, one, one, 8, 4, None) != 0 and b"n_k=0" in lib.vlb_last_error()
    assert lib.vlb_ridge_cv_center(one, one, one, one, None, 5, one, one, one, 8, 4, None) != 0
    assert lib.vlb_ridge_cv_score(one, one, one, one, one, one, None, 8, 4, None) != 0
    assert lib.vlb_ridge_cv_score(one, one, one, one, one, one, one, 0, 4, None) != 0 and b"E=0" in lib.vlb_last_error()
