"""One ``l2_lambda`` per target in the closed-form ridge fit, host side: the fp64 emulator
(tests/ridge_rows_emul.py) proved against the objective itself, the condition on the planted recipe that the GPU tests rely on,
its planted bugs, the selection rules on hand-made tables, the config refusals, the checkpoint keys and the new ABI entries.
No GPU.

The recipe (``ridge_rows_emul.planted_rows``): test_cpu_ridge_cv_emul's ``planted`` (N = 300 clips, E = 96 features of mean
0.5, V = 40 targets, K = 5 folds of blocks of 12 clips, seven lambdas 1e-6 .. 1) with a noise sd per target
(geomspace(0.3, 40, V), permuted) and a weight density per target (geomspace(0.03, 0.8, V)); seeds 5, 6 and 7.

Bars (derivations in ridge_rows_emul's and test_cpu_ridge_emul's docstrings): the gradient at the solution is bounded row by
row by the solve's residual bar of the factorisation that row came from; lstsq against Cholesky per row by twice
cond_2(A_v) gamma_{3E+1} || |L||L|^T ||_F / ||A_v||_2.
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
import ridge_rows_emul as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = [10.0 ** p for p in range(-6, 1)]
K, BLOCK = 5, 12
SEEDS = (5, 6, 7)
NEW_ENTRIES = {"vlb_ridge_cv_select": 10, "vlb_ridge_solve_rows": 16, "vlb_head_l2_rows_fwd": 7, "vlb_head_l2_rows_bwd": 7}


@pytest.fixture(scope="module")
def recipes():
    out = {}
    for seed in SEEDS:
        z, y = RR.planted_rows(seed=seed)
        out[seed] = (z, y, RR.fit(z, y, GRID, K, BLOCK, bars=True))
    return out


# ---------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("seed", SEEDS)
def test_solve_rows_minimises_the_objective_with_a_penalty_per_target(recipes, seed):
    z, y, f = recipes[seed]
    N, E = z.shape
    V = y.shape[1]
    W, b, lam, choice = f["W"][0], f["b"][0], f["lambda_rows"][0], f["choice"][0]
    sols = RR.solve_rows(CE.sum_except(f["cv"]["S"][0], -1), GRID, choice)["sols"]
    dW, db, mag_W, mag_b = RR.gradient_rows(W, b, z, y, lam)
    ev = (N + E + 8) * RE.U64
    zbar, ybar = z.mean(0), y.mean(0)
    b_err = (E + 4) * RE.U64 * (np.abs(ybar) + np.abs(W) @ np.abs(zbar))
    res = np.zeros_like(W)
    for i, sol in sols.items():                           # each row against the factorisation it came from
        res[choice == i] = RE.solve_bar(sol["L"], W[choice == i])
    bar_W = 2.0 / (N * V) * (res + np.outer(b_err, np.abs(z).sum(0))) + ev * mag_W
    bar_b = ev * mag_b + 2.0 / V * b_err
    print(f"seed {seed}: max |dW|/bar {np.max(np.abs(dW) / bar_W):.3f}, max |db|/bar {np.max(np.abs(db) / bar_b):.3f}, "
          f"max|dW| {np.abs(dW).max():.2e} of terms {mag_W.max():.2e}")
    assert np.all(np.abs(dW) <= bar_W) and np.all(np.abs(db) <= bar_b)
    J0 = RR.objective_rows(W, b, z, y, lam)[2]
    rng = np.random.default_rng(1)
    for _ in range(5):
        assert RR.objective_rows(W + 1e-3 * rng.standard_normal(W.shape), b + 1e-3 * rng.standard_normal(b.shape), z, y, lam)[2] > J0
    # with one lambda for every row the penalty, and so the solution, is the scalar one's
    same = RR.solve_rows(CE.sum_except(f["cv"]["S"][0], -1), GRID, np.full(V, 3))
    ref = RE.solve(CE.sum_except(f["cv"]["S"][0], -1), GRID[3])
    assert np.array_equal(same["W"], ref["W"]) and np.array_equal(same["b"], ref["b"])
    assert RR.objective_rows(ref["W"], ref["b"], z, y, np.full(V, GRID[3])) == pytest.approx(RE.objective(ref["W"], ref["b"], z, y, GRID[3]), rel=1e-13)


def test_each_row_equals_lstsq_on_its_own_augmented_system(recipes):
    z, y, f = recipes[5]
    E = z.shape[1]
    W, b, choice = f["W"][0], f["b"][0], f["choice"][0]
    sols = RR.solve_rows(CE.sum_except(f["cv"]["S"][0], -1), GRID, choice)["sols"]
    worst = 0.0
    for v in range(y.shape[1]):
        sol = sols[int(choice[v])]
        Lm = np.abs(sol["L"])
        rel = 2 * RE.cond2(sol["A"]) * RE.gamma(3 * E + 1) * np.linalg.norm(Lm @ Lm.T) / np.linalg.norm(sol["A"], 2)
        w2, b2 = RR.lstsq_row(z, y, v, GRID[choice[v]])
        err = np.linalg.norm(W[v] - w2) / np.linalg.norm(w2)
        worst = max(worst, err / rel)
        assert err <= rel, (v, err, rel)
        bar_b = rel * np.linalg.norm(w2) * np.linalg.norm(z.mean(0)) + (E + 4) * RE.U64 * (abs(y[:, v].mean()) + np.abs(w2) @ np.abs(z.mean(0)))
        assert abs(b[v] - b2) <= bar_b
    print(f"rows against lstsq: max err / bar {worst:.3e}")


# ---------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("seed", SEEDS)
def test_recipe_separates_every_targets_best_two_grid_points(recipes, seed):
    """The condition the GPU tests' per-target choices rest on: EVERY target's best rmean leads its runner-up by at least 100 x
    the larger of the two bars, at least 4 distinct grid points are chosen and some target leaves the global choice."""
    _, _, f = recipes[seed]
    cv, choice = f["cv"], f["choice"][0]
    m = f["margins"][0]
    gap = np.sort(f["rmean"][0], 0)
    print(f"seed {seed}: counts {f['lambda_counts'][0].tolist()}, global choice {cv['best_index']}, min margin {m.min():.0f} bars, "
          f"bars <= {f['rmean_bar'].max():.2e}, margins >= {(gap[-1] - gap[-2]).min():.2e}; mean held-out r global "
          f"{cv['score'][cv['best_index']]:.3f}, per target {f['score_per_target']:.3f}")
    assert cv["valid"].all()
    assert np.all(m >= 100), (int(np.argmin(m)), float(m.min()))
    assert len(set(choice.tolist())) >= 4
    assert np.any(choice != cv["best_index"])
    assert f["lambda_counts"].sum() == choice.size
    # per-target selection can only raise the (optimistic) score, and the table's global view is the parent's
    assert f["score_per_target"] >= cv["score"][cv["best_index"]]
    assert np.array_equal(f["rbest"][0], f["rmean"][0].max(0))


# ---------------------------------------------------------------------------------------------------- 3
def _tied_unsorted(r):
    """the recipe's table with its grid shuffled and every column duplicated under another lambda: exact ties everywhere, the
    larger lambda of each pair at the LOWER index"""
    L = r.shape[1]
    perm = np.random.default_rng(0).permutation(L)
    grid = [GRID[i] * 3.0 for i in perm] + [GRID[i] for i in perm]        # column j and column L + j hold the same values
    return np.concatenate([r[:, perm], r[:, perm]], 1), grid


@pytest.mark.parametrize("bug", RR.BUGS)
def test_every_planted_bug_breaks_a_check_on_the_recipe(recipes, bug):
    z, y, f = recipes[5]
    r, choice = f["cv"]["r"][0], f["choice"][0]
    V, E = f["W"][0].shape
    if bug in ("tie_smaller", "argmax_by_index"):
        r2, grid2 = _tied_unsorted(r)
        good, bad = RR.select_rows(r2, grid2), RR.select_rows(r2, grid2, bug=bug)
        assert np.array_equal(good["rbest"], f["rbest"][0]) and np.all(good["choice"] < len(GRID))     # the larger lambda of a pair
        assert np.array_equal(bad["rbest"], good["rbest"]) and np.all(bad["choice"] == good["choice"] + len(GRID))
    elif bug in ("first_fold", "max_over_folds"):
        bad = RR.select_rows(r, GRID, bug=bug)
        moved = bad["choice"] != choice
        assert moved.any()
        # a target that moved lost more than 100 bars of held-out r: outside anything rounding explains
        lost = (f["rbest"][0] - bad["rbest"])[moved] / f["rmean_bar"][0].max()
        assert np.all(lost >= 100)
    elif bug == "excluded_wins":
        ok = [True] * len(GRID)
        ok[int(np.argmax(f["lambda_counts"][0]))] = False          # the most popular point is out; its values stay in the table
        good, bad = RR.select_rows(r, GRID, ok), RR.select_rows(r, GRID, ok, bug=bug)
        assert not np.any(good["choice"] == ok.index(False)) and np.any(bad["choice"] == ok.index(False))
    elif bug == "choice_shifted":
        bad = RR.solve_rows(CE.sum_except(f["cv"]["S"][0], -1), GRID, choice, bug=bug)
        sols = RR.solve_rows(CE.sum_except(f["cv"]["S"][0], -1), GRID, choice)["sols"]
        cond = max(RE.cond2(s["A"]) for s in sols.values())
        assert np.all(np.any(np.abs(bad["W"] - f["W"][0]) > RE.master_bar(f["W"][0], cond, E), 1))      # every row
        lam = f["lambda_rows"][0]
        assert RR.objective_rows(bad["W"], bad["b"], z, y, lam)[2] > RR.objective_rows(f["W"][0], f["b"][0], z, y, lam)[2]
    else:
        Wb = RE.rne_bf16(f["W"][0].astype(np.float32)).astype(np.float64)
        lam = f["lambda_rows"][0].astype(np.float32)
        if bug == "l2_mean_lambda":
            good, bad = RR.l2_rows(Wb, lam), RR.l2_rows(Wb, lam, bug=bug)
            assert abs(bad - good) > 100 * RR.l2_bar(V, E, good)
        else:
            g = np.random.default_rng(2).standard_normal((V, E))
            good, bad = RR.l2_rows_grad(Wb, lam, 2.0), RR.l2_rows_grad(Wb, lam, 2.0, bug=bug)
            rows = lam != lam[0]
            assert rows.any() and np.all(np.any(np.abs(bad - good)[rows] > 100 * RR.grad_bar(g, good)[rows], 1))


# ---------------------------------------------------------------------------------------------------- 4
def test_tie_unsorted_grid_and_excluded_points_on_hand_made_tables():
    #           target 0: a tie of points 1 and 2; target 1: point 3 leads; target 2: constant (rmean 0 everywhere)
    one = np.array([[0.5, 0.1, 0.0], [0.7, 0.2, 0.0], [0.7, 0.3, 0.0], [0.1, 0.9, 0.0]])
    r = np.stack([one, one])                                         # two folds
    s = RR.select_rows(r, [1e-3, 1e-2, 1e-1, 1.0])
    assert s["choice"].tolist() == [2, 3, 3] and s["choice"].dtype == np.int32
    assert s["rbest"].tolist() == [0.7, 0.9, 0.0] and np.array_equal(s["rmean"], one)
    # the grid in another order: the tie goes to the larger VALUE, the constant target to the largest lambda wherever it sits
    s = RR.select_rows(r, [1.0, 1e-1, 1e-2, 1e-3])
    assert s["choice"].tolist() == [1, 3, 0]
    s = RR.select_rows(r, [1e-2, 1e-3, 1.0, 1e-1])
    assert s["choice"].tolist() == [2, 3, 2]
    # an excluded point does not win: holding NaN, or holding values above every other
    for fill in (np.nan, 7.0):
        r2 = r.copy()
        r2[:, 2] = fill
        s = RR.select_rows(r2, [1e-3, 1e-2, 1e-1, 1.0], ok=[1, 1, 0, 1])
        assert s["choice"].tolist() == [1, 3, 3] and s["rbest"].tolist() == [0.7, 0.9, 0.0]
    s = RR.select_rows(r, [1e-3, 1e-2, 1e-1, 1.0], ok=[0, 0, 0, 0])
    assert s["choice"].tolist() == [-1, -1, -1] and np.isnan(s["rbest"]).all()
    # the mean is over the folds, in order
    r3 = np.stack([one, 3 * one, -one])
    assert np.array_equal(RR.select_rows(r3, [1e-3, 1e-2, 1e-1, 1.0])["rmean"], ((one + 3 * one) + -one) / 3.0)
    assert RR.margins(one, np.full_like(one, 1e-3)).tolist() == [0.0, pytest.approx(600.0), 0.0]


def test_l2_terms_of_the_emulator():
    rng = np.random.default_rng(0)
    W = RE.rne_bf16(rng.standard_normal((6, 16)).astype(np.float32)).astype(np.float64)
    lam = np.array([1e-4, 0.0, 1e-2, 1.0, 0.0, 3e-3], np.float32)
    assert RR.l2_rows(W, lam) == pytest.approx(float((lam.astype(np.float64) * (W * W).sum(1)).sum()), rel=1e-14)
    assert RR.l2_rows(W, np.full(6, 0.25, np.float32)) == pytest.approx(0.25 * float((W * W).sum()), rel=1e-14)
    g = RR.l2_rows_grad(W, lam, 2.0)
    assert np.array_equal(g[1], np.zeros(16)) and np.allclose(g[3], 2.0 * W[3], rtol=1e-15)
    # the gradient of the term: a central difference along a random direction
    d = rng.standard_normal(W.shape)
    num = (RR.l2_rows(W + 1e-6 * d, lam) - RR.l2_rows(W - 1e-6 * d, lam)) / 2e-6
    assert num == pytest.approx(float((g * d).sum()), rel=1e-6)


# ---------------------------------------------------------------------------------------------------- 5
def _cfg(**kw):
    from phantom_vlb_amd.litmodule import VLBLitModuleConfig
    base = dict(model_path="none", freeze_backbone=True, use_lora=False, lora_r=None, lora_alpha=None, lora_dropout=None,
                dropout_rate=0.1, num_target=128, l2_lambda=1e-3, lr=1e-3, betas=[0.9, 0.999], eps=1e-8,
                weight_decay=1e-2, lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=50000, geometry="mini")
    base.update(kw)
    return VLBLitModuleConfig(**base)


ON = dict(cache_features=True, ridge_fit="closed_form", ridge_lambda_grid=[1e-3, 1e-2])


def test_config_accepts_and_refuses():
    assert _cfg().ridge_lambda_per_target is False and _cfg(**ON).ridge_lambda_per_target is False
    assert _cfg(ridge_lambda_per_target=True, **ON).ridge_lambda_per_target is True
    with pytest.raises(ValueError, match=r"ridge_lambda_per_target.*ridge_lambda_grid"):
        _cfg(ridge_lambda_per_target=True)
    with pytest.raises(ValueError, match=r"ridge_lambda_per_target.*ridge_lambda_grid"):
        _cfg(ridge_lambda_per_target=True, cache_features=True, ridge_fit="closed_form")
    for bad in (1, 0, "true", None, 1.0):
        with pytest.raises(ValueError, match=r"ridge_lambda_per_target.*true or false"):
            _cfg(ridge_lambda_per_target=bad, **ON)


def test_yaml_plumbing_reaches_the_field():
    from phantom_vlb_amd.config import instantiate, load_config
    cdir = os.path.join(ROOT, "config")
    plain = load_config(cdir, ["experiment=VLB_mini_synthetic"])
    assert "ridge_lambda_per_target" not in plain["litmodule"]["config"]
    assert instantiate(plain["litmodule"]["config"]).ridge_lambda_per_target is False
    cfg = load_config(cdir, ["experiment=VLB_mini_synthetic", "litmodule.config.cache_features=true",
                             "litmodule.config.ridge_fit=closed_form", "litmodule.config.ridge_lambda_grid=[1e-4,1e-3,1e-2]",
                             "litmodule.config.ridge_lambda_per_target=true"])
    assert instantiate(cfg["litmodule"]["config"]).ridge_lambda_per_target is True
    for name in ("VLB_mini_synthetic", "VLB_vllama2_friends_baseline"):
        assert "ridge_lambda_per_target" in open(os.path.join(cdir, "experiment", name + ".yaml")).read()


def test_head_takes_refuses_and_clears_the_vector_on_the_host():
    from phantom_vlb_amd.head import BrainHead
    h = BrainHead(8, 4, 1e-3, 1e-5, "cpu", subjects=["a", "b"])
    assert h.l2_lambda_rows is None and h._lam() == 1e-3
    rows = torch.tensor([1e-3, 0.0, 1e-1, 1.0] * 2)
    h.set_l2_lambda_rows(rows)
    assert torch.equal(h.l2_lambda_rows, rows) and h.l2_lambda_rows is not rows and h._lam() == 0.0 and h.l2_lambda == 1e-3
    for bad in (rows[:4], rows.double(), rows.tolist(), -rows, rows * float("inf"), torch.full((8,), float("nan"))):
        with pytest.raises(ValueError, match="set_l2_lambda_rows"):
            h.set_l2_lambda_rows(bad)
    assert torch.equal(h.l2_lambda_rows, rows)           # a refused vector leaves the one in force
    h.set_l2_lambda_rows(None)
    assert h.l2_lambda_rows is None and h._lam() == 1e-3
    for loss in ("cosine", "pearson"):
        with pytest.raises(ValueError, match="mse"):
            BrainHead(8, 4, 1e-3, 1e-5, "cpu", loss=loss).set_l2_lambda_rows(rows[:4])
    # ridge_solve_rows' host checks precede any launch
    h = BrainHead(8, 4, 1e-3, 1e-5, "cpu")
    with pytest.raises(RuntimeError, match="ridge_stats_begin"):
        h.ridge_solve_rows(torch.zeros(1, 4, dtype=torch.int32), [1e-3, 1e-2])
    h.ridge_stats_begin()
    with pytest.raises(ValueError, match="choice int32"):
        h.ridge_solve_rows(torch.zeros(1, 4, dtype=torch.int64), [1e-3, 1e-2])
    with pytest.raises(ValueError, match="no clips"):
        h.ridge_solve_rows(torch.zeros(1, 4, dtype=torch.int32), [1e-3, 1e-2])
    h._ridge["n"][0] = 5
    with pytest.raises(ValueError, match=r"outside \[0, 2\)"):
        h.ridge_solve_rows(torch.tensor([[0, 1, 2, 0]], dtype=torch.int32), [1e-3, 1e-2])
    with pytest.raises(ValueError, match="positive"):
        h.ridge_solve_rows(torch.zeros(1, 4, dtype=torch.int32), [1e-3, 0.0])


def test_unset_option_adds_nothing_and_the_checkpoint_carries_the_vector(tmp_path):
    from phantom_vlb_amd.head import BrainHead
    from phantom_vlb_amd.litmodule import VLBLitModule
    m = VLBLitModule(_cfg(**ON))
    m.rng_state = lambda: {}
    ck = {}
    m._ridge_cv_lambda = 1e-2
    m.on_save_checkpoint(ck)
    assert "vlb_ridge_l2_lambda_rows" not in ck and ck["vlb_ridge_l2_lambda"] == 1e-2
    rows = torch.tensor([1e-3, 1e-2, 1e-2, 1e-3])
    m._ridge_lambda_rows = rows
    m.on_save_checkpoint(ck)
    assert torch.equal(ck["vlb_ridge_l2_lambda_rows"], rows) and ck["vlb_ridge_l2_lambda_rows"] is not rows
    torch.save(ck, tmp_path / "ck.pt")
    ck = torch.load(tmp_path / "ck.pt", weights_only=False)
    h = BrainHead(8, 4, 1e-3, 1e-5, "cpu")
    m2 = VLBLitModule(_cfg(ridge_lambda_per_target=True, **ON))
    m2.set_rng_state = lambda s: None
    m2.on_load_checkpoint(ck)                             # before the head exists: kept for configure_model
    assert torch.equal(m2._ridge_lambda_rows, rows) and m2._ridge_cv_lambda == 1e-2
    m2.head = h
    m2.on_load_checkpoint(ck)
    assert torch.equal(h.l2_lambda_rows.view(torch.int32), rows.view(torch.int32)) and h.l2_lambda == 1e-2 and h._lam() == 0.0


# ---------------------------------------------------------------------------------------------------- 5, the entries
def test_new_entries_are_declared_bound_and_exported():
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
    assert re.search(r"\bint64_t\s+vlb_head_l2_rows_ws_doubles\s*\(int R\)", text)
    assert re.search(r"vlb_head_l2_rows_ws_doubles \(src/utils\.py:59-73", raw)
    assert _lib.SIGNATURES["vlb_head_l2_rows_ws_doubles"] == [ctypes.c_int]
    assert _lib.lib.vlb_head_l2_rows_ws_doubles.restype is ctypes.c_int64 and "vlb_head_l2_rows_ws_doubles" in exported
    assert raw.index("visibility push") < raw.index("int vlb_head_l2_rows_bwd(") < raw.index("visibility pop")
    assert _lib.lib.vlb_abi_version() == 2 and "#define VLB_ABI_VERSION 2" in raw
    # vlb_ridge_solve keeps its signature
    assert len(_lib.SIGNATURES["vlb_ridge_solve"]) == 14


def test_entries_refuse_bad_arguments_without_a_device():
    from phantom_vlb_amd._lib import lib
    one = ctypes.c_void_p(16)
    assert lib.vlb_head_l2_rows_ws_doubles(1) == 1 and lib.vlb_head_l2_rows_ws_doubles(9) == 3 and lib.vlb_head_l2_rows_ws_doubles(0) == 0
    assert lib.vlb_head_l2_rows_ws_doubles(65536) == 2048 and lib.vlb_head_l2_rows_ws_doubles(1 << 30) == 2048
    assert lib.vlb_ridge_cv_select(one, one, one, one, one, None, 5, 7, 40, None) != 0
    assert lib.vlb_ridge_cv_select(one, one, None, one, one, one, 5, 7, 40, None) != 0
    assert lib.vlb_ridge_cv_select(one, one, one, one, one, one, 0, 7, 40, None) != 0 and b"K=0" in lib.vlb_last_error()
    assert lib.vlb_ridge_cv_select(one, one, one, one, one, one, 5, 0, 40, None) != 0 and b"L=0" in lib.vlb_last_error()
    assert lib.vlb_ridge_cv_select(one, one, one, one, one, one, 5, 7, 0, None) != 0 and b"V=0" in lib.vlb_last_error()
    ok = (one,) * 4 + (5, 1e-3) + (one,) * 5 + (8, 4)
    assert lib.vlb_ridge_solve_rows(*ok, None, 0, None) != 0
    assert lib.vlb_ridge_solve_rows(*ok, one, -1, None) != 0 and b"want=-1" in lib.vlb_last_error()
    assert lib.vlb_ridge_solve_rows(one, one, one, one, 0, 1e-3, one, one, one, one, one, 8, 4, one, 0, None) != 0 and b"N=0" in lib.vlb_last_error()
    assert lib.vlb_ridge_solve_rows(one, one, one, one, 5, -1.0, one, one, one, one, one, 8, 4, one, 0, None) != 0 and b"negative" in lib.vlb_last_error()
    assert lib.vlb_ridge_solve_rows(one, one, one, one, 5, 1e-3, one, one, one, one, None, 8, 4, one, 0, None) != 0
    assert lib.vlb_head_l2_rows_fwd(one, one, one, None, 4, 8, None) != 0 and lib.vlb_head_l2_rows_fwd(None, one, one, one, 4, 8, None) != 0
    assert lib.vlb_head_l2_rows_fwd(one, one, one, one, 0, 8, None) != 0 and b"R=0" in lib.vlb_last_error()
    assert lib.vlb_head_l2_rows_fwd(one, one, one, one, 4, 12, None) != 0 and b"E=12" in lib.vlb_last_error()
    assert lib.vlb_head_l2_rows_fwd(one, one, one, one, 4, 8200, None) != 0 and b"E=8200" in lib.vlb_last_error()
    assert lib.vlb_head_l2_rows_fwd(ctypes.c_void_p(24), one, one, one, 4, 8, None) != 0 and b"aligned" in lib.vlb_last_error()
    assert lib.vlb_head_l2_rows_bwd(one, one, None, 4, 8, 2.0, None) != 0 and lib.vlb_head_l2_rows_bwd(one, None, one, 4, 8, 2.0, None) != 0
    assert lib.vlb_head_l2_rows_bwd(one, one, one, 4, 0, 2.0, None) != 0 and b"E=0" in lib.vlb_last_error()
    assert lib.vlb_head_l2_rows_bwd(one, one, one, -1, 8, 2.0, None) != 0 and b"R=-1" in lib.vlb_last_error()
    assert lib.vlb_head_l2_rows_bwd(one, one, ctypes.c_void_p(20), 4, 8, 2.0, None) != 0 and b"aligned" in lib.vlb_last_error()
