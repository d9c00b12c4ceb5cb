"""The closed-form ridge fit, host side: the fp64 emulator (tests/ridge_emul.py) proved against the objective itself, its bars
checked with planted bugs, the config refusals, the new ABI entries, and that ``ridge_fit=None`` adds nothing.  No GPU.

Bars used here (derivations in ridge_emul's docstring):
* gradient at the solution: eliminating b, dJ/dW = 2/(N V) (W A - R) with A, R the centred system, so the solve's residual bar
  (gamma_{3E+1} |X| |L||L|^T, Higham Thm 10.4) times 2/(N V) bounds it - independent of the conditioning - plus the fp64
  rounding of evaluating the gradient itself: (N + E + 8) 2^-53 times the sum of the magnitudes of its terms (one dot product
  over E, one over N, a handful of scalar operations).  dJ/db is that evaluation rounding alone, plus the rounding of forming
  b = ybar - W zbar: (E + 4) 2^-53 (|ybar| + |W| |zbar|), which enters every residual.
* lstsq against Cholesky: two backward-stable solvers of the same problem; each forward error is at most
  cond_2(A) * gamma_{3E+1} * || |L||L|^T ||_F / ||A||_2 relative (Thm 10.4 and first-order perturbation theory; lstsq works on
  the augmented matrix of condition sqrt(cond_2(A)) and is no worse): the sum of the two, i.e. twice that.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ridge_emul as RE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_ENTRIES = {"vlb_head_features_cached": 17, "vlb_ridge_gram_accumulate": 11, "vlb_chol_f64": 5, "vlb_chol_solve_f64": 8,
               "vlb_ridge_solve": 14}
LAM = 1e-3


def _bf16(x):
    return torch.from_numpy(np.asarray(x, np.float32)).to(torch.bfloat16).float().numpy().astype(np.float64)


def _data(N=75, E=24, V=7, seed=0, integers=False):
    """features with non-zero column means and unequal scales (so centring and the penalty's scale matter), bf16 / fp32 valued"""
    rng = np.random.default_rng(seed)
    if integers:
        return rng.integers(-3, 4, (N, E)).astype(np.float64), rng.integers(-4, 5, (N, V)).astype(np.float64)
    z = _bf16(rng.standard_normal((N, E)) * rng.uniform(0.3, 2.0, E) + rng.uniform(-1.5, 1.5, E))
    Wt = rng.standard_normal((V, E)) / np.sqrt(E)
    y = (z @ Wt.T + rng.uniform(-2, 2, V) + 0.5 * rng.standard_normal((N, V))).astype(np.float32).astype(np.float64)
    return z, y


@pytest.mark.parametrize("N,E,V", [(75, 24, 7), (20, 32, 3), (513, 16, 1)])
def test_gradient_of_the_objective_vanishes_at_the_solution(N, E, V):
    z, y = _data(N, E, V, seed=N)
    sol = RE.solve(RE.sums(z, y, chunk=32), LAM)
    W, b = sol["W"], sol["b"]
    dW, db, mag_W, mag_b = RE.gradient(W, b, z, y, LAM)
    ev = (N + E + 8) * RE.U64
    zbar, ybar = z.mean(0), y.mean(0)
    b_err = (E + 4) * RE.U64 * (np.abs(ybar) + np.abs(W) @ np.abs(zbar))            # [V]: b as formed, against ybar - W zbar
    bar_W = 2.0 / (N * V) * (RE.solve_bar(sol["L"], W) + np.outer(b_err, np.abs(z).sum(0))) + ev * mag_W
    bar_b = ev * mag_b + 2.0 / V * b_err
    # dJ/db = 2/(N V) sum_n (W z_n + b - y_n) = 2/V (W zbar + b - ybar): zero by the definition of b
    print(f"N={N} E={E} V={V}: max |dW|/bar {np.max(np.abs(dW) / bar_W):.3f}, max |db|/bar {np.max(np.abs(db) / bar_b):.3f}, "
          f"max|dW| {np.abs(dW).max():.2e} of terms {mag_W.max():.2e}")
    assert np.all(np.abs(dW) <= bar_W) and np.all(np.abs(db) <= bar_b)
    # and it IS a minimum of a strictly convex function: every perturbation raises J
    J0 = RE.objective(W, b, z, y, LAM)[2]
    rng = np.random.default_rng(1)
    for _ in range(5):
        dWp, dbp = 1e-3 * rng.standard_normal(W.shape), 1e-3 * rng.standard_normal(b.shape)
        assert RE.objective(W + dWp, b + dbp, z, y, LAM)[2] > J0


@pytest.mark.parametrize("N,E,V", [(75, 24, 7), (20, 32, 3)])
def test_solution_equals_lstsq_on_the_augmented_system(N, E, V):
    z, y = _data(N, E, V, seed=3 * N)
    sol = RE.solve(RE.sums(z, y, chunk=64), LAM)
    W2, b2 = RE.lstsq_solution(z, y, LAM)
    Lm = np.abs(sol["L"])
    rel = 2 * RE.cond2(sol["A"]) * RE.gamma(3 * E + 1) * np.linalg.norm(Lm @ Lm.T) / np.linalg.norm(sol["A"], 2)
    for v in range(V):
        err = np.linalg.norm(sol["W"][v] - W2[v]) / np.linalg.norm(W2[v])
        assert err <= rel, (v, err, rel)
    # b = ybar - W zbar: the weights' difference carried through zbar, plus forming it
    bar_b = rel * np.linalg.norm(W2, axis=1) * np.linalg.norm(z.mean(0)) + (E + 4) * RE.U64 * (np.abs(y.mean(0)) + np.abs(W2) @ np.abs(z.mean(0)))
    assert np.all(np.abs(sol["b"] - b2) <= bar_b)


def test_chunking_does_not_change_integer_sums_and_gaussian_sums_stay_within_the_bar():
    z, y = _data(513, 16, 5, integers=True)
    one = RE.sums(z, y, chunk=513)
    for chunk in (512, 200, 1):
        s = RE.sums(z, y, chunk=chunk)
        assert all(np.array_equal(s[k], one[k]) for k in ("G", "C", "sz", "sy")) and s["n"] == 513
    z, y = _data(513, 16, 5, seed=9)
    one, s = RE.sums(z, y, chunk=513), RE.sums(z, y, chunk=200)
    assert np.all(np.abs(s["G"] - one["G"]) <= RE.gram_bar(z, z)) and np.all(np.abs(s["C"] - one["C"]) <= RE.gram_bar(y, z))


@pytest.mark.parametrize("bug", RE.BUGS)
def test_every_planted_bug_breaks_a_bar(bug):
    """The bars the GPU tests assert - exact integer sums, the Gaussian-sum bar, the masters within one fp32 ulp (+ floor) of
    the emulator's solution - each reject the mistake they are there for."""
    N, E, V, chunk = 75, 24, 7, 32                      # 32 + 32 + 11: a partial last chunk; V != E, V > 1
    zi, yi = _data(N, E, V, integers=True)
    z, y = _data(N, E, V, seed=5)
    clean_i, clean = RE.sums(zi, yi, chunk), RE.sums(z, y, chunk)
    ref = RE.solve(clean, LAM)
    floor_cond = RE.cond2(ref["A"])
    broken = []
    if bug in ("c_transposed", "chunk_twice", "drop_last_chunk"):
        bad_i, bad = RE.sums(zi, yi, chunk, bug=bug), RE.sums(z, y, chunk, bug=bug)
        broken.append(not all(np.array_equal(bad_i[k], clean_i[k]) for k in ("G", "C", "sz", "sy")))
        over = [np.any(np.abs(bad["G"] - clean["G"]) > RE.gram_bar(z, z)), np.any(np.abs(bad["C"] - clean["C"]) > RE.gram_bar(y, z))]
        broken.append(any(over))
        got = RE.solve(bad, LAM)
    else:
        got = RE.solve(clean, LAM, bug=bug)
    broken.append(bool(np.any(np.abs(got["W"] - ref["W"]) > RE.master_bar(ref["W"], floor_cond, E))))
    print(bug, broken, f"max |dW| {np.abs(got['W'] - ref['W']).max():.2e}, max |db| {np.abs(got['b'] - ref['b']).max():.2e}")
    assert all(broken), (bug, broken)
    # ... and each raises the objective it claims to minimise
    assert RE.objective(got["W"], got["b"], z, y, LAM)[2] > RE.objective(ref["W"], ref["b"], z, y, LAM)[2]


def test_rne_bf16_matches_torch():
    x = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    x[:4] = [1.00390625, 1.01171875, -1.00390625, 0.0]              # ties: to even
    assert np.array_equal(RE.rne_bf16(x), torch.from_numpy(x).to(torch.bfloat16).float().numpy())


# ---------------------------------------------------------------------------------------------------- config
def _cfg(**kw):
    from phantom_vlb_amd.litmodule import VLBLitModuleConfig
    base = dict(model_path="none", freeze_backbone=True, use_lora=False, lora_r=None, lora_alpha=None, lora_dropout=None,
                dropout_rate=0.1, num_target=128, l2_lambda=1e-3, lr=1e-3, betas=[0.9, 0.999], eps=1e-8,
                weight_decay=1e-2, lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=50000, geometry="mini")
    base.update(kw)
    return VLBLitModuleConfig(**base)


def test_config_accepts_and_refuses():
    assert _cfg().ridge_fit is None
    assert _cfg(cache_features=True, ridge_fit="closed_form").ridge_fit == "closed_form"
    with pytest.raises(ValueError, match=r"ridge_fit='exact'.*closed_form"):
        _cfg(cache_features=True, ridge_fit="exact")
    with pytest.raises(ValueError, match=r"ridge_fit.*cache_features=True"):
        _cfg(ridge_fit="closed_form")
    with pytest.raises(ValueError, match=r"ridge_fit.*loss='mse'"):
        _cfg(cache_features=True, ridge_fit="closed_form", loss="pearson")
    for lam in (0.0, -1e-3):
        with pytest.raises(ValueError, match=r"ridge_fit.*l2_lambda > 0"):
            _cfg(cache_features=True, ridge_fit="closed_form", l2_lambda=lam)
    with pytest.raises(ValueError, match="frozen backbone"):            # what cache_features refuses stays refused
        _cfg(cache_features=True, ridge_fit="closed_form", freeze_backbone=False, use_lora=True, lora_r=16, lora_alpha=32,
             lora_dropout=0.1)


def test_yaml_plumbing_reaches_the_field():
    from phantom_vlb_amd.config import instantiate, load_config
    cdir = os.path.join(ROOT, "config")
    plain = load_config(cdir, ["experiment=VLB_mini_synthetic"])
    assert "ridge_fit" not in plain["litmodule"]["config"] and instantiate(plain["litmodule"]["config"]).ridge_fit is None
    cfg = load_config(cdir, ["experiment=VLB_mini_synthetic", "litmodule.config.cache_features=true",
                             "litmodule.config.ridge_fit=closed_form"])
    assert instantiate(cfg["litmodule"]["config"]).ridge_fit == "closed_form"
    for name in ("VLB_mini_synthetic", "VLB_vllama2_friends_baseline"):
        assert "ridge_fit" in open(os.path.join(cdir, "experiment", name + ".yaml")).read()


def test_unset_option_allocates_nothing_and_the_fingerprint_ignores_it(tmp_path):
    from phantom_vlb_amd import feature_cache as FC
    from phantom_vlb_amd.datamodule import VLB_Dataset
    from phantom_vlb_amd.head import BrainHead
    from phantom_vlb_amd.litmodule import VLBLitModule
    h = BrainHead(8, 4, 1e-3, 1e-5, "cpu")
    assert getattr(h, "_ridge", None) is None and tuple(h.master) == h.param_names
    m = VLBLitModule(_cfg(cache_features=True))
    m._maybe_fit_ridge()                                   # unset: returns before it looks at anything
    assert "_ridge_fit_done" not in m.__dict__ and "_ridge_fit_dataset" not in m.__dict__ and not m.feature_caches
    # a cache persisted by a run without the option serves a run with it, and the other way round
    lib = tmp_path / "libvlb.so"
    lib.write_bytes(b"bytes to hash")
    ds = VLB_Dataset([(1, 4)], "mini", 128)
    assert FC.fingerprint(_cfg(cache_features=True), ds, lib_path=str(lib)) == \
        FC.fingerprint(_cfg(cache_features=True, ridge_fit="closed_form"), ds, lib_path=str(lib))


def test_head_refuses_on_the_host_and_leaves_the_parameters_alone():
    from phantom_vlb_amd.head import BrainHead
    h = BrainHead(8, 4, 1e-3, 1e-5, "cpu", subjects=["a", "b"])
    before = {n: t.clone() for n, t in h.master.items()}
    with pytest.raises(RuntimeError, match="ridge_stats_begin"):
        h.ridge_solve()
    h.ridge_stats_begin()
    assert tuple(h._ridge["G"].shape) == (2, 8, 8) and h._ridge["G"].dtype == torch.float64 and tuple(h._ridge["C"].shape) == (2, 4, 8)
    h._ridge["n"] = [5, 0]
    with pytest.raises(ValueError, match=r"head 1 \('b'\) has no clips"):
        h.ridge_solve()
    h._ridge["n"] = [9, 8]
    with pytest.raises(ValueError, match=r"head 1 \('b'\) has N = 8 <= E = 8.*l2_lambda > 0"):
        h.ridge_solve(l2_lambda=0.0)
    with pytest.raises(ValueError, match="negative"):
        h.ridge_solve(l2_lambda=-1.0)
    assert all(torch.equal(h.master[n], t) for n, t in before.items())
    h.ridge_stats_end()
    assert h._ridge is None
    with pytest.raises(ValueError, match="loss='cosine'"):
        BrainHead(8, 4, 1e-3, 1e-5, "cpu", loss="cosine").ridge_stats_begin()


# ---------------------------------------------------------------------------------------------------- ABI
def test_new_entries_are_declared_bound_and_exported():
    """header == SIGNATURES == nm -D for every new entry (parameter kinds in the same positions), each citing the reference's
    RidgeRegressionLayer; ABI version still 2."""
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
        assert re.search(name + r" \(src/utils\.py:59-73", raw), f"{name} does not cite the reference's layer"
    assert raw.index("visibility push") < raw.index("int vlb_ridge_solve(") < raw.index("visibility pop")
    assert _lib.lib.vlb_abi_version() == 2 and "#define VLB_ABI_VERSION 2" in raw
    assert "ridge_solve.hip" in open(os.path.join(ROOT, "phantom_vlb_amd", "csrc", "Makefile")).read()


def test_entries_refuse_bad_arguments_without_a_device():
    from phantom_vlb_amd._lib import lib
    one = ctypes.c_void_p(16)
    assert lib.vlb_ridge_gram_accumulate(one, one, 4, one, one, one, None, 1, 8, 4, None) != 0
    assert lib.vlb_ridge_gram_accumulate(one, one, 4, one, one, one, one, 0, 8, 4, None) != 0 and b"n=0" in lib.vlb_last_error()
    assert lib.vlb_ridge_gram_accumulate(one, one, 3, one, one, one, one, 1, 8, 4, None) != 0 and b"ldy=3" in lib.vlb_last_error()
    assert lib.vlb_chol_f64(one, 0, 4, one, None) != 0 and lib.vlb_chol_f64(one, 5, 4, one, None) != 0
    assert lib.vlb_chol_f64(one, 4, 4, None, None) != 0
    assert lib.vlb_chol_solve_f64(one, 4, one, 4, 0, 4, one, None) != 0 and lib.vlb_chol_solve_f64(one, 3, one, 4, 1, 4, one, None) != 0
    assert lib.vlb_ridge_solve(one, one, one, one, 0, 1e-3, one, one, one, one, one, 8, 4, None) != 0 and b"N=0" in lib.vlb_last_error()
    assert lib.vlb_ridge_solve(one, one, one, one, 5, -1.0, one, one, one, one, one, 8, 4, None) != 0 and b"negative" in lib.vlb_last_error()
    assert lib.vlb_ridge_solve(one, one, one, one, 5, 1e-3, one, one, one, one, None, 8, 4, None) != 0
    assert lib.vlb_head_features_cached(one, one, one, one, one, one, one, one, one, one, one, one, 1, 12, 4, 1e-5, None) != 0
    assert lib.vlb_head_features_cached(one, one, None, one, one, one, one, one, one, one, one, one, 1, 8, 4, 1e-5, None) != 0
