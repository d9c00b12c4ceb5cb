"""CPU tier of the held-out scoring: the numpy restatement of the kernels against the definitions (a real
block bootstrap of the raw rows, np.corrcoef), the host rules of ``TargetScores`` (block of a clip, slab growth, draws,
Benjamini-Hochberg), the config / datamodule / CLI checks, and the C-ABI surface of the three new entries."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import score_emul as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- the moment bootstrap
def test_scores_match_their_definitions():
    c = E.make_case(seed=3, n_clips=23, V=9, block=4)
    out, avg = E.finish(c["sums"], c["n_j"])
    p, y = c["p"].astype(np.float64), c["y"].astype(np.float64)
    for v in range(9):
        assert abs(out[0, v] - np.corrcoef(p[:, v], y[:, v])[0, 1]) < 1e-10
        sse = ((p[:, v] - y[:, v]) ** 2).sum()
        assert abs(out[1, v] - (1 - sse / ((y[:, v] - y[:, v].mean()) ** 2).sum())) < 1e-10
        assert abs(out[2, v] - sse / 23) < 1e-10 and out[3, v] == 23
    assert np.allclose(avg, out[:3].mean(1), rtol=0, atol=1e-12)


def test_moment_bootstrap_equals_resampling_the_rows():
    """resampling the per-block sums is resampling the raw (p, y) rows block by block: r* agrees with np.corrcoef to 1e-10"""
    from phantom_vlb_amd.evaluate import bootstrap_draws
    c = E.make_case(seed=11, n_clips=30, V=6, block=4)          # 8 blocks, the last one short
    draws = bootstrap_draws(5, 0, c["nb"], 16)
    out, rs, _ = E.bootstrap(c["sums"], c["n_j"], draws)
    p, y = c["p"].astype(np.float64), c["y"].astype(np.float64)
    rows_of = [np.flatnonzero(c["slot"] == j) for j in range(c["nb"])]
    for rho in range(16):
        rows = np.concatenate([rows_of[j] for j in draws[rho]])
        for v in range(6):
            assert abs(rs[rho, v] - np.corrcoef(p[rows, v], y[rows, v])[0, 1]) < 1e-10
    assert np.allclose(out[0], rs.mean(0), rtol=0, atol=1e-12)
    assert np.allclose(out[1], rs.std(0, ddof=1), rtol=0, atol=1e-12)
    assert np.array_equal(out[2], (1 + (rs <= 0).sum(0)) / 17.0)


def test_degenerate_columns_and_one_block():
    c = E.make_case(seed=2, n_clips=12, V=8, block=4, const_y=(1,), const_p=(2,), masked=(5,))
    out, avg = E.finish(c["sums"], c["n_j"], c["keep"][0])
    assert out[0, 1] == 0 and out[1, 1] == 0                    # a constant target: vy = 0
    assert out[0, 2] == 0 and out[1, 2] < 0                     # a constant prediction: vp = 0, R^2 well defined
    assert np.isnan(out[:3, 5]).all() and out[3, 5] == 12       # masked
    kept = np.arange(8) != 5
    assert np.allclose(avg, out[:3, kept].mean(1), rtol=0, atol=1e-12)
    assert not c["sums"][:, :, 5].any() and not np.signbit(c["sums"][:, :, 5]).any()       # masked sums stay +0.0
    one = E.make_case(seed=2, n_clips=12, V=8, block=16)
    assert one["nb"] == 1
    b, rs, _ = E.bootstrap(one["sums"], one["n_j"], np.zeros((64, 1), np.int32))
    assert (b[1] == 0).all() and np.array_equal(b[0], rs[0])    # nothing to resample: sd exactly 0


def test_bars_are_small_and_positive_where_the_data_is_ordinary():
    c = E.make_case(seed=4, n_clips=40, V=16, block=4)
    bars = E.finish_bars(c["sums"], c["n_j"])
    assert (bars > 0).all() and (bars < 1e-12).all()


# ---------------------------------------------------------------------------------------------------- host rules
def test_bh_against_a_hand_worked_vector():
    from phantom_vlb_amd.evaluate import bh_q
    # sorted p: .01 .02 .03 .04 .20 ; m / rank: 5, 2.5, 5/3, 1.25, 1 -> .05 .05 .05 .05 .20 (running minimum from the right)
    q = bh_q(np.array([0.04, 0.01, 0.20, 0.03, 0.02]))
    assert np.allclose(q, [0.05, 0.05, 0.20, 0.05, 0.05], rtol=0, atol=1e-15)
    assert np.allclose(bh_q(np.array([0.9, 0.8])), [0.9, 0.9]) and bh_q(np.array([0.7, 1.0]))[1] == 1.0
    assert bh_q(np.array([])).size == 0


def test_block_rule_growth_and_draws():
    from phantom_vlb_amd.evaluate import bootstrap_draws, clip_blocks, grown_blocks
    counts = [0, 0, 0]
    got = clip_blocks(counts, [0, 2, 0, 0, 2, 0], 2)            # rank in the head's clips // block
    assert got == [(0, 0), (2, 0), (0, 0), (0, 1), (2, 0), (0, 1)] and counts == [4, 0, 2]
    assert clip_blocks(counts, [0, 1], 2) == [(0, 2), (1, 0)]
    assert [grown_blocks(4, n) for n in (1, 4, 5, 8, 9, 33)] == [4, 4, 8, 8, 16, 64]
    d = bootstrap_draws(7, 2, 5, 9)
    assert d.dtype == np.int32 and d.shape == (9, 5) and d.min() >= 0 and d.max() < 5
    assert np.array_equal(d, np.random.RandomState(7 + 1009 * 2).randint(0, 5, size=(9, 5)))
    assert np.array_equal(d, bootstrap_draws(7, 2, 5, 9)) and not np.array_equal(d, bootstrap_draws(7, 1, 5, 9))


# ---------------------------------------------------------------------------------------------------- config, datamodule, CLI
def _lit(**kw):
    from phantom_vlb_amd.litmodule import VLBLitModuleConfig
    base = dict(model_path="none", freeze_backbone=True, use_lora=False, lora_r=None, lora_alpha=None, lora_dropout=None,
                dropout_rate=0.0, num_target=128, l2_lambda=1e-3, lr=1e-4, betas=[0.9, 0.999], eps=1e-8, weight_decay=1e-2,
                lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=50000, geometry="mini")
    return VLBLitModuleConfig(**{**base, **kw})


def test_config_validation_messages():
    c = _lit()
    assert (c.score_block, c.score_bootstrap, c.score_bootstrap_seed, c.score_save_predictions) == (128, 0, 0, False)
    assert _lit(score_bootstrap=2, score_block=1, score_bootstrap_seed=9, score_save_predictions=True).score_bootstrap == 2
    for kw, msg in ((dict(score_block=0), "score_block=0"), (dict(score_block=True), "score_block=True"),
                    (dict(score_block=2.0), "score_block=2.0"), (dict(score_bootstrap=1), "score_bootstrap=1"),
                    (dict(score_bootstrap=-3), "score_bootstrap=-3"), (dict(score_bootstrap_seed=-1), "score_bootstrap_seed=-1"),
                    (dict(score_save_predictions=1), "score_save_predictions=1")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            _lit(**kw)


def _dm(**kw):
    from phantom_vlb_amd.datamodule import VLBDataModuleConfig, VLBDatasets
    base = dict(lazyload_path="synthetic:3x2", subject="sub-01", seasons=["s1"], delay=3, window=3, random_state=10,
                shuffle_val_data=False, batch_size=2, geometry="mini", num_target=16)
    return VLBDatasets(VLBDataModuleConfig(**{**base, **kw}))


def test_synthetic_test_split_seeds():
    assert _dm().test is None
    d = _dm(test_lazyload_path="synthetic:2x3")
    assert d.test.ds_paths == [(10 + 5003, 3), (10 + 5004, 3)] and len(d.test) == 6 and d.test.subject_of is None
    assert d.test_names == {"test_set": ["synthetic_test_0", "synthetic_test_1"]}
    assert len(d.train) == 4 and len(d.val) == 2                                 # the other splits are as they were
    m = _dm(test_lazyload_path="synthetic:2x3", subjects=["a", "b"])
    assert m.test.ds_paths == [(5013, 3), (5014, 3), (5013 + 1009, 3), (5014 + 1009, 3)] and m.test.subject_of == [0, 0, 1, 1]


def _npz(path):
    np.savez(path, dset_len=np.array([1]))
    return str(path)


def test_globbed_test_split_and_overlap(tmp_path):
    from phantom_vlb_amd.datamodule import VLBDataModule, VLBDataModuleConfig
    for sub in ("a", "b"):
        for name in ("s1_x", "s1_y", "s2_x", "s3_x", "s3_y"):
            _npz(tmp_path / f"{sub}_{name}.npz")
    pat = str(tmp_path / "{subject}_s*_*.npz")
    kw = dict(lazyload_path=pat, seasons=["s1", "s2"], subjects=["a", "b"])
    with pytest.raises(ValueError, match="test_seasons"):
        _dm(**kw, test_lazyload_path=pat)
    d = _dm(**kw, test_lazyload_path=pat, test_seasons=["s3"])
    assert [os.path.basename(p) for p in d.test.ds_paths] == ["a_s3_x.npz", "a_s3_y.npz", "b_s3_x.npz", "b_s3_y.npz"]
    assert d.test.subject_of == [0, 0, 1, 1] and d.test_names["b"] == {"test_set": ["b_s3_x.npz", "b_s3_y.npz"]}
    with pytest.raises(ValueError, match="also belong to the train or validation split"):
        _dm(**kw, test_lazyload_path=pat, test_seasons=["s3", "s2"])
    with pytest.raises(FileNotFoundError, match="test_lazyload_path"):
        _dm(**kw, test_lazyload_path=pat, test_seasons=["s9"])
    with pytest.raises(ValueError, match="{subject}"):
        _dm(**kw, test_lazyload_path=str(tmp_path / "a_s*_*.npz"), test_seasons=["s3"])
    one = _dm(lazyload_path=str(tmp_path / "a_s*_*.npz"), seasons=["s1"], test_lazyload_path=str(tmp_path / "a_s*_x.npz"),
              test_seasons=["s2"])
    assert [os.path.basename(p) for p in one.test.ds_paths] == ["a_s2_x.npz"]
    dm = VLBDataModule(VLBDataModuleConfig(lazyload_path="synthetic:3x2", subject="s", seasons=["s1"], delay=3, window=3,
                                           random_state=1, shuffle_val_data=False, geometry="mini", num_target=16))
    with pytest.raises(ValueError, match="test_lazyload_path"):
        dm.test_dataloader()


def test_cli_keys():
    sys.path.insert(0, ROOT)
    import train
    from phantom_vlb_amd.config import load_config
    def cfg(*ov):
        return load_config(os.path.join(ROOT, "config"), ["experiment=VLB_mini_synthetic", "subject=sub-01", *ov])
    assert train.check_evaluate_keys(cfg()) == (None, True, None)
    assert train.check_evaluate_keys(cfg("evaluate=test", "fit=false", "ckpt_path=x.ckpt")) == ("test", False, "x.ckpt")
    assert train.check_evaluate_keys(cfg("evaluate=val", "ckpt_path=x.ckpt")) == ("val", True, "x.ckpt")
    for ov, msg in ((["evaluate=test", "fit=false"], "needs ckpt_path"), (["evaluate=train"], "evaluate='train'"),
                    (["fit=false", "ckpt_path=x.ckpt"], "nothing to do"), (["evaluate_out=a.npz"], "needs evaluate"),
                    (["evaluate=test", "datamodule.config.test_lazyload_path=null"], "test_lazyload_path")):
        with pytest.raises(ValueError, match=msg):
            train.check_evaluate_keys(cfg(*ov))
    for name in ("VLB_mini_synthetic", "VLB_mini_synthetic_multisubject"):          # the quick start runs without data
        c = load_config(os.path.join(ROOT, "config"), [f"experiment={name}", "subject=sub-01"])
        assert c["datamodule"]["config"]["test_lazyload_path"].startswith("synthetic:")


def test_trainer_test_is_single_process(monkeypatch):
    from phantom_vlb_amd.trainer import Trainer
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.warns(UserWarning):
        t = Trainer()
    with pytest.raises(ValueError, match="single-process only"):
        t.test(object())


# ---------------------------------------------------------------------------------------------------- C-ABI surface
NEW_ENTRIES = {"vlb_score_accumulate": 12, "vlb_score_finish": 8, "vlb_score_bootstrap": 9}
DECLS = {
    "vlb_score_accumulate": "const float* pred, int ldp, const float* y, int ldy, const int* slot, const float* keep, double* sums, "
                            "int B, int V, int nb, int n_slots, void* stream",
    "vlb_score_finish": "const double* sums_h, const double* n_j, int nb, const float* keep_h, double* out, double* avg, int V, "
                        "void* stream",
    "vlb_score_bootstrap": "const double* sums_h, const double* n_j, int nb, const int* draws, int R, const float* keep_h, "
                           "double* out, int V, void* stream",
}


def test_new_entries_are_declared_bound_and_exported():
    from phantom_vlb_amd import _lib
    raw = open(os.path.join(ROOT, "include", "vlb.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()[-2] == "T"}
    want = {ctypes.c_void_p: "P", ctypes.c_int: "I"}
    for name, n in NEW_ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
        assert m, f"{name} is not declared in include/vlb.h"
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        assert params == DECLS[name].split(", "), name
        assert len(params) == len(_lib.SIGNATURES[name]) == n, name
        assert ["P" if "*" in p else "I" for p in params] == [want[t] for t in _lib.SIGNATURES[name]], name
        assert name in exported and getattr(_lib.lib, name).restype is ctypes.c_int
        assert re.search(name + r" \(src/utils\.py:85-110", raw), f"{name} does not cite the reference's callback"
        assert raw.index("visibility push") < raw.index(f"int {name}(") < raw.index("visibility pop")
    assert _lib.lib.vlb_abi_version() == 2 and "#define VLB_ABI_VERSION 2" in raw
    mk = open(os.path.join(ROOT, "phantom_vlb_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bscore\.hip\b", mk, flags=re.M)


def test_entries_refuse_bad_arguments_without_a_device():
    """every refusal comes back as VLB_ERR_INVALID with a message, before any launch (no device here)"""
    from phantom_vlb_amd._lib import lib
    one = ctypes.c_void_p(16)
    acc, fin, boot = lib.vlb_score_accumulate, lib.vlb_score_finish, lib.vlb_score_bootstrap
    for args, msg in (((None, 4, one, 4, one, None, one, 1, 4, 1, 1, None), b"null"), ((one, 4, None, 4, one, None, one, 1, 4, 1, 1, None), b"null"),
                      ((one, 4, one, 4, None, None, one, 1, 4, 1, 1, None), b"null"), ((one, 4, one, 4, one, None, None, 1, 4, 1, 1, None), b"null"),
                      ((one, 4, one, 4, one, None, one, 0, 4, 1, 1, None), b"B=0"), ((one, 4, one, 4, one, None, one, 1, 0, 1, 1, None), b"V=0"),
                      ((one, 3, one, 4, one, None, one, 1, 4, 1, 1, None), b"ldp=3"), ((one, 4, one, 3, one, None, one, 1, 4, 1, 1, None), b"ldy=3"),
                      ((one, 4, one, 4, one, None, one, 1, 4, 0, 4, None), b"nb=0"), ((one, 4, one, 4, one, None, one, 1, 4, 3, 4, None), b"n_slots=4"),
                      ((one, 4, one, 4, one, None, one, 1, 4, 2, 0, None), b"n_slots=0")):
        assert acc(*args) == -1 and msg in lib.vlb_last_error(), (args, lib.vlb_last_error())
    for args, msg in (((None, one, 1, None, one, one, 4, None), b"null"), ((one, None, 1, None, one, one, 4, None), b"null"),
                      ((one, one, 1, None, None, one, 4, None), b"null"), ((one, one, 1, None, one, None, 4, None), b"null"),
                      ((one, one, 0, None, one, one, 4, None), b"nb=0"), ((one, one, 1, None, one, one, 0, None), b"V=0")):
        assert fin(*args) == -1 and msg in lib.vlb_last_error(), (args, lib.vlb_last_error())
    for args, msg in (((None, one, 1, one, 2, None, one, 4, None), b"null"), ((one, None, 1, one, 2, None, one, 4, None), b"null"),
                      ((one, one, 1, None, 2, None, one, 4, None), b"null"), ((one, one, 1, one, 2, None, None, 4, None), b"null"),
                      ((one, one, 0, one, 2, None, one, 4, None), b"nb=0"), ((one, one, 1, one, 2, None, one, 0, None), b"V=0"),
                      ((one, one, 1, one, 1, None, one, 4, None), b"R=1"), ((one, one, 1, one, 0, None, one, 4, None), b"R=0")):
        assert boot(*args) == -1 and msg in lib.vlb_last_error(), (args, lib.vlb_last_error())
