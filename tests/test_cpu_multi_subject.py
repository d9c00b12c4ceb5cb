"""Per-subject ridge heads on one trunk (``subjects``), host side: config validation, the synthetic multi-subject datamodule,
the per-subject validation callback, the three new ABI entries, and tests/group_emul.py itself (it is the grouped head in
fp64, its bars accept an honest fp32 computation and reject every planted bug, its planner restatement matches head.hip).
No GPU."""
import ctypes
import os
import pathlib
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import group_emul as GE
import head_emul as H
import head_loss_emul as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"vlb_head_grouped_ws_floats": 4, "vlb_head_fwd_grouped": 31, "vlb_head_bwd_grouped": 32}
W_, B_ = "ridge_layer.linear.weight", "ridge_layer.linear.bias"


def _cfg(**kw):
    from phantom_vlb_amd.litmodule import VLBLitModuleConfig
    base = dict(model_path="none", freeze_backbone=True, use_lora=False, lora_r=None, lora_alpha=None, lora_dropout=None,
                dropout_rate=0.0, num_target=128, l2_lambda=1e-3, lr=1e-3, betas=[0.9, 0.999], eps=1e-8,
                weight_decay=1e-2, lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=50000, geometry="mini")
    base.update(kw)
    return VLBLitModuleConfig(**base)


def _dm_cfg(**kw):
    from phantom_vlb_amd.datamodule import VLBDataModuleConfig
    base = dict(subject="sub-01", lazyload_path="synthetic:3x4", seasons=["s1"], delay=3, window=3, random_state=3, batch_size=2,
                num_workers=0, shuffle_val_data=False, geometry="mini", num_target=128)
    base.update(kw)
    return VLBDataModuleConfig(**base)


# ---------------------------------------------------------------------------------------------------- config validation
@pytest.mark.parametrize("bad", [[], ["sub-01"], "sub-01", ["sub-01", "sub-01"]])
def test_subjects_needs_two_distinct_names(bad):
    from phantom_vlb_amd.head import BrainHead
    with pytest.raises(ValueError, match="subject"):
        _cfg(subjects=bad)
    with pytest.raises(ValueError, match="subject"):
        _dm_cfg(subjects=bad, lazyload_path="synthetic:3x4")
    with pytest.raises(ValueError, match="subject"):
        BrainHead(64, 8, 1e-3, 1e-5, "cpu", subjects=bad)
    assert _cfg().subjects is None and _dm_cfg().subjects is None
    assert list(_cfg(subjects=["a", "b"]).subjects) == ["a", "b"]


def test_lazyload_path_needs_the_subject_placeholder(tmp_path):
    with pytest.raises(ValueError, match=r"\{subject\}"):
        _dm_cfg(subjects=["sub-01", "sub-02"], lazyload_path=str(tmp_path / "friends_sub-01"))
    _dm_cfg(subjects=["sub-01", "sub-02"], lazyload_path=str(tmp_path / "friends_{subject}"))
    _dm_cfg(subjects=["sub-01", "sub-02"], lazyload_path="synthetic:2x2")


def test_module_and_datamodule_must_agree():
    """a batch with "subject" reaching a module without ``subjects``, or the reverse: a ValueError naming both config keys"""
    from phantom_vlb_amd.litmodule import check_batch_subjects
    two = ("sub-01", "sub-02")
    assert check_batch_subjects({"y": 0}, None) is None
    assert check_batch_subjects({"y": 0, "subject": torch.tensor([1, 0])}, two, 2).tolist() == [1, 0]
    for batch, subjects in (({"subject": torch.tensor([0, 1])}, None), ({"y": 0}, two)):
        with pytest.raises(ValueError, match=r"litmodule\.config\.subjects.*datamodule\.config\.subjects"):
            check_batch_subjects(batch, subjects, 2)


@pytest.mark.parametrize("bad", [[0, 2], [-1, 0], [0], [0.5, 1.0]])
def test_out_of_range_subject_in_a_batch(bad):
    from phantom_vlb_amd.litmodule import check_batch_subjects
    with pytest.raises(ValueError, match="subject"):
        check_batch_subjects({"subject": torch.tensor(bad)}, ("sub-01", "sub-02"), 2)


def test_head_state_shapes_and_single_subject_init_unchanged():
    """head g = 0 of a stacked head is the single head of the same seed; tensors handed in must have the stacked shape"""
    from phantom_vlb_amd.head import BrainHead
    one = BrainHead(64, 8, 1e-3, 1e-5, "cpu", seed=11)
    two = BrainHead(64, 8, 1e-3, 1e-5, "cpu", seed=11, subjects=["a", "b"])
    assert tuple(two.master[W_].shape) == (2, 8, 64) and tuple(two.master[B_].shape) == (2, 8)
    assert torch.equal(two.master[W_][0], one.master[W_]) and torch.equal(two.master[B_][0], one.master[B_])
    assert not torch.equal(two.master[W_][1], one.master[W_])
    assert torch.equal(two.master[W_].to(torch.bfloat16).float(), two.master[W_])          # bf16-valued, as ever
    sd = two.subject_state_dict("b")
    assert set(sd) == set(one.master) and torch.equal(sd[W_], two.master[W_][1]) and sd["layer_norm1.weight"].shape == (64,)
    with pytest.raises(ValueError, match="subjects"):
        BrainHead(64, 8, 1e-3, 1e-5, "cpu", sd=dict(one.master), subjects=["a", "b"])
    with pytest.raises(ValueError, match="subject"):
        two.subject_state_dict("c")


def test_feature_cache_fingerprint_includes_subjects():
    from phantom_vlb_amd.datamodule import VLBDataModule
    from phantom_vlb_amd.feature_cache import fingerprint
    train = VLBDataModule(_dm_cfg(subjects=["sub-01", "sub-02"], lazyload_path="synthetic:2x2")).datasets.train
    a = fingerprint(_cfg(subjects=["sub-01", "sub-02"]), train)
    b = fingerprint(_cfg(subjects=["sub-02", "sub-01"]), train)
    c = fingerprint(_cfg(), train)
    assert len({a, b, c}) == 3


def test_yaml_experiments_hand_the_same_list_to_both_configs():
    from phantom_vlb_amd.config import instantiate, load_config
    cdir = os.path.join(ROOT, "config")
    mini = load_config(cdir, ["experiment=VLB_mini_synthetic_multisubject", "subject=sub-99"])
    dmc, lmc = instantiate(mini["datamodule"]["config"]), instantiate(mini["litmodule"]["config"])
    assert dmc.subjects == lmc.subjects == ["sub-01", "sub-02"] and dmc.lazyload_path.startswith("synthetic:")
    assert mini["output_dir"].endswith("sub-99")
    lora = load_config(cdir, ["experiment=VLB_vllama2_friends_lora_multisubject", "subject=all"])
    dmc, lmc = instantiate(lora["datamodule"]["config"]), instantiate(lora["litmodule"]["config"])
    assert dmc.subjects == lmc.subjects == ["sub-01", "sub-02", "sub-03", "sub-05"] and "{subject}" in dmc.lazyload_path
    assert lmc.use_lora and not lmc.freeze_backbone
    over = load_config(cdir, ["experiment=VLB_vllama2_friends_lora_multisubject", "subject=all", "subjects=[sub-01,sub-06]"])
    assert instantiate(over["datamodule"]["config"]).subjects == instantiate(over["litmodule"]["config"]).subjects == ["sub-01", "sub-06"]
    # the single-subject experiments are as they were
    plain = load_config(cdir, ["experiment=VLB_mini_synthetic", "subject=sub-01"])
    assert "subjects" not in plain["litmodule"]["config"] and instantiate(plain["datamodule"]["config"]).subjects is None


# ---------------------------------------------------------------------------------------------------- datamodule
def test_synthetic_multi_subject_datamodule():
    from phantom_vlb_amd.datamodule import VLBDataModule
    subjects = ["sub-01", "sub-02", "sub-03"]
    dm = VLBDataModule(_dm_cfg(subjects=subjects, lazyload_path="synthetic:3x4"))
    single = VLBDataModule(_dm_cfg(lazyload_path="synthetic:3x4"))
    train, val, train1, val1 = dm.datasets.train, dm.datasets.val, single.datasets.train, single.datasets.val
    # lengths add up: per subject what one subject gives (2 train files + 1 validation file of 4 samples each)
    assert len(train) == 3 * len(train1) == 24 and len(val) == 3 * len(val1) == 12
    names = dm.datasets.dset_names
    assert list(names) == subjects and all(len(v["val_set"]) == 1 and len(v["train_set"]) == 2 for v in names.values())
    assert names["sub-02"] == single.datasets.dset_names            # each subject's list is split as a single subject's is
    per = len(train1)
    seen = []
    for i in range(len(train)):
        item = train[i]
        assert item["subject"].dtype == torch.int64 and int(item["subject"]) == i // per
        seen.append(item["timeseries"])
    for i in range(len(val)):
        assert int(val[i]["subject"]) == i // len(val1)
    assert not torch.equal(seen[0], seen[per]) and not torch.equal(seen[per], seen[2 * per])      # subjects' samples differ
    # subject 0 of the list is the single-subject run's data
    assert torch.equal(seen[0], train1[0]["timeseries"])
    assert "subject" not in train1[0]
    batch = next(iter(dm.train_dataloader()))
    assert batch["subject"].shape == (2,) and batch["subject"].dtype == torch.int64 and not batch["subject"].is_cuda


def test_features_only_items_carry_subject():
    from phantom_vlb_amd.datamodule import VLBDataModule
    ds = VLBDataModule(_dm_cfg(subjects=["sub-01", "sub-02"], lazyload_path="synthetic:2x3")).datasets.train
    ds.features_only = True
    item = ds[len(ds) - 1]
    assert set(item) == {"index", "timeseries", "subject"} and int(item["subject"]) == 1 and int(item["index"]) == len(ds) - 1


# ---------------------------------------------------------------------------------------------------- callback
def _corr_ref(pred, y):
    return np.array([np.corrcoef(pred[:, v], y[:, v])[0, 1] for v in range(pred.shape[1])])


class _Module:
    def __init__(self, num_target, subjects):
        import types
        self.logged = {}
        self.config = types.SimpleNamespace(num_target=num_target, subjects=subjects)
        self.device = torch.device("cpu")

    def log(self, name, value, **kw):
        self.logged[name] = float(value)


def _run_callback(batches, subjects=None, max_roi_logs=2):
    from phantom_vlb_amd.utils import LogValAccuracyCallback
    cb = LogValAccuracyCallback()
    cb.max_roi_logs = max_roi_logs
    mod = _Module(batches[0]["brain_vals"].shape[1], subjects)
    cb.on_validation_epoch_start(None, mod)
    for i, out in enumerate(batches):
        cb.on_validation_batch_end(None, mod, out, None, i)
    cb.on_validation_epoch_end(None, mod)
    return mod.logged


def test_callback_per_subject_correlations():
    rng = np.random.RandomState(0)
    V, names = 6, ["sub-01", "sub-02", "sub-03", "sub-05"]          # sub-05 never appears
    subj = np.array([0, 1, 2, 1, 0, 2, 2, 1, 0, 0, 1, 2, 0, 1, 2, 2])
    y = rng.randn(16, V)
    pred = 0.5 * y + rng.randn(16, V) + subj[:, None]
    batches = [{"brain_preds": torch.tensor(pred[i:i + 4], dtype=torch.float32), "brain_vals": torch.tensor(y[i:i + 4], dtype=torch.float32),
                "subject": torch.tensor(subj[i:i + 4])} for i in range(0, 16, 4)]               # every batch mixes subjects
    logged = _run_callback(batches, subjects=names)
    means = []
    for g, name in enumerate(names[:3]):
        ref = _corr_ref(pred[subj == g].astype(np.float32).astype(np.float64), y[subj == g].astype(np.float32).astype(np.float64))
        assert abs(logged[f"val_corr_avg/{name}"] - ref.mean()) < 1e-6, name
        assert abs(logged[f"val_corr_ROI_000001/{name}"] - ref[1]) < 1e-6, name
        assert f"val_corr_ROI_000002/{name}" not in logged                                   # capped by max_roi_logs
        means.append(ref.mean())
    assert not any(k.endswith("/sub-05") for k in logged)
    assert abs(logged["val_corr_avg"] - np.mean(means)) < 1e-6                               # mean over the subjects that appeared


def test_callback_single_subject_path_unchanged():
    """without "subject" in the outputs: the pooled correlation over all clips, what the callback gave before"""
    rng = np.random.RandomState(1)
    y = rng.randn(12, 5).astype(np.float32)
    pred = (0.3 * y + rng.randn(12, 5)).astype(np.float32)
    batches = [{"brain_preds": torch.tensor(pred[i:i + 4]), "brain_vals": torch.tensor(y[i:i + 4])} for i in range(0, 12, 4)]
    logged = _run_callback(batches, max_roi_logs=5)
    ref = _corr_ref(pred.astype(np.float64), y.astype(np.float64))
    assert abs(logged["val_corr_avg"] - ref.mean()) < 1e-6
    assert set(logged) == {"val_corr_avg"} | {f"val_corr_ROI_{v:06d}" for v in range(5)}
    for v in range(5):
        assert abs(logged[f"val_corr_ROI_{v:06d}"] - ref[v]) < 1e-6


# ---------------------------------------------------------------------------------------------------- ABI
def test_new_entries_are_declared_bound_and_exported():
    """header == SIGNATURES == nm -D for the three new entries (parameter kinds in the same positions); ABI version still 2"""
    from phantom_vlb_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vlb.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()[-2] == "T"}
    want = {ctypes.c_void_p: "P", ctypes.c_int: "I", ctypes.c_float: "F"}
    for name, n in NEW_ENTRIES.items():
        m = re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(([^)]*)\)", text)
        assert m, f"{name} is not declared in include/vlb.h"
        params = [p.strip() for p in m.group(2).split(",")]
        assert len(params) == len(_lib.SIGNATURES[name]) == n, name
        kinds = ["P" if "*" in p else "F" if p.startswith("float") else "I" for p in params]
        assert kinds == [want[t] for t in _lib.SIGNATURES[name]], name
        assert (m.group(1) == "int64_t") == (_lib._RESTYPES.get(name) is ctypes.c_int64), name
        assert name in exported and hasattr(_lib.lib, name), name
    assert _lib.lib.vlb_abi_version() == 2
    assert "#define VLB_ABI_VERSION 2" in open(os.path.join(ROOT, "include", "vlb.h")).read()


def test_grouped_entries_refuse_bad_arguments_without_a_device():
    """nulls, G < 1 and more rows than the kernels index come back as errors before anything is launched; the workspace
    covers the forward's partials and the backward's slabs, and 16 heads of 65,536 x 4096 are within range"""
    from phantom_vlb_amd._lib import lib
    one = ctypes.c_void_p(16)
    ok = [one] * 22
    assert lib.vlb_head_fwd_grouped(*([None] + ok[1:]), 2, 512, 8, 2, 2, 1e-5, 1e-3, 0, None) != 0
    assert lib.vlb_head_fwd_grouped(*ok, 2, 512, 8, 0, 2, 1e-5, 1e-3, 0, None) != 0                     # G = 0
    assert lib.vlb_head_fwd_grouped(*ok, 2, 512, 8, 2, 2, 1e-5, 1e-3, 3, None) != 0                     # unknown loss_kind
    assert lib.vlb_head_fwd_grouped(*ok, 2, 512, 1, 2, 2, 1e-5, 1e-3, 2, None) != 0                     # pearson, V = 1
    assert lib.vlb_head_fwd_grouped(*ok, 2, 516, 8, 2, 2, 1e-5, 1e-3, 0, None) != 0                     # E % 8
    assert lib.vlb_head_fwd_grouped(*ok, 2, 512, 1 << 24, 16, 2, 1e-5, 1e-3, 0, None) != 0               # G*V > 2^27
    assert lib.vlb_head_bwd_grouped(*([None] + ok[1:]), 2, 512, 8, 2, 1e-5, 1e-3, 1.0, 1.0, 0, None) != 0
    assert lib.vlb_head_bwd_grouped(*ok, 2, 512, 8, 0, 1e-5, 1e-3, 1.0, 1.0, 0, None) != 0
    assert lib.vlb_head_bwd_grouped(*ok, 2, 512, 1 << 24, 16, 1e-5, 1e-3, 1.0, 1.0, 0, None) != 0
    assert b"G*V" in lib.vlb_last_error()
    assert lib.vlb_head_grouped_ws_floats(3, 512, 1 << 24, 16) == 0
    assert lib.vlb_head_grouped_ws_floats(3, 4096, 65536, 16) > 0
    for B, E, V, G in ((5, 512, 40, 3), (17, 1024, 40, 3), (3, 4096, 2048, 6), (2, 264, 48, 2)):
        ws = lib.vlb_head_grouped_ws_floats(B, E, V, G)
        assert ws >= 2 * GE.grouped_fwd_parts(B, E, V, G)
        sp = H.wgrad_splits(G * V)
        assert ws >= (sp * 16 * E + 16 * E + G * V * 8 + 4 * B if B <= 16 else 32 * B * E + 4 * B)


# ---------------------------------------------------------------------------------------------------- group_emul
def _autograd(inp):
    """fp64 torch autograd through G separate F.linear heads on one trunk, from (pooled_raw, sumw) on"""
    c, p, loss = inp["case"], inp["params"], inp["loss"]
    B, V, G, E = c["B"], c["V"], c["G"], c["E"]
    po = H.pool(inp["hidden"], inp["wmask"], inp["eps"])
    raw = po["pooled_raw"].clone().requires_grad_(True)
    leaf = {n: t.to(H.F64).clone().requires_grad_(True) for n, t in p.items()}
    heads = [(leaf[W_][g], leaf[B_][g]) for g in range(G)]
    pv = leaf["layer_norm1.weight"] * raw + leaf["layer_norm1.bias"] * po["sumw"][:, None]
    z = F.layer_norm(pv, (E,), leaf["layer_norm2.weight"], leaf["layer_norm2.bias"], inp["eps"])
    if inp["keep"] is not None:
        z = z * inp["keep"].to(H.F64)
    pred = torch.stack([F.linear(z[b], *heads[g]) for b, g in enumerate(inp["group"])])
    y = inp["y"].to(H.F64)
    if loss == "mse":
        data = F.mse_loss(pred, y)
    else:
        pc, yc = (pred - pred.mean(1, keepdim=True), y - y.mean(1, keepdim=True)) if loss == "pearson" else (pred, y)
        data = 1 - F.cosine_similarity(pc, yc, dim=-1).mean()
    l2 = sum(inp["lam"] * (w * w).sum() for w, _ in heads)
    (inp["loss_scale"] * data + inp["l2_scale"] * l2).backward()
    return dict(pred=pred.detach(), loss_terms=torch.stack([data, l2, data + l2]).detach(), dW=leaf[W_].grad, dbias=leaf[B_].grad,
                dg1=leaf["layer_norm1.weight"].grad, db1=leaf["layer_norm1.bias"].grad, dg2=leaf["layer_norm2.weight"].grad,
                db2=leaf["layer_norm2.bias"].grad, dpooled=raw.grad)


_RUNS = [(c["id"], "mse") for c in GE.CASES] + [(cid, k) for cid in GE.LOSS_CASES for k in L.LOSSES]


@pytest.mark.parametrize("cid,loss", _RUNS)
def test_group_emul_is_the_grouped_head(cid, loss):
    inp = GE.inputs_for(cid, loss)
    got, ref = GE.run(inp), _autograd(inp)
    for k, r in ref.items():
        rel = float((got[k] - r).abs().max() / (r.abs().max() + 1e-300))
        assert rel < 1e-12, (cid, loss, k, rel)


@pytest.mark.parametrize("cid,loss", _RUNS)
def test_bars_accept_an_honest_fp32_computation(cid, loss):
    inp = GE.inputs_for(cid, loss)
    assert set(inp["case"]["expect"]) <= GE.dispatch(inp["case"]["B"], inp["case"]["E"], inp["case"]["G"])
    ratios = GE.check_stages(GE.run(inp, dt=H.F32, device_like=True), inp)
    print(cid, loss, GE.by_stage(ratios))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (cid, loss, bad)


BUG_CASES = {
    "route_next": [c["id"] for c in GE.CASES],
    "flat_tiles": [c["id"] for c in GE.CASES if c["V"] % 16],            # V = 48: no tile straddles two heads
    "l2_present_only": ["g4-absent"],                                     # the case with heads that have no clip
    "gscale_group_count": [c["id"] for c in GE.CASES],
    "absent_dbias": ["g4-absent"],
}


def test_every_planted_bug_has_cases():
    assert set(BUG_CASES) == set(GE.BUGS) and all(BUG_CASES.values())
    assert {c["id"] for c in GE.CASES if c["V"] % 16 == 0} == {"g2-E264"}
    assert any(not idx.numel() for idx in GE.clips_of(GE.BY_ID["g4-absent"]["subjects"], 4))


@pytest.mark.parametrize("bug,cid", [(b, c) for b, cs in BUG_CASES.items() for c in cs])
def test_bars_reject_planted_bug(bug, cid):
    inp = GE.inputs_for(cid)
    stage = GE.BUGS[bug]
    bufs = GE.run(inp, dt=H.F32, device_like=True, bug=bug)
    worst = GE.by_stage(GE.check_stages(bufs, inp, (stage,)))[stage]
    print(bug, cid, stage, worst)
    assert worst > 1.0, (bug, cid, worst)


def test_grouped_dispatch_restates_the_planner():
    """the branch conditions GE.dispatch / GE.grouped_fwd_parts / GE.tile_of copy are the ones head.hip branches on (the
    library does not report its launches; what can be held fast is the source text).  The plain and the grouped head share
    one launcher per direction, so each condition is looked for in the ONE place it lives, and the grouped entries are held
    to calling those bodies with (group, G)."""
    src = re.sub(r"\s+", " ", (pathlib.Path(ROOT) / "phantom_vlb_amd" / "csrc" / "head.hip").read_text())
    entry_fwd = src[src.index('extern "C" int vlb_head_fwd_grouped('):src.index('extern "C" int vlb_head_bwd_grouped(')]
    entry_bwd = src[src.index('extern "C" int vlb_head_bwd_grouped('):]
    entry_bwd = entry_bwd[:entry_bwd.index('extern "C" int vlb_head_pool(')]
    assert "return head_fwd_tail(" in entry_fwd and "keep_scale, group, ws," in entry_fwd and "B, E, V, G, eps," in entry_fwd
    assert "return head_bwd_params(" in entry_bwd and "keep_scale, group, pooled_raw," in entry_bwd and "B, E, V, G, l2_lambda," in entry_bwd
    assert "hipLaunchKernelGGL" not in entry_fwd + entry_bwd               # argument checks and a call: no launch of their own
    tail = src[src.index("int head_fwd_tail("):src.index("int ridge_bwd_launch(")]
    assert "ridge_fwd_launch(ridge_w, ridge_b, z, y, group, pred, lpart, B, E, V, G, ridge_fwd_is_mfma(B, E), st);" in tail
    fwd = src[src.index("int ridge_fwd_launch_as("):src.index("int head_loss_corr_launch(")]
    assert "if (mfma) {" in fwd and "ridge_fwd_mfma_kernel<KS, GROUPED>" in fwd
    assert "ridge_fwd_kernel<GROUPED>" in fwd and "const int tpg = (V + 15) / 16, ntiles = G * tpg;" in fwd
    assert "group ? ridge_fwd_launch_as<true>(" in fwd and ": ridge_fwd_launch_as<false>(" in fwd
    bwd = src[src.index("int ridge_bwd_launch("):src.index("int head_bwd_params(")]
    assert "const int GV = G * V;" in bwd
    assert "if (B <= 16 && E % 8 == 0) {" in bwd and "vlb_wgrad_skinny(dpT, 16, ridge_w, E, dz16, wg_ws, GV, 16, E," in bwd
    assert "ridge_bwd_z_kernel<CORR, GROUPED>" in bwd and "ridge_bwd_w_kernel<CORR, GROUPED>" in bwd and "dpred_t_kernel<CORR, GROUPED>" in bwd
    for cond in ("bool ridge_fwd_is_mfma(int B, int E) { return B <= 16 && E % 128 == 0 && E <= 4096; }",
                 "return mfma ? (int)(ntiles < 2048 ? ntiles : 2048) : G * ((V + RIDGE_ROWS - 1) / RIDGE_ROWS);",
                 "const int g = GROUPED ? t / tpg : 0, tl = GROUPED ? t % tpg : t;", "constexpr int RIDGE_ROWS = 16;",
                 "constexpr int64_t GROUPED_MAX_ROWS = (int64_t)1 << 27;"):
        assert src.count(cond) == 1, cond
    # one copy of each: the MFMA condition, the skinny-dz condition, the block cap, the skinny-wgrad call
    for once in ("B <= 16 && E % 128 == 0 && E <= 4096", "if (B <= 16 && E % 8 == 0) {", "ntiles < 2048 ? ntiles : 2048", "vlb_wgrad_skinny("):
        assert src.count(once) == 1, once
    assert GE.GROUPED_MAX_ROWS == 1 << 27
    assert GE.dispatch(16, 4096, 2) >= {"ridge_fwd_mfma_kernel<32,grouped>", "wgrad_mfma_kernel"}
    assert GE.dispatch(17, 1024, 3) >= {"ridge_fwd_kernel<grouped>", "ridge_bwd_z_kernel<grouped>", "ridge_bwd_w:b0_passes=3"}
    assert "ridge_fwd_kernel<grouped>" in GE.dispatch(2, 264, 2) and "wgrad_mfma_kernel" in GE.dispatch(2, 264, 2)
    assert GE.grouped_fwd_parts(5, 512, 40, 3) == 9 and GE.grouped_fwd_parts(17, 1024, 40, 3) == 9
    assert GE.grouped_fwd_parts(3, 4096, 65536, 6) == 2048
    assert [GE.tile_of(t, 40) for t in (0, 2, 3, 5)] == [(0, 0), (0, 32), (1, 0), (1, 32)]
