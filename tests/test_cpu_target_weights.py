"""Per-target loss weights and masks above the kernels, on the CPU: the config validates ``target_weights``, the .npy
loader (one file, a stacked file, one file per ``{subject}``), the head's and the module's ``set_target_weights``, the
validation callback's masked averages against numpy on the kept columns, the checkpoint key, and the two new entry points
declared, bound and exported with the ABI version unchanged."""
import ctypes
import pathlib
import re
import subprocess
import types

import numpy as np
import pytest
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent


def _cfg(**kw):
    from phantom_vlb_amd.litmodule import VLBLitModuleConfig
    base = dict(model_path="none", freeze_backbone=True, use_lora=False, lora_r=None, lora_alpha=None, lora_dropout=None,
                dropout_rate=0.0, num_target=6, l2_lambda=1e-3, lr=1e-3, betas=[0.9, 0.999], eps=1e-8, weight_decay=1e-2,
                lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=100, geometry="mini")
    base.update(kw)
    return VLBLitModuleConfig(**base)


# ---------------------------------------------------------------------------------------------------- config
def test_config_validates_target_weights():
    assert _cfg().target_weights is None
    assert _cfg(target_weights="w.npy").target_weights == "w.npy"
    assert _cfg(target_weights="w_{subject}.npy", subjects=["a", "b"]).target_weights == "w_{subject}.npy"
    for bad in ("w.txt", "", 3, ["w.npy"]):
        with pytest.raises(ValueError, match="target_weights"):
            _cfg(target_weights=bad)
    with pytest.raises(ValueError, match="subjects"):
        _cfg(target_weights="w_{subject}.npy")
    with pytest.raises(ValueError, match="closed_form"):
        _cfg(target_weights="w.npy", ridge_fit="closed_form", cache_features=True)


def test_target_weights_are_reachable_from_the_command_line():
    from phantom_vlb_amd.config import instantiate, load_config
    cfg = load_config(str(ROOT / "config"), ["experiment=VLB_mini_synthetic", "litmodule.config.target_weights=w.npy"])
    assert instantiate(cfg["litmodule"]["config"]).target_weights == "w.npy"
    cfg = load_config(str(ROOT / "config"), ["experiment=VLB_mini_synthetic"])
    assert instantiate(cfg["litmodule"]["config"]).target_weights is None


# ---------------------------------------------------------------------------------------------------- the loader
def test_npy_loading(tmp_path):
    from phantom_vlb_amd.litmodule import load_target_weights
    w = np.array([1, 0, 0.5, 2, 0, 1], dtype=np.float64)
    np.save(tmp_path / "w.npy", w)
    got = load_target_weights(str(tmp_path / "w.npy"), 6)
    assert got.dtype == torch.float32 and got.tolist() == w.tolist()
    np.save(tmp_path / "mask.npy", w > 0)                                  # a boolean mask file
    assert load_target_weights(str(tmp_path / "mask.npy"), 6).tolist() == [1, 0, 1, 1, 0, 1]
    subs = ["sub-01", "sub-02"]
    assert load_target_weights(str(tmp_path / "w.npy"), 6, subs).shape == (6,)         # one row for every subject
    np.save(tmp_path / "stack.npy", np.stack([w, w[::-1]]))
    assert load_target_weights(str(tmp_path / "stack.npy"), 6, subs).tolist() == [w.tolist(), w[::-1].tolist()]
    for i, s in enumerate(subs):
        np.save(tmp_path / f"w_{s}.npy", w * (i + 1))
    got = load_target_weights(str(tmp_path / "w_{subject}.npy"), 6, subs)
    assert got.tolist() == [w.tolist(), (2 * w).tolist()]
    with pytest.raises(ValueError, match="does not exist"):
        load_target_weights(str(tmp_path / "w_{subject}.npy"), 6, ["sub-01", "sub-09"])
    with pytest.raises(ValueError, match=r"expected numbers of shape \[5\]"):
        load_target_weights(str(tmp_path / "w.npy"), 5)
    with pytest.raises(ValueError, match="expected"):
        load_target_weights(str(tmp_path / "stack.npy"), 6)                # [2,6] without subjects
    with pytest.raises(ValueError, match="expected"):
        load_target_weights(str(tmp_path / "stack.npy"), 6, ["a", "b", "c"])
    for bad in (-1.0, np.nan, np.inf):
        b = w.copy()
        b[2] = bad
        np.save(tmp_path / "bad.npy", b)
        with pytest.raises(ValueError, match="finite and >= 0"):
            load_target_weights(str(tmp_path / "bad.npy"), 6)


# ---------------------------------------------------------------------------------------------------- head and module
def test_head_checks_the_weights_on_the_host():
    from phantom_vlb_amd.head import BrainHead
    h = BrainHead(8, 4, 1e-3, 1e-5, "cpu", loss="pearson")
    assert h.tw is None
    h.set_target_weights(torch.tensor([1.0, 0.0, 0.5, 0.0]))
    assert h.tw.shape == (1, 4) and h.tw.tolist() == [[1.0, 0.0, 0.5, 0.0]]
    with pytest.raises(ValueError, match="the head has 1 target.*at least 2"):
        h.set_target_weights(torch.tensor([0.0, 0.0, 0.5, 0.0]))
    with pytest.raises(ValueError, match="the head, target 1: weight -2.0"):
        h.set_target_weights(torch.tensor([1.0, -2.0, 0.5, 0.0]))
    with pytest.raises(ValueError, match=r"fp32 tensor \[4\] or \[1,4\]"):
        h.set_target_weights(torch.ones(5))
    with pytest.raises(ValueError, match="fp32 tensor"):
        h.set_target_weights([1.0, 1.0, 1.0, 1.0])
    assert h.tw.tolist() == [[1.0, 0.0, 0.5, 0.0]]
    h.set_target_weights(None)
    assert h.tw is None
    g = BrainHead(8, 4, 1e-3, 1e-5, "cpu", subjects=["a", "b", "c"])
    g.set_target_weights(torch.tensor([1.0, 0.0, 0.5, 0.0]))                 # one row: every head alike
    assert g.tw.shape == (3, 4) and g.tw[2].tolist() == [1.0, 0.0, 0.5, 0.0]
    with pytest.raises(ValueError, match=r"head 2 \('c'\) has 0 target"):
        g.set_target_weights(torch.tensor([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 0, 0]]))
    with pytest.raises(ValueError, match="target weights"):
        g.ridge_stats_begin()
    g.set_target_weights(None)
    m = BrainHead(8, 4, 1e-3, 1e-5, "cpu")                                  # composes with a penalty per row
    m.set_target_weights(torch.tensor([0.0, 0.0, 3.0, 0.0]))


def test_module_keeps_the_weights_and_the_checkpoint_carries_them(tmp_path):
    from phantom_vlb_amd.head import BrainHead
    from phantom_vlb_amd.litmodule import VLBLitModule
    m = VLBLitModule(_cfg())
    m.rng_state = lambda: {}
    ck = {}
    m.on_save_checkpoint(ck)
    assert "vlb_target_weights" not in ck and m.target_weight_mask() is None
    w = torch.tensor([1.0, 0.0, 0.5, 2.0, 0.0, 1.0])
    m.set_target_weights(w.double())                                       # before the head exists: kept for configure_model
    assert m.target_weight_mask().tolist() == [[True, False, True, True, False, True]]
    m.on_save_checkpoint(ck)
    assert ck["vlb_target_weights"].dtype == torch.float32 and ck["vlb_target_weights"].flatten().tolist() == w.tolist()
    torch.save(ck, tmp_path / "ck.pt")
    ck = torch.load(tmp_path / "ck.pt", weights_only=False)
    m2 = VLBLitModule(_cfg())
    m2.set_rng_state = lambda s: None
    m2.on_load_checkpoint(ck)
    assert torch.equal(m2._target_weights.flatten(), w)
    m2.head = BrainHead(8, 6, 1e-3, 1e-5, "cpu")
    m2.on_load_checkpoint(ck)                                              # with the head: it takes them
    assert torch.equal(m2.head.tw, w[None]) and torch.equal(m2._target_weights, w[None])
    m2.set_target_weights(None)
    assert m2.head.tw is None and "_target_weights" not in m2.__dict__
    # a configured file must agree with the checkpoint
    np.save(tmp_path / "w.npy", w.numpy())
    np.save(tmp_path / "other.npy", (w + 1).numpy())
    m3 = VLBLitModule(_cfg(target_weights=str(tmp_path / "w.npy")))
    m3.set_rng_state = lambda s: None
    m3.on_load_checkpoint(ck)
    assert torch.equal(m3._target_weights.flatten(), w)
    m4 = VLBLitModule(_cfg(target_weights=str(tmp_path / "other.npy")))
    m4.set_rng_state = lambda s: None
    with pytest.raises(ValueError, match="differ from target_weights"):
        m4.on_load_checkpoint(ck)
    m5 = VLBLitModule(_cfg(ridge_fit="closed_form", cache_features=True))
    with pytest.raises(ValueError, match="closed_form"):
        m5.set_target_weights(w)


# ---------------------------------------------------------------------------------------------------- the callback
class _Module:
    def __init__(self, num_target, subjects, tw):
        self.logged = {}
        self.config = types.SimpleNamespace(num_target=num_target, subjects=subjects)
        self.device = torch.device("cpu")
        self._tw = tw

    def target_weight_mask(self):
        return None if self._tw is None else torch.as_tensor(self._tw).reshape(-1, self.config.num_target) > 0

    def log(self, name, value, **kw):
        self.logged[name] = float(value)


def _run_callback(batches, tw, subjects=None):
    from phantom_vlb_amd.utils import LogValAccuracyCallback
    cb = LogValAccuracyCallback()
    mod = _Module(batches[0]["brain_vals"].shape[1], subjects, tw)
    cb.on_validation_epoch_start(None, mod)
    for i, out in enumerate(batches):
        cb.on_validation_batch_end(None, mod, out, None, i)
    cb.on_validation_epoch_end(None, mod)
    return mod.logged, cb.correlations


def _corr_ref(p, y):
    p, y = p - p.mean(0), y - y.mean(0)
    return (p * y).sum(0) / np.sqrt((p * p).sum(0) * (y * y).sum(0))


def test_callback_scores_the_kept_targets_of_one_head():
    rng = np.random.RandomState(3)
    y = rng.randn(12, 6).astype(np.float32)
    pred = (0.4 * y + rng.randn(12, 6)).astype(np.float32)
    w = np.array([1, 0, 0.5, 2, 0, 1], dtype=np.float32)
    keep = w > 0
    ynan = y.copy()
    ynan[:, ~keep] = np.nan                                                 # masked targets may be NaN in the data
    batches = [{"brain_preds": torch.tensor(pred[i:i + 4]), "brain_vals": torch.tensor(ynan[i:i + 4])} for i in range(0, 12, 4)]
    logged, corr = _run_callback(batches, w)
    ref = _corr_ref(pred[:, keep].astype(np.float64), y[:, keep].astype(np.float64))
    assert abs(logged["val_corr_avg"] - ref.mean()) < 1e-6
    assert sorted(k for k in logged if "ROI" in k) == [f"val_corr_ROI_{i:06d}" for i in np.nonzero(keep)[0]]
    for j, i in enumerate(np.nonzero(keep)[0]):
        assert abs(logged[f"val_corr_ROI_{i:06d}"] - ref[j]) < 1e-6
    assert torch.isnan(corr).tolist() == (~keep).tolist()
    plain, corr0 = _run_callback([dict(b, brain_vals=torch.tensor(y[4 * i:4 * i + 4])) for i, b in enumerate(batches)], None)
    full = _corr_ref(pred.astype(np.float64), y.astype(np.float64))
    assert abs(plain["val_corr_avg"] - full.mean()) < 1e-6 and len([k for k in plain if "ROI" in k]) == 6     # without weights: as ever
    assert not bool(torch.isnan(corr0).any())


def test_callback_scores_each_subject_on_its_own_targets():
    rng = np.random.RandomState(4)
    V, names = 6, ["sub-01", "sub-02", "sub-03"]
    subj = np.array([0, 1, 2, 1, 0, 2, 2, 1, 0, 0, 1, 2, 0, 1, 2, 2])
    y = rng.randn(16, V).astype(np.float32)
    pred = (0.5 * y + rng.randn(16, V) + subj[:, None]).astype(np.float32)
    tw = np.array([[1, 1, 0, 0, 1, 1], [0, 1, 1, 1, 0, 0.5], [1, 0, 0, 0, 0, 2]], dtype=np.float32)
    batches = [{"brain_preds": torch.tensor(pred[i:i + 4]), "brain_vals": torch.tensor(y[i:i + 4]), "subject": torch.tensor(subj[i:i + 4])}
               for i in range(0, 16, 4)]
    logged, corr = _run_callback(batches, tw, subjects=names)
    means = []
    for g, name in enumerate(names):
        keep = tw[g] > 0
        ref = _corr_ref(pred[subj == g][:, keep].astype(np.float64), y[subj == g][:, keep].astype(np.float64))
        assert abs(logged[f"val_corr_avg/{name}"] - ref.mean()) < 1e-6, name
        assert sorted(k for k in logged if "ROI" in k and k.endswith(name)) == [f"val_corr_ROI_{i:06d}/{name}" for i in np.nonzero(keep)[0]]
        assert torch.isnan(corr[g]).tolist() == (~keep).tolist()
        means.append(ref.mean())
    assert abs(logged["val_corr_avg"] - np.mean(means)) < 1e-6


# ---------------------------------------------------------------------------------------------------- C-ABI
NEW = ("vlb_head_wloss_fwd", "vlb_head_bwd_wloss")


def test_entry_points_are_declared_bound_and_exported():
    from phantom_vlb_amd import _lib
    header = (ROOT / "include" / "vlb.h").read_text()
    assert re.search(r"#define VLB_ABI_VERSION 2\b", header) and _lib.lib.vlb_abi_version() == 2
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()[-2] == "T"}
    want = {ctypes.c_void_p: "P", ctypes.c_int: "I", ctypes.c_float: "F"}
    for name in NEW:
        m = re.search(r"\bint " + name + r"\(([^)]*)\);", text)
        assert m, f"{name} is not declared in include/vlb.h"
        args = [a.strip() for a in m.group(1).split(",")]
        kinds = ["P" if "*" in a else "F" if a.startswith("float ") else "I" if a.startswith("int ") else "?" for a in args]
        assert kinds == [want[t] for t in _lib.SIGNATURES[name]], (name, kinds)
        assert name in exported and getattr(_lib.lib, name) is not None
    flat = re.sub(r"\s+", " ", header)
    doc = re.search(r"/\*((?:(?!\*/).)*)\*/ int vlb_head_wloss_fwd\(", flat)
    assert doc and all(s in doc.group(1) for s in ("W_b", "S_ut", "1e-8", "a select", "l2_scale*2*lambda*W"))
    assert "vlb_head_wloss_fwd" in (ROOT / "phantom_vlb_amd" / "csrc" / "libvlb.map").read_text()
    # the backward entry takes the cached form's pointers plus tw, group, wstat and dpred
    assert _lib.SIGNATURES["vlb_head_bwd_wloss"].count(_lib.P) == _lib.SIGNATURES["vlb_head_bwd_cached"].count(_lib.P) + 4
    for old in ("vlb_head_fwd", "vlb_head_bwd", "vlb_head_fwd_cached", "vlb_head_bwd_cached", "vlb_head_loss_fwd", "vlb_head_fwd_grouped",
                "vlb_head_bwd_grouped"):
        assert old in _lib.SIGNATURES and old in exported
