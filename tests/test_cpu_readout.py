"""``readout_layers`` (the head reads chosen decoder layers through a learned mix), host side: config validation, the new
ABI entries, the feature-cache fingerprint and the K-slab cache files, the YAML plumbing.  No GPU."""
import ctypes
import dataclasses
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_ENTRIES = {"vlb_head_pool": 12, "vlb_feature_cache_gather": 9, "vlb_head_mix_fwd": 8, "vlb_head_mix_ws_floats": 3,
               "vlb_head_mix_bwd": 10, "vlb_head_dhidden": 12}


def _cfg(**kw):
    from phantom_vlb_amd.litmodule import VLBLitModuleConfig
    base = dict(model_path="none", freeze_backbone=True, use_lora=False, lora_r=None, lora_alpha=None, lora_dropout=None,
                dropout_rate=0.1, num_target=128, l2_lambda=1e-3, lr=1e-3, betas=[0.9, 0.999], eps=1e-8,
                weight_decay=1e-2, lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=50000, geometry="mini")
    base.update(kw)
    return VLBLitModuleConfig(**base)


_LORA = dict(freeze_backbone=False, use_lora=True, lora_r=16, lora_alpha=32, lora_dropout=0.1)


def test_default_is_unset_and_negative_indices_normalise():
    from phantom_vlb_amd.litmodule import resolve_geometry
    assert _cfg().readout_layers is None
    L = resolve_geometry(_cfg()).layers
    assert L == 2
    assert _cfg(readout_layers=[-1]).readout_layers == [L]
    assert _cfg(readout_layers=[1, -1]).readout_layers == [1, L]
    assert _cfg(readout_layers=[-2, -1]).readout_layers == [1, 2]
    assert _cfg(readout_layers=[1], **_LORA).readout_layers == [1]
    assert _cfg(readout_layers=[8, 16, 24, 32], geometry="7b").readout_layers == [8, 16, 24, 32]
    assert _cfg(readout_layers=[-1], geometry="7b").readout_layers == [32]
    c = _cfg(readout_layers=[-1])
    assert dataclasses.replace(c, lr=1.0).readout_layers == [L]             # normalising is idempotent


@pytest.mark.parametrize("bad,names", [([2, 1], "1"), ([1, 1], "1"), ([0], "0"), ([3], "3"), ([-3], "-3"), ([1, -2], "1"),
                                       ([], "[]"), ([1.5], "1.5"), ("12", "12")])
def test_bad_lists_raise_and_name_the_value(bad, names):
    with pytest.raises(ValueError, match="readout_layers") as e:
        _cfg(readout_layers=bad)
    assert names in str(e.value)


def test_refused_with_the_full_fine_tune():
    with pytest.raises(ValueError, match=r"readout_layers.*freeze_backbone=False, use_lora=False"):
        _cfg(readout_layers=[1], freeze_backbone=False, use_lora=False)
    # everything already refused stays refused
    with pytest.raises(ValueError, match="frozen backbone"):
        _cfg(readout_layers=[1], cache_features=True, **_LORA)


def test_new_entries_are_declared_bound_and_exported():
    """header == SIGNATURES == nm -D for every new entry (parameter kinds in the same positions); ABI version still 2."""
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
    # the slab size the host allocates: K partials per 1024-element block of [B,E]
    assert _lib.lib.vlb_head_mix_ws_floats(5, 3, 4104) == 5 * -(-3 * 4104 // 1024)


def test_entries_refuse_bad_arguments_without_a_device():
    """null pointers and shapes outside the kernels' range come back as VLB_ERR_INVALID before anything is launched"""
    from phantom_vlb_amd._lib import lib
    one = ctypes.c_void_p(16)
    assert lib.vlb_head_mix_fwd(None, None, one, one, 1, 1, 8, None) != 0
    assert lib.vlb_head_mix_fwd(one, None, one, one, 2, 1, 8, None) != 0 and b"logits" in lib.vlb_last_error()
    assert lib.vlb_head_mix_fwd(one, one, one, one, 65, 1, 8, None) != 0
    assert lib.vlb_head_mix_fwd(one, one, one, one, 2, 1, 12, None) != 0
    assert lib.vlb_head_mix_bwd(one, one, one, one, one, None, 2, 1, 8, None) != 0
    assert lib.vlb_head_dhidden(one, one, one, one, one, 2, 4, 8, one, 9, 1, None) != 0 and b"total_rows" in lib.vlb_last_error()
    assert lib.vlb_head_dhidden(one, one, one, one, None, 2, 4, 8, None, 0, 0, None) != 0
    assert lib.vlb_head_pool(one, one, one, one, one, one, 1, 4, 12, 1e-5, None, None) != 0
    assert lib.vlb_feature_cache_gather(one, one, None, one, one, 1, 8, 4, None) != 0


def test_fingerprint_is_unchanged_when_unset_and_follows_the_tap_list(tmp_path):
    from phantom_vlb_amd import feature_cache as FC
    from phantom_vlb_amd.datamodule import VLB_Dataset
    from phantom_vlb_amd.litmodule import resolve_geometry
    lib = tmp_path / "libvlb.so"
    lib.write_bytes(b"not a library, only bytes to hash")
    ds = VLB_Dataset([(1, 4)], "mini", 128)
    cfg = _cfg(cache_features=True)
    unset = FC.fingerprint(cfg, ds, lib_path=str(lib))
    # the document as it was before the option existed, restated: an unset option adds no key to it
    g = dataclasses.asdict(resolve_geometry(cfg))
    for k in ("num_target", "l2_lambda", "lora_r", "lora_alpha"):
        g.pop(k, None)
    doc = {"format": 1, "geometry": g, "pack_tokens": True, "weights": {"init_seed": 1234},
           "dataset": {"files": [["synthetic", 1, 4, "mini", 128]], "n": 4},
           "libvlb_sha256": hashlib.sha256(lib.read_bytes()).hexdigest()}
    assert unset == hashlib.sha256(json.dumps(doc, sort_keys=True).encode()).hexdigest()
    one = FC.fingerprint(_cfg(cache_features=True, readout_layers=[1]), ds, lib_path=str(lib))
    two = FC.fingerprint(_cfg(cache_features=True, readout_layers=[1, 2]), ds, lib_path=str(lib))
    assert len({unset, one, two}) == 3
    assert two == FC.fingerprint(_cfg(cache_features=True, readout_layers=[-2, -1]), ds, lib_path=str(lib))      # normalised
    assert FC.fingerprint(_cfg(cache_features=True, readout_layers=[2]), ds, lib_path=str(lib)) != unset       # set is set


def test_k_slab_cache_files_round_trip_and_legacy_files_are_unchanged(tmp_path):
    from phantom_vlb_amd.feature_cache import FeatureCache
    c = FeatureCache("train", 5, 8, "cpu", layers=2)
    assert c.nbytes == 5 * (2 * 8 + 1) * 4
    c._alloc()
    assert tuple(c.pooled.shape) == (2, 5, 8)
    c.pooled.copy_(torch.arange(80, dtype=torch.float32).reshape(2, 5, 8))
    c.sumw.copy_(torch.arange(5, dtype=torch.float32))
    c.valid[:] = True
    c.save(str(tmp_path), "fp-k2")
    assert json.load(open(tmp_path / "train.json"))["layers"] == 2
    d = FeatureCache("train", 5, 8, "cpu", layers=2)
    assert d.load(str(tmp_path), "fp-k2") and torch.equal(d.pooled, c.pooled) and torch.equal(d.sumw, c.sumw)
    for other in (None, 1, 3):                    # another number of slabs never loads these files
        with pytest.warns(UserWarning, match="fingerprint mismatch"):
            assert not FeatureCache("train", 5, 8, "cpu", layers=other).load(str(tmp_path), "fp-k2")
    # without the option: [N,E] in memory, no "layers" key on disk - the files of a cache from before the option
    old = tmp_path / "old"
    e = FeatureCache("train", 5, 8, "cpu")
    assert e.layers is None and e.nbytes == 5 * 9 * 4
    e._alloc()
    assert tuple(e.pooled.shape) == (5, 8)
    e.valid[:] = True
    e.save(str(old), "fp-a")
    assert set(json.load(open(old / "train.json"))) == {"format", "fingerprint", "n", "dim", "split"}
    assert np.load(old / "train.pooled.npy").shape == (5, 8)
    assert FeatureCache("train", 5, 8, "cpu").load(str(old), "fp-a")


def test_yaml_plumbing_reaches_the_field():
    from phantom_vlb_amd.config import instantiate, load_config
    cdir = os.path.join(ROOT, "config")
    plain = load_config(cdir, ["experiment=VLB_vllama2_friends_lora"])
    assert "readout_layers" not in plain["litmodule"]["config"]
    assert instantiate(plain["litmodule"]["config"]).readout_layers is None
    cfg = load_config(cdir, ["experiment=VLB_vllama2_friends_lora", "litmodule.config.readout_layers=[16,24,32]"])
    assert instantiate(cfg["litmodule"]["config"]).readout_layers == [16, 24, 32]


def test_head_param_names_follow_the_taps():
    """HEAD_PARAMS itself is as it was; a head lists (creates, stores) layer_mix.weight only for K > 1, initial value 0
    (construction launches nothing, so a host-side head serves)."""
    from phantom_vlb_amd import head
    assert head.HEAD_PARAMS == ("layer_norm1.weight", "layer_norm1.bias", "layer_norm2.weight", "layer_norm2.bias",
                                "ridge_layer.linear.weight", "ridge_layer.linear.bias")
    assert head.LAYER_MIX == "layer_mix.weight"
    for taps, extra in ((None, ()), ([2], ()), ([1, 2], (head.LAYER_MIX,))):
        h = head.BrainHead(8, 4, 1e-3, 1e-5, "cpu", readout_layers=taps)
        assert h.param_names == head.HEAD_PARAMS + extra and tuple(h.master) == h.param_names == tuple(h.grads)
        if extra:
            assert h.master[head.LAYER_MIX].dtype == torch.float32 and h.master[head.LAYER_MIX].tolist() == [0.0, 0.0]
            assert h.compute[head.LAYER_MIX].dtype == torch.bfloat16
