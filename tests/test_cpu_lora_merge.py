"""Merged LoRA adapters: the ABI entry, the config switch and the train.py plumbing (no GPU)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(**kw):
    from phantom_vlb_amd.litmodule import VLBLitModuleConfig
    base = dict(model_path="none", freeze_backbone=False, use_lora=True, lora_r=16, lora_alpha=32, lora_dropout=0.0,
                dropout_rate=0.0, num_target=128, l2_lambda=1e-3, lr=1e-4, betas=[0.9, 0.999], eps=1e-8, weight_decay=1e-2,
                lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=50000, geometry="mini")
    base.update(kw)
    return VLBLitModuleConfig(**base)


def test_lora_merge_is_declared_bound_and_exported():
    """header == SIGNATURES == nm -D for the new entry, and the ABI version is still 2 (the change is additive)."""
    from phantom_vlb_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vlb.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+vlb_lora_merge\s*\(([^)]*)\)", text)
    assert m, "vlb_lora_merge is not declared in include/vlb.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == len(_lib.SIGNATURES["vlb_lora_merge"]) == 12
    # pointers / ints / the fp32 scale in the same positions on both sides
    kinds = ["P" if "*" in p else "F" if p.startswith("float") else "I" for p in params]
    want = {ctypes.c_void_p: "P", ctypes.c_int: "I", ctypes.c_float: "F"}
    assert kinds == [want[t] for t in _lib.SIGNATURES["vlb_lora_merge"]]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert any(ln.split()[-1] == "vlb_lora_merge" and ln.split()[-2] == "T" for ln in out.splitlines())
    assert hasattr(_lib.lib, "vlb_lora_merge")
    assert _lib.lib.vlb_abi_version() == 2
    assert "#define VLB_ABI_VERSION 2" in open(os.path.join(ROOT, "include", "vlb.h")).read()


def test_merge_lora_for_eval_defaults_off_and_needs_lora():
    assert _cfg().merge_lora_for_eval is False
    assert _cfg(merge_lora_for_eval=True).merge_lora_for_eval is True
    with pytest.raises(ValueError, match="use_lora"):
        _cfg(merge_lora_for_eval=True, use_lora=False, freeze_backbone=True, lora_r=None, lora_alpha=None, lora_dropout=None)


def test_yaml_plumbing_reaches_the_switch_and_export_merged(tmp_path):
    """``litmodule.config.merge_lora_for_eval=true`` and the root key ``export_merged=<file>`` on the reference's command
    line; the committed YAML files set neither."""
    from phantom_vlb_amd.config import instantiate, load_config
    cdir = os.path.join(ROOT, "config")
    plain = load_config(cdir, ["experiment=VLB_vllama2_friends_lora"])
    assert "export_merged" not in plain and "merge_lora_for_eval" not in plain["litmodule"]["config"]
    target = str(tmp_path / "merged.safetensors")
    cfg = load_config(cdir, ["experiment=VLB_vllama2_friends_lora", "litmodule.config.merge_lora_for_eval=true",
                             f"export_merged={target}"])
    assert cfg["export_merged"] == target
    lc = instantiate(cfg["litmodule"]["config"])
    assert lc.merge_lora_for_eval is True and lc.use_lora
    assert instantiate(plain["litmodule"]["config"]).merge_lora_for_eval is False


def test_export_merged_writes_for_lora_and_refuses_without():
    import train

    class _Mod:
        def __init__(self, use_lora):
            self.config = type("C", (), {"use_lora": use_lora})()
            self.saved = []

        def save_merged(self, path):
            self.saved.append(path)
            return path

    m = _Mod(True)
    assert train.export_merged(m, "out/merged.safetensors") == "out/merged.safetensors"
    assert m.saved == ["out/merged.safetensors"]
    bare = _Mod(False)
    with pytest.raises(ValueError, match="LoRA"):
        train.export_merged(bare, "x.safetensors")
    assert bare.saved == []
    # train() itself refuses a non-LoRA run before anything is built
    with pytest.raises(ValueError, match="export_merged"):
        train.train({"export_merged": "x.safetensors", "litmodule": {"config": {"use_lora": False}}})
