"""Frozen-backbone feature cache, host side (no GPU): config validation, the dataset's index / features-only items, the
fingerprint that guards a persisted cache, save / load, and the built-in Trainer refusing data parallelism."""
import os
import shutil

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _cfg(**kw):
    from phantom_vlb_amd.litmodule import VLBLitModuleConfig
    base = dict(model_path="none", freeze_backbone=True, use_lora=False, lora_r=None, lora_alpha=None, lora_dropout=None,
                dropout_rate=0.1, num_target=128, l2_lambda=1e-3, lr=1e-3, betas=[0.9, 0.999], eps=1e-8,
                weight_decay=1e-2, lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=50000, geometry="mini")
    base.update(kw)
    return VLBLitModuleConfig(**base)


def test_config_accepts_cache_only_with_a_frozen_backbone():
    c = _cfg(cache_features=True)
    assert c.cache_features and c.feature_cache_dir is None
    assert _cfg().cache_features is False                      # off by default
    with pytest.raises(ValueError, match="frozen backbone"):
        _cfg(cache_features=True, use_lora=True, lora_r=16, lora_alpha=32, lora_dropout=0.1)
    with pytest.raises(ValueError, match="frozen backbone"):
        _cfg(cache_features=True, freeze_backbone=False)       # full fine-tune
    with pytest.raises(ValueError):
        _cfg(cache_features=True, freeze_backbone=False, use_lora=True, lora_r=16, lora_alpha=32, lora_dropout=0.1)


class _Counting:
    """Wraps a sample store and records every (i, mod) it is asked for."""

    def __init__(self, f):
        self.f, self.calls = f, []
        self.length = f.length

    def get(self, i, mod):
        self.calls.append(mod)
        return self.f.get(i, mod)


def _count_gets(ds):
    for v in ds.ds_files.values():
        v["ds_file"] = _Counting(v["ds_file"])
    return [v["ds_file"] for v in ds.ds_files.values()]


def _check_flags(ds, indices):
    full = {i: ds[i] for i in indices}
    assert "index" not in full[indices[0]]                     # default items are unchanged
    ds.with_index = True
    for i in indices:
        it = ds[i]
        assert set(it) == set(full[i]) | {"index"}
        assert it["index"].dtype == torch.int64 and int(it["index"]) == i
        assert torch.equal(it["timeseries"], full[i]["timeseries"])
    ds.features_only = True
    counters = _count_gets(ds)
    for i in indices:
        it = ds[i]
        assert set(it) == {"index", "timeseries"}
        assert int(it["index"]) == i and torch.equal(it["timeseries"], full[i]["timeseries"])
    assert sorted({m for c in counters for m in c.calls}) == ["timeseries"]
    assert sum(len(c.calls) for c in counters) == len(indices)
    from torch.utils.data import DataLoader
    b = next(iter(DataLoader(ds, batch_size=3)))
    assert set(b) == {"index", "timeseries"} and b["index"].tolist() == [0, 1, 2]


def test_dataset_index_and_features_only_on_the_synthetic_set():
    from phantom_vlb_amd.datamodule import VLB_Dataset
    ds = VLB_Dataset([(7, 3), (8, 2)], geometry="mini", num_target=16)
    _check_flags(ds, [0, 2, 4])


def test_dataset_index_and_features_only_on_the_h5_fixture():
    from phantom_vlb_amd.datamodule import VLB_Dataset
    path = os.path.join(GOLD, "lazyload_fixture.h5")
    ds = VLB_Dataset([path, path])
    _check_flags(ds, [0, 4, 7])


def _lib_copy(tmp_path, name="lib.so"):
    from phantom_vlb_amd import _lib
    p = tmp_path / name
    shutil.copyfile(_lib.LIB_PATH, p)
    return str(p)


def test_fingerprint_is_stable_and_sees_every_input(tmp_path):
    from phantom_vlb_amd.datamodule import VLB_Dataset
    from phantom_vlb_amd.feature_cache import fingerprint
    lib = _lib_copy(tmp_path)
    data = tmp_path / "clips.h5"
    shutil.copyfile(os.path.join(GOLD, "lazyload_fixture.h5"), data)
    ds = lambda: VLB_Dataset([str(data)])
    base = fingerprint(_cfg(cache_features=True), ds(), lib_path=lib)
    assert base == fingerprint(_cfg(cache_features=True), ds(), lib_path=lib)         # two constructions
    # head-only hyper-parameters leave it alone (a persisted cache serves head sweeps)
    assert base == fingerprint(_cfg(cache_features=True, l2_lambda=0.5, lr=3e-4, dropout_rate=0.3), ds(), lib_path=lib)
    assert base != fingerprint(_cfg(cache_features=True, init_seed=99), ds(), lib_path=lib)
    assert base != fingerprint(_cfg(cache_features=True, pack_tokens=False), ds(), lib_path=lib)
    assert base != fingerprint(_cfg(cache_features=True, geometry="7b"), ds(), lib_path=lib)
    st = os.stat(data)
    with open(data, "ab") as f:                                  # a dataset file's size
        f.write(b"\0")
    os.utime(data, ns=(st.st_atime_ns, st.st_mtime_ns))
    assert base != fingerprint(_cfg(cache_features=True), ds(), lib_path=lib)
    with open(data, "r+b") as f:
        f.truncate(st.st_size)
    os.utime(data, ns=(st.st_atime_ns, st.st_mtime_ns))
    assert base == fingerprint(_cfg(cache_features=True), ds(), lib_path=lib)
    lst = os.stat(lib)
    with open(lib, "r+b") as f:                                  # the library bytes (same size)
        f.seek(100)
        byte = f.read(1)
        f.seek(100)
        f.write(bytes([byte[0] ^ 0xFF]))
    os.utime(lib, ns=(lst.st_atime_ns, lst.st_mtime_ns + 1))
    assert base != fingerprint(_cfg(cache_features=True), ds(), lib_path=lib)
    # the synthetic set: its spec and N
    syn = fingerprint(_cfg(cache_features=True), VLB_Dataset([(1, 4)], "mini", 128), lib_path=lib)
    assert syn != fingerprint(_cfg(cache_features=True), VLB_Dataset([(1, 5)], "mini", 128), lib_path=lib)
    assert syn != fingerprint(_cfg(cache_features=True), VLB_Dataset([(2, 4)], "mini", 128), lib_path=lib)
    # a checkpoint directory: shard names / sizes
    ck = tmp_path / "ckpt"
    ck.mkdir()
    (ck / "model-00001.safetensors").write_bytes(b"x" * 10)
    a = fingerprint(_cfg(cache_features=True, model_path=str(ck)), ds(), lib_path=lib)
    (ck / "model-00001.safetensors").write_bytes(b"x" * 11)
    assert a != fingerprint(_cfg(cache_features=True, model_path=str(ck)), ds(), lib_path=lib)


def test_cache_save_load_round_trip_and_mismatch(tmp_path):
    """Host-side state and the files (a CPU 'device': no kernel runs here)."""
    from phantom_vlb_amd.feature_cache import FeatureCache
    c = FeatureCache("train", 5, 8, "cpu")
    assert c.nbytes == 5 * 9 * 4 and not c.complete()
    assert not c.lookup([0, 1]) and c.hit_rate() == 0.0
    with pytest.raises(IndexError):
        c.lookup([0, 5])
    with pytest.raises(IndexError):
        c.lookup([-1])
    with pytest.raises(RuntimeError):
        c.save(str(tmp_path), "fp")                              # incomplete caches are not written
    c._alloc()
    c.pooled.copy_(torch.arange(40, dtype=torch.float32).reshape(5, 8))
    c.sumw.copy_(torch.tensor([1.5, 2.5, 3.5, 4.5, 5.5]))
    c.valid[:] = True
    assert c.lookup([4, 0]) and c.complete()
    c.save(str(tmp_path), "fp-a")
    assert sorted(os.listdir(tmp_path)) == ["train.json", "train.pooled.npy", "train.sumw.npy"]
    d = FeatureCache("train", 5, 8, "cpu")
    assert d.load(str(tmp_path), "fp-a") and d.complete()
    assert torch.equal(d.pooled, c.pooled) and torch.equal(d.sumw, c.sumw)
    e = FeatureCache("train", 5, 8, "cpu")
    with pytest.warns(UserWarning, match="fingerprint mismatch"):
        assert not e.load(str(tmp_path), "fp-b")
    assert not e.complete() and e.pooled is None
    with pytest.warns(UserWarning):
        assert not FeatureCache("train", 6, 8, "cpu").load(str(tmp_path), "fp-a")      # another N
    assert not FeatureCache("val", 5, 8, "cpu").load(str(tmp_path), "fp-a")            # nothing saved for val
    assert np.load(tmp_path / "train.pooled.npy").dtype == np.float32


def test_builtin_trainer_refuses_cache_features_under_data_parallelism(monkeypatch):
    from phantom_vlb_amd.litmodule import VLBLitModule
    from phantom_vlb_amd.trainer import Trainer
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    tr = Trainer(devices=2, max_epochs=1)
    m = VLBLitModule(_cfg(cache_features=True))
    with pytest.raises(ValueError, match="single-process"):
        tr.fit(m, datamodule=None)
    assert getattr(m, "nnmodule", None) is None                  # refused before the model (and the GPU) was touched
