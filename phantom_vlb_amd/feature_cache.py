"""Frozen-backbone feature cache: what the brain head needs of a clip, kept across epochs.

With ``freeze_backbone=True, use_lora=False`` nothing below the head trains and the frozen forward has no stochastic op,
so a clip's backbone output is the same in every epoch and every validation pass.  The head reads it only through two
fp32 quantities per clip: ``P[e] = sum_s w_s rstd_s (x_se - mu_s)`` (``pooled_raw``) and ``sum_s w_s``
(``sumw``).  ``FeatureCache`` keeps them per dataset index on the device; a batch whose clips are all cached runs the head
alone (``vlb_head_fwd_cached`` / ``vlb_head_bwd_cached``), on the same fp32 inputs and through the same kernels as the
uncached step.  Rows are written once (first write wins) and never change afterwards.

With ``readout_layers`` (K tapped decoder layers) a clip is K such vectors, one per tap and taken before the
learned mix, so the cache does not depend on the mix: ``FeatureCache(layers=K)`` keeps ``pooled`` as ``[K,N,E]`` (``sumw`` is the
same for every tap) and the fingerprint carries the normalised tap list.  Without the option nothing changes, in memory, on
disk or in the fingerprint.

Hit or miss is decided on a host-side bitmap (no device sync); the row indices are checked on the host before they are
uploaded.  Storage is allocated on first use: N * (E + 1) * 4 bytes for a split of N clips.
"""
from __future__ import annotations

import dataclasses
import hashlib
import json
import os
import warnings

import numpy as np
import torch

from ._lib import LIB_PATH, check, lib
from .head import check_readout_layers
from .ops import _stream

FORMAT_VERSION = 1
# Geometry fields that shape the frozen forward; the head's own (num_target, l2_lambda) and the adapters' are left out, so
# a persisted cache serves head hyper-parameter sweeps.
_HEAD_ONLY_FIELDS = ("num_target", "l2_lambda", "lora_r", "lora_alpha")


def _file_id(path: str) -> list:
    st = os.stat(path)
    return [os.path.abspath(path), st.st_size, st.st_mtime_ns]


_SHA_MEMO: dict = {}


def _sha256(path: str) -> str:
    key = tuple(_file_id(path))
    if key not in _SHA_MEMO:
        h = hashlib.sha256()
        with open(path, "rb") as f:
            for chunk in iter(lambda: f.read(1 << 20), b""):
                h.update(chunk)
        _SHA_MEMO[key] = h.hexdigest()
    return _SHA_MEMO[key]


def fingerprint(cfg, dataset, lib_path: str | None = None) -> str:
    """SHA-256 over everything the cached values depend on: format version; the geometry of the frozen forward and
    ``pack_tokens``; the weights (``init_seed`` of a random init, or the shard names / sizes / mtimes under ``model_path``);
    the dataset (file paths / sizes / mtimes, or the synthetic spec, plus N); the bytes of libvlb.so (a kernel change may
    change the features)."""
    from .litmodule import resolve_geometry
    g = dataclasses.asdict(resolve_geometry(cfg))
    for k in _HEAD_ONLY_FIELDS:
        g.pop(k, None)
    if cfg.model_path and os.path.isdir(cfg.model_path):
        weights = {"shards": [[f, *_file_id(os.path.join(cfg.model_path, f))[1:]] for f in sorted(os.listdir(cfg.model_path))
                              if f.endswith(".safetensors")]}
    else:
        weights = {"init_seed": int(cfg.init_seed)}
    files = []
    for p in dataset.ds_paths:
        if isinstance(p, tuple):          # synthetic:<files>x<samples> -> (seed, samples); the clips depend on geometry and V
            files.append(["synthetic", *[int(x) for x in p], dataset.geometry, int(dataset.num_target)])
        else:
            files.append(_file_id(str(p)))
    doc = {"format": FORMAT_VERSION, "geometry": g, "pack_tokens": bool(getattr(cfg, "pack_tokens", True)),
           "weights": weights, "dataset": {"files": files, "n": len(dataset)},
           "libvlb_sha256": _sha256(lib_path or LIB_PATH)}
    taps = getattr(cfg, "readout_layers", None)
    if taps is not None:                  # only when set: fingerprints (and caches) from before the option stay valid
        doc["readout_layers"] = [int(k) for k in check_readout_layers(taps, g["layers"])]
    subjects = getattr(cfg, "subjects", None)
    if subjects is not None:              # likewise: which subject a dataset index belongs to depends on the list and its order
        doc["subjects"] = [str(s) for s in subjects]
    return hashlib.sha256(json.dumps(doc, sort_keys=True).encode()).hexdigest()


class FeatureCache:
    """(pooled_raw, sumw) per dataset index of one split (train and val index spaces differ: one instance each)."""

    def __init__(self, split: str, n: int, dim: int, device, layers: int | None = None):
        """``layers`` = K with ``readout_layers`` set (K tapped layers: one ``pooled`` slab each, [K,N,E]; ``sumw`` does
        not depend on the layer); None: the single [N,E] slab of the last layer, in memory and on disk as ever."""
        if n <= 0 or dim <= 0 or (layers is not None and layers <= 0):
            raise ValueError(f"FeatureCache({split!r}): n={n}, dim={dim}, layers={layers}")
        self.split, self.n, self.E, self.dev = split, int(n), int(dim), torch.device(device)
        self.layers = None if layers is None else int(layers)
        self.valid = np.zeros(self.n, dtype=bool)        # host-side: hit / miss never syncs the device
        self.pooled = self.sumw = None                    # fp32 [N,E] / [N] on the device, allocated on first store
        self.hits = self.lookups = 0                      # batches since the last reset_counters()

    @property
    def nbytes(self) -> int:
        return self.n * ((self.layers or 1) * self.E + 1) * 4

    def _indices(self, indices) -> np.ndarray:
        idx = np.asarray(indices.cpu() if torch.is_tensor(indices) else indices, dtype=np.int64).reshape(-1)
        if idx.size == 0 or idx.min() < 0 or idx.max() >= self.n:
            raise IndexError(f"feature cache {self.split!r}: indices outside [0, {self.n}): {idx.tolist()}")
        return idx

    def _upload(self, rows: np.ndarray) -> torch.Tensor:
        host = torch.from_numpy(rows.astype(np.int32))
        if self.dev.type == "cuda":       # pinned: the copy is queued on the stream, the host does not wait for the device
            host = host.pin_memory()
        return host.to(self.dev, non_blocking=True)

    def _pooled_shape(self) -> tuple:
        return (self.n, self.E) if self.layers is None else (self.layers, self.n, self.E)

    def _alloc(self):
        if self.pooled is None:
            self.pooled = torch.zeros(*self._pooled_shape(), dtype=torch.float32, device=self.dev)
            self.sumw = torch.zeros(self.n, dtype=torch.float32, device=self.dev)

    def lookup(self, indices) -> bool:
        """True when every clip of the batch is cached."""
        hit = bool(self.valid[self._indices(indices)].all())
        self.lookups += 1
        self.hits += hit
        return hit

    def complete(self) -> bool:
        return bool(self.valid.all())

    def rows(self, indices) -> torch.Tensor:
        """Device int32 cache rows of a fully cached batch (for BrainHead.forward_cached)."""
        idx = self._indices(indices)
        if not self.valid[idx].all():
            raise KeyError(f"feature cache {self.split!r}: rows {idx[~self.valid[idx]].tolist()} are not cached")
        return self._upload(idx)

    def store(self, indices, head) -> int:
        """Write the batch's ``head.pooled_raw`` / ``head.sumw`` (the last head forward) into the rows of the clips not yet
        cached; rows already holding a value are left alone.  Returns the number of rows written."""
        idx = self._indices(indices)
        rows = np.full(idx.shape, -1, dtype=np.int64)
        fresh = ~self.valid[idx]
        _, first = np.unique(idx, return_index=True)      # a clip twice in one batch: its first position writes
        once = np.zeros(idx.shape, dtype=bool)
        once[first] = True
        fresh &= once
        if not fresh.any():
            return 0
        rows[fresh] = idx[fresh]
        self._alloc()
        dev_rows = self._upload(rows)
        if (self.layers or 0) != getattr(head, "K", 0):
            raise ValueError(f"feature cache {self.split!r}: {self.layers} slab(s) per clip, the head taps {head.K} layer(s)")
        # per slab: the tap's pooled vector (before the mix, so the cache outlives any change of the mix); sumw is the taps' own
        slabs = [(head.pooled_raw, head.sumw, self.pooled)] if self.layers is None else \
            [(head.p_stack[k], head.tap_sumw, self.pooled[k]) for k in range(self.layers)]
        for src, sw, dst in slabs:
            check(lib.vlb_feature_cache_store(src.data_ptr(), sw.data_ptr(), dev_rows.data_ptr(), dst.data_ptr(),
                                              self.sumw.data_ptr(), idx.size, self.E, self.n, _stream()),
                  "vlb_feature_cache_store")
        self.valid[idx[fresh]] = True
        return int(fresh.sum())

    def hit_rate(self) -> float | None:
        return self.hits / self.lookups if self.lookups else None

    def reset_counters(self):
        self.hits = self.lookups = 0

    # ------------------------------------------------------------------ persistence
    def _paths(self, d):
        return (os.path.join(d, f"{self.split}.pooled.npy"), os.path.join(d, f"{self.split}.sumw.npy"),
                os.path.join(d, f"{self.split}.json"))

    def save(self, d: str, fp: str) -> None:
        """``<split>.pooled.npy``, ``<split>.sumw.npy``, ``<split>.json``, each through a temporary file and a rename; the
        metadata (fingerprint) goes first and comes back last.  Complete caches only."""
        if not self.complete():
            raise RuntimeError(f"feature cache {self.split!r}: {int((~self.valid).sum())} of {self.n} rows missing")
        os.makedirs(d, exist_ok=True)
        pp, sp, jp = self._paths(d)
        if os.path.exists(jp):
            os.remove(jp)                 # an interrupted save leaves no metadata behind, so nothing half-written loads
        for path, t in ((pp, self.pooled), (sp, self.sumw)):
            tmp = path + ".tmp"
            with open(tmp, "wb") as f:
                np.save(f, t.cpu().numpy())
            os.replace(tmp, path)
        tmp = jp + ".tmp"
        with open(tmp, "w") as f:
            meta = {"format": FORMAT_VERSION, "fingerprint": fp, "n": self.n, "dim": self.E, "split": self.split}
            if self.layers is not None:
                meta["layers"] = self.layers
            json.dump(meta, f)
        os.replace(tmp, jp)

    def load(self, d: str, fp: str) -> bool:
        """Fill the cache from ``d`` when its fingerprint is ``fp``; otherwise (absent files: silently; a mismatch: with a
        warning) leave it untouched and return False."""
        pp, sp, jp = self._paths(d)
        if not all(os.path.exists(p) for p in (pp, sp, jp)):
            return False
        with open(jp) as f:
            meta = json.load(f)
        if meta.get("fingerprint") != fp or meta.get("n") != self.n or meta.get("dim") != self.E or meta.get("layers") != self.layers:
            warnings.warn(f"feature cache {self.split!r} under {d}: fingerprint mismatch (model, data, geometry or libvlb "
                          "changed) - ignored, the features are recomputed and the files overwritten")
            return False
        pooled, sumw = np.load(pp), np.load(sp)
        if pooled.shape != self._pooled_shape() or sumw.shape != (self.n,) or pooled.dtype != np.float32 or sumw.dtype != np.float32:
            warnings.warn(f"feature cache {self.split!r} under {d}: arrays do not match their metadata - ignored")
            return False
        self._alloc()
        self.pooled.copy_(torch.from_numpy(pooled))
        self.sumw.copy_(torch.from_numpy(sumw))
        self.valid[:] = True
        return True
