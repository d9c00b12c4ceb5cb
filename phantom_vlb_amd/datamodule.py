"""Mirror of the reference's ``src.datamodule`` (VLBDataModule, VLBDataModuleConfig, VLB_Dataset,
VLBDatasets; src/datamodule/videollama2_vlb_datamodule.py:24-238).

Same sample schema (6 arrays per sample: timeseries, vision, language as fp32 tensors; padvals,
vis_weights, lang_weights as numpy), same file-level train/val split (one random file is the
validation set, ``np.random.RandomState(random_state).choice``), same ``$SCRATCH_PATH`` /
``s*`` -> season substitution, same DataLoader settings.  HDF5 sample stores are read with h5py
when it is installed and with the package's own pure-Python reader (``h5lite``, pinned against files written by the real
h5py) otherwise.  Two additions because this environment has no CNeuroMod files:
  * ``.npz`` lazy-load files with the same keys (``{i}_{mod}`` + ``dset_len``) are read too
    (tools/h5_to_npz.py converts);
  * ``lazyload_path: synthetic:<n_files>x<samples>`` yields seeded synthetic samples.
"""
from __future__ import annotations

import glob
import os
from dataclasses import dataclass

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset


try:                                   # a LightningDataModule when Lightning is installed (reference datamodule :156), so the
    from lightning.pytorch import LightningDataModule as _Base      # reference's train.py can pass it to Trainer.fit
except Exception:
    class _Base:
        """Stand-in for ``lightning.pytorch.LightningDataModule`` where Lightning is absent: the built-in Trainer only calls
        ``train_dataloader`` / ``val_dataloader``."""

        def __init__(self):
            pass

MODS_T = ("timeseries", "vision", "language")
MODS_N = ("padvals", "vis_weights", "lang_weights")


def get_idx(ranges, val):
    for i, (lo, hi) in enumerate(ranges):
        if lo <= val < hi:
            return i
    return -1


@dataclass
class VLBDataModuleConfig:
    lazyload_path: str
    subject: str
    seasons: list
    delay: int
    window: int
    random_state: int
    shuffle_val_data: bool
    batch_size: int = 1
    num_workers: int = 0
    # extras
    geometry: str = "7b"
    num_target: int = 1000
    # two or more subject names: ``lazyload_path`` holds the literal ``{subject}`` and is expanded per subject (``synthetic:NxM``:
    # N files per subject), the subjects' datasets are concatenated in this order and every item carries "subject", its index
    # into this list (litmodule.config.subjects must be the same list).  None: one subject, ``subject``, as the reference
    subjects: list | None = None
    # the held-out test split: the same grammar as ``lazyload_path``, ``{subject}`` included; every matching
    # file of ``test_seasons`` (required with real files, expanded as ``seasons`` are) goes to ``datasets.test``, there is no
    # split; ``synthetic:NxM``: N files per subject with the seeds random_state + 5003 + k + 1009 g.  None: no test split
    test_lazyload_path: str | None = None
    test_seasons: list | None = None

    def __post_init__(self):
        from .head import check_subjects
        tp = self.test_lazyload_path
        if tp is not None:
            if not isinstance(tp, str) or not tp:
                raise ValueError(f"test_lazyload_path={tp!r}: a path pattern or synthetic:NxM is needed (leave it unset for no test split)")
            if not tp.startswith("synthetic:") and not self.test_seasons:
                raise ValueError(f"test_lazyload_path={tp!r} needs test_seasons, the seasons whose files form the test split")
            if self.subjects is not None and not tp.startswith("synthetic:") and "{subject}" not in tp:
                raise ValueError(f"subjects={list(self.subjects)!r} needs the literal {{subject}} in test_lazyload_path (it is expanded "
                                 f"per subject); got {tp!r}")
        if self.subjects is not None:
            self.subjects = list(check_subjects(self.subjects))
            if not self.lazyload_path.startswith("synthetic:") and "{subject}" not in self.lazyload_path:
                raise ValueError(f"subjects={self.subjects!r} needs the literal {{subject}} in lazyload_path (it is expanded per "
                                 f"subject); got {self.lazyload_path!r}")


def open_h5(path):
    """h5py when it is installed, else the package's own read-only HDF5 subset (h5lite) - same indexing surface."""
    try:
        import h5py
        return h5py.File(path, "r")
    except ImportError:
        from . import h5lite
        return h5lite.File(path)


class _H5File:
    """The reference's lazy-load sample store (src/preprocessing/videollama2_vlb_lazyloading.py:141-164), read exactly
    as its VLB_Dataset does (src/datamodule/...:83-109): f["{i}"]["{i}_{mod}"], f["dset_len"][0]."""

    def __init__(self, path):
        self.f = open_h5(path)
        self.length = int(np.array(self.f["dset_len"])[0])

    def get(self, i, mod):
        return np.array(self.f[f"{i}"][f"{i}_{mod}"])


class _NpzFile:
    def __init__(self, path):
        self.f = np.load(path, mmap_mode="r")
        self.length = int(self.f["dset_len"][0])

    def get(self, i, mod):
        return np.array(self.f[f"{i}_{mod}"])


class _SyntheticFile:
    def __init__(self, spec, geometry, num_target):
        from .geometry import geometry_7b, geometry_mini
        from .synthetic import synthetic_batch
        self.seed, self.length = spec
        self.g = geometry_mini(num_target=num_target) if geometry == "mini" else geometry_7b(num_target=num_target)
        self._gen = synthetic_batch

    def get(self, i, mod):
        b = self._gen(self.g, 1, seed=self.seed * 100003 + i)
        return b[mod][0].numpy()


class VLB_Dataset(Dataset):
    """``with_index`` adds the dataset index (``"index"``, int64) to every item; ``features_only`` makes an item
    ``{"index", "timeseries"}`` and reads nothing else from the file (a split whose frozen-backbone features are all
    cached, feature_cache.py).  Both are off by default and may be switched between epochs.  ``subject_of`` (one index per
    file, multi-subject runs) adds ``"subject"`` (int64) to every item, also under ``features_only``."""

    def __init__(self, ds_paths, geometry="7b", num_target=1000, subject_of=None):
        self.ds_paths, self.geometry, self.num_target = list(ds_paths), geometry, num_target
        self.subject_of = None if subject_of is None else [int(g) for g in subject_of]
        if self.subject_of is not None and len(self.subject_of) != len(self.ds_paths):
            raise ValueError(f"subject_of names {len(self.subject_of)} files, ds_paths {len(self.ds_paths)}")
        self.with_index = self.features_only = False
        self.ds_files, self.length, self.ranges = {}, 0, []
        for i, p in enumerate(ds_paths):
            if isinstance(p, tuple):
                f = _SyntheticFile(p, geometry, num_target)
            elif str(p).endswith(".npz"):
                f = _NpzFile(p)
            else:
                f = _H5File(p)
            self.ds_files[i] = {"ds_file": f, "idx_from": self.length}
            self.ranges.append((self.length, self.length + f.length))
            self.length += f.length

    def __len__(self):
        return self.length

    def __getitem__(self, idx):
        i = get_idx(self.ranges, idx)
        f = self.ds_files[i]["ds_file"]
        k = idx - self.ds_files[i]["idx_from"]
        subject = {} if self.subject_of is None else {"subject": torch.tensor(self.subject_of[i], dtype=torch.int64)}
        if self.features_only:
            return {"index": torch.tensor(int(idx), dtype=torch.int64),
                    "timeseries": torch.from_numpy(np.asarray(f.get(k, "timeseries"))).float(), **subject}
        item = {m: torch.from_numpy(np.asarray(f.get(k, m))).float() for m in MODS_T}
        item.update({m: np.asarray(f.get(k, m)) for m in MODS_N})
        if self.with_index:
            item["index"] = torch.tensor(int(idx), dtype=torch.int64)
        item.update(subject)
        return item


@dataclass
class VLBDatasets:
    config: VLBDataModuleConfig
    train: VLB_Dataset | None = None
    val: VLB_Dataset | None = None
    test: VLB_Dataset | None = None

    SUBJECT_SEED_STRIDE = 1009       # synthetic files of subject g: seeds random_state + k + 1009 g (subject 0: the single-subject run's)
    TEST_SEED_OFFSET = 5003          # synthetic test files: seeds random_state + 5003 + k + 1009 g

    def _expand(self, lazyload_path, seasons, seed_offset=0, prefix="synthetic"):
        """One subject's file list -> (files, their names): ``synthetic:NxM`` gives N seeded (seed, M) specs, anything else is
        globbed per season as the reference does"""
        c = self.config
        if lazyload_path.startswith("synthetic:"):
            n_files, n_samples = (int(x) for x in lazyload_path.split(":", 1)[1].split("x"))
            return [(c.random_state + k + seed_offset, n_samples) for k in range(n_files)], [f"{prefix}_{k}" for k in range(n_files)]
        f_list = []
        for s in seasons:
            f_list += sorted(glob.glob(
                lazyload_path.replace("$SCRATCH_PATH", os.environ.get("SCRATCH_PATH", ".")).replace("s*", f"{s}")))
        return f_list, [os.path.basename(x) for x in f_list]

    def _build_test(self, used):
        """``datasets.test`` from ``test_lazyload_path``: every matching file, no split; ``used``: the train and val files"""
        c = self.config
        path = getattr(c, "test_lazyload_path", None)
        self.test_names = {}
        if path is None:
            return
        subjects = getattr(c, "subjects", None)
        files, of, self.test_names = [], [], {}
        for g, name in enumerate(subjects or [None]):
            f, names = self._expand(path if name is None else path.replace("{subject}", name), c.test_seasons or [],
                                    self.TEST_SEED_OFFSET + self.SUBJECT_SEED_STRIDE * g, "synthetic_test")
            if not f:
                raise FileNotFoundError(f"no lazy-load files match test_lazyload_path={path!r}" + ("" if name is None else f" for {name!r}"))
            files, of = files + f, of + [g] * len(f)
            if name is None:
                self.test_names = {"test_set": names}
            else:
                self.test_names[name] = {"test_set": names}

        def key(x):         # a synthetic file is its seed, a real one its resolved path
            return ("seed", x[0]) if isinstance(x, tuple) else ("path", os.path.realpath(x))
        seen = {key(x) for x in used}
        both = [x for x in files if key(x) in seen]
        if both or len({key(x) for x in files}) != len(files):
            raise ValueError(f"test_lazyload_path={path!r}: {both or files!r} also belong to the train or validation split (or are "
                             "listed twice): a held-out split shares no file with them")
        self.test = VLB_Dataset(files, c.geometry, c.num_target, subject_of=None if subjects is None else of)

    def _split(self, lazyload_path, seed_offset=0):
        """One subject's file list, split as the reference does -> (val files, train files, their names as ``dset_names``)"""
        c = self.config
        f_list, names = self._expand(lazyload_path, c.seasons, seed_offset)
        if not f_list:
            raise FileNotFoundError(f"no lazy-load files match {lazyload_path!r}")
        r = np.random.RandomState(c.random_state)
        vi = int(r.choice(len(f_list), 1)[0])
        val_file = [f_list[vi]]
        train_files = [x for x in f_list if x != f_list[vi]]
        return val_file, train_files, {"val_set": [names[vi]], "train_set": [n for n, x in zip(names, f_list) if x != f_list[vi]]}

    def __post_init__(self):
        c = self.config
        subjects = getattr(c, "subjects", None)
        if subjects is None:
            val_file, train_files, self.dset_names = self._split(c.lazyload_path)
            self.val = VLB_Dataset(val_file, c.geometry, c.num_target)
            self.train = VLB_Dataset(train_files, c.geometry, c.num_target)
            self._build_test(val_file + train_files)
            return
        # one list and one split (one validation file, drawn with RandomState(random_state)) per subject, concatenated in order
        val, train, val_of, train_of, self.dset_names = [], [], [], [], {}
        for g, name in enumerate(subjects):
            v, t, self.dset_names[name] = self._split(c.lazyload_path.replace("{subject}", name), self.SUBJECT_SEED_STRIDE * g)
            val, train = val + v, train + t
            val_of, train_of = val_of + [g] * len(v), train_of + [g] * len(t)
        self.val = VLB_Dataset(val, c.geometry, c.num_target, subject_of=val_of)
        self.train = VLB_Dataset(train, c.geometry, c.num_target, subject_of=train_of)
        self._build_test(val + train)


class VLBDataModule(_Base):
    def __init__(self, config: VLBDataModuleConfig) -> None:
        super().__init__()
        self.config = config
        self.datasets = VLBDatasets(self.config)

    def x_dataloader(self, dataset, shuffle: bool = True, sampler=None):
        if dataset is None:
            raise AttributeError
        # pinned batches so DevicePrefetcher's host->device copies are truly asynchronous
        return DataLoader(dataset=dataset, batch_size=self.config.batch_size, shuffle=shuffle and sampler is None,
                          sampler=sampler, num_workers=self.config.num_workers, pin_memory=torch.cuda.is_available())

    def train_dataloader(self, rank: int = 0, world: int = 1):
        """reference :219-225 (shuffle=True).  The permutation is a function of (random_state, epoch) - set by
        ``sampler.set_epoch`` - instead of the global torch RNG, so a run resumed from a checkpoint continues with
        the same clip order; under data parallelism ranks draw disjoint, rank-strided clips of that permutation
        (the reference has no DistributedSampler: it never ran multi-GPU in mainline)."""
        from torch.utils.data.distributed import DistributedSampler
        sampler = DistributedSampler(self.datasets.train, num_replicas=world, rank=rank, shuffle=True,
                                     seed=self.config.random_state, drop_last=world > 1)
        return self.x_dataloader(dataset=self.datasets.train, sampler=sampler)

    def val_dataloader(self):
        return self.x_dataloader(dataset=self.datasets.val, shuffle=self.config.shuffle_val_data)

    def test_dataloader(self):
        """The held-out split in dataset order (never shuffled: a clip's bootstrap block is its rank in its head's clips)."""
        if self.datasets.test is None:
            raise ValueError("test_dataloader(): no test split - set datamodule.config.test_lazyload_path (and test_seasons)")
        return self.x_dataloader(dataset=self.datasets.test, shuffle=False)


class DevicePrefetcher:
    """Iterates a DataLoader one batch ahead of the consumer: the large tensors of batch i+1 (16.3 MB of fp32
    pixels per clip) are copied host->device on a side stream while step i computes, and are
    handed over with an event, so the step never waits on PCIe.  The token ids and ``padvals`` stay on the
    host: the step sizes its unpadded row layout from them without a device sync (they are tiny and are
    uploaded by the step itself); so does a multi-subject batch's ``subject`` index, which the head checks on the
    host.  Device tensors are tied to the consumer stream with ``record_stream`` so
    the caching allocator cannot recycle them while a kernel still reads them."""

    def __init__(self, loader, device, keep_on_host=("language", "padvals", "subject"), on_staged=None, on_discard=None):
        """``on_staged(batch, event)``: called for every batch right after its copies were enqueued (event = copies done),
        i.e. one step before the batch is handed over - VLBLitModule.prefetch_vision hooks in here.
        ``on_discard(batch)``: called for a batch that was staged but will never be handed over (the consumer stopped
        iterating: ``limit_val_batches``, ``max_steps``, an exception) - VLBLitModule.discard_prefetched_vision."""
        self.loader, self.device, self.keep = loader, torch.device(device), tuple(keep_on_host)
        self.on_staged, self.on_discard = on_staged, on_discard
        self.sampler = getattr(loader, "sampler", None)
        self.stream = torch.cuda.Stream(device=self.device)

    def __len__(self):
        return len(self.loader)

    def _stage(self, batch):
        out, ev = {}, torch.cuda.Event()
        with torch.cuda.stream(self.stream):
            for k, v in batch.items():
                out[k] = v if (k in self.keep or not torch.is_tensor(v)) else v.to(self.device, non_blocking=True)
            ev.record(self.stream)
        if self.on_staged is not None:
            self.on_staged(out, ev)
        return out, ev

    def __iter__(self):
        for _, batch in self.iter_selected():
            yield batch

    def iter_selected(self, select=None, limit=None):
        """Yields ``(index in the underlying loader, batch)`` for the batches with ``select(index)`` true (all when None),
        stopping in front of index ``limit``.  Only selected batches are copied to the device and announced through
        ``on_staged``: a batch the consumer skips (another rank's validation batch, the part of an epoch a resumed run has
        already seen) never starts a side-stream computation nobody would pick up."""
        def wanted():
            for i, b in enumerate(self.loader):
                if limit is not None and i >= limit:
                    return
                if select is None or select(i):
                    yield i, b
        it = wanted()
        nxt = None
        try:
            first = next(it, None)
            if first is None:
                return
            nxt = (first[0],) + self._stage(first[1])
            while nxt is not None:
                idx, cur, ev = nxt
                nxt = None
                follow = next(it, None)               # batch i+1 starts moving before step i is enqueued
                if follow is not None:
                    nxt = (follow[0],) + self._stage(follow[1])
                consumer = torch.cuda.current_stream(self.device)
                consumer.wait_event(ev)
                for v in cur.values():
                    if torch.is_tensor(v) and v.is_cuda:
                        v.record_stream(consumer)
                yield idx, cur
        finally:
            if nxt is not None and self.on_discard is not None:      # staged, never handed over
                self.on_discard(nxt[1])
            it.close()
