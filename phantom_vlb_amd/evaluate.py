"""Held-out evaluation per target: Pearson r, R^2 and MSE of every target over a split, with a block-bootstrap
standard error and one-sided p-value, written as one ``.npz`` - the vector the reference's
``src/postprocessing/make_acc_brainmaps.py`` reads, for voxel heads too.

``TargetScores`` keeps the five running sums of the reference's validation callback (src/utils.py:85-110) on the device in
fp64, per head and per block of ``block`` consecutive clips (vlb_score_accumulate); ``finish`` turns them into the scores
(vlb_score_finish) and resamples the blocks (vlb_score_bootstrap).  fMRI samples are autocorrelated, so clips are resampled in
contiguous blocks, the same reason ``ridge_cv_block`` exists.  One process; no fallback: the kernels are libvlb's.
"""
from __future__ import annotations

import warnings

import numpy as np
import torch

SUBJECT_SEED_STRIDE = 1009          # head g draws from RandomState(seed + 1009 g)
FIRST_BLOCKS = 4                    # blocks per head the slab starts with


def check_score_block(block) -> int:
    if isinstance(block, bool) or not isinstance(block, int) or block < 1:
        raise ValueError(f"score_block={block!r}: an integer >= 1 is needed (contiguous clips per bootstrap block)")
    return block


def check_score_bootstrap(R) -> int:
    if isinstance(R, bool) or not isinstance(R, int) or R < 0 or R == 1:
        raise ValueError(f"score_bootstrap={R!r}: 0 (no bootstrap) or an integer >= 2 (resamples) is needed")
    return R


def clip_blocks(counts: list, heads, block: int):
    """The (head, block) of every clip of a batch in dataset order: a clip's block is its rank within its head's clips so far,
    integer-divided by ``block`` (the rule of ``ridge_cv_block``'s fold).  ``counts`` (clips seen per head) is advanced in place."""
    out = []
    for h in heads:
        h = int(h)
        out.append((h, counts[h] // block))
        counts[h] += 1
    return out


def grown_blocks(have: int, need: int) -> int:
    """Blocks per head after growing a slab of ``have`` to hold ``need``: doubled until it fits (whole blocks, geometric)."""
    cap = max(int(have), 1)
    while cap < need:
        cap *= 2
    return cap


def bootstrap_draws(seed: int, g: int, nb: int, R: int) -> np.ndarray:
    """int32 [R, nb]: resample rho of head g adds the blocks draws[rho, 0], draws[rho, 1], ... in that order"""
    return np.random.RandomState(int(seed) + SUBJECT_SEED_STRIDE * int(g)).randint(0, nb, size=(R, nb)).astype(np.int32)


def bh_q(p: np.ndarray) -> np.ndarray:
    """Benjamini-Hochberg q-values of a vector of p-values: q_(i) = min_{j >= i} p_(j) m / j, at most 1 (ties keep their order)"""
    p = np.asarray(p, np.float64)
    m = p.size
    if m == 0:
        return p.copy()
    order = np.argsort(p, kind="stable")
    scaled = p[order] * m / np.arange(1, m + 1)
    q = np.minimum(np.minimum.accumulate(scaled[::-1])[::-1], 1.0)
    out = np.empty(m, np.float64)
    out[order] = q
    return out


class TargetScores:
    """``add(pred, y, subject)`` for every batch of a split in dataset order, then ``finish`` and ``write``.

    num_target: V.  subjects: the module's subject names (one ridge head each) or None.  keep_mask: bool / number [H,V] or [V]
    (``VLBLitModule.target_weight_mask()``), a target counts where it is positive; None: all.  block: contiguous clips per
    bootstrap block.  The slab of sums is fp64 [H * cap, 5, V] with H = max(1, G) and cap blocks per head: 40 V bytes per
    (head, block), grown geometrically by copy."""

    def __init__(self, num_target, subjects=None, keep_mask=None, block=128, device=None, save_predictions=False):
        self.V = int(num_target)
        self.subjects = None if subjects is None else [str(s) for s in subjects]
        self.G = 0 if self.subjects is None else len(self.subjects)
        self.H = max(1, self.G)
        self.block = check_score_block(block)
        self.dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("TargetScores needs a GPU device (no CPU fallback)")
        self.kept = np.ones((self.H, self.V), bool)
        self.keep = None
        if keep_mask is not None:
            k = torch.as_tensor(keep_mask).detach().cpu().reshape(-1, self.V)
            if k.shape[0] not in (1, self.H):
                raise ValueError(f"TargetScores: keep_mask has {k.shape[0]} rows for {self.H} head(s)")
            self.kept = (k > 0).expand(self.H, self.V).numpy().copy()
            self.keep = torch.from_numpy(self.kept.astype(np.float32)).to(self.dev).contiguous()
        self.cap = FIRST_BLOCKS
        self.sums = torch.zeros(self.H * self.cap, 5, self.V, dtype=torch.float64, device=self.dev)
        self.counts = [0] * self.H                   # clips seen per head
        self.n_j = [[] for _ in range(self.H)]       # clips per block, per head
        self.save_predictions = bool(save_predictions)
        self._pred, self._index, self._subject = [], [], []
        self.result = None

    # ------------------------------------------------------------------ accumulation
    def _grow(self, need: int) -> None:
        cap = grown_blocks(self.cap, need)
        if cap == self.cap:
            return
        new = torch.zeros(self.H * cap, 5, self.V, dtype=torch.float64, device=self.dev)
        new.view(self.H, cap, 5, self.V)[:, :self.cap].copy_(self.sums.view(self.H, self.cap, 5, self.V))
        self.sums, self.cap = new, cap

    def add(self, pred, y, subject=None, index=None) -> None:
        """pred, y: fp32 device tensors [B,V] (rows may be pitched; the last axis is contiguous); subject: one head index per
        clip (host ints or a CPU tensor) with ``subjects``, else None.  Clips arrive in dataset order."""
        from ._lib import check, lib
        from .ops import _stream
        for name, t in (("pred", pred), ("y", y)):
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == self.V
                    and t.stride(1) == 1 and t.stride(0) >= self.V):
                raise ValueError(f"TargetScores.add: {name} must be an fp32 device tensor [B, {self.V}] with a contiguous last axis")
        B = pred.shape[0]
        if y.shape[0] != B or B < 1:
            raise ValueError(f"TargetScores.add: pred has {B} clips, y {y.shape[0]}")
        if (subject is None) != (self.G == 0):
            raise ValueError(f"TargetScores.add: subjects={self.subjects!r} but subject is {'missing' if subject is None else 'given'}")
        heads = [0] * B
        if subject is not None:
            idx = torch.as_tensor(subject).detach().cpu().flatten()
            if idx.numel() != B or idx.is_floating_point() or idx.dtype == torch.bool:
                raise ValueError(f"TargetScores.add: subject has {idx.numel()} entries of {idx.dtype} for {B} clips")
            heads = idx.to(torch.int64).tolist()
            if min(heads) < 0 or max(heads) >= self.G:
                raise ValueError(f"TargetScores.add: subject={heads!r} has an index outside [0, {self.G})")
        where = clip_blocks(self.counts, heads, self.block)
        self._grow(max(j for _, j in where) + 1)
        for h, j in where:
            if j == len(self.n_j[h]):
                self.n_j[h].append(0)
            self.n_j[h][j] += 1
        slot = [h * self.cap + j for h, j in where]
        n_slots = self.H * self.cap
        if min(slot) < 0 or max(slot) >= n_slots:          # checked on the host before upload, as BrainHead._group does
            raise RuntimeError(f"TargetScores.add: slot {slot!r} outside [0, {n_slots})")
        slot_d = torch.tensor(slot, dtype=torch.int32).to(self.dev)
        check(lib.vlb_score_accumulate(pred.data_ptr(), pred.stride(0), y.data_ptr(), y.stride(0), slot_d.data_ptr(),
                                       None if self.keep is None else self.keep.data_ptr(), self.sums.data_ptr(), B, self.V,
                                       self.cap, n_slots, _stream()), "vlb_score_accumulate")
        if self.save_predictions:
            first = sum(self.counts) - B
            self._pred.append(pred.detach().cpu().clone())
            self._index += list(range(first, first + B)) if index is None else [int(i) for i in torch.as_tensor(index).flatten().tolist()]
            self._subject += heads
        self.result = None

    # ------------------------------------------------------------------ scores
    def finish(self, bootstrap: int = 0, seed: int = 0) -> dict:
        """-> dict of host numpy arrays [H,V]: r, r2, mse, n, boot_mean, boot_se, p, q (the last four NaN without bootstrap),
        plus kept [H,V], subjects, block, blocks [H], avg [H,3] (mean r, R^2, mse over the kept targets) and bootstrap / seed."""
        from ._lib import check, lib
        from .ops import _stream
        R = check_score_bootstrap(bootstrap)
        H, V = self.H, self.V
        res = {k: np.full((H, V), np.nan) for k in ("r", "r2", "mse", "boot_mean", "boot_se", "p", "q")}
        res["n"] = np.zeros((H, V))
        avg = np.full((H, 3), np.nan)
        slab = self.sums.view(H, self.cap, 5, V)
        out = torch.empty(4, V, dtype=torch.float64, device=self.dev)
        avg_d = torch.empty(3, dtype=torch.float64, device=self.dev)
        boot = torch.empty(3, V, dtype=torch.float64, device=self.dev)
        for g in range(H):
            nb = len(self.n_j[g])
            if nb == 0:
                continue                        # a head without clips: NaN rows, n = 0
            sums_h = slab[g, :nb]               # contiguous: the head's blocks are adjacent in the slab
            n_j = torch.tensor(self.n_j[g], dtype=torch.float64).to(self.dev)
            keep_h = None if self.keep is None else self.keep[g]
            kp = None if keep_h is None else keep_h.data_ptr()
            check(lib.vlb_score_finish(sums_h.data_ptr(), n_j.data_ptr(), nb, kp, out.data_ptr(), avg_d.data_ptr(), V, _stream()),
                  "vlb_score_finish")
            o = out.cpu().numpy()
            res["r"][g], res["r2"][g], res["mse"][g], res["n"][g] = o[0], o[1], o[2], o[3]
            avg[g] = avg_d.cpu().numpy()
            if R:
                if nb == 1:
                    who = "" if self.subjects is None else f" of subject {self.subjects[g]!r}"
                    warnings.warn(f"TargetScores.finish: the {self.counts[g]} clips{who} fit in one block of {self.block}: the "
                                  "block length leaves nothing to resample, the bootstrap error is 0 (choose a smaller score_block)")
                draws = bootstrap_draws(seed, g, nb, R)
                if draws.min() < 0 or draws.max() >= nb:        # range-checked on the host before upload
                    raise RuntimeError(f"TargetScores.finish: a draw outside [0, {nb})")
                draws_d = torch.from_numpy(draws).to(self.dev)
                check(lib.vlb_score_bootstrap(sums_h.data_ptr(), n_j.data_ptr(), nb, draws_d.data_ptr(), R, kp, boot.data_ptr(), V,
                                              _stream()), "vlb_score_bootstrap")
                b = boot.cpu().numpy()
                res["boot_mean"][g], res["boot_se"][g], res["p"][g] = b[0], b[1], b[2]
                k = self.kept[g]
                res["q"][g, k] = bh_q(b[2][k])
        res.update(kept=self.kept.copy(), subjects=np.array(self.subjects or [], dtype=str), block=np.int64(self.block),
                   blocks=np.array([len(x) for x in self.n_j], np.int64), avg=avg, bootstrap=np.int64(R), seed=np.int64(seed))
        self.result = res
        return res

    def write(self, path: str) -> str:
        """``np.savez`` of ``finish``'s dict (run first); with ``save_predictions`` also ``pred`` fp32 [N,V] and ``index`` /
        ``subject`` [N] in the order the clips arrived (dataset order)."""
        import os
        if self.result is None:
            raise RuntimeError("TargetScores.write: call finish() first")
        extra = {}
        if self.save_predictions:
            extra = dict(pred=(torch.cat(self._pred).numpy() if self._pred else np.zeros((0, self.V), np.float32)),
                         index=np.array(self._index, np.int64), subject=np.array(self._subject, np.int64))
        path = str(path)
        if not path.endswith(".npz"):
            path += ".npz"
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        np.savez(path, **self.result, **extra)
        return path
