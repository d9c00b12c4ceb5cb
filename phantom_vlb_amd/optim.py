"""AdamW on libvlb (vlb_adamw_step) behind the torch.optim.Optimizer interface.

Mirrors ``torch.optim.AdamW(lr, betas, eps, weight_decay)`` as the reference configures it
(src/litmodule/videollama2_vlb_litmodule.py:357-363) so ``CosineAnnealingLR`` and a Lightning
Trainer can drive it unchanged.  Differences, documented in DESIGN.md: the update runs on fp32
masters with fp32 moments (the reference updates bf16 params in place), the global-norm clip of
``Trainer(gradient_clip_val=1)`` is fused into the same kernel (device-side norm, no host sync),
and the bf16 compute copies read by the kernels are refreshed in the same launch.

All state lives in the flat buffers of ``flat.FlatTrainables``: one sum-of-squares launch and one
clip+AdamW launch per step.  Under data parallelism ``parallel.ShardedFlatState`` is attached and
the same two launches run on this rank's 1/world slice between a gradient reduce-scatter and an
all-gather of the refreshed bf16 copies.

Gradient accumulation (``accumulate_grad_batches = k > 1``): every ``training_step`` still overwrites the stores' gradient
buffers, and ``accumulate(index_in_window, is_last)`` adds them into one fp32 accumulator per store (``vlb_grad_accum`` /
``vlb_grad_accum_bf16``; allocated on first use, never at k = 1).  The ``step()`` that closes the window reads the
accumulators instead of the gradient buffers; the accumulators are not part of ``state_dict()`` (a checkpoint is taken on a
window boundary).

Parameter groups (``litmodule.config.optimizer_groups``): with ``groups`` the optimiser has one torch
``param_groups`` entry per non-empty group, each with its own ``lr`` / ``weight_decay`` (schedulers and learning-rate monitors
see them like any torch optimiser's), every store gets a range table (``optim_groups.group_ranges``; rebuilt for a rank's slices
when data parallelism is attached) and the step makes one ``vlb_adamw_step_groups`` / ``_g16`` launch per store.  Without
``groups`` nothing of this exists: one group, no table, the two launches above.

Weight averaging (``litmodule.config.ema_decay``): with ``ema_decay`` the optimiser owns one more flat fp32 buffer,
``ema``, an exponential moving average of store 0's masters.  The AdamW launch of the step is then ``vlb_adamw_step_ema`` (or
``vlb_adamw_step_groups_ema``), which updates the average in the same pass with the decay ``ema_decay_at`` gives for this
update; master, moments and bf16 copies come out bit-identical to the plain launch.  Without ``ema_decay`` there is no buffer
and the launches above are the ones made.
"""
from __future__ import annotations

import ctypes

import torch

from ._lib import check, lib
from .optim_groups import MAX_GROUPS, group_ranges
from .ops import _stream


def ema_decay_at(t: int, decay: float, warmup: bool = True) -> float:
    """Decay of the t-th EMA update (t = 1, 2, ...): ``decay``, or with ``warmup`` ``min(decay, (1 + t) / (10 + t))`` - the
    usual warm-up (2/11, 3/12, ... up to the cap), so that the average is not dominated by the initial weights."""
    if t < 1:
        raise ValueError(f"ema_decay_at: updates count from 1 (got t={t})")
    return min(float(decay), (1 + t) / (10 + t)) if warmup else float(decay)


FULLFT_EMA_MESSAGE = ("ema_decay with the full fine-tune (freeze_backbone=False, use_lora=False) is not supported: the backbone's "
                      "bf16-gradient store has no EMA kernel, and an fp32 average of 7B weights costs 28 GB.  Average a LoRA or "
                      "frozen-backbone run (use_lora=True or freeze_backbone=True), or leave ema_decay unset")


class VlbAdamW(torch.optim.Optimizer):
    """``flat``: one flat store or a list of them (head + LoRA: fp32 gradients; ``fullft.FlatBackbone``: bf16
    gradients, attribute ``grad_bf16``).  One clip norm over all of them, one AdamW launch per store.

    ``groups``: None (one group: ``lr`` / ``weight_decay`` for everything), or ``(assignment, specs)`` - ``assignment`` maps
    every parameter name to an index into ``specs``, a list of ``{"name", "lr", "weight_decay"}`` (index 0: the default
    group).  Groups no parameter is assigned to are dropped; the rest become ``param_groups`` in that order.

    ``ema_decay``: None, or the decay of the moving average of store 0's masters kept in ``ema`` (``ema_warmup``: see
    ``ema_decay_at``); one update per ``step()``, ``ema_updates`` counts them."""

    def __init__(self, named_params, flat, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 max_norm: float = 0.0, groups=None, ema_decay: float | None = None, ema_warmup: bool = True):
        named_params = list(named_params)
        self.names = [n for n, _ in named_params]
        self.named_params = named_params
        params = [p for _, p in named_params]
        for p in params:
            assert p.dtype == torch.float32 and p.is_cuda and p.is_contiguous()
        self.group_names = ["default"]
        self.group_of_name = None     # name -> index into param_groups; None: one group, no table, the ungrouped kernels
        if groups is not None:
            assignment, specs = groups
            used = sorted({int(assignment[n]) for n in self.names})
            if len(used) > MAX_GROUPS:
                raise ValueError(f"{len(used)} optimiser groups: at most {MAX_GROUPS} are supported")
            if len(used) > 1:
                self.group_of_name = {n: used.index(int(assignment[n])) for n in self.names}
                self.group_names = [str(specs[k]["name"]) for k in used]
                params = [dict(params=[p for n, p in named_params if self.group_of_name[n] == i], lr=float(specs[k]["lr"]),
                               weight_decay=float(specs[k]["weight_decay"])) for i, k in enumerate(used)]      # one dict per group
            elif used:                # everything in one group: that group's rates, the parent's path
                lr, weight_decay = float(specs[used[0]]["lr"]), float(specs[used[0]]["weight_decay"])
                self.group_names = [str(specs[used[0]]["name"])]
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.max_norm = float(max_norm)
        self.flats = list(flat) if isinstance(flat, (list, tuple)) else [flat]
        self.flat = self.flats[0]         # head (+ LoRA) store
        self.shardeds = [None] * len(self.flats)      # parallel.ShardedFlatState per store under data parallelism
        dev = named_params[0][1].device
        self.sumsq = torch.zeros(1, dtype=torch.float32, device=dev)
        self.sumsq_ws = torch.zeros(max(lib.vlb_sumsq_ws_floats(), 1024), dtype=torch.float32, device=dev)
        self.step_count = 0
        self.post_step = []           # callables run after every update (e.g. LoRA derived layouts, W^T refresh)
        self.accum = [None] * len(self.flats)         # fp32 accumulator per store: allocated by the first accumulate() only
        self._acc_live = False        # accumulate() ran since the last step(): step() consumes the accumulators
        self._acc_sumsq = False       # ... and the last accumulate() left the clip norm's sum of squares in self.sumsq
        self._acc_pos = None          # (index_in_window, is_last) announced by begin_micro_batch (data parallelism)
        self.tables = None            # groups only: per store (bounds int64, group_of int32) on the device, built and uploaded once
        if self.group_of_name is not None:
            self.tables = [self._range_table(i) for i in range(len(self.flats))]
            self._lr_arg = (ctypes.c_float * MAX_GROUPS)()
            self._wd_arg = (ctypes.c_float * MAX_GROUPS)()
        self.ema = None               # ema_decay only: flat fp32 moving average of store 0's masters, same element order
        self.ema_decay, self.ema_warmup = ema_decay, bool(ema_warmup)
        self.ema_updates = 0          # EMA updates so far (the warm-up's t)
        self.ema_last_decay = None    # decay the last update used
        if ema_decay is not None:
            if len(self.flats) > 1 or getattr(self.flat, "grad_bf16", False):
                raise ValueError(FULLFT_EMA_MESSAGE)
            self.ema = self.flat.master.detach().clone()

    def _range_table(self, i: int):
        """Store i's range table in the coordinates of the buffer its AdamW launch is handed: the flat store, or (data
        parallelism) this rank's concatenated 1/world slices.  Built on the host, uploaded once."""
        f, sh = self.flats[i], self._active(i)
        prefix = "backbone." if i >= 1 else ""             # the backbone store's own names lack the prefix
        assign = {n: self.group_of_name[prefix + n] for n in f.offsets}
        shard = (sh.segments, sh.shard_off, sh.world, sh.rank) if sh is not None else None
        bounds, group_of = group_ranges(f.offsets, f.numel, assign, shard)
        assert int(bounds[-1]) == (sh.numel if sh is not None else f.numel)
        dev = f.compute.device
        return bounds.to(dev), group_of.to(dev)

    @property
    def sharded(self):
        return self.shardeds[0]

    def attach_sharded(self, state):
        """Data parallelism: gradients are reduce-scattered, this rank updates its 1/world slice of every segment
        and the bf16 copies are all-gathered (parallel.ShardedFlatState); one state per flat store."""
        i = [k for k, f in enumerate(self.flats) if f is state.flat]
        assert i, "attach_sharded: the state wraps a flat store this optimiser does not own"
        if self.ema is not None:
            raise ValueError("ema_decay under data parallelism (WORLD_SIZE > 1) is not supported: every rank updates a 1/world slice "
                             "of the optimiser state, and the moving average would need a slice of its own, which is not built.  "
                             "Run one process, or leave ema_decay unset")
        self.shardeds[i[0]] = state
        if self.tables is not None:
            self.tables[i[0]] = self._range_table(i[0])

    def full_state(self, name: str, index: int = 0):
        """Full-size flat fp32 buffer 'master' | 'm' | 'v' of store `index` (gathered from the shards under data parallelism)."""
        sh = self.shardeds[index]
        return sh.gather_full(name) if sh is not None else getattr(self.flats[index], name)

    def load_full_state(self, name: str, full, index: int = 0):
        f, sh = self.flats[index], self.shardeds[index]
        full = full.to(f.compute.device)
        if sh is not None:
            sh.load_full(name, full)
            if name == "master" and f.master is not None:       # (None: FULL_SHARD keeps no full-size staging copy)
                f.master.copy_(full)
        else:
            getattr(f, name).copy_(full)

    def compute_from_master(self, index: int):
        """bf16 weights of store `index` <- its restored fp32 masters (checkpoint resume)."""
        f, sh = self.flats[index], self.shardeds[index]
        if sh is not None:
            sh.compute_from_master()
        else:
            chunk = 1 << 28
            for a in range(0, f.numel, chunk):
                f.compute[a:a + chunk].copy_(f.master[a:a + chunk])

    def reset_moments(self, names):
        """Zero both Adam moments of the named tensors of the head (+ LoRA) store - after their masters were set by something
        other than an AdamW step (the closed-form ridge fit): the history of the values they replaced says
        nothing about the new ones.  The bias-correction step count is left alone.  Single process only."""
        f = self.flats[0]
        if self.shardeds[0] is not None and self.shardeds[0].active:
            raise RuntimeError("VlbAdamW.reset_moments: the moments are sharded over ranks (data parallelism); not supported")
        for n in names:
            if n not in f.offsets:
                raise KeyError(f"VlbAdamW.reset_moments: {n!r} is not a tensor of the flat store ({sorted(f.offsets)[:6]} ...)")
            o, k, _ = f.offsets[n]
            f.m[o:o + k].zero_()
            f.v[o:o + k].zero_()

    def reset_ema(self, names):
        """EMA of the named tensors of the head (+ LoRA) store <- their masters (``reset_moments``' sibling: the average of
        the values the closed-form ridge fit replaced says nothing about the new ones).  Nothing without ``ema_decay``."""
        if self.ema is None:
            return
        f = self.flats[0]
        for n in names:
            if n not in f.offsets:
                raise KeyError(f"VlbAdamW.reset_ema: {n!r} is not a tensor of the flat store ({sorted(f.offsets)[:6]} ...)")
            o, k, _ = f.offsets[n]
            self.ema[o:o + k].copy_(f.master[o:o + k])

    def load_ema(self, ema=None, updates: int = 0):
        """Checkpoint resume with ``ema_decay``: the saved average and its update count - or, from a checkpoint without them,
        a fresh average of the (already restored) masters: starting to average late is a legitimate use."""
        if self.ema is None:
            return
        if ema is None:
            self.ema.copy_(self.flat.master)
            self.ema_updates = 0
        else:
            if ema.numel() != self.ema.numel():
                raise ValueError(f"the checkpoint's ema holds {ema.numel()} elements, this optimiser's flat store {self.ema.numel()}")
            self.ema.copy_(ema.to(self.ema.device, torch.float32))
            self.ema_updates = int(updates)

    # ------------------------------------------------------------------ checkpoint surface (torch.optim.Optimizer)
    def state_dict(self):
        """``torch.optim`` layout (``state`` / ``param_groups``) plus ``vlb``: the bias-correction step count and, per flat
        store, both fp32 Adam moments (gathered under data parallelism) - and for the stores whose weights are NOT in the
        module's ``state_dict()`` (index >= 1: the full fine-tune's backbone in kernel layouts) the fp32 masters too.  This
        is what a Lightning ``ModelCheckpoint`` stores under ``optimizer_states``; the built-in runner's own checkpoint
        (trainer.trainable_state) carries the same tensors."""
        sd = super().state_dict()
        stores = []
        for i in range(len(self.flats)):
            st = {"m": self.full_state("m", i).detach().cpu().clone(), "v": self.full_state("v", i).detach().cpu().clone()}
            if i >= 1:
                st["master"] = self.full_state("master", i).detach().cpu().clone()
            stores.append(st)
        sd["vlb"] = {"step_count": self.step_count, "stores": stores}
        if self.ema is not None:
            sd["vlb"].update(ema=self.ema.detach().cpu().clone(), ema_updates=self.ema_updates)
        return sd

    def load_state_dict(self, state_dict):
        state_dict = dict(state_dict)
        vlb = state_dict.pop("vlb", None)
        super().load_state_dict(state_dict)
        if vlb is None:
            raise KeyError("VlbAdamW.load_state_dict: no 'vlb' entry (moments / step count) - not a checkpoint of this optimiser")
        if len(vlb["stores"]) != len(self.flats):
            raise ValueError(f"checkpoint holds {len(vlb['stores'])} flat stores, this optimiser {len(self.flats)}")
        self.step_count = int(vlb["step_count"])
        for i, st in enumerate(vlb["stores"]):
            f = self.flats[i]
            if i == 0:
                self.load_full_state("master", f.master, 0)       # the module's load_state_dict restored the masters
            else:
                self.load_full_state("master", st["master"], i)
                self.compute_from_master(i)
            self.load_full_state("m", st["m"], i)
            self.load_full_state("v", st["v"], i)
        self.load_ema(vlb.get("ema"), vlb.get("ema_updates", 0))
        for fn in self.post_step:
            fn()                      # derived layouts (LoRA A^T / B pads, W^T copies) from the restored weights

    # ------------------------------------------------------------------ gradient accumulation (accumulate_grad_batches > 1)
    def _active(self, i: int):
        """Store i's ShardedFlatState when it runs collectives (at world 1 its buffers ARE the flat buffers), else None."""
        sh = self.shardeds[i]
        return sh if sh is not None and sh.active else None

    def _accumulator(self, i: int):
        if self.accum[i] is None:
            f = self.flats[i]
            if self._active(i) is not None and getattr(f, "grad_bf16", False):
                raise ValueError("accumulate_grad_batches > 1 with the full fine-tune under data parallelism is not supported (FULL_SHARD's "
                                 "two rotating layer gradient buffers, and SHARD_GRAD_OP's bf16 shards, have nowhere to accumulate): "
                                 "use accumulate_grad_batches=1 with more ranks, or LoRA / the frozen head, which do accumulate")
            self.accum[i] = torch.empty(f.numel, dtype=torch.float32, device=f.compute.device)
        return self.accum[i]

    def accumulate_range(self, i: int, start: int, end: int, first: bool, sumsq: bool = False):
        """accumulator[start:end] (+)= store i's gradient buffer [start:end]; ``sumsq``: also self.sumsq += sum(result^2)."""
        f, acc = self.flats[i], self._accumulator(i)
        bf = getattr(f, "grad_bf16", False)
        fn = lib.vlb_grad_accum_bf16 if bf else lib.vlb_grad_accum
        check(fn(acc.data_ptr() + 4 * start, f.grad.data_ptr() + (2 if bf else 4) * start, end - start, int(first),
                 self.sumsq.data_ptr() if sumsq else None, self.sumsq_ws.data_ptr() if sumsq else None, _stream()), "vlb_grad_accum")

    def begin_micro_batch(self, index_in_window: int, is_last: bool):
        """Before the backward pass of a micro-batch of an accumulation window.  Only data parallelism needs it: micro-batches
        that do not close the window start no collective (Lightning's ``no_sync``); on the closing one every segment is
        accumulated and reduce-scattered FROM THE ACCUMULATOR the moment its layers are differentiated."""
        self._acc_pos = (int(index_in_window), bool(is_last))
        for i in range(len(self.flats)):
            sh = self._active(i)
            if sh is not None:
                acc = self._accumulator(i)
                first = index_in_window == 0
                sh.defer = not is_last
                sh.accum_src = acc
                sh.accum_add = (lambda s, e, i=i, first=first: self.accumulate_range(i, s, e, first)) if is_last else None

    def accumulate(self, index_in_window: int, is_last: bool):
        """After the backward pass of micro-batch ``index_in_window`` (0-based): add the gradient buffers into the
        accumulators (``index_in_window == 0`` overwrites them: no memset).  ``is_last`` says that the next ``step()`` follows
        directly: the same pass then also computes the clip norm's sum of squares of the accumulated gradient - bit-identical
        to ``vlb_grad_sumsq`` on it - and ``step()`` runs no separate norm pass.  A window that is closed without
        ``is_last`` is still stepped correctly (``step()`` then runs that pass itself)."""
        first = index_in_window == 0
        any_active = any(self._active(i) is not None for i in range(len(self.flats)))
        if any_active and self._acc_pos != (int(index_in_window), bool(is_last)):
            raise RuntimeError("accumulate() under data parallelism needs begin_micro_batch() with the same position before the backward pass")
        fuse = bool(is_last) and self.max_norm > 0 and not any_active
        if fuse:
            self.sumsq.zero_()
        for i, f in enumerate(self.flats):
            sh = self._active(i)
            if sh is None:
                self.accumulate_range(i, 0, f.numel, first, sumsq=fuse)
            elif not is_last:
                self.accumulate_range(i, 0, f.numel, first)
            else:
                for si in range(len(sh.segments)):          # the segments backward has not handed over yet (the head's at least)
                    sh.reduce_segment(si)
        self._acc_live, self._acc_sumsq, self._acc_pos = True, fuse, None

    def window_gradient(self, index: int = 0):
        """The accumulated fp32 gradient of store ``index`` while a window is waiting for its ``step()``, else None."""
        return self.accum[index] if self._acc_live else None

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:               # Lightning's automatic optimisation: training_step + zero_grad + backward
            with torch.enable_grad():
                loss = closure()
        self.step_count += 1
        st = _stream()
        acc_live, acc_sumsq = self._acc_live, self._acc_sumsq
        self._acc_live = self._acc_sumsq = False
        for sh in self.shardeds:
            if sh is not None:
                sh.defer = False             # (a window closed without notice: its segments are reduced from the accumulator now)
                sh.finish_reduce()           # reduce-scatters started under backward + the rest
                sh.accum_src = sh.accum_add = None
        bufs = [sh if sh is not None else f for f, sh in zip(self.flats, self.shardeds)]
        # gradient the update reads: the store's buffer (a rank's reduce-scattered slice under data parallelism), or after an
        # accumulation window the fp32 accumulator - also for the full fine-tune's bf16 store
        grads = [(self.accum[i], False) if acc_live and self._active(i) is None else (b.grad, getattr(f, "grad_bf16", False))
                 for i, (f, b) in enumerate(zip(self.flats, bufs))]
        if not acc_sumsq:
            self.sumsq.zero_()
        if self.max_norm > 0:
            for b, (g, bf) in zip(bufs, grads):
                if acc_sumsq:
                    break                    # the window's last accumulate() computed it in the same pass
                fn = lib.vlb_grad_sumsq_bf16 if bf else lib.vlb_grad_sumsq
                check(fn(g.data_ptr(), b.numel, self.sumsq.data_ptr(), self.sumsq_ws.data_ptr(), st), "vlb_grad_sumsq")
            active = [sh for sh in self.shardeds if sh is not None]
            if active:
                active[0].all_reduce_scalar(self.sumsq)      # the clip norm covers every rank's slices
        for i, (b, (g, bf)) in enumerate(zip(bufs, grads)):      # one launch per store (ema_decay: there is only store 0)
            self._launch(b, g, bf, self.tables[i] if self.tables is not None else None, st)
        for sh in self.shardeds:
            if sh is not None:
                sh.gather_compute()
        for fn in self.post_step:
            fn()
        return loss

    def _launch(self, b, g, bf, table, st):
        """The clip+AdamW launch of one store.  Its entry point follows from (bf16 gradient?, range table?, EMA?):
        ``vlb_adamw_step`` [``_groups``] [``_g16`` | ``_ema``] - all six run the same kernel family (csrc/adamw.hip).  With a table
        every group's current lr / weight_decay goes by value, as does the EMA decay of this update (the kernel knows nothing
        about the warm-up); there is no bf16-gradient EMA (``__init__`` refuses it)."""
        group = self.param_groups[0]
        b1, b2 = group["betas"]
        ema = self.ema is not None
        name = "vlb_adamw_step" + ("_groups" if table is not None else "") + ("_ema" if ema else "_g16" if bf else "")
        args = [b.master.data_ptr(), b.compute.data_ptr(), g.data_ptr(), b.m.data_ptr(), b.v.data_ptr()]
        if ema:
            args.append(self.ema.data_ptr())
        args.append(b.numel)
        if table is not None:
            bounds, group_of = table
            assert int(bounds.numel()) >= 2 and b.numel % 8 == 0
            for k, pg in enumerate(self.param_groups):
                self._lr_arg[k], self._wd_arg[k] = float(pg["lr"]), float(pg["weight_decay"])
            args += [bounds.data_ptr(), group_of.data_ptr(), group_of.numel(), self._lr_arg, self._wd_arg, len(self.param_groups),
                     float(b1), float(b2), float(group["eps"])]
        else:
            args += [float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"])]
        args += [self.step_count, self.sumsq.data_ptr(), self.max_norm]
        if ema:
            d = ema_decay_at(self.ema_updates + 1, self.ema_decay, self.ema_warmup)
            args.append(d)
        check(getattr(lib, name)(*args, st), name)
        if ema:
            self.ema_updates += 1
            self.ema_last_decay = d

    def grad_norm(self) -> float:
        """Global gradient norm of the last step (host sync; for logging only)."""
        return float(self.sumsq.sqrt().item())
