"""Per-group learning rates and weight decay (``litmodule.config.optimizer_groups``): the host side.

Pure functions, none of which needs a GPU or a torch device:

* ``normalize_optimizer_groups``  - the configuration value -> plain Python, validated as far as that needs no model;
* ``assign_groups``               - trainable names -> group index (``fnmatch`` patterns, first match wins, group 0 =
                                    everything no entry takes), with the typo guard;
* ``group_specs``                 - every group's initial ``lr`` / ``weight_decay`` from the configured pair;
* ``group_ranges``                - a flat store's layout + that assignment -> the ``(bounds, group_of)`` range table the
                                    grouped AdamW kernel searches (``vlb_adamw_step_groups``), in the coordinates of the buffer
                                    the kernel is handed: the full store, or a rank's concatenated 1/world slices.
"""
from __future__ import annotations

import math
from collections.abc import Mapping, Sequence
from fnmatch import fnmatchcase

import torch

MAX_GROUPS = 8          # the default group included: the kernel argument carries 8 (lr, weight_decay) pairs


def _number(x):
    return isinstance(x, (int, float)) and not isinstance(x, bool)


def normalize_optimizer_groups(value):
    """``None`` or a list of 1..7 ``{params: [glob, ...], lr_scale: float = 1.0, weight_decay: float | None = None}``
    (an OmegaConf list / dict is accepted) -> ``None`` or a list of plain dicts with exactly these three keys."""
    if value is None:
        return None
    if isinstance(value, (str, bytes, Mapping)) or not isinstance(value, Sequence):
        raise ValueError(f"optimizer_groups={value!r}: a list of {{params: [...], lr_scale: ..., weight_decay: ...}} entries is needed")
    entries = list(value)
    if not 1 <= len(entries) <= MAX_GROUPS - 1:
        raise ValueError(f"optimizer_groups has {len(entries)} entries: 1 to {MAX_GROUPS - 1} are supported ({MAX_GROUPS} groups with "
                         "the default one that takes every tensor no entry matches)")
    out = []
    for i, e in enumerate(entries):
        if not isinstance(e, Mapping):
            raise ValueError(f"optimizer_groups[{i}]={e!r}: a mapping with 'params' (and optionally 'lr_scale', 'weight_decay') is needed")
        e = dict(e)
        for k in [k for k, v in e.items() if v is None and isinstance(k, str) and k.split(":", 1)[0] in ("lr_scale", "weight_decay")
                  and ":" in k]:
            # Hydra's compact `{lr_scale:10}` read by a YAML parser (config.load_config) is the key "lr_scale:10" without a value
            import yaml
            del e[k]
            e[k.split(":", 1)[0]] = yaml.safe_load(k.split(":", 1)[1])
        unknown = sorted(set(e) - {"params", "lr_scale", "weight_decay"})
        if unknown:
            raise ValueError(f"optimizer_groups[{i}]: unknown key(s) {unknown}; the keys are 'params', 'lr_scale' and 'weight_decay'")
        params = e.get("params")
        if isinstance(params, (str, bytes)) or not isinstance(params, Sequence) or len(params) == 0 or \
                not all(isinstance(p, str) and p for p in params):
            raise ValueError(f"optimizer_groups[{i}].params={params!r}: a non-empty list of name patterns is needed")
        scale = e.get("lr_scale", 1.0)
        if not _number(scale) or not (math.isfinite(scale) and scale > 0):
            raise ValueError(f"optimizer_groups[{i}].lr_scale={scale!r}: a finite number > 0 is needed")
        wd = e.get("weight_decay")
        if wd is not None and (not _number(wd) or not (math.isfinite(wd) and wd >= 0)):
            raise ValueError(f"optimizer_groups[{i}].weight_decay={wd!r}: None (config.weight_decay) or a finite number >= 0 is needed")
        out.append({"params": [str(p) for p in params], "lr_scale": float(scale), "weight_decay": None if wd is None else float(wd)})
    return out


def assign_groups(names, entries) -> dict:
    """name -> group index for every name in ``names``: entry k (0-based) of ``entries`` is group k + 1, the first entry with
    a matching pattern takes the tensor, a tensor no entry matches is in group 0.  An entry that takes no tensor - it matches
    nothing, or only what earlier entries already took - is refused: that is a typo, not a choice."""
    names = list(names)
    entries = entries or []
    out, taken, matched = {}, [0] * len(entries), [0] * len(entries)
    for n in names:
        grp = 0
        for k, e in enumerate(entries):
            if any(fnmatchcase(n, pat) for pat in e["params"]):
                matched[k] += 1
                if grp == 0:
                    grp = k + 1
                    taken[k] += 1
        out[n] = grp
    for k, e in enumerate(entries):
        if not taken[k]:
            shown = ", ".join(names[:4] + (["..."] if len(names) > 8 else []) + names[max(4, len(names) - 4):])
            why = "matches no trainable tensor" if not matched[k] else "matches only tensors that earlier entries already took"
            raise ValueError(f"optimizer_groups[{k}] (params={e['params']!r}) {why}.  The trainable names are: {shown}")
    return out


def group_specs(entries, lr: float, weight_decay: float) -> list:
    """``[{"name", "lr", "weight_decay"}]`` for group 0 (the configured ``lr`` / ``weight_decay``) and one per entry:
    ``lr * lr_scale`` and the entry's own ``weight_decay`` (None: the configured one)."""
    specs = [{"name": "default", "lr": lr, "weight_decay": weight_decay}]
    for e in entries or []:
        specs.append({"name": ",".join(e["params"]), "lr": lr * e["lr_scale"],
                      "weight_decay": weight_decay if e["weight_decay"] is None else e["weight_decay"]})
    return specs


def group_ranges(offsets: Mapping, numel: int, group_of_name: Mapping, shard=None):
    """The range table of one flat store.

    ``offsets``: name -> (offset, numel, ...) as ``FlatTrainables.offsets`` / ``FlatBackbone.offsets``; ``numel``: the store's
    padded size; ``group_of_name``: name -> group (every name of ``offsets``).  ``shard``: None for the full store, else
    ``(segments, shard_off, world, rank)`` as ``parallel.ShardedFlatState`` computes them - the table then describes this
    rank's buffer, the concatenation of its 1/world slice of every segment.

    -> ``bounds`` (int64 [R + 1], ascending, ``bounds[0] = 0``, ``bounds[-1]`` = the buffer's size, all multiples of 8) and
    ``group_of`` (int32 [R]); range r is ``[bounds[r], bounds[r + 1])``.  The padding behind a tensor belongs to that tensor's
    range (its master, gradient and moments are zero and stay zero under any rate); adjacent ranges of one group are merged."""
    order = sorted(offsets, key=lambda n: offsets[n][0])
    if not order or offsets[order[0]][0] != 0:
        raise ValueError("group_ranges: the store's first tensor must start at offset 0")
    starts = [int(offsets[n][0]) for n in order] + [int(numel)]
    groups = [int(group_of_name[n]) for n in order]
    for i, n in enumerate(order):
        assert starts[i] % 8 == 0 and starts[i] + int(offsets[n][1]) <= starts[i + 1], f"{n}: tensors must be 8-aligned and disjoint"
    assert numel % 8 == 0
    if shard is None:
        pieces = [(0, int(numel), 0)]                     # (start, end) in the store -> start in the buffer
    else:
        segments, shard_off, world, rank = shard
        pieces = []
        for (s, e), off in zip(segments, shard_off):
            assert (e - s) % (8 * world) == 0, f"segment [{s}, {e}) does not split into {world} slices of whole 8-element units"
            n = (e - s) // world
            pieces.append((s + rank * n, s + (rank + 1) * n, int(off)))
    bounds, group_of, pos, ti = [0], [], 0, 0
    for a, b, off in pieces:
        assert off == pos, "the slices must be laid out back to back"
        while ti > 0 and starts[ti] > a:                   # (segments are in store order; be safe if not)
            ti -= 1
        while starts[ti + 1] <= a:
            ti += 1
        x = a
        while x < b:
            y = min(b, starts[ti + 1])
            if group_of and group_of[-1] == groups[ti]:
                bounds[-1] = pos + (y - x)
            else:
                group_of.append(groups[ti])
                bounds.append(pos + (y - x))
            pos += y - x
            x = y
            if x < b:
                ti += 1
    assert all(v % 8 == 0 for v in bounds) and all(p < q for p, q in zip(bounds, bounds[1:]))
    return torch.tensor(bounds, dtype=torch.int64), torch.tensor(group_of, dtype=torch.int32)
