"""optimizer_groups on the host: configuration checks, name -> group assignment, the range table the grouped
AdamW kernel searches - against an element-by-element brute force for full stores and for every rank's slices of both
sharded layouts - and the stock cosine scheduler over three groups.  No GPU."""
import math

import pytest
import torch

from phantom_vlb_amd.flat import SEG_ALIGN
from phantom_vlb_amd.optim_groups import MAX_GROUPS, assign_groups, group_ranges, group_specs, normalize_optimizer_groups

EXAMPLE = [{"params": ["layer_norm*", "*.bias"], "lr_scale": 10, "weight_decay": 0},
           {"params": ["ridge_layer.*", "layer_mix.weight"], "lr_scale": 10},
           {"params": ["*.lora_B.weight"], "lr_scale": 4}]
HEAD = ["layer_norm1.weight", "layer_norm1.bias", "layer_norm2.weight", "layer_norm2.bias", "ridge_layer.linear.weight",
        "ridge_layer.linear.bias"]
LORA_GROUPS = (("q_proj", "k_proj", "v_proj"), ("o_proj",), ("gate_proj", "up_proj"), ("down_proj",))


def _lora_names(layers=3):
    out = []
    for li in range(layers):
        for targets in LORA_GROUPS:
            out += [f"model.layers.{li}.{t}.lora_A.weight" for t in targets]
            out += [f"model.layers.{li}.{t}.lora_B.weight" for t in targets]
    return out


def _cfg(**kw):
    from phantom_vlb_amd.litmodule import VLBLitModuleConfig
    base = dict(model_path="none", freeze_backbone=True, use_lora=False, lora_r=None, lora_alpha=None, lora_dropout=None,
                dropout_rate=0.0, num_target=128, l2_lambda=1e-3, lr=1e-3, betas=[0.9, 0.999], eps=1e-8,
                weight_decay=1e-2, lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=50000, geometry="mini")
    base.update(kw)
    return VLBLitModuleConfig(**base)


# ------------------------------------------------------------------------------------------------ configuration
def test_config_default_and_normalisation():
    assert _cfg().optimizer_groups is None
    got = _cfg(optimizer_groups=tuple(EXAMPLE)).optimizer_groups
    assert got == [{"params": ["layer_norm*", "*.bias"], "lr_scale": 10.0, "weight_decay": 0.0},
                   {"params": ["ridge_layer.*", "layer_mix.weight"], "lr_scale": 10.0, "weight_decay": None},
                   {"params": ["*.lora_B.weight"], "lr_scale": 4.0, "weight_decay": None}]
    assert all(type(e) is dict and type(e["params"]) is list for e in got)


def test_config_value_from_the_command_line_parser():
    """The value as config.load_config's override parser (YAML) delivers it, written with and without a space after the
    colons (the compact form is Hydra's; a YAML parser reads `lr_scale:10` as one key without a value)."""
    import yaml
    spaced = yaml.safe_load('[{params: ["layer_norm*","*.bias"], lr_scale: 10, weight_decay: 0}, {params: ["*.lora_B.weight"], lr_scale: 4}]')
    compact = yaml.safe_load('[{params:["layer_norm*","*.bias"],lr_scale:10,weight_decay:0},{params:["*.lora_B.weight"],lr_scale:4}]')
    want = [{"params": ["layer_norm*", "*.bias"], "lr_scale": 10.0, "weight_decay": 0.0},
            {"params": ["*.lora_B.weight"], "lr_scale": 4.0, "weight_decay": None}]
    assert normalize_optimizer_groups(spaced) == want
    assert normalize_optimizer_groups(compact) == want


@pytest.mark.parametrize("bad", [
    [],                                                                   # no entry
    [{"params": [f"p{i}"]} for i in range(MAX_GROUPS)],                   # 8 entries: 9 groups with the default
    "layer_norm*",                                                        # not a list
    {"params": ["x"]},                                                    # a mapping instead of a list of mappings
    [["x"]],                                                              # an entry that is no mapping
    [{"params": []}],
    [{"params": "layer_norm*"}],
    [{"params": [""]}],
    [{"params": ["x"], "lr": 3.0}],                                       # unknown key
    [{"lr_scale": 2.0}],                                                  # no params
    [{"params": ["x"], "lr_scale": 0.0}],
    [{"params": ["x"], "lr_scale": -1.0}],
    [{"params": ["x"], "lr_scale": float("inf")}],
    [{"params": ["x"], "lr_scale": float("nan")}],
    [{"params": ["x"], "lr_scale": "2"}],
    [{"params": ["x"], "lr_scale": True}],
    [{"params": ["x"], "lr_scale": None}],
    [{"params": ["x"], "weight_decay": -1e-3}],
    [{"params": ["x"], "weight_decay": float("inf")}],
    [{"params": ["x"], "weight_decay": float("nan")}],
    [{"params": ["x"], "weight_decay": "0"}],
])
def test_config_refuses(bad):
    with pytest.raises(ValueError, match="optimizer_groups"):
        _cfg(optimizer_groups=bad)


def test_config_accepts_the_limits():
    assert len(_cfg(optimizer_groups=[{"params": [f"p{i}"]} for i in range(MAX_GROUPS - 1)]).optimizer_groups) == 7
    assert _cfg(optimizer_groups=[{"params": ["x"], "weight_decay": 0}]).optimizer_groups[0]["weight_decay"] == 0.0


# ------------------------------------------------------------------------------------------------ names -> groups
def test_first_match_wins_and_unmatched_names_are_group_zero():
    names = HEAD + _lora_names()
    entries = normalize_optimizer_groups(EXAMPLE)
    got = assign_groups(names, entries)
    assert set(got) == set(names)
    for n in names:
        want = 1 if n.startswith("layer_norm") or n.endswith(".bias") else 2 if n.startswith("ridge_layer.") else \
            3 if n.endswith(".lora_B.weight") else 0
        assert got[n] == want, n
    assert got["ridge_layer.linear.bias"] == 1            # matched by entries 0 and 1: the first takes it
    assert got["model.layers.2.down_proj.lora_A.weight"] == 0
    # order matters: the same patterns the other way round
    flipped = assign_groups(names, [entries[1], entries[0]])
    assert flipped["ridge_layer.linear.bias"] == 1 and flipped["layer_norm1.bias"] == 2
    # patterns are case sensitive and match the whole name
    assert assign_groups(["a.weight", "A.weight", "xa.weight"], [{"params": ["a.*"]}]) == {"a.weight": 1, "A.weight": 0, "xa.weight": 0}
    assert assign_groups(names, None) == {n: 0 for n in names}


def test_entry_matching_nothing_raises_and_shows_names():
    names = HEAD + _lora_names()
    entries = normalize_optimizer_groups([{"params": ["layer_norm*"]}, {"params": ["*.lora_C.weight", "ridge.*"]}])
    with pytest.raises(ValueError) as ei:
        assign_groups(names, entries)
    msg = str(ei.value)
    assert "optimizer_groups[1]" in msg and "lora_C" in msg and "matches no trainable" in msg
    assert "layer_norm1.weight" in msg and "lora_B.weight" in msg          # a few of the available names
    # everything an entry matches was already taken: equally dead, equally refused
    with pytest.raises(ValueError, match=r"optimizer_groups\[1\].*earlier entries"):
        assign_groups(names, normalize_optimizer_groups([{"params": ["*.bias"]}, {"params": ["ridge_layer.linear.bias"]}]))


def test_group_specs():
    specs = group_specs(normalize_optimizer_groups(EXAMPLE), 1e-4, 1e-2)
    assert [s["lr"] for s in specs] == [1e-4, 1e-4 * 10.0, 1e-4 * 10.0, 1e-4 * 4.0]
    assert [s["weight_decay"] for s in specs] == [1e-2, 0.0, 1e-2, 1e-2]
    assert specs[0]["name"] == "default" and specs[3]["name"] == "*.lora_B.weight"


# ------------------------------------------------------------------------------------------------ the range table
def _layout(entries):
    """flat.FlatTrainables' / fullft.FlatBackbone's offset rule: tensors padded to 8 elements, a segment's end to SEG_ALIGN.
    entries: [(name, numel, segment)] -> offsets, numel, head_range, layer_ranges."""
    offs, off, seg_start, head_range, layer_ranges = {}, 0, 0, None, []
    for i, (n, k, seg) in enumerate(entries):
        offs[n] = (off, k, (k,))
        off += (k + 7) // 8 * 8
        if i + 1 == len(entries) or entries[i + 1][2] != seg:
            off = (off + SEG_ALIGN - 1) // SEG_ALIGN * SEG_ALIGN
            if seg < 0:
                head_range = (seg_start, off)
            else:
                layer_ranges.append((seg_start, off))
            seg_start = off
    return offs, off, head_range, layer_ranges


def _trainables_like():
    """head + 3 layers x (A of each target, then B of each target) per LoRA group, odd sizes."""
    sizes = {"layer_norm1.weight": 61, "layer_norm1.bias": 61, "layer_norm2.weight": 61, "layer_norm2.bias": 61,
             "ridge_layer.linear.weight": 61 * 37, "ridge_layer.linear.bias": 37}
    entries = [(n, sizes[n], -1) for n in HEAD]
    for li in range(3):
        for gi, targets in enumerate(LORA_GROUPS):
            entries += [(f"model.layers.{li}.{t}.lora_A.weight", 16 * (61 + 2 * gi), li) for t in targets]
            entries += [(f"model.layers.{li}.{t}.lora_B.weight", 16 * (53 + 8 * j) + 3, li) for j, t in enumerate(targets)]
    return _layout(entries)


def _backbone_like():
    """tail (connector, embeddings, final norm) + 4 decoder layers of six tensors, as fullft.FlatBackbone orders them."""
    entries = [("mm_projector.s1.b1.conv.weight", 9 * 67, -1), ("mm_projector.s1.b1.ln.weight", 67, -1), ("mm_projector.s1.b1.ln.bias", 67, -1),
               ("mm_projector.sampler.weight", 8 * 67 * 3, -1), ("mm_projector.sampler.bias", 67, -1), ("mm_projector.ro0.weight", 67 * 67, -1),
               ("mm_projector.ro0.bias", 67, -1), ("embed_tokens", 211 * 67, -1), ("norm", 67, -1)]
    for li in range(4):
        entries += [(f"layers.{li}.{k}", n, li) for k, n in (("wqkv", 67 * 99), ("wo", 67 * 67), ("wgu", 67 * 2 * 131),
                                                            ("wdown", 131 * 67), ("in_norm", 67), ("post_norm", 67))]
    return _layout(entries)


def _segments(head_range, layer_ranges, chunks, full_shard):
    """parallel.ShardedFlatState.__init__'s cut: the head segment, then runs of whole layers."""
    segs, L = [head_range], len(layer_ranges)
    if full_shard:
        chunks = max(L, 1)
    per = max(1, -(-L // chunks)) if L else 1
    for lo in range(0, L, per):
        hi = min(lo + per, L) - 1
        segs.append((layer_ranges[lo][0], layer_ranges[hi][1]))
    return segs


def _brute_force(offs, numel, group_of_name):
    """element -> group for the full store: a tensor's elements and the padding behind it are the tensor's group."""
    elem = torch.full((numel,), -1, dtype=torch.int32)
    order = sorted(offs, key=lambda n: offs[n][0])
    for n, nxt in zip(order, order[1:] + [None]):
        elem[offs[n][0]:(offs[nxt][0] if nxt is not None else numel)] = group_of_name[n]
    assert int(elem.min()) >= 0
    return elem


def _expand(bounds, group_of):
    assert bounds.dtype == torch.int64 and group_of.dtype == torch.int32 and bounds.numel() == group_of.numel() + 1
    return torch.repeat_interleave(group_of, bounds[1:] - bounds[:-1])


def _check_table(bounds, group_of, want):
    b = bounds.tolist()
    assert b[0] == 0 and b[-1] == want.numel()
    assert all(x % 8 == 0 for x in b) and all(x < y for x, y in zip(b, b[1:]))            # ascending multiples of 8
    g = group_of.tolist()
    assert all(x != y for x, y in zip(g, g[1:]))                                          # adjacent ranges were merged
    assert torch.equal(_expand(bounds, group_of), want)


STORES = {
    "trainables": (_trainables_like, "", normalize_optimizer_groups(EXAMPLE)),
    "backbone": (_backbone_like, "backbone.", normalize_optimizer_groups(
        [{"params": ["backbone.mm_projector.*"], "lr_scale": 0.1}, {"params": ["backbone.*norm"], "weight_decay": 0},
         {"params": ["backbone.layers.3.wqkv", "backbone.layers.1.w*"], "lr_scale": 2}])),
}


@pytest.mark.parametrize("store", sorted(STORES))
def test_range_table_full_store_and_every_shard(store):
    make, prefix, entries = STORES[store]
    offs, numel, head_range, layer_ranges = make()
    by_name = assign_groups([prefix + n for n in offs], entries)         # (the backbone store's own names lack the prefix)
    assign = {n: by_name[prefix + n] for n in offs}
    assert len(set(assign.values())) == 4
    elem = _brute_force(offs, numel, assign)
    bounds, group_of = group_ranges(offs, numel, assign)
    _check_table(bounds, group_of, elem)
    assert group_of.numel() > 8                                      # (the layouts alternate groups: a real table)
    for world in (1, 2, 3, 4, 8):
        for chunks, full_shard in ((2, False), (4, True)):           # head + layer chunks; one segment per layer (FULL_SHARD)
            segs = _segments(head_range, layer_ranges, chunks, full_shard)
            assert len(segs) == (1 + len(layer_ranges) if full_shard else 3)
            shard_off, off = [], 0
            for s, e in segs:
                shard_off.append(off)
                off += (e - s) // world
            assert off * world == numel
            for rank in range(world):
                want = torch.cat([elem[s + rank * ((e - s) // world):s + (rank + 1) * ((e - s) // world)] for s, e in segs])
                bounds, group_of = group_ranges(offs, numel, assign, (segs, shard_off, world, rank))
                _check_table(bounds, group_of, want)
    # world 1 describes the same buffer as no shard description at all
    one = group_ranges(offs, numel, assign, (segs, [s for s, _ in segs], 1, 0))
    full = group_ranges(offs, numel, assign)
    assert torch.equal(one[0], full[0]) and torch.equal(one[1], full[1])


def test_range_table_one_group_and_padding():
    offs, numel, _, _ = _trainables_like()
    bounds, group_of = group_ranges(offs, numel, {n: 5 for n in offs})
    assert bounds.tolist() == [0, numel] and group_of.tolist() == [5]
    # the padding behind the last head tensor (to SEG_ALIGN) goes with that tensor, not with the next segment's first
    assign = {n: (1 if n == "ridge_layer.linear.bias" else 0) for n in offs}
    bounds, group_of = group_ranges(offs, numel, assign)
    o = offs["ridge_layer.linear.bias"][0]
    assert bounds.tolist() == [0, o, SEG_ALIGN, numel] and group_of.tolist() == [0, 1, 0]
    with pytest.raises(AssertionError):
        group_ranges(offs, numel, assign, ([(0, SEG_ALIGN), (SEG_ALIGN, numel)], [0, SEG_ALIGN // 16], 16, 0))   # 8 * 16 does not divide 6720


# ------------------------------------------------------------------------------------------------ scheduler
def test_cosine_scheduler_keeps_the_group_ratios():
    """torch's CosineAnnealingLR over a CPU optimiser with the three groups the example configuration gives a frozen-backbone
    module: every group follows lr_scale x the default group's curve at every step."""
    entries = normalize_optimizer_groups(EXAMPLE[:2])
    assign = assign_groups(HEAD, entries)
    specs = group_specs(entries, 3e-4, 1e-2)
    params = {n: torch.nn.Parameter(torch.zeros(3)) for n in HEAD}
    # (nothing stays in the default group here, so give it one tensor of its own)
    params["extra"] = torch.nn.Parameter(torch.zeros(3))
    assign["extra"] = 0
    opt = torch.optim.AdamW([dict(params=[p for n, p in params.items() if assign[n] == k], lr=s["lr"], weight_decay=s["weight_decay"])
                             for k, s in enumerate(specs)], lr=3e-4)
    assert len(opt.param_groups) == 3 and [len(g["params"]) for g in opt.param_groups] == [1, 5, 1]
    T = 40
    sch = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=T)
    for step in range(T + 5):
        base = opt.param_groups[0]["lr"]
        closed = 3e-4 * 0.5 * (1 + math.cos(math.pi * step / T)) if step <= T else None
        if closed is not None:
            assert base == pytest.approx(closed, rel=1e-9, abs=1e-18)
        for g, scale in zip(opt.param_groups, (1.0, 10.0, 10.0)):
            assert g["lr"] == pytest.approx(scale * base, rel=1e-9, abs=1e-18), (step, scale)
        assert [g["weight_decay"] for g in opt.param_groups] == [1e-2, 0.0, 1e-2]
        opt.step()
        sch.step()
