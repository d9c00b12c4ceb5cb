"""The decoder layer's seven linears: the geometry's table, the stacking ``Weights`` applies and its inverse (no GPU)."""
import pytest
import torch

BF = torch.bfloat16
SUFFIXES = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj",
            "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]


def _geometries():
    from phantom_vlb_amd.geometry import geometry_7b, geometry_mini
    return {"mini": geometry_mini(), "7b": geometry_7b()}


# (out, in) of the seven linears, written out: Mistral-7B (modeling_mistral.py:113-116,163-165 at hidden 4096, 32 heads of 128,
# 8 kv heads, intermediate 14336) and the mini configuration (hidden 512, 4 heads of 128, 1 kv head, intermediate 1024)
SHAPES = {"7b": [(4096, 4096), (1024, 4096), (1024, 4096), (4096, 4096), (14336, 4096), (14336, 4096), (4096, 14336)],
          "mini": [(512, 512), (128, 512), (128, 512), (512, 512), (1024, 512), (1024, 512), (512, 1024)]}


@pytest.mark.parametrize("name", ["mini", "7b"])
def test_table_lists_the_seven_linears_in_upstream_order(name):
    from phantom_vlb_amd.geometry import decoder_linears
    g = _geometries()[name]
    lins = decoder_linears(g)
    assert [lin.suffix for lin in lins] == SUFFIXES
    assert [(lin.out, lin.inp) for lin in lins] == SHAPES[name]
    assert (g.q_dim, g.kv_dim) == (SHAPES[name][0][0], SHAPES[name][1][0])
    # bands: q | k | v tile wqkv, gate | up tile wgu, o and down are whole tensors; every member of a stack shares its input
    rows = {}
    for lin in lins:
        assert lin.row == rows.get(lin.stacked, 0), lin
        rows[lin.stacked] = lin.row + lin.out
        assert lin.inp == next(m.inp for m in lins if m.stacked == lin.stacked)
    assert rows == {"wqkv": g.q_dim + 2 * g.kv_dim, "wo": g.dim, "wgu": 2 * g.ff, "wdown": g.dim}


def test_table_matches_random_state_dict_named_modules_and_lora_groups():
    """The other statements of the same seven linears agree with the table: the shapes ``random_state_dict`` draws, the
    decoder part of ``Backbone.named_modules`` (names, order, features) and the flat order of ``lora.GROUPS``."""
    from phantom_vlb_amd.backbone import Backbone, Weights
    from phantom_vlb_amd.lora import GROUPS
    g = _geometries()["mini"]
    import vlb_oracle as O
    sd = Weights.random_state_dict(g, "cpu")
    # the oracle's own geometry dataclass (same fields, no properties of this package) is accepted too: the full-depth GPU test
    # draws its weights that way
    assert {k: v.shape for k, v in Weights.random_state_dict(O.geometry_mini(), "cpu").items()} == {k: v.shape for k, v in sd.items()}
    for i in range(g.layers):
        got = [(k, tuple(v.shape)) for k, v in sd.items() if k.startswith(f"model.layers.{i}.") and "norm" not in k]
        assert got == [(f"model.layers.{i}.{s}.weight", shp) for s, shp in zip(SUFFIXES, SHAPES["mini"])]
    bb = Backbone.__new__(Backbone)         # named_modules reads the geometry only
    bb.g = g
    mods = [(n, (m.out_features, m.in_features)) for n, m in bb.named_modules()]
    dec = [e for e in mods if e[0].startswith("model.layers.")]
    assert dec == [(f"model.layers.{i}.{s}", shp) for i in range(g.layers) for s, shp in zip(SUFFIXES, SHAPES["mini"])]
    # the decoder entries sit between the connector's readout and lm_head, as before
    assert mods[-1] == ("lm_head", (g.vocab, g.dim)) and mods[-1 - len(dec):-1] == dec
    assert mods[-2 - len(dec)][0] == "model.mm_projector.readout.2"
    assert len(mods) == 6 * g.vit_layers + 2 + len(dec) + 1
    assert [t for _, ts in GROUPS for t in ts] == SUFFIXES
    assert [name for name, _ in GROUPS] == ["qkv", "o", "gu", "down"]


def test_destack_inverts_the_stacking_of_weights():
    """Random bf16 linears of the mini geometry -> ``Weights`` (frozen forward layout: q|k|v stacked, gate/up interleaved)
    and the plain [gate; up] stack of the trainable layouts -> ``destack_decoder_layer`` returns the seven inputs."""
    from phantom_vlb_amd import ops
    from phantom_vlb_amd.backbone import Weights, destack_decoder_layer
    g = _geometries()["mini"]
    sd = Weights.random_state_dict(g, "cpu", seed=77)
    w = Weights(g, sd, "cpu")
    for i, lw in enumerate(w.layers):
        want = {s: sd[f"model.layers.{i}.{s}.weight"] for s in SUFFIXES}
        assert all(t.dtype == BF and float(t.float().abs().max()) > 0 for t in want.values())
        assert len({float(t.float().sum()) for t in want.values()}) == 7          # seven different tensors
        assert "wgu" not in lw and lw["wgu_il"].shape == (2 * g.ff, g.dim)
        got = destack_decoder_layer(g, lw["wqkv"], lw["wo"], lw["wdown"], wgu_il=lw["wgu_il"])
        assert list(got) == SUFFIXES
        for s in SUFFIXES:
            assert torch.equal(got[s], want[s]), s
        # plain form, stacked as Weights(keep_transposed=True) does: cat([gate; up])
        wgu = torch.cat([want["mlp.gate_proj"], want["mlp.up_proj"]], 0)
        assert torch.equal(ops.interleave_gate_up(wgu[:g.ff], wgu[g.ff:]), lw["wgu_il"])
        got = destack_decoder_layer(g, lw["wqkv"], lw["wo"], lw["wdown"], wgu=wgu)
        assert list(got) == SUFFIXES
        for s in SUFFIXES:
            assert torch.equal(got[s], want[s]), s
        assert got["self_attn.k_proj"].data_ptr() == lw["wqkv"][g.q_dim:].data_ptr()      # bands are views, not copies
