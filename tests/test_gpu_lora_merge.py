"""Merged LoRA adapters (-m gpu): vlb_lora_merge against fp64, its exact identities, validation on merged weights,
staleness of the cached merge, the export round trip, the untouched default and the refusal under sharding."""
import dataclasses

import pytest
import torch

from conftest import rel_err
from gen_golden import load_golden

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _r(*shape, dev, std, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * std).to(BF).to(dev)


def _rows(N, row_map, dev):
    """Rows of W / Wm that hold output features 0..N-1 (the row maps of include/vlb.h)."""
    n = torch.arange(N, device=dev)
    return n if row_map == 0 else 32 * (n // 16) + (16 if row_map == 2 else 0) + n % 16


def _expect(w_rows, bt, a, scale):
    """fp64 value E of w + scale * sum_r b_r a_r on the same bf16 inputs, and the per-element bound
    2^-8 |E| (half a bf16 ulp of the result) + (R+2) 2^-24 (|w| + |scale| sum_r |b_r a_r|) (fp32 accumulate, scale, add)."""
    R = a.shape[0]
    E = w_rows.double() + scale * (bt.double().t() @ a.double())
    S = bt.double().abs().t() @ a.double().abs()
    bound = 2.0 ** -8 * E.abs() + (R + 2) * 2.0 ** -24 * (w_rows.double().abs() + abs(scale) * S)
    return E, bound


def _worst(got_rows, E, bound):
    """max over elements of |Wm - E| / bound: the check passes when this is <= 1."""
    return float(((got_rows.double() - E).abs() / bound.clamp_min(1e-300)).max())


def _case(dev, N, K, R, row_map, seed):
    rows = N if row_map == 0 else 2 * N
    W = _r(rows, K, dev=dev, std=0.02, seed=seed)
    return W, _r(R, N, dev=dev, std=0.05, seed=seed + 1), _r(R, K, dev=dev, std=0.05, seed=seed + 2)


# ------------------------------------------------------------------ 1. kernel versus fp64
@pytest.mark.parametrize("row_map", [0, 1, 2])
@pytest.mark.parametrize("scale", [2.0, 0.8, 0.25])
@pytest.mark.parametrize("R", [16, 32, 48, 64])
def test_merge_matches_fp64(dev, R, scale, row_map):
    """N = 160 ends inside a block's 128-row band and K = 328 inside a lane's 16 columns (the second 8-column half of the
    last lane group is out of range)."""
    from phantom_vlb_amd import ops
    N, K = 160, 328
    W, Bt, A = _case(dev, N, K, R, row_map, seed=100 * R + row_map)
    keep = W.clone()
    Wm = torch.full_like(W, 7.0)
    ops.lora_merge(W, Wm, Bt, A, scale, row_map)
    idx = _rows(N, row_map, dev)
    E, bound = _expect(W[idx], Bt, A, scale)
    worst = _worst(Wm[idx], E, bound)
    print(f"R={R} scale={scale} map={row_map}: worst |Wm-E|/bound = {worst:.3f}")
    assert worst <= 1.0
    assert torch.equal(W, keep)                                   # the base weight is read only
    other = torch.ones(W.shape[0], dtype=torch.bool, device=dev)
    other[idx] = False
    assert (Wm[other] == 7.0).all()                               # the other half of an interleaved image is not written


def test_merge_check_rejects_planted_bugs(dev):
    """The bound is tight enough to see the two mistakes a merge can make silently: each is shown by handing the check
    the reference such a kernel would satisfy."""
    from phantom_vlb_amd import ops
    N, K, R, scale = 160, 328, 16, 0.8
    W, Bt, A = _case(dev, N, K, R, 1, seed=5)
    Wm = torch.zeros_like(W)
    ops.lora_merge(W, Wm, Bt, A, scale, ops.MERGE_GATE)
    gate, up = _rows(N, 1, dev), _rows(N, 2, dev)
    assert _worst(Wm[gate], *_expect(W[gate], Bt, A, scale)) <= 1.0
    assert _worst(Wm[gate], *_expect(W[gate], Bt, A, scale * scale)) > 1.0          # scale applied twice
    Wu = torch.zeros_like(W)
    ops.lora_merge(W, Wu, Bt, A, scale, ops.MERGE_UP)
    assert _worst(Wu[up], *_expect(W[up], Bt, A, scale)) <= 1.0
    assert _worst(Wu[gate], *_expect(W[gate], Bt, A, scale)) > 1.0                  # gate / up maps swapped
    assert _worst(Wm[up], *_expect(W[up], Bt, A, scale)) > 1.0
    for s in (2.0, 0.25):
        ops.lora_merge(W, Wm, Bt, A, s, ops.MERGE_GATE)
        assert _worst(Wm[gate], *_expect(W[gate], Bt, A, s * s)) > 1.0


def test_merge_bands_of_a_stacked_weight_and_strided_views(dev):
    """q / k / v bands inside one stacked wqkv (base pointer of the band, row_map 0): each call writes its band only, three
    calls fill the image; W and Wm are column views of wider tensors with different row strides."""
    from phantom_vlb_amd import ops
    qd, kd, K, R, scale = 256, 64, 192, 32, 0.8
    tot = qd + 2 * kd
    Wbig = _r(tot, K + 64, dev=dev, std=0.02, seed=1)
    Mbig = torch.full((tot + 32, K + 8), 7.0, dtype=BF, device=dev)
    W, Wm = Wbig[:, :K], Mbig[16:16 + tot, :K]
    assert W.stride(0) != K and Wm.stride(0) != K and W.stride(0) != Wm.stride(0)
    A = _r(3 * R, K, dev=dev, std=0.05, seed=2)
    bts = [_r(R, n, dev=dev, std=0.05, seed=3 + j) for j, n in enumerate((qd, kd, kd))]
    row = 0
    for j, n in enumerate((qd, kd, kd)):
        ops.lora_merge(W[row:row + n], Wm[row:row + n], bts[j], A[R * j:R * j + R], scale)
        assert (Wm[row + n:] == 7.0).all()                        # bands not merged yet
        assert _worst(Wm[row:row + n], *_expect(W[row:row + n], bts[j], A[R * j:R * j + R], scale)) <= 1.0
        row += n
    assert (Mbig[:16] == 7.0).all() and (Mbig[16 + tot:] == 7.0).all() and (Mbig[:, K:] == 7.0).all()
    row = 0
    for j, n in enumerate((qd, kd, kd)):                          # an earlier band is not disturbed by a later call
        assert _worst(Wm[row:row + n], *_expect(W[row:row + n], bts[j], A[R * j:R * j + R], scale)) <= 1.0
        row += n


def test_merge_full_size_gate_up(dev):
    """The 7B gate + up projections (14336 x 4096 each, R = 16) into a 28672 x 4096 interleaved image."""
    from phantom_vlb_amd import ops
    ff, K, R, scale = 14336, 4096, 16, 2.0
    W = _r(2 * ff, K, dev=dev, std=0.02, seed=11)
    Wm = torch.empty_like(W)
    A = _r(2 * R, K, dev=dev, std=0.02, seed=12)
    bts = [_r(R, ff, dev=dev, std=0.02, seed=13 + j) for j in range(2)]
    for j, rm in enumerate((ops.MERGE_GATE, ops.MERGE_UP)):
        ops.lora_merge(W, Wm, bts[j], A[R * j:R * j + R], scale, rm)
    for j, rm in enumerate((1, 2)):
        idx = _rows(ff, rm, dev)
        worst = _worst(Wm[idx], *_expect(W[idx], bts[j], A[R * j:R * j + R], scale))
        print(f"full size map {rm}: worst |Wm-E|/bound = {worst:.3f}")
        assert worst <= 1.0


def test_merge_refuses_bad_arguments(dev):
    from phantom_vlb_amd import ops
    from phantom_vlb_amd._lib import VlbError
    W, Bt, A = _case(dev, 64, 128, 16, 0, seed=3)
    with pytest.raises(VlbError, match="alias"):
        ops.lora_merge(W, W, Bt, A, 1.0)                          # in-place merge
    with pytest.raises(VlbError, match="alias"):
        ops.lora_merge(W[:32], W.view(-1)[64:64 + 32 * 128].view(32, 128), Bt[:, :32].contiguous(), A, 1.0)    # overlapping
    with pytest.raises(VlbError, match="rank"):
        ops.lora_merge(W, torch.empty_like(W), _r(24, 64, dev=dev, std=1, seed=1), _r(24, 128, dev=dev, std=1, seed=2), 1.0)
    W2 = _r(48, 128, dev=dev, std=1, seed=4)                      # N = 24: not a multiple of 16 for the interleaved maps
    with pytest.raises(VlbError, match="multiple of 16"):
        ops.lora_merge(W2, torch.empty_like(W2), _r(16, 24, dev=dev, std=1, seed=5), A, 1.0, ops.MERGE_GATE)
    with pytest.raises(VlbError, match="aligned"):
        ops.lora_merge(W.view(-1)[4:4 + 32 * 128].view(32, 128), torch.empty(32, 128, dtype=BF, device=dev),
                       Bt[:, :32].contiguous(), A, 1.0)


# ------------------------------------------------------------------ 2. identities, bit for bit
def test_merge_identities(dev):
    from phantom_vlb_amd import ops
    ff, K, R = 96, 264, 48
    gate_w, up_w = _r(ff, K, dev=dev, std=0.02, seed=1), _r(ff, K, dev=dev, std=0.02, seed=2)
    A = _r(2 * R, K, dev=dev, std=0.05, seed=3)
    bg, bu = _r(R, ff, dev=dev, std=0.05, seed=4), _r(R, ff, dev=dev, std=0.05, seed=5)
    out = torch.empty_like(gate_w)
    assert torch.equal(ops.lora_merge(gate_w, out, torch.zeros_like(bg), A[:R], 0.8), gate_w)      # B = 0: fresh adapters
    out = torch.empty_like(gate_w)
    assert torch.equal(ops.lora_merge(gate_w, out, bg, A[:R], 0.0), gate_w)                        # scale = 0
    m1 = ops.lora_merge(gate_w, torch.empty_like(gate_w), bg, A[:R], 0.8)
    m2 = ops.lora_merge(gate_w, torch.empty_like(gate_w), bg, A[:R], 0.8)
    assert torch.equal(m1, m2) and not torch.equal(m1, gate_w)
    # merging the interleaved image == interleaving the merged plain halves
    mu = ops.lora_merge(up_w, torch.empty_like(up_w), bu, A[R:], 0.8)
    W_il = ops.interleave_gate_up(gate_w, up_w)
    Wm_il = torch.empty_like(W_il)
    ops.lora_merge(W_il, Wm_il, bg, A[:R], 0.8, ops.MERGE_GATE)
    ops.lora_merge(W_il, Wm_il, bu, A[R:], 0.8, ops.MERGE_UP)
    assert torch.equal(Wm_il, ops.interleave_gate_up(m1, mu))


# ------------------------------------------------------------------ module level
def _cfg(**kw):
    from phantom_vlb_amd.litmodule import VLBLitModuleConfig
    base = dict(model_path="none", freeze_backbone=False, use_lora=True, lora_r=16, lora_alpha=32, lora_dropout=0.1,
                dropout_rate=0.0, num_target=128, l2_lambda=1e-3, lr=1e-4, betas=[0.9, 0.999], eps=1e-8, weight_decay=1e-2,
                lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=50000, geometry="mini")
    base.update(kw)
    return VLBLitModuleConfig(**base)


def _module(p, **kw):
    from phantom_vlb_amd.litmodule import VLBLitModule
    m = VLBLitModule(_cfg(**kw))
    m.configure_model(state_dict=p, head_state=p)
    m.configure_optimizers()
    return m


@pytest.mark.parametrize("r", [16, 40])
def test_merged_validation_meets_the_unmerged_bars(dev, r):
    """validation_step on merged weights against the bars test_validation_step_applies_the_adapters holds the unmerged
    path to (loss 1e-3 relative, predictions 3e-2 max/max): r = 16 against the committed golden, r = 40 (alpha/r = 0.8, not
    a power of two; three 16-rank blocks, the last one padded) against the fp32 oracle with the adapters applied."""
    import vlb_oracle as O
    if r == 16:
        g = O.geometry_mini()
        p = O.round_bf16(O.init_params(g, seed=1234, lora=True, lora_b_std=0.02))
        batch = O.synthetic_batch(g, 4, seed=1234)
        gold = load_golden("mini_lora.npz")
        gold_loss, gold_pred = float(gold["loss"]), torch.from_numpy(gold["pred"])
    else:
        g = O.geometry_mini(lora_r=r, lora_alpha=32)
        p = O.round_bf16(O.init_params(g, seed=5, lora=True, lora_b_std=0.05))
        batch = O.synthetic_batch(g, 4, seed=1234)
        with torch.no_grad():
            loss_ref, pred_ref = O.training_loss(p, batch, g)
        gold_loss, gold_pred = float(loss_ref), pred_ref
    m = _module(p, lora_r=r, merge_lora_for_eval=True)
    assert m.lora.p == 0.1 and m.lora._merged is None
    out = m.validation_step(batch)
    assert m.lora._merged is not None                                               # the merged path ran
    loss_rel = abs(float(out["loss"]) - gold_loss) / gold_loss
    pred_rel = rel_err(out["brain_preds"], gold_pred)
    print(f"r={r}: merged validation loss rel {loss_rel:.2e}, pred rel {pred_rel:.2e}")
    assert loss_rel < 1e-3
    assert pred_rel < 3e-2
    again = m.validation_step(batch)
    assert torch.equal(out["brain_preds"], again["brain_preds"]) and torch.equal(out["loss"], again["loss"])
    lora, m.lora = m.lora, None                                                     # the bare backbone: what it must NOT be
    bare = m.validation_step(batch)
    m.lora = lora
    assert rel_err(bare["brain_preds"], gold_pred) > 2 * pred_rel
    assert m.training                                                               # mode restored


def test_merge_is_cached_until_the_adapters_change(dev):
    import vlb_oracle as O
    from phantom_vlb_amd import ops
    g = O.geometry_mini()
    p = O.round_bf16(O.init_params(g, seed=1234, lora=True, lora_b_std=0.02))
    batch = O.synthetic_batch(g, 4, seed=1234)
    m = _module(p, merge_lora_for_eval=True, lr=1e-3)
    first = m.validation_step(batch)
    layers = m.lora.merge()
    ptrs = [lw[k].data_ptr() for lw in layers for k in sorted(lw)]
    launches, version = ops.merge_launches, m.lora.version
    assert launches >= 7 * g.layers
    # nothing changed: the same list, the same buffers, no launch
    same = m.validation_step(batch)
    assert m.lora.merge() is layers and ops.merge_launches == launches and m.lora.version == version
    assert torch.equal(first["brain_preds"], same["brain_preds"])
    # the base weights are referenced, never copied or changed, for the norms; the linears are new buffers
    assert layers[0]["in_norm"] is m.backbone.w.layers[0]["in_norm"]
    assert layers[0]["wqkv"].data_ptr() != m.backbone.w.layers[0]["wqkv"].data_ptr()
    # one optimiser step: the next validation re-merges (into the same buffers) and moves
    m.training_step(batch)
    m.optimizer.step()
    assert m.lora.version > version
    stepped = m.validation_step(batch)
    assert ops.merge_launches == launches + 7 * g.layers
    assert [lw[k].data_ptr() for lw in m.lora.merge() for k in sorted(lw)] == ptrs
    assert not torch.equal(stepped["brain_preds"], first["brain_preds"])
    # ... and again agrees with the unmerged eval forward of the same module, to the bars of the merged validation test
    m.config.merge_lora_for_eval = False
    unmerged = m.validation_step(batch)
    m.config.merge_lora_for_eval = True
    assert ops.merge_launches == launches + 7 * g.layers
    assert abs(float(stepped["loss"]) - float(unmerged["loss"])) / float(unmerged["loss"]) < 1e-3
    assert rel_err(stepped["brain_preds"], unmerged["brain_preds"]) < 3e-2
    # load_state_dict invalidates too
    v = m.lora.version
    m.lora.load_state_dict(m.lora.state_dict())
    assert m.lora.version > v


def test_export_round_trip_is_bit_exact(dev, tmp_path):
    """save_merged -> a plain frozen module built from {base without adapters, merged file}: the same kernels on the same
    weight bits in the same packed layout, so the predictions are equal, not close."""
    import vlb_oracle as O
    from safetensors.torch import load_file
    from phantom_vlb_amd.head import HEAD_PARAMS
    g = O.geometry_mini(lora_r=40, lora_alpha=32)
    p = O.round_bf16(O.init_params(g, seed=5, lora=True, lora_b_std=0.05))
    batch = O.synthetic_batch(g, 4, seed=1234)
    m = _module(p, lora_r=40, merge_lora_for_eval=True)
    want = m.validation_step(batch)
    sd = m.merged_state_dict()
    names = {f"{n}.weight": (mod.out_features, mod.in_features) for n, mod in m.backbone.named_modules()
             if n.startswith("model.layers.")}
    assert len(names) == 7 * g.layers
    assert {k: tuple(v.shape) for k, v in sd.items() if k not in HEAD_PARAMS} == names
    assert all(sd[k].dtype == BF for k in names) and all(n in sd for n in HEAD_PARAMS)
    path = m.save_merged(str(tmp_path / "export" / "merged.safetensors"))
    loaded = load_file(path)
    assert set(loaded) == set(sd) and all(torch.equal(loaded[k], sd[k]) for k in sd)
    base = {k: v for k, v in p.items() if ".lora_" not in k}
    plain = _module({**base, **loaded}, use_lora=False, freeze_backbone=True, lora_r=None, lora_alpha=None, lora_dropout=None)
    assert plain.lora is None
    got = plain.validation_step(batch)
    assert torch.equal(got["brain_preds"], want["brain_preds"]) and torch.equal(got["loss"], want["loss"])


def test_default_validation_is_untouched(dev):
    """Flag off: validation_step is the adapted decoder's train=False forward, bit for bit, and no merged buffer exists."""
    import vlb_oracle as O
    from phantom_vlb_amd import ops
    g = O.geometry_mini()
    p = O.round_bf16(O.init_params(g, seed=1234, lora=True, lora_b_std=0.02))
    batch = O.synthetic_batch(g, 4, seed=1234)
    m = _module(p)
    assert m.config.merge_lora_for_eval is False
    calls, trains = [], []
    inner = m.lora.decoder_forward

    def spy(backbone, x, key_mask, B, layout=None, train=True):
        calls.append(1)
        trains.append(train)
        return inner(backbone, x, key_mask, B, layout, train=train)
    m.lora.decoder_forward = spy
    launches = ops.merge_launches
    out = m.validation_step(batch)
    assert calls == [1] and ops.merge_launches == launches
    assert trains == [False]
    assert getattr(m.lora, "_merged", None) is None
    # the same forward by hand: adapted eval decoder, then the head
    del m.lora.decoder_forward
    layout = m.backbone.row_layout(batch["language"], batch["padvals"])
    ids = batch["language"].to(m.device).long()
    wm = m.make_weight_mask(batch["padvals"], batch["vis_weights"], batch["lang_weights"], ids.shape[1], g.max_len)
    y = batch["timeseries"].to(m.device, torch.float32).to(BF).float().contiguous()
    hidden, _ = m.lora.forward(m.backbone, m._vision_tensor(batch["vision"]), ids, layout, train=False)
    pred, terms = m.head.forward(hidden, wm, y, None, layout)
    assert torch.equal(out["brain_preds"], pred) and torch.equal(out["loss"], terms[2])
    assert getattr(m.lora, "_merged", None) is None


def test_merged_path_refuses_a_sharded_layer_store(dev):
    import vlb_oracle as O
    g = O.geometry_mini()
    p = O.round_bf16(O.init_params(g, seed=1234, lora=True, lora_b_std=0.02))
    batch = O.synthetic_batch(g, 2, seed=3)
    m = _module(p, merge_lora_for_eval=True)
    m.backbone.enable_sharding()
    assert m.backbone.w.layers[0]["wqkv"] is None
    with pytest.raises(ValueError, match="shard"):
        m.validation_step(batch)
    with pytest.raises(ValueError, match="shard"):
        m.lora.merge()
    with pytest.raises(ValueError, match="shard"):
        m.merged_state_dict()
    assert m.lora._merged is None
    m.config.merge_lora_for_eval = False                          # the unmerged path still runs on the gathered layers
    m.validation_step(batch)
