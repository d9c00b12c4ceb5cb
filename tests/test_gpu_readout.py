"""``readout_layers`` through the module (mini geometry, packed rows): bit identity with the default path where they
overlap, gradients against an autograd restatement built on the oracle's decoder, validation / merged eval, training the
mix, checkpoint resume, the K-slab feature cache and data parallelism with skipped layers.  (-m gpu)"""
import dataclasses
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIX = "layer_mix.weight"


def _cfg(**kw):
    from phantom_vlb_amd.litmodule import VLBLitModuleConfig
    base = dict(model_path="none", freeze_backbone=True, use_lora=False, lora_r=None, lora_alpha=None, lora_dropout=None,
                dropout_rate=0.0, num_target=128, l2_lambda=1e-3, lr=1e-3, betas=[0.9, 0.999], eps=1e-8,
                weight_decay=1e-2, lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=50000, geometry="mini")
    base.update(kw)
    return VLBLitModuleConfig(**base)


def _lora_kw(p=0.0):
    return dict(freeze_backbone=False, use_lora=True, lora_r=16, lora_alpha=32, lora_dropout=p)


def _build(p, **kw):
    from phantom_vlb_amd.litmodule import VLBLitModule
    m = VLBLitModule(_cfg(**kw))
    m.configure_model(state_dict=p, head_state=p)
    return m, m.configure_optimizers()[0][0]


# ---------------------------------------------------------------------------------------------------- 1. bit identity
@pytest.mark.parametrize("lora", [False, True], ids=["frozen", "lora-dropout"])
def test_last_layer_tap_is_the_default_path_bit_for_bit(dev, lora):
    """readout_layers=[L] computes what the unset option computes: loss, pred, every head and adapter gradient and the
    trainables after one optimiser step are the same bits (LoRA: both dropouts at 0.1)."""
    import vlb_oracle as O
    g = O.geometry_mini(lora_r=16, lora_alpha=32) if lora else O.geometry_mini()
    p = O.round_bf16(O.init_params(g, seed=5, lora=lora, lora_b_std=0.05) if lora else O.init_params(g, seed=5))
    batch = O.synthetic_batch(g, 2, seed=6)
    kw = dict(_lora_kw(0.1), dropout_rate=0.1) if lora else {}
    out = []
    for taps in (None, [g.layers], [-1]):
        m, opt = _build(p, readout_layers=taps, **kw)
        loss = m.training_step(batch).clone()
        grads = {n: t.clone() for n, t in m.head.grads.items()}
        if lora:
            grads.update({n: t.clone() for n, t in m.lora.grads.items()})
        opt.step()
        torch.cuda.synchronize()
        out.append(dict(loss=loss, pred=m.head.pred.clone(), grads=grads, sd=m.trainable_state_dict()))
    ref = out[0]
    assert len(ref["grads"]) == (6 + 28 if lora else 6) and MIX not in ref["sd"]
    for got in out[1:]:
        assert torch.equal(got["loss"], ref["loss"]) and torch.equal(got["pred"], ref["pred"])
        assert set(got["grads"]) == set(ref["grads"]) and set(got["sd"]) == set(ref["sd"])
        bad = [n for n in ref["grads"] if not torch.equal(got["grads"][n], ref["grads"][n])]
        assert not bad, bad
        bad = [n for n in ref["sd"] if not torch.equal(got["sd"][n], ref["sd"][n])]
        assert not bad, bad
    assert any(float(t.abs().max()) > 0 for n, t in ref["grads"].items() if ".lora_" in n) or not lora


# ---------------------------------------------------------------------------------------------------- 2. the oracle
def _oracle(p, batch, g, taps, mix, train_names):
    """The tapped head as autograd sees it: hidden_states = the oracle decoder's layer outputs [:L-1] + [post-norm];
    LN1 without affine and HRF pooling per tapped layer, softmax mix, LN1's affine on the mix, then the head's tail."""
    import vlb_oracle as O
    q = {n: (t.clone().requires_grad_(True) if n in train_names else t) for n, t in p.items()}
    a = mix.clone().requires_grad_(True) if mix is not None else None
    stages = {}
    O.backbone_forward(q, batch, g, stages)
    hs = list(stages["layer_outputs"][:g.layers - 1]) + [stages["hidden"]]
    wm = O.make_weight_mask(batch["padvals"], batch["vis_weights"], batch["lang_weights"], batch["language"].shape[1], g.max_len,
                            g.ds_grid * g.ds_grid).to(torch.bfloat16).float()
    y = batch["timeseries"].to(torch.bfloat16).float()
    P = torch.stack([O.hrf_convolve(F.layer_norm(hs[t - 1], (g.dim,), None, None, g.ln_eps), wm) for t in taps])
    alpha = torch.softmax(a, 0) if a is not None else torch.ones(1)
    pooled = q["layer_norm1.weight"] * (alpha[:, None, None] * P).sum(0) + q["layer_norm1.bias"] * wm.sum(1, keepdim=True)
    z = F.layer_norm(pooled, (g.dim,), q["layer_norm2.weight"], q["layer_norm2.bias"], g.ln_eps)
    pred, l2 = O.ridge_regression(q["ridge_layer.linear.weight"], q["ridge_layer.linear.bias"], z, g.l2_lambda)
    loss = F.mse_loss(pred, y) + l2
    return dict(loss=loss, pred=pred, q=q, a=a, alpha=alpha)


def _mix_values(K):
    return None if K == 1 else torch.tensor([0.75, -0.5, 0.25][:K])          # bf16-representable, non-zero


def _lora_case(dev, monkeypatch, L, taps):
    import vlb_oracle as O
    from phantom_vlb_amd import litmodule as LM
    from phantom_vlb_amd.geometry import geometry_mini
    g = O.geometry_mini(lora_r=16, lora_alpha=32, layers=L)
    if L != 2:          # the mini geometry with another depth, for the module as for the oracle
        monkeypatch.setattr(LM, "resolve_geometry", lambda cfg: geometry_mini(num_target=cfg.num_target, l2_lambda=cfg.l2_lambda,
                                                                              lora_r=cfg.lora_r, lora_alpha=cfg.lora_alpha, layers=L))
    p = O.round_bf16(O.init_params(g, seed=11, lora=True, lora_b_std=0.02))
    batch = O.synthetic_batch(g, 2, seed=12)
    mix = _mix_values(len(taps))
    sd = dict(p) if mix is None else {**p, MIX: mix}
    m, opt = _build(sd, readout_layers=taps, **_lora_kw(0.0))
    assert m.geometry.layers == L and m.head.readout_layers == tuple(taps)
    return g, p, batch, mix, m, opt


@pytest.mark.parametrize("L,taps", [(2, [1]), (2, [1, 2]), (3, [1, 2])], ids=["truncated", "mix", "truncated-mix"])
def test_lora_step_against_the_oracle(dev, monkeypatch, L, taps):
    g, p, batch, mix, m, opt = _lora_case(dev, monkeypatch, L, taps)
    stop = taps[-1]
    asked = []
    lw = m.backbone.layer_weights
    monkeypatch.setattr(m.backbone, "layer_weights", lambda i, *a, **k: (asked.append(i), lw(i, *a, **k))[1])
    loss = m.training_step(batch)
    torch.cuda.synchronize()
    assert sorted(set(asked)) == list(range(stop)), asked           # forward and backward: the skipped layers' weights never
    train = [n for n in p if n.startswith(("layer_norm1", "layer_norm2", "ridge_layer")) or ".lora_" in n]
    ref = _oracle(p, batch, g, taps, mix, train)
    ref["loss"].backward()
    loss_rel = abs(float(loss) - float(ref["loss"])) / float(ref["loss"])
    pred_rel = rel_err(m.head.pred, ref["pred"])
    worst = {}
    for n in train:
        rg = ref["q"][n].grad
        layer = int(n.split(".")[2]) if n.startswith("model.layers.") else -1
        if layer >= stop:           # a layer above the highest tap: no gradient in autograd, exactly zero on the device
            assert rg is None or float(rg.abs().max()) == 0.0, n
            assert float(m.lora.grads[n].abs().max()) == 0.0, n
            continue
        got = m.lora.grads[n] if ".lora_" in n else m.head.grads[n]
        if "lora_B" in n:
            got = got.t()
        kind = "adapter" if ".lora_" in n else "head"
        worst[kind] = max(worst.get(kind, 0.0), rel_err(got, rg))
        assert rel_err(got, rg) < 6e-2, (n, rel_err(got, rg))
    if mix is not None:
        worst["mix"] = rel_err(m.head.grads[MIX], ref["a"].grad)
        assert rel_err(m.head.alpha, ref["alpha"].detach()) < 1e-5
    print(f"readout-oracle L={L} taps={taps}: loss {loss_rel:.2e} pred {pred_rel:.2e} " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert loss_rel < 1e-3 and pred_rel < 3e-2
    assert worst.get("mix", 0.0) < 6e-2
    assert len(m.lora.saved) == 0 and m.lora.stop == stop
    opt.step()              # the flat store carries layer_mix.weight like any head tensor
    torch.cuda.synchronize()
    if mix is not None:
        assert not torch.equal(m.head.master[MIX].cpu(), mix) and torch.equal(m.head.compute[MIX].float(), m.head.master[MIX].to(torch.bfloat16).float())


# ---------------------------------------------------------------------------------------------------- 3. validation, merged eval
def test_validation_against_the_oracle_changes_nothing_and_merged_eval_agrees(dev, monkeypatch):
    import vlb_oracle as O
    g = O.geometry_mini(lora_r=16, lora_alpha=32)
    p = O.round_bf16(O.init_params(g, seed=5, lora=True, lora_b_std=0.05))
    mix = _mix_values(2)
    b1, b2, bval = (O.synthetic_batch(g, 2, seed=s) for s in (6, 7, 8))
    kw = dict(_lora_kw(0.1), dropout_rate=0.2, readout_layers=[1, 2])

    def run(validate):
        m, opt = _build({**p, MIX: mix}, **kw)
        losses, val = [], None
        for i, batch in enumerate((b1, b2)):
            if validate and i == 1:
                val = m.validation_step(bval), m.validation_step(bval)
            losses.append(m.training_step(batch).clone())
            opt.step()
        return m.trainable_state_dict(), losses, val

    sd_a, loss_a, _ = run(False)
    sd_b, loss_b, (v1, v2) = run(True)
    assert torch.equal(v1["brain_preds"], v2["brain_preds"]) and torch.equal(v1["loss"], v2["loss"])
    assert all(torch.equal(x, y) for x, y in zip(loss_a, loss_b))
    assert MIX in sd_a and not [n for n in sd_a if not torch.equal(sd_a[n], sd_b[n])]
    # eval forward (adapters kept, no dropout) against the oracle, and the merged-weights eval against the unmerged one
    m, _ = _build({**p, MIX: mix}, **kw)
    out = m.validation_step(bval)
    with torch.no_grad():
        ref = _oracle(p, bval, g, [1, 2], mix, ())
    assert abs(float(out["loss"]) - float(ref["loss"])) / float(ref["loss"]) < 1e-3
    assert rel_err(out["brain_preds"], ref["pred"]) < 3e-2
    mm, _ = _build({**p, MIX: mix}, merge_lora_for_eval=True, **kw)
    merged = mm.validation_step(bval)
    assert abs(float(merged["loss"]) - float(out["loss"])) / float(out["loss"]) < 1e-3
    assert rel_err(merged["brain_preds"], out["brain_preds"]) < 3e-2
    mm.on_validation_epoch_end()
    al = torch.softmax(mix.to(torch.bfloat16).float(), 0)
    assert abs(mm.logged["readout/alpha_1"] - float(al[0])) < 1e-6 and abs(mm.logged["readout/alpha_2"] - float(al[1])) < 1e-6


# ---------------------------------------------------------------------------------------------------- 4. training moves the mix
def test_training_moves_the_mix_towards_the_informative_layer(dev):
    """Frozen backbone, taps [1, 2], targets a fixed linear read-out of LAYER 1's normalised pooled features alone: over 20
    steps alpha_1 grows monotonically over the last 10 and the loss (on two held-out clips) falls.
    What makes the mix identifiable (worked out on the oracle in fp32, not on the code under test): (a) two clips and 128
    targets can be fitted by the ridge weight from ANY features within a few Adam steps, after which the logits' gradient is
    noise - so every step sees two fresh clips; (b) with std-0.02 weights layer 2 barely moves the residual stream (the two
    layers' pooled features have cosine 0.83-0.97) - so layer 2's output projections are scaled by 8 (cosine 0.3-0.5);
    (c) the head starts at the read-out that made the targets, so at step 0 only the uniform mix is wrong."""
    import vlb_oracle as O
    g = O.geometry_mini()
    p = O.round_bf16(O.init_params(g, seed=21))
    for n in ("model.layers.1.self_attn.o_proj.weight", "model.layers.1.mlp.down_proj.weight"):
        p[n] = p[n] * 8.0
    gen = torch.Generator().manual_seed(23)
    Wt = (torch.randn(128, g.dim, generator=gen) / g.dim ** 0.5).to(torch.bfloat16).float()
    p.update({"layer_norm1.weight": torch.ones(g.dim), "layer_norm1.bias": torch.zeros(g.dim), "layer_norm2.weight": torch.ones(g.dim),
              "layer_norm2.bias": torch.zeros(g.dim), "ridge_layer.linear.weight": Wt, "ridge_layer.linear.bias": torch.zeros(128)})
    whole = O.synthetic_batch(g, 42, seed=22)
    m, opt = _build(p, readout_layers=[1, 2], lr=2e-3, weight_decay=0.0)
    batches = []
    for i in range(21):                            # 20 training batches and a held-out one
        b = {k: v[2 * i:2 * i + 2] for k, v in whole.items()}
        m.validation_step(b)                       # fills head.p_stack with the taps' pooled vectors of these clips
        P1 = m.head.p_stack[0]
        batches.append(dict(b, timeseries=(F.layer_norm(P1, (g.dim,), eps=g.ln_eps) @ Wt.to(dev).t()).cpu()))
    before = float(m.validation_step(batches[20])["loss"])
    alpha1 = []
    for b in batches[:20]:
        m.training_step(b)
        opt.step()
        alpha1.append(float(torch.softmax(m.head.master[MIX], 0)[0]))
    after = float(m.validation_step(batches[20])["loss"])
    print("readout-train alpha_1:", " ".join(f"{a:.4f}" for a in alpha1), "held-out loss", f"{before:.4f} -> {after:.4f}")
    assert all(b > a for a, b in zip(alpha1[-11:-1], alpha1[-10:])), alpha1
    assert alpha1[-1] > 0.5 and after < before


def _dm(batch_size=2):
    from phantom_vlb_amd.datamodule import VLBDataModule, VLBDataModuleConfig
    return VLBDataModule(VLBDataModuleConfig(lazyload_path="synthetic:3x4", subject="sub-01", seasons=["s1"], delay=3, window=3,
                                             random_state=1234, shuffle_val_data=False, batch_size=batch_size, geometry="mini",
                                             num_target=128))


def test_checkpoint_resume_is_exact_with_the_mix(dev, tmp_path):
    """6 steps straight == 4 steps, checkpoint, resume for steps 5-6: masters, bf16 copies and both Adam moments, the
    mix logits' included (they live in the flat store like every head tensor)."""
    from phantom_vlb_amd.litmodule import VLBLitModule
    from phantom_vlb_amd.trainer import TrainableCheckpoint, Trainer
    kw = dict(readout_layers=[1, 2], dropout_rate=0.1)
    a = VLBLitModule(_cfg(**kw))
    ta = Trainer(max_epochs=2, max_steps=6, val_check_interval=1.0, log_every_n_steps=1,
                 callbacks=[TrainableCheckpoint(str(tmp_path), filename="best")])
    ta.fit(a, _dm())
    st = torch.load(tmp_path / "last.ckpt", map_location="cpu", weights_only=False)
    assert st["global_step"] == 4 and tuple(st["state_dict"][MIX].shape) == (2,)
    b = VLBLitModule(_cfg(**kw))
    tb = Trainer(max_epochs=2, max_steps=6, val_check_interval=1.0, log_every_n_steps=1)
    tb.fit(b, _dm(), ckpt_path=str(tmp_path / "last.ckpt"))
    assert tb.global_step == 6 and b.optimizer.step_count == 6
    for name in ("master", "compute", "m", "v"):
        assert torch.equal(getattr(a.flat, name), getattr(b.flat, name)), name
    o, n, _ = a.flat.offsets[MIX]
    assert n == 2 and float(a.flat.master[o:o + n].abs().max()) > 0 and float(a.flat.v[o:o + n].min()) > 0
    assert "readout/alpha_1" in a.logged and abs(a.logged["readout/alpha_1"] + a.logged["readout/alpha_2"] - 1.0) < 1e-5


# ---------------------------------------------------------------------------------------------------- 5. feature cache
def test_feature_cache_with_two_taps(dev, tmp_path):
    """Epoch 2 runs from the cache (hit rate 1, no backbone call) with the loss bits of an uncached module on the same clips
    and parameters; save / load round-trips; files written for [1] are ignored, with the warning, under [1, 2]."""
    import vlb_oracle as O
    from phantom_vlb_amd.feature_cache import FeatureCache
    g = O.geometry_mini()
    p = O.round_bf16(O.init_params(g, seed=31))
    whole = O.synthetic_batch(g, 4, seed=32)
    batches = [dict({k: v[2 * i:2 * i + 2] for k, v in whole.items()}, index=torch.arange(2 * i, 2 * i + 2)) for i in range(2)]
    kw = dict(readout_layers=[1, 2], dropout_rate=0.1, cache_features=True)
    m, opt = _build(p, **kw)
    u, uopt = _build(p, **dict(kw, cache_features=False))
    cache = m.feature_caches["train"] = FeatureCache("train", 4, g.dim, dev, layers=2)
    calls = []
    fwd = m.backbone.forward
    m.backbone.forward = lambda *a, **k: (calls.append(1), fwd(*a, **k))[1]
    for epoch in range(2):
        cache.reset_counters()
        for b in batches:
            got = m.training_step(b).clone()
            opt.step()
            want = u.training_step({k: v for k, v in b.items() if k != "index"}).clone()
            uopt.step()
            assert torch.equal(got, want), (epoch, float(got), float(want))
            assert m._cached_step == (epoch == 1)
        assert cache.hit_rate() == float(epoch) and len(calls) == 2
    assert torch.equal(m.flat.master, u.flat.master)
    assert cache.complete() and tuple(cache.pooled.shape) == (2, 4, g.dim) and not torch.equal(cache.pooled[0], cache.pooled[1])
    cache.save(str(tmp_path), "fp-12")
    back = FeatureCache("train", 4, g.dim, dev, layers=2)
    assert back.load(str(tmp_path), "fp-12") and torch.equal(back.pooled, cache.pooled) and torch.equal(back.sumw, cache.sumw)
    # through the module: a directory written under [1] is not picked up under [1, 2]
    from phantom_vlb_amd.datamodule import VLB_Dataset
    ds = VLB_Dataset([(1, 4)], "mini", 128)
    d1 = tmp_path / "dir"
    one, _ = _build(p, readout_layers=[1], cache_features=True, feature_cache_dir=str(d1))
    one.setup_feature_cache(train_dataset=ds)
    c1 = one.feature_caches["train"]
    assert c1.layers == 1
    c1._alloc()
    c1.valid[:] = True
    c1.save(str(d1), one._feature_cache_fp["train"])
    again, _ = _build(p, readout_layers=[1], cache_features=True, feature_cache_dir=str(d1))
    again.setup_feature_cache(train_dataset=VLB_Dataset([(1, 4)], "mini", 128))
    assert again.feature_caches["train"].complete()                      # the same tap list: loaded
    two, _ = _build(p, readout_layers=[1, 2], cache_features=True, feature_cache_dir=str(d1))
    with pytest.warns(UserWarning, match="fingerprint mismatch"):
        two.setup_feature_cache(train_dataset=VLB_Dataset([(1, 4)], "mini", 128))
    assert not two.feature_caches["train"].valid.any() and two.feature_caches["train"].layers == 2


# ---------------------------------------------------------------------------------------------------- 6. data parallel
def _dp_worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    for q in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if q not in sys.path:
            sys.path.insert(0, q)
    import vlb_oracle as O
    from phantom_vlb_amd.parallel import attach_data_parallel
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        g = O.geometry_mini(lora_r=16, lora_alpha=32)
        p = O.round_bf16(O.init_params(g, seed=3, lora=True, lora_b_std=0.02))
        full = O.synthetic_batch(g, 4, seed=4)
        m, opt = _build(p, readout_layers=[1], **_lora_kw(0.0))
        fired = []
        st = attach_data_parallel(m, opt)
        hook = m.lora.grad_hook
        m.lora.grad_hook = lambda li: (fired.append(li), hook(li))[1]
        m.training_step({k: v[rank * 2:rank * 2 + 2] for k, v in full.items()})
        opt.step()
        st.gather_masters()
        torch.cuda.synchronize()
        ret[rank] = {"master": m.flat.master.cpu(), "compute": m.flat.compute.float().cpu(), "fired": fired,
                     "before": {n: t.cpu() for n, t in p.items() if ".lora_A." in n},
                     "after": {n: t.cpu() for n, t in m.trainable_state_dict().items() if ".lora_A." in n}}
    finally:
        dist.destroy_process_group()


def test_two_ranks_with_a_truncated_decoder(dev):
    """readout_layers=[1] on a 2-layer decoder under 2-rank data parallelism: layer 2 is skipped, its hook still fires (the
    reduce-scatter counts on one call per layer), the step finishes and the ranks hold identical trainables."""
    import random
    ret = mp.Manager().dict()
    mp.spawn(_dp_worker, args=(2, 29600 + random.randint(0, 2000), ret), nprocs=2, join=True)
    assert ret[0]["fired"] == ret[1]["fired"] == [1, 0]
    assert torch.equal(ret[0]["master"], ret[1]["master"]) and torch.equal(ret[0]["compute"], ret[1]["compute"])
    moved = {n: not torch.equal(ret[0]["after"][n], ret[0]["before"][n]) for n in ret[0]["before"]}
    assert all(v for n, v in moved.items() if ".layers.0." in n)                      # the layer below the tap trains
