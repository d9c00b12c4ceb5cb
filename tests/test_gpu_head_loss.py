"""The brain head's correlation objectives (loss="cosine" / "pearson") on the GPU, against tests/head_loss_emul.py.

Stage by stage: each new kernel (row statistics, the finalize, the correlation forms of ridge_bwd_w and of the two dz routes)
is judged on the device's own upstream buffers at its derived fp32 bar, and the stages the objective leaves alone by
head_emul's own checks; loss_terms[1] must carry the bits the plain forward wrote.  End to end: fp64 autograd-equivalent
mathematics (head_emul's chain + the objective) at the bars of test_head_fwd_bwd.  Then: the MSE path never enters the new
entry points, a step is reproducible bit for bit and the cached step equals the uncached one, and at module level
(mini geometry, frozen and LoRA) the logged loss, d ridge bias, a window of two micro-batches and ten optimiser steps.
Run with -s to see max(err / bar)."""
import pytest
import torch

import head_emul as H
import head_loss_emul as L
import test_gpu_head_stages as S

pytestmark = pytest.mark.gpu


def _head(dev, inp, loss=None):
    from phantom_vlb_amd.head import BrainHead
    c = inp["case"]
    return BrainHead(c["E"], c["V"], inp["lam"], inp["eps"], dev, sd=inp["params"], loss=inp["loss"] if loss is None else loss)


def _tensors(head, dh):
    t = S._device_tensors(head, dh)
    t.update(rowstat=head.rowstat, loss_aux=head.loss_aux)
    return t


def _host_buffers(head, dh, inp):
    bufs = S._host_buffers(head, dh, inp)
    bufs.update(L.rowstat_columns(head.rowstat.detach().cpu()), loss_aux=head.loss_aux.detach().cpu())
    return bufs


@pytest.mark.parametrize("cid,loss", L.PAIRS)
def test_head_loss_stages(dev, cid, loss):
    inp = L.inputs_for(cid, loss)
    c = inp["case"]
    assert set(c["expect"]) <= H.dispatch(c["B"], c["E"])
    dinp = S._device_inputs(dev, inp)
    plain = _head(dev, inp, loss="mse")                       # what the plain forward writes into loss_terms
    plain.forward(dinp[0], dinp[1], dinp[2], dinp[3], layout=dinp[4])
    plain_terms = plain.loss_terms.clone()
    head = _head(dev, inp)
    dh = S._step(head, dinp, inp)
    bufs = _host_buffers(head, dh, inp)
    assert all(bool(torch.isfinite(v.float()).all()) for v in bufs.values())
    assert torch.equal(head.loss_terms[1], plain_terms[1]), "loss_terms[1] is not the plain forward's l2, bit for bit"
    assert torch.equal(head.loss_aux[0], plain_terms[0]), "loss_aux[0] is not the plain forward's MSE, bit for bit"
    assert torch.equal(head.pred, plain.pred)
    assert bool((head.rowstat[:, 6:] == 0).all())
    if loss == "cosine":
        assert bool((head.rowstat[:, :2] == 0).all())
    if c["zero_target"]:
        assert float(head.rowstat[1, 5]) == 0.0
    ratios = {**L.check_stages(bufs, inp), **L.check_rest(bufs, inp)}
    print(f"head-loss-stages {cid} {loss}: " + " ".join(f"{k}={v:.3f}" for k, v in H.by_stage(ratios).items()))
    print(f"head-loss-stages-detail {cid} {loss}: " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (cid, loss, bad)
    e2e, bars = L.end_to_end(bufs, inp), H.E2E_BARS
    print(f"head-loss-e2e {cid} {loss}: " + " ".join(f"{k}={v:.2e}/{bars[k]:.0e}" for k, v in e2e.items()))
    bad = {k: (v, bars[k]) for k, v in e2e.items() if not v < bars[k]}
    assert not bad, (cid, loss, bad)


# ---------------------------------------------------------------------------------------------------- mse is untouched
NEW = ("vlb_head_loss_fwd", "vlb_head_bwd_loss", "vlb_head_bwd_cached_loss")


def test_mse_never_enters_the_new_entry_points(dev, monkeypatch):
    from phantom_vlb_amd import _lib
    from phantom_vlb_amd.feature_cache import FeatureCache

    def refuse(*a):
        raise AssertionError("a correlation entry point was called")
    for name in NEW:
        monkeypatch.setattr(_lib.lib, name, refuse)
    inp = L.inputs_for("loss-B3", "cosine")
    c = inp["case"]
    hidden, wmask, y, keep, lay = S._device_inputs(dev, inp)
    head = _head(dev, inp, loss="mse")
    assert head.loss == "mse" and head.loss_kind == 0
    head.forward(hidden, wmask, y, keep, layout=lay)
    head.backward(need_dhidden=True)
    cache = FeatureCache("train", 8, c["E"], dev)
    idx = torch.arange(c["B"])
    cache.store(idx, head)
    head.forward_cached(cache, idx, y, keep)
    head.backward_cached()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(head.loss_terms).all())
    with pytest.raises(AssertionError, match="correlation entry point"):       # ... and the replacement does bite
        _head(dev, inp).forward(hidden, wmask, y, keep, layout=lay)


def test_new_entry_points_refuse_mse_pearson_on_one_target_and_null(dev):
    from phantom_vlb_amd._lib import VlbError
    from phantom_vlb_amd.head import BrainHead
    inp = L.inputs_for("loss-V1", "cosine")
    hidden, wmask, y, keep, lay = S._device_inputs(dev, inp)
    head = _head(dev, inp)
    head.forward(hidden, wmask, y, keep, layout=lay)
    for kind, what in ((0, "mse"), (2, "pearson"), (3, "unknown")):
        head.loss_kind = kind
        with pytest.raises(VlbError, match=what):
            head._loss_fwd(y, *wmask.shape)
        with pytest.raises(VlbError, match=what):
            head.backward(need_dhidden=False) if kind else _bwd_loss_kind0(head)
    head.loss_kind = 1
    head.rowstat = torch.empty(0, device=dev)                   # data_ptr() == 0
    with pytest.raises(VlbError, match="null"):
        head._loss_fwd(y, *wmask.shape)
    with pytest.raises(ValueError, match="pearson"):
        BrainHead(inp["case"]["E"], 1, H.LAMBDA, H.EPS, dev, loss="pearson")
    torch.cuda.synchronize()


def _bwd_loss_kind0(head):
    """vlb_head_bwd_loss with loss_kind = 0 (BrainHead itself routes kind 0 to vlb_head_bwd)"""
    from phantom_vlb_amd._lib import check, lib
    from phantom_vlb_amd.ops import _stream
    hidden, wmask, y, keep, cu, rows = head._saved
    B, Sq = wmask.shape
    c, gr = head.compute, head.grads
    check(lib.vlb_head_bwd_loss(hidden.data_ptr(), wmask.data_ptr(), c["layer_norm1.weight"].data_ptr(),
                                c["layer_norm2.weight"].data_ptr(), c["ridge_layer.linear.weight"].data_ptr(), y.data_ptr(), None,
                                head.stats.data_ptr(), head.pooled_raw.data_ptr(), head.sumw.data_ptr(), head.zhat.data_ptr(),
                                head.ln2_rstd.data_ptr(), head.z.data_ptr(), head.pred.data_ptr(),
                                gr["ridge_layer.linear.weight"].data_ptr(), gr["ridge_layer.linear.bias"].data_ptr(),
                                gr["layer_norm2.weight"].data_ptr(), gr["layer_norm2.bias"].data_ptr(),
                                gr["layer_norm1.weight"].data_ptr(), gr["layer_norm1.bias"].data_ptr(), head.ws.data_ptr(),
                                head.dz.data_ptr(), head.dpooled.data_ptr(), None, B, Sq, head.E, head.V, head.eps, head.l2_lambda,
                                1.0, 1.0, None, rows, _stream(), 0, head.rowstat.data_ptr()), "vlb_head_bwd_loss")


# ---------------------------------------------------------------------------------------------------- same bits
@pytest.mark.parametrize("cid,loss", [("loss-B16", "cosine"), ("loss-scales-B17", "pearson"), ("loss-V32784", "pearson")])
def test_head_loss_step_is_deterministic(dev, cid, loss):
    inp = L.inputs_for(cid, loss)
    head, dinp = _head(dev, inp), S._device_inputs(dev, inp)
    first = {k: v.clone() for k, v in _tensors(head, S._step(head, dinp, inp)).items()}
    for v in _tensors(head, None).values():
        if v is not None:
            v.fill_(float("nan"))
    second = _tensors(head, S._step(head, dinp, inp))
    live = (inp["wmask"] != 0).to(dev)
    for k, v in first.items():
        a, b = (v[live], second[k][live]) if k == "stats" else (v, second[k])
        assert torch.equal(a, b), k


@pytest.mark.parametrize("loss", L.LOSSES)
@pytest.mark.parametrize("cid", ["loss-scales", "loss-scales-B17"])
def test_cached_step_is_bit_identical(dev, cid, loss):
    """forward_cached / backward_cached against the uncached step for the same (pooled_raw, sumw), on both dz routes"""
    from phantom_vlb_amd.feature_cache import FeatureCache
    inp = L.inputs_for(cid, loss)
    c = inp["case"]
    B, E = c["B"], c["E"]
    head = _head(dev, inp)
    hidden, wmask, y, keep, _ = S._device_inputs(dev, inp)
    cache = FeatureCache("train", 41, E, dev)
    idx = torch.randperm(41, generator=torch.Generator().manual_seed(B))[:B]
    for ks in (None, keep):
        head.forward(hidden, wmask, y, ks)
        head.backward(need_dhidden=False, loss_scale=0.25, l2_scale=0.5)
        kept = (head.pred, head.loss_terms, head.rowstat, head.loss_aux, head.dz, head.dpooled)
        ref = [t.clone() for t in kept] + [g.clone() for g in head.grads.values()]
        cache.store(idx, head)
        for t in kept + (head.pooled_raw, head.sumw, head.zhat, head.ln2_rstd) + tuple(head.grads.values()):
            t.fill_(float("nan"))
        head.forward_cached(cache, idx, y, ks)
        head.backward_cached(loss_scale=0.25, l2_scale=0.5)
        torch.cuda.synchronize()
        got = list(kept) + list(head.grads.values())
        for i, (a, b) in enumerate(zip(got, ref)):
            assert torch.equal(a, b), i
        cache.valid[:] = False


# ---------------------------------------------------------------------------------------------------- module level
LORA = dict(use_lora=True, freeze_backbone=False, lora_r=16, lora_alpha=32, lora_dropout=0.0)


def _module(p, loss, k=None, **kw):
    from phantom_vlb_amd.litmodule import VLBLitModule, VLBLitModuleConfig
    base = dict(model_path="none", freeze_backbone=True, use_lora=False, lora_r=None, lora_alpha=None, lora_dropout=None,
                dropout_rate=0.0, num_target=128, l2_lambda=1e-3, lr=1e-3, betas=[0.9, 0.999], eps=1e-8, weight_decay=1e-2,
                lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=50000, geometry="mini", loss=loss)
    base.update(kw)
    m = VLBLitModule(VLBLitModuleConfig(**base))
    m.configure_model(state_dict=p)
    opt, _ = m.configure_optimizers()
    if k is not None:
        m.accumulate_grad_batches = k
    return m, opt[0]


@pytest.mark.parametrize("loss", L.LOSSES)
@pytest.mark.parametrize("mode", ["frozen", "lora"])
def test_module_trains_on_the_objective(dev, mode, loss):
    import vlb_oracle as O
    kw = LORA if mode == "lora" else {}
    g = O.geometry_mini(lora_r=16, lora_alpha=32) if mode == "lora" else O.geometry_mini()
    p = O.round_bf16(O.init_params(g, seed=3, lora=True, lora_b_std=0.02) if mode == "lora" else O.init_params(g, seed=3))
    whole = O.synthetic_batch(g, 4, seed=4)
    micro = [{key: v[i * 2:(i + 1) * 2] for key, v in whole.items()} for i in range(2)]
    m, opt = _module(p, loss, 1, **kw)
    assert m.head.loss == loss
    grads = []
    for i, b in enumerate(micro):
        out = m.training_step(b)
        torch.cuda.synchronize()
        grads.append(m.flat.grad.float().clone())
        head = m.head
        pred, rs = head.pred.detach().cpu(), L.rowstat_columns(head.rowstat.detach().cpu())
        y = b["timeseries"].float().to(torch.bfloat16).float()
        # the logged loss = 1 - mean c_b + l2, recomputed in fp64 from the module's own predictions.  c_b: at most
        # rowstat_chain + 3 + 8 roundings of quantities <= 1; l2: the ridge forward's chains (< 128 additions per partial)
        W = head.compute["ridge_layer.linear.weight"].detach().cpu().double()
        l2 = float(head.l2_lambda * (W * W).sum())
        ref = float(L.objective(pred, y, loss)[0]) + l2
        got = float(m.logged["train/brain_loss"])
        bar = (L.rowstat_chain(128) + 11 + 2) * H.U + (128 * H.U + H.R) * l2 + H.R * abs(ref)
        print(f"module {mode} {loss} batch {i}: loss {got:.7f} vs fp64 {ref:.7f} (bar {bar:.1e})")
        assert abs(got - ref) <= bar and float(out) == got
        mse = float(((pred.double() - y.double()) ** 2).mean())
        assert abs(float(m.logged["train/brain_mse"]) - mse) <= 1e-5 * mse
        # d ridge bias = sum_b d pred (closed form, with the device's own row statistics)
        dp, mag = L.dpred(pred, y, rs, 1.0)
        want = L.ridge_bwd_w(dp, mag, head.z.detach().cpu().float(), W, 0.0)
        err = H.ratio(head.grads["ridge_layer.linear.bias"].detach().cpu(), want["dbias"], L.ridge_bwd_w_bars(want, 2)["dbias"])
        assert err <= 1.0, err
    # accumulate_grad_batches = 2: the window's accumulator is the average of the two single-batch gradients, to the
    # rounding of one fp32 addition and of the two scaled terms
    m2, opt2 = _module(p, loss, 2, **kw)
    for b in micro:
        m2.training_step(b)
    torch.cuda.synchronize()
    want, got = (grads[0] + grads[1]) / 2, opt2.accum[0]
    slack = 4 * H.U * (grads[0].abs() + grads[1].abs()) / 2 + 1e-30
    assert bool(((got - want).abs() <= slack).all()), float((got - want).abs().max())
    val = m.validation_step(micro[0])
    assert "val/brain_mse" in m.logged and float(val["loss"]) == float(m.logged["val/brain_loss"])
    # ten optimiser steps on one repeated batch lower the objective
    losses = []
    for _ in range(10):
        losses.append(float(m.training_step(micro[0])))
        opt.step()
    losses.append(float(m.training_step(micro[0])))
    print(f"module {mode} {loss}: objective {losses[0]:.5f} -> {losses[-1]:.5f}")
    assert losses[-1] < losses[0], losses
