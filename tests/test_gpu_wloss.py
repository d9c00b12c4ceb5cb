"""Per-target loss weights and masks of the brain head (BrainHead.set_target_weights) on the GPU, against tests/wloss_emul.py.

Stage by stage: each new kernel (weighted row statistics, the finalize, d pred, and the read-d-pred forms of ridge_bwd_w and
of the two dz routes) is judged on the device's own upstream buffers at its derived fp32 bar, the stages the weights leave
alone by head_emul's own checks, and the whole step against fp64 mathematics at head_emul.E2E_BARS.  Then the promises:
masked targets may hold NaN / Inf and change no bit, their dW rows are the fp32 product l2coef*W and their dbias 0, unit
weights give the unweighted head, every route (plain, packed, cached, tapped, grouped) ends in the same kernels, an unweighted
head never enters the new entry points, and the entry points refuse what they must.  Module level: the mini geometry, frozen
and LoRA.  Run with -s to see max(err / bar)."""
import numpy as np
import pytest
import torch

import head_emul as H
import head_loss_emul as L
import test_gpu_head_stages as S
import wloss_emul as W

pytestmark = pytest.mark.gpu


def _head(dev, inp, weighted=True, loss=None, **kw):
    from phantom_vlb_amd.head import BrainHead
    c = inp["case"]
    G, V, E = c["G"], c["V"], c["E"]
    sd = dict(inp["params"])
    if G:
        sd["ridge_layer.linear.weight"] = sd["ridge_layer.linear.weight"].view(G, V, E)
        sd["ridge_layer.linear.bias"] = sd["ridge_layer.linear.bias"].view(G, V)
    head = BrainHead(E, V, inp["lam"], inp["eps"], dev, sd=sd, loss=inp["loss"] if loss is None else loss,
                     subjects=[f"sub-{g}" for g in range(G)] if G else None, **kw)
    if weighted:
        head.set_target_weights(inp["tw"].to(dev) if G else inp["tw"][0].to(dev))
    return head


def _subject(inp):
    return None if inp["group"] is None else inp["group"].tolist()


def _step(head, dinp, inp, y=None):
    hidden, wmask, y0, keep, lay = dinp
    head.forward(hidden, wmask, y0 if y is None else y, keep, layout=lay, subject=_subject(inp))
    dh = head.backward(need_dhidden=True, loss_scale=inp["loss_scale"], l2_scale=inp["l2_scale"])
    torch.cuda.synchronize()
    return dh


def _tensors(head, dh):
    t = S._device_tensors(head, dh)
    t.update(wstat=head.wstat, loss_aux=head.loss_aux, dpred=head.dpred)
    return t


def _host_buffers(head, dh, inp):
    bufs = S._host_buffers(head, dh, inp)
    bufs.update(W.wstat_columns(head.wstat.detach().cpu()), loss_aux=head.loss_aux.detach().cpu(), dpred=head.dpred.detach().cpu())
    return bufs


def _rel(a, ref):
    a, ref = a.detach().float(), ref.detach().float()
    return float((a - ref).abs().max() / (ref.abs().max() + 1e-12))


def _nan_targets(inp, fill=float("nan")):
    return torch.where(W.clip_weights(inp) > 0, inp["y"], torch.full((), fill))


def _l2_seed(inp):
    """the fp32 product l2coef * W, as ridge_bwd_w_kernel forms it"""
    l2coef = H.host_scales(inp["case"]["B"], inp["case"]["V"], inp["lam"], inp["loss_scale"], inp["l2_scale"])[1]
    return torch.tensor(l2coef, dtype=torch.float32) * inp["params"]["ridge_layer.linear.weight"]


def _masked_rows(inp):
    """[H*V] bool: rows of the stacked ridge weight no clip of the batch trains - weight 0, or a head without a clip"""
    c = inp["case"]
    tw = inp["tw"]
    present = torch.zeros(tw.shape[0], dtype=torch.bool)
    present[[0] if inp["group"] is None else sorted(set(c["group"]))] = True
    return ((tw == 0) | ~present[:, None]).flatten()


# ---------------------------------------------------------------------------------------------------- stage by stage
@pytest.mark.parametrize("cid,loss", W.PAIRS)
def test_wloss_stages(dev, cid, loss):
    inp = W.inputs_for(cid, loss)
    c = inp["case"]
    assert set(c["expect"]) <= H.dispatch(c["B"], c["E"])
    dinp = S._device_inputs(dev, inp)
    plain = _head(dev, inp, weighted=False, loss="mse")              # what the unweighted forward writes
    plain.forward(dinp[0], dinp[1], dinp[2], dinp[3], layout=dinp[4], subject=_subject(inp))
    head = _head(dev, inp)
    dh = _step(head, dinp, inp)
    bufs = _host_buffers(head, dh, inp)
    assert all(bool(torch.isfinite(v.float()).all()) for v in bufs.values())
    assert torch.equal(head.pred, plain.pred), "pred is not the unweighted forward's, bit for bit"
    assert torch.equal(head.loss_terms[1], plain.loss_terms[1]), "loss_terms[1] is not the plain forward's l2, bit for bit"
    ratios = {**W.check_stages(bufs, inp), **W.check_rest(bufs, inp)}
    print(f"wloss-stages {cid} {loss}: " + " ".join(f"{k}={v:.3f}" for k, v in H.by_stage(ratios).items()))
    print(f"wloss-stages-detail {cid} {loss}: " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (cid, loss, bad)
    # a masked target, and a head without a clip: dW is the fp32 product l2coef * W, dbias is 0, exactly
    rows = _masked_rows(inp)
    assert bool(rows.any()) == (c["V"] > 2)                  # V = 1, 2: every target carries weight (pearson needs two)
    assert torch.equal(bufs["dW"].reshape(-1, c["E"])[rows], _l2_seed(inp)[rows]), "a masked row of dW is not l2coef * W"
    assert bool((bufs["dbias"].flatten()[rows] == 0).all()), "a masked target has a dbias"
    e2e, bars = W.end_to_end(bufs, inp), H.E2E_BARS
    print(f"wloss-e2e {cid} {loss}: " + " ".join(f"{k}={v:.2e}/{bars[k]:.0e}" for k, v in e2e.items()))
    bad = {k: (v, bars[k]) for k, v in e2e.items() if not v < bars[k]}
    assert not bad, (cid, loss, bad)


# ---------------------------------------------------------------------------------------------------- masked targets
@pytest.mark.parametrize("cid,loss", [("w-V17", "mse"), ("w-V5", "cosine"), ("w-V1030", "pearson"), ("w-G3", "cosine"),
                                      ("w-G3-B17", "pearson"), ("w-packed", "mse")])
def test_nan_and_inf_at_masked_targets_change_no_bit(dev, cid, loss):
    """... and a repeated step is bit-equal (the zeros run twice)"""
    inp = W.inputs_for(cid, loss)
    head, dinp = _head(dev, inp), S._device_inputs(dev, inp)
    live = (inp["wmask"] != 0).to(dev)
    first = None
    for fill in (0.0, 0.0, float("nan"), float("inf"), float("-inf")):
        for v in _tensors(head, None).values() if first is not None else ():
            if v is not None:
                v.fill_(float("nan"))
        y = _nan_targets(inp, fill).to(dev)
        got = _tensors(head, _step(head, dinp, inp, y=y))
        assert bool(torch.isfinite(head.loss_terms).all()) and all(bool(torch.isfinite(g).all()) for g in head.grads.values())
        if first is None:
            first = {k: v.clone() for k, v in got.items()}
            continue
        for k, v in first.items():
            a, b = (v[live], got[k][live]) if k == "stats" else (v, got[k])
            assert torch.equal(a, b), (k, fill)


# ---------------------------------------------------------------------------------------------------- unit weights
@pytest.mark.parametrize("cid,loss", [("w-V17", "mse"), ("w-V5", "cosine"), ("w-V300", "pearson"), ("w-V1030", "mse"), ("w-G3", "pearson")])
def test_unit_weights_give_the_unweighted_head(dev, cid, loss):
    """tw = 1: pred and loss_terms[1] in the unweighted head's bits; the data term within the sum of the two kernels' derived
    bars around the fp64 value from the (shared) pred; the weighted stages inside wloss_emul's bars with unit weights, and
    every gradient within head_emul's end-to-end bars of the unweighted head's"""
    inp = dict(W.inputs_for(cid, loss))
    inp["tw"] = torch.ones_like(inp["tw"])
    c = inp["case"]
    B, E, V = c["B"], c["E"], c["V"]
    dinp = S._device_inputs(dev, inp)
    plain = _head(dev, inp, weighted=False)
    dhp = _step(plain, dinp, inp)
    head = _head(dev, inp)
    dh = _step(head, dinp, inp)
    assert torch.equal(head.pred, plain.pred) and torch.equal(head.loss_terms[1], plain.loss_terms[1])
    bufs = _host_buffers(head, dh, inp)
    ratios = W.check_stages(bufs, inp)
    assert all(v <= 1.0 for v in ratios.values()), ratios
    pred, y = bufs["pred"], inp["y"]
    chain = L.rowstat_chain(V)
    if loss == "mse":
        ref = float(((pred.double() - y.double()) ** 2).mean())
        rr = H.ridge(bufs["z"], inp["params"]["ridge_layer.linear.weight"], inp["params"]["ridge_layer.linear.bias"], y, inp["lam"],
                     pred_for_loss=pred)
        bar = float(H.ridge_bars(rr, B, E, V)["loss"][0]) + ((2 * chain + 5 + 2) * H.U + H.R) * ref
    else:
        rs = L.rowstat(pred, y, loss)
        ref = float(1 - rs["c"].sum() / B)
        # c_b of either kernel: its three sums at (chain + 4) roundings of sum|w u t| relative to nu nt, the 8 of the quotient
        rel = ((chain + 4) * H.U + H.R) * (rs["mag_ut"] / (rs["suu"].sqrt() * rs["stt"].sqrt()).clamp_min(1e-300) + rs["c"].abs()) + 8 * H.U * rs["c"].abs()
        bar = 2 * (float(rel.sum() / B) + 2 * H.U * (1 + abs(1 - ref)) + H.R * abs(ref))
    got, unw = float(head.loss_terms[0]), float(plain.loss_terms[0])
    print(f"wloss-ones {cid} {loss}: data term {got:.8f} vs unweighted {unw:.8f} (fp64 {ref:.8f}, bar {bar:.1e})")
    assert abs(got - unw) <= bar and abs(got - ref) <= bar
    for n, g in head.grads.items():
        assert _rel(g, plain.grads[n]) < H.E2E_BARS[H.GRAD_KEYS[n]], n
    assert _rel(dh, dhp) < H.E2E_BARS["dh"]


# ---------------------------------------------------------------------------------------------------- every route
@pytest.mark.parametrize("cid,loss", [("w-V300", "pearson"), ("w-V1030", "mse"), ("w-G3", "cosine"), ("w-G3-B17", "mse")])
def test_cached_step_is_bit_identical(dev, cid, loss):
    """forward_cached / backward_cached against the uncached step for the same (pooled_raw, sumw): one head and grouped, both dz routes"""
    from phantom_vlb_amd.feature_cache import FeatureCache
    inp = W.inputs_for(cid, loss)
    c = inp["case"]
    B, E = c["B"], c["E"]
    head = _head(dev, inp)
    hidden, wmask, y, keep, _ = S._device_inputs(dev, inp)
    y = _nan_targets(inp).to(dev)
    cache = FeatureCache("train", 41, E, dev)
    idx = torch.randperm(41, generator=torch.Generator().manual_seed(B))[:B]
    head.forward(hidden, wmask, y, keep, subject=_subject(inp))
    head.backward(need_dhidden=False, loss_scale=0.25, l2_scale=0.5)
    kept = (head.pred, head.loss_terms, head.wstat, head.loss_aux, head.dpred, head.dz, head.dpooled)
    ref = [t.clone() for t in kept] + [g.clone() for g in head.grads.values()]
    cache.store(idx, head)
    for t in kept + (head.pooled_raw, head.sumw, head.zhat, head.ln2_rstd) + tuple(head.grads.values()):
        t.fill_(float("nan"))
    head.forward_cached(cache, idx, y, keep, subject=_subject(inp))
    head.backward_cached(loss_scale=0.25, l2_scale=0.5)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(list(kept) + list(head.grads.values()), ref)):
        assert torch.equal(a, b), i
    bufs = {k: v.detach().cpu() for k, v in dict(z=head.z, pred=head.pred, loss_terms=head.loss_terms, loss_aux=head.loss_aux,
                                                   dpred=head.dpred, dz=head.dz).items()}
    bufs.update(W.wstat_columns(head.wstat.detach().cpu()), dW=head.grads["ridge_layer.linear.weight"].detach().cpu(),
                dbias=head.grads["ridge_layer.linear.bias"].detach().cpu())
    ratios = W.check_stages(bufs, dict(inp, loss_scale=0.25, l2_scale=0.5), y=y.cpu())
    assert all(v <= 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("cid,loss", [("w-V17", "pearson"), ("w-V5", "mse"), ("w-G3", "mse")])
def test_tapped_route(dev, cid, loss):
    """readout_layers with K = 2: the tail of forward_tapped / backward_tapped ends in the same new stages, judged on the
    device's own buffers; the taps' d hidden come out finite"""
    inp = W.inputs_for(cid, loss)
    c = inp["case"]
    B, Sq = c["B"], c["S"]
    head = _head(dev, inp, readout_layers=(1, 2))
    hidden, wmask, y, keep, lay = S._device_inputs(dev, inp)
    taps = (hidden, hidden.flip(0).contiguous())
    head.begin(B, Sq)
    for i, h in enumerate(taps):
        head.tap(i, h, wmask, lay)
    head.forward_tapped(y, keep, subject=_subject(inp))
    head.backward_tapped(loss_scale=inp["loss_scale"], l2_scale=inp["l2_scale"])
    dx = head.dhidden(1, taps[1])
    head.dhidden(0, taps[0], into=dx)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dx.float()).all()) and bool(torch.isfinite(head.grads["layer_mix.weight"]).all())
    bufs = {k: v.detach().cpu() for k, v in dict(z=head.z, pred=head.pred, loss_terms=head.loss_terms, loss_aux=head.loss_aux,
                                                   dpred=head.dpred, dz=head.dz).items()}
    bufs.update(W.wstat_columns(head.wstat.detach().cpu()), dW=head.grads["ridge_layer.linear.weight"].detach().cpu(),
                dbias=head.grads["ridge_layer.linear.bias"].detach().cpu())
    ratios = W.check_stages(bufs, inp)
    print(f"wloss-tapped {cid} {loss}: " + " ".join(f"{k}={v:.3f}" for k, v in H.by_stage(ratios).items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios


def test_weights_compose_with_a_penalty_per_row(dev):
    """set_l2_lambda_rows: the penalty is separate - the data term keeps its bits, d ridge bias too, and a masked row's dW
    is the per-row penalty's gradient alone"""
    inp = W.inputs_for("w-V17", "mse")
    c = inp["case"]
    head, dinp = _head(dev, inp), S._device_inputs(dev, inp)
    _step(head, dinp, inp)
    data, dbias = head.loss_terms[0].clone(), head.grads["ridge_layer.linear.bias"].clone()
    lam = torch.linspace(0.0, 2e-3, c["V"], device=dev)
    head.set_l2_lambda_rows(lam)
    _step(head, dinp, inp)
    assert torch.equal(head.loss_terms[0], data) and torch.equal(head.grads["ridge_layer.linear.bias"], dbias)
    Wt = head.compute["ridge_layer.linear.weight"].float()
    want = float((lam.double()[:, None] * Wt.double() ** 2).sum())
    assert abs(float(head.loss_terms[1]) - want) <= 1e-5 * want
    rows = (inp["tw"][0] == 0).to(dev)
    got, ref = head.grads["ridge_layer.linear.weight"][rows], (2.0 * lam[:, None] * Wt)[rows]
    assert float((got - ref).abs().max()) <= 4 * H.U * float(ref.abs().max())
    with pytest.raises(ValueError, match="target weights"):
        head.ridge_stats_begin()


# ---------------------------------------------------------------------------------------------------- unweighted is untouched
NEW = ("vlb_head_wloss_fwd", "vlb_head_bwd_wloss")


@pytest.mark.parametrize("cid", ["w-V17", "w-G3"])
def test_an_unweighted_head_never_enters_the_new_entry_points(dev, monkeypatch, cid):
    from phantom_vlb_amd import _lib
    from phantom_vlb_amd.feature_cache import FeatureCache

    def refuse(*a):
        raise AssertionError("a weighted-loss entry point was called")
    for name in NEW:
        monkeypatch.setattr(_lib.lib, name, refuse)
    for loss in W.LOSSES:
        inp = W.inputs_for(cid, loss)
        c = inp["case"]
        hidden, wmask, y, keep, lay = S._device_inputs(dev, inp)
        head = _head(dev, inp, weighted=False)
        assert head.tw is None
        head.forward(hidden, wmask, y, keep, layout=lay, subject=_subject(inp))
        head.backward(need_dhidden=True)
        cache = FeatureCache("train", 32, c["E"], dev)
        idx = torch.arange(c["B"])
        cache.store(idx, head)
        head.forward_cached(cache, idx, y, keep, subject=_subject(inp))
        head.backward_cached()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(head.loss_terms).all())
        head.set_target_weights(inp["tw"].to(dev))
        with pytest.raises(AssertionError, match="weighted-loss entry point"):      # ... and the replacement does bite
            head.forward(hidden, wmask, y, keep, layout=lay, subject=_subject(inp))
        head.set_target_weights(None)                                               # back on the unweighted path
        head.forward(hidden, wmask, y, keep, layout=lay, subject=_subject(inp))
        head.backward(need_dhidden=False)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals(dev):
    from phantom_vlb_amd._lib import VlbError, check, lib
    from phantom_vlb_amd.ops import _stream
    inp = W.inputs_for("w-V17", "pearson")
    V = inp["case"]["V"]
    hidden, wmask, y, keep, lay = S._device_inputs(dev, inp)
    head = _head(dev, inp)
    tw = inp["tw"][0].to(dev)
    for bad, what in ((tw[:-1], "fp32 tensor"), (tw.double(), "fp32 tensor"), (tw.cpu(), "fp32 tensor"), (tw.expand(2, V), "fp32 tensor")):
        with pytest.raises(ValueError, match=what):
            head.set_target_weights(bad)
    for val in (-1.0, float("nan"), float("inf")):
        bad = tw.clone()
        bad[3] = val
        with pytest.raises(ValueError, match="the head, target 3"):
            head.set_target_weights(bad)
    one = torch.zeros(V, device=dev)
    one[4] = 2.0
    with pytest.raises(ValueError, match="1 target.*pearson.*at least 2"):
        head.set_target_weights(one)
    _head(dev, inp, weighted=False, loss="cosine").set_target_weights(one)          # one positive weight serves cosine and mse
    with pytest.raises(ValueError, match="0 target"):
        _head(dev, inp, weighted=False, loss="mse").set_target_weights(torch.zeros(V, device=dev))
    g3 = W.inputs_for("w-G3", "mse")
    hg = _head(dev, g3, weighted=False)
    bad = g3["tw"].clone()
    bad[1] = 0
    with pytest.raises(ValueError, match=r"head 1 \('sub-1'\)"):
        hg.set_target_weights(bad.to(dev))
    assert head.tw is not None and torch.equal(head.tw, tw[None])                   # refusals left the weights as they were
    # the entry points themselves
    head.forward(hidden, wmask, y, keep, layout=lay)
    B, Sq = wmask.shape

    def fwd(tw_ptr=None, wstat_ptr=None, group=None, S_=Sq, V_=V, G=1, kind=2):
        check(lib.vlb_head_wloss_fwd(head.pred.data_ptr(), y.data_ptr(), head.tw.data_ptr() if tw_ptr is None else tw_ptr, group,
                                     head.ws.data_ptr(), head.wstat.data_ptr() if wstat_ptr is None else wstat_ptr,
                                     head.loss_terms.data_ptr(), head.loss_aux.data_ptr(), B, S_, head.E, V_, G, kind, head.l2_lambda,
                                     _stream()), "vlb_head_wloss_fwd")
    fwd()
    empty = torch.empty(0, device=dev)                                              # data_ptr() == 0
    for kw, what in ((dict(tw_ptr=empty.data_ptr()), "null"), (dict(wstat_ptr=empty.data_ptr()), "null"), (dict(V_=0), "bad shape"),
                     (dict(V_=1), "pearson"), (dict(kind=3), "unknown"), (dict(G=0), "bad shape"), (dict(G=2), "group"),
                     (dict(group=head.wstat.data_ptr(), G=2), "group")):
        with pytest.raises(VlbError, match=what):
            fwd(**kw)
    head.wstat = empty
    with pytest.raises(VlbError, match="null"):
        head.backward(need_dhidden=False)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- module level
LORA = dict(use_lora=True, freeze_backbone=False, lora_r=16, lora_alpha=32, lora_dropout=0.0)


def _module(p, loss, k=None, head_state=None, **kw):
    from phantom_vlb_amd.litmodule import VLBLitModule, VLBLitModuleConfig
    base = dict(model_path="none", freeze_backbone=True, use_lora=False, lora_r=None, lora_alpha=None, lora_dropout=None,
                dropout_rate=0.0, num_target=128, l2_lambda=1e-3, lr=1e-3, betas=[0.9, 0.999], eps=1e-8, weight_decay=1e-2,
                lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=50000, geometry="mini", loss=loss)
    base.update(kw)
    m = VLBLitModule(VLBLitModuleConfig(**base))
    m.configure_model(state_dict=p, head_state=head_state)
    opt, _ = m.configure_optimizers()
    if k is not None:
        m.accumulate_grad_batches = k
    return m, opt[0]


def _masked_batch(batch, w):
    """the batch with NaN targets wherever the clip's weight row (w [B,V]) is 0"""
    ts = batch["timeseries"].float()
    return dict(batch, timeseries=torch.where(w > 0, ts, torch.full((), float("nan"))).to(batch["timeseries"].dtype))


@pytest.mark.parametrize("mode,loss,mask", [("frozen", "mse", True), ("frozen", "pearson", False), ("lora", "cosine", True)])
def test_module_trains_on_the_weighted_objective(dev, mode, loss, mask, tmp_path):
    import vlb_oracle as O
    kw = LORA if mode == "lora" else {}
    g = O.geometry_mini(lora_r=16, lora_alpha=32) if mode == "lora" else O.geometry_mini()
    p = O.round_bf16(O.init_params(g, seed=3, lora=True, lora_b_std=0.02) if mode == "lora" else O.init_params(g, seed=3))
    tw = W.make_weights(128, 77)
    if mask:
        tw = (tw > 0).float()                                       # a 0/1 mask, and NaN targets under it
    np.save(tmp_path / "tw.npy", tw.numpy())
    kw = dict(kw, target_weights=str(tmp_path / "tw.npy"))          # through the config: configure_model loads the file
    w4 = tw[None].expand(4, -1)
    whole = _masked_batch(O.synthetic_batch(g, 4, seed=4), w4)
    micro = [{key: v[i * 2:(i + 1) * 2] for key, v in whole.items()} for i in range(2)]
    m, opt = _module(p, loss, 1, **kw)
    assert m.head.loss == loss and torch.equal(m.head.tw.cpu(), tw[None])
    grads = []
    chain = L.rowstat_chain(128)
    for i, b in enumerate(micro + [whole]):
        out = m.training_step(b)
        torch.cuda.synchronize()
        grads.append(m.flat.grad.float().clone())
        head = m.head
        B = len(b["timeseries"])
        pred = head.pred.detach().cpu()
        y = b["timeseries"].float().to(torch.bfloat16).float().cpu()
        # the logged loss = the weighted data term + l2, recomputed in fp64 from the module's own predictions
        Wt = head.compute["ridge_layer.linear.weight"].detach().cpu().double()
        l2 = float(head.l2_lambda * (Wt * Wt).sum())
        rs = W.rowstat(pred, y, w4[:B], loss)
        data = float(W.loss_terms(rs["m"], rs["c"], torch.zeros((), dtype=torch.float64), loss)["loss"][0])
        ref, got = data + l2, float(m.logged["train/brain_loss"])
        # mse: m_b at (2 chain + 5) relative, the mean's rounding 2; cosine / pearson: c_b from sums at (chain + 4) of
        # quantities <= 1 and the quotient's 8, the mean's rounding 2; l2: the ridge forward's chains (< 128 additions)
        bar = ((2 * chain + 7) * H.U * data if loss == "mse" else (chain + 14) * H.U) + (128 * H.U + H.R) * l2 + H.R * abs(ref)
        print(f"wloss-module {mode} {loss} batch {i}: loss {got:.7f} vs fp64 {ref:.7f} (bar {bar:.1e})")
        assert abs(got - ref) <= bar and float(out) == got
        assert abs(float(m.logged["train/brain_mse"]) - float(rs["m"].mean())) <= 1e-5 * float(rs["m"].mean())
        assert bool(torch.isfinite(grads[-1]).all())
    # accumulate_grad_batches = 2: the window's accumulator is the average of the two single-batch gradients, to the rounding
    # of one fp32 addition and of the two scaled terms ...
    m2, opt2 = _module(p, loss, 2, **kw)
    for b in micro:
        m2.training_step(b)
    torch.cuda.synchronize()
    want, got = (grads[0] + grads[1]) / 2, opt2.accum[0]
    slack = 4 * H.U * (grads[0].abs() + grads[1].abs()) / 2 + 1e-30
    assert bool(((got - want).abs() <= slack).all()), float((got - want).abs().max())
    # ... and, each clip being normalised by its own W_b, the gradient of ONE batch of both (max-norm relative, at head_emul's
    # end-to-end bar for a gradient: the two differ by summation order and bf16 roundings only)
    assert _rel(got, grads[2]) < H.E2E_BARS["dW"], _rel(got, grads[2])
    val = m.validation_step(micro[0])
    assert "val/brain_mse" in m.logged and float(val["loss"]) == float(m.logged["val/brain_loss"])
    ck = {}
    m.on_save_checkpoint(ck)
    assert torch.equal(ck["vlb_target_weights"], tw[None])
    # ten optimiser steps on one repeated batch (NaN under the mask) stay finite and lower the objective
    losses = []
    for _ in range(10):
        losses.append(float(m.training_step(micro[0])))
        opt.step()
    losses.append(float(m.training_step(micro[0])))
    torch.cuda.synchronize()
    print(f"wloss-module {mode} {loss}: objective {losses[0]:.5f} -> {losses[-1]:.5f}")
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert all(bool(torch.isfinite(t).all()) for t in m.head.master.values())


def test_module_scores_each_subject_on_its_own_targets(dev):
    """two subjects with their own masks: the step runs the grouped tail into the weighted stages, and the validation callback
    logs val_corr_avg/<subject> over that subject's kept targets only"""
    import vlb_oracle as O
    from phantom_vlb_amd.utils import LogValAccuracyCallback
    g = O.geometry_mini()
    p = O.round_bf16(O.init_params(g, seed=1234))
    names = ["sub-01", "sub-02"]
    W_, B_ = "ridge_layer.linear.weight", "ridge_layer.linear.bias"
    hs = {n: p[n] for n in p if n.startswith(("layer_norm1", "layer_norm2"))}
    hs[W_], hs[B_] = torch.stack([p[W_], p[W_].flip(0)]), torch.stack([p[B_], p[B_].flip(0)])      # a second head: the first's rows reversed
    m, opt = _module(p, "mse", head_state=hs, subjects=names)
    tw = torch.stack([(W.make_weights(128, 5) > 0).float(), (W.make_weights(128, 6) > 0).float()])
    assert not torch.equal(tw[0], tw[1])
    m.set_target_weights(tw)
    assert torch.equal(m.head.tw.cpu(), tw) and m.target_weight_mask().tolist() == (tw > 0).tolist()
    subj = torch.tensor([0, 1, 1, 0])
    batches = [_masked_batch(dict(O.synthetic_batch(g, 4, seed=s), subject=subj), tw[subj]) for s in (11, 12)]
    loss = m.training_step(batches[0])
    opt.step()
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and all(bool(torch.isfinite(t).all()) for t in m.head.master.values())
    cb = LogValAccuracyCallback()
    cb.on_validation_epoch_start(None, m)
    preds, ys = [], []
    for i, b in enumerate(batches):
        out = m.validation_step(b)
        cb.on_validation_batch_end(None, m, out, b, i)
        preds.append(out["brain_preds"].detach().double().cpu())
        ys.append(out["brain_vals"].detach().double().cpu())
    cb.on_validation_epoch_end(None, m)
    torch.cuda.synchronize()
    pred, y, s = torch.cat(preds).numpy(), torch.cat(ys).numpy(), torch.cat([subj, subj]).numpy()
    for gi, name in enumerate(names):
        keep = (tw[gi] > 0).numpy()
        pk, yk = pred[s == gi][:, keep], y[s == gi][:, keep]
        pk, yk = pk - pk.mean(0), yk - yk.mean(0)
        ref = ((pk * yk).sum(0) / np.sqrt((pk * pk).sum(0) * (yk * yk).sum(0))).mean()
        assert abs(float(m.logged[f"val_corr_avg/{name}"]) - ref) < 1e-5, (name, float(m.logged[f"val_corr_avg/{name}"]), ref)
        assert torch.isnan(cb.correlations[gi]).cpu().tolist() == (~keep).tolist()
        rois = sorted(k for k in m.logged if k.startswith("val_corr_ROI_") and k.endswith("/" + name))
        assert rois == [f"val_corr_ROI_{i:06d}/{name}" for i in np.nonzero(keep)[0]]
