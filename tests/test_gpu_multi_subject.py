"""Per-subject ridge heads on one trunk (``BrainHead(subjects=[...])``, vlb_head_fwd_grouped / vlb_head_bwd_grouped), on the
device: every grouped kernel against the fp64 staged reference of tests/group_emul.py on the device's own upstream buffers,
the exact relations the grouped entries promise (G = 1 == ungrouped, a head's rows == an ungrouped head holding that head,
absent heads, repeatability, cached == uncached, tapped), the module against the live CPU oracle with each clip's own W_g,
and the trainer on the two-subject synthetic experiment.  Run with -s to see max(err / bar)."""
import os
import subprocess
import sys

import pytest
import torch

import group_emul as GE
import head_emul as H
import head_loss_emul as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sub-01", "sub-02", "sub-03", "sub-05", "sub-06", "sub-04")
W_, B_ = "ridge_layer.linear.weight", "ridge_layer.linear.bias"


def _head(dev, inp, loss="mse", readout_layers=None):
    from phantom_vlb_amd.head import BrainHead
    c = inp["case"]
    return BrainHead(c["E"], c["V"], inp["lam"], inp["eps"], dev, sd=inp["params"], loss=loss, subjects=list(NAMES[:c["G"]]),
                     readout_layers=readout_layers)


def _single(dev, inp, g, loss="mse", readout_layers=None):
    from phantom_vlb_amd.head import BrainHead
    c = inp["case"]
    return BrainHead(c["E"], c["V"], inp["lam"], inp["eps"], dev, sd=GE.single_head_inputs(inp, g)["params"], loss=loss,
                     readout_layers=readout_layers)


def _dinp(dev, inp):
    c = inp["case"]
    keep = None if inp["keep"] is None else inp["keep"].to(dev)
    return inp["hidden"].view(c["B"] * c["S"], c["E"]).to(dev), inp["wmask"].to(dev), inp["y"].to(dev), keep


def _step(head, dinp, inp, need_dh=True):
    hidden, wmask, y, keep = dinp
    head.forward(hidden, wmask, y, keep, subject=inp["group"] if head.G else None)
    dh = head.backward(need_dhidden=need_dh, loss_scale=inp["loss_scale"], l2_scale=inp["l2_scale"])
    torch.cuda.synchronize()
    return dh


def _tensors(head, dh=None):
    t = dict(pooled_raw=head.pooled_raw, sumw=head.sumw, zhat=head.zhat, ln2_rstd=head.ln2_rstd, z=head.z, pred=head.pred,
             loss_terms=head.loss_terms, dz=head.dz, dpooled=head.dpooled)
    if head.loss_kind:
        t.update(rowstat=head.rowstat, loss_aux=head.loss_aux)
    if dh is not None:
        t["dh"] = dh
    t.update({H.GRAD_KEYS[n]: g for n, g in head.grads.items() if n in H.GRAD_KEYS})
    return t


def _host(head, dh=None):
    bufs = {k: v.detach().cpu() for k, v in _tensors(head, dh).items()}
    if "rowstat" in bufs:
        bufs.update(L.rowstat_columns(bufs.pop("rowstat")))
    return bufs


# ---------------------------------------------------------------------------------------------------- stage checks
_STAGE_RUNS = [(c["id"], "mse") for c in GE.CASES] + [(cid, k) for cid in GE.LOSS_CASES for k in L.LOSSES]


@pytest.mark.parametrize("cid,loss", _STAGE_RUNS)
def test_grouped_stages(dev, cid, loss):
    inp = GE.inputs_for(cid, loss)
    c = inp["case"]
    assert set(c["expect"]) <= GE.dispatch(c["B"], c["E"], c["G"]), f"{cid} no longer reaches {set(c['expect']) - GE.dispatch(c['B'], c['E'], c['G'])}"
    head = _head(dev, inp, loss)
    dh = _step(head, _dinp(dev, inp), inp)
    ratios = GE.check_stages(_host(head, dh), inp)
    print(f"grouped-stages {cid} {loss}: " + " ".join(f"{k}={v:.3f}" for k, v in GE.by_stage(ratios).items()))
    print(f"grouped-stages-detail {cid} {loss}: " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (cid, loss, bad)


# ---------------------------------------------------------------------------------------------------- exact relations
@pytest.mark.parametrize("case", GE.G1_CASES, ids=lambda c: c["id"])
@pytest.mark.parametrize("loss", ("mse",) + L.LOSSES)
def test_one_group_gives_the_ungrouped_bits(dev, case, loss):
    """vlb_head_fwd_grouped / vlb_head_bwd_grouped called with G = 1 against vlb_head_fwd_cached (+ vlb_head_loss_fwd) /
    vlb_head_bwd_cached[_loss] on the same (pooled_raw, sumw): every output bit-equal.  The two sides are the GROUPED = true
    and GROUPED = false instantiations of ONE kernel template each: a real test of that switch (the (head, row) split, the
    `group` test, the row offsets), but no anchor for the arithmetic the two share - that is test_gpu_head_ridge_bits.py,
    which holds both to bits recorded from the library in which they were separate kernels"""
    from phantom_vlb_amd.head import BrainHead
    inp = H.make_inputs(case)
    E, V, B = case["E"], case["V"], case["B"]
    plain = BrainHead(E, V, inp["lam"], inp["eps"], dev, sd=inp["params"], loss=loss)
    hidden, wmask, y, keep = _dinp(dev, inp)
    plain.forward(hidden, wmask, y, keep)
    plain.backward(need_dhidden=False, loss_scale=inp["loss_scale"], l2_scale=inp["l2_scale"])
    ref = {k: v.clone() for k, v in _tensors(plain).items()}
    # the grouped entries driven by hand on the same head: G = 1, group all zero, rows = identity
    g = plain
    g.G, group = 1, torch.zeros(B, dtype=torch.int32, device=dev)
    from phantom_vlb_amd._lib import lib
    g.gws = torch.empty(lib.vlb_head_grouped_ws_floats(B, E, V, 1), dtype=torch.float32, device=dev)
    src, srcw = plain.pooled_raw.clone(), plain.sumw.clone()
    rows = torch.arange(B, dtype=torch.int32, device=dev)
    for t in _tensors(g).values():
        t.fill_(float("nan"))
    g._tail(src, srcw, rows, B, y, keep, group)
    g._backward_tail(inp["loss_scale"], inp["l2_scale"])
    torch.cuda.synchronize()
    for k, v in _tensors(g).items():
        assert torch.equal(v, ref[k]), (case["id"], loss, k)


@pytest.mark.parametrize("cid", [c["id"] for c in GE.CASES])
def test_a_heads_rows_are_the_ungrouped_heads_bits(dev, cid):
    """for each head g: pred rows of g's clips == an ungrouped head holding (W[g], b[g]) run on the whole batch; an absent
    head's dW is the fp32 product l2coef * W[g] and its dbias is 0; a repeated step gives the same bits"""
    inp = GE.inputs_for(cid)
    c = inp["case"]
    dinp = _dinp(dev, inp)
    head = _head(dev, inp)
    _step(head, dinp, inp, need_dh=False)
    first = {k: v.clone() for k, v in _tensors(head).items()}
    for g, idx in enumerate(GE.clips_of(inp["group"], c["G"])):
        if idx.numel():
            one = _single(dev, inp, g)
            one.forward(*dinp)
            torch.cuda.synchronize()
            assert torch.equal(first["pred"][idx.to(dev)], one.pred[idx.to(dev)]), (cid, g)
        else:
            l2coef = torch.tensor(H.host_scales(c["B"], c["V"], inp["lam"], inp["loss_scale"], inp["l2_scale"])[1], dtype=torch.float32)
            want = l2coef.to(dev) * head.compute[W_][g].float()
            assert torch.equal(first["dW"][g], want), (cid, g)
            assert bool((first["dbias"][g] == 0).all()), (cid, g)
    for t in _tensors(head).values():
        t.fill_(float("nan"))
    _step(head, dinp, inp, need_dh=False)
    for k, v in _tensors(head).items():
        assert torch.equal(v, first[k]), (cid, k)


@pytest.mark.parametrize("cid", ["g3-B5", "g3-B17"])
def test_grouped_cached_step_equals_the_uncached_one(dev, cid):
    from phantom_vlb_amd.feature_cache import FeatureCache
    inp = GE.inputs_for(cid)
    c = inp["case"]
    B, E = c["B"], c["E"]
    head, dinp = _head(dev, inp), _dinp(dev, inp)
    _step(head, dinp, inp, need_dh=False)
    ref = {k: v.clone() for k, v in _tensors(head).items()}
    cache = FeatureCache("train", 41, E, dev)
    idx = torch.randperm(41, generator=torch.Generator().manual_seed(B))[:B]
    cache.store(idx, head)
    for t in _tensors(head).values():
        t.fill_(float("nan"))
    head.forward_cached(cache, idx, dinp[2], dinp[3], subject=inp["group"])
    head.backward_cached(loss_scale=inp["loss_scale"], l2_scale=inp["l2_scale"])
    torch.cuda.synchronize()
    for k, v in _tensors(head).items():
        assert torch.equal(v, ref[k]), (cid, k)


def test_grouped_tapped_rows_are_the_ungrouped_tapped_heads_bits(dev):
    """subjects + readout_layers (K = 2, a synthetic second hidden tensor): pred rows of head g == the ungrouped tapped head
    holding W[g]; the mix gradient and d hidden of both taps come out finite"""
    inp = GE.inputs_for("g3-B5")
    c = inp["case"]
    B, S, E, G = c["B"], c["S"], c["E"], c["G"]
    hidden, wmask, y, keep = _dinp(dev, inp)
    gen = torch.Generator().manual_seed(5)
    second = (inp["hidden"].float() * 0.5 + torch.randn(B, S, E, generator=gen)).to(torch.bfloat16).view(B * S, E).to(dev)
    mix = {"layer_mix.weight": torch.tensor([0.25, -0.5])}

    def tapped(head, subject):
        head.begin(B, S)
        head.tap(0, hidden, wmask)
        head.tap(1, second, wmask)
        pred, _ = head.forward_tapped(y, keep, **({"subject": subject} if subject is not None else {}))
        head.backward_tapped()
        dx = head.dhidden(1, second)
        head.dhidden(0, hidden, into=dx)
        torch.cuda.synchronize()
        return pred.clone(), dx

    from phantom_vlb_amd.head import BrainHead
    grouped = BrainHead(E, c["V"], inp["lam"], inp["eps"], dev, sd=dict(inp["params"], **mix), subjects=list(NAMES[:G]),
                        readout_layers=(1, 2))
    pred, dx = tapped(grouped, inp["group"])
    assert bool(torch.isfinite(dx.float()).all()) and bool(torch.isfinite(grouped.grads["layer_mix.weight"]).all())
    for g, idx in enumerate(GE.clips_of(inp["group"], G)):
        one = BrainHead(E, c["V"], inp["lam"], inp["eps"], dev, sd=dict(GE.single_head_inputs(inp, g)["params"], **mix),
                        readout_layers=(1, 2))
        p1, _ = tapped(one, None)
        assert torch.equal(pred[idx.to(dev)], p1[idx.to(dev)]), g


def test_subject_is_checked_on_the_host(dev):
    inp = GE.inputs_for("g3-B5")
    head, (hidden, wmask, y, keep) = _head(dev, inp), _dinp(dev, inp)
    for bad in ([0, 1, 2, 3, 0], [0, 1, -1, 0, 0], [0, 1], None):
        with pytest.raises(ValueError, match="subject"):
            head.forward(hidden, wmask, y, keep, subject=bad)
    one = _single(dev, inp, 0)
    with pytest.raises(ValueError, match="subject"):
        one.forward(hidden, wmask, y, keep, subject=[0] * 5)
    sd = head.subject_state_dict("sub-02")
    assert tuple(sd[W_].shape) == (inp["case"]["V"], inp["case"]["E"]) and torch.equal(sd[W_].cpu(), inp["params"][W_][1])
    assert torch.equal(head.subject_state_dict(2)[B_].cpu(), inp["params"][B_][2])


# ---------------------------------------------------------------------------------------------------- the module
def _cfg(lora=False, **kw):
    from phantom_vlb_amd.litmodule import VLBLitModuleConfig
    base = dict(model_path="none", freeze_backbone=not lora, use_lora=lora, lora_r=16 if lora else None,
                lora_alpha=32 if lora else None, lora_dropout=0.0 if lora else None, dropout_rate=0.0,
                num_target=128, l2_lambda=1e-3, lr=1e-4, betas=[0.9, 0.999], eps=1e-8, weight_decay=1e-2,
                lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=50000, geometry="mini")
    base.update(kw)
    return VLBLitModuleConfig(**base)


def _two_heads(p, seed=99):
    """the oracle's parameters with a second, differently drawn ridge head stacked behind its own: [2,V,E] / [2,V]"""
    gen = torch.Generator().manual_seed(seed)
    W0, b0 = p[W_], p[B_]
    W1 = ((torch.rand(W0.shape, generator=gen) * 2 - 1) / W0.shape[1] ** 0.5).to(torch.bfloat16).float()
    b1 = ((torch.rand(b0.shape, generator=gen) * 2 - 1) / W0.shape[1] ** 0.5).to(torch.bfloat16).float()
    return torch.stack([W0, W1]), torch.stack([b0, b1])


def _oracle_step(O, p, Ws, bs, batch, subject, g, names):
    """The live CPU oracle with per-subject heads: O.backbone_forward once, then O.brain_head's arithmetic per head (the clip
    keeps the prediction of its own W_g), MSE over the batch + the l2 terms of ALL heads; gradients from autograd."""
    import torch.nn.functional as F
    pr = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in p.items()}
    Wl, bl = Ws.clone().requires_grad_(True), bs.clone().requires_grad_(True)
    hidden, _ = O.backbone_forward(pr, batch, g)
    wm = O.make_weight_mask(batch["padvals"], batch["vis_weights"], batch["lang_weights"], batch["language"].shape[1], g.max_len,
                            g.ds_grid * g.ds_grid).to(torch.bfloat16).float()
    y = batch["timeseries"].to(torch.bfloat16).float()
    preds, l2 = [], 0.0
    for k in range(Ws.shape[0]):
        pk, l2k, _ = O.brain_head({**pr, W_: Wl[k], B_: bl[k]}, hidden, wm, g)
        preds.append(pk)
        l2 = l2 + l2k
    pred = torch.stack([preds[k][b] for b, k in enumerate(subject)])
    loss = F.mse_loss(pred, y) + l2
    loss.backward()
    grads = {n: pr[n].grad for n in names}
    grads[W_], grads[B_] = Wl.grad, bl.grad
    return loss.detach(), pred.detach(), grads


def test_module_frozen_two_subjects_vs_live_oracle(dev):
    """frozen backbone, two subjects, B = 4, subjects [0,1,1,0], dropout off, at the tolerances test_gpu_end_to_end holds the
    single-subject step to: loss 1e-3 relative, pred 3e-2, every head gradient (stacked ones per head) 4e-2"""
    import vlb_oracle as O
    from conftest import rel_err
    from phantom_vlb_amd.litmodule import VLBLitModule
    g = O.geometry_mini()
    p = O.round_bf16(O.init_params(g, seed=1234))
    Ws, bs = _two_heads(p)
    batch = dict(O.synthetic_batch(g, 4, seed=1234), subject=torch.tensor([0, 1, 1, 0]))
    head_names = [n for n in p if n.startswith(("layer_norm1", "layer_norm2"))]
    loss_ref, pred_ref, gref = _oracle_step(O, p, Ws, bs, batch, [0, 1, 1, 0], g, head_names)
    m = VLBLitModule(_cfg(subjects=["sub-01", "sub-02"]))
    m.configure_model(state_dict=p, head_state={**{n: p[n] for n in head_names}, W_: Ws, B_: bs})
    m.configure_optimizers()
    loss = m.training_step(batch)
    torch.cuda.synchronize()
    print(f"multi-subject frozen: loss {float(loss):.6f} vs oracle {float(loss_ref):.6f}")
    assert abs(float(loss) - float(loss_ref)) / float(loss_ref) < 1e-3
    assert rel_err(m.head.pred, pred_ref) < 3e-2
    for n in head_names:
        assert rel_err(m.head.master[n].grad, gref[n]) < 4e-2, n
    for k in range(2):
        assert rel_err(m.head.master[W_].grad[k], gref[W_][k]) < 4e-2, k
        assert rel_err(m.head.master[B_].grad[k], gref[B_][k]) < 4e-2, k
    out = m.validation_step(batch)
    assert set(out) == {"loss", "brain_preds", "brain_vals", "subject"} and out["subject"].tolist() == [0, 1, 1, 0]
    # a batch without "subject" reaching this module, and the reverse: both config keys are named
    with pytest.raises(ValueError, match=r"litmodule\.config\.subjects.*datamodule\.config\.subjects"):
        m.training_step({k: v for k, v in batch.items() if k != "subject"})
    with pytest.raises(ValueError, match="subject"):
        m.training_step(dict(batch, subject=torch.tensor([0, 1, 2, 0])))


def test_module_lora_two_subjects_vs_live_oracle(dev):
    """one LoRA step on the same batch: loss within 1e-3; adapter gradients at the bar test_gpu_lora holds the mini model to (6e-2)"""
    import vlb_oracle as O
    from conftest import rel_err
    from phantom_vlb_amd.litmodule import VLBLitModule
    from phantom_vlb_amd.lora import LoraState
    g = O.geometry_mini()
    p = O.round_bf16(O.init_params(g, seed=1234, lora=True, lora_b_std=0.02))
    Ws, bs = _two_heads(p)
    batch = dict(O.synthetic_batch(g, 4, seed=1234), subject=torch.tensor([0, 1, 1, 0]))
    names = [n for n in O.trainable_names(p, False, True) if not n.startswith("ridge_layer")]
    loss_ref, pred_ref, gref = _oracle_step(O, p, Ws, bs, batch, [0, 1, 1, 0], g, names)
    m = VLBLitModule(_cfg(lora=True, subjects=["sub-01", "sub-02"]))
    head_state = {**{n: p[n] for n in names if n.startswith("layer_norm")}, W_: Ws, B_: bs}
    m.configure_model(state_dict=p, head_state=head_state)
    m.lora = LoraState(m.geometry, m.backbone.w, 16, 32, 0.0, m.device, sd=p)
    m.configure_optimizers()
    loss = m.training_step(batch)
    torch.cuda.synchronize()
    print(f"multi-subject lora: loss {float(loss):.6f} vs oracle {float(loss_ref):.6f}")
    assert abs(float(loss) - float(loss_ref)) / float(loss_ref) < 1e-3
    assert rel_err(m.head.pred, pred_ref) < 3e-2
    checked = 0
    for n in names:
        if ".lora_" not in n:
            continue
        got = m.lora.grads[n].t() if "lora_B" in n else m.lora.grads[n]
        assert rel_err(got, gref[n]) < 6e-2, n
        checked += 1
    assert checked >= 28
    for k in range(2):
        assert rel_err(m.head.grads[W_][k], gref[W_][k]) < 4e-2, k


def test_module_without_subjects_runs_the_single_head_as_before(dev):
    """subjects=None: the module's step on a single-subject batch gives the bits of a head built the old way (BrainHead without
    `subjects`, the fused vlb_head_fwd / vlb_head_bwd) on the same hidden tensor: loss and every head gradient"""
    import vlb_oracle as O
    from phantom_vlb_amd.head import BrainHead
    from phantom_vlb_amd.litmodule import VLBLitModule
    g = O.geometry_mini()
    p = O.round_bf16(O.init_params(g, seed=1234))
    batch = O.synthetic_batch(g, 4, seed=1234)
    m = VLBLitModule(_cfg())
    m.configure_model(state_dict=p, head_state=p)
    m.configure_optimizers()
    assert m.head.G == 0 and m.head.subjects is None and tuple(m.head.master[W_].shape) == (128, g.dim)
    loss = m.training_step(batch)
    hidden, wmask, y, keep, cu, rows = m.head._saved
    old = BrainHead(g.dim, 128, 1e-3, g.ln_eps, dev, sd=p)
    layout = m.backbone.row_layout(batch["language"], batch["padvals"])
    _, terms = old.forward(hidden, wmask, y, keep, layout)
    old.backward(need_dhidden=False)
    torch.cuda.synchronize()
    assert float(terms[2]) == float(loss)
    for n in old.grads:
        assert torch.equal(old.grads[n], m.head.grads[n]), n


# ---------------------------------------------------------------------------------------------------- the trainer
def test_train_py_multi_subject_experiment(tmp_path):
    """python train.py experiment=VLB_mini_synthetic_multisubject subject=sub-99: two short epochs run, val_corr_avg/<subject>
    is logged for both subjects, the checkpoint holds the stacked heads"""
    out = tmp_path / "run"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "experiment=VLB_mini_synthetic_multisubject", "subject=sub-99",
                        f"output_dir={out}"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    import csv
    rows = list(csv.DictReader(open(out / "mini_multisubject_sub-99" / "metrics.csv")))
    for name in ("sub-01", "sub-02"):
        vals = [float(x[f"val_corr_avg/{name}"]) for x in rows if x.get(f"val_corr_avg/{name}")]
        assert len(vals) >= 2 and all(-1.0 <= v <= 1.0 for v in vals), (name, vals)
    both = [x for x in rows if x.get("val_corr_avg")]
    assert both and abs(float(both[-1]["val_corr_avg"]) - 0.5 * (float(both[-1]["val_corr_avg/sub-01"]) + float(both[-1]["val_corr_avg/sub-02"]))) < 1e-6
    st = torch.load(out / "final.ckpt", map_location="cpu")
    assert tuple(st["state_dict"][W_].shape[:2]) == (2, 128) and tuple(st["state_dict"][B_].shape) == (2, 128)      # stacked heads


def _dm(batch_size=2):
    from phantom_vlb_amd.datamodule import VLBDataModule, VLBDataModuleConfig
    return VLBDataModule(VLBDataModuleConfig(lazyload_path="synthetic:3x2", subject="sub-99", subjects=["sub-01", "sub-02"],
                                             seasons=["s1"], delay=3, window=3, random_state=1234, shuffle_val_data=False,
                                             batch_size=batch_size, geometry="mini", num_target=128))


def test_multi_subject_checkpoint_resume_is_exact(dev, tmp_path):
    """6 steps straight through == 4 steps, checkpoint, resume for steps 5-6, with the stacked heads and head dropout on: the
    trainables (fp32 masters and bf16 copies) are bit-equal, as test_gpu_trainer asks of one subject"""
    from phantom_vlb_amd.litmodule import VLBLitModule
    from phantom_vlb_amd.trainer import TrainableCheckpoint, Trainer
    kw = dict(subjects=["sub-01", "sub-02"], dropout_rate=0.1, lr=1e-3)
    a = VLBLitModule(_cfg(**kw))
    ta = Trainer(max_epochs=2, max_steps=6, val_check_interval=1.0, log_every_n_steps=1,
                 callbacks=[TrainableCheckpoint(str(tmp_path), filename="best")])
    ta.fit(a, _dm())
    assert ta.global_step == 6
    st = torch.load(tmp_path / "last.ckpt", map_location="cpu", weights_only=False)
    assert st["global_step"] == 4 and tuple(st["state_dict"][W_].shape) == (2, 128, a.geometry.dim)
    b = VLBLitModule(_cfg(**kw))
    tb = Trainer(max_epochs=2, max_steps=6, val_check_interval=1.0, log_every_n_steps=1)
    tb.fit(b, _dm(), ckpt_path=str(tmp_path / "last.ckpt"))
    assert tb.global_step == 6 and b.optimizer.step_count == 6
    assert torch.equal(a.flat.master, b.flat.master) and torch.equal(a.flat.compute, b.flat.compute)
    assert not torch.equal(a.head.master[W_][0], a.head.master[W_][1])
