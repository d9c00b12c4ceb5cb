"""The brain head's kernels (csrc/head.hip), one at a time, against the fp64 staged reference of tests/head_emul.py.

Each case runs BrainHead.forward and .backward(need_dhidden=True) ONCE, copies every buffer the head keeps to the host and
judges each kernel on the device's own upstream buffers, at that kernel's fp32 accumulation error (bars: head_emul.py).
One end-to-end comparison with the head as mathematics at the bars of test_head_fwd_bwd rides along.  Every case names,
as literals, the kernels it is there for and fails if head_emul.dispatch(B, E), a Python restatement of the planner's
branch conditions, does not lead there (the library does not report its launches; the restatement itself is held to the
source text of head.hip by test_cpu_head_emul).  Run with -s to see max(err / bar)."""
import pytest
import torch

import head_emul as H

pytestmark = pytest.mark.gpu


def _head(dev, inp):
    from phantom_vlb_amd.head import BrainHead
    c = inp["case"]
    return BrainHead(c["E"], c["V"], inp["lam"], inp["eps"], dev, sd=inp["params"])


def _device_inputs(dev, inp):
    from phantom_vlb_amd import ops
    c = inp["case"]
    B, S, E = c["B"], c["S"], c["E"]
    lay = None
    if c["lens"] is None:
        hidden = inp["hidden"].view(B * S, E).to(dev)
    else:
        lay = ops.RowLayout(B, S, c["lens"], device=dev)
        hidden = torch.cat([inp["hidden"][b, :n] for b, n in enumerate(c["lens"])], 0).contiguous().to(dev)
    keep = None if inp["keep"] is None else inp["keep"].to(dev)
    return hidden, inp["wmask"].to(dev), inp["y"].to(dev), keep, lay


def _step(head, dinp, inp):
    hidden, wmask, y, keep, lay = dinp
    head.forward(hidden, wmask, y, keep, layout=lay)
    dh = head.backward(need_dhidden=True, loss_scale=inp["loss_scale"], l2_scale=inp["l2_scale"])
    torch.cuda.synchronize()
    return dh


def _device_tensors(head, dh):
    t = dict(stats=head.stats, pooled_raw=head.pooled_raw, sumw=head.sumw, zhat=head.zhat, ln2_rstd=head.ln2_rstd, z=head.z,
             pred=head.pred, loss_terms=head.loss_terms, dz=head.dz, dpooled=head.dpooled, dh=dh)
    t.update({H.GRAD_KEYS[n]: g for n, g in head.grads.items()})
    return t


def _host_buffers(head, dh, inp):
    c = inp["case"]
    B, S, E = c["B"], c["S"], c["E"]
    bufs = {k: v.detach().cpu() for k, v in _device_tensors(head, dh).items()}
    stats = bufs.pop("stats")
    bufs["mu"], bufs["rstd"] = stats[..., 0].contiguous(), stats[..., 1].contiguous()
    if c["lens"] is None:
        bufs["dh"] = bufs["dh"].view(B, S, E)
    else:                                           # packed rows -> dense [B,S,E]; the rows that are not there count as zero
        dense, r = torch.zeros(B, S, E, dtype=bufs["dh"].dtype), 0
        for b, n in enumerate(c["lens"]):
            dense[b, :n] = bufs["dh"][r:r + n]
            r += n
        assert r == bufs["dh"].shape[0]
        bufs["dh"] = dense
    return bufs


def _run_case(dev, cid, end_to_end):
    inp = H.inputs_for(cid)
    c = inp["case"]
    assert set(c["expect"]) <= H.dispatch(c["B"], c["E"]), f"{cid} no longer reaches {set(c['expect']) - H.dispatch(c['B'], c['E'])}"
    head = _head(dev, inp)
    dh = _step(head, _device_inputs(dev, inp), inp)
    bufs = _host_buffers(head, dh, inp)
    ratios = H.check_stages(bufs, inp, c["stages"])
    print(f"head-stages {cid}: " + " ".join(f"{k}={v:.3f}" for k, v in H.by_stage(ratios).items()))
    print(f"head-stages-detail {cid}: " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (cid, bad)
    if end_to_end:
        e2e, bars = H.end_to_end(bufs, inp), H.E2E_BARS
        print(f"head-e2e {cid}: " + " ".join(f"{k}={v:.2e}/{bars[k]:.0e}" for k, v in e2e.items()))
        bad = {k: (v, bars[k]) for k, v in e2e.items() if not v < bars[k]}
        assert not bad, (cid, bad)


@pytest.mark.parametrize("cid", [c["id"] for c in H.CASES])
def test_head_stages(dev, cid):
    _run_case(dev, cid, end_to_end=True)


@pytest.mark.parametrize("cid", [c["id"] for c in H.KSWEEP])
def test_ridge_mfma_every_ksteps(dev, cid):
    """ridge_fwd_mfma_kernel<KSTEPS> for KSTEPS = 1..32 (E = 128*KSTEPS), and the skinny-wgrad dz at the same K"""
    _run_case(dev, cid, end_to_end=False)


@pytest.mark.parametrize("cid", ["clips-B16", "clips-B17-drop"])
def test_head_step_is_deterministic(dev, cid):
    """fixed-order reductions (the file header's claim): a second forward + backward gives the same bits, on both dz paths"""
    inp = H.inputs_for(cid)
    assert ("wgrad_mfma_kernel" if cid == "clips-B16" else "ridge_bwd_z_kernel") in H.dispatch(inp["case"]["B"], inp["case"]["E"])
    head, dinp = _head(dev, inp), _device_inputs(dev, inp)
    first = {k: v.clone() for k, v in _device_tensors(head, _step(head, dinp, inp)).items()}
    for v in _device_tensors(head, None).values():
        if v is not None:
            v.fill_(float("nan"))
    second = _device_tensors(head, _step(head, dinp, inp))
    live = (inp["wmask"] != 0).to(dev)
    for k, v in first.items():
        a, b = (v[live], second[k][live]) if k == "stats" else (v, second[k])       # stats of zero-weight tokens are never written
        assert torch.equal(a, b), k


def test_cached_step_is_bit_identical_beyond_16_clips(dev):
    """forward_cached / backward_cached at B = 17 (ridge_fwd_kernel, ridge_bwd_z_kernel, head_dz_reduce_kernel)"""
    from phantom_vlb_amd.feature_cache import FeatureCache
    inp = H.inputs_for("clips-B17-drop")
    c = inp["case"]
    B, E = c["B"], c["E"]
    assert {"ridge_fwd_kernel", "ridge_bwd_z_kernel", "head_dz_reduce_kernel"} <= H.dispatch(B, E) and (B, E, c["V"]) == (17, 1024, 40)
    head = _head(dev, inp)
    hidden, wmask, y, keep, _ = _device_inputs(dev, inp)
    cache = FeatureCache("train", 41, E, dev)
    idx = torch.randperm(41, generator=torch.Generator().manual_seed(B))[:B]
    for ks in (None, keep):
        pred, terms = head.forward(hidden, wmask, y, ks)
        head.backward(need_dhidden=False, loss_scale=0.25, l2_scale=0.5)
        ref = (pred.clone(), terms.clone(), {n: g.clone() for n, g in head.grads.items()}, head.dz.clone(), head.dpooled.clone())
        cache.store(idx, head)
        for t in (head.pooled_raw, head.sumw, head.zhat, head.ln2_rstd, head.pred, head.loss_terms, head.dz, head.dpooled):
            t.fill_(float("nan"))
        for g in head.grads.values():
            g.fill_(float("nan"))
        pred2, terms2 = head.forward_cached(cache, idx, y, ks)
        head.backward_cached(loss_scale=0.25, l2_scale=0.5)
        torch.cuda.synchronize()
        assert torch.equal(pred2, ref[0]) and torch.equal(terms2, ref[1])
        for n, g in head.grads.items():
            assert torch.equal(g, ref[2][n]), n
        assert torch.equal(head.dz, ref[3]) and torch.equal(head.dpooled, ref[4])
        cache.valid[:] = False


@pytest.mark.parametrize("E", [260, 8200])
def test_head_refuses_unsupported_width(dev, E):
    """E % 8 != 0 and E > 8192: VlbError from vlb_head_fwd and from vlb_head_bwd, before anything is launched"""
    from phantom_vlb_amd._lib import VlbError
    from phantom_vlb_amd.head import BrainHead
    B, S, V = 2, 4, 16
    head = BrainHead(E, V, H.LAMBDA, H.EPS, dev)
    hidden = torch.zeros(B * S, E, dtype=torch.bfloat16, device=dev)
    wmask, y = torch.ones(B, S, device=dev), torch.zeros(B, V, device=dev)
    with pytest.raises(VlbError, match="head_fwd"):
        head.forward(hidden, wmask, y)
    with pytest.raises(VlbError, match="head_bwd"):
        head.backward(need_dhidden=True)


def test_packed_backward_refuses_too_many_rows(dev):
    from phantom_vlb_amd._lib import VlbError
    inp = H.inputs_for("packed")
    c = inp["case"]
    head, dinp = _head(dev, inp), _device_inputs(dev, inp)
    head.forward(dinp[0], dinp[1], dinp[2], dinp[3], layout=dinp[4])
    hidden, wmask, y, keep, cu, rows = head._saved
    head._saved = (hidden, wmask, y, keep, cu, c["B"] * c["S"] + 1)
    with pytest.raises(VlbError, match="total_rows"):
        head.backward(need_dhidden=True)
    torch.cuda.synchronize()
