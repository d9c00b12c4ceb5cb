"""The kernels ``readout_layers`` adds to the brain head (csrc/head.hip: layer mix forward / backward, d hidden in write
and accumulate mode, the pooling half on its own), each alone against the fp64 restatement and the derived bars of
tests/layer_mix_emul.py.  Inputs are seeded; a stage is fed the device's own upstream buffers.  Run with -s for
max(err / bar)."""
import pytest
import torch

import head_emul as H
import layer_mix_emul as M
from layer_mix_emul import BF16, F32

pytestmark = pytest.mark.gpu


def _ptr(t):
    return None if t is None else t.data_ptr()


def _mix(dev, inp):
    """vlb_head_mix_fwd then vlb_head_mix_bwd on the device's own alpha -> host tensors"""
    from phantom_vlb_amd._lib import check, lib
    from phantom_vlb_amd.ops import _stream
    K, B, E = inp["K"], inp["B"], inp["E"]
    P, draw = inp["P"].to(dev), inp["draw"].to(dev)
    a = None if inp["a"] is None else inp["a"].to(dev, BF16)
    alpha = torch.full((K,), float("nan"), device=dev)
    pooled, d_a = torch.full((B, E), float("nan"), device=dev), torch.full((K,), float("nan"), device=dev)
    dstack = torch.full((K, B, E), float("nan"), device=dev)
    n_ws = lib.vlb_head_mix_ws_floats(K, B, E)
    guard = 64                                          # floats behind the slab the kernels must leave alone
    ws = torch.full((n_ws + guard,), -7.0, device=dev)
    check(lib.vlb_head_mix_fwd(P.data_ptr(), _ptr(a), alpha.data_ptr(), pooled.data_ptr(), K, B, E, _stream()), "vlb_head_mix_fwd")
    check(lib.vlb_head_mix_bwd(P.data_ptr(), draw.data_ptr(), alpha.data_ptr(), d_a.data_ptr(), dstack.data_ptr(), ws.data_ptr(),
                               K, B, E, _stream()), "vlb_head_mix_bwd")
    torch.cuda.synchronize()
    assert bool((ws[n_ws:] == -7.0).all()), "vlb_head_mix_bwd wrote past vlb_head_mix_ws_floats"
    return {k: v.cpu() for k, v in dict(alpha=alpha, pooled=pooled, d_a=d_a, draw_stack=dstack).items()}


@pytest.mark.parametrize("E", [264, 512, 4104])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("K", [1, 2, 5])
def test_mix_forward_and_backward(dev, K, B, E):
    inp = M.mix_inputs(K, B, E)
    got = _mix(dev, inp)
    ref = M.mix_fwd(inp["P"], inp["a"])
    bars = M.mix_fwd_bars(ref, inp["P"], inp["a"])
    refb = M.mix_bwd(inp["P"], inp["draw"], got["alpha"])              # the backward is fed the device's own alpha
    barb = M.mix_bwd_bars(refb, got["alpha"], B, E)
    ratios = dict(alpha=M.ratio(got["alpha"], ref["alpha"], bars["alpha"]), pooled=M.ratio(got["pooled"], ref["pooled"], bars["pooled"]),
                  d_a=M.ratio(got["d_a"], refb["d_a"], barb["d_a"]), draw_stack=M.ratio(got["draw_stack"], refb["draw_stack"], barb["draw_stack"]))
    print(f"layer-mix K={K} B={B} E={E}: " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    if K == 1:              # no logit: alpha = 1, both outputs are copies of their inputs, the (absent) logit's gradient is 0
        assert torch.equal(got["pooled"], inp["P"][0]) and torch.equal(got["draw_stack"][0], inp["draw"])
        assert got["alpha"].tolist() == [1.0] and got["d_a"].tolist() == [0.0]
    else:
        assert float(got["alpha"].max() / got["alpha"].min()) > 3.0         # far from uniform
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, bad


def test_mix_keeps_the_sign_of_zero_for_one_layer(dev):
    """K = 1 must hand on the bits, a negative zero included (1.0f * p, never 0 + p)"""
    inp = M.mix_inputs(1, 1, 264)
    inp["P"][0, 0, :8] = torch.tensor([-0.0, 0.0, -0.0, 1.0, -1.0, 3.0e38, -0.0, 2.0 ** -126])
    got = _mix(dev, inp)
    assert torch.equal(got["pooled"].view(torch.int32), inp["P"][0].view(torch.int32))


def _dh_device(dev, packed, E=512):
    """Two taps pooled on the device (vlb_head_pool: the device's own statistics) and every d hidden launch the tests need."""
    from phantom_vlb_amd import ops
    from phantom_vlb_amd._lib import check, lib
    from phantom_vlb_amd.ops import _stream
    lens = [33, 20, 26] if packed else None           # 79 rows: no multiple of the 4 rows per block either
    inp = M.dh_inputs(E=E, lens=lens)
    B, S, E = inp["B"], inp["S"], inp["E"]
    lay = ops.RowLayout(B, S, lens, device=dev) if packed else None
    cu, rows = (lay.cu, lay.rows) if packed else (None, B * S)
    to_rows = (lambda t: M.pack_rows(t, lens).contiguous()) if packed else (lambda t: t.reshape(B * S, *t.shape[2:]).contiguous())
    wmask = inp["wmask"].to(dev)
    hid = [to_rows(h).to(dev) for h in inp["hidden"]]
    draw = inp["draw"].to(dev)
    ws = torch.empty(lib.vlb_head_ws_floats(B, S, E, 8), device=dev)
    stats = torch.zeros(2, B, S, 2, device=dev)
    pooled, sumw = torch.empty(2, B, E, device=dev), torch.empty(B, device=dev)
    for k in range(2):
        check(lib.vlb_head_pool(hid[k].data_ptr(), wmask.data_ptr(), ws.data_ptr(), stats[k].data_ptr(), pooled[k].data_ptr(),
                                sumw.data_ptr(), B, S, E, inp["eps"], _ptr(cu), _stream()), "vlb_head_pool")

    def dhidden(k, dx, accumulate, stats_k=None):
        check(lib.vlb_head_dhidden(hid[k].data_ptr(), wmask.data_ptr(), stats[k if stats_k is None else stats_k].data_ptr(),
                                   draw[k].data_ptr(), dx.data_ptr(), B, S, E, _ptr(cu), rows, int(accumulate), _stream()),
              "vlb_head_dhidden")
        return dx
    dense = (lambda t, fill: M.unpack_rows(t.cpu(), lens, S, fill)) if packed else (lambda t, fill: t.cpu().view(B, S, E))
    return dict(inp=inp, hid=hid, wmask=wmask, draw=draw, stats=stats, pooled=pooled, sumw=sumw, dhidden=dhidden, rows=rows, cu=cu,
                to_rows=to_rows, dense=dense, B=B, S=S, E=E)


@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
def test_pool_entry_gives_the_bits_of_head_fwd(dev, packed):
    """vlb_head_pool is the pooling half of vlb_head_fwd: statistics at live tokens, pooled_raw and sumw are its bits"""
    from phantom_vlb_amd import ops
    from phantom_vlb_amd.head import BrainHead
    d = _dh_device(dev, packed)
    inp, B, S, E = d["inp"], d["B"], d["S"], d["E"]
    head = BrainHead(E, 8, 1e-3, inp["eps"], dev)
    lay = ops.RowLayout(B, S, inp["lens"], device=dev) if packed else None
    live = inp["wmask"].to(dev) != 0
    for k in range(2):
        head.forward(d["hid"][k], d["wmask"], torch.zeros(B, 8, device=dev), None, layout=lay)
        assert torch.equal(head.pooled_raw, d["pooled"][k]) and torch.equal(head.sumw, d["sumw"])
        assert torch.equal(head.stats[live], d["stats"][k][live])
    assert not torch.equal(d["pooled"][0], d["pooled"][1])


@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
def test_dhidden_write_mode_is_head_bwd(dev, packed):
    """write mode == what vlb_head_bwd writes for the same (hidden, statistics, draw): the same kernel behind its own entry"""
    from phantom_vlb_amd import ops
    from phantom_vlb_amd.head import BrainHead
    d = _dh_device(dev, packed)
    inp, B, S, E = d["inp"], d["B"], d["S"], d["E"]
    assert (S * B) % 4 != 0 and d["rows"] % 4 != 0 and bool((inp["wmask"][1] == 0).all())
    gen = torch.Generator().manual_seed(5)
    head = BrainHead(E, 8, 1e-3, inp["eps"], dev)
    lay = ops.RowLayout(B, S, inp["lens"], device=dev) if packed else None
    head.forward(d["hid"][0], d["wmask"], torch.randn(B, 8, generator=gen).to(dev), None, layout=lay)
    want = head.backward(need_dhidden=True)
    d["stats"][0].copy_(head.stats)
    d["draw"][0].copy_(head.dpooled)
    got = d["dhidden"](0, torch.full((d["rows"], E), float("nan"), dtype=BF16, device=dev), False)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert bool((d["dense"](got, torch.zeros(B, S, E, dtype=BF16))[1] == 0).all())        # the all-zero clip: zeroed rows


@pytest.mark.parametrize("packed,E", [(False, 512), (True, 512), (False, 1024), (True, 1544), (True, 4096), (False, 4104)],
                         ids=["dense", "packed", "dense-E1024", "packed-E1544", "packed-E4096", "dense-E4104"])
def test_dhidden_accumulate_mode(dev, packed, E):
    """E = 512 is the case to check; the others take the accumulate kernel's 2-, 4-, 8- and 16-chunk forms, two of them
    with a column guard (a row is held in registers in ceil(E/512) chunks per lane: the kernel is a template over that)."""
    d = _dh_device(dev, packed, E)
    inp, B, S, E = d["inp"], d["B"], d["S"], d["E"]
    dx0_rows = d["to_rows"](inp["dx0"])
    stats = d["stats"].cpu()
    w = inp["wmask"]
    ratios = {}
    for k in range(2):
        got = d["dhidden"](k, dx0_rows.clone().to(dev), True)
        again = d["dhidden"](k, dx0_rows.clone().to(dev), True)
        torch.cuda.synchronize()
        assert torch.equal(got, again), "two runs differ"
        ref = M.dhidden_acc(inp["dx0"], inp["hidden"][k], w, stats[k, ..., 0], stats[k, ..., 1], inp["draw"][k])
        dense = d["dense"](got, inp["dx0"])                  # rows a packed layout does not hold: nothing to compare
        ratios[f"tap{k}"] = M.ratio(dense, ref["dx"], M.dhidden_acc_bars(ref, E))
        dead = w == 0
        assert torch.equal(dense[dead].view(torch.int16), inp["dx0"][dead].view(torch.int16)), "a zero-weight row changed"
        assert not torch.equal(dense[~dead], inp["dx0"][~dead])
        # the write-mode value at the same bar; with the other tap's statistics it must miss it (the planted bug, on the device)
        wr = d["dhidden"](k, torch.empty(d["rows"], E, dtype=BF16, device=dev), False)
        wrong = d["dhidden"](k, torch.empty(d["rows"], E, dtype=BF16, device=dev), False, stats_k=1 - k)
        refw = M.dhidden_write(inp["hidden"][k], w, stats[k, ..., 0], stats[k, ..., 1], inp["draw"][k])
        zeros = torch.zeros(B, S, E, dtype=BF16)
        # added to +0 the value is itself: accumulate mode forms the write-mode value, bit for bit (up to the sign of a zero)
        onto0 = d["dhidden"](k, torch.zeros(d["rows"], E, dtype=BF16, device=dev), True)
        assert torch.equal(onto0.float(), wr.float())
        ratios[f"write{k}"] = M.ratio(d["dense"](wr, zeros), refw["dh"], M.dhidden_write_bars(refw, E))
        assert M.ratio(d["dense"](wrong, zeros), refw["dh"], M.dhidden_write_bars(refw, E)) > 1
    print(f"dhidden-acc {'packed' if packed else 'dense'} E={E}: " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, bad
