"""The vision-ingest and connector kernels that index a 2-D or 3-D neighbourhood (csrc/ops.hip, csrc/train.hip, the plain
transpose of csrc/gemm.hip), one operation at a time, per element against tests/stencil_emul.py: the arithmetic ones against
the fp64 restatement with its derived bars, patchify against torch's fp32 -> bf16 rounding bit for bit, the copies bit for bit
on inputs drawn from all 65536 bf16 bit patterns.

Every output lies in a NaN-filled buffer with guard rows before and behind it (guard columns too where the entry point takes
a leading dimension): after the call the written region holds what it should and the guard is bit-untouched.  The entry
points are called through phantom_vlb_amd._lib wherever the ops wrapper would allocate the output itself.  Each case names,
as literals in stencil_emul.CASES, the grid, the partly filled last block, the partial slabs, the LDS bytes or the second
grid-stride trip it is there for, and fails if stencil_emul.launch (held to the source text by test_cpu_stencil_emul) does
not say the same.  Bars: stencil_emul.py; test_cpu_stencil_emul.py shows on the CPU that honest fp32 meets them and that
sixteen planted bugs do not.  Run with -s to see max(err / bar) and the number of elements outside per operation and case."""
import pytest
import torch

import stencil_emul as E

pytestmark = pytest.mark.gpu

BF, I16 = torch.bfloat16, torch.int16
G = 2                     # guard rows on either side of an output


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Out:
    """[rows, cols] bf16 output inside a NaN-filled [G + rows + G, ld] buffer"""

    def __init__(self, dev, rows, cols, ld=None):
        ld = cols if ld is None else ld
        self.full = torch.full((G + rows + G, ld), float("nan"), dtype=BF, device=dev)
        self.view = self.full[G:G + rows, :cols] if ld != cols else self.full[G:G + rows]
        self.inside = torch.zeros(G + rows + G, ld, dtype=torch.bool, device=dev)
        self.inside[G:G + rows, :cols] = True
        self.before = self.full.clone()
        self.ld = ld

    def ptr(self):
        return self.view.data_ptr()

    def untouched(self):
        torch.cuda.synchronize()
        return torch.equal(self.full.view(I16), self.before.view(I16))

    def bits(self):
        """-> the written region's bit patterns on the host, after checking that nothing around it changed"""
        torch.cuda.synchronize()
        assert torch.equal(self.full.view(I16)[~self.inside], self.before.view(I16)[~self.inside]), "guard region touched"
        return self.view.contiguous().view(I16).cpu()

    def host(self):
        """-> the written region as fp32 on the host: finite everywhere (no element left unwritten), guard untouched"""
        b = self.bits()
        v = b.view(BF).float()
        assert bool(torch.isfinite(v).all()), "NaN / inf in the written region"
        return v


def _check(rc, what):
    from phantom_vlb_amd._lib import check
    check(rc, what)


def _expect(op, shape):
    expect = dict(E.CASES[op])[shape]
    got = E.launch(op, shape)
    for k, v in expect.items():
        assert got[k] == v, (op, shape, k, got[k], v)
    return expect


def _report(op, shape, got, expect):
    """max(err / bar) per output <= 1, and every element within the bf16 values its fp32 bar can reach (rows_emul.reach)"""
    ref, bar = E.call(op, shape)
    r, out = E.ratios(got, ref, bar), E.outside(got, ref, bar)
    print(op, E.sid(shape), expect, {k: round(v, 3) for k, v in r.items()}, "outside:", out)
    assert all(v <= 1.0 for v in r.values()), (op, shape, r)
    assert not any(out.values()), (op, shape, out)


def _report_bits(op, shape, got, expect):
    ref = E.call(op, shape)
    d = E.bits_differ(got, ref)
    print(op, E.sid(shape), expect, "elements whose bits differ:", d)
    assert not any(d.values()), (op, shape, d)


def _dev(dev, op, shape):
    """the inputs of a case on the device (bit patterns as the bf16 tensors they are)"""
    out = {}
    for k, v in E.inputs_for(op, shape).items():
        if torch.is_tensor(v):
            out[k] = (v.view(BF) if v.dtype == I16 else v).to(dev)
    return out


def _params(op, runnable=True):
    s = E.shapes(op, runnable)
    return dict(argnames="shape", argvalues=s, ids=[E.sid(v) for v in s])


# ---------------------------------------------------------------------------------------------------- depthwise 3x3
@pytest.mark.parametrize(**_params("dwconv3x3"))
def test_dwconv3x3_forward_and_data_gradient(dev, shape):
    """forward, and the data gradient as FullFT._block_bwd takes it (the same kernel on dy with the taps reversed) against the
    fp64 autograd dx that test_cpu_stencil_emul ties stencil_emul.dwconv3x3_dx to"""
    from phantom_vlb_amd._lib import lib
    N, H, W, C = shape
    expect = _expect("dwconv3x3", shape)
    d = _dev(dev, "dwconv3x3", shape)
    y, dx = Out(dev, N * H * W, C), Out(dev, N * H * W, C)
    _check(lib.vlb_dwconv3x3(d["x"].data_ptr(), d["w9"].data_ptr(), y.ptr(), N, H, W, C, _stream()), "vlb_dwconv3x3")
    w9f = torch.flip(d["w9"], dims=[0]).contiguous()
    _check(lib.vlb_dwconv3x3(d["dy"].data_ptr(), w9f.data_ptr(), dx.ptr(), N, H, W, C, _stream()), "vlb_dwconv3x3")
    _report("dwconv3x3", shape, dict(y=y.host()), expect)
    _report("dwconv3x3_dx", shape, dict(dx=dx.host()), expect)


def test_dwconv3x3_refuses_a_plane_that_does_not_fit_in_lds(dev):
    """2583 positions = 165,312 bytes: VlbError, and nothing is launched (the output stays as it was)"""
    from phantom_vlb_amd._lib import VlbError, lib
    (shape,) = [s for s in E.shapes("dwconv3x3", runnable=False) if s not in E.shapes("dwconv3x3")]
    N, H, W, C = shape
    expect = _expect("dwconv3x3", shape)
    assert expect["refused"] and H * W == 2583
    x = torch.zeros(N * H * W, C, dtype=BF, device=dev)
    w9 = torch.zeros(9, C, dtype=BF, device=dev)
    y = Out(dev, N * H * W, C)
    with pytest.raises(VlbError, match="does not fit in LDS"):
        _check(lib.vlb_dwconv3x3(x.data_ptr(), w9.data_ptr(), y.ptr(), N, H, W, C, _stream()), "vlb_dwconv3x3")
    assert y.untouched()


def _dwconv3x3_bwd_w(dev, shape, expect):
    from phantom_vlb_amd._lib import lib
    N, H, W, C = shape
    d = _dev(dev, "dwconv3x3_bwd_w", shape)
    n_ws = int(lib.vlb_dwconv3x3_bwd_w_ws_floats(N, H, C))
    assert n_ws == expect["slabs"] * 9 * C
    ws = torch.full((n_ws,), float("nan"), dtype=torch.float32, device=dev)        # a slab entry left unwritten would surface as NaN
    dw = Out(dev, 9, C)
    _check(lib.vlb_dwconv3x3_bwd_w(d["x"].data_ptr(), d["dy"].data_ptr(), dw.ptr(), ws.data_ptr(), N, H, W, C, _stream()), "vlb_dwconv3x3_bwd_w")
    return dw


@pytest.mark.parametrize(**_params("dwconv3x3_bwd_w"))
def test_dwconv3x3_bwd_w(dev, shape):
    expect = _expect("dwconv3x3_bwd_w", shape)
    _report("dwconv3x3_bwd_w", shape, dict(dw=_dwconv3x3_bwd_w(dev, shape, expect).host()), expect)


def test_dwconv3x3_bwd_w_repeats_bit_for_bit(dev):
    """train.hip: the slabs are reduced in a fixed order.  18 slabs over 8 uneven groups, and two blockIdx.x, twice."""
    for shape in ((9, 2, 3, 8), (1, 3, 4, 2056)):
        expect = _expect("dwconv3x3_bwd_w", shape)
        assert torch.equal(_dwconv3x3_bwd_w(dev, shape, expect).bits(), _dwconv3x3_bwd_w(dev, shape, expect).bits())


# ---------------------------------------------------------------------------------------------------- squeeze-excite
@pytest.mark.parametrize(**_params("se_pool"))
def test_se_pool(dev, shape):
    from phantom_vlb_amd._lib import lib
    N, HW, C = shape
    expect = _expect("se_pool", shape)
    d = _dev(dev, "se_pool", shape)
    pooled = Out(dev, N, C)
    _check(lib.vlb_se_pool(d["x"].data_ptr(), pooled.ptr(), N, HW, C, _stream()), "vlb_se_pool")
    _report("se_pool", shape, dict(pooled=pooled.host()), expect)


@pytest.mark.parametrize(**_params("se_scale"))
def test_se_scale(dev, shape):
    from phantom_vlb_amd._lib import lib
    N, HW, C = shape
    expect = _expect("se_scale", shape)
    d = _dev(dev, "se_scale", shape)
    y = Out(dev, N * HW, C)
    _check(lib.vlb_se_scale(d["x"].data_ptr(), d["s"].data_ptr(), y.ptr(), N, HW, C, _stream()), "vlb_se_scale")
    _report("se_scale", shape, dict(y=y.host()), expect)


@pytest.mark.parametrize(**_params("se_bwd_gate"))
def test_se_bwd_gate(dev, shape):
    from phantom_vlb_amd._lib import lib
    N, HW, C = shape
    expect = _expect("se_bwd_gate", shape)
    d = _dev(dev, "se_bwd_gate", shape)
    ds = Out(dev, N, C)
    _check(lib.vlb_se_bwd_gate(d["x"].data_ptr(), d["dy"].data_ptr(), d["s"].data_ptr(), ds.ptr(), N, HW, C, _stream()), "vlb_se_bwd_gate")
    _report("se_bwd_gate", shape, dict(ds=ds.host()), expect)


@pytest.mark.parametrize(**_params("se_bwd_x"))
def test_se_bwd_x_with_and_without_dpool(dev, shape):
    from phantom_vlb_amd._lib import lib
    N, HW, C = shape
    expect = _expect("se_bwd_x", shape)
    d = _dev(dev, "se_bwd_x", shape)
    for op, dpool in (("se_bwd_x", d["dpool"].data_ptr()), ("se_bwd_x_nopool", None)):
        dx = Out(dev, N * HW, C)
        _check(lib.vlb_se_bwd_x(d["dy"].data_ptr(), d["s"].data_ptr(), dpool, dx.ptr(), N, HW, C, _stream()), "vlb_se_bwd_x")
        _report(op, shape, dict(dx=dx.host()), expect)


# ---------------------------------------------------------------------------------------------------- vision ingest
@pytest.mark.parametrize(**_params("patchify"))
def test_patchify(dev, shape):
    from phantom_vlb_amd._lib import lib
    N, H, W, P, Kpad = shape
    expect = _expect("patchify", shape)
    vis = E.inputs_for("patchify", shape)["vis"].to(dev)
    out = Out(dev, N * (H // P) * (W // P), Kpad)
    _check(lib.vlb_patchify(vis.data_ptr(), out.ptr(), N, H, W, P, Kpad, _stream()), "vlb_patchify")
    _report_bits("patchify", shape, dict(patches=out.bits()), expect)


@pytest.mark.parametrize(**_params("vit_assemble"))
def test_vit_assemble(dev, shape):
    from phantom_vlb_amd._lib import lib
    N, Gr, D = shape
    expect = _expect("vit_assemble", shape)
    d = _dev(dev, "vit_assemble", shape)
    tok = Out(dev, N * (Gr + 1), D)
    _check(lib.vlb_vit_assemble(d["pe"].data_ptr(), d["cls"].data_ptr(), d["pos"].data_ptr(), tok.ptr(), N, Gr, D, _stream()), "vlb_vit_assemble")
    _report("vit_assemble", shape, dict(tok=tok.host()), expect)


@pytest.mark.parametrize(**_params("drop_cls"))
def test_drop_cls(dev, shape):
    from phantom_vlb_amd._lib import lib
    N, Gr, D = shape
    expect = _expect("drop_cls", shape)
    d = _dev(dev, "drop_cls", shape)
    out = Out(dev, N * Gr, D)
    _check(lib.vlb_drop_cls(d["tok"].data_ptr(), out.ptr(), N, Gr, D, _stream()), "vlb_drop_cls")
    _report_bits("drop_cls", shape, dict(out=out.bits()), expect)


# ---------------------------------------------------------------------------------------------------- Conv3d k2 s2 p1 as a GEMM
@pytest.mark.parametrize(**_params("im2col3d"))
def test_im2col3d(dev, shape):
    from phantom_vlb_amd._lib import lib
    B, T, H, W, C = shape
    expect = _expect("im2col3d", shape)
    d = _dev(dev, "im2col3d", shape)
    T2, H2, W2 = E.launch("im2col3d", shape)["out"]
    cols = Out(dev, B * T2 * H2 * W2, 8 * C)
    _check(lib.vlb_im2col3d_k2s2p1(d["x"].data_ptr(), cols.ptr(), B, T, H, W, C, _stream()), "vlb_im2col3d_k2s2p1")
    got = cols.bits()
    _report_bits("im2col3d", shape, dict(cols=got), expect)
    pad = E.padding_taps(T, H, W)
    assert bool((got.reshape(B, -1, 8, C)[:, pad] == 0).all())               # +0 bits, not -0


@pytest.mark.parametrize(**_params("col2im3d"))
def test_col2im3d(dev, shape):
    """on random dcols whose padding taps hold non-zero "gradient" (ignored), and on im2col3d's own output (the inverse)"""
    from phantom_vlb_amd._lib import lib
    B, T, H, W, C = shape
    expect = _expect("col2im3d", shape)
    d = _dev(dev, "col2im3d", shape)
    pad = E.padding_taps(T, H, W)
    if bool(pad.any()):
        assert bool((E.inputs_for("col2im3d", shape)["dcols"].reshape(B, -1, 8, C)[:, pad] != 0).any())
    dx = Out(dev, B * T * H * W, C)
    _check(lib.vlb_col2im3d_k2s2p1(d["dcols"].data_ptr(), dx.ptr(), B, T, H, W, C, _stream()), "vlb_col2im3d_k2s2p1")
    _report_bits("col2im3d", shape, dict(dx=dx.bits()), expect)
    x = _dev(dev, "im2col3d", shape)["x"]
    T2, H2, W2 = expect["out"]
    cols = torch.empty(B * T2 * H2 * W2, 8 * C, dtype=BF, device=dev)
    _check(lib.vlb_im2col3d_k2s2p1(x.data_ptr(), cols.data_ptr(), B, T, H, W, C, _stream()), "vlb_im2col3d_k2s2p1")
    back = Out(dev, B * T * H * W, C)
    _check(lib.vlb_col2im3d_k2s2p1(cols.data_ptr(), back.ptr(), B, T, H, W, C, _stream()), "vlb_col2im3d_k2s2p1")
    _report_bits("col2im3d_of_im2col", shape, dict(dx=back.bits()), expect)


# ---------------------------------------------------------------------------------------------------- transposes
@pytest.mark.parametrize(**_params("transpose_pad"))
def test_transpose_pad(dev, shape):
    """x is the first C columns of a [R, ld_in] matrix; the output has ld_out = Rpad + 8: eight guard columns per row"""
    from phantom_vlb_amd._lib import lib
    Rr, C, ld_in, Rpad = shape
    expect = _expect("transpose_pad", shape)
    d = _dev(dev, "transpose_pad", shape)
    out = Out(dev, C, Rpad, ld=Rpad + 8)
    _check(lib.vlb_transpose_pad(d["x"].data_ptr(), ld_in, out.ptr(), out.ld, Rr, C, Rpad, _stream()), "vlb_transpose_pad")
    got = out.bits()
    _report_bits("transpose_pad", shape, dict(out=got), expect)
    assert bool((got[:, Rr:] == 0).all())                                      # +0 bits


@pytest.mark.parametrize(**_params("transpose"))
def test_transpose(dev, shape):
    from phantom_vlb_amd._lib import lib
    Rr, C = shape
    expect = _expect("transpose", shape)
    d = _dev(dev, "transpose", shape)
    out = Out(dev, C, Rr)
    _check(lib.vlb_transpose_bf16(d["x"].data_ptr(), out.ptr(), Rr, C, _stream()), "vlb_transpose_bf16")
    _report_bits("transpose", shape, dict(out=out.bits()), expect)


# ---------------------------------------------------------------------------------------------------- splice
@pytest.mark.parametrize(**_params("splice_embed"))
def test_splice_embed_dense(dev, shape):
    """video token at position 0, in the middle and at L - 1; left padding with id 0; S = 19 rows per clip in blocks of 16"""
    from phantom_vlb_amd._lib import lib
    from vlb_oracle import VIDEO_TOKEN_ID
    B, L, Nv, D = shape
    S = L - 1 + Nv
    expect = _expect("splice_embed", shape)
    d = _dev(dev, "splice_embed", shape)
    emb = Out(dev, B * S, D)
    mask = torch.full((G + B * S + G,), 0xAB, dtype=torch.uint8, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    _check(lib.vlb_splice_embed(d["ids"].data_ptr(), d["emb"].data_ptr(), d["vid"].data_ptr(), emb.ptr(), mask[G:].data_ptr(), err.data_ptr(),
                                B, L, Nv, D, VIDEO_TOKEN_ID, E.SPLICE_VOCAB, None, None, _stream()), "vlb_splice_embed")
    got = dict(embeds=emb.bits(), key_mask=mask[G:G + B * S].reshape(B, S).cpu())
    assert int(err.item()) == 0
    assert bool((mask[:G] == 0xAB).all()) and bool((mask[G + B * S:] == 0xAB).all())
    _report_bits("splice_embed", shape, got, expect)
