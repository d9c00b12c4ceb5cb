"""The stencil kernels' reference (tests/stencil_emul.py) checked on the CPU: every stage is the operation (torch.nn.functional
and autograd in fp64, 1e-12 of the sum of its terms' magnitudes; bit for bit for the copies), an fp32 restatement of each
arithmetic kernel in the kernel's own order stays inside every bar at every GPU case, every planted bug leaves a bar or
changes a bit at the cases it lists, ``launch`` restates grid arithmetic that is still in the source, and the case table
names every path the GPU tests are there for."""
import pathlib
import re

import pytest
import torch
import torch.nn.functional as F

import stencil_emul as E

F64, BF16, I16 = torch.float64, torch.bfloat16, torch.int16
TOL = 1e-12


def _close(a, ref, mag, what):
    err = (a - ref).abs()
    assert a.shape == ref.shape, what
    assert bool((err <= TOL * mag).all()), (what, float((err / mag.clamp_min(1e-300)).max()))


def _ids(shapes):
    return [E.sid(s) for s in shapes]


# ---------------------------------------------------------------------------------------------------- against torch fp64
@pytest.mark.parametrize("shape", E.shapes("dwconv3x3")[:6], ids=_ids(E.shapes("dwconv3x3")[:6]))
def test_dwconv_stages_equal_fp64_conv2d_and_its_autograd(shape):
    N, H, W, C = shape
    i = E.inputs_for("dwconv3x3", shape)
    nchw = lambda t: t.to(F64).reshape(N, H, W, C).permute(0, 3, 1, 2)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(N * H * W, C)
    w = i["w9"].to(F64).t().reshape(C, 1, 3, 3)                 # [9, C] tap-major -> conv2d's [C, 1, ky, kx]
    xs, ws = nchw(i["x"]).clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv2d(xs, ws, padding=1, groups=C)
    y.backward(nchw(i["dy"]))
    mag = rows(F.conv2d(nchw(i["x"]).abs(), w.abs(), padding=1, groups=C))
    _close(E.call("dwconv3x3", shape)[0]["y"], rows(y.detach()), mag, "dwconv3x3")
    # the data gradient is the same stencil on dy with the taps reversed: the composition FullFT._block_bwd relies on
    mag_dx = rows(F.conv2d(nchw(i["dy"]).abs(), torch.flip(w.abs(), dims=[2, 3]), padding=1, groups=C))
    _close(E.call("dwconv3x3_dx", shape)[0]["dx"], rows(xs.grad), mag_dx, "dwconv3x3_dx")
    assert torch.equal(torch.flip(i["w9"], dims=[0]).to(F64).t().reshape(C, 1, 3, 3), torch.flip(w, dims=[2, 3]))


@pytest.mark.parametrize("shape", E.shapes("dwconv3x3_bwd_w"), ids=_ids(E.shapes("dwconv3x3_bwd_w")))
def test_dwconv_weight_gradient_equals_fp64_autograd(shape):
    N, H, W, C = shape
    i = E.inputs_for("dwconv3x3_bwd_w", shape)
    nchw = lambda t: t.to(F64).reshape(N, H, W, C).permute(0, 3, 1, 2)
    ws = torch.zeros(C, 1, 3, 3, dtype=F64, requires_grad=True)
    F.conv2d(nchw(i["x"]), ws, padding=1, groups=C).backward(nchw(i["dy"]))
    ref, bar = E.call("dwconv3x3_bwd_w", shape)
    mag = (bar["dw"] - E.HB * ref["dw"].abs()) / E.U            # >= sum|terms|
    _close(ref["dw"], ws.grad.reshape(C, 9).t(), mag + 1e-300, "dwconv3x3_bwd_w")


@pytest.mark.parametrize("shape", [(1, 1, 8), (2, 3, 8), (3, 35, 520), (2, 169, 96)], ids=_ids([(1, 1, 8), (2, 3, 8), (3, 35, 520), (2, 169, 96)]))
def test_squeeze_excite_stages_equal_fp64_autograd(shape):
    N, HW, C = shape
    i = E.inputs_for("se_pool", shape)
    x, dy = (i[k].to(F64).reshape(N, HW, C) for k in ("x", "dy"))
    xs, ss = x.clone().requires_grad_(True), i["s"].to(F64).requires_grad_(True)
    y = xs * torch.sigmoid(ss)[:, None]
    pooled = xs.mean(1)
    _close(E.se_pool(i["x"], N, HW, C)[0]["pooled"], pooled.detach(), x.abs().mean(1) + 1e-300, "se_pool")
    _close(E.se_scale(i["x"], i["s"], N, HW, C)[0]["y"], y.detach().reshape(-1, C), x.abs().reshape(-1, C) + 1e-300, "se_scale")
    y.backward(dy, retain_graph=True)
    _close(E.se_bwd_gate(i["x"], i["dy"], i["s"], N, HW, C)[0]["ds"], ss.grad, (x * dy).abs().sum(1) + 1e-300, "se_bwd_gate")
    _close(E.se_bwd_x(i["dy"], i["s"], None, N, HW, C)[0]["dx"], xs.grad.reshape(-1, C), dy.abs().reshape(-1, C), "se_bwd_x without dpool")
    pooled.backward(i["dpool"].to(F64))                          # accumulates the mean's gradient onto x's
    mag = (dy.abs() + i["dpool"].to(F64).abs()[:, None]).reshape(-1, C)
    _close(E.se_bwd_x(i["dy"], i["s"], i["dpool"], N, HW, C)[0]["dx"], xs.grad.reshape(-1, C), mag, "se_bwd_x")


@pytest.mark.parametrize("shape", E.shapes("im2col3d")[:5], ids=_ids(E.shapes("im2col3d")[:5]))
def test_im2col3d_is_conv3d_unfolded_and_col2im3d_its_adjoint(shape):
    B, T, H, W, C = shape
    T2, H2, W2 = T // 2 + 1, H // 2 + 1, W // 2 + 1
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B * T * H * W, C, dtype=F64, generator=g)
    cols = E.im2col3d(x, B, T, H, W, C)["cols"]
    assert cols.shape == (B * T2 * H2 * W2, 8 * C)
    # Conv3d(k 2, s 2, p 1) with one-hot kernels: output channel (tap, c) is the unfolded column itself
    w = torch.zeros(8, C, C, 2, 2, 2, dtype=F64)
    for tap in range(8):
        w[tap, torch.arange(C), torch.arange(C), tap >> 2, (tap >> 1) & 1, tap & 1] = 1
    xn = x.reshape(B, T, H, W, C).permute(0, 4, 1, 2, 3)
    ref = F.conv3d(xn, w.reshape(8 * C, C, 2, 2, 2), stride=2, padding=1).permute(0, 2, 3, 4, 1).reshape(-1, 8 * C)
    assert torch.equal(cols, ref)
    pad = E.padding_taps(T, H, W)
    assert int(pad.sum()) == 8 * T2 * H2 * W2 - T * H * W        # every real element sits in exactly one window
    assert bool((cols.reshape(B, -1, 8, C)[:, pad] == 0).all())
    d = torch.randn(cols.shape, dtype=F64, generator=g)          # padding taps hold "gradient" too: it must be ignored
    assert bool((d.reshape(B, -1, 8, C)[:, pad] != 0).all())
    dx = E.col2im3d(d, B, T, H, W, C)["dx"]
    lhs, rhs = float((d * cols).sum()), float((dx * x).sum())
    assert abs(lhs - rhs) <= TOL * float((d * cols).abs().sum())
    xs = x.clone().requires_grad_(True)
    (E.im2col3d(xs, B, T, H, W, C)["cols"] * d).sum().backward()
    assert torch.equal(dx, xs.grad)
    assert torch.equal(E.col2im3d(cols, B, T, H, W, C)["dx"], x)
    # the same on bit patterns, NaN payloads and -0 included
    i = E.inputs_for("im2col3d", shape)
    assert torch.equal(E.call("col2im3d_of_im2col", shape)["dx"], i["x"])


def test_ingest_stages_equal_torch():
    for shape in E.shapes("vit_assemble")[:3]:
        N, G, D = shape
        i = E.inputs_for("vit_assemble", shape)
        ref = torch.cat([i["cls"].to(F64).expand(N, 1, D), i["pe"].to(F64).reshape(N, G, D)], 1) + i["pos"].to(F64)[None]
        assert torch.equal(E.call("vit_assemble", shape)[0]["tok"], ref.reshape(-1, D))
        t = E.inputs_for("drop_cls", shape)["tok"]
        assert torch.equal(E.call("drop_cls", shape)["out"], t.reshape(N, G + 1, D)[:, 1:].reshape(-1, D))
    for shape in E.shapes("patchify"):
        N, H, W, P, Kpad = shape
        vis = E.inputs_for("patchify", shape)["vis"]
        got = E.call("patchify", shape)["patches"]
        K = 3 * P * P
        ref = F.unfold(vis, kernel_size=P, stride=P).transpose(1, 2).reshape(-1, K).to(BF16)      # column c P P + py P + px, patches row-major
        assert got.shape == (N * (H // P) * (W // P), Kpad)
        assert torch.equal(got[:, :K], ref.view(I16)) and bool((got[:, K:] == 0).all())
        assert K % 8 != 0 or Kpad > K


def test_patchify_inputs_sit_on_the_rounding_rule():
    sp = E._f32_from_bits(list(E.PATCHIFY_SPECIALS))
    got = sp.to(BF16).view(I16).tolist()
    u = lambda v: v - 65536 if v >= 32768 else v
    # halfway above an even value: down; above an odd value: up; one fp32 ulp beside halfway: to the nearer one
    assert got[:10] == [u(v) for v in (0x3F80, 0x3F82, 0xC0A0, 0xC0A2, 0x0080, 0x7F7E, 0x3F81, 0x3F81, 0xBF81, 0xBF81)]
    assert got[10:] == [u(v) for v in (0x0000, 0x8000, 0x0080, 0x8080, 0x7F7F, 0xFF7F)]
    for shape in E.shapes("patchify"):
        vis = E.inputs_for("patchify", shape)["vis"]
        a = vis.abs()
        assert bool(torch.isfinite(vis).all()) and bool(((a == 0) | (a >= 2.0 ** -126)).all())     # finite normals and +-0 only
        bits = vis.view(torch.int32)
        for s in E.PATCHIFY_SPECIALS:
            assert bool((bits == (s - 2 ** 32 if s >= 2 ** 31 else s)).any()), hex(s)


def test_copy_stages_equal_torch_and_inputs_span_the_bit_patterns():
    for shape in E.shapes("transpose"):
        x = E.inputs_for("transpose", shape)["x"]
        assert torch.equal(E.call("transpose", shape)["out"], x.t())
    for shape in E.shapes("transpose_pad"):
        Rr, C, ld_in, Rpad = shape
        x = E.inputs_for("transpose_pad", shape)["x"]
        out = E.call("transpose_pad", shape)["out"]
        assert out.shape == (C, Rpad) and torch.equal(out[:, :Rr], x[:, :C].t()) and bool((out[:, Rr:] == 0).all())
        assert ld_in % 8 == 0 and ld_in >= C and Rpad % 8 == 0 and Rpad >= Rr
    big = E.inputs_for("transpose", (300, 520))["x"].reshape(-1)
    v = big.view(BF16).float()
    assert bool(torch.isnan(v).any()) and bool(torch.isinf(v).any()) and bool(((v == 0) & torch.signbit(v)).any())
    assert bool(((v != 0) & (v.abs() < 2.0 ** -126)).any())                                   # denormals
    assert len(set(big.tolist())) > 50000                                                     # most of the 65536 patterns
    first = [b - 65536 if b >= 32768 else b for b in E.SPECIAL_BITS]
    assert big[: len(first)].tolist() == first


def test_splice_case_holds_the_positions_it_is_for():
    from vlb_oracle import VIDEO_TOKEN_ID
    for shape in E.shapes("splice_embed"):
        B, L, Nv, D = shape
        i = E.inputs_for("splice_embed", shape)
        ids = i["ids"]
        assert [int((ids[b] == VIDEO_TOKEN_ID).nonzero()[0]) for b in range(B)] == [0, L // 2, L - 1] and 0 < L // 2 < L - 1
        assert int((ids == VIDEO_TOKEN_ID).sum()) == B and (L - 1 + Nv) % 16 != 0
        assert ids[1, :2].tolist() == [0, 0] and ids[2, :3].tolist() == [0, 0, 0] and int((ids == 0).sum()) == 5
        ref = E.call("splice_embed", shape)
        assert ref["embeds"].shape == (B * (L - 1 + Nv), D) and ref["key_mask"].shape == (B, L - 1 + Nv)
        assert int((ref["key_mask"] == 0).sum()) == 5 and bool(ref["key_mask"][:, : Nv - 1].all())
        e = ref["embeds"].reshape(B, L - 1 + Nv, D)
        for b, pos in enumerate(i["video_pos"]):
            assert torch.equal(e[b, pos:pos + Nv], i["vid"][b])
            if pos > 0:
                assert torch.equal(e[b, 0], i["emb"][int(ids[b, 0])])
            if pos < L - 1:
                assert torch.equal(e[b, -1], i["emb"][int(ids[b, -1])])


def test_inputs_hold_what_the_bars_are_for():
    shape = (3, 5, 7, 96)
    N, H, W, C = shape
    i = E.inputs_for("dwconv3x3", shape)
    x, dy = (i[k].double().reshape(N, H, W, C) for k in ("x", "dy"))
    assert bool((x[..., 8:16] == 0).all()) and bool((x[..., :8] != 0).any())
    live = torch.cat([x[..., :8], x[..., 16:]], -1).abs()
    assert float(live[:, 0, W - 1].min()) >= E.CORNER and float(live.reshape(N, H * W, -1)[:, torch.arange(H * W) != W - 1].max()) < E.CORNER / 8
    assert float(dy[:, H - 1, 0].abs().min()) >= E.CORNER and float(dy[:, 0, W - 1].abs().max()) < E.CORNER / 8
    per_pos = live.reshape(N * H * W, -1).median(1).values
    assert float(per_pos.min()) < 2.0 ** -9 and float(per_pos[per_pos < E.CORNER].max()) > 2.0 ** 4       # 2^-10 .. 2^6
    s = E.inputs_for("se_scale", (3, 35, 520))
    assert s["s"][0, :8].float().tolist()[2:] == list(E.GATE_EDGES)[2:] and bool(torch.signbit(s["s"][0, 1].float()))
    xs = s["x"].double().reshape(3, 35, 520)
    assert bool((xs[..., 8:16] == 0).all()) and bool((xs[..., 512:] != 0).all())
    assert float(xs[:, -1, :8].abs().median()) > 16                                            # the last row carries the top scale


# ---------------------------------------------------------------------------------------------------- cases and launches
def test_launch_restates_the_launchers():
    """``launch`` is a restatement in Python; what can be held fast is the source: the grid arithmetic it copies is still
    what ops.hip, train.hip and gemm.hip launch with."""
    csrc = pathlib.Path(__file__).resolve().parent.parent / "phantom_vlb_amd" / "csrc"
    ops, train, gemm = (re.sub(r"\s+", " ", (csrc / n).read_text()) for n in ("ops.hip", "train.hip", "gemm.hip"))
    for cond in ("constexpr int kMaxBlocks = 256 * 8;",
                 "inline int grid_for(int64_t n, int block) { int64_t b = (n + block - 1) / block; return (int)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b)); }",
                 "const int lds = H * W * 64;",
                 "VLB_REQUIRE(lds <= 160 * 1024,",
                 "hipLaunchKernelGGL(dwconv3x3_kernel, dim3(C / 32, N), dim3(256), lds,",
                 "for (int p = threadIdx.x >> 2; p < HW; p += 64) {",
                 "hipLaunchKernelGGL(se_pool_kernel, dim3((C / 8 + 63) / 64, N), dim3(256),",
                 "const int c = (blockIdx.x * 64 + cc) * 8;",
                 "for (int r = rg; r < HW; r += 4) {",
                 "const int64_t total = (int64_t)N * HW * (C / 8); hipLaunchKernelGGL(se_scale_kernel, dim3(grid_for(total, 256)), dim3(256),",
                 "const int T2 = T / 2 + 1, H2 = H / 2 + 1, W2 = W / 2 + 1; const int64_t total = (int64_t)B * T2 * H2 * W2 * 8 * (C / 8); "
                 "hipLaunchKernelGGL(im2col3d_kernel, dim3(grid_for(total, 256)), dim3(256),",
                 "const int64_t total = (int64_t)N * (H / P) * (W / P) * (Kpad / 8); hipLaunchKernelGGL(patchify_kernel, dim3(grid_for(total, 256)), dim3(256),",
                 "const int64_t total = (int64_t)N * (G + 1) * (D / 8); hipLaunchKernelGGL(vit_assemble_kernel, dim3(grid_for(total, 256)), dim3(256),",
                 "const int64_t total = (int64_t)N * G * (D / 8); hipLaunchKernelGGL(drop_cls_kernel, dim3(grid_for(total, 256)), dim3(256),",
                 "const int S = L - 1 + Nv; hipLaunchKernelGGL(splice_kernel, dim3((S + 15) / 16, B), dim3(256),"):
        assert cond in ops, cond
    for cond in ("hipLaunchKernelGGL(dwconv_dw_partial_kernel, dim3((C / 8 + 255) / 256, N * H), dim3(256),",
                 "hipLaunchKernelGGL(colpart_reduce_kernel, dim3((9 * C + 31) / 32), dim3(256), 0, st, ws, N * H, 9 * C,",
                 "const int n = blockIdx.y / H, h = blockIdx.y % H;",
                 "hipLaunchKernelGGL(se_bwd_gate_kernel, dim3((C / 8 + 255) / 256, N), dim3(256),",
                 "const int c = (blockIdx.x * 256 + threadIdx.x) * 8; if (c >= C) return;",
                 "const int64_t total8 = (int64_t)N * HW * (C / 8); hipLaunchKernelGGL(se_bwd_x_kernel, dim3(blocks_for(total8, 256)), dim3(256),",
                 "const int T2 = T / 2 + 1, H2 = H / 2 + 1, W2 = W / 2 + 1; const int64_t total8 = (int64_t)B * T * H * W * (C / 8); "
                 "hipLaunchKernelGGL(col2im3d_kernel, dim3(blocks_for(total8, 256)), dim3(256),",
                 "inline int blocks_for(int64_t n, int block) { return (int)((n + block - 1) / block); }",
                 "dim3 grid((C + 63) / 64, (Rpad + 63) / 64);",
                 "if (c0 + cc + 8 <= C) v =",
                 "for (int b = grp; b < nb; b += 8) s += part[(int64_t)b * dim + c];"):
        assert cond in train, cond
    assert train.count("const int c = (blockIdx.x * 256 + threadIdx.x) * 8; if (c >= C) return;") == 2        # weight gradient, gate gradient
    assert "dim3 grid((C + 31) / 32, (R + 31) / 32), block(32, 8);" in gemm
    assert E.K_MAX_BLOCKS == 2048 and E.LDS_LIMIT == 163840


ALL_OPS = E.ARITH_OPS + E.BIT_OPS


@pytest.mark.parametrize("op", ALL_OPS)
def test_cases_lead_where_they_say(op):
    for shape, expect in E.CASES[op]:
        got = E.launch(op, shape)
        for k, v in expect.items():
            assert got[k] == v, (op, shape, k, got[k], v)


def test_case_table_names_every_path():
    L = lambda op: [E.launch(op, s) for s, _ in E.CASES[op]]
    dw = E.CASES["dwconv3x3"]
    assert any(s[1] != s[2] and s[1] > 1 and s[2] > 1 for s, _ in dw) and any(s[1] == 1 for s, _ in dw) and any(s[2] == 1 for s, _ in dw)
    assert {(5, 7), (7, 5)} <= {(s[1], s[2]) for s, _ in dw}                                                  # both orientations of one plane
    assert [l["above_64k"] for l in L("dwconv3x3")].count(True) == 2 and [l["refused"] for l in L("dwconv3x3")].count(True) == 1
    assert max(l["blocks_x"] for l in L("dwconv3x3")) >= 3 and max(l["position_trips"] for l in L("dwconv3x3") if not l["refused"]) >= 2
    assert all(s[1] * s[2] * 64 != E.LDS_LIMIT for s, _ in dw)                                                # the limit itself is not probed
    for op, per_block in (("se_pool", 64), ("se_bwd_gate", 256), ("dwconv3x3_bwd_w", 256)):
        ls = L(op)
        assert any(l["blocks_x"] == 2 and l["last_active"] == 1 for l in ls), op                              # second block, c < C guard
        assert any(l["blocks_x"] == 1 and 1 < l["last_active"] < per_block for l in ls), op
    assert {l["idle_row_groups"] for l in L("se_pool")} >= {0, 1, 3}
    lw = L("dwconv3x3_bwd_w")
    assert any(l["reduce_last_active"] != 32 for l in lw) and any(l["reduce_last_active"] == 32 for l in lw)  # 9 C a multiple of 32 or not
    assert any(l["slabs"] > 8 and l["slabs"] % 8 for l in lw) and any(l["slabs"] == 1 for l in lw)            # uneven reduce groups
    assert any(s[1] != s[2] for s, _ in E.CASES["dwconv3x3_bwd_w"])
    for op in ("se_scale", "im2col3d", "vit_assemble", "drop_cls", "patchify"):
        trips = [l for l in L(op) if l["second_trip"]]
        assert len(trips) == 1 and trips[0]["items"] % (E.K_MAX_BLOCKS * 256) != 0 and trips[0]["blocks"] == E.K_MAX_BLOCKS, op
    for op in ("im2col3d", "col2im3d"):
        pads = {l["trailing_pad"] for l in L(op)}
        assert (True, True, True) in pads and (False, False, False) in pads and len(pads) >= 4, op           # odd and even extents, mixed
        assert any(len({s[1], s[2], s[3]}) == 3 for s, _ in E.CASES[op]), op                                  # T, H, W all different
    assert any(l["straddle"] for l in L("patchify")) and any(s[1] != s[2] for s, _ in E.CASES["patchify"])
    tp = L("transpose_pad")
    assert any(l["scalar_tail"] for l in tp) and any(not l["scalar_tail"] for l in tp) and any(l["pad_octets"] > 0 for l in tp)
    assert any(l["grid"] == (2, 2) for l in tp)
    assert {s[3] for s, _ in E.CASES["splice_embed"]} == {8, 264} and all(l["last_rows"] < 16 for l in L("splice_embed"))


# ---------------------------------------------------------------------------------------------------- bars accept fp32
def _report(what, got, ref, bar):
    r, out = E.ratios(got, ref, bar), E.outside(got, ref, bar)
    print(what, {k: round(v, 3) for k, v in r.items()}, "outside:", out)
    assert all(v <= 1.0 for v in r.values()), (what, r)
    assert not any(out.values()), (what, out)


@pytest.mark.parametrize("op,shape", [(op, s) for op in E.ARITH_OPS for s in E.shapes(op)],
                         ids=[f"{op}-{E.sid(s)}" for op in E.ARITH_OPS for s in E.shapes(op)])
def test_bars_accept_the_fp32_restatement(op, shape):
    ref, bar = E.call(op, shape)
    _report(f"{op} {E.sid(shape)}", E.call(op, shape, emu=True), ref, bar)


# ---------------------------------------------------------------------------------------------------- bars reject bugs
def test_every_planted_bug_is_listed():
    assert set(E.BUGS) == {"hw_swapped", "tap_transposed", "no_pad_bottom_right", "border_wraps", "pool_div_padded", "pool_drop_last_row",
                           "drop_last_octet", "gate_grad_no_1mg", "dpool_not_divided", "im2col_tap_order", "col2im_unpadded_coords",
                           "assemble_pos_off_by_one", "drop_cls_keeps_cls", "patchify_channel_minor", "transpose_pad_tail_dropped",
                           "dw_flip_missing"}
    for bug, sites in E.BUGS.items():
        for op, shape in sites:
            assert shape in E.shapes(op), (bug, op, shape)


@pytest.mark.parametrize("bug,op,shape", [(b, op, s) for b, sites in E.BUGS.items() for op, s in sites],
                         ids=[f"{b}-{op}-{E.sid(s)}" for b, sites in E.BUGS.items() for op, s in sites])
def test_planted_bug_is_caught(bug, op, shape):
    """the stage with the bug planted (an arithmetic one rounded to bf16 as a device would write it) against the honest stage:
    an output leaves its bar, or a bit changes"""
    if op in E.BIT_OPS:
        d = E.bits_differ(E.call(op, shape, bug=bug), E.call(op, shape))
        print(bug, op, E.sid(shape), "bits differ:", d)
        assert max(d.values()) > 0, (bug, op, shape)
        return
    (ref, bar), (bad, _) = E.call(op, shape), E.call(op, shape, bug=bug)
    bad = {k: E.rbf(v) for k, v in bad.items()}
    r = E.ratios(bad, ref, bar)
    print(bug, op, E.sid(shape), {k: round(v, 2) for k, v in r.items()}, "outside:", E.outside(bad, ref, bar))
    assert max(r.values()) > 1.0, (bug, op, shape, r)
