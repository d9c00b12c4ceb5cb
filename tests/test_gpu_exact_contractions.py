"""Every MFMA contraction bit for bit on integer-valued operands (-m gpu): gemm.hip, gemm_fp8.hip and the skinny
contractions of lora.hip against the exact reference of tests/exact_ints.py, one case per route of the GEMM planner.

Operands are ternary, so fp32 accumulation is exact in any order and the outputs are integers bf16 holds exactly: the
linear epilogues are checked with ``assert_bits_equal`` (no tolerance), the non-linear ones with the derived element-wise
bar of ``assert_within_ulp``.  Every case names the route it is meant to enter and asserts the library's own decision
first (``vlb_gemm_kernel_choice`` / ``vlb_gemm_plan``: encodings of plan_route, the planner the dispatch runs, with the
alignment facts taken as met), so a planner change fails loudly instead of silently testing another kernel.  Every plain
route runs act NONE with all four (bias, residual) presences - the EPI_PLAIN, EPI_RESIDUAL and EPI_GENERIC + NONE nests of
the four-wave and split-K reduce kernels; tests/test_gpu_gemm_epilogues.py holds the table of epilogue kinds against
kernel instantiations and the activations on a fractional grid.  What the
library does not export - pick_order's tile order and the facts plan_route takes from the call itself (the 16-byte-store
rule, the pointer rules of the generic kernel) - is named next to the case that turns on it.

Shapes up to 2^30 multiply-adds take the reference from CPU fp64; larger ones build operands and the whole reference on
the device (fp32 matmul, exact on these operands) and confirm it against CPU fp64 on a row subsample.
"""
import pytest
import torch

import exact_ints as E

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
CPU_REF_MACS = 1 << 30
P_DROP, PAIR_SCALE = 0.5, 2.0          # 1/(1-p) = 2 and the 16-bit threshold 32768 are both exact

# ------------------------------------------------------------------ route tables: (route, M, N, K, K2, choice, plan with ws, how)
# choice: vlb_gemm_kernel_choice (0 generic 64x64, 1 = 256x256 tiles, 2 = 256x128 tiles); plan: vlb_gemm_plan with the
# workspace (tile rows * 1000 + tail mode * 100 + K splits; 0 when K + K2 < 4096); how: output / operand layout
PLAIN = [
    # generic 64x64
    ("generic ragged", 37, 100, 72, 0, 0, 0, ""),
    ("generic skinny M long K", 5, 128, 4096, 0, 0, 0, ""),
    ("generic M < 128", 127, 256, 64, 0, 0, 0, ""),
    ("generic ldc % 4 != 0", 300, 250, 128, 0, 0, 0, ""),
    ("generic C off by one element", 300, 256, 128, 0, 2, 0, "c+1"),         # the shape alone picks 256x128; (C % 8 != 0) -> generic
    ("generic K2 = 8", 300, 256, 128, 8, 0, 0, ""),
    ("generic K2 = 16", 300, 256, 128, 16, 0, 0, ""),
    ("generic K = 8", 300, 256, 8, 0, 0, 0, ""),
    # ping-pong 256x128: M on both sides of one and two 128-row halves, one / two / three K tiles
    *[(f"ping-pong 256x128 M={m} K={k}", m, 128, k, 0, 2, 0, "") for m in (129, 255, 257, 300) for k in (64, 128, 192)],
    ("ping-pong 256x128 N % 256 != 0", 1184, 384, 128, 0, 2, 0, ""),
    ("ping-pong 256x128 K2 = 64", 300, 128, 128, 64, 2, 0, ""),
    # ping-pong 256x256
    ("ping-pong 256x256 one K tile", 2048, 4096, 64, 0, 1, 0, ""),
    ("ping-pong 256x256 three K tiles", 2048, 4096, 192, 0, 1, 0, ""),
    ("ping-pong 256x256 one K tile + K2", 2048, 4096, 64, 64, 1, 0, ""),
    ("ping-pong 256x256 three K tiles + K2", 2048, 4096, 192, 64, 1, 0, ""),
    ("ping-pong 256x256 residual aliases C", 2048, 4096, 192, 0, 1, 0, "alias"),
    ("ping-pong 256x256 A a strided column view", 2048, 4096, 192, 64, 1, 0, "aview"),
    # non-wide stores: C rows 8-byte but not 16-byte aligned (GemmArgs::wide = 0; long K then stays on the ping-pong kernel)
    ("non-wide 256x128", 512, 256, 128, 0, 2, 0, "c+4"),
    ("non-wide 256x256 long K", 2048, 4096, 4096, 0, 1, 256001, "c+4"),
    # four-wave kernel
    ("four-wave NT=8", 2048, 4096, 4096, 0, 1, 256001, ""),
    ("four-wave NT=8, K + K2 crosses 4096 by K2", 2048, 4096, 4032, 64, 1, 256001, ""),
    ("four-wave NT=4", 600, 256, 4096, 0, 2, 256001, ""),
    ("four-wave NT=4 + K2", 600, 256, 4096, 64, 2, 256001, ""),
    # partial-wave plans
    ("ping-pong + 256x128 halves", 4500, 4096, 128, 0, 1, 0, ""),
    ("four-wave 192-row tiles + 192x128 halves", 4500, 4096, 4096, 0, 1, 192101, ""),
    ("four-wave 192-row tiles", 5861, 4096, 4096, 0, 1, 192001, ""),
    ("four-wave 192-row tiles + halves + K2", 3000, 6144, 4096, 64, 1, 192101, ""),
]
# split-K through the workspace: (route, M, N, K, K2, plan with the workspace, plan without)
SPLIT_K = [
    ("split-K 256-row x4", 5015, 4096, 4096, 0, 256204, 192001),
    ("split-K 192-row x3", 2573, 6144, 4096, 0, 192203, 192101),
    ("split-K 256-row x2 + K2", 5861, 4096, 14336, 64, 256202, 192001),
]
# tile order 2 (pick_order: A larger than W and above 128 MB; xcd_remap_pid deals full rounds of 256 tiles to the XCDs)
ORDER2 = [
    ("order 2, 128 tiles, no full round", 16384, 512, 4096, 256001, 256001),
    ("order 2, one full round of 256 tiles", 16384, 1024, 4096, 256001, 256001),
    # 16640 x 1280 no longer re-cuts its remainder: the cost model prefers 435 whole 192-row tiles (a full round + 179)
    ("order 2, full round + whole-tile remainder (192-row)", 16640, 1280, 4096, 192001, 192001),
    # ... the nearest shape that does: 65 x 6 = 390 tiles of 256 rows = a full round + 134 tiles re-cut into halves
    ("order 2, full round + re-cut remainder", 16640, 1536, 4096, 256101, 256101),
]
# gate/up + SwiGLU: (route, M, ff, K, K2, choice of [M, 2ff, K, K2], plan with ws) - the shapes of test_gemm_swiglu_save
SWIGLU = [
    ("generic", 40, 48, 64, 16, 0, 0),
    ("ping-pong 256x128", 512, 256, 128, 64, 2, 0),
    ("four-wave NT=4, M tail", 1000, 512, 4096, 64, 2, 256001),
    ("four-wave + split-K tail", 5015, 2048, 4096, 64, 1, 256204),
]
# masked pair: (M, N, K, plan with the workspace under the masked-pair rules, plan without; 0 = not exported below K + 64 = 4096)
MASKED = [(700, 512, 256, 0, 0), (300, 256, 128, 0, 0), (4500, 4096, 256, 0, 0), (5009, 4096, 4096, 192001, 192001),
          (2573, 6144, 4096, 192203, 192101), (5861, 4096, 4096, 192001, 192001)]
MASKED_SWIGLU_BWD = [(700, 512, 256), (2573, 6144, 4096)]
MXFP8 = [(77, 256, 128), (300, 512, 1024), (5861, 4096, 512), (3000, 3072, 256)]

# every (K, K2) a bf16-output case above contracts over (tests/test_cpu_exact_ints.py proves the 256 cap for each); the
# masked pair's 2 * keep * (64 products) has the variance of 128 plain products
ALL_K_K2 = sorted({(c[3], c[4]) for c in PLAIN} | {(c[3], c[4]) for c in SPLIT_K} | {(c[3], 0) for c in ORDER2} |
                  {(c[3], c[4]) for c in SWIGLU} | {(c[2], 128) for c in MASKED} | {(c[2], 128) for c in MASKED_SWIGLU_BWD} |
                  {(c[2], 0) for c in MXFP8})


def _ids(table):
    return [f"{c[0]} [{'x'.join(str(v) for v in c[1:5])}]" if isinstance(c[0], str) else "x".join(str(v) for v in c[:3]) for c in table]


def _seed(*shape):
    return 1000 + sum(int(s) * (i + 1) for i, s in enumerate(shape))


def _on_device(M, N, Ktot):
    return M * N * Ktot > CPU_REF_MACS


class _SplitK:
    """ops.split_k_tails for the duration of a block."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from phantom_vlb_amd import ops
        self.old, ops.split_k_tails = ops.split_k_tails, self.on

    def __exit__(self, *a):
        from phantom_vlb_amd import ops
        ops.split_k_tails = self.old


def _passes_ws(M, N, Ktot):
    """ops.gemm hands the workspace to the library (more than one wave of tiles, long K)."""
    return Ktot >= 4096 and M * N > 256 * 192 * 256


def _assert_route(M, N, K, K2, choice, plan_ws, plan_nows=None):
    from phantom_vlb_amd._lib import lib
    assert lib.vlb_gemm_kernel_choice(M, N, K, K2) == choice, "the planner no longer picks this case's tile kernel"
    assert lib.vlb_gemm_plan(M, N, K, K2, 1) == plan_ws, "the planner no longer cuts this case as the route says"
    if plan_nows is not None:
        assert lib.vlb_gemm_plan(M, N, K, K2, 0) == plan_nows


def _offset_out(M, N, off, dev):
    """[M, N] output view that starts ``off`` elements into a sentinel-filled buffer (torch allocations are 256-byte
    aligned, so the view's address is off * 2 mod 16), and the buffer for the out-of-bounds check."""
    buf = torch.full((M * N + off + 64,), 7.0, dtype=BF, device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf[off:off + M * N].view(M, N), buf


def _assert_guards(buf, M, N, off):
    assert bool((buf[:off] == 7.0).all()) and bool((buf[off + M * N:] == 7.0).all()), "wrote outside the output view"


def _plain_operands(M, N, K, K2, dev, how=""):
    s = _seed(M, N, K, K2)
    on_dev = _on_device(M, N, K + K2)
    gdev = dev if on_dev else None                  # large shapes are generated where they are used
    if how == "aview":
        big = E.ternary((M, 3 * K), s, gdev).to(dev)
        a = big[:, K:2 * K]                         # row stride 3K
        assert a.stride(0) == 3 * K
    else:
        a = E.ternary((M, K), s, gdev).to(dev)
    w = E.ternary((N, K), s + 1, gdev).to(dev)
    a2 = w2 = None
    if K2:
        a2, w2 = E.ternary((M, K2), s + 2, gdev).to(dev), E.ternary((N, K2), s + 3, gdev).to(dev)
    bias, res = E.bias_ints(N, s + 4, gdev).to(dev), E.residual_ints(M, N, s + 5, gdev).to(dev)
    if on_dev:
        pre = E.device_pre(a, w, a2, w2, bias)
        E.confirm_rows(pre, a, w, a2, w2, bias, seed=s)
    else:
        pre = E.exact_pre(a, w, a2, w2, bias).to(dev)
    return a, w, a2, w2, bias, res, pre


def _run_plain(dev, a, w, a2, w2, bias, res, pre, how="", act_silu=True):
    """act NONE with integer bias and residual: bit-equal.  act SILU: within the ulp bar of silu(exact integers) + residual.
    Then act NONE with each other (bias, residual) presence - the four-wave and reduce kernels' EPI_RESIDUAL, EPI_PLAIN and
    EPI_GENERIC + NONE with a null residual, the null sides of ``if (p.bias)`` / ``if (p.residual)`` elsewhere - from the same
    operands and the same ``pre``: bit-equal to ``pre - bias`` (+ residual) where the bias is absent."""
    from phantom_vlb_amd import ops
    M, N = pre.shape
    exact = pre.double() + res.double()
    off = {"c+1": 1, "c+4": 4}.get(how, 0)

    def output(with_res):
        if off:
            out, buf = _offset_out(M, N, off, dev)
            assert out.data_ptr() % 16 == (2 * off) % 16
            return out, res, buf
        if how == "alias" and with_res:
            out = res.clone()                       # residual aliases C
            return out, out, None
        return torch.full((M, N), 7.0, dtype=BF, device=dev), res, None

    for act in (ops.ACT_NONE, ops.ACT_SILU) if act_silu else (ops.ACT_NONE,):
        out, residual, buf = output(True)
        got = ops.gemm(a, w, bias=bias, residual=residual, act=act, a2=a2, w2=w2, out=out)
        if act == ops.ACT_NONE:
            E.assert_bits_equal(got, exact)
        else:
            E.assert_within_ulp(got, E.ACTS["silu"](pre.double()) + res.double(), pre)
        if buf is not None:
            _assert_guards(buf, M, N, off)
    pre_nb = pre.double() - bias.double()[None, :]                                  # exact: integers
    for with_bias, with_res in ((False, False), (False, True), (True, False)):
        out, residual, buf = output(with_res)
        got = ops.gemm(a, w, bias=bias if with_bias else None, residual=residual if with_res else None, a2=a2, w2=w2, out=out)
        try:
            E.assert_bits_equal(got, (pre.double() if with_bias else pre_nb) + (res.double() if with_res else 0))
        except AssertionError as e:
            raise AssertionError(f"act NONE, bias {with_bias}, residual {with_res}: {e}") from None
        if buf is not None:
            _assert_guards(buf, M, N, off)


# ------------------------------------------------------------------ vlb_gemm_bf16(_ws)
@pytest.mark.parametrize("route,M,N,K,K2,choice,plan,how", PLAIN, ids=_ids(PLAIN))
def test_gemm_routes(dev, route, M, N, K, K2, choice, plan, how):
    _assert_route(M, N, K, K2, choice, plan)
    ops_in = _plain_operands(M, N, K, K2, dev, how)
    for split in ((True, False) if _passes_ws(M, N, K + K2) else (True,)):       # no split-K in these plans: both must agree anyway
        with _SplitK(split):
            _run_plain(dev, *ops_in, how=how, act_silu=split)


@pytest.mark.parametrize("route,M,N,K,K2,plan_ws,plan_nows", SPLIT_K, ids=_ids(SPLIT_K))
def test_gemm_split_k_tail_routes(dev, route, M, N, K, K2, plan_ws, plan_nows):
    """The partial last wave cut along K through the workspace and, with split_k_tails off, re-cut or whole: both equal the
    reference bit for bit, and therefore each other - whatever the fp32 summation order."""
    assert _passes_ws(M, N, K + K2)
    _assert_route(M, N, K, K2, 1, plan_ws, plan_nows)
    assert (plan_ws // 100) % 10 == 2 and (plan_nows // 100) % 10 != 2
    ops_in = _plain_operands(M, N, K, K2, dev)
    for split in (True, False):
        with _SplitK(split):
            _run_plain(dev, *ops_in)


@pytest.mark.parametrize("route,M,N,K,plan_ws,plan_nows", ORDER2, ids=[f"{c[0]} [{c[1]}x{c[2]}x{c[3]}]" for c in ORDER2])
def test_gemm_tile_order_2(dev, route, M, N, K, plan_ws, plan_nows):
    assert 2.0 * M * K > 2.0 * N * K and 2.0 * M * K > 128e6            # pick_order's rule for order 2, restated
    _assert_route(M, N, K, 0, 1, plan_ws, plan_nows)
    ops_in = _plain_operands(M, N, K, 0, dev)
    _run_plain(dev, *ops_in)


# ------------------------------------------------------------------ SWIGLU_PAIR and vlb_gemm_swiglu_save
def _swiglu_save(a, w_il, a2, w2_il, h, gu, ws):
    from phantom_vlb_amd._lib import check, lib
    M, K = a.shape
    N = w_il.shape[0]
    K2 = 0 if a2 is None else a2.shape[1]
    check(lib.vlb_gemm_swiglu_save(a.data_ptr(), a.stride(0), w_il.data_ptr(), w_il.stride(0), h.data_ptr(), h.stride(0), gu.data_ptr(),
                                   gu.stride(0), M, N, K, None if a2 is None else a2.data_ptr(), 0 if a2 is None else a2.stride(0),
                                   None if a2 is None else w2_il.data_ptr(), 0 if a2 is None else w2_il.stride(0), K2,
                                   None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(),
                                   torch.cuda.current_stream().cuda_stream), "vlb_gemm_swiglu_save")


@pytest.mark.parametrize("gu_off", [0, 4])
@pytest.mark.parametrize("route,M,ff,K,K2,choice,plan", SWIGLU, ids=_ids(SWIGLU))
def test_gemm_swiglu_routes(dev, route, M, ff, K, K2, choice, plan, gu_off):
    """[gate | up] bit-equal, h within the ulp bar of silu(g) * u of the exact integers; through vlb_gemm_swiglu_save (with
    the LoRA pair, and with GU rows 8- but not 16-byte aligned -> the non-wide epilogue) and through ACT_SWIGLU_PAIR."""
    from phantom_vlb_amd import ops
    N = 2 * ff
    _assert_route(M, N, K, K2, choice, plan)
    s = _seed(M, ff, K, K2)
    gdev = dev if _on_device(M, N, K + K2) else None
    a, t = E.ternary((M, K), s, gdev).to(dev), E.ternary((M, K2), s + 1, gdev).to(dev)
    wg, wu = E.ternary((ff, K), s + 2, gdev).to(dev), E.ternary((ff, K), s + 3, gdev).to(dev)
    bg, bu = E.ternary((ff, K2), s + 4, gdev).to(dev), E.ternary((ff, K2), s + 5, gdev).to(dev)
    w_cat, b_cat = torch.cat([wg, wu], 0), torch.cat([bg, bu], 0)
    if gdev is not None:
        pre = E.device_pre(a, w_cat, t, b_cat)
        E.confirm_rows(pre, a, w_cat, t, b_cat, seed=s)
    else:
        pre = E.exact_pre(a, w_cat, t, b_cat).to(dev)
    g64, u64 = pre[:, :ff].double(), pre[:, ff:].double()
    h_ref = E.ACTS["silu"](g64) * u64
    w_il, b_il = ops.interleave_gate_up(wg, wu), ops.interleave_gate_up(bg, bu)
    for split in ((True, False) if _passes_ws(M, N, K + K2) else (True,)):
        with _SplitK(split):
            h = torch.full((M, ff), 7.0, dtype=BF, device=dev)
            gu, buf = _offset_out(M, N, gu_off, dev)
            _swiglu_save(a, w_il, t, b_il, h, gu, ops._gemm_workspace(dev) if _passes_ws(M, N, K + K2) else None)
            E.assert_bits_equal(gu, pre)
            _assert_guards(buf, M, N, gu_off)
            E.assert_within_ulp(h, h_ref, g64)
            if gu_off == 0:
                h2 = ops.gemm(a, w_il, act=ops.ACT_SWIGLU_PAIR, a2=t, w2=b_il)
                E.assert_within_ulp(h2, h_ref, g64)
                h3, gu3 = ops.gemm_swiglu_save(a, w_il, a2=t, w2_il=b_il)       # the product wrapper
                assert torch.equal(h3, h) and torch.equal(gu3, gu)


# ------------------------------------------------------------------ masked pair
def _masked_operands(M, N, K, dev, seed):
    gdev = dev if _on_device(M, N, K + 64) else None
    a, w = E.ternary((M, K), seed, gdev).to(dev), E.ternary((N, K), seed + 1, gdev).to(dev)
    u, at = E.ternary((M, 64), seed + 2, gdev).to(dev), E.ternary((N, 64), seed + 3, gdev).to(dev)
    mseed = 0x1234ABCD ^ seed
    if gdev is not None:
        pre = E.device_pre(a, w, u, at, keep=E.keep_mask_device(mseed, M, N, P_DROP, dev), pair_scale=PAIR_SCALE)
        E.confirm_rows(pre, a, w, u, at, keep_seed=mseed, keep_p=P_DROP, pair_scale=PAIR_SCALE, seed=seed)
    else:
        pre = E.exact_pre(a, w, u, at, keep=E.keep_mask(mseed, M, N, P_DROP), pair_scale=PAIR_SCALE).to(dev)
    return a, w, u, at, mseed, pre


@pytest.mark.parametrize("M,N,K,plan_ws,plan_nows", MASKED, ids=_ids(MASKED))
def test_gemm_masked_pair_bit_exact(dev, M, N, K, plan_ws, plan_nows):
    """A.W^T + 2 * keep o (U.At^T), all 64 columns of the pair live."""
    from phantom_vlb_amd import ops
    from phantom_vlb_amd._lib import lib
    assert ops.gemm_masked_pair_ok(M, N, K)
    assert lib.vlb_gemm_plan(M, N, K, 64, 3) == plan_ws and lib.vlb_gemm_plan(M, N, K, 64, 2) == plan_nows      # bit 1: masked-pair rules
    a, w, u, at, mseed, pre = _masked_operands(M, N, K, dev, _seed(M, N, K))
    for split in ((True, False) if _passes_ws(M, N, K + 64) else (True,)):
        with _SplitK(split):
            out = torch.full((M, N), 7.0, dtype=BF, device=dev)
            E.assert_bits_equal(ops.gemm_masked_pair(a, w, u, at, P_DROP, mseed, out=out), pre)


@pytest.mark.parametrize("M,ff,K", MASKED_SWIGLU_BWD, ids=_ids(MASKED_SWIGLU_BWD))
def test_gemm_masked_pair_swiglu_bwd_from_exact_dh(dev, M, ff, K):
    """[d gate | d up] = SwiGLU backward of the exact integer d_h = dy.W^T + 2 keep o (u.At^T) at integer [gate | up]."""
    from phantom_vlb_amd import ops
    a, w, u, at, mseed, dh = _masked_operands(M, ff, K, dev, _seed(M, ff, K, 1))
    gu = E.gate_up_ints(M, 2 * ff, _seed(M, ff, K, 2), dev)
    dh = dh.double()
    g, up = gu[:, :ff].double(), gu[:, ff:].double()
    sg = torch.sigmoid(g)
    ref = torch.cat([dh * up * sg * (1 + g * (1 - sg)), dh * g * sg], 1)
    x = torch.cat([dh, dh], 1)
    for split in ((True, False) if _passes_ws(M, ff, K + 64) else (True,)):
        with _SplitK(split):
            E.assert_within_ulp(ops.gemm_masked_pair_swiglu_bwd(a, w, gu, u, at, P_DROP, mseed), ref, x)


# ------------------------------------------------------------------ MX-fp8
E4M3 = (0x00, 0x38, 0xB8)              # 0, +1, -1


def _mx_operand(rows, K, seed, dev, mixed):
    """(e4m3 bytes, E8M0 scale bytes, dequantised fp32) built directly: no quantiser in the loop."""
    v = E.small_ints((rows, K), -1, 1, seed, dev, dtype=torch.int64)
    q = torch.tensor(E4M3, dtype=torch.uint8, device=dev)[v % 3]          # -1 % 3 == 2 -> 0xB8
    s = E.small_ints((rows, K // 32), 126, 128, seed + 1, dev, dtype=torch.uint8) if mixed else torch.full((rows, K // 32), 127, dtype=torch.uint8, device=dev)
    deq = (v.view(rows, K // 32, 32).float() * torch.exp2(s.float() - 127)[..., None]).view(rows, K)
    return q.contiguous(), s.contiguous(), deq


@pytest.mark.parametrize("mixed", [False, True], ids=["scales 127", "scales 126..128"])
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("M,N,K", MXFP8, ids=_ids(MXFP8))
def test_gemm_mxfp8_bit_exact(dev, M, N, K, with_res, mixed):
    """All scales 2^0: integers under the cap.  Per-block scales 2^-1 .. 2^1 on both operands: exact multiples of 1/4, and
    the output is the bf16 round-to-nearest-even of the exact value (the rounding itself is checked, so no cap)."""
    from phantom_vlb_amd import ops
    s = _seed(M, N, K)
    aq, sa, ad = _mx_operand(M, K, s, dev, mixed)
    wq, sw, wd = _mx_operand(N, K, s + 2, dev, mixed)
    res = E.residual_ints(M, N, s + 4, dev) if with_res else None
    if _on_device(M, N, K):
        pre = ad @ wd.t()
        rows = torch.as_tensor(E.row_subsample(M, s), device=dev)
        assert torch.equal(pre[rows].double().cpu(), ad[rows].double().cpu() @ wd.double().cpu().t())
    else:
        pre = (ad.double().cpu() @ wd.double().cpu().t()).to(dev)
    assert bool((pre * 4 == (pre * 4).round()).all())
    exact = pre.double() + (res.double() if with_res else 0)
    out = torch.full((M, N), 7.0, dtype=BF, device=dev)
    E.assert_bits_equal(ops.gemm_mxfp8(aq, sa, wq, sw, residual=res, out=out), exact, cap=not mixed)


# ------------------------------------------------------------------ skinny contractions (lora.hip)
def _pad64(t):
    out = torch.zeros(t.shape[0], 64, dtype=BF, device=t.device)
    out[:, :t.shape[1]] = t
    return out


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("M", [1, 200, 257])
@pytest.mark.parametrize("R", [16, 32, 48])
def test_lora_down_bit_exact(dev, R, M, p):
    from phantom_vlb_amd.lora import lora_down
    K, scale = 288, 2.0
    s = _seed(R, M, int(2 * p))
    x, A = E.ternary((M, K), s), E.ternary((R, K), s + 1)
    seeds = [11 + 7 * g for g in range(R // 16)]
    ref = torch.full((M, 64), 7.0, dtype=torch.float64)                     # columns >= R are not written
    for g in range(R // 16):
        xm = x.double() * (E.keep_mask(seeds[g], M, K, p).double() / (1 - p) if p > 0 else 1.0)
        ref[:, 16 * g:16 * g + 16] = scale * xm @ A[16 * g:16 * g + 16].double().t()
    out = torch.full((M, 64), 7.0, dtype=BF, device=dev)
    lora_down(x.to(dev), A.to(dev), R, scale, p, seeds, out)
    E.assert_bits_equal(out, ref)


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("M", [1, 100, 257])
@pytest.mark.parametrize("R", [16, 32, 48])
def test_lora_dx_masked_bit_exact(dev, R, M, p):
    """dx += sum_g keep_g o (u_g.A_g) / (1-p) on integer dx_in: the += rounds once (the reference rounds the exact sum)."""
    from phantom_vlb_amd.lora import lora_dx_masked
    K = 1088                                                              # two column blocks of 1024, the second partial
    s = _seed(R, M, int(2 * p), 3)
    u, A, dx0 = E.ternary((M, R), s), E.ternary((R, K), s + 1), E.small_ints((M, K), -128, 128, s + 2)
    seeds = [3 + g for g in range(R // 16)]
    ref = dx0.double()
    for g in range(R // 16):
        term = u[:, 16 * g:16 * g + 16].double() @ A[16 * g:16 * g + 16].double()
        ref = ref + (term * E.keep_mask(seeds[g], M, K, p).double() / (1 - p) if p > 0 else term)
    dx = dx0.to(dev)
    lora_dx_masked(_pad64(u.to(dev)), _pad64(A.t().contiguous().to(dev)), dx, R, p, seeds)
    E.assert_bits_equal(dx, ref)


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("M", [1, 64, 700, 2048])
@pytest.mark.parametrize("N", [16, 32, 48])
def test_wgrad_skinny_bit_exact(dev, N, M, p):
    """dW fp32 = alpha/(1-p) G^T keep(X) + beta dW, beta = 0 then beta = 1; M across the row splits of vlb_wgrad_splits."""
    from phantom_vlb_amd._lib import lib
    from phantom_vlb_amd.lora import wgrad_skinny
    assert [lib.vlb_wgrad_splits(m) for m in (1, 64, 700, 2048)] == [1, 1, 3, 8]
    K, alpha = 776, 0.5
    s = _seed(N, M, int(2 * p), 5)
    G, Xw = E.ternary((M, N), s), E.ternary((M, K + 64), s + 1)
    seeds = [99 + 5 * g for g in range(N // 16)]
    ref = torch.zeros(N, K, dtype=torch.float64)
    for g in range(N // 16):
        xm = Xw[:, :K].double() * (E.keep_mask(seeds[g], M, K, p).double() / (1 - p) if p > 0 else 1.0)
        ref[16 * g:16 * g + 16] = alpha * G[:, 16 * g:16 * g + 16].double().t() @ xm
    X = Xw.to(dev)[:, :K]                                                 # strided view
    dW = torch.full((N, K), 7.0, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.vlb_wgrad_splits(M) * N * K, dtype=torch.float32, device=dev)
    Gd = _pad64(G.to(dev))
    wgrad_skinny(Gd, X, dW, ws, N, alpha=alpha, beta=0.0, p=p, seeds=seeds)
    E.assert_bits_equal(dW, ref)
    wgrad_skinny(Gd, X, dW, ws, N, alpha=alpha, beta=1.0, p=p, seeds=seeds)
    E.assert_bits_equal(dW, 2 * ref)


@pytest.mark.parametrize("M", [300, 2500])
@pytest.mark.parametrize("cols", [[256], [512, 256, 256]], ids=["256", "512+256+256"])
def test_wgrad_skinny_u_single_and_multi_bit_exact(dev, cols, M):
    """dB^T = t^T dy (fp32) and u = 2 dy.B (bf16) per projection and for the projections sharing one dy in one launch."""
    from phantom_vlb_amd._lib import lib
    from phantom_vlb_amd.lora import wgrad_skinny_u, wgrad_skinny_u_multi
    n, K = len(cols), sum(cols)
    s = _seed(M, K, n)
    t, dyw = E.ternary((M, 16 * n), s), E.ternary((M, K + 64), s + 1)
    bts = [E.ternary((16, c), s + 2 + j) for j, c in enumerate(cols)]
    td, dy = _pad64(t.to(dev)), dyw.to(dev)[:, :K]                        # strided view, as dqkv's column slices are
    btd = [b.to(dev) for b in bts]
    ws = torch.empty(lib.vlb_wgrad_splits(M) * 16 * K, dtype=torch.float32, device=dev)
    uws = torch.empty(lib.vlb_wgrad_u_ws_floats(M, K), dtype=torch.float32, device=dev)
    dws = [torch.full((16, c), 7.0, dtype=torch.float32, device=dev) for c in cols]
    u = torch.full((M, 64), 7.0, dtype=BF, device=dev)
    wgrad_skinny_u_multi(td, dy, cols, dws, btd, ws, 2.0, u, uws)
    u_ref = torch.full((M, 64), 7.0, dtype=torch.float64)
    c0 = 0
    for j, c in enumerate(cols):
        dyj = dyw[:, c0:c0 + c].double()
        dw_ref = t[:, 16 * j:16 * j + 16].double().t() @ dyj
        u_ref[:, 16 * j:16 * j + 16] = 2.0 * dyj @ bts[j].double().t()
        E.assert_bits_equal(dws[j], dw_ref)
        dw1 = torch.full((16, c), 7.0, dtype=torch.float32, device=dev)
        u1 = torch.full((M, 16), 7.0, dtype=BF, device=dev)
        wgrad_skinny_u(td[:, 16 * j:16 * j + 16], dy[:, c0:c0 + c], dw1, ws, btd[j], 2.0, u1, uws)
        E.assert_bits_equal(dw1, dw_ref)
        E.assert_bits_equal(u1, u_ref[:, 16 * j:16 * j + 16])
        wgrad_skinny_u(td[:, 16 * j:16 * j + 16], dy[:, c0:c0 + c], dw1, ws, btd[j], 2.0, u1, uws, alpha=1.0, beta=1.0)
        E.assert_bits_equal(dw1, 2 * dw_ref)                              # beta = 1 accumulates
        c0 += c
    E.assert_bits_equal(u, u_ref)                                         # columns >= 16 n untouched


@pytest.mark.parametrize("row_map", [0, 1, 2], ids=["plain", "gate", "up"])
@pytest.mark.parametrize("scale", [0.5, 2.0])
@pytest.mark.parametrize("R", [16, 64])
def test_lora_merge_bit_exact(dev, R, scale, row_map):
    """Wm[row(n)] = bf16(W[row(n)] + scale * Bt[:, n].A) with W in [-64, 64]: |exact| <= 192, multiples of 1/2, one rounding.
    N = 160 ends inside a block's row band, K = 328 inside a lane's columns; rows outside the map keep their bytes."""
    from phantom_vlb_amd import ops
    N, K = 160, 328
    s = _seed(R, int(2 * scale), row_map, 9)
    rows = N if row_map == 0 else 2 * N
    W, Bt, A = E.small_ints((rows, K), -64, 64, s), E.ternary((R, N), s + 1), E.ternary((R, K), s + 2)
    n = torch.arange(N)
    idx = n if row_map == 0 else 32 * (n // 16) + (16 if row_map == 2 else 0) + n % 16
    ref = torch.full((rows, K), 7.0, dtype=torch.float64)
    ref[idx] = W[idx].double() + scale * (Bt.double().t() @ A.double())
    Wd = W.to(dev)
    Wm = torch.full((rows, K), 7.0, dtype=BF, device=dev)
    ops.lora_merge(Wd, Wm, Bt.to(dev), A.to(dev), scale, row_map)
    E.assert_bits_equal(Wm, ref)
    assert torch.equal(Wd.cpu(), W)                                       # the base weight is read only
