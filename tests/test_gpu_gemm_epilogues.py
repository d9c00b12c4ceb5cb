"""Every compiled GEMM epilogue on every planner route, per element (-m gpu): gemm.hip compiles its epilogue as separate,
fully unrolled nests chosen at run time, and this file and tests/test_gpu_exact_contractions.py (G below) enter each of
them on each kernel instantiation of ``launch_kernel`` - bit for bit where the epilogue is linear, within the derived
element-wise bar of ``exact_ints.ulp_bar`` where it is not.

Kinds.  Four-wave kernel and gemm_splitk_reduce_kernel: ``w4_epilogue_kind`` picks EPI_PLAIN (no bias, no activation, no
residual), EPI_RESIDUAL (residual only), EPI_SWIGLU_BWD or EPI_GENERIC + act (NONE / QUICK_GELU / GELU / SILU; inside it
``if (p.bias)`` and ``if (p.residual)`` are run-time branches); ACT_SWIGLU_PAIR is a path of its own.  Ping-pong kernels:
one nest per activation (PP_EPILOGUE_WIDE with 16-byte stores, PP_EPILOGUE_NARROW without), bias / residual at run time -
their "PLAIN" and "RESIDUAL" below are the NONE nest with the null pointers.  Generic kernel: run-time ``apply_act``.

Cases.
  P  = G.test_gemm_routes / test_gemm_split_k_tail_routes / test_gemm_tile_order_2: act NONE with all four (bias,
       residual) presences on the integer operands, bit-equal -> PLAIN, RESIDUAL, GENERIC + NONE (bias alone, bias +
       residual); and SILU with both, in saturation
  L  = test_gemm_residual_only_layouts: RESIDUAL with the residual aliasing C and as a column view (ldr = N + 64)
  A  = test_gemm_grid_activations: QUICK_GELU, GELU and SILU, each with all four presences, on the fractional grid
  S  = G.test_gemm_swiglu_routes (integers) and test_gemm_swiglu_grid: SWIGLU_PAIR with and without the saved [gate | up]
  Mk = G.test_gemm_masked_pair_bit_exact and test_gemm_masked_pair_recut_halves: the masked pair, PLAIN
  B  = G.test_gemm_masked_pair_swiglu_bwd_from_exact_dh (integer gate / up) and test_gemm_masked_pair_swiglu_bwd_grid

  instantiation (launch_kernel)        PLAIN, RESIDUAL, GENERIC+NONE   QUICK_GELU, GELU, SILU    SWIGLU_PAIR
  generic 64x64                        P 37x100x72 (L too)             A 37x100x72               S 40x96x64+16
  ping-pong 256x256, wide              P 2048x4096x192+64              A 2048x4096x192+64        S 2048x4096x64+64
  ping-pong 256x256, narrow            P 2048x4096x4096 c+4            A 2048x4096x64 c+4        S 5015x4096x4096+64 gu+4
  ping-pong 256x128, wide              P 300x128x192 (L too)           A 300x128x192             S 512x512x128+64
  ping-pong 256x128, narrow            P 512x256x128 c+4               A 512x256x128 c+4         S 512x512x128+64 gu+4
  four-wave NT 8, MT 8                 P, L 2048x4096x4096             A 2048x4096x4096          S 5015x4096x4096+64 (main launch)
  four-wave NT 4, MT 8                 P, L 600x256x4096(+64)          A 600x256x4096+64         S 1000x1024x4096+64
  four-wave NT 8, MT 6                 P, L 5861x4096x4096             A 5861x4096x4096          S 4500x4096x4096+64
  four-wave NT 4, MT 6                 P 4500x4096x4096 (tail halves)  A 4500x4096x4096          S 4500x4096x4096+64 (tail halves)
  split-K + reduce MT 8                P, L 5015x4096x4096             A 5015x4096x4096 (and     S 5015x4096x4096+64
                                                                       5861x4096x14336+64)
  split-K + reduce MT 6                P, L 2573x6144x4096             A 2573x6144x4096          S 2573x6144x4096+64
  (SWIGLU_PAIR takes N = 2 ff; the split-K rows enter the reduce kernel's kind with split_k_tails on and the whole-tile or
  re-cut kernels of the same row with it off.)

  EPI_SWIGLU_BWD in the instantiations above: not reachable - only vlb_gemm_masked_pair_swiglu_bwd sets that activation, and
  masked_pair_impl routes to the MASKED instantiations alone.

  MASKED instantiation                 PLAIN                            SWIGLU_BWD
  four-wave NT 8, MT 8                 Mk 700x512x256                   B 700x512x256
  four-wave NT 4, MT 8                 Mk 16640x1536x4032 (tail halves) B 16640x1536x4032 (tail halves)
  four-wave NT 8, MT 6                 Mk 5861x4096x4096                B 2573x6144x4096 (main launch)
  four-wave NT 4, MT 6                 Mk 2573x6144x4096, no workspace  B 2573x6144x4096, no workspace
  split-K + reduce MT 6                Mk 2573x6144x4096                B 2573x6144x4096
  RESIDUAL, GENERIC + act and SWIGLU_PAIR in the MASKED instantiations: not reachable - masked_pair_impl passes no bias, a
  residual only as the saved [gate | up] of SWIGLU_BWD, and the activation NONE or SWIGLU_BWD.  There is no MASKED split-K
  at 256 rows (plan_route), so reduce MT 8 never sees a masked launch.

The fractional grid (exact_ints.grid_operands): ternary A, ternary W times a power of two, bias and residual on multiples
of 1/8 - fp32 accumulation is still exact in any order, so the pre-activation is known exactly, and at least 90 % of it
lies in |x| <= 4 (``assert_grid_case``), where the three activations differ from their asymptotes and from each other.
"""
import pytest
import torch

import exact_ints as E
import test_gpu_exact_contractions as G

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
P_DROP = G.P_DROP

# (route, M, N, K, K2, choice, plan with the workspace, plan without, how): one row per compiled instantiation, the smallest
# row of G.PLAIN / G.SPLIT_K that enters it (plans as G.PLAIN states them; 0 when K + K2 < 4096)
GRID = [
    ("generic", 37, 100, 72, 0, 0, 0, 0, ""),
    ("ping-pong 256x128", 300, 128, 192, 0, 2, 0, 0, ""),
    ("ping-pong 256x256", 2048, 4096, 192, 64, 1, 0, 0, ""),
    ("ping-pong 256x128 narrow", 512, 256, 128, 0, 2, 0, 0, "c+4"),
    ("ping-pong 256x256 narrow", 2048, 4096, 64, 0, 1, 0, 0, "c+4"),
    ("four-wave NT=8", 2048, 4096, 4096, 0, 1, 256001, 256001, ""),
    ("four-wave NT=4 + K2", 600, 256, 4096, 64, 2, 256001, 256001, ""),
    ("four-wave 192-row tiles", 5861, 4096, 4096, 0, 1, 192001, 192001, ""),
    ("four-wave 192-row tiles + 192x128 halves", 4500, 4096, 4096, 0, 1, 192101, 192101, ""),
    ("split-K 256-row x4", 5015, 4096, 4096, 0, 1, 256204, 192001, ""),
    ("split-K 192-row x3", 2573, 6144, 4096, 0, 1, 192203, 192101, ""),
    ("split-K 256-row x2 + K2", 5861, 4096, 14336, 64, 1, 256202, 192001, ""),           # the longest K: grid scale 1/64
]
# residual-only layouts: (route, M, N, K, K2, choice, plan with the workspace, plan without)
RES_LAYOUTS = [
    ("generic", 37, 100, 72, 0, 0, 0, 0),
    ("ping-pong 256x128", 300, 128, 192, 0, 2, 0, 0),
    ("four-wave NT=8", 2048, 4096, 4096, 0, 1, 256001, 256001),
    ("four-wave NT=4", 600, 256, 4096, 0, 2, 256001, 256001),
    ("four-wave 192-row tiles", 5861, 4096, 4096, 0, 1, 192001, 192001),
    ("split-K 256-row x4", 5015, 4096, 4096, 0, 1, 256204, 192001),
    ("split-K 192-row x3", 2573, 6144, 4096, 0, 1, 192203, 192101),
]
# gate/up + SwiGLU on the grid: G.SWIGLU and the instantiations it does not enter; (route, M, ff, K, K2, choice of
# [M, 2ff, K, K2], plan with the workspace, plan without)
SWIGLU_GRID = [(*c, c[6]) for c in G.SWIGLU[:3]] + [
    ("four-wave + split-K tail", 5015, 2048, 4096, 64, 1, 256204, 192001),
    ("ping-pong 256x256", 2048, 2048, 64, 64, 1, 0, 0),
    ("four-wave 192-row tiles + 192x128 halves", 4500, 2048, 4096, 64, 1, 192101, 192101),
    ("split-K 192-row x3", 2573, 3072, 4096, 64, 1, 192203, 192101),
]
# masked pair whose partial last wave is re-cut into 256x128 halves at 256 rows (MASKED, NT = 4, MT = 8): 65 x 6 = 390 tiles =
# a full round + 134; (M, N, K, plan with the workspace under the masked-pair rules, plan without)
MASKED_HALVES = [(16640, 1536, 4032, 256101, 256101)]
MASKED_SWIGLU_BWD_GRID = [(700, 512, 256, 0, 0), (2573, 6144, 4096, 192203, 192101), (16640, 1536, 4032, 256101, 256101)]

# every (K, K2) contracted on the fractional grid / on integers by this file (tests/test_cpu_exact_ints.py proves the grid
# conditions and the 256 cap for each)
GRID_K_K2 = sorted({(c[3], c[4]) for c in GRID} | {(c[3], c[4]) for c in SWIGLU_GRID})
INT_K_K2 = sorted({(c[3], c[4]) for c in RES_LAYOUTS} | {(c[2], 128) for c in MASKED_HALVES} | {(c[2], 128) for c in MASKED_SWIGLU_BWD_GRID})

ACT_NAMES = ("quick_gelu", "gelu", "silu")
PRESENCES = ((False, False), (False, True), (True, False), (True, True))          # (bias, residual)


def _act_code(name):
    from phantom_vlb_amd import ops
    return {"quick_gelu": ops.ACT_QUICK_GELU, "gelu": ops.ACT_GELU, "silu": ops.ACT_SILU}[name]


def _splits(M, N, Ktot):
    return (True, False) if G._passes_ws(M, N, Ktot) else (True,)


# ------------------------------------------------------------------ EPI_RESIDUAL: residual layouts
@pytest.mark.parametrize("route,M,N,K,K2,choice,plan_ws,plan_nows", RES_LAYOUTS, ids=G._ids(RES_LAYOUTS))
def test_gemm_residual_only_layouts(dev, route, M, N, K, K2, choice, plan_ws, plan_nows):
    """No bias, no activation, a residual: bit-equal with the residual aliasing C and with the residual a column view
    whose row stride is N + 64 (a read from row m of an [M, N] image, or at n + 16 of the neighbouring row, moves an
    output by an integer)."""
    from phantom_vlb_amd import ops
    G._assert_route(M, N, K, K2, choice, plan_ws, plan_nows)
    a, w, a2, w2, bias, res, pre = G._plain_operands(M, N, K, K2, dev)
    exact = pre.double() - bias.double()[None, :] + res.double()
    wide = torch.full((M, N + 64), 9.0, dtype=BF, device=dev)
    view = wide[:, 32:32 + N]
    view.copy_(res)
    assert view.stride(0) == N + 64 and view.data_ptr() % 16 == 0
    for split in _splits(M, N, K + K2):
        with G._SplitK(split):
            out = res.clone()
            E.assert_bits_equal(ops.gemm(a, w, residual=out, a2=a2, w2=w2, out=out), exact)
            out = torch.full((M, N), 7.0, dtype=BF, device=dev)
            E.assert_bits_equal(ops.gemm(a, w, residual=view, a2=a2, w2=w2, out=out), exact)
    assert torch.equal(view, res) and bool((wide[:, :32] == 9.0).all()) and bool((wide[:, 32 + N:] == 9.0).all())


# ------------------------------------------------------------------ activations on the fractional grid
def _grid_case(M, N, K, K2, dev):
    s = G._seed(M, N, K, K2)
    on_dev = G._on_device(M, N, K + K2)
    a, w, a2, w2, bias, res = (t if t is None else t.to(dev) for t in E.grid_operands(M, N, K, K2, s, dev if on_dev else None))
    if on_dev:
        pre = E.device_pre(a, w, a2, w2, bias)
        E.confirm_rows(pre, a, w, a2, w2, bias, seed=s)
    else:
        pre = E.exact_pre(a, w, a2, w2, bias).to(dev)
    return a, w, a2, w2, bias, res, pre.double()


@pytest.mark.parametrize("route,M,N,K,K2,choice,plan_ws,plan_nows,how", GRID, ids=G._ids(GRID))
def test_gemm_grid_activations(dev, route, M, N, K, K2, choice, plan_ws, plan_nows, how):
    """QUICK_GELU, GELU (erf) and SILU with every (bias, residual) presence: act(exact pre-activation) + residual in fp64,
    within the ulp bar at the exact pre-activation."""
    from phantom_vlb_amd import ops
    G._assert_route(M, N, K, K2, choice, plan_ws, plan_nows if plan_ws else None)
    a, w, a2, w2, bias, res, pre = _grid_case(M, N, K, K2, dev)
    xs = {True: pre, False: pre - bias.double()[None, :]}                       # with / without the bias; both exact
    for x in xs.values():
        E.assert_grid_case(x)
    res64 = res.double()
    off = {"c+4": 4}.get(how, 0)
    for split in _splits(M, N, K + K2):
        with G._SplitK(split):
            for name in ACT_NAMES:
                acted = {wb: E.ACTS[name](x) for wb, x in xs.items()}
                for with_bias, with_res in PRESENCES:
                    out, buf = G._offset_out(M, N, off, dev)
                    assert out.data_ptr() % 16 == (2 * off) % 16
                    got = ops.gemm(a, w, bias=bias if with_bias else None, residual=res if with_res else None, act=_act_code(name),
                                   a2=a2, w2=w2, out=out)
                    try:
                        E.assert_within_ulp(got, acted[with_bias] + res64 if with_res else acted[with_bias], xs[with_bias])
                    except AssertionError as e:
                        raise AssertionError(f"{name}, bias {with_bias}, residual {with_res}, split_k_tails {split}: {e}") from None
                    G._assert_guards(buf, M, N, off)


# ------------------------------------------------------------------ SWIGLU_PAIR on the grid
@pytest.mark.parametrize("gu_off", [0, 4])
@pytest.mark.parametrize("route,M,ff,K,K2,choice,plan_ws,plan_nows", SWIGLU_GRID, ids=G._ids(SWIGLU_GRID))
def test_gemm_swiglu_grid(dev, route, M, ff, K, K2, choice, plan_ws, plan_nows, gu_off):
    """[gate | up] bit-equal (multiples of the grid scale, at most 256 of them: bf16 holds them), h within the ulp bar of
    silu(gate) * up with the activation's error multiplied by |up|."""
    from phantom_vlb_amd import ops
    N = 2 * ff
    G._assert_route(M, N, K, K2, choice, plan_ws, plan_nows if plan_ws else None)
    s = G._seed(M, ff, K, K2, 7)
    gdev = dev if G._on_device(M, N, K + K2) else None
    sc = E.grid_scale(K, K2)
    a, t = E.ternary((M, K), s, gdev).to(dev), E.ternary((M, K2), s + 1, gdev).to(dev)
    wg, wu, bg, bu = ((E.ternary(shape, s + 2 + i, gdev).float() * sc).to(BF).to(dev) for i, shape in enumerate(((ff, K), (ff, K), (ff, K2), (ff, K2))))
    w_cat, b_cat = torch.cat([wg, wu], 0), torch.cat([bg, bu], 0)
    if gdev is not None:
        pre = E.device_pre(a, w_cat, t, b_cat)
        E.confirm_rows(pre, a, w_cat, t, b_cat, seed=s)
    else:
        pre = E.exact_pre(a, w_cat, t, b_cat).to(dev)
    assert E.cap_fraction(pre / sc) <= E.CAP_FRACTION
    g64, u64 = pre[:, :ff].double(), pre[:, ff:].double()
    E.assert_grid_case(g64)
    h_ref, gain = E.ACTS["silu"](g64) * u64, u64.abs().clamp_min(1.0)
    w_il, b_il = ops.interleave_gate_up(wg, wu), ops.interleave_gate_up(bg, bu)
    for split in _splits(M, N, K + K2):
        with G._SplitK(split):
            h = torch.full((M, ff), 7.0, dtype=BF, device=dev)
            gu, buf = G._offset_out(M, N, gu_off, dev)
            G._swiglu_save(a, w_il, t, b_il, h, gu, ops._gemm_workspace(dev) if G._passes_ws(M, N, K + K2) else None)
            E.assert_bits_equal(gu, pre, cap=False)                          # the cap is the one on pre / scale, above
            G._assert_guards(buf, M, N, gu_off)
            E.assert_within_ulp(h, h_ref, g64, gain)
            if gu_off == 0:
                h2 = torch.full((M, ff), 7.0, dtype=BF, device=dev)
                E.assert_within_ulp(ops.gemm(a, w_il, act=ops.ACT_SWIGLU_PAIR, a2=t, w2=b_il, out=h2), h_ref, g64, gain)


# ------------------------------------------------------------------ masked pair: the 256-row re-cut halves, SwiGLU backward on the grid
@pytest.mark.parametrize("M,N,K,plan_ws,plan_nows", MASKED_HALVES, ids=G._ids(MASKED_HALVES))
def test_gemm_masked_pair_recut_halves(dev, M, N, K, plan_ws, plan_nows):
    """The MASKED NT = 4, MT = 8 instantiation, which no row of G.MASKED enters: bit-equal like them."""
    G.test_gemm_masked_pair_bit_exact(dev, M, N, K, plan_ws, plan_nows)


@pytest.mark.parametrize("M,ff,K,plan_ws,plan_nows", MASKED_SWIGLU_BWD_GRID, ids=G._ids(MASKED_SWIGLU_BWD_GRID))
def test_gemm_masked_pair_swiglu_bwd_grid(dev, M, ff, K, plan_ws, plan_nows):
    """[d gate | d up] from the exact integer d_h at saved [gate | up] on multiples of 1/8 in [-4, 4], where sigmoid and its
    derivative bend; the bar's activation term carries the gains ulp_bar derives for this epilogue."""
    from phantom_vlb_amd import ops
    from phantom_vlb_amd._lib import lib
    assert ops.gemm_masked_pair_ok(M, ff, K)
    assert lib.vlb_gemm_plan(M, ff, K, 64, 3) == plan_ws and lib.vlb_gemm_plan(M, ff, K, 64, 2) == plan_nows
    a, w, u, at, mseed, dh = G._masked_operands(M, ff, K, dev, G._seed(M, ff, K, 1))
    gu = E.grid_gate_up(M, 2 * ff, G._seed(M, ff, K, 2), dev)
    dh = dh.double()
    g, up = gu[:, :ff].double(), gu[:, ff:].double()
    sg = torch.sigmoid(g)
    ref = torch.cat([dh * up * sg * (1 + g * (1 - sg)), dh * g * sg], 1)
    x = torch.cat([dh, dh], 1)
    gain = torch.cat([(1 + g.abs()) * up.abs().clamp_min(1.0), 1 + g.abs()], 1)
    for split in _splits(M, ff, K + 64):
        with G._SplitK(split):
            out = torch.full((M, 2 * ff), 7.0, dtype=BF, device=dev)
            E.assert_within_ulp(ops.gemm_masked_pair_swiglu_bwd(a, w, gu, u, at, P_DROP, mseed, out=out), ref, x, gain)

