"""Test-only helper: integer-valued operands for tolerance-free checks of the MFMA contractions (gemm.hip, gemm_fp8.hip,
lora.hip).

With operands drawn from {-1, 0, +1} every product and every partial sum is an integer far below 2^24, so fp32
accumulation is exact in ANY order - MFMA, split-K through the workspace, re-cut halves, fixed-order slab sums - and
(nearly) every output is an integer of magnitude < 256, i.e. exactly representable in bf16.  A correct kernel therefore
equals the reference bit for bit on every route, and one missing, repeated or misplaced product moves an output by >= 1.

  * generators: ``ternary`` / ``small_ints`` (seeded; CPU or device), ``keep_mask`` (the kernels' counter-based dropout
    mask restated in numpy) and ``keep_mask_device`` (the same hash in torch int64, for the large shapes)
  * ``exact_ref``: act(A.W^T + A2.W2^T [* keep * pair_scale] + bias) + residual in fp64
  * ``device_pre`` + ``confirm_rows``: the same pre-activation from torch's fp32 matmul on the device (exact for the same
    reason), confirmed against CPU fp64 on ``row_subsample``
  * ``assert_bits_equal`` (with the 256 cap) and ``assert_within_ulp`` (non-linear epilogues only)
  * the fractional grid (``grid_scale`` / ``grid_operands`` / ``grid_gate_up`` / ``assert_grid_case``): ternary A, ternary
    W times a power of two, bias and residual on multiples of 1/8 - still exact in fp32 in any order, but with the
    pre-activations where the activations bend (|x| <= 4) instead of in saturation
"""
from __future__ import annotations

import numpy as np
import torch

BF16 = torch.bfloat16
CAP = 256.0            # |exact| <= 256 is an integer bf16 holds exactly; above it bf16 rounding could hide a +-1 error
CAP_FRACTION = 0.01    # a case with more than this share of entries above CAP is refused


# ------------------------------------------------------------------ the kernels' dropout mask (phantom_vlb_amd/csrc/lora.hip)
def _lowbias32(x):
    x = x.astype(np.uint64)
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7feb352d)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846ca68b)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(16)
    return x


def keep_mask_rows(seed, rows, K, p):
    """keep bits of the given rows (any integer sequence) of an [*, K] mask: numpy bool [len(rows), K]."""
    thresh = min(65535, int(p * 65536 + 0.5))
    m = np.asarray(rows, dtype=np.uint64)[:, None]
    kp = np.arange(K // 2, dtype=np.uint64)[None, :]
    c = m * np.uint64(K // 2) + kp
    h = _lowbias32((c & np.uint64(0xffffffff)) ^ _lowbias32(((c >> np.uint64(32)) + np.uint64(seed)) & np.uint64(0xffffffff)))
    keep = np.empty((m.shape[0], K), dtype=bool)
    keep[:, 0::2] = (h & np.uint64(0xffff)) >= thresh
    keep[:, 1::2] = (h >> np.uint64(16)) >= thresh
    return keep


def keep_mask(seed, M, K, p):
    return torch.from_numpy(keep_mask_rows(seed, np.arange(M), K, p))


def _lowbias32_t(x):
    """lowbias32 on non-negative int64 tensors < 2^32 (int64 products wrap; their low 32 bits are still right)."""
    m = 0xffffffff
    x = x ^ (x >> 16); x = (x * 0x7feb352d) & m
    x = x ^ (x >> 15); x = (x * 0x846ca68b) & m
    return x ^ (x >> 16)


def keep_mask_device(seed, M, K, p, device):
    """keep_mask in torch integer arithmetic on ``device`` (bool [M, K]); confirm_rows checks it against the numpy one."""
    thresh = min(65535, int(p * 65536 + 0.5))
    c = torch.arange(M, dtype=torch.int64, device=device)[:, None] * (K // 2) + torch.arange(K // 2, dtype=torch.int64, device=device)[None, :]
    key = _lowbias32_t(((c >> 32) + int(seed)) & 0xffffffff)
    h = _lowbias32_t((c & 0xffffffff) ^ key)
    return torch.stack([(h & 0xffff) >= thresh, (h >> 16) >= thresh], dim=2).reshape(M, K)


# ------------------------------------------------------------------ generators
def _gen(seed, device):
    g = torch.Generator(device=device if device is not None else "cpu")
    g.manual_seed(int(seed))
    return g


def small_ints(shape, lo, hi, seed, device=None, dtype=BF16):
    """Uniform integers in [lo, hi] (inclusive) as ``dtype``; generated where they are used (``device``)."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    return torch.randint(lo, hi + 1, shape, generator=_gen(seed, device), device=device).to(dtype)


def ternary(shape, seed, device=None, dtype=BF16):
    """Uniform over {-1, 0, +1}."""
    return small_ints(shape, -1, 1, seed, device, dtype)


def bias_ints(N, seed, device=None):
    return small_ints(N, -4, 4, seed, device)


def residual_ints(M, N, seed, device=None):
    return small_ints((M, N), -4, 4, seed, device)


def gate_up_ints(M, ff2, seed, device=None):
    """Saved [gate | up] pre-activations in [-3, 3]."""
    return small_ints((M, ff2), -3, 3, seed, device)


# ------------------------------------------------------------------ the fractional grid
GRID_SD = 1.4          # target standard deviation of a grid pre-activation (before the bias)
GRID_X = 4.0           # the range in which quick_gelu / gelu / silu differ from their asymptotes and from each other
GRID_SHARE = 0.90      # a grid case with a smaller share of its pre-activations in |x| <= GRID_X is refused


def grid_scale(K, K2=0):
    """The largest power of two s with s * sqrt(4 (K + K2) / 9) <= GRID_SD: a sum of K + K2 products of two ternary
    operands has variance 4 (K + K2) / 9, so s times it has a standard deviation in (GRID_SD / 2, GRID_SD]."""
    sd = (4.0 * (K + K2) / 9.0) ** 0.5
    s = 1.0
    while s * sd > GRID_SD:
        s /= 2
    while 2 * s * sd <= GRID_SD:
        s *= 2
    return s


def eighths(shape, lo, hi, seed, device=None):
    """Uniform multiples of 1/8 in [lo, hi] (bf16 holds them exactly up to 16)."""
    return (small_ints(shape, int(8 * lo), int(8 * hi), seed, device, dtype=torch.float32) / 8).to(BF16)


def grid_operands(M, N, K, K2, seed, device=None):
    """(a, w, a2, w2, bias, residual) for act(A.W^T + A2.W2^T + bias) + residual on a fractional grid: A / A2 ternary,
    W / W2 ternary times ``grid_scale(K, K2)``, bias multiples of 1/8 in [-1, 1], residual multiples of 1/8 in [-4, 4].
    Every product and partial sum is a multiple of s below (K + K2) s, far below 2^24 s: fp32 accumulation is exact in
    any order (split-K included), adding the bias (a multiple of min(s, 1/8)) is exact too, and the pre-activation is
    known exactly.  a2 / w2 are None when K2 == 0.  Seeds: seed .. seed + 5, as the integer cases draw them."""
    s = grid_scale(K, K2)
    a, w = ternary((M, K), seed, device), (ternary((N, K), seed + 1, device).float() * s).to(BF16)
    a2 = w2 = None
    if K2:
        a2, w2 = ternary((M, K2), seed + 2, device), (ternary((N, K2), seed + 3, device).float() * s).to(BF16)
    return a, w, a2, w2, eighths(N, -1, 1, seed + 4, device), eighths((M, N), -4, 4, seed + 5, device)


def grid_gate_up(M, ff2, seed, device=None):
    """Saved [gate | up] pre-activations on multiples of 1/8 in [-4, 4]."""
    return eighths((M, ff2), -4, 4, seed, device)


def grid_share(x):
    """Share of pre-activations with |x| <= GRID_X."""
    return float((x.abs() <= GRID_X).double().mean())


def assert_grid_case(x):
    """Refuses a grid case whose pre-activations ``x`` do not sample the activation where it bends: a condition on the
    inputs (like the 256 cap of ``assert_bits_equal``), never on what a kernel returned."""
    share = grid_share(x)
    assert share >= GRID_SHARE, f"case refused: only {100 * share:.1f} % of the pre-activations lie in |x| <= {GRID_X:.0f}"


# ------------------------------------------------------------------ references
ACTS = {
    None: lambda x: x,
    "none": lambda x: x,
    "quick_gelu": lambda x: x * torch.sigmoid(1.702 * x),
    "gelu": lambda x: 0.5 * x * (1 + torch.erf(x * 2.0 ** -0.5)),
    "silu": lambda x: x * torch.sigmoid(x),
}


def _d(t):
    return None if t is None else t.detach().double().cpu()


def exact_pre(a, w, a2=None, w2=None, bias=None, keep=None, pair_scale=1.0):
    """x = A.W^T + pair_scale * keep o (A2.W2^T) + bias in fp64 on the CPU (``keep``: bool [M, N] or None)."""
    x = _d(a) @ _d(w).t()
    if a2 is not None:
        pair = _d(a2) @ _d(w2).t()
        if keep is not None:
            pair = pair * torch.as_tensor(keep).double().cpu()
        x = x + pair_scale * pair
    if bias is not None:
        x = x + _d(bias)[None, :]
    return x


def exact_ref(a, w, a2=None, w2=None, bias=None, residual=None, act=None, keep=None, pair_scale=1.0):
    """act(A.W^T + A2.W2^T + bias) + residual in fp64; with ``keep`` the masked-pair form A.W^T + pair_scale * keep o (A2.W2^T)."""
    y = ACTS[act](exact_pre(a, w, a2, w2, bias, keep, pair_scale))
    if residual is not None:
        y = y + _d(residual)
    return y


def device_pre(a, w, a2=None, w2=None, bias=None, keep=None, pair_scale=1.0):
    """exact_pre from torch's fp32 matmul on the operands' device: exact on integer operands (every partial sum is an
    integer below 2^24).  Returns fp32 [M, N]; ``confirm_rows`` ties it to CPU fp64."""
    x = a.float() @ w.float().t()
    if a2 is not None:
        pair = a2.float() @ w2.float().t()
        if keep is not None:
            pair = pair * keep.to(pair.device).float()
        x = x + float(pair_scale) * pair
    if bias is not None:
        x = x + bias.float()[None, :]
    return x


def row_subsample(M, seed=0, extra=32):
    """Row 0, row M-1, both sides of every 192- and 256-row tile boundary inside [0, M), and ``extra`` random rows."""
    rows = {0, M - 1}
    for t in (192, 256):
        for b in range(t, M, t):
            rows.update((b - 1, b))
    rng = np.random.RandomState(seed)
    rows.update(int(r) for r in rng.randint(0, M, size=extra))
    return sorted(r for r in rows if 0 <= r < M)


def confirm_rows(pre_dev, a, w, a2=None, w2=None, bias=None, keep_seed=None, keep_p=0.0, pair_scale=1.0, seed=0):
    """The device fp32 pre-activation equals CPU fp64 on ``row_subsample`` (only those rows of A / A2 / pre_dev come to the
    CPU).  With ``keep_seed`` the pair is masked by the numpy keep_mask of those rows."""
    M, N = pre_dev.shape
    rows = row_subsample(M, seed)
    idx = torch.as_tensor(rows, device=pre_dev.device)
    keep = None
    if keep_seed is not None:
        keep = torch.from_numpy(keep_mask_rows(keep_seed, rows, N, keep_p))
    want = exact_pre(a[idx], w, None if a2 is None else a2[idx], w2, bias, keep, pair_scale)
    got = pre_dev[idx].double().cpu()
    bad = got != want
    assert not bool(bad.any()), f"device fp32 reference differs from CPU fp64 on {int(bad.sum())} entries of {len(rows)} sampled rows"


# ------------------------------------------------------------------ checks
def cap_fraction(ref):
    """Share of reference entries with |exact| > CAP."""
    return float((ref.abs() > CAP).float().mean())


def _describe(got, want, bad, limit=6):
    nz = bad.nonzero()[:limit].tolist()
    parts = []
    for ix in nz:
        ix = tuple(ix)
        parts.append(f"{ix}: got {float(got[ix])!r} want {float(want[ix])!r}")
    msg = f"{int(bad.sum())} of {bad.numel()} entries differ; first: " + "; ".join(parts)
    if bad.dim() == 2 and nz:
        m, n = nz[0]
        tm, tn = m // 256, n // 256
        tile = bad[tm * 256:(tm + 1) * 256, tn * 256:(tn + 1) * 256]
        rows_bad = tile.any(1).nonzero().flatten()
        cols_bad = tile.any(0).nonzero().flatten()
        msg += (f"; 256x256 tile ({tm}, {tn}) = rows {tm * 256}.., cols {tn * 256}..: {int(tile.sum())} bad entries, "
                f"tile rows {int(rows_bad[0])}..{int(rows_bad[-1])}, tile cols {int(cols_bad[0])}..{int(cols_bad[-1])}; "
                f"tiles with a bad entry: {int(_bad_tiles(bad))}")
    return msg


def _bad_tiles(bad):
    M, N = bad.shape
    tm, tn = (M + 255) // 256, (N + 255) // 256
    pad = torch.zeros(tm * 256, tn * 256, dtype=torch.bool, device=bad.device)
    pad[:M, :N] = bad
    return pad.view(tm, 256, tn, 256).any(3).any(1).sum()


def assert_bits_equal(got, ref64, cap=True):
    """``got`` (bf16) must equal ``ref64.float().to(bf16)``, an fp32 ``got`` must equal ``ref64.float()`` - torch.equal, no
    tolerance.  ``ref64`` is the exact value (fp64 on the CPU, or the exact fp32 device reference).  The case itself is
    refused when more than CAP_FRACTION of the reference lies above CAP (bf16 outputs; ``cap=False`` only where the
    rounding of the exact value is itself what is checked), or when an fp32 output would leave the exact-integer range."""
    assert tuple(got.shape) == tuple(ref64.shape), (tuple(got.shape), tuple(ref64.shape))
    assert got.dtype in (BF16, torch.float32), got.dtype
    ref64 = ref64.to(got.device)
    assert bool(torch.isfinite(ref64).all())
    if got.dtype == BF16:
        if cap:
            frac = cap_fraction(ref64)
            assert frac <= CAP_FRACTION, f"case refused: {100 * frac:.2f} % of the reference entries exceed {CAP:.0f}"
        want = ref64.float().to(BF16)
    else:
        assert float(ref64.abs().max()) < 2.0 ** 24, "case refused: fp32 reference outside the exact-integer range"
        want = ref64.float()
    if torch.equal(got, want):
        return
    bad = (got != want) | torch.isnan(got)
    raise AssertionError("not bit-equal: " + _describe(got, want, bad))


def ulp_bar(ref64, x, gain=1.0):
    """|got - ref| <= 2^-8 |ref| + 2^-20 (1 + |x|) gain: one bf16 rounding (half an ulp is at most 2^-8 |ref|, including the
    flip to the neighbour when the fp32 value sits next to a tie) plus the fp32 evaluation of exp / erf at pre-activation x.

    The second term is an ABSOLUTE bound on the error of act(x): with u = 2^-24 the kernels' sigmoid (``__expf`` then
    ``__builtin_amdgcn_rcpf``: an ulp each, a rounding of 1 + e, and |x| u from rounding the exponent's argument) is within
    (3 + |x|) u relative, so x * sigmoid(x) is within |x| (3 + |x|) u <= 16 (1 + |x|) u = 2^-20 (1 + |x|) for |x| <= 14
    (quick_gelu's argument 1.702 x: |x| (3.5 + 1.702 |x|) u, for |x| <= 8; erf GELU: 0.5 x (1 + erff) with erff and the
    roundings a few u absolute, |x| times a few u).

    ``gain`` (default 1: nothing changes) is for epilogues that MULTIPLY the activation by something after evaluating it; it
    is what the absolute error of the activation is multiplied by, derived from the epilogue's formula and never from
    kernel output:
      * SwiGLU h = silu(g) * up, x = g:  gain = max(1, |up|).
      * SwiGLU backward, x = d_h:  d up = d_h * (g s) and d gate = d_h * up * F, F = s (1 + g (1 - s)), s = sigmoid(g).  With
        delta_s <= s (3 + |g|) u:  delta(g s) <= (|g| (3 + |g|) + 2) u and delta_F <= ((3 + |g|) (1.1 + |g|) + 2) u (the error
        of s enters 1 - s absolutely and is multiplied by g); both are <= 16 (1 + |g|) u for |g| <= 12.  So gain =
        1 + |g| for d up and (1 + |g|) max(1, |up|) for d gate."""
    return 2.0 ** -8 * ref64.abs() + 2.0 ** -20 * (1 + x.abs()) * gain


def assert_within_ulp(got, ref64, x, gain=1.0):
    """For the non-linear epilogues: ``x`` is the exact pre-activation, ``ref64`` the fp64 value of the epilogue on it; only
    the activation is inexact.  Element-wise, derived bar (``ulp_bar``; ``gain``: see there)."""
    assert tuple(got.shape) == tuple(ref64.shape) == tuple(x.shape), (tuple(got.shape), tuple(ref64.shape), tuple(x.shape))
    dev = got.device
    ref64, x = ref64.to(dev).double(), x.to(dev).double()
    if torch.is_tensor(gain):
        gain = gain.to(dev).double()
    g = got.double()
    err = (g - ref64).abs()
    bar = ulp_bar(ref64, x, gain)
    bad = ~(err <= bar)                      # NaN fails
    if not bool(bad.any()):
        return
    worst = float((err / bar)[~torch.isnan(err)].max()) if bool((~torch.isnan(err)).any()) else float("nan")
    raise AssertionError(f"outside the ulp bar (worst |got-ref|/bar = {worst:.3f}): " + _describe(g, ref64, bad))
