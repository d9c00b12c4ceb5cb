"""Attention forward / backward (phantom_vlb_amd/csrc/attention.hip) against references that round where the kernels
round (tests/attn_emul.py), at bars derived from that rounding, on the inputs and shapes where attention kernels go
wrong.

Backward bar.  Kernel and emulator build the same bf16 operands from the same bf16 inputs, the device's own ``out`` and
``lse``: bf16(P) for dV, bf16(P.(dP - delta).scale) for dK and dQ, bf16 per-head partials for a GQA dK / dV.  What is
left between them is (a) fp32 summation order, (b) the final bf16 rounding of each output, which may go either way,
and (c) an occasional P, dS or partial whose fp32 value (computed in another order) lies on the other side of a bf16
rounding boundary.  A bf16 ulp is at most 2^-7 of the value it belongs to.  So, per output element,

    |got - emu| <= 2^-7 * |emu|          (b: one output ulp)
                 + 2^-7 * flip           (c: one ulp of the largest single operand contribution; attn_emul's budget)
                 + 2^-12 * max|emu|      (a: fp32 order floor, 2^-24 * sqrt(S) * sum|terms| with room to spare)
                 + noise                 (a, where dP ~ delta: the fp32 error of dP - delta, carried through dS)

and over a tensor, where the flips of (b) and (c) are rare and of random sign, ||got - emu|| / ||emu|| <= 2e-3.  Neither
number comes from a measurement of the kernels.  The mutation check proves that the bar rejects the bug classes a
rebuilt backward could plausibly carry.

Forward bar.  The forward rounds P (unnormalised, fp32) to bf16 before O += P.V and normalises by the fp32 sum of the
unrounded P; each bf16(P) is within 2^-8 of P relative, so |O_kernel - O| <= 2^-8 * (P.|V|) before the output rounding
(one ulp, 2^-7 |O|), plus fp32 error in P itself (an exp argument of up to ~100 carries ~2^-16 relative).  lse is
m.scale + log(l) in fp32: <= 1e-4 * (1 + |lse|).

Regimes (inputs rounded to bf16 before either side sees them): flat (randn * 0.7, score std ~0.5), peaky (score std
~4), sink (key 0 of every clip aligned with the mean query: most rows put >= 0.9 of their mass on it), outlier (three
of the 128 channels of q and k at 20x) and cancelling (sink scores with dO = 3 O + noise, so delta ~ dP on the dominant
key and dS = P (dP - delta) cancels).
"""
import pytest
import torch

from attn_emul import MUTATIONS, attn_bwd_emul, attn_fwd_ref

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
D = 128
REGIMES = ("flat", "peaky", "sink", "outlier", "cancel")
S_EDGES = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 300)      # 32-query, 64-key and 128-key tile boundaries


def _layout(B, S, lens):
    """-> (cu host list or None, [(row0, n)] per clip, rows)"""
    if lens is None:
        return None, [(b * S, S) for b in range(B)], B * S
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return cu, [(cu[b], lens[b]) for b in range(len(lens))], cu[-1]


def _inputs(regime, Hq, Hkv, clips, rows, seed, Dh=D, fwd_kw=None):
    """bf16 q [rows, Hq*Dh], k / v [rows, Hkv*Dh], dout [rows, Hq*Dh] of one regime (see the module docstring)."""
    g = torch.Generator().manual_seed(seed)
    base = 2.0 if regime == "peaky" else 0.7                  # score std = base^2 at scale Dh^-0.5
    q = torch.randn(rows, Hq, Dh, generator=g) * base
    k = torch.randn(rows, Hkv, Dh, generator=g) * base
    v = torch.randn(rows, Hkv, Dh, generator=g)
    dout = torch.randn(rows, Hq, Dh, generator=g)
    if regime in ("sink", "cancel"):
        m = torch.randn(Hkv, Dh, generator=g)                  # the mean query of each GQA group
        q = q + m.repeat_interleave(Hq // Hkv, 0)
        for r0, _ in clips:
            k[r0] = 1.2 * m                                    # logit ~ 1.2 |m|^2 / sqrt(Dh) ~ 13.6 against ~1 for the rest
    if regime == "outlier":
        ch = [5, 60, 101]
        q[..., ch] *= 20.0
        k[..., ch] *= 20.0
    q, k, v, dout = (t.reshape(rows, -1).to(BF) for t in (q, k, v, dout))
    if regime == "cancel":
        out, _, _ = attn_fwd_ref(q, k, v, **fwd_kw)
        dout = (3.0 * out + 0.1 * torch.randn(rows, Hq * Dh, generator=g, dtype=out.dtype)).to(BF)
    return q, k, v, dout


def _kernels(dev, q, k, v, dout, Hq, Hkv, causal, scale, mask, B, S, lens=None, views=False):
    """forward (out, lse) then backward (dqkv) on the device; ``views``: out and dout are strided column views."""
    from phantom_vlb_amd import ops
    layout = ops.RowLayout(B, S, lens, device=dev) if lens is not None else None
    qd, kd = Hq * D, Hkv * D
    qkv = torch.cat([q, k, v], 1).to(dev)
    rows = qkv.shape[0]
    dmask = None if mask is None else mask.to(dev)
    out_arg, dout_d = None, dout.to(dev)
    if views:
        out_arg = torch.zeros(rows, qd + 2 * D, dtype=BF, device=dev)[:, D:D + qd]
        big = torch.zeros(rows, qd + 3 * D, dtype=BF, device=dev)
        big[:, 2 * D:2 * D + qd] = dout_d
        dout_d = big[:, 2 * D:2 * D + qd]
    out, lse = ops.attention_fwd(qkv[:, :qd], qkv[:, qd:qd + kd], qkv[:, qd + kd:], B, S, Hq, Hkv, D, causal, scale,
                                 key_mask=dmask, need_lse=True, out=out_arg, layout=layout)
    dqkv = ops.attention_bwd(qkv, qd, kd, out, dout_d, lse, dmask, B, S, Hq, Hkv, D, causal, scale, layout=layout)
    torch.cuda.synchronize()
    return out, lse, dqkv


def _bar(got, emu, flip, noise):
    """-> (elements over the element-wise bar, ||got - emu|| / ||emu||, worst err / tol)"""
    got = got.to(emu.dtype)
    err = (got - emu).abs()
    tol = 2.0 ** -7 * (emu.abs() + flip) + 2.0 ** -12 * emu.abs().max() + noise
    bad = int((err > tol).sum())
    en = float(emu.norm())
    nrm = float(err.norm()) / en if en > 0 else float(err.norm())
    worst = float((err / tol.clamp_min(1e-30)).max())
    return bad, nrm, worst


def _split(dqkv, Hq, Hkv):
    qd, kd = Hq * D, Hkv * D
    return dqkv[:, :qd], dqkv[:, qd:qd + kd], dqkv[:, qd + kd:]


def _failures(dqkv, emu, budget, Hq, Hkv):
    """[(tensor, bad elements, norm error, worst ratio)] of the tensors that miss the bar (empty: all within).  The
    norm-wise bar is 2e-3 of ||emu|| plus the norm of the fp32 noise budget (which only matters where emu is noise)."""
    out = []
    for name, g, e, f, z in zip(("dq", "dk", "dv"), _split(dqkv, Hq, Hkv), emu, *budget):
        g = g.to(e.device)
        bad, nrm, worst = _bar(g, e, f, z)
        en = float(e.norm())
        if not torch.isfinite(g).all() or bad or nrm > 2e-3 + (float(z.norm()) / en if en > 0 else float(z.norm())):
            out.append((name, bad, nrm, worst))
    return out


def _emulate(q, k, v, dout, out, lse, mask, Hq, Hkv, causal, scale, B, S, cu, device="cpu", dtype=torch.float64,
             mutation=None):
    emu, flip, noise = attn_bwd_emul(q, k, v, dout, out.to(device), lse.to(device), Hq=Hq, Hkv=Hkv, causal=causal,
                                     scale=scale, key_mask=mask, B=B, S=S, cu=cu, device=device, dtype=dtype, budget=True,
                                     mutation=mutation)
    return emu, (flip, noise)


def _case(dev, regime, B, S, Hq, Hkv, causal, mask_fn=None, lens=None, scale=None, views=False, seed=0):
    """Build one case, run the kernels, check the backward against the fp64 CPU emulator; -> (out, lse, dqkv, mask)."""
    scale = D ** -0.5 if scale is None else scale
    cu, clips, rows = _layout(B, S, lens)
    mask = None
    if mask_fn is not None:
        mask = torch.ones(rows, dtype=torch.uint8)
        mask_fn(mask, clips)
    kw = dict(Hq=Hq, Hkv=Hkv, causal=causal, scale=scale, key_mask=mask, B=B, S=S if lens is None else max(lens), cu=cu)
    q, k, v, dout = _inputs(regime, Hq, Hkv, clips, rows, seed=seed or S * 31 + Hq, fwd_kw=kw)
    out, lse, dqkv = _kernels(dev, q, k, v, dout, Hq, Hkv, causal, scale, mask, B, S, lens, views)
    emu, flips = _emulate(q, k, v, dout, out.cpu(), lse.cpu(), mask, Hq, Hkv, causal, scale, kw["B"], kw["S"], cu)
    fails = _failures(dqkv.cpu(), emu, flips, Hq, Hkv)
    assert not fails, (regime, B, S, Hq, Hkv, causal, lens, scale, fails)
    return out, lse, dqkv, mask


def _mask_tail_and_interior(mask, clips):
    """clip 1 (or the only clip): padded tail of n/4 keys and one interior key masked"""
    r0, n = clips[min(1, len(clips) - 1)]
    mask[r0 + n - n // 4:r0 + n] = 0
    if n >= 3:
        mask[r0 + n // 2] = 0


# ------------------------------------------------------------------ backward: tile edges
@pytest.mark.parametrize("S", S_EDGES)
@pytest.mark.parametrize("causal,masked", [(True, False), (True, True), (False, False), (False, True)])
def test_attention_bwd_tile_edges(dev, S, causal, masked):
    _case(dev, "flat", 2, S, 8, 2, causal, _mask_tail_and_interior if masked else None)


# ------------------------------------------------------------------ backward: head counts x regimes
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("Hq,Hkv", [(8, 8), (16, 8), (32, 8), (8, 1), (16, 2), (32, 16)])
def test_attention_bwd_heads_regimes(dev, regime, Hq, Hkv):
    """group sizes 1 / 2 / 4 / 8 with Hq in {8, 16, 32} (xcd_head permutes heads at Hq = 16 and 32), causal, clip 1
    masked"""
    _case(dev, regime, 2, 129, Hq, Hkv, True, _mask_tail_and_interior)


@pytest.mark.parametrize("regime", REGIMES)
def test_attention_bwd_regimes_noncausal(dev, regime):
    _case(dev, regime, 2, 200, 32, 8, False, _mask_tail_and_interior)


# ------------------------------------------------------------------ backward: edges
def test_attention_bwd_causal_leading_rows_dead(dev):
    """causal clip 1 with keys 0..2 masked: its rows 0..2 see no key (lse = -inf, out = 0, dq = 0)"""
    def m(mask, clips):
        mask[clips[1][0]:clips[1][0] + 3] = 0
    out, lse, dqkv, _ = _case(dev, "flat", 2, 100, 8, 2, True, m)
    assert torch.isinf(lse[1, :, :3]).all() and (lse[1, :, :3] < 0).all()
    assert torch.isfinite(lse[1, :, 3:100]).all() and torch.isfinite(lse[0]).all()
    assert (out[100:103] == 0).all() and (dqkv[100:103, :8 * D] == 0).all()


def test_attention_bwd_noncausal_clip_all_masked(dev):
    """non-causal clip 1 with every key masked: zeros everywhere in it, finite, lse = -inf"""
    def m(mask, clips):
        mask[clips[1][0]:clips[1][0] + clips[1][1]] = 0
    out, lse, dqkv, _ = _case(dev, "peaky", 2, 150, 8, 2, False, m)
    assert torch.isfinite(dqkv).all() and (dqkv[150:] == 0).all() and (out[150:] == 0).all()
    assert torch.isinf(lse[1]).all() and (lse[1] < 0).all() and torch.isfinite(lse[0]).all()
    assert dqkv[:150].abs().max() > 0


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("regime", ["flat", "peaky"])
def test_attention_bwd_scale(dev, causal, regime):
    """scale = 0.05 (not D^-0.5): the kernels apply it to S and, before the bf16 rounding, to dS"""
    _case(dev, regime, 2, 160, 16, 4, causal, _mask_tail_and_interior, scale=0.05)


@pytest.mark.parametrize("causal", [True, False])
def test_attention_bwd_strided_views(dev, causal):
    """out and dout as column views of wider buffers (row stride != Hq*D)"""
    _case(dev, "sink", 2, 140, 8, 2, causal, _mask_tail_and_interior, views=True)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("regime", ["flat", "sink"])
def test_attention_bwd_packed(dev, causal, regime):
    """packed rows (cu) against the emulator directly, with an interior masked key in clip 1"""
    _case(dev, regime, 3, 256, 16, 4, causal, _mask_tail_and_interior, lens=[200, 61, 130])


# ------------------------------------------------------------------ backward: full size, fp32 emulator on the device
@pytest.mark.parametrize("case", ["7b_clip_padded_sink", "bench_batch_packed"])
def test_attention_bwd_full_size(dev, case):
    """32 / 8 heads at S = 2048: one clip with 150 padded keys in the sink regime, and the benchmark's batch (B = 3,
    S = 2048, clip lengths summing to 5861 packed rows)"""
    Hq, Hkv, scale = 32, 8, D ** -0.5
    B, S, lens, regime = (1, 2048, None, "sink") if case.startswith("7b") else (3, 2048, [2048, 1900, 1913], "flat")
    cu, clips, rows = _layout(B, S, lens)
    mask = None
    if lens is None:
        mask = torch.ones(rows, dtype=torch.uint8)
        mask[S - 150:] = 0
    q, k, v, dout = _inputs(regime, Hq, Hkv, clips, rows, seed=7)
    out, lse, dqkv = _kernels(dev, q, k, v, dout, Hq, Hkv, True, scale, mask, B, S, lens)
    if regime == "sink":        # the regime really is one: most valid rows put >= 0.9 of their mass on key 0
        s0 = (q.view(rows, Hq, D).float() * k.view(rows, Hkv, D)[0].float().repeat_interleave(Hq // Hkv, 0)).sum(-1)
        p0 = torch.exp(s0[:S - 150] * scale - lse[0, :, :S - 150].t().cpu())
        assert float((p0 >= 0.9).float().mean()) > 0.5
    prev = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        emu, flips = _emulate(q, k, v, dout, out, lse, mask, Hq, Hkv, True, scale, B, max(lens) if lens else S, cu,
                              device=dev, dtype=torch.float32)
    finally:
        torch.backends.cuda.matmul.allow_tf32 = prev
    fails = _failures(dqkv, emu, flips, Hq, Hkv)
    assert not fails, (case, fails)


# ------------------------------------------------------------------ the bar catches real bug classes
def test_attention_bwd_mutations_fail_the_bar(dev):
    """The real kernel output against deliberately wrong emulators: each must miss the bar (and the right one pass)."""
    B, S, Hq, Hkv, causal, scale = 1, 300, 8, 2, True, D ** -0.5
    cu, clips, rows = _layout(B, S, None)
    q, k, v, dout = _inputs("flat", Hq, Hkv, clips, rows, seed=300)
    out, lse, dqkv = _kernels(dev, q, k, v, dout, Hq, Hkv, causal, scale, None, B, S)
    out, lse, dqkv = out.cpu(), lse.cpu(), dqkv.cpu()
    emu, flips = _emulate(q, k, v, dout, out, lse, None, Hq, Hkv, causal, scale, B, S, cu)
    assert not _failures(dqkv, emu, flips, Hq, Hkv)
    caught = {}
    for mut in MUTATIONS:
        emu, flips = _emulate(q, k, v, dout, out, lse, None, Hq, Hkv, causal, scale, B, S, cu, mutation=mut)
        caught[mut] = _failures(dqkv, emu, flips, Hq, Hkv)
        print(f"mutation {mut}: " + ("FAILS the bar: " + ", ".join(f"{n} {b} elements, norm {e:.2e}"
                                                                  for n, b, e, _ in caught[mut]) if caught[mut]
                                      else "passes the bar"))
    assert all(caught.values()), {m: f for m, f in caught.items() if not f}


# ------------------------------------------------------------------ determinism
def test_attention_bwd_deterministic(dev):
    """two backward calls on the same inputs give the same bits (GQA, packed rows, masked key)"""
    from phantom_vlb_amd import ops
    Hq, Hkv, lens, B, S = 32, 8, [300, 77, 257], 3, 300
    cu, clips, rows = _layout(B, S, lens)
    q, k, v, dout = _inputs("sink", Hq, Hkv, clips, rows, seed=9)
    mask = torch.ones(rows, dtype=torch.uint8)
    mask[310] = 0
    out, lse, d1 = _kernels(dev, q, k, v, dout, Hq, Hkv, True, D ** -0.5, mask, B, S, lens)
    layout = ops.RowLayout(B, S, lens, device=dev)
    qkv = torch.cat([q, k, v], 1).to(dev)
    d2 = ops.attention_bwd(qkv, Hq * D, Hkv * D, out, dout.to(dev), lse, mask.to(dev), B, S, Hq, Hkv, D, True, D ** -0.5,
                           layout=layout)
    torch.cuda.synchronize()
    for a, b in zip(_split(d1, Hq, Hkv), _split(d2, Hq, Hkv)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ forward: regimes and tile edges
def _fwd_case(dev, regime, B, S, Hq, Hkv, causal, Dh, mask_fn=None, scale=None):
    from phantom_vlb_amd import ops
    scale = Dh ** -0.5 if scale is None else scale
    cu, clips, rows = _layout(B, S, None)
    mask = None
    if mask_fn is not None:
        mask = torch.ones(rows, dtype=torch.uint8)
        mask_fn(mask, clips)
    q, k, v, _ = _inputs(regime, Hq, Hkv, clips, rows, seed=S * 7 + Dh, Dh=Dh)
    qkv = torch.cat([q, k, v], 1).to(dev)
    qd, kd = Hq * Dh, Hkv * Dh
    out, lse = ops.attention_fwd(qkv[:, :qd], qkv[:, qd:qd + kd], qkv[:, qd + kd:], B, S, Hq, Hkv, Dh, causal, scale,
                                 key_mask=None if mask is None else mask.to(dev), need_lse=True)
    ref, lse_ref, pv = attn_fwd_ref(q, k, v, Hq=Hq, Hkv=Hkv, causal=causal, scale=scale, key_mask=mask, B=B, S=S)
    got = out.cpu().double()
    tol = (2.0 ** -8 + 2.0 ** -15) * pv + 2.0 ** -7 * ref.abs()
    bad = int(((got - ref).abs() > tol).sum())
    assert torch.isfinite(got).all() and bad == 0, (regime, S, Hq, Hkv, causal, Dh, bad)
    lse = lse.cpu().double()
    dead = torch.isinf(lse_ref)
    assert torch.equal(dead, torch.isinf(lse)) and (lse[dead] < 0).all()
    le = (lse - lse_ref).abs()[~dead]
    assert (le <= 1e-4 * (1 + lse_ref.abs()[~dead])).all(), float(le.max())


@pytest.mark.parametrize("S", S_EDGES)
@pytest.mark.parametrize("Dh", [128, 64])
def test_attention_fwd_tile_edges(dev, S, Dh):
    _fwd_case(dev, "flat", 2, S, 8, 2, True, Dh, _mask_tail_and_interior)
    _fwd_case(dev, "peaky", 2, S, 4, 4, False, Dh, _mask_tail_and_interior)


@pytest.mark.parametrize("regime", ["peaky", "sink", "outlier"])
@pytest.mark.parametrize("causal", [True, False])
def test_attention_fwd_regimes(dev, regime, causal):
    _fwd_case(dev, regime, 2, 300, 32, 8, causal, 128, _mask_tail_and_interior)


def test_attention_fwd_dead_rows(dev):
    """a causal clip whose key 0 is masked and a non-causal clip with every key masked: out = 0, lse = -inf"""
    _fwd_case(dev, "flat", 2, 70, 8, 2, True, 128, lambda m, c: m.__setitem__(c[1][0], 0))
    _fwd_case(dev, "flat", 2, 70, 8, 2, False, 128, lambda m, c: m.__setitem__(slice(c[1][0], c[1][0] + c[1][1]), 0))


# ------------------------------------------------------------------ refusals: an error, never a crash or a launch
def test_attention_refuses_bad_arguments(dev):
    from phantom_vlb_amd import ops
    from phantom_vlb_amd._lib import VlbError
    B, S, Hq, Hkv = 1, 64, 4, 2
    z = lambda *s: torch.zeros(*s, dtype=BF, device=dev)        # noqa: E731
    qkv64 = z(B * S, (Hq + 2 * Hkv) * 64)
    o64 = z(B * S, Hq * 64)
    lse = torch.zeros(B, Hq, S, dtype=torch.float32, device=dev)
    with pytest.raises(VlbError):                                # backward: D = 64 (the ViT never needs one)
        ops.attention_bwd(qkv64, Hq * 64, Hkv * 64, o64, o64, lse, None, B, S, Hq, Hkv, 64, True, 0.125)
    q96 = z(B * S, Hq * 96)
    with pytest.raises(VlbError):                                # forward: D = 96
        ops.attention_fwd(q96, z(B * S, Hkv * 96), z(B * S, Hkv * 96), B, S, Hq, Hkv, 96, True, 0.1)
    qkv = z(B * S, (4 + 2 * 3) * D)
    with pytest.raises(VlbError):                                # Hq % Hkv != 0
        ops.attention_fwd(qkv[:, :4 * D], qkv[:, 4 * D:7 * D], qkv[:, 7 * D:], B, S, 4, 3, D, True, 0.1)
    with pytest.raises(VlbError):
        ops.attention_bwd(qkv, 4 * D, 3 * D, z(B * S, 4 * D), z(B * S, 4 * D), lse, None, B, S, 4, 3, D, True, 0.1)
    wide = z(B * S, (Hq + 2 * Hkv) * D + 4)                      # row stride % 8 != 0
    qd, kd = Hq * D, Hkv * D
    with pytest.raises(VlbError):
        ops.attention_fwd(wide[:, :qd], wide[:, qd:qd + kd], wide[:, qd + kd:qd + 2 * kd], B, S, Hq, Hkv, D, True, 0.1)
    o = z(B * S, qd)
    with pytest.raises(VlbError):
        ops.attention_bwd(wide[:, :qd + 2 * kd], qd, kd, o, o, lse, None, B, S, Hq, Hkv, D, True, 0.1)
    ob = z(B * S, qd + 8)
    with pytest.raises(VlbError):                                # out / dout 2 bytes off their 16-byte alignment
        ops.attention_bwd(z(B * S, qd + 2 * kd), qd, kd, ob[:, 1:1 + qd], o, lse, None, B, S, Hq, Hkv, D, True, 0.1)
    with pytest.raises(VlbError):
        ops.attention_bwd(z(B * S, qd + 2 * kd), qd, kd, o, ob[:, 1:1 + qd], lse, None, B, S, Hq, Hkv, D, True, 0.1)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ report: how much of the error is rounding alone
def test_attention_bwd_rounding_gap_report(dev):
    """Prints (asserts nothing): per regime, the emulator's and the kernel's gap to the exact fp64 backward on the same
    bf16 inputs (max error / max, and norm-wise), for dQ, dK, dV.  The emulator's gap is what bf16 P / dS / partials
    cost by themselves; DESIGN.md section 3 records these numbers."""
    B, S, Hq, Hkv, causal, scale = 1, 384, 8, 2, True, D ** -0.5
    cu, clips, rows = _layout(B, S, None)
    kw = dict(Hq=Hq, Hkv=Hkv, causal=causal, scale=scale, B=B, S=S)
    for regime in REGIMES:
        q, k, v, dout = _inputs(regime, Hq, Hkv, clips, rows, seed=384, fwd_kw=kw)
        out, lse, dqkv = _kernels(dev, q, k, v, dout, Hq, Hkv, causal, scale, None, B, S)
        o64, l64, _ = attn_fwd_ref(q, k, v, **kw)
        exact = attn_bwd_emul(q, k, v, dout, o64, l64, rounding=False, **kw)
        emu = attn_bwd_emul(q, k, v, dout, out.cpu(), lse.cpu(), **kw)
        line = []
        for name, e, x, g in zip(("dq", "dk", "dv"), emu, exact, _split(dqkv.cpu().double(), Hq, Hkv)):
            xm, xn = float(x.abs().max()), float(x.norm())
            line.append(f"{name} emu {float((e - x).abs().max()) / xm:.2e}/{float((e - x).norm()) / xn:.2e} "
                        f"hip {float((g - x).abs().max()) / xm:.2e}/{float((g - x).norm()) / xn:.2e}")
        print(f"rounding gap vs fp64 (max/max, norm) {regime:8s}: " + "; ".join(line))
