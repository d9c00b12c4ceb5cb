"""The attention-backward emulator (tests/attn_emul.py) is itself a claim: with its rounding switched off it must be the
exact gradient of softmax attention.  Here it is checked against fp64 autograd through the softmax definition, for
grouped-query heads, causal and not, key masks, packed clips and a scale that is not D^-0.5; and with rounding on, a
row whose keys are all masked must come out as exact zeros."""
import pytest
import torch

from attn_emul import MUTATIONS, attn_bwd_emul, attn_fwd_ref

F64 = torch.float64


def _autograd(q, k, v, dout, Hq, Hkv, causal, scale, key_mask, clips):
    """dq, dk, dv of sum(out * dout) with out = softmax(q k^T scale, masked) v, per clip, by fp64 autograd.  A row with
    no valid key has output 0 (its softmax is replaced by zeros, so no NaN reaches the gradient)."""
    rows, D = q.shape[0], q.shape[1] // Hq
    rep = Hq // Hkv
    qa, ka, va = (t.detach().clone().to(F64).requires_grad_(True) for t in (q, k, v))
    loss = 0.0
    for r0, n in clips:
        Q = qa[r0:r0 + n].view(n, Hq, D).transpose(0, 1)
        K = ka[r0:r0 + n].view(n, Hkv, D).transpose(0, 1).repeat_interleave(rep, 0)
        V = va[r0:r0 + n].view(n, Hkv, D).transpose(0, 1).repeat_interleave(rep, 0)
        allow = torch.ones(n, n, dtype=torch.bool)
        if key_mask is not None:
            allow &= key_mask.reshape(-1)[r0:r0 + n].bool()[None, :]
        if causal:
            allow &= torch.ones(n, n, dtype=torch.bool).tril()
        live = allow.any(-1)
        s = (Q @ K.transpose(1, 2) * scale).masked_fill(~allow, float("-inf"))
        s = torch.where(live[:, None], s, torch.zeros((), dtype=F64))       # dead rows: finite, then zeroed below
        P = torch.softmax(s, -1) * live[:, None]
        o = (P @ V).transpose(0, 1)
        loss = loss + (o * dout[r0:r0 + n].to(F64).view(n, Hq, D)).sum()
    loss.backward()
    return qa.grad, ka.grad, va.grad


def _inputs(rows, Hq, Hkv, D, seed, peaky=False):
    g = torch.Generator().manual_seed(seed)
    s = 2.0 if peaky else 0.7
    q = (torch.randn(rows, Hq * D, generator=g, dtype=F64) * s)
    k = (torch.randn(rows, Hkv * D, generator=g, dtype=F64) * s)
    v = torch.randn(rows, Hkv * D, generator=g, dtype=F64)
    dout = torch.randn(rows, Hq * D, generator=g, dtype=F64)
    return q, k, v, dout


# (Hq, Hkv, causal, masked, packed lens or None, scale): every axis of the emulator's exact mode
CASES = [
    (4, 4, True, False, None, None),
    (4, 2, True, True, None, None),
    (8, 2, False, True, None, None),
    (8, 1, False, False, None, 0.05),
    (4, 1, True, True, [37, 5, 20], None),
    (6, 3, False, True, [9, 40], 0.3),
    (2, 2, True, True, None, 0.05),
]


@pytest.mark.parametrize("Hq,Hkv,causal,masked,lens,scale", CASES)
def test_emulator_exact_mode_equals_fp64_autograd(Hq, Hkv, causal, masked, lens, scale):
    D, B, S = 32, 2, 40
    scale = D ** -0.5 if scale is None else scale
    cu = None
    if lens is not None:
        B, cu = len(lens), [0]
        for n in lens:
            cu.append(cu[-1] + n)
        S = max(lens)
        rows, clips = cu[-1], [(cu[b], lens[b]) for b in range(B)]
    else:
        rows, clips = B * S, [(b * S, S) for b in range(B)]
    q, k, v, dout = _inputs(rows, Hq, Hkv, D, seed=Hq * 100 + rows, peaky=not causal)
    mask = None
    if masked:
        mask = torch.ones(rows, dtype=torch.uint8)
        r0, n = clips[-1]
        mask[r0 + n - n // 3:] = 0                  # padded tail of the last clip
        mask[clips[0][0] + 3] = 0                   # an interior key of the first
        if causal:
            mask[r0] = 0                            # key 0 of the last clip: its first row sees no key at all
    kw = dict(Hq=Hq, Hkv=Hkv, causal=causal, scale=scale, key_mask=mask, B=B, S=S, cu=cu)
    out, lse, _ = attn_fwd_ref(q, k, v, **kw)
    got = attn_bwd_emul(q, k, v, dout, out, lse, rounding=False, **kw)
    ref = _autograd(q, k, v, dout, Hq, Hkv, causal, scale, mask, clips)
    for name, a, r in zip(("dq", "dk", "dv"), got, ref):
        assert torch.isfinite(a).all(), name
        err = float((a - r).abs().max())
        assert err <= 1e-9 * max(1.0, float(r.abs().max())), (name, err)


def test_emulator_fully_masked_rows_are_zero():
    """rounding on: rows with no valid key (a causal clip whose key 0 is masked, a non-causal clip with every key
    masked) carry lse = -inf and must give exact zeros, never NaN."""
    D, B, S, Hq, Hkv = 32, 2, 24, 4, 2
    q, k, v, dout = _inputs(B * S, Hq, Hkv, D, seed=3)
    q, k, v, dout = (t.to(torch.bfloat16) for t in (q, k, v, dout))
    for causal in (True, False):
        mask = torch.ones(B * S, dtype=torch.uint8)
        if causal:
            mask[S] = 0                             # clip 1, key 0: its row 0 is fully masked
            dead = [S]
        else:
            mask[S:] = 0                            # clip 1: every key
            dead = list(range(S, 2 * S))
        kw = dict(Hq=Hq, Hkv=Hkv, causal=causal, scale=D ** -0.5, key_mask=mask, B=B, S=S)
        out, lse, _ = attn_fwd_ref(q, k, v, **kw)
        assert torch.isinf(lse[1, :, 0]).all() and (lse[1, :, 0] < 0).all()
        dq, dk, dv = attn_bwd_emul(q, k, v, dout, out.to(torch.bfloat16), lse.float(), rounding=True, **kw)
        for t in (dq, dk, dv):
            assert torch.isfinite(t).all()
        assert (dq[dead] == 0).all()
        if not causal:
            assert (dk[S:] == 0).all() and (dv[S:] == 0).all()
        assert dq[:S].abs().max() > 0 and dk[:S].abs().max() > 0


def test_emulator_rounding_points_are_bf16():
    """rounding on: every output is a bf16 value, and it is not the exact result (the rounding points are live)."""
    D, B, S, Hq, Hkv = 32, 1, 48, 4, 2
    q, k, v, dout = (t.to(torch.bfloat16) for t in _inputs(B * S, Hq, Hkv, D, seed=11))
    kw = dict(Hq=Hq, Hkv=Hkv, causal=True, scale=D ** -0.5, B=B, S=S)
    out, lse, _ = attn_fwd_ref(q, k, v, **kw)
    rnd = attn_bwd_emul(q, k, v, dout, out, lse, rounding=True, **kw)
    ex = attn_bwd_emul(q, k, v, dout, out, lse, rounding=False, **kw)
    for a, e in zip(rnd, ex):
        assert torch.equal(a, a.to(torch.bfloat16).to(a.dtype))
        assert not torch.equal(a, e)
        assert float((a - e).norm() / e.norm()) < 2e-2


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_emulator_mutations_change_the_result(mutation):
    """Each deliberately wrong emulator the GPU mutation check uses really computes something else at that check's
    shape (GQA, causal, S = 300 so the last 64-key tile is partial)."""
    D, B, S, Hq, Hkv = 32, 1, 300, 4, 2
    q, k, v, dout = (t.to(torch.bfloat16) for t in _inputs(B * S, Hq, Hkv, D, seed=5))
    kw = dict(Hq=Hq, Hkv=Hkv, causal=True, scale=D ** -0.5, B=B, S=S)
    out, lse, _ = attn_fwd_ref(q, k, v, **kw)
    good = attn_bwd_emul(q, k, v, dout, out, lse, **kw)
    bad = attn_bwd_emul(q, k, v, dout, out, lse, mutation=mutation, **kw)
    worst = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(bad, good))
    assert worst > 5e-2, (mutation, worst)
