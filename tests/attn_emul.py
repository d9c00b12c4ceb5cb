"""Test-only references for the HIP attention kernels (phantom_vlb_amd/csrc/attention.hip).

``attn_bwd_emul`` restates the backward pass (attn_delta_kernel, attn_bwd_dkdv_kernel, attn_dkdv_reduce_kernel,
attn_bwd_dq_kernel) in plain torch and rounds exactly where the kernels round: the operands both sides feed to the
matrix products are then the same bf16 values, and what is left between kernel and emulator is fp32 summation order
and the occasional P or dS that rounds the other way.  With ``rounding=False`` every rounding point is the identity and
the function is the exact backward of softmax attention (tests/test_cpu_attn_emul.py proves that against autograd).

``attn_fwd_ref`` is the forward in the working precision: output, lse, and P.|V| (the magnitude the forward's bf16 P
rounding is relative to).

Layout, as the kernels see it: q / dout / out are [rows, Hq*D], k / v are [rows, Hkv*D], lse is [B, Hq, S] with S the
longest clip, key_mask holds one byte per ROW (dense: [B, S] flattened; packed: one per packed row).  Clips are dense
(``cu=None``: clip b = rows b*S .. b*S+S) or packed (``cu``: host ints, clip b = rows cu[b] .. cu[b+1]).
"""
from __future__ import annotations

import torch

BF16 = torch.bfloat16

# deliberately wrong variants for the mutation check (tests/test_gpu_attention.py): each is a bug class a rebuilt
# backward kernel could plausibly have, and the bar must reject the real kernel's output against every one of them
MUTATIONS = ("causal_off_by_one", "ds_scale_omitted", "ds_scale_twice", "gqa_mod", "lse_neighbour", "drop_last_tile")


def _clips(B, S, cu):
    if cu is None:
        return [(b * S, S) for b in range(B)]
    cu = [int(x) for x in cu]
    return [(cu[b], cu[b + 1] - cu[b]) for b in range(len(cu) - 1)]


def _allow(n, keyok, causal, off_by_one=False):
    """[n(query), n(key)] bool: key valid and (causal) key <= query."""
    allow = keyok[None, :].expand(n, n).clone()
    if causal:
        allow &= torch.ones(n, n, dtype=torch.bool, device=keyok.device).tril(-1 if off_by_one else 0)
    return allow


def _keyok(key_mask, r0, n, device):
    if key_mask is None:
        return torch.ones(n, dtype=torch.bool, device=device)
    return key_mask.reshape(-1)[r0:r0 + n].to(device).bool()


def attn_fwd_ref(q, k, v, *, Hq, Hkv, causal, scale, key_mask=None, B=None, S=None, cu=None, dtype=torch.float64,
                 device="cpu"):
    """-> (out [rows, Hq*D], lse [B, Hq, Smax], pv [rows, Hq*D] = P.|V|) in ``dtype``; a row whose keys are all masked
    gives out = 0 and lse = -inf (what the forward kernel writes)."""
    rows, D = q.shape[0], q.shape[1] // Hq
    gsz = Hq // Hkv
    clips = _clips(B, S, cu)
    smax = max(n for _, n in clips)
    out = torch.zeros(rows, Hq, D, dtype=dtype, device=device)
    pv = torch.zeros(rows, Hq, D, dtype=dtype, device=device)
    lse = torch.full((len(clips), Hq, smax), float("-inf"), dtype=dtype, device=device)
    for b, (r0, n) in enumerate(clips):
        allow = _allow(n, _keyok(key_mask, r0, n, device), causal)
        for g in range(Hkv):
            hs = slice(g * gsz, (g + 1) * gsz)
            Q = q[r0:r0 + n].to(device).view(n, Hq, D)[:, hs].to(dtype).transpose(0, 1)       # [G, n, D]
            K = k[r0:r0 + n].to(device).view(n, Hkv, D)[:, g].to(dtype)
            V = v[r0:r0 + n].to(device).view(n, Hkv, D)[:, g].to(dtype)
            s = (Q @ K.t() * scale).masked_fill(~allow, float("-inf"))
            L = torch.logsumexp(s, -1)                                                         # -inf on a dead row
            P = torch.where(allow, torch.exp(s - L[..., None]), torch.zeros((), dtype=dtype, device=device))
            out[r0:r0 + n, hs] = (P @ V).transpose(0, 1)
            pv[r0:r0 + n, hs] = (P @ V.abs()).transpose(0, 1)
            lse[b, hs, :n] = L
    return out.view(rows, Hq * D), lse, pv.view(rows, Hq * D)


def attn_bwd_emul(q, k, v, dout, out, lse, *, Hq, Hkv, causal, scale, key_mask=None, B=None, S=None, cu=None,
                  rounding=True, dtype=torch.float64, device="cpu", budget=False, mutation=None):
    """dQ [rows, Hq*D], dK / dV [rows, Hkv*D] of softmax attention, rounded where attention.hip rounds.

    Returned as bf16-valued tensors in ``dtype`` (exact values in ``dtype`` with ``rounding=False``).  With ``budget``
    also returns two per-element magnitudes for each output:
      flip  - the largest single bf16 operand contribution to it (an upper bound of max_i |a_i . b_i| over the summed
              index, and for a GQA dK / dV the largest per-head bf16 partial): one bf16 ulp of that is what one P, dS
              or partial rounding the other way can move the element;
      noise - what the fp32 error of dP - delta can move it: dP and delta are D-term fp32 dot products (error
              <= D 2^-24 sum|terms| each, on each side), and where dP ~ delta their difference is that error alone.
    """
    assert mutation is None or mutation in MUTATIONS, mutation
    rows, D = q.shape[0], q.shape[1] // Hq
    gsz = Hq // Hkv
    zero = torch.zeros((), dtype=dtype, device=device)

    def r32(x):        # a value the kernel holds in an fp32 register
        return x.float().to(dtype) if rounding else x

    def r16(x):        # an fp32 value the kernel converts to bf16 (round to nearest even, as v_cvt_pk_bf16_f32)
        return x.float().to(BF16).to(dtype) if rounding else x

    ds_scale = {"ds_scale_omitted": 1.0, "ds_scale_twice": scale * scale}.get(mutation, scale)
    dq = torch.zeros(rows, Hq, D, dtype=dtype, device=device)
    dk = torch.zeros(rows, Hkv, D, dtype=dtype, device=device)
    dv = torch.zeros(rows, Hkv, D, dtype=dtype, device=device)
    if budget:
        fq, fk, fv = torch.zeros_like(dq), torch.zeros_like(dk), torch.zeros_like(dv)
        nq, nk = torch.zeros_like(dq), torch.zeros_like(dk)
        ecoef = 2 * D * 2.0 ** -24 * abs(ds_scale)
    for b, (r0, n) in enumerate(_clips(B, S, cu)):
        allow = _allow(n, _keyok(key_mask, r0, n, device), causal, mutation == "causal_off_by_one")
        if mutation == "drop_last_tile" and n % 64:
            allow[:, n - n % 64:] = False
        for g in range(Hkv):
            # heads of kv-head g: hq // gsz == g (the kernels' hkv = hq / (Hq / Hkv))
            hs = [h for h in range(Hq) if (h % Hkv if mutation == "gqa_mod" else h // gsz) == g]
            sl = lambda t, H: t[r0:r0 + n].to(device).view(n, H, D)         # noqa: E731
            Q = sl(q, Hq)[:, hs].to(dtype).transpose(0, 1)                  # [G, n, D]
            dO = sl(dout, Hq)[:, hs].to(dtype).transpose(0, 1)
            O = sl(out, Hq)[:, hs].to(dtype).transpose(0, 1)
            K = sl(k, Hkv)[:, g].to(dtype)                                  # [n, D]
            V = sl(v, Hkv)[:, g].to(dtype)
            lh = [(h + 1) % Hq for h in hs] if mutation == "lse_neighbour" else hs
            L = lse[b, lh, :n].to(device).to(dtype)                         # [G, n]
            live = allow[None] & torch.isfinite(L)[..., None]               # a dead row (lse = -inf) has P = 0, not NaN
            # attn_delta_kernel: delta = sum_d float(out) * float(dO), an fp32 sum
            delta = r32((O * dO).sum(-1))
            # P = exp(S.scale - lse) in fp32; masked entries exactly 0 (attn_bwd_dkdv_kernel :495, attn_bwd_dq_kernel :714)
            P = r32(torch.where(live, torch.exp(Q @ K.t() * scale - L[..., None]), zero))
            # dV^T += dO^T.bf16(P) (:497, :512)
            dV = r16(P).transpose(1, 2) @ dO                                # [G, n(key), D]
            # dS = bf16(P.(dP - delta).scale): the scale is applied before the rounding (:496-498, :715, :724)
            dP = dO @ V.t()
            dS = r16(r32(P * (dP - delta[..., None]) * ds_scale))
            dK = dS.transpose(1, 2) @ Q                                     # dK^T += Q^T.dS (:520)
            dq[r0:r0 + n, hs] = r16(dS @ K).transpose(0, 1)                 # one fp32 accumulation, one rounding (:748)
            if gsz == 1 and mutation != "gqa_mod":
                dk[r0:r0 + n, g], dv[r0:r0 + n, g] = r16(dK[0]), r16(dV[0])   # written directly (:530-531)
            else:
                # bf16 per-head partials (:538), summed in fp32 in head order and rounded (attn_dkdv_reduce_kernel)
                pk, pvv = r16(dK), r16(dV)
                ak, av = torch.zeros_like(pk[0]), torch.zeros_like(pvv[0])
                for j in range(len(hs)):
                    ak, av = r32(ak + pk[j]), r32(av + pvv[j])
                dk[r0:r0 + n, g], dv[r0:r0 + n, g] = r16(ak), r16(av)
            if budget:
                aS, aP = dS.abs(), r16(P).abs()
                fq[r0:r0 + n, hs] = (aS.amax(2)[..., None] * K.abs().amax(0)).transpose(0, 1)
                bk = (aS.amax(1)[..., None] * Q.abs().amax(1)[:, None, :]).amax(0)
                bv = (aP.amax(1)[..., None] * dO.abs().amax(1)[:, None, :]).amax(0)
                if gsz > 1:
                    bk = torch.maximum(bk, dK.abs().amax(0))
                    bv = torch.maximum(bv, dV.abs().amax(0))
                fk[r0:r0 + n, g], fv[r0:r0 + n, g] = bk, bv
                eS = P.abs() * ecoef * (dO.abs() @ V.abs().t() + (O * dO).abs().sum(-1)[..., None])     # |dS| error
                nq[r0:r0 + n, hs] = (eS @ K.abs()).transpose(0, 1)
                nk[r0:r0 + n, g] = (eS.transpose(1, 2) @ Q.abs()).sum(0)
    res = (dq.view(rows, Hq * D), dk.view(rows, Hkv * D), dv.view(rows, Hkv * D))
    if budget:
        flip = (fq.view(rows, Hq * D), fk.view(rows, Hkv * D), fv.view(rows, Hkv * D))
        noise = (nq.view(rows, Hq * D), nk.view(rows, Hkv * D), torch.zeros_like(dv).view(rows, Hkv * D))
        return res, flip, noise
    return res
