"""The clip+AdamW step of csrc/adamw.hip, restated on the host, and the real-number AdamW it approximates.

Three layers, each tied to the next by a test:

  * ``emul_step`` (+ ``host_scalars``): ``adamw_update`` and the host part of ``adamw_launch`` operation for operation in
    numpy float32 - every product, quotient and square root rounded once, every fused multiply-add through ``fma32`` (one
    rounding), ``powf`` from the C library the launcher itself calls.  It reproduces every digest of
    tests/golden/adamw_parent_bits.json on the CPU (test_cpu_adamw_emul.py), i.e. bits a GPU produced, and is what
    test_gpu_adamw_emul.py compares the kernels with under ``torch.equal``.  The EMA line is ema_emul.ema_step.
  * ``ref_step``: the same update in real-number form in torch float64 (CPU or device), fed the float32 VALUES of the
    hyperparameters; equal to torch.optim.AdamW on float64 tensors to 1e-12.
  * ``bars``: the per-element bound on |emul_step - ref_step| derived from the roundings the kernel makes.
"""
import ctypes
import ctypes.util

import numpy as np
import torch

F32 = np.float32
U = 2.0 ** -24                      # unit roundoff of float32: one rounding moves a value by at most U * |value|

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.powf.restype = ctypes.c_float
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]


# --------------------------------------------------------------------------------------------------- float32 primitives
def fma32(a, b, c):
    """float32 round(a * b + c) with ONE rounding, element-wise.

    The product of two float32 is exact in float64 (48 significant bits).  s = fl64(prod + c) and its TwoSum residual r
    (s + r = prod + c exactly) give the exact sum; where r != 0, s is replaced by its round-to-odd neighbour (the one of the two
    float64 values around the exact sum whose last bit is set), which keeps "above / below / on a float32 tie" visible to the
    final rounding to float32: 53 >= 24 + 2 bits, so the double rounding is innocuous (Boldo & Melquiond)."""
    a, b, c = (np.asarray(x, dtype=F32).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        prod = a * b
        s = np.asarray(prod + c)
        bb = s - prod
        r = (prod - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & (r != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(r > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


def bf16_bits(x):
    """float32 -> bf16 bit patterns (uint16), round to nearest even on the fp32 pattern; a NaN becomes a quiet NaN of its sign
    (which NaN the device writes is not specified: compare NaN-ness, not NaN bits)."""
    x = np.ascontiguousarray(x, dtype=F32)
    bits = x.view(np.uint32).astype(np.uint64)
    out = ((bits + np.uint64(0x7FFF) + ((bits >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
    nan = np.isnan(x)
    return np.where(nan, ((bits >> np.uint64(16)).astype(np.uint16) & np.uint16(0x8000)) | np.uint16(0x7FC0), out)


def bf16_is_nan(bits):
    bits = np.asarray(bits, dtype=np.uint16)
    return (bits & np.uint16(0x7FFF)) > np.uint16(0x7F80)


def powf(x, y):
    return F32(_libm.powf(float(F32(x)), float(F32(y))))


# --------------------------------------------------------------------------------------------------- the restatement
def host_scalars(lr, b1, b2, eps, wd, step, sumsq=None, max_norm=0.0):
    """What adamw_launch (bc1, bc2s) and the kernel's prologue (clip, decay, lr_bc, ob1, ob2) compute, in float32.
    ``sumsq`` None: the entry got a null pointer.  -> dict of float32 scalars."""
    lr, b1, b2, eps, wd, max_norm, one = F32(lr), F32(b1), F32(b2), F32(eps), F32(wd), F32(max_norm), F32(1)
    with np.errstate(all="ignore"):
        t = float(F32(step))
        bc1 = F32(one - powf(b1, t))
        bc2s = F32(np.sqrt(F32(one - powf(b2, t))))
        clip = one
        if max_norm > 0 and sumsq is not None:
            clip = F32(np.fmin(one, F32(max_norm / F32(np.sqrt(F32(sumsq)) + F32(1e-6)))))
        return dict(lr=lr, b1=b1, b2=b2, eps=eps, wd=wd, bc1=bc1, bc2s=bc2s, clip=clip, decay=F32(fma32(-lr, wd, one)),
                    lr_bc=F32(lr / bc1), ob1=F32(one - b1), ob2=F32(one - b2))


def emul_step(p, m, v, g, *, g16, scalars):
    """adamw_update on float32 arrays (``g``: the gradient's float32 values - a bf16 gradient widened, which is exact).
    ``g16`` picks the moment order of the bf16-gradient kernels.  -> (p', m', v', bf16 bit patterns of p')."""
    p, m, v, g = (np.asarray(x) for x in (p, m, v, g))
    assert all(x.dtype == F32 for x in (p, m, v, g))
    s = scalars
    with np.errstate(all="ignore"):
        gi = g * s["clip"]
        if g16:
            m2 = fma32(s["b1"], m, s["ob1"] * gi)
            v2 = fma32(s["b2"], v, (s["ob2"] * gi) * gi)
        else:
            m2 = fma32(s["ob1"], gi, s["b1"] * m)
            v2 = fma32(gi, s["ob2"] * gi, s["b2"] * v)
        q = (s["lr_bc"] * m2) / (np.sqrt(v2) / s["bc2s"] + s["eps"])
        p2 = fma32(s["decay"], p, -q)
    assert p2.dtype == m2.dtype == v2.dtype == q.dtype == F32
    return p2, m2, v2, bf16_bits(p2)


def emul_groups(p, m, v, g, group, lrs, wds, *, g16, b1, b2, eps, step, sumsq=None, max_norm=0.0):
    """The table entries: ``group`` holds every element's group; emul_step with each group's (lr, weight_decay) on its elements
    (the update is element-wise, so this is one call per range with that range's pair)."""
    p, m, v, g, group = (np.asarray(x) for x in (p, m, v, g, group))
    out = [np.empty_like(p), np.empty_like(p), np.empty_like(p), np.empty(p.shape, np.uint16)]
    done = np.zeros(p.shape, bool)
    for k, (lr, wd) in enumerate(zip(lrs, wds)):
        sel = group == k
        res = emul_step(p[sel], m[sel], v[sel], g[sel], g16=g16, scalars=host_scalars(lr, b1, b2, eps, wd, step, sumsq, max_norm))
        for o, r in zip(out, res):
            o[sel] = r
        done |= sel
    assert done.all()
    return tuple(out)


def group_of_elements(bounds, group_of, idx):
    """Element indices -> their range's group (bounds[r] <= e < bounds[r + 1])."""
    r = np.searchsorted(np.asarray(bounds, dtype=np.int64), np.asarray(idx, dtype=np.int64), side="right") - 1
    return np.asarray(group_of)[r]


# --------------------------------------------------------------------------------------------------- the reference
MUTATIONS = ("no_bc1", "no_bc2", "step_plus_1", "eps_in_sqrt", "l2_decay", "clip_by_sumsq", "unclipped_moments")


def _f(x):
    """A hyperparameter's float32 value as a python float; a tensor (one value per element, float32-valued) passes."""
    return x.double() if torch.is_tensor(x) else float(F32(x))


def ref_step(p, m, v, g, *, lr, b1, b2, eps, wd, step, sumsq=None, max_norm=0.0, mutation=None):
    """Clip + AdamW in real-number form, torch float64 on the inputs' device:

        clip = min(1, max_norm / (sqrt(sumsq) + 1e-6f))  when max_norm > 0 and a sumsq is given, else 1;   gi = g * clip
        m' = b1 m + (1 - b1) gi;   v' = b2 v + (1 - b2) gi^2;   bc1 = 1 - b1^t;   bc2 = 1 - b2^t
        p' = (1 - lr wd) p - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps)

    on the float32 values of lr, b1, b2, eps, wd, max_norm, 1e-6f and sumsq (``lr`` / ``wd`` may be per-element tensors).
    ``mutation`` (one of MUTATIONS) is a deliberately WRONG optimiser, for the sensitivity test only.
    -> dict: m, v, p and the intermediates ``bars`` needs."""
    assert mutation is None or mutation in MUTATIONS
    p, m, v, g = (x.double() for x in (p, m, v, g))
    lr, wd, b1, b2, eps = _f(lr), _f(wd), _f(b1), _f(b2), _f(eps)
    t = step + 1 if mutation == "step_plus_1" else step
    ratio = None
    if float(F32(max_norm)) > 0 and sumsq is not None:
        ss = float(F32(sumsq))
        norm = ss if mutation == "clip_by_sumsq" else (ss ** 0.5 if ss >= 0 else float("nan"))
        ratio = float(F32(max_norm)) / (norm + float(F32(1e-6)))
    clip = 1.0 if ratio is None or not ratio < 1.0 else ratio
    gc = g * clip
    gi = g if mutation == "unclipped_moments" else gc
    if mutation == "l2_decay":
        gi = gi + wd * p
    b1t, b2t = b1 ** t, b2 ** t
    bc1 = 1.0 if mutation == "no_bc1" else 1.0 - b1t
    bc2 = 1.0 if mutation == "no_bc2" else 1.0 - b2t
    t_m, t_g = b1 * m, (1.0 - b1) * gi
    t_v, t_gg = b2 * v, (1.0 - b2) * gi * gi
    m2, v2 = t_m + t_g, t_v + t_gg
    if mutation == "eps_in_sqrt":
        s = (v2 / bc2).sqrt()
        den = (v2 / bc2 + eps).sqrt()
    else:
        s = v2.sqrt() / bc2 ** 0.5
        den = s + eps
    q = (lr / bc1) * m2 / den
    decay = 1.0 if mutation == "l2_decay" else 1.0 - lr * wd
    p2 = decay * p - q
    return dict(m=m2, v=v2, p=p2, q=q, s=s, den=den, lr_bc=lr / bc1, decay_p=decay * p, t_m=t_m, t_g=t_g, t_v=t_v, t_gg=t_gg,
                b1t=b1t, b2t=b2t, bc1=bc1, bc2=bc2, clip_ratio=ratio)


def bars(R):
    """Per-element bound on |kernel - ref_step| for (m', v', p'), from ``R`` = ref_step(...) of the same inputs.  u = 2^-24;
    first order in u, every rounding counted at its full u * |value|.

      gi   clip = fmin(1, max_norm / (sqrt(sumsq) + 1e-6)) rounds in sqrt, add and divide, and g * clip once more:
           e_c = 4u relative when the clip is active (ratio < 1 on either side of its rounding), 0 otherwise (clip = 1, gi = g).
      m'   two terms, b1 m and ob1 gi.  Roundings: ob1 = 1 - b1 (u), the product kept rounded (u), the fma's result (u), and
           e_c on gi.  No term sees more than e_c + 3u:                 bar_m = (e_c + 3u) (|b1 m| + |ob1 gi|).
      v'   gi^2 carries 2 e_c; ob2 = 1 - b2 (u), ob2 gi (u), the bf16 order's (ob2 gi) gi (u), the fma's result (u):
                                                                        bar_v = (2 e_c + 4u) (b2 v + ob2 gi^2).
      bc1  = 1 - powf(b1, t): powf is good to one ulp (2u b1^t absolute), the subtraction rounds once (u bc1):
           e_bc1 = u (1 + 2 b1^t / bc1) relative - at step 2 with b2 = 0.999 the cancellation loses 9 bits, and this term is
           what carries them.  bc2s = sqrtf(1 - powf(b2, t)): the square root halves the incoming error and rounds once:
           e_bc2s = u (1 + 2 b2^t / bc2) / 2 + u.
      den  = sqrtf(v') / bc2s + eps.  With s = sqrt(v') / sqrt(bc2): sqrtf halves bar_v / v' and rounds (u), the division
           carries e_bc2s and rounds (u), the sum rounds (u den):       D_den = (bar_v / v' / 2 + 2u + e_bc2s) s + u den.
      q    = (lr_bc m') / den with lr_bc = lr / bc1 (e_bc1 + u), the product (u), the division (u):
                                                                        bar_q = |lr / bc1 / den| bar_m + |q| (e_bc1 + 3u + D_den / den).
      p'   = fma(decay, p, -q) with decay = fma(-lr, wd, 1) (u): one rounding of decay on |decay p|, one of the result on |p'|;
           a second u |decay p| + u |q| is kept as slack for second-order terms:
                                                                        bar_p = bar_q + u (2 |decay p| + |q|) + u |p'|.
    Relative bounds: they hold where no operand or result is subnormal in float32."""
    u = U
    active = R["clip_ratio"] is not None and R["clip_ratio"] < 1.0 + 4 * u
    e_c = 4 * u if active else 0.0
    e_bc1 = u * (1 + 2 * R["b1t"] / R["bc1"])
    e_bc2s = 0.5 * u * (1 + 2 * R["b2t"] / R["bc2"]) + u
    bar_m = (e_c + 3 * u) * (R["t_m"].abs() + R["t_g"].abs())
    bar_v = (2 * e_c + 4 * u) * (R["t_v"] + R["t_gg"])
    s, den, q = R["s"], R["den"], R["q"].abs()
    rel_v = torch.where(R["v"] > 0, bar_v / R["v"], torch.zeros_like(bar_v))
    d_den = (0.5 * rel_v + 2 * u + e_bc2s) * s + u * den
    bar_q = (R["lr_bc"] / den).abs() * bar_m + q * (e_bc1 + 3 * u + d_den / den)
    bar_p = bar_q + u * (2 * R["decay_p"].abs() + q) + u * R["p"].abs()
    return bar_m, bar_v, bar_p


def worst_ratio(got, R, B):
    """max over m', v', p' and all elements of |got - ref| / bar (0 / 0 counts as 0) and the number of elements outside.
    ``got`` = (p', m', v') as float tensors."""
    worst, outside = torch.zeros((), dtype=torch.float64, device=R["p"].device), 0
    for x, key, bar in ((got[1], "m", B[0]), (got[2], "v", B[1]), (got[0], "p", B[2])):
        err = (x.double() - R[key]).abs()
        ok = err <= bar
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bar)
        worst = torch.maximum(worst, torch.nan_to_num(ratio, nan=float("inf")).max())
        outside = outside + (~ok).sum()
    return worst, outside
