"""The EMA line of vlb_adamw_step_ema / vlb_adamw_step_groups_ema, restated on the host.

    ema' = (d * ema) + (omd * p')        d = float32(ema_decay), omd = float32(1) - d

``ema_step`` is the kernel's arithmetic: float32 operands, the two products and the sum each rounded to float32 on their own
(numpy rounds every float32 operation; there is no fused multiply-add), so it reproduces the kernel's ``ema`` bit for bit.
``ema_step_ref`` is the same recurrence in float64 on the SAME float32 values of d and omd: what the kernel would give with
exact arithmetic.  ``drift_bound`` is how far the two can be apart."""
import numpy as np

F32 = np.float32


def decay_pair(d):
    """(d, omd) as the kernel holds them: float32(d) and float32(1) - float32(d), one rounding."""
    d32 = F32(d)
    return d32, F32(F32(1.0) - d32)


def ema_step(ema, p_new, d):
    """One update in the kernel's arithmetic.  ema, p_new: float32 arrays -> float32 array."""
    ema, p_new = np.asarray(ema), np.asarray(p_new)
    assert ema.dtype == F32 and p_new.dtype == F32
    d32, omd = decay_pair(d)
    a = (d32 * ema).astype(F32)
    b = (omd * p_new).astype(F32)
    return (a + b).astype(F32)


def ema_step_ref(ema64, p_new, d):
    """One update in float64 with the float32 values of d and omd.  ema64: float64 array, p_new: float32 array."""
    d32, omd = decay_pair(d)
    return np.float64(d32) * np.asarray(ema64, dtype=np.float64) + np.float64(omd) * np.asarray(p_new, dtype=np.float64)


def drift_bound(steps: int, max_abs: float) -> float:
    """|ema_step chain - ema_step_ref chain| after ``steps`` updates on values of magnitude <= max_abs: every update makes
    three roundings (two products, one sum), each of at most half an ulp of a value <= max_abs, i.e. <= max_abs * 2^-24, and
    carries the error so far forward with the factor d <= 1: 3 * steps * max_abs * 2^-24."""
    return 3.0 * steps * max_abs * 2.0 ** -24
