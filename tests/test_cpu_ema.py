"""Weight averaging (litmodule.config.ema_decay), the parts that need no GPU: the float32 emulation of the
kernel's EMA line against its float64 reference, the warm-up schedule, the configuration checks, and the ABI of the two
new entry points (their host-side argument checks included: they return before anything is launched)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ema_emul as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(**kw):
    from phantom_vlb_amd.litmodule import VLBLitModuleConfig
    base = dict(model_path="none", freeze_backbone=True, use_lora=False, lora_r=None, lora_alpha=None, lora_dropout=None,
                dropout_rate=0.0, num_target=128, l2_lambda=1e-3, lr=1e-3, betas=[0.9, 0.999], eps=1e-8,
                weight_decay=1e-2, lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=50000, geometry="mini")
    base.update(kw)
    return VLBLitModuleConfig(**base)


# ------------------------------------------------------------------------------------------------ emulation
def test_decay_pair_is_float32_and_one_minus_d_is_one_rounding():
    for d in (0.0, 0.5, 0.9, 0.999, 2 / 11, 0.9999):
        d32, omd = E.decay_pair(d)
        assert d32.dtype == np.float32 and omd.dtype == np.float32
        assert float(omd) == float(np.float32(1.0 - float(d32)))         # the exact difference, rounded once
    assert E.decay_pair(0.0) == (0.0, 1.0)


def test_emulation_rounds_each_of_the_three_operations():
    """A case where a fused multiply-add would differ: the emulation is the separately rounded value, by construction of the
    operands (d * ema is inexact in float32, and its rounding error survives the sum)."""
    ema = np.array([1.0 + 2.0 ** -23], dtype=np.float32)
    p = np.array([3.0], dtype=np.float32)
    d = 0.999
    d32, omd = E.decay_pair(d)
    got = E.ema_step(ema, p, d)
    a = np.float32(np.float64(d32) * np.float64(ema[0]))              # product rounded to float32
    b = np.float32(np.float64(omd) * np.float64(p[0]))
    assert got.dtype == np.float32 and got[0] == np.float32(np.float64(a) + np.float64(b))
    assert np.float64(a) != np.float64(d32) * np.float64(ema[0])      # the product really was rounded
    # d = 0 copies p' exactly; d = 0.5 of equal values returns them
    assert np.array_equal(E.ema_step(ema, p, 0.0), p)
    assert np.array_equal(E.ema_step(p, p, 0.5), p)


@pytest.mark.parametrize("d", [0.5, 0.9, 0.999])
@pytest.mark.parametrize("M", [1.0, 37.5])
def test_emulation_stays_within_the_derived_bound_of_the_fp64_reference(d, M):
    rng = np.random.default_rng(int(d * 1000) + int(M))
    n, T = 4096, 200
    ema = rng.uniform(-M, M, n).astype(np.float32)
    ref = ema.astype(np.float64)
    worst = 0.0
    for t in range(1, T + 1):
        p = rng.uniform(-M, M, n).astype(np.float32)
        ema = E.ema_step(ema, p, d)
        ref = E.ema_step_ref(ref, p, d)
        err = float(np.abs(ema.astype(np.float64) - ref).max())
        assert err <= E.drift_bound(t, M), (t, err, E.drift_bound(t, M))
        worst = max(worst, err)
    assert worst > 0.0                                                   # float32 does round: the bound is not vacuous
    assert float(np.abs(ema).max()) <= M


def test_drift_bound_formula():
    assert E.drift_bound(1, 1.0) == 3 * 2.0 ** -24
    assert E.drift_bound(6, 2.0) == 3 * 6 * 2.0 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ warm-up
def test_ema_decay_at():
    from phantom_vlb_amd.optim import ema_decay_at
    got = [ema_decay_at(t, 0.999, True) for t in range(1, 6)]
    assert got == [2 / 11, 3 / 12, 4 / 13, 5 / 14, 6 / 15]
    # (1 + t) / (10 + t) reaches 0.999 at t = 8990: below it the ramp, behind it the cap
    assert ema_decay_at(8980, 0.999, True) == 8981 / 8990 < 0.999
    assert ema_decay_at(9000, 0.999, True) == 0.999 and ema_decay_at(10 ** 6, 0.999, True) == 0.999
    assert [ema_decay_at(t, 0.5, True) for t in (1, 7, 8, 9)] == [2 / 11, 8 / 17, 0.5, 0.5]
    assert all(ema_decay_at(t, 0.999, False) == 0.999 for t in (1, 2, 50, 10 ** 6))
    assert all(0 < ema_decay_at(t, 0.9, True) < 1 for t in range(1, 100))
    with pytest.raises(ValueError):
        ema_decay_at(0, 0.999, True)


# ------------------------------------------------------------------------------------------------ configuration
def test_config_defaults_and_accepted_values():
    c = _cfg()
    assert c.ema_decay is None and c.ema_warmup is True and c.ema_eval is True
    c = _cfg(ema_decay=0.999, ema_warmup=False, ema_eval=False)
    assert c.ema_decay == 0.999 and c.ema_warmup is False and c.ema_eval is False
    assert _cfg(use_lora=True, freeze_backbone=False, lora_r=16, lora_alpha=32, lora_dropout=0.0, ema_decay=0.5).ema_decay == 0.5
    # off: the other two are not looked at, whatever they are - also for the full fine-tune
    for warm in (True, False):
        for ev in (True, False):
            assert _cfg(ema_decay=None, ema_warmup=warm, ema_eval=ev).ema_decay is None
            assert _cfg(freeze_backbone=False, use_lora=False, ema_decay=None, ema_warmup=warm, ema_eval=ev).ema_decay is None


def test_config_value_from_the_command_line_parser():
    """`litmodule.config.ema_decay=0.999 litmodule.config.ema_warmup=false` as config.load_config's override parser sets them."""
    from phantom_vlb_amd.config import _set
    cfg = {"litmodule": {"config": {}}}
    _set(cfg, "litmodule.config.ema_decay", "0.999")
    _set(cfg, "litmodule.config.ema_warmup", "false")
    _set(cfg, "litmodule.config.ema_eval", "true")
    c = _cfg(**cfg["litmodule"]["config"])
    assert c.ema_decay == 0.999 and c.ema_warmup is False and c.ema_eval is True


@pytest.mark.parametrize("bad", [0, 1, -0.1, True, "x", 1.5, float("nan")])
def test_config_refuses_ema_decay(bad):
    with pytest.raises(ValueError, match="ema_decay"):
        _cfg(ema_decay=bad)


@pytest.mark.parametrize("field", ["ema_warmup", "ema_eval"])
@pytest.mark.parametrize("bad", [1, 0, "true", None, 0.5])
def test_config_refuses_flags_that_are_not_booleans(field, bad):
    with pytest.raises(ValueError, match=field):
        _cfg(ema_decay=0.9, **{field: bad})


def test_config_refuses_the_full_finetune():
    with pytest.raises(ValueError, match=r"ema_decay.*full fine-tune.*bf16-gradient store has no EMA kernel.*28 GB"):
        _cfg(freeze_backbone=False, use_lora=False, ema_decay=0.999)


# ------------------------------------------------------------------------------------------------ ABI
NEW_ENTRIES = {"vlb_adamw_step_ema": 17, "vlb_adamw_step_groups_ema": 21}


def test_new_entries_are_declared_bound_and_exported():
    """header == SIGNATURES == nm -D for the two new entries (parameter kinds in the same positions); ABI version still 2"""
    from phantom_vlb_amd import _lib
    raw = open(os.path.join(ROOT, "include", "vlb.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()[-2] == "T"}
    want = {ctypes.c_void_p: "P", ctypes.c_int: "I", ctypes.c_float: "F", ctypes.c_int64: "L"}
    for name, n in NEW_ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
        assert m, f"{name} is not declared in include/vlb.h"
        params = [p.strip() for p in m.group(1).split(",")]
        assert len(params) == len(_lib.SIGNATURES[name]) == n, name
        kinds = ["P" if "*" in p else "F" if p.startswith("float") else "L" if p.startswith("int64_t") else "I" for p in params]
        assert kinds == [want[t] for t in _lib.SIGNATURES[name]], name
        assert any("ema" in p and "*" in p for p in params) and params[-2] == "float ema_decay" and params[-1] == "void* stream"
        assert name in exported and hasattr(_lib.lib, name), name
    # the parents' own declarations are where they were
    assert _lib.SIGNATURES["vlb_adamw_step"] == [ctypes.c_void_p] * 5 + [ctypes.c_int64] + [ctypes.c_float] * 5 + \
        [ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p]
    assert _lib.lib.vlb_abi_version() == 2 and "#define VLB_ABI_VERSION 2" in raw


def test_entries_refuse_bad_arguments_without_a_device():
    """n % 8, a misaligned or missing ema, ema_decay outside [0, 1), a missing table: errors before anything is launched
    (the pointers are never dereferenced on the host)."""
    from phantom_vlb_amd._lib import lib
    P = ctypes.c_void_p
    ok = [P(4096), P(8192), P(12288), P(16384), P(20480), P(24576)]            # master, bf16, grad, m, v, ema

    def plain(ptrs=ok, n=64, d=0.9, step=1):
        return lib.vlb_adamw_step_ema(*ptrs, n, 1e-3, 0.9, 0.999, 1e-8, 1e-2, step, None, 1.0, d, None)

    def grouped(ptrs=ok, n=64, d=0.9, bounds=P(32768), group_of=P(36864), n_ranges=1, G=1):
        lr = (ctypes.c_float * 8)(*([1e-3] * 8))
        return lib.vlb_adamw_step_groups_ema(*ptrs, n, bounds, group_of, n_ranges, lr, lr, G, 0.9, 0.999, 1e-8, 1, None, 1.0, d, None)

    for call in (plain, grouped):
        assert call(n=60) != 0 and call(n=0) != 0                                  # a positive multiple of 8
        assert call(d=1.0) != 0 and call(d=-0.1) != 0 and call(d=1.5) != 0         # 0 <= ema_decay < 1
        assert call(ptrs=ok[:5] + [P(24576 + 4)]) != 0                             # ema not 16-byte aligned
        assert call(ptrs=ok[:5] + [None]) != 0                                     # no ema
        assert call(ptrs=[None] + ok[1:]) != 0
    assert plain(step=0) != 0
    assert grouped(bounds=None) != 0 and grouped(group_of=None) != 0 and grouped(n_ranges=0) != 0 and grouped(n_ranges=9) != 0
    assert grouped(G=0) != 0 and grouped(G=9) != 0
    assert b"ema" in lib.vlb_last_error()
