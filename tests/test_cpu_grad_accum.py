"""Gradient accumulation, the parts that need no GPU: the runner's window arithmetic, its argument check, and the ABI
surface of the two accumulate kernels."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("k", [1, 2, 3, 5])
@pytest.mark.parametrize("n_batches", [1, 4, 5, 6])
def test_every_batch_is_in_exactly_one_window(k, n_batches):
    """Lightning's windows: runs of k batches from the start of the epoch; every batch in exactly one window, no window
    crosses the epoch's end, only the epoch's last window may be short."""
    from phantom_vlb_amd.trainer import accumulation_window
    windows, cur = [], None
    for bi in range(n_batches):
        opens, closes = accumulation_window(bi, n_batches, k)
        assert opens == (cur is None), (bi, opens)          # a window opens exactly when none is open
        if opens:
            cur = []
        cur.append(bi)
        if closes:
            windows.append(cur)
            cur = None
    assert cur is None                                      # the epoch's last batch closed its window
    assert [b for w in windows for b in w] == list(range(n_batches))
    assert all(len(w) == k for w in windows[:-1]) and 1 <= len(windows[-1]) <= k
    assert len(windows) == -(-n_batches // k)               # optimiser steps per epoch


def test_trainer_checks_accumulate_grad_batches():
    from phantom_vlb_amd.trainer import Trainer
    assert Trainer().accumulate_grad_batches == 1 and Trainer(accumulate_grad_batches=4).accumulate_grad_batches == 4
    for bad in (0, -2, "2", 2.0, None, True):
        with pytest.raises(ValueError, match="accumulate_grad_batches"):
            Trainer(accumulate_grad_batches=bad)


def test_accumulate_kernels_are_declared_bound_and_exported():
    """include/vlb.h declares both entry points with the argument order the issue fixes, the ctypes table binds them with
    matching types, the built library exports them, and the ABI version is still 2 (an additive change)."""
    from ctypes import c_int, c_int64, c_void_p
    from phantom_vlb_amd import _lib
    header = open(os.path.join(ROOT, "include", "vlb.h")).read()
    for name, gtype in (("vlb_grad_accum", r"const float\* g"), ("vlb_grad_accum_bf16", r"const void\* g_bf16")):
        assert re.search(rf"int {name}\(float\* acc, {gtype}, int64_t n, int first, float\* sumsq, float\* ws, void\* stream\);", header)
        assert _lib.SIGNATURES[name] == [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p]
        assert getattr(_lib.lib, name).restype is c_int
    assert _lib.lib.vlb_abi_version() == 2 and "#define VLB_ABI_VERSION 2" in header
    # bad arguments are refused by the entry point before any launch (no GPU needed): n = 0, a missing workspace
    assert _lib.lib.vlb_grad_accum(c_void_p(16), c_void_p(32), 0, 1, None, None, None) != 0
    assert _lib.lib.vlb_grad_accum(c_void_p(16), c_void_p(32), 8, 1, c_void_p(64), None, None) != 0
    assert _lib.lib.vlb_grad_accum_bf16(c_void_p(16), c_void_p(36), 8, 1, None, None, None) != 0        # g not 8-byte aligned
