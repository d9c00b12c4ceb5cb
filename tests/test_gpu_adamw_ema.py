"""vlb_adamw_step_ema / vlb_adamw_step_groups_ema against the entries they stand in for (helpers shared with
test_gpu_adamw_groups.py live in adamw_cases.py).

master, both moments and the bf16 copy must be torch.equal to the parent's (vlb_adamw_step / vlb_adamw_step_groups) on the
same inputs; ``ema`` must be torch.equal to tests/ema_emul.py's float32 restatement applied to the kernel's OWN new master
(three separately rounded operations: a fused multiply-add in the kernel would show).  Bare buffers with 64 guard elements
behind each; the shapes are the smallest at which the loop can go wrong (one vector pair, a workgroup chunk's edge, a
ragged last workgroup, the grid-stride loop's second trip with its prefetch of ``ema``)."""
import numpy as np
import pytest
import torch

import ema_emul as E
from adamw_cases import BETAS, EPS, LR, MAX_NORM, TAIL, WD, _clone, _random_bounds, _rates, _state, _stream, _table_args

pytestmark = pytest.mark.gpu

SHAPES = {"one_vector_pair": 8, "chunk_edge": 8 * 1031, "ragged_last_workgroup": 8 * (3 * 2 ** 16 + 5),
          "second_grid_stride_trip": 8 * (2 ** 23 + 2 ** 10 + 3)}
DECAYS = (0.0, 0.5, 0.999)


def _parent(st, n, step, sumsq, with_pb, lr=LR, wd=WD):
    from phantom_vlb_amd._lib import check, lib
    check(lib.vlb_adamw_step(st["p"].data_ptr(), st["pb"].data_ptr() if with_pb else None, st["g"].data_ptr(), st["m"].data_ptr(),
                             st["v"].data_ptr(), n, lr, BETAS[0], BETAS[1], EPS, wd, step, sumsq.data_ptr(), MAX_NORM, _stream()),
          "vlb_adamw_step")


def _ema_step(st, n, step, sumsq, with_pb, d, ema_off=0, lr=LR, wd=WD):
    from phantom_vlb_amd._lib import check, lib
    check(lib.vlb_adamw_step_ema(st["p"].data_ptr(), st["pb"].data_ptr() if with_pb else None, st["g"].data_ptr(), st["m"].data_ptr(),
                                 st["v"].data_ptr(), st["ema"].data_ptr() + ema_off, n, lr, BETAS[0], BETAS[1], EPS, wd, step,
                                 sumsq.data_ptr(), MAX_NORM, d, _stream()), "vlb_adamw_step_ema")


def _parent_groups(st, n, table, step, sumsq, with_pb):
    from phantom_vlb_amd._lib import check, lib
    check(lib.vlb_adamw_step_groups(st["p"].data_ptr(), st["pb"].data_ptr() if with_pb else None, st["g"].data_ptr(), st["m"].data_ptr(),
                                    st["v"].data_ptr(), n, *table, BETAS[0], BETAS[1], EPS, step, sumsq.data_ptr(), MAX_NORM, _stream()),
          "vlb_adamw_step_groups")


def _ema_groups(st, n, table, step, sumsq, with_pb, d):
    from phantom_vlb_amd._lib import check, lib
    check(lib.vlb_adamw_step_groups_ema(st["p"].data_ptr(), st["pb"].data_ptr() if with_pb else None, st["g"].data_ptr(),
                                        st["m"].data_ptr(), st["v"].data_ptr(), st["ema"].data_ptr(), n, *table, BETAS[0], BETAS[1], EPS,
                                        step, sumsq.data_ptr(), MAX_NORM, d, _stream()), "vlb_adamw_step_groups_ema")


def _emulated(ema_before, p_after, d):
    """ema_emul.ema_step on host copies -> a tensor on the buffers' device."""
    out = E.ema_step(ema_before.cpu().numpy(), p_after.cpu().numpy(), d)
    return torch.from_numpy(out).to(p_after.device)


def _compare(got, want, st0, n, d, with_pb, tag):
    for k in ("p", "m", "v", "pb", "g"):
        assert torch.equal(got[k], want[k]), (tag, k, int((got[k] != want[k]).sum()))
    for k in got:
        assert torch.equal(got[k][n:], st0[k][n:]), (tag, k, "wrote behind the end")
    assert not torch.equal(got["p"][:n], st0["p"][:n])
    assert torch.equal(got["pb"], st0["pb"]) == (not with_pb)
    emu = _emulated(st0["ema"][:n], got["p"][:n], d)
    assert torch.equal(got["ema"][:n], emu), (tag, "ema", int((got["ema"][:n] != emu).sum()))
    if d == 0.0:
        assert torch.equal(got["ema"][:n], got["p"][:n])


def _variants(n):
    """(sum of squares for the clip, step, write the bf16 copy, decay): clip active / inactive, bias correction at step 1 / 7,
    with / without the bf16 pointer, every decay.  The small shapes run the full product; the 1.5M-element shape the eight
    combinations with the decays in rotation; the 67M-element shape three runs that between them take every value of
    every option (a run there moves gigabytes through the host emulation)."""
    if n > 2 ** 24:
        return [(1e4, 1, True, 0.999), (1e-2, 7, False, 0.5), (1e4, 7, False, 0.0)]
    combos = [(ss, step, pb) for ss in (1e4, 1e-2) for step in (1, 7) for pb in (True, False)]
    if n > 8 * 1031:
        return [c + (DECAYS[i % 3],) for i, c in enumerate(combos)]
    return [c + (d,) for c in combos for d in DECAYS]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_ungrouped_equals_vlb_adamw_step_and_the_emulation(dev, shape):
    n = SHAPES[shape]
    st0 = _state(n, dev, seed=n % 1000, ema=True)
    seen = set()
    for ss, step, with_pb, d in _variants(n):
        seen.add(d)
        sumsq = torch.tensor([ss], dtype=torch.float32, device=dev)
        want, got = _clone(st0), _clone(st0)
        _parent(want, n, step, sumsq, with_pb)
        _ema_step(got, n, step, sumsq, with_pb, d)
        torch.cuda.synchronize()
        assert torch.equal(want["ema"], st0["ema"])
        _compare(got, want, st0, n, d, with_pb, (shape, ss, step, with_pb, d))
        del want, got
    assert seen == set(DECAYS)


@pytest.mark.parametrize("table", ["ranges300_G3_lds", "ranges700_G5_global"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_grouped_equals_vlb_adamw_step_groups_and_the_emulation(dev, shape, table):
    n = SHAPES[shape]
    n_ranges, G = (300, 3) if table.startswith("ranges300") else (700, 5)
    n_ranges = min(n_ranges, n // 8)                       # (a table cannot have more ranges than 8-element units)
    bounds = _random_bounds(n, n_ranges, 11 + G)
    groups = [r % G for r in range(n_ranges)]
    assert bounds[0] == 0 and bounds[-1] == n and all(b % 8 == 0 for b in bounds) and len(groups) == len(bounds) - 1
    lrs, wds = _rates(G)
    d_bounds = torch.tensor(bounds, dtype=torch.int64, device=dev)
    d_groups = torch.tensor(groups, dtype=torch.int32, device=dev)
    args = _table_args(d_bounds, d_groups, lrs, wds)
    st0 = _state(n, dev, seed=n % 1000 + G, ema=True)
    for ss, step, with_pb, d in _variants(n):
        sumsq = torch.tensor([ss], dtype=torch.float32, device=dev)
        want, got = _clone(st0), _clone(st0)
        _parent_groups(want, n, args, step, sumsq, with_pb)
        _ema_groups(got, n, args, step, sumsq, with_pb, d)
        torch.cuda.synchronize()
        _compare(got, want, st0, n, d, with_pb, (shape, table, ss, step, with_pb, d))
        del want, got


def test_trajectory_of_six_steps_with_the_warm_up_decays(dev):
    """Fresh gradients every step, decays 2/11, 3/12, ...: ema equals the emulation after every step and stays within the
    derived bound (ema_emul.drift_bound) of the float64 reference fed with the same masters."""
    from phantom_vlb_amd.optim import ema_decay_at
    n = SHAPES["chunk_edge"]
    st = _state(n, dev, seed=5, ema=True)
    twin = _clone(st)
    gen = torch.Generator(device=dev).manual_seed(6)
    emu = st["ema"][:n].cpu().numpy().copy()
    ref = emu.astype(np.float64)
    peak = float(st["ema"][:n].abs().max())
    for step in range(1, 7):
        g = torch.randn(n + TAIL, device=dev, generator=gen)
        st["g"].copy_(g)
        twin["g"].copy_(g)
        sumsq = (g[:n].double().square().sum()).float().reshape(1)
        d = ema_decay_at(step, 0.999, True)
        _ema_step(st, n, step, sumsq, True, d)
        _parent(twin, n, step, sumsq, True)
        torch.cuda.synchronize()
        for k in ("p", "m", "v", "pb"):
            assert torch.equal(st[k], twin[k]), (step, k)
        p = st["p"][:n].cpu().numpy()
        peak = max(peak, float(np.abs(p).max()))
        emu = E.ema_step(emu, p, d)
        ref = E.ema_step_ref(ref, p, d)
        got = st["ema"][:n].cpu().numpy()
        assert np.array_equal(got, emu), (step, int((got != emu).sum()))
        err = float(np.abs(got.astype(np.float64) - ref).max())
        assert err <= E.drift_bound(step, peak), (step, err, E.drift_bound(step, peak))
    assert d == 7 / 16


def test_bad_arguments_are_refused_before_any_launch(dev):
    from phantom_vlb_amd._lib import VlbError
    n = 64
    st = _state(n, dev, seed=2, ema=True)
    before = _clone(st)
    ss = torch.zeros(1, device=dev)
    bounds = torch.tensor([0, n], dtype=torch.int64, device=dev)
    groups = torch.zeros(1, dtype=torch.int32, device=dev)
    args = _table_args(bounds, groups, [1e-3], [0.0])
    with pytest.raises(VlbError):
        _ema_step(st, n, 1, ss, True, 0.9, ema_off=4)              # ema not 16-byte aligned
    with pytest.raises(VlbError):
        _ema_step(st, n - 4, 1, ss, True, 0.9)                     # n is no multiple of 8
    with pytest.raises(VlbError):
        _ema_step(st, n, 1, ss, True, 1.0)                         # ema_decay = 1
    with pytest.raises(VlbError):
        _ema_groups(st, n - 4, args, 1, ss, True, 0.9)
    with pytest.raises(VlbError):
        _ema_groups(st, n, args, 1, ss, True, 1.0)
    torch.cuda.synchronize()
    assert all(torch.equal(st[k], before[k]) for k in st)
