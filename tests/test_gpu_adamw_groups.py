"""vlb_adamw_step_groups / vlb_adamw_step_groups_g16 against the ungrouped entries they stand in for.  All four
launch one kernel family (csrc/adamw.hip): this tests the table search, the LDS staging and the pointer offsets; the arithmetic
is anchored by test_gpu_adamw_bits.py.  Helpers shared with test_gpu_adamw_ema.py live in adamw_cases.py.

AdamW is element-wise once the clip scalar is known, so the grouped step over a range table IS one parent launch
(vlb_adamw_step / vlb_adamw_step_g16) per range, pointers offset to the range, with the range's group's (lr, weight_decay) and
the same sumsq / max_norm / step.  Every comparison is torch.equal on master, both moments and the bf16 copy; the elements
behind the buffer's end must stay untouched.  Bare buffers; the whole file takes a few seconds."""
import pytest
import torch

from adamw_cases import BETAS, BF, EPS, MAX_NORM, _clone, _random_bounds, _rates, _state, _stream, _table_args

pytestmark = pytest.mark.gpu


def _parent(st, s, e, lr, wd, step, sumsq, with_pb):
    from phantom_vlb_amd._lib import check, lib
    bf = st["g"].dtype == BF
    fn = lib.vlb_adamw_step_g16 if bf else lib.vlb_adamw_step
    check(fn(st["p"].data_ptr() + 4 * s, st["pb"].data_ptr() + 2 * s if with_pb else None, st["g"].data_ptr() + (2 if bf else 4) * s,
             st["m"].data_ptr() + 4 * s, st["v"].data_ptr() + 4 * s, e - s, lr, BETAS[0], BETAS[1], EPS, wd, step,
             sumsq.data_ptr(), MAX_NORM, _stream()), "parent adamw")


def _grouped(st, n, bounds, group_of, lrs, wds, step, sumsq, with_pb):
    from phantom_vlb_amd._lib import check, lib
    bf = st["g"].dtype == BF
    fn = lib.vlb_adamw_step_groups_g16 if bf else lib.vlb_adamw_step_groups
    check(fn(st["p"].data_ptr(), st["pb"].data_ptr() if with_pb else None, st["g"].data_ptr(), st["m"].data_ptr(), st["v"].data_ptr(), n,
             *_table_args(bounds, group_of, lrs, wds), BETAS[0], BETAS[1], EPS, step, sumsq.data_ptr(), MAX_NORM, _stream()), "vlb_adamw_step_groups")


def _case(name):
    """-> n, bounds (list), group of every range (list), number of groups."""
    if name == "one_vector_pair":
        return 8, [0, 8], [0], 1
    if name == "block_edges":                 # boundaries one 4-vector pair inside the first / behind the last full workgroup chunk
        return 8 * 1031, [0, 8, 8 * 1029, 8 * 1031], [0, 1, 0], 2
    if name.startswith("ranges300_G"):        # several workgroups, a partial last one, a table no thread could hold in registers
        G = int(name[len("ranges300_G"):])
        n = 8 * (3 * 2 ** 16 + 5)
        return n, _random_bounds(n, 300, 7 + G), [r % G for r in range(300)], G
    if name == "ranges700_global_table":      # more ranges than the kernel stages in LDS (512): the table is searched in global memory
        n = 8 * (2 ** 15 + 3)
        return n, _random_bounds(n, 700, 3), [r % 5 for r in range(700)], 5
    if name == "one_group":
        n = 8 * (2 ** 12 + 1)
        return n, [0, n], [0], 1
    if name == "second_grid_stride_trip":     # more 4-vectors than 32768 workgroups x 512: the loop's second trip, ragged
        n = 8 * (2 ** 23 + 2 ** 10 + 3)
        return n, _random_bounds(n, 12, 5), [r % 3 for r in range(12)], 3
    raise KeyError(name)


CASES = ["one_vector_pair", "block_edges", "ranges300_G2", "ranges300_G3", "ranges300_G8", "ranges700_global_table", "one_group",
         "second_grid_stride_trip"]


@pytest.mark.parametrize("gdtype", [torch.float32, BF], ids=["fp32grad", "bf16grad"])
@pytest.mark.parametrize("case", CASES)
def test_grouped_step_equals_one_parent_launch_per_range(dev, case, gdtype):
    n, bounds, groups, G = _case(case)
    assert bounds[0] == 0 and bounds[-1] == n and all(b % 8 == 0 for b in bounds) and len(groups) == len(bounds) - 1
    lrs, wds = _rates(G, tie_last_two=True)
    d_bounds = torch.tensor(bounds, dtype=torch.int64, device=dev)
    d_groups = torch.tensor(groups, dtype=torch.int32, device=dev)
    st0 = _state(n, dev, seed=n % 1000 + G, gdtype=gdtype)
    big = n > 2 ** 24
    # (sum of squares for the clip, step, write the bf16 copy): clip active and inactive, bias correction at step 1 and 7
    variants = [(1e4, 1, True), (1e-2, 7, False)] if big else \
        [(ss, step, pb) for ss in (1e4, 1e-2) for step in (1, 7) for pb in (True, False)]
    for ss, step, with_pb in variants:
        sumsq = torch.tensor([ss], dtype=torch.float32, device=dev)
        want, got = _clone(st0), _clone(st0)
        if case == "one_group":
            _parent(want, 0, n, lrs[0], wds[0], step, sumsq, with_pb)             # ONE whole-buffer parent call
        else:
            for r, grp in enumerate(groups):
                _parent(want, bounds[r], bounds[r + 1], lrs[grp], wds[grp], step, sumsq, with_pb)
        _grouped(got, n, d_bounds, d_groups, lrs, wds, step, sumsq, with_pb)
        torch.cuda.synchronize()
        for k in ("p", "m", "v", "pb", "g"):
            assert torch.equal(got[k], want[k]), (case, k, ss, step, with_pb, int((got[k] != want[k]).sum()))
            assert torch.equal(got[k][n:], st0[k][n:]), (case, k, "wrote behind the end")
        assert not torch.equal(got["p"][:n], st0["p"][:n])
        assert torch.equal(got["pb"], st0["pb"]) == (not with_pb)
        del want, got


def test_groups_actually_differ(dev):
    """The reference above would also pass if every group used group 0's rates in both paths - it does not: with lr 0 and
    weight_decay 0 a group's masters stay put while its moments move, and the other group's masters move."""
    n = 8 * 600
    bounds = torch.tensor([0, 8 * 100, 8 * 350, n], dtype=torch.int64, device=dev)
    groups = torch.tensor([0, 1, 0], dtype=torch.int32, device=dev)
    st0 = _state(n, dev, seed=1, gdtype=torch.float32)
    got = _clone(st0)
    _grouped(got, n, bounds, groups, [1e-3, 0.0], [1e-2, 0.0], 1, torch.tensor([1e-2], device=dev), True)
    torch.cuda.synchronize()
    frozen = slice(8 * 100, 8 * 350)
    assert torch.equal(got["p"][frozen], st0["p"][frozen]) and not torch.equal(got["m"][frozen], st0["m"][frozen])
    assert bool((got["p"][:8 * 100] != st0["p"][:8 * 100]).all()) and bool((got["p"][8 * 350:n] != st0["p"][8 * 350:n]).all())


def test_bad_arguments_are_refused_before_any_launch(dev):
    from phantom_vlb_amd._lib import VlbError
    n = 64
    st = _state(n, dev, seed=2, gdtype=torch.float32)
    before = _clone(st)
    bounds = torch.tensor([0, n], dtype=torch.int64, device=dev)
    groups = torch.zeros(1, dtype=torch.int32, device=dev)
    ss = torch.zeros(1, device=dev)
    with pytest.raises(VlbError):
        _grouped(st, n, bounds, groups, [1e-3] * 9, [0.0] * 9, 1, ss, True)            # more than 8 groups
    with pytest.raises(VlbError):
        _grouped(st, n - 4, bounds, groups, [1e-3], [0.0], 1, ss, True)                # n is no multiple of 8
    with pytest.raises(VlbError):
        _grouped(st, n, bounds, groups, [1e-3], [0.0], 0, ss, True)                    # steps count from 1
    with pytest.raises(VlbError):
        _grouped(st, 8, bounds, torch.zeros(2, dtype=torch.int32, device=dev), [1e-3], [0.0], 1, ss, True)   # more ranges than 8-element units
    torch.cuda.synchronize()
    assert all(torch.equal(st[k], before[k]) for k in st)
