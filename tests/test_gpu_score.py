"""The held-out scoring kernels alone (phantom_vlb_amd/csrc/score.hip) against tests/score_emul.py: seeded
inputs, fp32 values rounded to bf16 like real ``pred`` / ``y``.

vlb_score_accumulate is held to the emulation bit for bit (the products of widened fp32 values are exact and the order of the
additions is fixed).  vlb_score_finish and vlb_score_bootstrap are held to bars derived in score_emul.py from the rounded
operations of the code (k stated there, not fitted); each test prints max(err / bar) before it asserts <= 1.

The p-value's count is compared exactly.  Its precondition is checked on the emulation alone: |r*| >= 1e-9 at every kept
(rho, v) whose variances are not exactly zero; the constant columns of a case have vp or vy == 0 exactly on both sides (sums of
one bf16 value are exact), so their r* = 0 comes from the branch and not from rounding, and they are compared too."""
import ctypes

import numpy as np
import pytest
import torch

import score_emul as E

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _pitched(a, pad, dev, fill=7.0):
    """device fp32 [B,V] view with row pitch V + pad (the padding holds ``fill``, which must never be read)"""
    B, V = a.shape
    big = torch.full((B, V + pad), fill, dtype=torch.float32, device=dev)
    big[:, :V] = torch.from_numpy(a).to(dev)
    return big[:, :V]


def gpu_accumulate(sums, pred, y, slot, keep, nb, dev, pads=(3, 8)):
    from phantom_vlb_amd._lib import check, lib
    n_slots, _, V = sums.shape
    assert min(slot) >= 0 and max(slot) < n_slots           # the caller's check, on the host
    p, t = _pitched(pred, pads[0], dev), _pitched(y, pads[1], dev, fill=float("nan"))
    s = torch.tensor(list(slot), dtype=torch.int32).to(dev)
    k = None if keep is None else torch.from_numpy(keep).to(dev).contiguous()
    check(lib.vlb_score_accumulate(p.data_ptr(), p.stride(0), t.data_ptr(), t.stride(0), s.data_ptr(), None if k is None else k.data_ptr(),
                                   sums.data_ptr(), len(slot), V, nb, n_slots, torch.cuda.current_stream().cuda_stream), "accumulate")
    torch.cuda.synchronize()


def _rows(rng, B, V):
    y = rng.randn(B, V)
    p = 0.5 * y + rng.randn(B, V) + 0.25
    return E.bf16_round(p.astype(np.float32)), E.bf16_round(y.astype(np.float32))


@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("V", [1, 5, 63, 64, 65, 300, 1000])
def test_accumulate_is_bit_exact(dev, V, H):
    nb = 3
    heads = [0] if H == 1 else [0, 2]                        # with three heads, head 1 never appears
    for B in (1, 3, 17):
        rng = np.random.RandomState(1000 * V + 10 * B + H)
        p, y = _rows(rng, B, V)
        # several clips in one slot, slots out of order within the batch
        slot = [int(rng.choice(heads)) * nb + int(rng.randint(0, nb)) for _ in range(B)]
        if B >= 3:
            slot[0], slot[1], slot[2] = heads[-1] * nb + 2, heads[0] * nb, heads[-1] * nb + 2
        ref = E.accumulate(np.zeros((H * nb, 5, V)), p, y, slot, None, nb)
        one = torch.zeros(H * nb, 5, V, dtype=torch.float64, device=dev)
        gpu_accumulate(one, p, y, slot, None, nb, dev)
        assert np.array_equal(_bits(one.cpu().numpy()), _bits(ref)), (V, B, H)
        if H == 3:
            assert not one[nb:2 * nb].any()
        if B >= 2:                                           # two successive calls equal one call on the concatenation
            two = torch.zeros_like(one)
            cut = B // 2
            gpu_accumulate(two, p[:cut], y[:cut], slot[:cut], None, nb, dev)
            gpu_accumulate(two, p[cut:], y[cut:], slot[cut:], None, nb, dev)
            assert np.array_equal(_bits(two.cpu().numpy()), _bits(ref)), (V, B, H)


@pytest.mark.parametrize("V,H", [(5, 1), (65, 3), (300, 3)])
def test_accumulate_mask_is_a_select(dev, V, H):
    nb, B = 2, 9
    rng = np.random.RandomState(V + H)
    p, y = _rows(rng, B, V)
    slot = [int(rng.randint(0, H)) * nb + int(rng.randint(0, nb)) for _ in range(B)]
    keep = (rng.rand(H, V) < 0.6).astype(np.float32) * rng.choice([0.5, 1.0, 3.0], size=(H, V)).astype(np.float32)
    keep[:, 0] = 0.0
    ref = E.accumulate(np.zeros((H * nb, 5, V)), p, y, slot, keep, nb)
    bad_p, bad_y = p.copy(), y.copy()
    for b in range(B):                                       # NaN / Inf wherever the clip's head masks the target
        m = keep[slot[b] // nb] <= 0
        bad_p[b, m] = np.where(np.arange(m.sum()) % 2 == 0, np.nan, np.inf)
        bad_y[b, m] = np.where(np.arange(m.sum()) % 2 == 0, -np.inf, np.nan)
    got = torch.zeros(H * nb, 5, V, dtype=torch.float64, device=dev)
    gpu_accumulate(got, bad_p, bad_y, slot, keep, nb, dev)
    got = got.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(ref))            # the kept columns keep their bits ...
    for s in range(H * nb):
        m = keep[s // nb] <= 0
        assert (_bits(got[s][:, m]) == 0).all()               # ... and the masked sums stay +0.0


# ---------------------------------------------------------------------------------------------------- finish and bootstrap
CASES = {nb: E.make_case(seed=20 + nb, n_clips=4 * nb - 1, V=300, block=4, const_y=(3, 299), const_p=(7, 64), masked=(0, 9, 255, 256))
         for nb in (1, 2, 7)}


def _ratio(err, bar):
    with np.errstate(all="ignore"):
        return np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err == 0, 0.0, np.inf))


def gpu_finish(c, dev, masked=True):
    from phantom_vlb_amd._lib import check, lib
    nb, _, V = c["sums"].shape
    s, n = torch.from_numpy(c["sums"]).to(dev), torch.from_numpy(c["n_j"]).to(dev)
    k = torch.from_numpy(c["keep"][0]).to(dev) if masked else None
    out = torch.full((4, V), 5.0, dtype=torch.float64, device=dev)
    avg = torch.full((3,), 5.0, dtype=torch.float64, device=dev)
    check(lib.vlb_score_finish(s.data_ptr(), n.data_ptr(), nb, None if k is None else k.data_ptr(), out.data_ptr(), avg.data_ptr(), V,
                               torch.cuda.current_stream().cuda_stream), "finish")
    return out.cpu().numpy(), avg.cpu().numpy()


def gpu_bootstrap(c, draws, dev, masked=True):
    from phantom_vlb_amd._lib import check, lib
    nb, _, V = c["sums"].shape
    s, n = torch.from_numpy(c["sums"]).to(dev), torch.from_numpy(c["n_j"]).to(dev)
    assert draws.dtype == np.int32 and draws.min() >= 0 and draws.max() < nb           # the caller's check, on the host
    d = torch.from_numpy(draws).to(dev)
    k = torch.from_numpy(c["keep"][0]).to(dev) if masked else None
    out = torch.full((3, V), 5.0, dtype=torch.float64, device=dev)
    check(lib.vlb_score_bootstrap(s.data_ptr(), n.data_ptr(), nb, d.data_ptr(), draws.shape[0], None if k is None else k.data_ptr(),
                                  out.data_ptr(), V, torch.cuda.current_stream().cuda_stream), "bootstrap")
    return out.cpu().numpy()


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("nb", [1, 2, 7])
def test_finish_within_the_derived_bars(dev, nb, masked):
    c = CASES[nb]
    keep = c["keep"][0] if masked else None
    ref, ref_avg = E.finish(c["sums"], c["n_j"], keep)
    bars = E.finish_bars(c["sums"], c["n_j"])
    got, avg = gpu_finish(c, dev, masked)
    kept = np.ones(300, bool) if keep is None else keep > 0
    assert np.isfinite(bars[:, kept]).all()
    worst = float(_ratio(np.abs(got[:3] - ref[:3])[:, kept], bars[:, kept]).max())
    print(f"finish nb={nb} masked={masked}: max(err / bar) = {worst:.3g}")
    assert worst <= 1
    assert np.array_equal(got[3], ref[3]) and (got[3] == 4 * nb - 1).all()
    assert np.isnan(got[:3, ~kept]).all()                                             # masked targets: NaN out
    for v in (3, 299):                                                                # a constant target: r = 0 and R^2 = 0
        assert got[0, v] == 0 and got[1, v] == 0
    for v in (7, 64):                                                                 # a constant prediction: r = 0
        assert got[0, v] == 0
    # the averages: the kept targets' bars, averaged (the additions of at most 300 terms of size <= max|x| add 300 u max|x| per side)
    abar = bars[:, kept].mean(1) + 2 * 300 * E.U * np.abs(ref[:3, kept]).max(1)
    aworst = float(_ratio(np.abs(avg - ref_avg), abar).max())
    print(f"finish nb={nb} masked={masked}: avg max(err / bar) = {aworst:.3g}")
    assert aworst <= 1
    again, avg2 = gpu_finish(c, dev, masked)                                          # a repeated call gives the same bits
    assert np.array_equal(_bits(again[:, kept]), _bits(got[:, kept])) and np.array_equal(_bits(avg2), _bits(avg))


@pytest.mark.parametrize("R", [2, 64])
@pytest.mark.parametrize("nb", [1, 2, 7])
def test_bootstrap_within_the_derived_bars(dev, nb, R):
    from phantom_vlb_amd.evaluate import bootstrap_draws
    c = CASES[nb]
    keep = c["keep"][0]
    kept = keep > 0
    draws = bootstrap_draws(nb + R, 0, nb, R)
    ref, rs, parts = E.bootstrap(c["sums"], c["n_j"], draws, keep)
    # the precondition of the exact count, on the emulation alone
    degenerate = np.stack([(vp == 0) | (vy == 0) for _, vp, vy, _, _ in parts])
    assert degenerate[:, [3, 299, 7, 64]].all() and (rs[degenerate] == 0).all()
    live = kept[None, :] & ~degenerate
    assert live[:, kept & ~np.isin(np.arange(300), [3, 299, 7, 64])].all()
    assert np.abs(rs[live]).min() >= 1e-9
    bars = E.bootstrap_bars(rs, parts)
    got = gpu_bootstrap(c, draws, dev)
    worst = float(_ratio(np.abs(got[:2] - ref[:2])[:, kept], bars[:, kept]).max())
    print(f"bootstrap nb={nb} R={R}: max(err / bar) = {worst:.3g}")
    assert worst <= 1
    assert np.array_equal(got[2, kept] * (R + 1), ref[2, kept] * (R + 1))              # the count, exactly
    assert np.array_equal(_bits(got[2, kept]), _bits(ref[2, kept]))
    assert np.isnan(got[:, ~kept]).all()
    if nb == 1:
        assert (got[1, kept] == 0).all()                                              # one block: sd exactly 0
    else:
        assert (got[1, kept & ~degenerate.any(0)] > 0).all()
    again = gpu_bootstrap(c, draws, dev)
    assert np.array_equal(_bits(again[:, kept]), _bits(got[:, kept]))
    unmasked = gpu_bootstrap(c, draws, dev, masked=False)                             # without a mask every target is scored
    assert np.isfinite(unmasked).all() and np.array_equal(_bits(unmasked[:, kept]), _bits(got[:, kept]))


def test_refusals_launch_nothing(dev):
    from phantom_vlb_amd._lib import lib
    st = torch.cuda.current_stream().cuda_stream
    V = 8
    sums = torch.full((4, 5, V), 3.0, dtype=torch.float64, device=dev)
    x = torch.ones(2, V, device=dev)
    slot = torch.zeros(2, dtype=torch.int32, device=dev)
    n = torch.ones(4, dtype=torch.float64, device=dev)
    out = torch.full((4, V), 3.0, dtype=torch.float64, device=dev)
    avg = torch.full((3,), 3.0, dtype=torch.float64, device=dev)
    draws = torch.zeros(2, 4, dtype=torch.int32, device=dev)
    P = lambda t: t.data_ptr()       # noqa: E731
    bad = [
        (lib.vlb_score_accumulate, (None, V, P(x), V, P(slot), None, P(sums), 2, V, 2, 4, st), b"null"),
        (lib.vlb_score_accumulate, (P(x), V, P(x), V, P(slot), None, P(sums), 0, V, 2, 4, st), b"B=0"),
        (lib.vlb_score_accumulate, (P(x), V, P(x), V, P(slot), None, P(sums), 2, 0, 2, 4, st), b"V=0"),
        (lib.vlb_score_accumulate, (P(x), V, P(x), V, P(slot), None, P(sums), 2, V, 0, 4, st), b"nb=0"),
        (lib.vlb_score_accumulate, (P(x), V, P(x), V, P(slot), None, P(sums), 2, V, 3, 4, st), b"n_slots=4"),
        (lib.vlb_score_finish, (P(sums), P(n), 0, None, P(out), P(avg), V, st), b"nb=0"),
        (lib.vlb_score_finish, (P(sums), None, 4, None, P(out), P(avg), V, st), b"null"),
        (lib.vlb_score_bootstrap, (P(sums), P(n), 4, P(draws), 1, None, P(out), V, st), b"R=1"),
        (lib.vlb_score_bootstrap, (P(sums), P(n), 0, P(draws), 2, None, P(out), V, st), b"nb=0"),
        (lib.vlb_score_bootstrap, (P(sums), P(n), 4, None, 2, None, P(out), V, st), b"null"),
    ]
    for fn, args, msg in bad:
        assert fn(*args) == -1 and msg in lib.vlb_last_error(), (fn.__name__, lib.vlb_last_error())
    torch.cuda.synchronize()
    assert (sums == 3).all() and (out == 3).all() and (avg == 3).all()
