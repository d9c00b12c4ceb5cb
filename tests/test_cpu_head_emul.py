"""The brain head's staged fp64 reference (tests/head_emul.py) checked on the CPU: it is the head (fp64 autograd through
the oracle), its bars accept an honest fp32 computation at every shape the GPU tests use, and reject every planted bug."""
import pytest
import torch
import torch.nn.functional as F

import head_emul as H

ALL = H.CASES + H.KSWEEP


# ---------------------------------------------------------------------------------------------------- against autograd
@pytest.mark.parametrize("drop,zero_clip,scales", [(False, False, (1.0, 1.0)), (True, False, (1.0, 1.0)),
                                                   (False, True, (1.0, 1.0)), (True, True, (0.25, 0.5))])
def test_whole_equals_fp64_autograd(drop, zero_clip, scales):
    import vlb_oracle as O
    E, S, B, V, p_drop = 40, 13, 3, 7, 0.1
    case = H._case("small", E, S, B, V, drop=drop, zero_clip=zero_clip, scales=scales)
    inp = H.make_inputs(case, seed=5)
    assert bool((inp["wmask"] > 0).any()) and bool((inp["wmask"] < 0).any())          # weights of both signs
    assert not zero_clip or bool((inp["wmask"][1] == 0).all())
    if drop:
        inp["keep"] = (inp["keep"] > 0).double() / (1.0 - p_drop)                       # 1/(1-p) in fp64, as the oracle forms it
    got = H.whole(inp)
    g = O.Geometry(dim=E, num_target=V, l2_lambda=inp["lam"], ln_eps=inp["eps"])
    pr = {k: v.double().requires_grad_(True) for k, v in inp["params"].items()}
    hr = inp["hidden"].double().requires_grad_(True)
    pred, l2, _ = O.brain_head(pr, hr, inp["wmask"].double(), g, keep_mask=(inp["keep"] > 0).double() if drop else None,
                               dropout_p=p_drop if drop else 0.0)
    mse = F.mse_loss(pred, inp["y"].double())
    (scales[0] * mse + scales[1] * l2).backward()

    def close(a, ref, what):
        err = float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300))
        assert err <= 1e-9, (what, err)
    close(got["pred"], pred.detach(), "pred")
    close(got["loss_terms"], torch.stack([mse, l2, mse + l2]).detach(), "loss terms")
    for name, key in H.GRAD_KEYS.items():
        close(got[key], pr[name].grad, name)
    close(got["dh"], hr.grad, "d hidden")
    assert bool((got["dh"][inp["wmask"] == 0] == 0).all())


# ---------------------------------------------------------------------------------------------------- cases and dispatch
def test_cases_cover_the_issue_and_name_reachable_kernels():
    ids = [c["id"] for c in ALL]
    assert len(set(ids)) == len(ids)
    for c in ALL:
        assert set(c["expect"]) <= H.dispatch(c["B"], c["E"]), c["id"]
        assert c["E"] % 8 == 0 and c["E"] <= 8192
    reached = set().union(*(H.dispatch(c["B"], c["E"]) for c in ALL))
    for ni in (1, 2, 4, 8, 16):
        assert f"head_pool_kernel<{ni}>" in reached
    for k in range(1, 33):
        assert f"ridge_fwd_mfma_kernel<{k}>" in reached
    assert {"ridge_fwd_kernel", "ridge_bwd_z_kernel", "head_dz_reduce_kernel", "ridge_bwd_w:b0_passes=4"} <= reached
    assert H.BY_ID["pool-E1536"]["E"] // 512 == 3 and H.pool_ni(1536) == 4                      # NI=4 serving ni=3
    assert -(-32784 // 16) == 2049 and H.wgrad_splits(32784) == 32 and H.wgrad_splits(300) == 2


def test_dispatch_restates_the_planner():
    """``dispatch`` is a restatement in Python; the library does not say which kernels it launched.  What can be held
    fast is the source: the branch conditions dispatch() copies are still the ones head.hip branches on."""
    import pathlib
    import re
    src = re.sub(r"\s+", " ", (pathlib.Path(__file__).resolve().parent.parent / "phantom_vlb_amd" / "csrc" / "head.hip").read_text())
    for cond in ("bool ridge_fwd_is_mfma(int B, int E) { return B <= 16 && E % 128 == 0 && E <= 4096; }",      # the one MFMA condition ...
                 "ridge_fwd_launch(ridge_w, ridge_b, z, y, group, pred, lpart, B, E, V, G, ridge_fwd_is_mfma(B, E), st);",   # ... head_fwd_tail asks
                 "if (mfma) {",                                           # ridge_fwd_launch_as: MFMA ridge, else ridge_fwd_kernel
                 "if (B <= 16 && E % 8 == 0) {",                          # ridge_bwd_launch: skinny wgrad, else ridge_bwd_z
                 "constexpr int BMAX = 8;", "for (int b0 = 0; b0 < B; b0 += BMAX) {",      # the b0 passes
                 "const int ni = (E + 511) / 512;",
                 "if (ni <= 1) rc = launch_pool<1>(", "else if (ni <= 2) rc = launch_pool<2>(",
                 "else if (ni <= 4) rc = launch_pool<4>(", "else if (ni <= 8) rc = launch_pool<8>(",
                 "else rc = launch_pool<16>("):
        assert cond in src, cond
    assert H.dispatch(16, 4096) >= {"ridge_fwd_mfma_kernel<32>", "wgrad_mfma_kernel"} and "ridge_fwd_kernel" in H.dispatch(16, 4104)
    assert H.dispatch(17, 1024) >= {"ridge_fwd_kernel", "ridge_bwd_z_kernel", "ridge_bwd_w:b0_passes=3"}


def test_every_live_subset_mask():
    assert H.wave_patterns(H.subsets_mask_live(128)) == set(range(16))
    inp = H.inputs_for("tok-S128")
    live = inp["wmask"] != 0
    assert H.wave_patterns(live[0]) == set(range(16)) and H.wave_patterns(live[2]) == set(range(16))
    assert not bool(live[1].any())                                                             # the all-zero clip
    for cid in ("tok-S1", "tok-S31", "tok-S32", "tok-S33"):                                    # ... in every S case
        w = H.inputs_for(cid)["wmask"]
        assert not bool(w[1].any()) and bool((w[0] != 0).any()) and bool((w[2] != 0).any()), cid
    packed = H.inputs_for("packed")["wmask"] != 0                                              # lens (70, 1, 37)
    assert packed[1].tolist() == [True] + [False] * 69                                         # the one-row clip is live
    assert not bool(packed[0, :23].any()) and not bool(packed[2, :12].any()) and not bool(packed[2, 37:].any())
    assert bool(packed[2, 12:37].all())
    lead = H.inputs_for("tok-S33")["wmask"]
    assert bool((lead[:, :11] == 0).all()) and bool((lead[0, 11:] < 0).any()) and bool((lead[0, 11:] > 0).any())
    keep = H.inputs_for("scales-mfma")["keep"]
    assert set(keep.unique().tolist()) == {0.0, float(torch.tensor(1.0) / torch.tensor(0.9))}


# ---------------------------------------------------------------------------------------------------- bars accept fp32
@pytest.mark.parametrize("cid", [c["id"] for c in ALL])
def test_bars_accept_an_honest_fp32_computation(cid):
    """every stage in plain fp32 torch (torch's summation order, not the kernels'), chained as on the device, stays
    within its bar when judged the way the GPU test judges the kernels"""
    inp = H.inputs_for(cid)
    bufs = H.run(inp, dt=H.F32, device_like=True)
    ratios = H.check_stages(bufs, inp, inp["case"]["stages"])
    worst = H.by_stage(ratios)
    print(cid, {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= 1.0 for v in ratios.values()), {k: v for k, v in ratios.items() if v > 1.0}
    if inp["case"]["stages"] == H.STAGES:            # the end-to-end bars the GPU test also applies
        e2e = H.end_to_end(bufs, inp)
        assert all(v < H.E2E_BARS[k] for k, v in e2e.items()), e2e


@pytest.mark.parametrize("cid", [c["id"] for c in H.CASES])
def test_number_formats_leave_room_under_the_end_to_end_bars(cid):
    """fp64 arithmetic with only the device's bf16 roundings stays within E2E_FORMAT_SHARE of every end-to-end bar, so the
    unwidened bars can be asked of the device at these inputs; RESEED names the first draw that does, nothing later"""
    case = H.BY_ID[cid]
    dev = H.format_deviation(H.inputs_for(cid))
    print(cid, {k: f"{v:.1e}" for k, v in dev.items()})
    assert all(v <= H.E2E_FORMAT_SHARE * H.E2E_BARS[k] for k, v in dev.items()), dev
    for n in range(case["reseed"]):                  # every earlier draw was passed over for a reason
        dev = H.format_deviation(H.make_inputs(dict(case, reseed=n)))
        assert any(v > H.E2E_FORMAT_SHARE * H.E2E_BARS[k] for k, v in dev.items()), (cid, n)


# ---------------------------------------------------------------------------------------------------- bars reject bugs
BUG_CASES = {
    "drop_token": ("pool-E264", "pool-E8192", "tok-S128", "packed"),
    "drop_chunk": ("pool-E264", "pool-E520", "pool-E8192"),
    "pool_no_eps": ("pool-E512", "pool-E8192"),
    "ln2_no_eps": ("pool-E512", "pool-E8192", "clips-B25"),
    "no_b1": ("pool-E1536", "tok-S1", "clips-B17"),
    "fwd_no_keep": ("clips-B17-drop", "scales-mfma"),
    "dz_no_keep": ("clips-B17-drop", "scales-mfma"),
    "lose_quarter": ("pool-E4096", "pool-E4104", "targets-V1", "ksteps-1", "ksteps-32"),
    "dbias_first8": ("clips-B9", "clips-B17", "clips-B25"),
    "no_l2_seed": ("clips-B1", "clips-B25", "scales-mfma", "targets-V32784"),
    "swap_scales": ("scales-mfma", "scales-B17"),
    # (not targets-V32784: a worst-case bar over a chain of 1025 + 32 additions is wider than the AVERAGE effect of 32784
    # independent roundings; the bug is pinned at the shapes where a split is short)
    "dz_unrounded": ("clips-B16", "targets-V1", "targets-V300", "ksteps-32"),
    "m2_no_rstd": ("pool-E264", "pool-E8192", "tok-S1"),
}


def test_every_planted_bug_has_cases():
    assert set(BUG_CASES) == set(H.BUGS)


@pytest.mark.parametrize("bug,cid", [(b, c) for b, cs in BUG_CASES.items() for c in cs])
def test_bars_reject_planted_bug(bug, cid):
    inp = H.inputs_for(cid)
    stage = H.BUGS[bug]
    stages = (stage,)
    bufs = H.run(inp, dt=H.F32, device_like=True, bug=bug)
    worst = H.by_stage(H.check_stages(bufs, inp, stages))[stage]
    print(bug, cid, stage, worst)
    assert worst > 1.0, (bug, cid, worst)
