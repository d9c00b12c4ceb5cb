"""The correlation objectives of the brain head (loss="cosine" / "pearson") on the CPU: the fp64 restatement of
tests/head_loss_emul.py is the objective (fp64 torch autograd through F.cosine_similarity), its bars accept an honest fp32
computation at every shape the GPU tests use and reject every planted bug, the number formats leave room under the
end-to-end bars, the config validates, and the three new entry points are declared, bound and exported."""
import pathlib
import re

import pytest
import torch
import torch.nn.functional as F

import head_emul as H
import head_loss_emul as L

ROOT = pathlib.Path(__file__).resolve().parent.parent


# ---------------------------------------------------------------------------------------------------- against autograd
def _autograd(p, y, loss, loss_scale):
    p = p.clone().requires_grad_(True)
    if loss == "pearson":
        val = 1 - F.cosine_similarity(p - p.mean(-1, keepdim=True), y - y.mean(-1, keepdim=True), dim=-1).mean()
    else:
        val = 1 - F.cosine_similarity(p, y, dim=-1).mean()
    (loss_scale * val).backward()
    return val.detach(), p.grad


def _rows(kind, B, V):
    gen = torch.Generator().manual_seed(11 + V)
    p, y = torch.randn(B, V, generator=gen, dtype=torch.float64), torch.randn(B, V, generator=gen, dtype=torch.float64)
    if kind == "zero_target":
        y[1] = 0
    elif kind == "tiny_pred":
        p[0] *= 1e-10                        # |p| ~ 1e-10 * sqrt(V): below the 1e-8 clamp, the norm is a constant
    elif kind == "offset":
        p, y = p + 50, y + 50
    return p, y


_ROWS = [("plain", 7, 1.0), ("plain", 300, 0.125), ("zero_target", 7, 1.0), ("tiny_pred", 7, 0.5), ("offset", 33, 1.0),
         ("plain", 1, 1.0), ("plain", 2, 0.25)]


@pytest.mark.parametrize("loss,kind,V,scale", [(k,) + r for k in L.LOSSES for r in _ROWS if not (k == "pearson" and r[1] == 1)])
def test_closed_form_equals_fp64_autograd(loss, kind, V, scale):
    p, y = _rows(kind, 3, V)
    val, dp = L.objective(p, y, loss, loss_scale=scale)
    ref_val, ref_dp = _autograd(p, y, loss, scale)
    assert torch.isfinite(dp).all() and torch.isfinite(val)
    assert abs(float(val - ref_val)) <= 1e-12, float(val - ref_val)
    if kind == "tiny_pred" and loss == "cosine":
        assert float(p[0].norm()) < L.CLAMP and bool((dp[0] != 0).any())
    tol = 1e-12 * max(1.0, float(ref_dp.abs().max()))
    assert float((dp - ref_dp).abs().max()) <= tol, float((dp - ref_dp).abs().max())
    if kind == "zero_target":
        assert bool((dp[1] == 0).all()) and float(L.rowstat(p, y, loss)["c"][1]) == 0.0
    if loss == "pearson":                    # both terms sum to zero over v: no further mean subtraction
        assert float(dp.sum(1).abs().max()) <= 1e-12 * max(1.0, float(dp.abs().max()) * V)


# ---------------------------------------------------------------------------------------------------- cases
def test_cases_cover_the_issue():
    ids = [c["id"] for c in L.CASES]
    assert len(set(ids)) == len(ids) and not set(ids) & set(H.BY_ID)
    for c in L.CASES:
        assert set(c["expect"]) <= H.dispatch(c["B"], c["E"]), c["id"]
        assert "pearson" not in c["losses"] or c["V"] >= 2
    assert {c["B"] for c in L.CASES} >= {1, 3, 8, 9, 16, 17} and {c["E"] for c in L.CASES} == {264, 1024}
    assert {c["V"] for c in L.CASES} >= {1, 2, 17, 300, 32784} and all(c["S"] == 33 for c in L.CASES if c["lens"] is None)
    reached = set().union(*(H.dispatch(c["B"], c["E"]) for c in L.CASES))
    assert {"ridge_fwd_kernel", "ridge_fwd_mfma_kernel<8>", "ridge_bwd_z_kernel", "wgrad_mfma_kernel", "ridge_bwd_w:b0_passes=1",
            "ridge_bwd_w:b0_passes=2", "ridge_bwd_w:b0_passes=3"} <= reached
    assert any(c["drop"] and c["scales"] != (1.0, 1.0) for c in L.CASES) and any(c["lens"] for c in L.CASES)
    inp = L.inputs_for("loss-zero-target", "cosine")
    assert bool((inp["y"][1] == 0).all()) and bool((inp["y"][0] != 0).any())
    inp = L.inputs_for("loss-offset50", "pearson")
    pred = L.whole(inp)["pred"]
    for rows in (pred, inp["y"].double()):
        assert float((rows.mean(1) - 50).abs().max()) < 1.0 and 0.5 < float(rows.std(1).min()) and float(rows.std(1).max()) < 2.0
    # rows of pred that start off a 16-byte boundary, and rows long enough for more than one f32x4 per thread
    assert any(c["V"] % 4 for c in L.CASES) and L.rowstat_chain(32784) > L.rowstat_chain(17)


# ---------------------------------------------------------------------------------------------------- bars accept fp32
@pytest.mark.parametrize("cid,loss", L.PAIRS)
def test_bars_accept_an_honest_fp32_computation(cid, loss):
    """every stage in plain fp32 torch (torch's summation order, not the kernels'), chained as on the device, stays
    within its bar when judged the way the GPU test judges the kernels"""
    inp = L.inputs_for(cid, loss)
    bufs = L.run(inp, dt=H.F32, device_like=True)
    ratios = {**L.check_stages(bufs, inp), **L.check_rest(bufs, inp)}
    print(cid, loss, {k: round(v, 3) for k, v in H.by_stage(ratios).items()})
    assert all(v <= 1.0 for v in ratios.values()), {k: v for k, v in ratios.items() if not v <= 1.0}
    e2e = L.end_to_end(bufs, inp)
    assert all(v < H.E2E_BARS[k] for k, v in e2e.items()), e2e


@pytest.mark.parametrize("cid,loss", L.PAIRS)
def test_number_formats_leave_room_under_the_end_to_end_bars(cid, loss):
    """fp64 arithmetic with only the device's bf16 roundings (z, d pred on the B <= 16 route, d hidden) stays within
    E2E_FORMAT_SHARE of every end-to-end bar at the chosen draw; RESEED names the first draw that does"""
    dev = L.format_deviation(L.inputs_for(cid, loss))
    print(cid, loss, {k: f"{v:.1e}" for k, v in dev.items()})
    assert all(v <= H.E2E_FORMAT_SHARE * H.E2E_BARS[k] for k, v in dev.items()), dev
    for n in range(L.RESEED.get((cid, loss), 0)):
        dev = L.format_deviation(L.make_inputs(L.BY_ID[cid], loss, reseed=n))
        assert any(v > H.E2E_FORMAT_SHARE * H.E2E_BARS[k] for k, v in dev.items()), (cid, loss, n)


# ---------------------------------------------------------------------------------------------------- bars reject bugs
BUG_CASES = {
    "no_centre": (("loss-offset50", "pearson"), ("loss-B3", "pearson"), ("loss-V32784", "pearson"), ("loss-V2-B17", "pearson")),
    "centre_p_only": (("loss-offset50", "pearson"), ("loss-B17", "pearson"), ("loss-V2", "pearson")),
    "no_inv_b": (("loss-B3", "cosine"), ("loss-B17", "pearson"), ("loss-V32784", "pearson")),
    "no_inv_b_grad": (("loss-B3", "cosine"), ("loss-B17", "pearson"), ("loss-E264", "pearson")),
    "drop_a": (("loss-B1", "cosine"), ("loss-B9", "pearson"), ("loss-B17", "cosine"), ("loss-offset50", "pearson"),
               ("loss-E264-B17-V300", "pearson")),
    "sign_b": (("loss-B1", "pearson"), ("loss-B16", "cosine"), ("loss-B17", "pearson"), ("loss-V32784", "cosine")),
    "unclamped": (("loss-zero-target", "cosine"), ("loss-zero-target", "pearson")),
    "scale_twice": (("loss-scales", "cosine"), ("loss-scales", "pearson"), ("loss-scales-B17", "pearson")),
}


def test_every_planted_bug_has_cases():
    assert set(BUG_CASES) == set(L.BUGS)


@pytest.mark.parametrize("bug,cid,loss", [(b, c, k) for b, cs in BUG_CASES.items() for c, k in cs])
def test_bars_reject_planted_bug(bug, cid, loss):
    inp = L.inputs_for(cid, loss)
    bufs = L.run(inp, dt=H.F32, device_like=True, bug=bug)
    stages = (L.BUGS[bug],) + (("dz",) if bug in L.DZ_BUGS else ())
    worst = H.by_stage(L.check_stages(bufs, inp, stages))
    print(bug, cid, loss, worst)
    assert all(worst[s] > 1.0 for s in stages), (bug, cid, loss, worst)


# ---------------------------------------------------------------------------------------------------- config
def _cfg(**kw):
    from phantom_vlb_amd.litmodule import VLBLitModuleConfig
    base = dict(model_path="none", freeze_backbone=True, use_lora=False, lora_r=None, lora_alpha=None, lora_dropout=None,
                dropout_rate=0.0, num_target=16, l2_lambda=1e-3, lr=1e-3, betas=[0.9, 0.999], eps=1e-8, weight_decay=1e-2,
                lr_scheduler_name="CosineAnnealingLR", last_epoch=-1, t_max=100, geometry="mini")
    base.update(kw)
    return VLBLitModuleConfig(**base)


def test_config_validates_the_objective():
    assert _cfg().loss == "mse"
    assert _cfg(loss="cosine").loss == "cosine" and _cfg(loss="pearson").loss == "pearson"
    assert _cfg(loss="cosine", num_target=1).loss == "cosine"
    for bad in ("MSE", "corr", "", None):
        with pytest.raises(ValueError, match="loss"):
            _cfg(loss=bad)
    with pytest.raises(ValueError, match="pearson"):
        _cfg(loss="pearson", num_target=1)


def test_objective_is_reachable_from_the_command_line():
    from phantom_vlb_amd.config import instantiate, load_config
    cfg = load_config(str(ROOT / "config"), ["experiment=VLB_mini_synthetic", "litmodule.config.loss=cosine"])
    assert instantiate(cfg["litmodule"]["config"]).loss == "cosine"
    cfg = load_config(str(ROOT / "config"), ["experiment=VLB_mini_synthetic"])
    assert instantiate(cfg["litmodule"]["config"]).loss == "mse"


# ---------------------------------------------------------------------------------------------------- C-ABI
NEW = ("vlb_head_loss_fwd", "vlb_head_bwd_loss", "vlb_head_bwd_cached_loss")


def test_entry_points_are_declared_bound_and_exported():
    from phantom_vlb_amd import _lib
    header = (ROOT / "include" / "vlb.h").read_text()
    assert re.search(r"#define VLB_ABI_VERSION 2\b", header) and _lib.lib.vlb_abi_version() == 2
    flat = re.sub(r"\s+", " ", header)
    for name in NEW:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/ int " + name + r"\(([^)]*)\);", flat)
        assert m, f"{name} is not declared behind a comment"
        assert "290-301" in m.group(1), f"{name}: the comment does not cite the reference's docstring"
        assert len(m.group(2).split(",")) == len(_lib.SIGNATURES[name]), name
        assert getattr(_lib.lib, name) is not None
    # the *_loss backward entry points take their MSE sibling's list plus (loss_kind, rowstat)
    assert _lib.SIGNATURES["vlb_head_bwd_loss"] == _lib.SIGNATURES["vlb_head_bwd"] + [_lib.I, _lib.P]
    assert _lib.SIGNATURES["vlb_head_bwd_cached_loss"] == _lib.SIGNATURES["vlb_head_bwd_cached"] + [_lib.I, _lib.P]
    for old in ("vlb_head_fwd", "vlb_head_bwd", "vlb_head_fwd_cached", "vlb_head_bwd_cached"):
        assert old in _lib.SIGNATURES
    from phantom_vlb_amd.head import LOSS_KINDS
    for name, k in LOSS_KINDS.items():
        assert re.search(rf"#define VLB_LOSS_{name.upper()} {k}\b", header)


def test_workspace_only_grows():
    """vlb_head_ws_floats: never below what the MSE path needed, and room for 4 coefficients per clip behind the backward's"""
    from phantom_vlb_amd._lib import lib
    for B, S, E, V in ((1, 1, 8, 1), (3, 33, 1024, 17), (17, 33, 1024, 300), (3, 2048, 4096, 2048), (2, 33, 264, 32784)):
        pool = B * H.cdiv(S, 32) * (E + 2) + 2 * H.cdiv(V, 16)
        bwd = max(32 * B * E, H.wgrad_splits(V) * 16 * E + 16 * E + (V * 16 + 1) // 2 + 64)
        assert lib.vlb_head_ws_floats(B, S, E, V) == max(pool, bwd + 4 * B) >= max(pool, bwd)
