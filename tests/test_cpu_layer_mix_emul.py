"""The fp64 restatement of the layer-mix stages (layer_mix_emul.py): its backward against torch autograd, its bars against
an honest fp32 computation (they must hold) and against the planted bugs (each must break its bar).  No GPU."""
import pytest
import torch

import head_emul as H
import layer_mix_emul as M
from layer_mix_emul import BF16, F32, F64


def _pooled(x, w, eps):
    """sum_s w_s LN(x_s) without affine, differentiable: P of one tap"""
    E = x.shape[-1]
    return (w[..., None] * torch.nn.functional.layer_norm(x, (E,), eps=eps)).sum(1)


def test_analytic_backward_equals_autograd():
    """mix_bwd + dhidden (write for the highest tap, accumulate below) == autograd of  sum(c * sum_k softmax(a)_k P_k(x_k))
    wrt a and every tapped hidden tensor, in fp64 to 1e-12 relative.  The lower tap's gradient is added to a stream
    gradient dx0, as in the decoder's backward."""
    inp = M.dh_inputs(E=64, B=2, S=9)
    K = 2
    x = [h.to(F64).requires_grad_(True) for h in inp["hidden"]]
    w = inp["wmask"].to(F64)
    a = torch.tensor([0.75, -1.25], dtype=F64, requires_grad=True)
    c = inp["draw"][0].to(F64)                        # d loss / d pooled, a constant
    P = torch.stack([_pooled(xk, w, inp["eps"]) for xk in x])
    (torch.softmax(a, 0)[:, None, None] * P).sum(0).mul(c).sum().backward()
    mb = M.mix_bwd(P.detach(), c, torch.softmax(a.detach(), 0))
    assert (mb["d_a"] - a.grad).abs().max() <= 1e-12 * a.grad.abs().max()
    live = (inp["wmask"] != 0)[..., None]
    for k in range(K):
        mu, rstd = M.stats_of(inp["hidden"][k], inp["eps"])
        got = M.dhidden_write(inp["hidden"][k], inp["wmask"], mu, rstd, mb["draw_stack"][k])["dh"]
        assert (got - x[k].grad).abs().max() <= 1e-12 * x[k].grad.abs().max()
        assert float(x[k].grad.masked_select(~live.expand_as(got)).abs().max()) == 0.0       # zero weight: no gradient
    mu, rstd = M.stats_of(inp["hidden"][0], inp["eps"])
    acc = M.dhidden_acc(inp["dx0"], inp["hidden"][0], inp["wmask"], mu, rstd, mb["draw_stack"][0])["dx"]
    want = inp["dx0"].to(F64) + x[0].grad
    assert (acc - want).abs().max() <= 1e-12 * want.abs().max()


@pytest.mark.parametrize("K,B,E", [(1, 1, 264), (2, 3, 512), (5, 3, 4104)])
def test_bars_hold_for_an_honest_fp32_mix(K, B, E):
    """fp32 in torch's own order sits inside the bars (they are not too tight); K = 1 is a bit copy."""
    inp = M.mix_inputs(K, B, E)
    ref = M.mix_fwd(inp["P"], inp["a"])
    got = M.mix_fwd(inp["P"], inp["a"], dt=F32)
    bars = M.mix_fwd_bars(ref, inp["P"], inp["a"])
    assert M.ratio(got["alpha"], ref["alpha"], bars["alpha"]) <= 1 and M.ratio(got["pooled"], ref["pooled"], bars["pooled"]) <= 1
    if K == 1:
        assert torch.equal(got["pooled"], inp["P"][0])
    al = got["alpha"]
    refb = M.mix_bwd(inp["P"], inp["draw"], al)
    gotb = M.mix_bwd(inp["P"], inp["draw"], al, dt=F32)
    barb = M.mix_bwd_bars(refb, al, B, E)
    assert M.ratio(gotb["d_a"], refb["d_a"], barb["d_a"]) <= 1
    assert M.ratio(gotb["draw_stack"], refb["draw_stack"], barb["draw_stack"]) <= 1
    exact = M.mix_bwd(inp["P"], inp["draw"], ref["alpha"])["d_a"]          # with an alpha that sums to 1 (fp64) ...
    assert abs(float(exact.sum())) <= 1e-12 * float(exact.abs().sum() + 1e-300)     # ... the logits' gradient sums to 0


def test_bars_hold_for_an_honest_fp32_dhidden():
    inp = M.dh_inputs()
    x, w = inp["hidden"][0], inp["wmask"]
    mu, rstd = (t.float() for t in M.stats_of(x, inp["eps"]))
    ref = M.dhidden_acc(inp["dx0"], x, w, mu, rstd, inp["draw"][0])
    got = M.dhidden_acc(inp["dx0"], x, w, mu, rstd, inp["draw"][0], dt=F32)["dx"].to(BF16)
    assert M.ratio(got, ref["dx"], M.dhidden_acc_bars(ref, inp["E"])) <= 1
    dead = (w == 0)
    assert dead[1].all() and torch.equal(got[dead], inp["dx0"][dead])


def test_planted_bugs_break_their_bars():
    assert set(M.BUGS) == {"swap_alpha", "no_jacobian_sum", "overwrite", "touch_dead", "wrong_tap_stats"}
    inp = M.mix_inputs(5, 3, 512)
    ref = M.mix_fwd(inp["P"], inp["a"])
    bars = M.mix_fwd_bars(ref, inp["P"], inp["a"])
    assert M.ratio(M.mix_fwd(inp["P"], inp["a"], bug="swap_alpha")["pooled"], ref["pooled"], bars["pooled"]) > 1
    refb = M.mix_bwd(inp["P"], inp["draw"], ref["alpha"])
    barb = M.mix_bwd_bars(refb, ref["alpha"], 3, 512)
    assert M.ratio(M.mix_bwd(inp["P"], inp["draw"], ref["alpha"], bug="no_jacobian_sum")["d_a"], refb["d_a"], barb["d_a"]) > 1
    d = M.dh_inputs()
    x, w = d["hidden"][0], d["wmask"]
    mu, rstd = M.stats_of(x, d["eps"])
    ra = M.dhidden_acc(d["dx0"], x, w, mu, rstd, d["draw"][0])
    ba = M.dhidden_acc_bars(ra, d["E"])
    assert M.ratio(M.dhidden_acc(d["dx0"], x, w, mu, rstd, d["draw"][0], bug="overwrite")["dx"].to(BF16), ra["dx"], ba) > 1
    touched = M.dhidden_acc(d["dx0"], x, w, mu, rstd, d["draw"][0], bug="touch_dead")["dx"].to(BF16)
    assert M.ratio(touched, ra["dx"], ba) > 1 and not torch.equal(touched[w == 0], d["dx0"][w == 0])
    mu2, rstd2 = M.stats_of(d["hidden"][1], d["eps"])                 # the other tap's statistics
    rw = M.dhidden_write(x, w, mu, rstd, d["draw"][0])
    wrong = M.dhidden_write(x, w, mu2, rstd2, d["draw"][0])["dh"].to(BF16)
    assert M.ratio(wrong, rw["dh"], M.dhidden_write_bars(rw, d["E"])) > 1
    assert M.ratio(M.dhidden_acc(d["dx0"], x, w, mu2, rstd2, d["draw"][0])["dx"].to(BF16), ra["dx"], ba) > 1


def test_kernel_constants_restated():
    """MIX_CHUNK and the chains the bars count are those of head.hip (a change there must come back here)."""
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "phantom_vlb_amd", "csrc", "head.hip")).read()
    assert f"constexpr int MIX_CHUNK = {M.MIX_CHUNK};" in src
    assert "for (int j = 0; j < 4; ++j) dot += d[j] * p[j];" in src and "dot = block_sum(dot, red);" in src
    assert "for (int blk = 0; blk < nblk; ++blk) s += slab[(int64_t)blk * K + k];" in src
    assert "#pragma clang fp contract(off)" in src
