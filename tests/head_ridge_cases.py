"""Shared by tools/record_head_ridge_bits.py, test_gpu_head_ridge_bits.py and test_cpu_head_ridge_bits.py: the RECORDED
cases of the ridge path of the brain head - plain and per-subject - and the runner that pushes them through the public
entry points, so that the recording tool and the test that replays tests/golden/head_ridge_parent_bits.json cannot drift apart.

A case is a tail step from (pooled_raw, sumw): vlb_head_fwd_cached (+ vlb_head_loss_fwd) and vlb_head_bwd_cached[_loss], or
vlb_head_fwd_grouped and vlb_head_bwd_grouped, or vlb_ridge_fwd on its own.  Shapes are the smallest at which each path of
head.hip can go wrong; inputs are those of head_emul / head_loss_emul / group_emul (their cases where one has the shape,
their case makers otherwise, their seeded input makers always) with (pooled_raw, sumw) = head_emul.pool's fp64 result rounded
to fp32.  test_cpu_head_ridge_bits.py holds the inputs to the recorded input digests."""
import hashlib

import numpy as np
import torch

import group_emul as GE
import head_emul as H
import head_loss_emul as L

BF = torch.bfloat16
LOSS_KIND = {"mse": 0, "cosine": 1, "pearson": 2}
PARAMS = ("layer_norm1.weight", "layer_norm1.bias", "layer_norm2.weight", "layer_norm2.bias", "ridge_layer.linear.weight",
          "ridge_layer.linear.bias")
TAIL_OUTPUTS = ("pred", "loss_terms", "loss_aux", "rowstat", "dW", "dbias", "dz", "dpooled", "dg1", "db1", "dg2", "db2")
RIDGE_OUTPUTS = ("pred", "l2_out")

# plain head: (case, what it is there for); the two LOSS shapes also run with cosine and pearson
_PLAIN = [
    H._case("E512-B5", 512, 33, 5, 40),                         # MFMA<4>, skinny dz, one b0 pass
    H.BY_ID["clips-B16"],                                       # E=1024 B=16 V=40: MFMA<8>, two passes
    H.BY_ID["scales-B17"],                                      # E=1024 B=17 V=40, dropout, scales (0.25, 0.5): scalar forward, ridge_bwd_z, three passes
    H.BY_ID["pool-E264"],                                       # E=264 B=2 V=48 (S=70): scalar forward, skinny dz
    H.BY_ID["targets-V17"],                                     # E=512 B=3 V=17: one live row in the last tile
    H._case("E4096-B3-V33", 4096, 33, 3, 33),                   # KSTEPS = 32
    H.BY_ID["targets-V32784"],                                  # E=128 B=2 V=32784 (S=32): 2049 tiles over 2048 persistent blocks
]
_PLAIN_LOSS = ("E512-B5", "scales-B17")
_RIDGE_FWD = [H._case("ridge-E264-B9-V17", 264, 33, 9, 17),     # y = nullptr, two passes
              H._case("ridge-E512-B5", 512, 33, 5, 40)]         # an MFMA shape: the layer on its own stays on the scalar form
# grouped: group_emul's cases, its G = 1 cases, and the persistent MFMA loop wrapping across a head boundary
# (tpg = 683, 3 * 683 = 2049 tiles over 2048 blocks: block 0 takes tile 0 of head 0 and tile 2048 = the last tile of head 2)
_WRAP = GE._case("g3-wrap", 128, 2, 10928, 3, [2, 0])
_GROUPED = GE.CASES + GE.G1_CASES + [_WRAP]


def recorded_cases():
    """-> list of dicts: name, kind ("plain" | "grouped" | "ridge_fwd"), case, loss"""
    out = [dict(name=f"plain/{c['id']}/mse", kind="plain", case=c, loss="mse") for c in _PLAIN]
    out += [dict(name=f"plain/{c['id']}/{k}", kind="plain", case=c, loss=k) for c in _PLAIN if c["id"] in _PLAIN_LOSS for k in L.LOSSES]
    out += [dict(name=f"ridge_fwd/{c['id']}", kind="ridge_fwd", case=c, loss="mse") for c in _RIDGE_FWD]
    out += [dict(name=f"grouped/{c['id']}/mse", kind="grouped", case=c, loss="mse") for c in _GROUPED]
    out += [dict(name=f"grouped/{cid}/{k}", kind="grouped", case=GE.BY_ID[cid], loss=k) for cid in GE.LOSS_CASES for k in L.LOSSES]
    return out


def inputs(rc):
    """The recorded case's input arrays as numpy, in a fixed order: pooled_raw, sumw (fp32), the six parameters (bf16-valued
    fp32), y, keep (absent without dropout), group (int32, grouped only), scales = (loss_scale, l2_scale, lam, eps)."""
    c, loss = rc["case"], rc["loss"]
    if rc["kind"] == "grouped":
        inp = GE.make_inputs(c, loss)
    elif loss != "mse":
        inp = L.make_inputs(L._case(c["id"], c["E"], c["S"], c["B"], c["V"], drop=c["drop"], scales=c["scales"]), loss)
    else:
        inp = H.make_inputs(c)
    po = H.pool(inp["hidden"], inp["wmask"], inp["eps"])
    a = {"pooled_raw": po["pooled_raw"].float().numpy(), "sumw": po["sumw"].float().numpy()}
    for k in PARAMS:
        a[k] = inp["params"][k].float().contiguous().numpy()
    a["y"] = inp["y"].float().numpy()
    if inp["keep"] is not None:
        a["keep"] = inp["keep"].float().numpy()
    if rc["kind"] == "grouped":
        a["group"] = np.asarray(inp["group"], dtype=np.int32)
    a["scales"] = np.asarray([inp["loss_scale"], inp["l2_scale"], inp["lam"], inp["eps"]], dtype=np.float32)
    return a


def digest(arrays):
    h = hashlib.sha256()
    for k, a in arrays.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def run_recorded(rc, a, dev):
    """One forward (+ backward) of the case through the public entry points on device copies of ``a`` -> {output: numpy}."""
    from phantom_vlb_amd._lib import check, lib
    c, kind = rc["case"], rc["kind"]
    B, E, V, G = c["B"], c["E"], c["V"], c.get("G", 1)
    lk = LOSS_KIND[rc["loss"]]
    loss_scale, l2_scale, lam, eps = (float(x) for x in a["scales"])
    f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)               # noqa: E731
    t = {k: torch.from_numpy(v).to(dev) for k, v in a.items() if k != "scales"}
    g1, b1, g2, b2, W, bias = (t[k].to(BF).contiguous() for k in PARAMS)
    ptr = lambda x: None if x is None else x.data_ptr()                                      # noqa: E731
    out = {}
    if kind == "ridge_fwd":
        x = t["pooled_raw"].to(BF).contiguous()              # any bf16 [B,E] serves as the layer's input
        pred, l2 = f32(B, V), f32(1)
        ws = f32(int(lib.vlb_ridge_ws_floats(V)))
        check(lib.vlb_ridge_fwd(ptr(x), ptr(W), ptr(bias), ptr(pred), ptr(l2), ptr(ws), B, E, V, lam, _stream()), "vlb_ridge_fwd")
        out = {"pred": pred, "l2_out": l2}
    else:
        keep = t.get("keep")
        rows = torch.arange(B, dtype=torch.int32, device=dev)
        pooled_raw, sumw, zhat, rstd, z, pred = f32(B, E), f32(B), f32(B, E), f32(B), torch.zeros(B, E, dtype=BF, device=dev), f32(B, V)
        rowstat, terms, aux = f32(B, 8), f32(3), f32(2)
        dW, db, dg2, db2, dg1, db1 = f32(G * V, E), f32(G * V), f32(E), f32(E), f32(E), f32(E)
        dz, dpooled = f32(B, E), f32(B, E)
        if kind == "plain":
            ws = f32(int(lib.vlb_head_ws_floats(B, 1, E, V)))
            check(lib.vlb_head_fwd_cached(ptr(t["pooled_raw"]), ptr(t["sumw"]), ptr(rows), ptr(g1), ptr(b1), ptr(g2), ptr(b2), ptr(W),
                                          ptr(bias), ptr(t["y"]), ptr(keep), ptr(ws), ptr(pooled_raw), ptr(sumw), ptr(zhat), ptr(rstd),
                                          ptr(z), ptr(pred), ptr(terms), B, E, V, B, eps, lam, _stream()), "vlb_head_fwd_cached")
            tail = [ptr(g1), ptr(g2), ptr(W), ptr(t["y"]), ptr(keep), ptr(pooled_raw), ptr(sumw), ptr(zhat), ptr(rstd), ptr(z),
                    ptr(pred), ptr(dW), ptr(db), ptr(dg2), ptr(db2), ptr(dg1), ptr(db1), ptr(ws), ptr(dz), ptr(dpooled), B, E, V, eps, lam,
                    loss_scale, l2_scale, _stream()]
            if lk:
                check(lib.vlb_head_loss_fwd(ptr(pred), ptr(t["y"]), ptr(ws), ptr(rowstat), ptr(terms), ptr(aux), B, 0, E, V, lk, lam,
                                            _stream()), "vlb_head_loss_fwd")
                check(lib.vlb_head_bwd_cached_loss(*tail, lk, ptr(rowstat)), "vlb_head_bwd_cached_loss")
            else:
                check(lib.vlb_head_bwd_cached(*tail), "vlb_head_bwd_cached")
        else:
            ws = f32(int(lib.vlb_head_grouped_ws_floats(B, E, V, G)))
            check(lib.vlb_head_fwd_grouped(ptr(t["pooled_raw"]), ptr(t["sumw"]), ptr(rows), ptr(g1), ptr(b1), ptr(g2), ptr(b2), ptr(W),
                                           ptr(bias), ptr(t["y"]), ptr(keep), ptr(t["group"]), ptr(ws), ptr(pooled_raw), ptr(sumw),
                                           ptr(zhat), ptr(rstd), ptr(z), ptr(pred), ptr(rowstat), ptr(terms), ptr(aux), B, E, V, G, B, eps,
                                           lam, lk, _stream()), "vlb_head_fwd_grouped")
            check(lib.vlb_head_bwd_grouped(ptr(g1), ptr(g2), ptr(W), ptr(t["y"]), ptr(keep), ptr(t["group"]), ptr(pooled_raw), ptr(sumw),
                                           ptr(zhat), ptr(rstd), ptr(z), ptr(pred), ptr(dW), ptr(db), ptr(dg2), ptr(db2), ptr(dg1),
                                           ptr(db1), ptr(ws), ptr(dz), ptr(dpooled), ptr(rowstat), B, E, V, G, eps, lam, loss_scale,
                                           l2_scale, lk, _stream()), "vlb_head_bwd_grouped")
        out = dict(pred=pred, loss_terms=terms, dW=dW, dbias=db, dz=dz, dpooled=dpooled, dg1=dg1, db1=db1, dg2=dg2, db2=db2)
        if lk:
            out.update(loss_aux=aux, rowstat=rowstat)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def output_digests(got):
    return {k: digest({k: v}) for k, v in got.items()}
