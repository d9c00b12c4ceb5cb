"""The recorded ridge-path cases' inputs (head_ridge_cases.inputs) against the input digests in
tests/golden/head_ridge_parent_bits.json: a drift in the fixture's inputs - torch's generators, the platform, an edit of an
emulator's input maker - shows here as a fixture problem, and never as a kernel problem in test_gpu_head_ridge_bits.py."""
import json
import os

import group_emul as GE
import head_emul as H
import head_ridge_cases as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_ridge_parent_bits.json")


def test_inputs_reproduce_every_recorded_input_digest():
    with open(GOLDEN) as f:
        recorded = json.load(f)["cases"]
    cases = C.recorded_cases()
    assert sorted(recorded) == sorted(rc["name"] for rc in cases) and len(cases) == 27
    for rc in cases:
        assert C.digest(C.inputs(rc)) == recorded[rc["name"]]["inputs"], rc["name"]


def test_cases_reach_the_paths_they_are_there_for():
    """the shapes, restated through the emulators' planners: both forward forms, both dz routes, one to three b0 passes,
    KSTEPS 4 / 8 / 32, the 2048-block cap with and without a head boundary inside the wrap"""
    by = {rc["name"]: rc["case"] for rc in C.recorded_cases()}
    plain = {n.split("/")[1]: c for n, c in by.items() if n.startswith("plain/") and n.endswith("/mse")}
    assert [(c["E"], c["B"], c["V"]) for c in plain.values()] == [(512, 5, 40), (1024, 16, 40), (1024, 17, 40), (264, 2, 48), (512, 3, 17),
                                                                  (4096, 3, 33), (128, 2, 32784)]
    assert "ridge_fwd_mfma_kernel<4>" in H.dispatch(5, 512) and "ridge_fwd_mfma_kernel<32>" in H.dispatch(3, 4096)
    assert H.dispatch(16, 1024) >= {"ridge_fwd_mfma_kernel<8>", "ridge_bwd_w:b0_passes=2", "dpred_t_kernel"}
    assert H.dispatch(17, 1024) >= {"ridge_fwd_kernel", "ridge_bwd_z_kernel", "ridge_bwd_w:b0_passes=3"}
    assert H.dispatch(2, 264) >= {"ridge_fwd_kernel", "dpred_t_kernel"}
    assert plain["scales-B17"]["drop"] and plain["scales-B17"]["scales"] == (0.25, 0.5)
    assert H.cdiv(32784, 16) == 2049 and H.cdiv(17, 16) == 2
    wrap = by["grouped/g3-wrap/mse"]
    tpg = H.cdiv(wrap["V"], 16)
    assert (tpg, wrap["G"] * tpg) == (683, 2049) and GE.grouped_fwd_parts(wrap["B"], wrap["E"], wrap["V"], wrap["G"]) == 2048
    assert GE.tile_of(2048, wrap["V"])[0] == 2 and wrap["subjects"] == (2, 0)       # block 0: a tile of head 0, then one of head 2
    grouped = {n.split("/")[1] for n in by if n.startswith("grouped/")}
    assert grouped == {c["id"] for c in GE.CASES + GE.G1_CASES} | {"g3-wrap"}
    for kind, ids in (("plain", ("E512-B5", "scales-B17")), ("grouped", GE.LOSS_CASES)):
        for cid in ids:
            assert {f"{kind}/{cid}/{k}" for k in ("mse", "cosine", "pearson")} <= set(by)
    assert (by["ridge_fwd/ridge-E264-B9-V17"]["E"], by["ridge_fwd/ridge-E264-B9-V17"]["B"], by["ridge_fwd/ridge-E264-B9-V17"]["V"]) == (264, 9, 17)
