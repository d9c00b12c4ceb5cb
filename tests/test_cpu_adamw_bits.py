"""The recorded clip+AdamW cases' inputs (adamw_cases.exact_inputs) against the input digests in
tests/golden/adamw_parent_bits.json: a drift in the fixture's inputs - numpy, the platform, an edit of the generator - shows
here as a fixture problem, and never as a kernel problem in test_gpu_adamw_bits.py."""
import json
import os

import numpy as np

import adamw_cases as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adamw_parent_bits.json")


def test_generator_reproduces_every_recorded_input_digest():
    with open(GOLDEN) as f:
        recorded = json.load(f)["cases"]
    cases = C.recorded_cases()
    assert sorted(recorded) == sorted(c["name"] for c in cases) and len(cases) == 13
    for case in cases:
        assert C.digest(C.exact_inputs(case)) == recorded[case["name"]]["inputs"], case["name"]


def test_generator_is_what_it_says():
    """Values on their grids and in range, v >= 0, no two arrays alike, the bf16 patterns 8 significant bits wide."""
    case = dict(C.recorded_cases()[1])
    a = C.exact_inputs(case)
    n = case["n"] + C.TAIL
    assert all(len(x) == n for x in a.values()) and "ema" not in a
    for k in ("p", "g"):
        assert a[k].dtype == np.float32 and np.abs(a[k]).max() < 2 and np.array_equal(a[k] * 2.0 ** 22, np.round(a[k] * 2.0 ** 22))
    assert a["v"].min() >= 0 and a["v"].max() < 0.04 and np.abs(a["m"]).max() < 0.25
    assert len({C.digest({k: x}) for k, x in a.items()}) == len(a) and np.unique(a["p"]).size > n // 2
    g16 = C.exact_inputs(C.recorded_cases()[4])
    assert g16["g"].dtype == np.uint16 and g16["pb"].dtype == np.uint16
    f = (g16["g"].astype(np.uint32) << 16).view(np.float32)
    assert np.abs(f).max() <= 2 and np.array_equal(f * 64, np.round(f * 64)) and np.unique(f).size > 100
    # the first values, written out: index 0 .. 3 of case 0's master, and of its would-be bf16 gradient
    assert C._hash32(4, 0, 0).tolist() == [1753845952, 742688469, 1297640789, 119468856]
    assert C._exact_f32(4, 0, 0).tolist() == [(h >> 8) / 2 ** 22 - 2 for h in (1753845952, 742688469, 1297640789, 119468856)]
    assert C._exact_bf16_bits(4, 0, 3).tolist() == [48848, 16310, 49032, 49050]
    assert all(0 <= int(x) < 2 ** 32 for x in C._hash32(1000, 12, 5))
