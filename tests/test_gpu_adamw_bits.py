"""The six clip+AdamW entry points against bits recorded from the library that preceded the unified kernel
(tests/golden/adamw_parent_bits.json, written by tools/record_adamw_bits.py from the parent commit's build).

test_gpu_adamw_groups.py / test_gpu_adamw_ema.py compare instantiations of one kernel family with each other: real tests of
the table search, the LDS staging and the pointer offsets, but no anchor for the arithmetic.  This is the anchor: every case
must reproduce the digest of every output array; vlb_adamw_step also on the shapes only its one-element-per-lane path serves
(n = 1, n % 8 != 0, pointers aligned to their element only).  Inputs come from exact integer arithmetic
(adamw_cases.exact_inputs; test_cpu_adamw_bits.py holds them to the recorded input digests).  A mismatch names the case, the
variant and the array: rerun tools/record_adamw_bits.py against a parent build to look at the values."""
import json
import os

import numpy as np
import pytest

import adamw_cases as C

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adamw_parent_bits.json")
CASES = C.recorded_cases()


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def test_every_case_is_recorded(recorded):
    assert sorted(recorded) == sorted(c["name"] for c in CASES)
    for rec in recorded.values():
        assert sorted(rec["outputs"]) == sorted(C.variant_name(*v) for v in C.RECORDED_VARIANTS)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_entry_reproduces_the_recorded_bits(dev, recorded, case):
    n = case["n"]
    arrays = C.exact_inputs(case)
    for variant in C.RECORDED_VARIANTS:
        vname = C.variant_name(*variant)
        want = recorded[case["name"]]["outputs"][vname]
        got = C.run_recorded(case, variant, arrays, dev)
        assert sorted(want) == sorted(name for k, name in C.OUTPUTS.items() if k in got)
        for k, a in got.items():
            assert np.array_equal(a[n:], arrays[k][n:]), (case["name"], vname, k, "wrote behind the end")
        assert np.array_equal(got["g"], arrays["g"]), (case["name"], vname, "the gradient was written")
        assert not np.array_equal(got["p"][:n], arrays["p"][:n]), (case["name"], vname, "master did not move")
        assert np.array_equal(got["pb"], arrays["pb"]) == (not variant[2]), (case["name"], vname, "bf16 copy")
        for k, name in C.OUTPUTS.items():
            if k in got:
                assert C.digest({k: got[k][:n]}) == want[name], \
                    f"{case['name']} {vname}: array '{name}' differs from the recorded parent bits"
