"""The ridge path of the brain head, plain and per-subject, against bits recorded from the library that preceded the one
ridge kernel family (tests/golden/head_ridge_parent_bits.json, written by tools/record_head_ridge_bits.py from the parent
commit's build, where the per-subject kernels were copies of the plain ones).

test_gpu_multi_subject.py::test_one_group_gives_the_ungrouped_bits compares two instantiations of one template with each
other: a real test of the GROUPED switch, but no anchor for the arithmetic.  This is the anchor: every case must reproduce the
digest of every output array, no tolerance.  Inputs come from the emulators' seeded generators
(head_ridge_cases.inputs; test_cpu_head_ridge_bits.py holds them to the recorded input digests).  A mismatch names the case
and the array: rerun tools/record_head_ridge_bits.py against a parent build to look at the values."""
import json
import os

import pytest

import head_ridge_cases as C

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_ridge_parent_bits.json")
CASES = C.recorded_cases()


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def test_every_case_is_recorded(recorded):
    assert sorted(recorded) == sorted(rc["name"] for rc in CASES)
    for rc in CASES:
        want = C.RIDGE_OUTPUTS if rc["kind"] == "ridge_fwd" else [k for k in C.TAIL_OUTPUTS if rc["loss"] != "mse" or k not in ("loss_aux", "rowstat")]
        assert sorted(recorded[rc["name"]]["outputs"]) == sorted(want), rc["name"]


@pytest.mark.parametrize("rc", CASES, ids=[rc["name"] for rc in CASES])
def test_entries_reproduce_the_recorded_bits(dev, recorded, rc):
    arrays = C.inputs(rc)
    assert C.digest(arrays) == recorded[rc["name"]]["inputs"], "the fixture's inputs drifted: see test_cpu_head_ridge_bits.py"
    got = C.output_digests(C.run_recorded(rc, arrays, dev))
    want = recorded[rc["name"]]["outputs"]
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], f"{rc['name']}: array '{k}' differs from the recorded parent bits"
