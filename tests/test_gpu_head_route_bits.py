"""Every host route of ``BrainHead`` against bits recorded from the head.py that spelled each route out on its own
(tests/golden/head_route_parent_bits.json, written by tools/record_head_routes.py --bits on an MI355X from the parent commit's
checkout and build): dense, packed, cached, tapped (K = 1, 3) and tapped-and-cached, one head and G = 2, every objective,
unweighted and masked, at the two shapes at which the host's decisions differ (MFMA / scalar ridge form, skinny / wide dz,
partials behind pooling slabs or at 0); the four closed-form fit sequences; one head object reused across shapes and routes.

Every output the route defines must reproduce its digest, no tolerance.  The cases and the runner are head_route_cases.py's,
shared with the recorder; test_cpu_head_route_trace.py holds the inputs to the recorded input digests and the C-ABI call
sequence to its own recording, so a mismatch here with that test green is a difference in what the host hands the kernels
that the trace cannot see (buffer contents, initialisation), or in the library."""
import json
import os

import pytest

import head_route_cases as C

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_route_parent_bits.json")
CASES = C.bits_cases()


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def test_every_case_is_recorded(recorded):
    assert sorted(recorded) == sorted(c["name"] for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_routes_reproduce_the_recorded_bits(dev, recorded, case):
    import torch
    from phantom_vlb_amd.feature_cache import FeatureCache
    from phantom_vlb_amd.head import BrainHead
    inputs, out = C.run_case(case, dev, BrainHead, FeatureCache)
    torch.cuda.synchronize()
    assert C.digest(inputs) == recorded[case["name"]]["inputs"], "the fixture's inputs drifted: see test_cpu_head_route_trace.py"
    got, want = C.output_digests(out), recorded[case["name"]]["outputs"]
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], f"{case['name']}: '{k}' differs from the recorded parent bits"
