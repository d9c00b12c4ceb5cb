"""The sequence of C-ABI calls ``BrainHead`` issues on every host route against tests/golden/head_route_trace.json, recorded
by tools/record_head_routes.py from the head.py that spelled every route out on its own: the entries, their order and every
argument - the same buffer at the same offset, the same scalars, the same S / 0 placement of the loss partials.  "Without the
option, every launch stays as it was" is a promise about exactly this sequence; here it is pinned.

No GPU: ``head.lib`` is the recording proxy of head_route_cases.py (size functions go to the real library, nothing else is
called), ``head._stream`` gives 0 and every tensor lives on the CPU.  A mismatch names the case, the public call and the line.
The second test holds the inputs of the GPU cases (test_gpu_head_route_bits.py) to their recorded digests, so that a drift
in the generators shows here as a fixture problem and never there as a kernel problem."""
import json
import os

import head_route_cases as C

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _expand(doc, name):
    return [s.split(":")[0] + ": " + " | ".join(doc["calls"][int(i)] for i in s.split(":")[1].split()) for s in doc["cases"][name]["steps"]]


def test_every_route_issues_the_recorded_calls(monkeypatch):
    from phantom_vlb_amd import head
    from phantom_vlb_amd.feature_cache import FeatureCache
    with open(os.path.join(_GOLDEN, "head_route_trace.json")) as f:
        text = f.read()
    want = json.loads(text)
    got = C.trace_doc(head, FeatureCache, monkeypatch.setattr)
    assert sorted(got["cases"]) == sorted(want["cases"]) and len(want["cases"]) == 165
    for name in want["cases"]:
        assert got["cases"][name]["inputs"] == want["cases"][name]["inputs"], f"{name}: the fixture's inputs drifted"
        g, w = _expand(got, name), _expand(want, name)
        assert [s.split(":")[0] for s in g] == [s.split(":")[0] for s in w], name
        for a, b in zip(g, w):
            assert a == b, f"{name}: {a.split(':')[0]} issues other calls than recorded"
    assert json.dumps(got, indent=1, sort_keys=True) + "\n" == text        # what the recorder would write: the same bytes


def test_gpu_case_inputs_reproduce_every_recorded_input_digest(monkeypatch):
    from phantom_vlb_amd import _lib, head
    from phantom_vlb_amd.feature_cache import FeatureCache
    with open(os.path.join(_GOLDEN, "head_route_parent_bits.json")) as f:
        recorded = json.load(f)["cases"]
    cases = C.bits_cases()
    assert sorted(recorded) == sorted(c["name"] for c in cases) and len(cases) == 72 + 16 + 4 + 1
    rec = C.Recorder(head.lib, _lib.SIGNATURES, _lib.P)
    monkeypatch.setattr(head, "lib", rec)
    monkeypatch.setattr(head, "_stream", lambda: 0)
    for case in cases:
        inputs, _ = C.run_case(case, "cpu", head.BrainHead, FeatureCache, rec)
        assert C.digest(inputs) == recorded[case["name"]]["inputs"], case["name"]
