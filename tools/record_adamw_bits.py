"""Record what the six clip+AdamW entry points compute, as digests, from a library that is trusted to be right.

  VLB_LIB=/path/to/a/parent/build/libvlb.so python tools/record_adamw_bits.py [out.json]

Run once, with VLB_LIB pointing at a build of the commit whose bits are to be kept (built in a worktree outside this
repository).  Calls only the public entry points, on the cases of tests/adamw_cases.py (inputs from exact integer arithmetic),
and writes tests/golden/adamw_parent_bits.json: per case the sha256 of the input bytes, per case and variant the sha256 of
master, m, v, the bf16 copy (and ema) over [0, n).  Digests and names only.  tests/test_gpu_adamw_bits.py replays it against
the in-tree library; run against two libraries, the two files must be identical.
"""
import json
import os
import sys

import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_ROOT, os.path.join(_ROOT, "tests")]
import adamw_cases as C  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(_ROOT, "tests", "golden", "adamw_parent_bits.json")
    dev = torch.device("cuda:0")
    cases = {}
    for case in C.recorded_cases():
        arrays = C.exact_inputs(case)
        n = case["n"]
        outputs = {}
        for variant in C.RECORDED_VARIANTS:
            got = C.run_recorded(case, variant, arrays, dev)
            outputs[C.variant_name(*variant)] = {name: C.digest({k: got[k][:n]}) for k, name in C.OUTPUTS.items() if k in got}
        cases[case["name"]] = {"inputs": C.digest(arrays), "outputs": outputs}
    doc = {"what": "sha256 of the inputs (all arrays, guards included) and of every output array over [0, n) of the recorded clip+AdamW "
                   "cases (tests/adamw_cases.py), written by tools/record_adamw_bits.py from the library that preceded the unified kernel",
           "cases": cases}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(cases)} cases x {len(C.RECORDED_VARIANTS)} variants -> {out}")


if __name__ == "__main__":
    main()
