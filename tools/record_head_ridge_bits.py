"""Record what the ridge path of the brain head computes - plain and per-subject - as digests, from a library that is trusted
to be right.

  VLB_LIB=/path/to/a/parent/build/libvlb.so python tools/record_head_ridge_bits.py [out.json]

Run once, with VLB_LIB pointing at a build of the commit whose bits are to be kept (built in a worktree outside this
repository).  Calls only the public entry points (vlb_head_fwd_cached, vlb_head_loss_fwd, vlb_head_bwd_cached[_loss],
vlb_head_fwd_grouped, vlb_head_bwd_grouped, vlb_ridge_fwd), on the cases of tests/head_ridge_cases.py, and writes
tests/golden/head_ridge_parent_bits.json: per case the sha256 of the input bytes and the sha256 of every output array (pred,
loss_terms, loss_aux, rowstat, dW, dbias, dz, dpooled, the four LN gradients; pred and l2_out for vlb_ridge_fwd).  Digests and
names only.  tests/test_gpu_head_ridge_bits.py replays it against the in-tree library; run against two libraries, the two files
must be identical.
"""
import json
import os
import sys

import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_ROOT, os.path.join(_ROOT, "tests")]
import head_ridge_cases as C  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(_ROOT, "tests", "golden", "head_ridge_parent_bits.json")
    dev = torch.device("cuda:0")
    cases = {}
    for rc in C.recorded_cases():
        arrays = C.inputs(rc)
        cases[rc["name"]] = {"inputs": C.digest(arrays), "outputs": C.output_digests(C.run_recorded(rc, arrays, dev))}
    doc = {"what": "sha256 of the inputs and of every output array of the recorded ridge-path cases of the brain head "
                   "(tests/head_ridge_cases.py), written by tools/record_head_ridge_bits.py from the library that preceded the one "
                   "ridge kernel family",
           "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(cases)} cases -> {out}")


if __name__ == "__main__":
    main()
