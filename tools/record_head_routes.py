"""Record what ``BrainHead`` does on every host route, from a head.py that is trusted to be right.

  python tools/record_head_routes.py --tree DIR [--out FILE]           # the call trace, on the CPU
  python tools/record_head_routes.py --tree DIR --bits [--out FILE]    # output digests, on the GPU

``DIR`` is a checkout with its own build of libvlb.so (of the commit whose behaviour is to be kept, outside this repository);
it is put first on sys.path, so ``phantom_vlb_amd.head`` is that tree's copy.  The cases and the runner are this tree's
tests/head_route_cases.py.  Without ``--bits`` the head's library is replaced by the recording proxy of that file and
tests/golden/head_route_trace.json is written: per case the sha256 of the inputs and the sequence of C-ABI calls, pointers as
owner+offset; a buffer the recorded tree names differently is mapped through ``ALIASES`` of the cases file.  With ``--bits``
the cases run on cuda:0 and tests/golden/head_route_parent_bits.json is written: digests and names only.
tests/test_cpu_head_route_trace.py and tests/test_gpu_head_route_bits.py replay the two files against the in-tree head.py;
recorded from two trees, each file must come out byte-identical.
"""
import argparse
import json
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", required=True)
    ap.add_argument("--bits", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    sys.path[:0] = [os.path.abspath(args.tree), os.path.join(_ROOT, "tests")]
    import head_route_cases as C
    from phantom_vlb_amd import head
    from phantom_vlb_amd.feature_cache import FeatureCache
    assert os.path.abspath(head.__file__).startswith(os.path.abspath(args.tree) + os.sep), head.__file__
    if args.bits:
        import torch
        doc = C.bits_doc(torch.device("cuda:0"), head.BrainHead, FeatureCache)
    else:
        doc = C.trace_doc(head, FeatureCache, setattr)
    out = args.out or os.path.join(_ROOT, "tests", "golden", "head_route_parent_bits.json" if args.bits else "head_route_trace.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(doc['cases'])} cases -> {out}")


if __name__ == "__main__":
    main()
