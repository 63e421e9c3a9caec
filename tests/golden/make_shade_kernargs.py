"""Writes tests/golden/shade_kernargs_frames.json: per form of k_shade the ray counts and the SHA-256 of the frame that tests/test_gpu_shade_kernargs.py renders.
Run on an MI355X with the library of the commit BEFORE k_shade took its arguments as one struct (LPT_LIB_PATH=<that build's libloupiote_hip.so>): the test then holds
the changed kernels to those frames.  --only CASE renders that case alone, with the library of the commit before the case came, and leaves the file's other entries
as they are.  usage: python tests/golden/make_shade_kernargs.py [--only CASE] [out.json]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import torch  # noqa: E402,F401  (before the library, as tests/conftest.py: one copy of the HIP runtime per process)
import loupiote_amd as lp  # noqa: E402
import test_gpu_shade_kernargs as K  # noqa: E402


def main():
    args = sys.argv[1:]
    only = None
    if args[:1] == ["--only"]:
        only, args = args[1], args[2:]
        assert only in K.CASES, only
    out = args[0] if args else K.GOLDEN
    res = {}
    if only is not None:
        with open(K.GOLDEN) as f:
            res = json.load(f)
    dev = lp.Device(0)
    for case in ([only] if only is not None else K.CASES):
        arrays, launches, counts = K.render(dev, case)
        assert launches["shading"] == K.DEPTH and launches["path"] == 0 and launches["primary intersection"] == 1, (case, launches)
        assert arrays[0][..., :3].any(), case
        res[case] = {"counts": list(counts), "sha256": K.digest(arrays)}
        print(case, res[case], flush=True)
    dev.close()
    with open(out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
