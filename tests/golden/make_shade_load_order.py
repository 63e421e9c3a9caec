"""Writes tests/golden/shade_load_order_frames.json and .npz: per feature form of k_shade the ray counts and the SHA-256 of the frame that
tests/test_gpu_shade_load_order.py renders, and the frames themselves (64 x 36, float32).  Run on an MI355X with the library of the commit BEFORE shade_hit issued a hit's loads together (LPT_LIB_PATH=<that build's libloupiote_hip.so>): the test
then holds the changed kernels to those frames.  usage: python tests/golden/make_shade_load_order.py [out.json]  (the frames go beside it, .npz)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before the library, as tests/conftest.py: one copy of the HIP runtime per process)
import loupiote_amd as lp  # noqa: E402
import test_gpu_shade_load_order as K  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else K.GOLDEN
    res, frames = {}, {}
    dev = lp.Device(0)
    for case in K.FEATURES:
        img, launches, counts = K.render_feature(dev, case)
        assert launches["shading"] == K.DEPTH and launches["path"] == 0, (case, launches)
        assert img[..., :3].any(), case
        frames[case] = img
        res[case] = {"counts": list(counts), "sha256": K.digest(img)}
        print(case, res[case], flush=True)
    dev.close()
    with open(out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    np.savez_compressed(os.path.splitext(out)[0] + ".npz", **frames)


if __name__ == "__main__":
    main()
