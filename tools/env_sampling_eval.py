#!/usr/bin/env python3
"""Environment importance sampling (SPEC.md §18) on the bench workload: cost and gain of lpt_renderer_set_env_sampling.

  * ms per frame with the mode off and on at the bench span (synthetic_atrium(seed=2), sky probe with sun, 1920x1080, 4 spp, depth 8);
  * RMSE of 4-spp frames against a high-spp on-mode reference at a reduced size, off and on;
  * the equal-time error ratio: RMSE_on / RMSE_off x sqrt(ms_on / ms_off) (error falls with the square root of the samples a budget buys).

usage: python tools/env_sampling_eval.py [--frames 20] [--ref-spp 2048] [--small 320x180]   (one GPU; prints one JSON line)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import loupiote_amd as lp  # noqa: E402
from loupiote_amd import scenes, testing as T  # noqa: E402


def make_renderer(dev, sg, pr, w, h, env, seed=0):
    r = lp.Renderer(dev, (w, h))
    r.downsample_factor = 1.0
    r.resize(dev, sg, pr, (w, h))
    r.set_max_bounces(8)
    r.set_vfov(T.VFOV)
    r.set_seed(seed)
    r.set_env_sampling(env)
    return r


def frame(r, view, spp):
    r.reset_accumulation()
    r.accumulate = True
    for _ in range(spp):
        r.raytrace(view)
    return r.read_radiance()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--ref-spp", type=int, default=2048)
    ap.add_argument("--small", default="320x180")
    ap.add_argument("--trials", type=int, default=8)
    a = ap.parse_args()
    dev = lp.Device(0)
    desc = scenes.synthetic_atrium(seed=2)
    sg = lp.SceneGPU.new_from_scene(scenes.to_product(desc), dev)
    pr = lp.ProbeGPU(dev, desc["probe"], desc["probe"].shape[1], desc["probe"].shape[0])
    view = T.look(desc["camera"]["origin"], desc["camera"]["direction"])
    out = {"workload": "synthetic_atrium(seed=2), sky probe 1024x512 with sun, depth 8"}
    # cost at the bench span
    for env in (False, True):
        r = make_renderer(dev, sg, pr, 1920, 1080, env)
        frame(r, view, 4)   # warm-up (and the distribution's one-time build)
        t0 = time.perf_counter()
        for _ in range(a.frames):
            frame(r, view, 4)
        out["ms_per_frame_" + ("on" if env else "off")] = (time.perf_counter() - t0) * 1e3 / a.frames
        r.close()
    # error at a reduced size against a high-spp on-mode reference
    w, h = (int(v) for v in a.small.split("x"))
    r = make_renderer(dev, sg, pr, w, h, True, seed=12345)
    ref = frame(r, view, a.ref_spp)[..., :3].astype(np.float64)
    r.close()
    for env in (False, True):
        errs = []
        for t in range(a.trials):
            r = make_renderer(dev, sg, pr, w, h, env, seed=t + 1)
            img = frame(r, view, 4)[..., :3].astype(np.float64)
            r.close()
            errs.append(float(np.sqrt(np.mean((img - ref) ** 2))))
        out["rmse_4spp_" + ("on" if env else "off")] = float(np.mean(errs))
    out["reference"] = "%dx%d, %d spp, mode on" % (w, h, a.ref_spp)
    out["rmse_ratio_equal_spp"] = out["rmse_4spp_on"] / out["rmse_4spp_off"]
    out["error_ratio_equal_time"] = out["rmse_ratio_equal_spp"] * np.sqrt(out["ms_per_frame_on"] / out["ms_per_frame_off"])
    print(json.dumps(out))
    pr.close()
    sg.close()
    dev.close()


if __name__ == "__main__":
    main()
