#!/usr/bin/env python3
"""Emissive materials (SPEC.md §22) on the bench workload: what the EMIS instantiations of k_shade cost.

ms per frame at the bench span (synthetic_atrium(seed=2), its sky probe, 1920x1080, 4 spp, depth 8) without an emitter and with one emissive panel
in the camera's view, the two scenes alternating — a figure to report, not a bar.

--sampling (SPEC.md §23): the scene with the panel, emitter sampling off against on, alternating: ms per frame, the per-pixel variance at equal spp (over
--seeds independent 4-spp frames, averaged over the pixels) and the equal-time variance ratio (variance x ms, off / on) — figures for DESIGN §5.2f.

usage: python tools/emissive_eval.py [--frames 20] [--rounds 3] [--sampling [--seeds 8]]   (one GPU; prints one JSON line)
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


def frame(r, view, spp):
    r.reset_accumulation()
    r.accumulate = True
    for _ in range(spp):
        r.raytrace(view)
    return r.read_radiance()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sampling", action="store_true")
    ap.add_argument("--seeds", type=int, default=8)
    a = ap.parse_args()
    dev = lp.Device(0)
    desc = scenes.synthetic_atrium(seed=2)
    pr = lp.ProbeGPU(dev, desc["probe"], desc["probe"].shape[1], desc["probe"].shape[0])
    view = T.look(desc["camera"]["origin"], desc["camera"]["direction"])
    rs = {}
    arms = ("off", "on") if a.sampling else ("without", "with")
    for name in arms:
        scene = scenes.to_product(desc)
        if name != "without":   # a 1 x 1 emissive panel three units in front of the camera, facing it
            o, d = np.asarray(desc["camera"]["origin"], np.float64), np.asarray(desc["camera"]["direction"], np.float64)
            d /= np.linalg.norm(d)
            u = np.cross(d, (0.0, 1.0, 0.0))
            u /= np.linalg.norm(u)
            v = np.cross(u, d)
            c = o + 3.0 * d
            pos = np.array([c - 0.5 * u - 0.5 * v, c + 0.5 * u - 0.5 * v, c + 0.5 * u + 0.5 * v, c - 0.5 * u + 0.5 * v], np.float32)
            nrm = np.tile((-d).astype(np.float32)[None], (4, 1))
            blas = scene.add_mesh(pos, nrm, np.zeros((4, 2), np.float32), np.array([0, 2, 1, 0, 3, 2], np.uint32))
            mat = scene.add_material((0.1, 0.1, 0.1, 1.0), 0.8, 0.0)
            scene.set_material_emission(mat, (1.0, 0.8, 0.6), 5.0)
            scene.add_instance(blas, np.eye(4, dtype=np.float32), mat)
        sg = lp.SceneGPU.new_from_scene(scene, dev)
        r = lp.Renderer(dev, (1920, 1080))
        r.downsample_factor = 1.0
        r.resize(dev, sg, pr, (1920, 1080))
        r.set_max_bounces(8)
        r.set_vfov(T.VFOV)
        r.set_emissive_sampling(name == "on")
        frame(r, view, 4)   # warm-up
        rs[name] = (r, sg)
    ms = {name: [] for name in arms}
    for _ in range(a.rounds):   # the two scenes alternate, so that drift of the machine lands on both
        for name, (r, _) in rs.items():
            t0 = time.perf_counter()
            for _ in range(a.frames):
                frame(r, view, 4)
            ms[name].append((time.perf_counter() - t0) * 1e3 / a.frames)
    if a.sampling:
        var = {}
        for name, (r, _) in rs.items():
            x = []
            for k in range(a.seeds):
                r.set_seed(1000 + k)
                x.append(frame(r, view, 4)[..., :3].astype(np.float64))
            var[name] = float(np.var(np.stack(x), axis=0, ddof=1).mean())
        med = {name: sorted(v)[len(v) // 2] for name, v in ms.items()}
        print(json.dumps({"workload": "synthetic_atrium(seed=2) + one 1 x 1 emissive panel (Le = (5, 4, 3)), 1920x1080, 4 spp, depth 8; emitter sampling off / on",
                          "ms_per_frame_off": ms["off"], "ms_per_frame_on": ms["on"], "variance_off": var["off"], "variance_on": var["on"],
                          "variance_ratio_equal_spp": var["off"] / var["on"], "variance_ratio_equal_time": (var["off"] * med["off"]) / (var["on"] * med["on"])}))
        for r, sg in rs.values():
            r.close()
            sg.close()
        pr.close()
        dev.close()
        return
    out = {"workload": "synthetic_atrium(seed=2), 1920x1080, 4 spp, depth 8; with = + one 1 x 1 emissive panel (Le = (5, 4, 3)) three units before the camera",
           "ms_per_frame_without": ms["without"], "ms_per_frame_with": ms["with"],
           "ratio_of_medians": sorted(ms["with"])[len(ms["with"]) // 2] / sorted(ms["without"])[len(ms["without"]) // 2]}
    print(json.dumps(out))
    for r, sg in rs.values():
        r.close()
        sg.close()
    pr.close()
    dev.close()


if __name__ == "__main__":
    main()
