#!/usr/bin/env python3
"""Normal maps (SPEC.md §24) on the bench workload: what the NMAP instantiations of k_shade cost.

ms per frame at the bench span (synthetic_atrium(seed=2), its sky probe, 1920x1080, 4 spp, depth 8) as it is and with a 64x64 normal map (scale 1) on its
largest material — the one whose instances hold the most triangles —, the two scenes alternating: a figure to report, not a bar.

usage: python tools/normal_map_eval.py [--frames 20] [--rounds 3]   (one GPU; prints one JSON line)
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


def bumps(size=64):
    """a normal image of gentle random bumps: x and y within +-0.25 of flat, z up"""
    rng = np.random.RandomState(24)
    img = np.full((size, size, 4), 255, np.uint8)
    img[..., :2] = 128 + rng.randint(-32, 33, (size, size, 2))
    img[..., 2] = 240
    return img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = lp.Device(0)
    desc = scenes.synthetic_atrium(seed=2)
    pr = lp.ProbeGPU(dev, desc["probe"], desc["probe"].shape[1], desc["probe"].shape[0])
    view = T.look(desc["camera"]["origin"], desc["camera"]["direction"])
    rs, share = {}, 0.0
    for name in ("without", "with"):
        scene = scenes.to_product(desc)
        if name == "with":
            inst, ent = scene.instances, scene.entries
            tris = np.zeros(scene.counts().materials, np.int64)
            np.add.at(tris, np.minimum(inst["material_index"], len(tris) - 1), ent["index_count"][inst["blas_index"]] // 3)
            mat = int(np.argmax(tris))
            share = float(tris[mat] / tris.sum())
            scene.set_material_normal_map(mat, scene.add_image(bumps()), 1.0)
        sg = lp.SceneGPU.new_from_scene(scene, dev)
        r = lp.Renderer(dev, (1920, 1080))
        r.downsample_factor = 1.0
        r.resize(dev, sg, pr, (1920, 1080))
        r.set_max_bounces(8)
        r.set_vfov(T.VFOV)
        frame(r, view, 4)   # warm-up
        rs[name] = (r, sg)
    ms = {name: [] for name in rs}
    for _ in range(a.rounds):   # the two scenes alternate, so that drift of the machine lands on both
        for name, (r, _) in rs.items():
            t0 = time.perf_counter()
            for _ in range(a.frames):
                frame(r, view, 4)
            ms[name].append((time.perf_counter() - t0) * 1e3 / a.frames)
    out = {"workload": "synthetic_atrium(seed=2), 1920x1080, 4 spp, depth 8; with = a 64x64 normal map, scale 1, on the material with the most triangles",
           "triangle_share_of_the_mapped_material": share, "ms_per_frame_without": ms["without"], "ms_per_frame_with": ms["with"],
           "ratio_of_medians": sorted(ms["with"])[len(ms["with"]) // 2] / sorted(ms["without"])[len(ms["without"]) // 2]}
    print(json.dumps(out))
    for r, sg in rs.values():
        r.close()
        sg.close()
    pr.close()
    dev.close()


if __name__ == "__main__":
    main()
