#!/usr/bin/env python3
"""The thin lens (SPEC.md §25) on the bench workload: what a lens frame costs.

ms per frame at the bench span (synthetic_atrium(seed=2), its sky probe, 1920x1080, 4 spp, depth 8) with the lens closed, with the lens closed and bounce 0 kept off the
packet kernel (LPT_OPT_PACKET_PRIMARY 0: the launches a lens frame takes, with the pinhole's rays), and with the lens open (radius --radius, focused at --focus), the
three renderers alternating: a figure to report, not a bar.  The second column separates what losing the packets costs from what the lens rays
themselves cost (an origin per ray, less coherent primary rays).

usage: python tools/lens_eval.py [--frames 20] [--rounds 3] [--radius 0.05] [--focus 6.0]   (one GPU; prints one JSON line)
"""
import argparse
import json
import os
import sys
import time

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
    ap.add_argument("--radius", type=float, default=0.05)
    ap.add_argument("--focus", type=float, default=6.0)
    a = ap.parse_args()
    dev = lp.Device(0)
    desc = scenes.synthetic_atrium(seed=2)
    pr = lp.ProbeGPU(dev, desc["probe"], desc["probe"].shape[1], desc["probe"].shape[0])
    view = T.look(desc["camera"]["origin"], desc["camera"]["direction"])
    sg = lp.SceneGPU.new_from_scene(scenes.to_product(desc), dev)
    rs = {}
    for name in ("closed", "closed_no_packets", "open"):
        r = lp.Renderer(dev, (1920, 1080))
        r.downsample_factor = 1.0
        r.resize(dev, sg, pr, (1920, 1080))
        r.set_max_bounces(8)
        r.set_vfov(T.VFOV)
        if name == "closed_no_packets":
            r.set_option("packet_primary", 0)
        if name == "open":
            r.set_lens(a.radius, a.focus)
        frame(r, view, 4)   # warm-up
        rs[name] = r
    ms = {name: [] for name in rs}
    for _ in range(a.rounds):   # the renderers alternate, so that drift of the machine lands on all of them
        for name, r in rs.items():
            t0 = time.perf_counter()
            for _ in range(a.frames):
                frame(r, view, 4)
            ms[name].append((time.perf_counter() - t0) * 1e3 / a.frames)
    med = {name: sorted(v)[len(v) // 2] for name, v in ms.items()}
    out = {"workload": "synthetic_atrium(seed=2), 1920x1080, 4 spp, depth 8; open = lens radius %g focused at %g" % (a.radius, a.focus),
           "ms_per_frame_closed": ms["closed"], "ms_per_frame_closed_no_packets": ms["closed_no_packets"], "ms_per_frame_open": ms["open"],
           "ratio_of_medians_open_to_closed": med["open"] / med["closed"], "ratio_of_medians_no_packets_to_closed": med["closed_no_packets"] / med["closed"]}
    print(json.dumps(out))
    for r in rs.values():
        r.close()
    sg.close()
    pr.close()
    dev.close()


if __name__ == "__main__":
    main()
