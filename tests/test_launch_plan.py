"""Host logic: which kernels a wavefront runs and with which grids (loupiote_amd/csrc/launch_plan.h plan_wavefront), checked on the CPU through
tests/tools/plan_check.cpp: named cases whose plans are worked out by hand from the rules, the exclusion rules as properties over a sweep of ray
counts, modes and knobs, and purity (every case is planned twice, in the program and from here)."""
import itertools
import json
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "loupiote_amd", "csrc")
VARIANTS = {"0000", "0100", "1000", "1100", "0010", "0110", "0001", "1001"}   # (STATS, PIPE, TAIL, MASK): the k_trace instantiations that exist
MAX_RAYS = 0x7FFFFFFF
GBUF, ENV, PUNCT, TRANS, EMIS, ESAMP, NMAP = (1 << i for i in range(7))   # kernel_forms.h: the bits of a k_shade / k_path form
DEFAULT_COOP_RAYS, DEFAULT_PATH_RAYS = 32000, 120000


def _constant(text, name):
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([0-9.eE+-]+)" % name, text)
    assert m, name
    return m.group(1)


@pytest.fixture(scope="module")
def limits():
    """the kernels' constants as the sources state them (what device.hip hands to the plan as KernelLimits)"""
    kernels, device = (open(os.path.join(CSRC, f)).read() for f in ("kernels.h", "device.hip"))
    lim = {n: _constant(kernels, n) for n in ("kBlock", "kTraceBlock", "kTailMax")}
    lim.update({n: _constant(device, n) for n in ("kCoopWavesPerCu", "kPacketBlocksPerCu", "kPacketMaxPixelRad")})
    assert (int(lim["kBlock"]), int(lim["kTraceBlock"]), int(lim["kTailMax"]), int(lim["kCoopWavesPerCu"]), int(lim["kPacketBlocksPerCu"])) == (256, 64, 8, 32, 128)
    return lim


@pytest.fixture(scope="module")
def plan(tmp_path_factory, limits):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "tools", "plan_check.cpp")], check=True)

    def run(cases):
        """cases: dicts of LaunchTuning / WavefrontFacts fields; every case is planned twice and the two answers must be the same"""
        lines = [" ".join("%s=%s" % kv for kv in dict(limits, cus=256, **c).items()) for c in cases]
        p = subprocess.run([exe], input="\n".join(lines + lines) + "\n", capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        out = [json.loads(l) for l in p.stdout.splitlines()]
        assert len(out) == 2 * len(cases) and out[:len(cases)] == out[len(cases):]
        assert all(o["same_again"] == 1 for o in out)
        return out[:len(cases)]
    return run


def frame(w, h, spp, parts=1, vfov=math.pi / 4, **more):
    """a wavefront over 1 / parts of a w x h frame with spp samples per pixel (tiles of 32 x 8: dense and block8 where they divide the frame)"""
    slots = w * h // parts
    f = dict(n_rays=slots * spp, n_slots=slots, slot0=0, n_samples=spp, pixel_rad=repr(2.0 * math.tan(0.5 * vfov) / h),
             dense=int(w % 32 == 0 and h % 8 == 0), block8=1, max_depth=12, stack_entries=11)
    f.update(more)
    return f


def div_up(a, b):
    return (a + b - 1) // b


def test_named_cases(plan):
    shard = dict(frame(1920, 1080, 4, parts=8), solo=1)
    small = dict(frame(256, 256, 1), solo=1)
    masked = dict(small, masked=1, packet_primary=1, path_rays=MAX_RAYS)
    half = frame(1920, 1080, 4, parts=2)
    (bench_half, eighth, no_tail, refill2, tiny, path, trans, stats, mask, mask_stats, no_pipe, no_pipe_stats, pinned) = plan([
        half, shard, dict(shard, tail_lanes=0), dict(shard, refill=2), dict(frame(64, 36, 4), solo=1), small, dict(small, trans=1), dict(small, stats=1),
        masked, dict(masked, stats=1), dict(half, pipe_rays=0), dict(half, pipe_rays=0, stats=1), dict(half, trace_waves_per_cu=3)])

    def off(p, *names):
        return all(not p[n] for n in names)
    # one half of the bench frame: 4 147 200 rays / 160 = 25 920 waves wanted, 24 per CU allowed; 16 200 shading blocks wanted, 3 per CU for a piece
    assert bench_half["variant"] == "0100" and bench_half["packet"] and bench_half["quad_slots"] == 1036800
    assert (bench_half["shade_form"], bench_half["shade_form0"], bench_half["path_form"]) == (0, 0, 0) and bench_half["variant_name"] == "Pipe"   # k_shade<0u> on every bounce
    assert off(bench_half, "tail", "budget", "coop_all", "path")
    assert (bench_half["trace_blocks"], bench_half["shade_blocks"], bench_half["stream_blocks"]) == (6144, 768, 2048)
    # a solo 1/8 shard: 1 036 800 rays / 160 = 6480 waves wanted; the tail in place, so no budget
    assert eighth["variant"] == "0110" and (eighth["tail"], eighth["budget"]) == (4, 0)
    assert (eighth["trace_blocks"], eighth["shade_blocks"]) == (6144, 1024)
    assert no_tail["variant"] == "0100" and (no_tail["tail"], no_tail["budget"]) == (0, 48) and no_tail["coop_blocks"] == 256 * 32
    assert refill2["tail"] == 2
    # 64 x 36, 4 spp: 9216 rays, 23 mrad per pixel
    assert tiny["coop_all"] and tiny["coop_blocks"] == min(18432, 8192) == 8192 and off(tiny, "path", "packet")
    # 256 x 256, 1 spp: 65 536 rays in 1024 waves, the path kernel allows 16 per CU
    assert path["path"] and path["path_blocks"] == 1024 and not path["coop_all"]
    assert not trans["path"] and not trans["coop_all"]                                          # per bounce
    assert stats["variant"] == "1100" and off(stats, "tail", "budget") and stats["stats_lds_pad"]
    for m, v in ((mask, "0001"), (mask_stats, "1001")):
        assert m["variant"] == v and off(m, "pipe", "packet", "quad_slots", "tail", "budget", "coop_all", "path", "occ_probe", "coop_blocks", "packet_blocks", "path_blocks")
    assert mask_stats["stats_lds_pad"] and not mask["stats_lds_pad"]
    # without the one-round-trip step a CU takes 32 waves instead of 24
    assert no_pipe["variant"] == "0000" and no_pipe_stats["variant"] == "1000" and no_pipe["trace_blocks"] == no_pipe_stats["trace_blocks"] == 256 * 32
    assert pinned["trace_waves"] == max(8, (256 * 3) & ~7) == 768 and pinned["trace_blocks"] == 768


def test_the_exclusion_rules_hold_over_a_sweep(plan):
    rays = (1, 63, 64, 65, 2304, 32000, 32001, 120000, 120001, 3000000, 3000001, 8294400)
    flags = ("solo", "stats", "masked", "trans", "denoise")
    cases = []
    for n, bits, pp, tl, cr, pr in itertools.product(rays, itertools.product((0, 1), repeat=len(flags)), (0, 1, 2), (0, 4, 8),
                                                     (0, DEFAULT_COOP_RAYS), (0, DEFAULT_PATH_RAYS, MAX_RAYS)):
        cases.append(dict(frame(1920, 1080, 1), n_rays=n, n_slots=n, packet_primary=pp, tail_lanes=tl, coop_rays=cr, path_rays=pr, **dict(zip(flags, bits))))
    out = plan(cases)
    assert len(out) == len(rays) * 32 * 3 * 3 * 2 * 3
    for c, p in zip(cases, out):
        assert p["variant"] in VARIANTS, (c, p)
        st, pi, ta, ma = (ch == "1" for ch in p["variant"])
        assert (st, ma) == (bool(c["stats"]), bool(c["masked"])) and pi == bool(p["pipe"]) and ta == bool(p["tail"]), (c, p)
        if c["masked"]:
            assert not any(p[k] for k in ("pipe", "packet", "quad_slots", "tail", "budget", "occ_probe", "coop_all", "path")), (c, p)
        if c["stats"]:
            assert not any(p[k] for k in ("tail", "budget", "coop_all")), (c, p)
        if c["trans"] or p["coop_all"]:
            assert not p["path"], (c, p)
        if p["tail"]:
            assert not p["budget"], (c, p)
        assert p["stats_lds_pad"] == c["stats"], (c, p)
        assert 1 <= p["trace_blocks"] <= div_up(c["n_rays"], 64), (c, p)
        assert p["trace_waves"] % 8 == 0 and p["trace_waves"] >= 8 and p["trace_blocks"] == min(div_up(c["n_rays"], 64), p["trace_waves"]), (c, p)
        assert bool(p["coop_blocks"]) == bool(p["coop_all"] or p["budget"]) and bool(p["path_blocks"]) == bool(p["path"]) and bool(p["packet_blocks"]) == bool(p["packet"]), (c, p)


def test_the_shading_forms_are_the_facts_bits(plan):
    """kernel_forms.h's words as plan_wavefront states them, over every combination of the facts that pick a shading kernel, at a size that takes coop-all (9216 rays),
    one that takes the path kernel (65 536) and the full bench frame's"""
    facts = ("denoise", "env", "punct", "trans", "emis", "esamp", "nmap", "stats")
    bit = dict(env=ENV, punct=PUNCT, trans=TRANS, emis=EMIS, nmap=NMAP)
    sizes = (frame(64, 36, 4), frame(256, 256, 1), frame(3840, 2160, 1))
    assert [s["n_rays"] for s in sizes] == [9216, 65536, 8294400]
    cases = [dict(s, solo=1, **dict(zip(facts, bits))) for s in sizes for bits in itertools.product((0, 1), repeat=len(facts))]
    out = plan(cases)
    assert len(out) == 3 * 2 ** 8
    seen = set()
    for c, p in zip(cases, out):
        want = sum(b for k, b in bit.items() if c[k]) | (ESAMP if c["emis"] and c["esamp"] else 0)
        assert p["shade_form"] == want, (c, p)
        assert p["shade_form0"] == want | (GBUF if c["denoise"] else 0), (c, p)
        for form in (p["shade_form"], p["shade_form0"]):   # shade_form_valid
            assert form < 128 and (not form & ESAMP or form & EMIS), (c, p)
        if p["path"]:
            assert p["path_form"] == (GBUF if c["denoise"] else 0) | (ENV if c["env"] else 0) | (PUNCT if c["punct"] else 0), (c, p)
            assert not p["shade_form"] & (TRANS | EMIS | NMAP), (c, p)
        else:
            assert p["path_form"] == 0, (c, p)
        seen.add((c["n_rays"], bool(p["coop_all"]), bool(p["path"])))
    # the three sizes are what they are chosen for (stats keeps a tiny wavefront off coop-all, and it then takes the path kernel)
    assert {(9216, True, False), (65536, False, True), (8294400, False, False)} <= seen and not any(n == 8294400 and (co or pa) for n, co, pa in seen)
