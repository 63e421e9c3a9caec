"""Host logic: SPEC.md §27's fact in the launch plan (loupiote_amd/csrc/launch_plan.h plan_wavefront), checked on the CPU through tests/tools/plan_check.cpp.
`glass_shadow` excludes what `masked` excludes — pipe, packet, tail, budget, occluder probe, coop-all, path — at every size class and picks k_trace_glass<STATS>;
with the fact false the plan is the plan of a case that never names the field, field for field, and its kernel is one of the eight k_trace
instantiations, by name what the bit string says."""
import itertools
import json
import os
import subprocess

import pytest

from test_launch_plan import DEFAULT_COOP_RAYS, DEFAULT_PATH_RAYS, MAX_RAYS, frame, limits   # noqa: F401 (limits: the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAYS = (1, 63, 64, 65, 2304, 32000, 32001, 120000, 120001, 3000000, 3000001, 8294400)      # the size classes test_launch_plan.py sweeps
EXCLUDED = ("pipe", "packet", "quad_slots", "tail", "budget", "occ_probe", "coop_all", "path", "coop_blocks", "packet_blocks", "path_blocks")
CODES = {"0000": "Lane", "0100": "Pipe", "1000": "Stats", "1100": "StatsPipe", "0010": "Tail", "0110": "PipeTail", "0001": "Mask", "1001": "StatsMask"}


def _build(tmp_path_factory, source):
    exe = str(tmp_path_factory.mktemp("plan_glass") / source.replace(".cpp", ""))
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "tools", source)], check=True)
    return exe


def _run(exe, limits, cases):
    lines = [" ".join("%s=%s" % kv for kv in dict(limits, cus=256, **c).items()) for c in cases]
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = [json.loads(l) for l in p.stdout.splitlines()]
    assert len(out) == len(cases)
    return out


@pytest.fixture(scope="module")
def plan(tmp_path_factory, limits):
    exe = _build(tmp_path_factory, "plan_check.cpp")
    return lambda cases: _run(exe, limits, cases)


@pytest.fixture(scope="module")
def old_plan(plan):
    return plan   # one driver since it knows every fact: the case that never names the field, by the bit strings of the eight k_trace instantiations


def _sweep():
    flags = ("solo", "stats", "masked", "trans", "denoise")
    cases = []
    for n, bits, pp, tl, cr, pr in itertools.product(RAYS, itertools.product((0, 1), repeat=len(flags)), (0, 1, 2), (0, 4), (0, DEFAULT_COOP_RAYS), (0, DEFAULT_PATH_RAYS, MAX_RAYS)):
        cases.append(dict(frame(1920, 1080, 1), n_rays=n, n_slots=n, packet_primary=pp, tail_lanes=tl, coop_rays=cr, path_rays=pr, punct=1, **dict(zip(flags, bits))))
    return cases


def test_glass_shadow_excludes_what_masked_excludes_at_every_size(plan):
    cases = _sweep()
    on = plan([dict(c, glass_shadow=1) for c in cases])
    as_masked = plan([dict(c, masked=1) for c in cases])
    assert len(on) == len(RAYS) * 32 * 3 * 2 * 2 * 3
    for c, p, m in zip(cases, on, as_masked):
        assert p["variant_name"] == ("StatsGlass" if c["stats"] else "Glass"), (c, p)
        assert not any(p[k] for k in EXCLUDED), (c, p)
        assert p["stats_lds_pad"] == c["stats"], (c, p)
        # everything but the kernel's name is the masked scene's plan: the same step, the same grids
        assert {k: v for k, v in p.items() if not k.startswith("variant")} == {k: v for k, v in m.items() if not k.startswith("variant")}, (c, p, m)
        assert m["variant_name"] == ("StatsMask" if c["stats"] else "Mask")


def test_with_the_fact_false_the_plan_is_the_plan_without_the_field(plan, old_plan):
    cases = _sweep()
    unset, off, before = plan(cases), plan([dict(c, glass_shadow=0) for c in cases]), old_plan(cases)
    assert unset == off
    for c, p, b in zip(cases, unset, before):
        assert p["variant_name"] == CODES[b["variant"]] and p["variant_index"] < 8, (c, p, b)
        for k, v in b.items():
            if k not in ("variant", "same_again"):
                assert p[k] == v, (k, c, p, b)


def test_named_cases(plan):
    shard = dict(frame(1920, 1080, 4, parts=8), solo=1, punct=1, trans=1)
    tiny = dict(frame(64, 64, 16), solo=1, punct=1, trans=1)
    a, b, c, d = plan([dict(shard, glass_shadow=1), shard, dict(tiny, glass_shadow=1), tiny])
    assert a["variant_name"] == "Glass" and a["tail"] == 0 and b["variant_name"] == "PipeTail" and b["tail"] == 4 and b["packet"]
    # 64 x 64 x 16 = 65 536 rays: 409 waves wanted, at least 8 per CU (2048) taken, capped by one wave per 64 rays (1024)
    assert c["variant_name"] == "Glass" and c["trace_blocks"] == min(1024, 256 * 8) and not c["path"] and not c["coop_all"]
    assert d["variant_name"] == "PipeTail"
