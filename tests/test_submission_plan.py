"""Host logic: how a submission leaves for the GPU — where the recorded batch is cut, which lane and ticket every piece takes, and the order of the pieces'
halves and stages with the events they wait for and record (loupiote_amd/csrc/submission_plan.h plan_submission), checked on the CPU through
tests/tools/submission_check.cpp: named cases whose plans are worked out by hand from the rules, the invariants of the step list as properties over a sweep
of frames, shards, batches and knobs, and purity (every case is planned twice, in the program and from here)."""
import itertools
import json
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVEFRONT_RAYS, SPLIT_RAYS = 1 << 22, 3000000      # device.hip kWavefrontRays, kSplitRays


def div_up(a, b):
    return (a + b - 1) // b


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("submission") / "submission_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "tools", "submission_check.cpp")], check=True)

    def run(cases):
        """cases: dicts of SubmissionFacts fields; every case is planned twice and the two answers must be the same"""
        lines = [" ".join("%s=%d" % kv for kv in c.items()) for c in cases]
        p = subprocess.run([exe], input="\n".join(lines + lines) + "\n", capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        out = [json.loads(l) for l in p.stdout.splitlines()]
        assert len(out) == 2 * len(cases) and out[:len(cases)] == out[len(cases):]
        assert all(o["same_again"] == 1 for o in out)
        return out[:len(cases)]
    return run


def facts(w, h, n, world=1, tile=(32, 8), **more):
    """rank 0 of `world` ranks of a w x h frame (tile t belongs to rank t mod world) with n recorded samples; the library's defaults for the rest"""
    tiles_x, tiles_y = div_up(w, tile[0]), div_up(h, tile[1])
    f = dict(n_slots=div_up(tiles_x * tiles_y, world) * tile[0] * tile[1], tiles_x=tiles_x, tile_w=tile[0], tile_h=tile[1], world=world, height=h, n=n, max_fused=0,
             pathtrace=1, wavefront_rays=WAVEFRONT_RAYS, split_rays=SPLIT_RAYS, n_lanes=2, lane_phase=1, bounces=8, lane_rr=0, read=0)
    f.update(more)
    return f


def P(k):
    return ["P", k]


def F(k):
    return ["F", k]


def S(k, t, wait_start=None, wait_trav=None, record=0):
    return ["S", k, t, wait_start, wait_trav, record]


def free_order(pieces, ahead, bounces):
    """the un-phased order: piece by piece, every stage without waits or records, the second half of the piece that held the ticket first"""
    steps = []
    for k in range(pieces):
        steps += ([F(k - ahead)] if k >= ahead else []) + [P(k)] + [S(k, t) for t in range(bounces + 1)]
    return steps + [F(k) for k in range(max(pieces - ahead, 0), pieces)]


# ---------------------------------------------------------------- named cases
def test_the_bench_frame(plan):
    # 1920x1080, 32x8 tiles: 60 x 135 tiles, a granule = one tile row = 60 * 256 = 15 360 slots, 135 granules, 2 073 600 slots x 4 samples = 8 294 400 rays > 4 194 304.
    # fit = 4 194 304 // (15 360 * 4 = 61 440) = 68; pieces = max(2, ceil(135 / 68) = 2) = 2; evened out: ceil(135 / 2) = 68 tile rows, then the 67 left.
    # rows: 68 * 8 = 544 and min(1080, 135 * 8) = 1080.  Two lanes: ahead 2, one group of two; phase 1: stage 0 of piece 1 waits for trav[0] of piece 0.
    f = facts(1920, 1080, 4, read=1)
    assert f["n_slots"] * 4 == 8294400
    out, = plan([f])
    assert out["pieces"] == [[0, 68 * 15360, 0, 544, 0, 0, 0], [68 * 15360, 67 * 15360, 544, 1080, 1, 1, 0]]
    assert out["lane_rr"] == 2 and out["trav_events"] == 9
    assert out["steps"] == [P(0), P(1)] + [s for t in range(9) for s in (S(0, t, record=1), S(1, t, [0, 0] if t == 0 else None, record=1))] + [F(0), F(1)]
    # without a read-back the pieces are the same and carry no rows
    out, = plan([facts(1920, 1080, 4)])
    assert out["pieces"] == [[0, 68 * 15360, 0, 0, 0, 0, 0], [68 * 15360, 67 * 15360, 0, 0, 1, 1, 0]]


def test_half_a_shard_of_the_bench_frame(plan):
    # world 2: rank 0 owns 8100 / 2 = 4050 tiles = 1 036 800 slots, x 4 = 4 147 200 rays: below wavefront_rays, above split_rays (3 M) — two pieces on two lanes.
    # granule = one tile (256 slots); fit = 4 194 304 // 1024 = 4096; pieces = max(2, ceil(4050 / 4096) = 1) = 2 of 2025 tiles = 518 400 slots.  No rows: a sharded frame.
    two, one, off = plan([facts(1920, 1080, 4, world=2, read=1), facts(1920, 1080, 4, world=2, read=1, n_lanes=1), facts(1920, 1080, 4, world=2, split_rays=0)])
    assert two["pieces"] == [[0, 518400, 0, 0, 0, 0, 0], [518400, 518400, 0, 0, 1, 1, 0]]
    assert two["steps"][:4] == [P(0), P(1), S(0, 0, record=1), S(1, 0, [0, 0], record=1)] and two["steps"][-2:] == [F(0), F(1)]
    for whole in (one, off):      # one lane, or LPT_EXP_SPLIT_RAYS 0: the wavefront that holds them all
        assert whole["pieces"] == [[0, 1036800, 0, 0, 0, 0, 1]] and whole["steps"] == free_order(1, whole is off and 2 or 1, 8)
    assert (one["lane_rr"], off["lane_rr"]) == (0, 1)


def test_the_lane_phase_frame(plan):
    # tests/test_gpu_lane_phase.py: 480x272, 15 x 34 tiles, a tile row = 3840 slots, CUT_RAYS = 17 * 15 * 256 * 4 + 1000 = 262 120; 130 560 slots x 4 = 522 240 rays.
    # fit = 262 120 // 15 360 = 17; pieces = max(2, ceil(34 / 17)) = 2 of 17 tile rows = 65 280 slots, rows [0, 136) and [136, 272).
    cut = 17 * 15 * 256 * 4 + 1000
    assert cut == 262120
    pieces = [[0, 65280, 0, 136, 0, 0, 0], [65280, 65280, 136, 272, 1, 1, 0]]
    free, offset, alternating, one_lane = plan([facts(480, 272, 4, wavefront_rays=cut, read=1, lane_phase=ph) for ph in (0, 1, 2)] +
                                               [facts(480, 272, 4, wavefront_rays=cut, read=1, lane_phase=2, n_lanes=1)])
    assert free["pieces"] == offset["pieces"] == alternating["pieces"] == pieces
    assert free["steps"] == free_order(2, 2, 8) and free["trav_events"] == 0
    assert offset["steps"] == [P(0), P(1)] + [s for t in range(9) for s in (S(0, t, record=1), S(1, t, [0, 0] if t == 0 else None, record=1))] + [F(0), F(1)]
    # alternating traversal: piece 1's traversal t behind piece 0's traversal t, piece 0's traversal t behind piece 1's traversal t - 1
    assert alternating["steps"] == ([P(0), P(1), S(0, 0, record=1), S(1, 0, None, [0, 0], 1)] +
                                    [s for t in range(1, 9) for s in (S(0, t, None, [1, t - 1], 1), S(1, t, None, [0, t], 1))] + [F(0), F(1)])
    assert alternating["trav_events"] == 9
    assert one_lane["pieces"] == [p[:4] + [0, 0, 0] for p in pieces] and one_lane["steps"] == free_order(2, 1, 8) and one_lane["lane_rr"] == 0


def test_the_cuts_of_the_deferred_suite(plan):
    # tests/test_gpu_deferred.py: 203x117, 7 x 15 tiles, wavefront_rays = 3 * 256 * 7 * 4 = 21 504 = three tile rows (1792 slots each) of 4 samples:
    # fit = 3, pieces = ceil(15 / 3) = 5 of 3 tile rows = 5376 slots, rows 24 each, the last to min(117, 120)
    rays = 3 * 256 * 7 * 4
    two, one = plan([facts(203, 117, 4, wavefront_rays=rays, read=1, bounces=5, n_lanes=l) for l in (2, 1)])
    assert [p[:4] for p in two["pieces"]] == [[k * 5376, 5376, 24 * k, min(117, 24 * k + 24)] for k in range(5)] == [p[:4] for p in one["pieces"]]
    assert [p[4:] for p in two["pieces"]] == [[k % 2, k % 2, 0] for k in range(5)] and two["lane_rr"] == 5
    assert [p[4:] for p in one["pieces"]] == [[0, 0, 0]] * 5 and one["steps"] == free_order(5, 1, 5)
    # groups {0, 1}, {2, 3}, {4}: the second halves of a group's predecessors in front of its first halves
    stage = lambda k0, k1: [S(k, t, [k - 1, 0] if (t == 0 and k > k0) else None, None, 1) for t in range(6) for k in range(k0, k1)]
    assert two["steps"] == [P(0), P(1)] + stage(0, 2) + [F(0), P(2), F(1), P(3)] + stage(2, 4) + [F(2), P(4)] + stage(4, 5) + [F(3), F(4)]
    # 97x301, 3 lanes: 4 x 38 tiles, wavefront_rays = 3 * 256 * 4 * 4 = 12 288 = three tile rows (1024 slots each): fit 3, ceil(38 / 3) = 13 pieces, ceil(38 / 13) = 3 rows each, the last 2
    three, = plan([facts(97, 301, 4, wavefront_rays=3 * 256 * 4 * 4, read=1, bounces=5, n_lanes=3, lane_rr=2)])
    assert [p[:4] for p in three["pieces"]] == [[k * 3072, 3072 if k < 12 else 2048, 24 * k, min(301, 24 * k + 24)] for k in range(13)]
    assert [p[4:] for p in three["pieces"]] == [[(2 + k) % 3, k % 3, 0] for k in range(13)] and three["lane_rr"] == 15


def test_one_piece(plan):
    # the explicit batch (max_fused >= 1, raytrace_n): one wavefront whatever its size; a denoising mode: one piece on lane 0 with ahead 1; nothing owned: one empty wavefront
    fused, denoise, empty, empty_denoise = plan([facts(1920, 1080, 4, max_fused=4, read=1, lane_rr=1), facts(1920, 1080, 4, pathtrace=0, read=1, lane_rr=1),
                                                 facts(1920, 1080, 4, n_slots=0, world=8, lane_rr=3), facts(1920, 1080, 1, n_slots=0, world=8, pathtrace=0, lane_rr=3)])
    assert fused["pieces"] == [[0, 2073600, 0, 1080, 1, 0, 1]] and fused["lane_rr"] == 2
    assert denoise["pieces"] == [[0, 2073600, 0, 0, 0, 0, 1]] and denoise["lane_rr"] == 1
    for out in (fused, denoise):
        assert out["steps"] == [P(0)] + [S(0, t) for t in range(9)] + [F(0)] and out["trav_events"] == 0
    assert empty["pieces"] == [[0, 0, 0, 0, 1, 0, 1]] and empty["steps"] == [P(0), F(0)] and empty["lane_rr"] == 4      # the empty wavefront takes its turn on the lanes too
    assert empty_denoise["pieces"] == [[0, 0, 0, 0, 0, 0, 1]] and empty_denoise["steps"] == [P(0), F(0)] and empty_denoise["lane_rr"] == 3


# ---------------------------------------------------------------- properties
SIZES = [(96, 72), (203, 117), (97, 301), (33, 9), (480, 272), (64, 8), (250, 100)]
AXES = dict(size=SIZES, tile=[(32, 8), (16, 16)], world=[1, 2, 8], n=[1, 2, 3, 4, 7, 16, 64], n_lanes=[1, 2, 3, 4], lane_phase=[0, 1, 2],
            wavefront_rays=[64, 5000, 20000, 262120, WAVEFRONT_RAYS], split_rays=[0, SPLIT_RAYS, 30000], fused=[0, 1], read=[0, 1], pathtrace=[0, 1], lane_rr=[0, 1, 2, 3], bounces=[0, 1, 3])


def sweep():
    rnd = random.Random(20)
    cases = [{k: rnd.choice(v) for k, v in AXES.items()} for _ in range(6000)]
    for k, v in AXES.items():      # every value of every axis is there
        assert {c[k] for c in cases} == set(v), k
    return [facts(c["size"][0], c["size"][1], c["n"], c["world"], c["tile"], n_lanes=c["n_lanes"], lane_phase=c["lane_phase"], wavefront_rays=c["wavefront_rays"], split_rays=c["split_rays"],
                  max_fused=c["n"] if c["fused"] else 0, read=c["read"], pathtrace=c["pathtrace"], lane_rr=c["lane_rr"], bounces=c["bounces"]) for c in cases]


@pytest.fixture(scope="module")
def swept(plan):
    cases = sweep()
    return list(zip(cases, plan(cases)))


def test_the_pieces_partition_the_slots_in_whole_granules(swept):
    seen = set()
    for f, out in swept:
        pieces = out["pieces"]
        granule = f["tile_w"] * f["tile_h"] * (f["tiles_x"] if f["world"] == 1 else 1)
        assert f["n_slots"] % granule == 0 and pieces
        at = 0
        for slot0, n, *_ in pieces:
            assert slot0 == at and n % granule == 0 and n > 0
            at += n
        assert at == f["n_slots"]
        assert len({p[1] for p in pieces[:-1]}) <= 1 and pieces[-1][1] <= pieces[0][1]
        assert all(p[6] == (len(pieces) == 1) for p in pieces)                                   # solo
        early = f["read"] and f["world"] == 1 and f["pathtrace"]
        if early:
            assert pieces[0][2] == 0 and pieces[-1][3] == f["height"]
            assert all(a[3] == b[2] for a, b in zip(pieces, pieces[1:])) and all(p[2] < p[3] for p in pieces)
        else:
            assert all(p[2:4] == [0, 0] for p in pieces)
        laned = f["pathtrace"] and f["n_lanes"] > 1
        assert [p[4] for p in pieces] == [(f["lane_rr"] + k) % f["n_lanes"] if laned else 0 for k in range(len(pieces))]
        assert out["lane_rr"] == f["lane_rr"] + (len(pieces) if laned else 0)
        if f["max_fused"] or not f["pathtrace"]:
            assert len(pieces) == 1
        seen.add((min(len(pieces), 9), bool(early)))
    assert {n for n, _ in seen} == set(range(1, 10))                                             # the sweep cuts into one piece, two, ... and many


def test_every_wait_names_an_event_recorded_before_and_not_since(swept):
    waits = 0
    for f, out in swept:
        pieces, last = out["pieces"], {}
        for step in out["steps"]:
            if step[0] != "S":
                continue
            _, k, t, wait_start, wait_trav, record = step
            for w in (wait_start, wait_trav):
                if w is not None:
                    assert last.get((pieces[w[0]][4], w[1])) == w[0], (f, step)                  # trav[w[1]] of that piece's lane: the latest record is that piece's
                    waits += 1
            if record:
                last[(pieces[k][4], t)] = k
        assert out["trav_events"] == (f["bounces"] + 1 if any(s[0] == "S" and s[5] for s in out["steps"]) else 0)
    assert waits > 10000


def test_every_piece_has_its_steps_once_and_in_order(swept):
    for f, out in swept:
        pieces, steps = out["pieces"], out["steps"]
        at = {}
        for i, step in enumerate(steps):
            assert tuple(step[:3] if step[0] == "S" else step[:2]) not in at
            at[tuple(step[:3] if step[0] == "S" else step[:2])] = i
        stages = f["bounces"] + 1
        for k, p in enumerate(pieces):
            order = [at[("P", k)]] + [at[("S", k, t)] for t in range(stages if p[1] else 0)] + [at[("F", k)]]
            assert order == sorted(order)
        assert len(at) == sum(2 + (stages if p[1] else 0) for p in pieces)
        finishes = [s[1] for s in steps if s[0] == "F"]
        assert finishes == list(range(len(pieces)))


def test_a_lane_and_a_ticket_hold_one_piece_at_a_time(swept):
    most = 0
    for f, out in swept:
        pieces, open_ = out["pieces"], []
        for step in out["steps"]:
            if step[0] == "P":
                assert all(pieces[k][4] != pieces[step[1]][4] and pieces[k][5] != pieces[step[1]][5] for k in open_), (f, step)
                open_.append(step[1])
                assert len(open_) <= f["n_lanes"]
                most = max(most, len(open_))
            elif step[0] == "F":
                open_.remove(step[1])
            else:
                assert step[1] in open_
        assert not open_
    assert most == 4


def groups_of(f, out):
    """(phase in effect, ahead, the groups of pieces that are enqueued stage by stage)"""
    n = len(out["pieces"])
    ahead = f["n_lanes"] if (f["pathtrace"] and f["n_lanes"] > 1) else 1
    phase = f["lane_phase"] if (ahead > 1 and n > 1) else 0
    size = ahead if phase else 1
    return phase, ahead, [list(range(k0, min(n, k0 + size))) for k0 in range(0, n, size)]


def test_without_a_phase_the_order_is_the_free_one(swept):
    n = 0
    for f, out in swept:
        phase, ahead, _ = groups_of(f, out)
        if phase == 0 and out["pieces"][0][1]:
            assert out["steps"] == free_order(len(out["pieces"]), ahead, f["bounces"]), f
            n += 1
    assert n > 1000


def test_a_group_is_enqueued_stage_by_stage_with_the_three_hook_rules(swept):
    seen = set()
    for f, out in swept:
        phase, ahead, groups = groups_of(f, out)
        if not phase:
            continue
        pieces, steps = out["pieces"], out["steps"]
        stages = f["bounces"] + 1
        expect = []
        for g in groups:
            assert len({pieces[k][4] for k in g}) == len(g)                                      # side by side: distinct lanes
            for k in g:
                expect += ([F(k - ahead)] if k >= ahead else []) + [P(k)]
            for t in range(stages):
                for k in g:
                    prev = k - 1 if k > g[0] else g[-1]
                    start = [prev, 0] if (phase == 1 and t == 0 and k > g[0]) else None
                    trav = ([prev, t] if k > g[0] else ([prev, t - 1] if t > 0 else None)) if phase == 2 else None
                    expect.append(S(k, t, start, trav, 1))
            seen.add((phase, len(g)))
        expect += [F(k) for k in range(max(len(pieces) - ahead, 0), len(pieces))]
        assert steps == expect, f
    assert seen == {(ph, n) for ph in (1, 2) for n in (1, 2, 3, 4)}                              # single-member groups (the last of an odd cut) among them


def test_alternating_traversal_is_one_traversal_grid_at_a_time(swept):
    n = 0
    for f, out in swept:
        phase, _, groups = groups_of(f, out)
        if phase != 2:
            continue
        stage_steps = [s for s in out["steps"] if s[0] == "S"]
        for g in groups:
            mine = [s for s in stage_steps if s[1] in g]
            assert mine[0][4] is None
            for a, b in zip(mine, mine[1:]):
                assert b[4] == [a[1], a[2]]                                                      # a traversal launch waits for the one enqueued just before it: a chain
            assert [s[1] for s in mine] == g * (f["bounces"] + 1)                                # between two turns of a piece every other member has had its own
            n += 1
    assert n > 500
