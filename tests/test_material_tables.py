"""Host logic: the derivation of the four per-triangle material side tables (loupiote_amd/csrc/material_tables.h: SPEC §20 alpha masks, §21 transmission,
§22 emission, §24 normal maps) and the residency of the plain images, on the CPU.  tests/tools/material_tables_check.cpp is compiled by g++ with the header and
scene.cpp (fail() and lpt_last_error()) under AddressSanitizer + UBSan, fed every case of this file in one run, and prints the tables as JSON.  Every expected
table is written out by hand from the rules, none is produced by the code under test.  Records are compared as the bit patterns of their four floats."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 0xFFFFFFFF
INVALID_ARG = 6
KINDS = ("alpha", "trans", "emis", "nmap")
PAIR_ONLY = "material 1 now %s was uploaded only as half of an (albedo, mra) pair: upload the scene again"


def F(x):
    """the bits of a float32"""
    return int(np.float32(x).view(np.uint32))


def tables(alpha=((), ()), trans=((), ()), emis=((), ()), nmap=((), ())):
    """the four tables as (records, per-triangle entries); a kind that is not named is empty"""
    return dict(zip(KINDS, ((list(map(list, recs)), list(tri)) for recs, tri in (alpha, trans, emis, nmap))))


GLASS_A, GLASS_B = [F(0.5), F(1.5), F(1.0), 0], [F(0.9), F(1.25), 0, 0]
TWO_GLASSES = ["scene 0 3", "trans 1 0.5 1.5 1", "trans 2 0.9 1.25 0"]

# name -> (commands before `derive`, expected tables | expected error text)
CASES = {
    "no feature anywhere": (["scene 1 2", "inst 0 0 2", "inst 1 2 2", "tris 4", "resident 1"], tables()),
    "one instance, one material with all four features": (
        ["scene 3 2", "mat 1 -1 -1 0.75 0", "alpha 1 1 0.5 0", "trans 1 0.625 1.33 0", "emis 1 1 0.5 0.25 1", "nmap 1 2 2.0", "inst 1 0 3", "tris 3", "resident 1 1 1"],
        tables(alpha=([[F(0.5), F(0.75), 0, 0]], [1, 1, 1]), trans=([[F(0.625), F(1.33), 0, 0]], [1, 1, 1]), emis=([[F(1.0), F(0.5), F(0.25), 1]], [1, 1, 1]),
               nmap=([[2, F(2.0), 0, 0]], [1, 1, 1]))),
    "two instances share one material: one record": (TWO_GLASSES + ["inst 1 0 2", "inst 1 2 1", "tris 3"], tables(trans=([GLASS_A], [1, 1, 1]))),
    "records in the order of first use by instance: B, A": (
        TWO_GLASSES + ["inst 2 0 1", "inst 1 1 2", "inst 0 3 1", "inst 2 4 1", "tris 5"], tables(trans=([GLASS_B, GLASS_A], [1, 2, 2, 0, 1]))),
    "a zero-triangle instance of a feature material: no record, no allocation": (TWO_GLASSES + ["inst 1 0 0", "inst 0 0 2", "tris 2"], tables()),
    "a material index past the end is material 0": (
        ["scene 0 2", "trans 0 0.5 1.5 1", "inst 7 0 2", "inst 1 2 1", "inst -1 3 1", "tris 4"], tables(trans=([GLASS_A], [1, 1, 0, 1]))),
    "no baked triangle at all, yet a record: one entry": (TWO_GLASSES + ["inst 1 0 1", "tris 0"], tables(trans=([GLASS_A], [1]))),
    "an instance range past the baked triangles": (TWO_GLASSES + ["inst 0 0 2", "inst 1 2 3", "tris 4"], "instance 1 lies beyond the baked triangles"),
    "alpha and emission keep a record without their out-of-range image, a normal map has none": (
        ["scene 1 2", "alpha 1 1 0.25 5", "emis 1 2 0 0 9", "nmap 1 3 1.0", "inst 1 0 1", "tris 1", "resident 1"],
        tables(alpha=([[F(0.25), F(1.0), INVALID, 0]], [1]), emis=([[F(2.0), 0, 0, INVALID]], [1]))),
    "... and without an image at all": (
        ["scene 1 2", "alpha 1 1 0.25 -1", "emis 1 0 0 3 -1", "nmap 1 -1 1.0", "inst 1 0 1", "tris 1", "resident 1"],
        tables(alpha=([[F(0.25), F(1.0), INVALID, 0]], [1]), emis=([[0, 0, F(3.0), INVALID]], [1]))),
    "a mask image resident only as half of a pair": (["scene 2 2", "alpha 1 1 0.5 0", "inst 1 0 1", "tris 1", "resident 0 1"], PAIR_ONLY % "masks with an image that"),
    "an emissive image resident only as half of a pair": (["scene 2 2", "emis 1 1 1 1 0", "inst 1 0 1", "tris 1", "resident 0 1"], PAIR_ONLY % "emits with an image that"),
    "a normal image resident only as half of a pair": (["scene 2 2", "nmap 1 0 1.0", "inst 1 0 1", "tris 1", "resident 0 1"], PAIR_ONLY % "has a normal map whose image"),
    "an image beyond the residency flags is not resident": (["scene 2 2", "nmap 1 1 1.0", "inst 1 0 1", "tris 1", "resident 1"], PAIR_ONLY % "has a normal map whose image"),
    "the first error in the order of the kinds": (
        ["scene 2 2", "nmap 1 0 1.0", "alpha 1 1 0.5 0", "emis 1 1 1 1 0", "inst 1 0 1", "tris 1", "resident 0 1"], PAIR_ONLY % "masks with an image that"),
    "transmission names no image": (TWO_GLASSES + ["inst 1 0 1", "tris 1", "resident 0 0"], tables(trans=([GLASS_A], [1]))),
    "the other half of the pair is resident: no error": (
        ["scene 2 2", "alpha 1 1 0.5 1", "emis 1 1 1 1 1", "nmap 1 1 1.0", "inst 1 0 1", "tris 1", "resident 0 1"],
        tables(alpha=([[F(0.5), F(1.0), 1, 0]], [1]), emis=([[F(1.0), F(1.0), F(1.0), 1]], [1]), nmap=([[1, F(1.0), 0, 0]], [1]))),
    "a layout shorter than the instance list: the tail is ignored": (TWO_GLASSES + ["inst 1 0 2", "inst 2", "tris 2"], tables(trans=([GLASS_A], [1, 1]))),
}

# Residency.  Fourteen images: (0, 1) a pair and nothing else — a mask switched off and an emission of zero name them and do not count; (2, 3), (4, 5), (6, 7) pairs
# of which a mask names 2, an emission 5, a normal map 6; 8 a mask image in no pair; 9 referenced by nothing; (10, 11) two textures that are no pair; (12, 13) a
# pair whose albedo another material samples on its own; a mask image out of range names nothing.
RESIDENCY = ["scene 14 9", "mat 1 0 1 1 1", "alpha 1 0 0.5 0", "emis 1 0 0 0 1", "trans 1 1 1.5 1", "mat 2 2 3 1 1", "alpha 2 1 0.5 2", "mat 3 4 5 1 1", "emis 3 0 0.5 0 5",
             "mat 4 6 7 1 1", "nmap 4 6 1.0", "alpha 5 1 0.5 8", "mat 6 10 11 1 0", "mat 7 12 -1 1 0", "mat 8 12 13 1 1", "alpha 8 1 0.5 99"]
RESIDENT = [0, 0, 1, 0, 0, 1, 1, 0, 1, 1, 1, 1, 1, 0]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("mattab") / "material_tables_check")
    src = [os.path.join(ROOT, "tests", "tools", "material_tables_check.cpp"), os.path.join(ROOT, "loupiote_amd", "csrc", "scene.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include")] + src + ["-o", exe])
    lines = [l for cmds, _ in CASES.values() for l in cmds + ["derive"]] + RESIDENCY + ["residency"]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:allocator_may_return_null=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0 and not p.stderr, (p.stdout[-2000:], p.stderr[-4000:])       # clean under the sanitizers
    out = [json.loads(l) for l in p.stdout.splitlines()]
    assert len(out) == len(CASES) + 1
    return dict(zip(CASES, out[:-1])), out[-1]


@pytest.mark.parametrize("name", list(CASES))
def test_derivation(results, name):
    got, want = results[0][name], CASES[name][1]
    assert [t["section"] for t in got["tables"]] == [20, 21, 22, 24]
    if isinstance(want, str):
        assert got["status"] == INVALID_ARG and got["error"] == want
        return
    assert got["status"] == 0 and got["error"] == ""
    assert {k: (t["recs"], t["tri"]) for k, t in zip(KINDS, got["tables"])} == want


def test_residency_of_the_plain_images(results):
    assert results[1]["resident"] == RESIDENT
