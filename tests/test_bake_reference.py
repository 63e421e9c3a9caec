"""Host logic: instance baking (SPEC §2.5, §6) of the host (`bake_instance`, `woop_from_triangle`, through tests/tools/bake_check.cpp) and of the oracle
(`gltf_oracle.bake`, `orc_woop`, the brute-force `trace_closest`) against the binary64 reference tests/bake_ref.py — general rotation, non-uniform scale, shear, mirrors,
rank-deficient matrices, scales far from 1, a small object far from the origin — and against each other bit for bit.  Every bound is bake_ref's (derived; none measured).
The tests print their per-case report: run with -s to see it."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bake_ref as B
from oracle import gltf_oracle as G, orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "loupiote_amd", "csrc")
GROUPS = list(B.groups())


@pytest.fixture(scope="module")
def bake_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bake") / "bake_check")
    src = [os.path.join(ROOT, "tests", "tools", "bake_check.cpp")] + [os.path.join(CSRC, f) for f in ("scene.cpp", "bvh.cpp", "png.cpp", "jpeg.cpp", "gltf.cpp")]
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe] + src + ["-lpthread"], check=True)
    return exe


def oracle_scene(instances, ms):
    """the oracle's scene of [(mesh name, m16, ...)] over the meshes `ms`"""
    s = G.Scene()
    blas = {n: s.add_mesh(m["pos"], m["nrm"], m["uv"], m["idx"]) for n, m in ms.items()}
    for inst in instances:
        s.add_instance(blas[inst[0]], inst[1], 0)
    return s


def host_bake(exe, tmp_path, instances, ms):
    """tests/tools/bake_check over the same scene -> (vertices (3 nt,), Woop rows (nt, 3, 4))"""
    names = list(ms)
    path, out = str(tmp_path / "scene.bin"), str(tmp_path / "baked.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(names)))
        for n in names:
            m = ms[n]
            f.write(struct.pack("<II", m["pos"].shape[0], m["idx"].size))
            for a, dt in ((m["pos"], "<f4"), (m["nrm"], "<f4"), (m["uv"], "<f4"), (m["idx"], "<u4")):
                f.write(np.ascontiguousarray(a, dt).tobytes())
        f.write(struct.pack("<I", len(instances)))
        for inst in instances:
            f.write(struct.pack("<II", names.index(inst[0]), 0))
            f.write(np.ascontiguousarray(inst[1], "<f4").tobytes())
    subprocess.run([exe, path, out], check=True)
    raw = open(out, "rb").read()
    nt = struct.unpack_from("<I", raw, 0)[0]
    verts = np.frombuffer(raw, G.VERTEX_DT, 3 * nt, 4)
    rows = np.frombuffer(raw, "<f4", 12 * nt, 4 + 96 * nt).reshape(nt, 3, 4)
    return verts, rows


def oracle_rows(verts):
    nt = verts.shape[0] // 3
    p = np.ascontiguousarray(verts["position"][:, :3]).reshape(nt, 3, 3)
    rows = np.zeros((nt, 12), np.float32)
    L = orc.lib()
    for t in range(nt):
        L.orc_woop(orc._p(p[t, 0]), orc._p(p[t, 1]), orc._p(p[t, 2]), orc._p(rows[t]))
    return rows.reshape(nt, 3, 4)


def report(title, rep):
    print("\n%s" % title)
    for case, v in rep.items():
        print("  %-16s %s" % (case, "  ".join("%s %.3f" % kv for kv in v.items()) if isinstance(v, dict) else v))


@pytest.mark.parametrize("name", GROUPS)
def test_reference_excludes_little_and_compares_every_triangle(name):
    """the reference alone: at most 2 % of a case's rays and of its normal elements are excluded, every triangle of every case is compared at least once by a ray that
    must hit it (or, all of its triangles degenerate, must miss) and by a normal, the determinant's sign is certain, and no ray comes near another case's triangles"""
    g, tr, nm = B.reference(name)
    assert B.isolated(g)
    c = B.census(g, tr, nm)
    report("reference, scene %s" % name, c)
    for case, v in c.items():
        assert v["rays_excluded"] <= B.MAX_EXCLUDED and v["normals_excluded"] <= B.MAX_EXCLUDED, (case, v)
        assert v["least_rays_per_triangle"] >= 1 and v["least_normals_per_triangle"] >= 1, (case, v)


def test_reference_orientation_rule():
    """the reference's own rule: the two mirrors exchange vertices 1 and 2 and keep the normal on the mesh's front face; nothing else does"""
    ms = B.meshes()
    for name, a, t, unit in B.groups()["main"]:
        bt = B.baked_triangles(ms["octahedron"], B.matrix(a, t))
        assert bt["mirrored"] == (name in ("mirror-x", "minus-identity")), name
        if name not in ("identity", "rotation", "mirror-x", "minus-identity"):      # orthogonal 3x3 parts: angles are kept, so the side of a vertex normal is too
            continue
        P, N = bt["P"], bt["N"]
        ng = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
        centre = P.reshape(-1, 3).mean(0)
        assert np.all((ng * (P.mean(1) - centre)).sum(1) > 0), name                     # outward winding stays outward
        assert np.all((N * ng[:, None, :]).sum(-1) > 0), name                           # and the vertex normals stay on that side


@pytest.mark.parametrize("name", GROUPS)
def test_oracle_bake_and_brute_force_against_float64(name):
    g, tr, nm = B.reference(name)
    ms = B.meshes()
    verts, mats = G.bake(oracle_scene(g["instances"], ms))
    rep_b = B.check_bake(g, verts)
    rep_w = B.check_woop(g, verts, oracle_rows(verts))
    sc = orc.OracleScene(verts, mats, G.default_material(), B.dark_light(G.LIGHT_DT))
    rep_t = B.check_trace(g, tr, sc.trace_closest(g["o"], g["d"], brute_force=True))
    rep = {c: {"positions": rep_b[c][0], "normals": rep_b[c][1], "woop": rep_w[c], "tuv": rep_t[c]} for c in g["cases"]}
    report("oracle, worst |error| / bound (must stay below %g), scene %s" % (B.TOL, name), rep)
    assert B.passes(rep_b) and B.passes(rep_w) and B.passes(rep_t), rep


@pytest.mark.parametrize("name", GROUPS)
def test_host_bake_against_float64_and_equal_to_the_oracle(name, bake_check, tmp_path):
    g, tr, nm = B.reference(name)
    ms = B.meshes()
    verts, rows = host_bake(bake_check, tmp_path, g["instances"], ms)
    rep_b = B.check_bake(g, verts)
    rep_w = B.check_woop(g, verts, rows)
    rep = {c: {"positions": rep_b[c][0], "normals": rep_b[c][1], "woop": rep_w[c]} for c in g["cases"]}
    report("host, worst |error| / bound (must stay below %g), scene %s" % (B.TOL, name), rep)
    assert B.passes(rep_b) and B.passes(rep_w), rep
    overts, _ = G.bake(oracle_scene(g["instances"], ms))
    assert verts.tobytes() == overts.tobytes()
    assert rows.tobytes() == oracle_rows(overts).tobytes()


def test_outside_the_domain_bakes_stay_finite_and_equal(bake_check, tmp_path):
    """uniform scales 2^-60 and 2^60: no bound is claimed, only finite output and host == oracle"""
    ms = B.meshes()
    inst = [(mn, B.matrix(a), 0) for a in B.OUTSIDE.values() for mn in ms]
    verts, rows = host_bake(bake_check, tmp_path, inst, ms)
    overts, _ = G.bake(oracle_scene(inst, ms))
    assert np.all(np.isfinite(verts["position"])) and np.all(np.isfinite(verts["normal"])) and np.all(np.isfinite(rows))
    assert verts.tobytes() == overts.tobytes() and rows.tobytes() == oracle_rows(overts).tobytes()


def mirror_pairs(names=("rotation", "rotation-scale")):
    """(meshes, instances of the original meshes under M, instances of the mirror-image meshes under M·diag(−1, 1, 1)) for the named cases of the main scene"""
    ms = B.meshes()
    both = dict(ms)
    both.update({"mirror-" + n: B.mirror_mesh(m) for n, m in ms.items()})
    cases = [c for c in B.groups()["main"] if c[0] in names]
    plain = [(mn, B.matrix(a, t), 0) for _, a, t, _ in cases for mn in ms]
    mirrored = [("mirror-" + mn, B.mirror_matrix(m), 0) for mn, m, _ in plain]
    return both, plain, mirrored


def same_numbers(a, b):
    """equal as numbers: +0 == −0, everything else bit for bit"""
    return all(np.array_equal(a[f], b[f]) for f in ("position", "normal")) if a.dtype.names else np.array_equal(a, b)


def test_mirror_image_mesh_under_a_mirrored_node_bakes_to_the_same_bytes(bake_check, tmp_path):
    """SPEC §2.5's mirrored-instance rule pinned: the mirror image of a mesh (x negated, winding authored outward again, normals mirrored) under M·diag(−1, 1, 1) is the
    same object in the world as the mesh under M, and every sign flip on the way is exact: vertices, normals, uv and Woop rows are the same bytes, host and oracle.
    Exact for every number but a zero: a cofactor 0·a − 0·b is +0 under either sign of its zeros, so a matrix with exact zeros (the shear) can give a normal component −0
    where its mirror twin gives +0; there the two bakes are held equal as numbers"""
    for names, same in ((("rotation", "rotation-scale"), lambda a, b: a.tobytes() == b.tobytes()), (("shear",), same_numbers)):
        both, plain, mirrored = mirror_pairs(names)
        da, db = tmp_path / ("a" + names[0]), tmp_path / ("b" + names[0])
        da.mkdir(); db.mkdir()
        va, ra = host_bake(bake_check, da, plain, both)
        vb, rb = host_bake(bake_check, db, mirrored, both)
        assert va.shape[0] == 3 * 64 * len(names) and np.abs(ra).sum() > 0
        assert same(va, vb) and same(ra, rb), names
        oa, _ = G.bake(oracle_scene(plain, both))
        ob, _ = G.bake(oracle_scene(mirrored, both))
        assert same(oa, ob) and oa.tobytes() == va.tobytes() and ob.tobytes() == vb.tobytes(), names
