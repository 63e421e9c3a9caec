"""-m gpu: instance baking on the device (SPEC §2.5, §6; `k_bake_instance`, `woop_device`) and on the host, as the probes see it, against the binary64 reference
tests/bake_ref.py: every case of the reference — general rotation, non-uniform scale, shear, mirrors, rank-deficient matrices, scales far from 1, a small object far
from the origin — uploaded through the four build paths (host-built; gpu_build; uploaded at identity, then update_instances; rebuild).  `trace_closest` must name the
reference's prim and (t, u, v) within bounds, `shading_normal` must be within bounds from both sides of every triangle, and the four paths must answer the same bytes.
Every bound is bake_ref's (derived; none measured).  The tests print their per-case report: run with -s to see it."""
import numpy as np
import pytest

import bake_ref as B
import loupiote_amd as lp
from loupiote_amd import testing as T

pytestmark = pytest.mark.gpu
PATHS = ("host", "gpu_build", "update", "rebuild")
IDENTITY = np.eye(4, dtype=np.float32).reshape(16)


def product_scene(instances, ms, at_identity=False):
    """the product's scene of [(mesh name, m16, ...)]: the mapped half of the patch under a material with the 5x3 normal map, the octahedron solid glass.
    -> (scene, [instance index])"""
    s = lp.Scene()
    s.set_light(0, B.dark_light(lp._abi.LIGHT_DT))
    img = s.add_image(B.normal_image())
    plain = s.add_material((0.8, 0.8, 0.8, 1.0), 0.7, 0.0)
    mapped = s.add_material((0.8, 0.7, 0.6, 1.0), 0.6, 0.0)
    s.set_material_normal_map(mapped, img, B.NORMAL_SCALE)
    glass = s.add_material((0.9, 0.95, 1.0, 1.0), 0.2, 0.0)
    s.set_material_transmission(glass, 1.0, 1.5, False)
    mat = {"patch-mapped": mapped, "patch-plain": plain, "octahedron": glass}
    blas = {n: s.add_mesh(m["pos"], m["nrm"], m["uv"], m["idx"]) for n, m in ms.items()}
    idx = [s.add_instance(blas[i[0]], IDENTITY if at_identity else i[1], mat[i[0].replace("mirror-", "")]) for i in instances]
    return s, idx


def upload(device, path, instances, ms):
    """one of the four build paths -> (scene, scene on the device, instance indices)"""
    s, idx = product_scene(instances, ms, at_identity=path in ("update", "rebuild"))
    sg = lp.SceneGPU.new_from_scene(s, device, gpu_build=path == "gpu_build")
    if path in ("update", "rebuild"):
        for i, inst in zip(idx, instances):
            s.set_instance_transform(i, inst[1])
        if path == "update":
            sg.update_instances(s)
        else:
            sg.rebuild(s)
    return s, sg, idx


def probes(sg, g, nm):
    return sg.trace_closest(g["o"], g["d"]), sg.shading_normal(nm["prim"], nm["bary"], nm["d"])


def report(title, rep):
    print("\n%s" % title)
    for case, v in rep.items():
        print("  %-16s %s" % (case, "  ".join("%s %.3f" % kv for kv in v.items())))


@pytest.mark.parametrize("name", list(B.groups()))
def test_four_build_paths_against_float64(device, name):
    """Measured on an MI355X (the four paths answer the same bytes, so one figure each), worst |error| / bound against the limit of 2: (t, u, v) 0.39 identity and both
    uniform scales, 0.48 rotation, 0.47 rotation x scale, 0.55 shear, 0.46 mirror, 0.53 minus identity, 0.11 rank 2, 0.44 far; shading normal 0.16 - 0.19, 0.09 rank 2;
    rank 1 and zero: every ray a miss, every normal zero.  The test prints the table"""
    g, tr, nm = B.reference(name)
    ms = B.meshes()
    first, rep = None, {c: {} for c in g["cases"]}
    for path in PATHS:
        s, sg, _ = upload(device, path, g["instances"], ms)
        assert sg.stats().triangles == g["tris"]["P"].shape[0]
        hits, (ns, mapped) = probes(sg, g, nm)
        sg.close()
        rt, rn = B.check_trace(g, tr, hits), B.check_normals(g, nm, ns, mapped)
        for c in g["cases"]:
            rep[c].update({path + " tuv": rt[c], path + " Ns": rn[c]})
        assert B.passes(rt) and B.passes(rn), (path, rt, rn)
        got = (hits.tobytes(), ns.tobytes(), mapped.tobytes())
        first = first or got
        assert got == first, "%s differs from the host-built upload" % path              # kernels.h: the device bake is bit-identical to the host's
    report("device, worst |error| / bound (must stay below %g), scene %s" % (B.TOL, name), rep)


def test_one_instance_edited_identity_mirror_rank2_and_back(device):
    """identity -> mirror in x -> rank 2 -> identity on one instance of each mesh by update_instances: every step answers what a fresh upload of that step answers,
    and the last step what the first did, bit for bit"""
    ms = B.meshes()
    steps = [np.eye(3), np.diag([-1.0, 1.0, 1.0]), np.diag([1.0, 1.0, 0.0]), np.eye(3)]
    layout = lambda a: B.build_group([("step", a, (0.0, 0.0, 0.0), 1.0)], ms)["instances"]
    g = B.build_group([("step", steps[0], (0.0, 0.0, 0.0), 1.0)], ms)                 # the first step's rays and elements serve every step: only agreement is asked
    nt = g["tris"]["P"].shape[0]
    q = {"prim": np.repeat(np.arange(nt, dtype=np.uint32), 16), "bary": np.tile(B.BARY, (nt, 1)), "d": g["d"]}
    s, sg, idx = upload(device, "host", layout(steps[0]), ms)
    seen = []
    for a in steps:
        for i, inst in zip(idx, layout(a)):
            s.set_instance_transform(i, inst[1])
        sg.update_instances(s)
        got = probes(sg, g, q)
        _, fresh, _ = upload(device, "host", layout(a), ms)
        want = probes(fresh, g, q)
        fresh.close()
        assert got[0].tobytes() == want[0].tobytes() and got[1][0].tobytes() == want[1][0].tobytes() and got[1][1].tobytes() == want[1][1].tobytes()
        assert np.all(np.isfinite(got[1][0])) and np.all(np.isfinite(np.stack([got[0]["t"], got[0]["u"], got[0]["v"]])))
        seen.append((got[0].tobytes(), got[1][0].tobytes(), got[1][1].tobytes()))
    sg.close()
    assert seen[-1] == seen[0] and seen[1] != seen[0] and seen[2] != seen[1]


def test_outside_the_domain_probes_stay_finite_and_paths_agree(device):
    """uniform scales 2^-60 and 2^60: no bound is claimed; every probe output is finite and the four paths agree"""
    ms = B.meshes()
    for a in B.OUTSIDE.values():
        g = B.build_group([("outside", a, (0.0, 0.0, 0.0), float(a[0, 0]))])
        nt = g["tris"]["P"].shape[0]
        q = {"prim": np.repeat(np.arange(nt, dtype=np.uint32), 16), "bary": np.tile(B.BARY, (nt, 1)), "d": g["d"]}
        first = None
        for path in PATHS:
            _, sg, _ = upload(device, path, g["instances"], ms)
            hits, (ns, mapped) = probes(sg, g, q)
            sg.close()
            assert np.all(np.isfinite(ns)) and np.all(np.isfinite(np.stack([hits["t"], hits["u"], hits["v"]])))
            got = (hits.tobytes(), ns.tobytes(), mapped.tobytes())
            first = first or got
            assert got == first, path


# ------------------------------------------------------------------ the mirrored-instance rule (SPEC §2.5) pinned on the device
def mirror_pair(names=("rotation", "rotation-scale")):
    """(meshes, the original meshes under M, the mirror-image meshes under M·diag(−1, 1, 1)): the same objects in the world (tests/test_bake_reference.py)"""
    ms = B.meshes()
    both = dict(ms)
    both.update({"mirror-" + n: B.mirror_mesh(m) for n, m in ms.items()})
    cases = [c for c in B.groups()["main"] if c[0] in names]
    plain = [(mn, B.matrix(a, (t[0], t[1] + (B.ASIDE if mn == "octahedron" else 0.0), t[2])), 0) for _, a, t, _ in cases for mn in ms]
    return both, plain, [("mirror-" + mn, B.mirror_matrix(m), 0) for mn, m, _ in plain]


@pytest.mark.parametrize("path", PATHS)
def test_mirror_image_mesh_under_a_mirrored_node_probes_the_same(device, path):
    """both probes answer the same bytes for the two scenes, through every build path, and the hits name the prims of the reference of the original"""
    g, tr, nm = B.reference("main")
    sel_r = np.isin(g["ray_case"], (1, 2))
    sel_n = np.isin(g["tri_case"][nm["prim"]], (1, 2))
    first_tri = int(np.nonzero(g["tri_case"] == 1)[0][0])
    both, plain, mirrored = mirror_pair()
    got = []
    for inst in (plain, mirrored):
        _, sg, _ = upload(device, path, inst, both)
        hits = sg.trace_closest(g["o"][sel_r], g["d"][sel_r])
        ns, mapped = sg.shading_normal(nm["prim"][sel_n] - first_tri, nm["bary"][sel_n], nm["d"][sel_n])
        sg.close()
        got.append((hits.tobytes(), ns.tobytes(), mapped.tobytes()))
        c = tr["compared"][sel_r]
        assert np.array_equal(hits["prim"][c] + first_tri, tr["prim"][sel_r][c])
        assert np.any(mapped)
    assert got[0] == got[1]


def _render(device, sg):
    """64x48, 4 bounces, 2 frames, a fixed seed"""
    pr = lp.ProbeGPU(device, T.CORNELL_PROBE, 1, 1)
    r = lp.Renderer(device, (64, 48))
    r.downsample_factor = 1.0
    r.resize(device, sg, pr, (64, 48))
    r.set_max_bounces(4)
    r.set_vfov(0.6)
    r.set_seed(7)
    r.reset_accumulation()
    r.accumulate = True
    r.reset_ray_counts()
    view = T.look((0.3, 0.4, 4.0), (0.0, 0.0, -1.0))
    for _ in range(2):
        r.raytrace(view)
    img, c = r.read_radiance(), r.ray_counts()
    r.close(); pr.close()
    return img, (c.closest, c.shadow, c.shaded)


def _render_scene(device, mirrored):
    """the glass octahedron beside the normal-mapped patch under a general rotation, lit by a rectangle above; or their mirror-image meshes under the mirrored nodes"""
    ms = B.meshes()
    rot = [c for c in B.groups()["main"] if c[0] == "rotation"][0][1]
    s = lp.Scene()
    light = np.zeros(1, lp._abi.LIGHT_DT)
    light["normal"], light["tangent"], light["bitangent"], light["origin"] = (0, -1, 0, 0), (1, 0, 0, 1.0), (0, 0, 1, 1.0), (0.0, 2.5, 0.0, 12.0)
    s.set_light(0, light)
    img = s.add_image(B.normal_image())
    mapped = s.add_material((0.8, 0.7, 0.6, 1.0), 0.5, 0.0)
    s.set_material_normal_map(mapped, img, 2.0)
    glass = s.add_material((0.9, 0.95, 1.0, 1.0), 0.2, 0.0)
    s.set_material_transmission(glass, 1.0, 1.5, False)
    for mn, mat, t, scale in (("patch-mapped", mapped, (-0.3, 0.2, 0.0), 2.0), ("patch-plain", mapped, (-0.3, 0.2, 0.0), 2.0), ("octahedron", glass, (0.9, 0.5, 0.6), 1.0)):
        mesh, m = ms[mn], B.matrix(rot * scale, t)
        if mirrored:
            mesh, m = B.mirror_mesh(mesh), B.mirror_matrix(m)
        s.add_instance(s.add_mesh(mesh["pos"], mesh["nrm"], mesh["uv"], mesh["idx"]), m, mat)
    return s


@pytest.mark.usefixtures("pipeline")
def test_mirror_image_scene_renders_the_same_frame(device):
    """the glass octahedron and the normal-mapped patch: the frame of the mirror-image meshes under mirrored nodes is the frame of the originals, bit for bit and with
    equal ray counts — solid glass refracts on the way in (§21) and a bump stays a bump (§24) under a negative determinant"""
    frames = []
    for mirrored in (False, True):
        sg = lp.SceneGPU.new_from_scene(_render_scene(device, mirrored), device)
        frames.append(_render(device, sg))
        sg.close()
    (a, ca), (b, cb) = frames
    print("\nray counts (closest, shadow, shaded): original %s, mirror image under mirrored nodes %s; pixels that differ: %d of %d" % (ca, cb, int(np.any(a != b, -1).sum()), a.shape[0] * a.shape[1]))
    assert np.all(np.isfinite(a)) and a[..., :3].max() > 0
    assert a.tobytes() == b.tobytes() and ca == cb
