"""CPU: normal maps (SPEC.md §24) on the host — the scene API's side table, what the glTF loader reads (normalTexture and its scale; SPEC §14(10)), the launch plan's
`nmap` fact through tests/tools/plan_fact_check.cpp, the bindings' agreement on the new entry points, tests/normal_ref.py against closed forms and against its own
binary32 restatement, and the cap on the decisions that the GPU test's committed inputs leave to rounding."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import _abi as A

import normal_ref as N
from test_gpu_normal_map import IMAGE1, N_HOOK, hook_cases, hook_reference, hook_shapes, image4, normal_glb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NONE = (None, 1.0)


def _load(glb, into=None):
    s = lp.Scene() if into is None else into
    lp.loaders.load_gltf(glb, s)
    return s


def _snapshot(s):
    c = s.counts()
    return (tuple(getattr(c, f) for f, _ in c._fields_), s.materials.tobytes(), s.instances.tobytes(), s.vertices.tobytes(), s.indices.tobytes(), s.punctual_lights.tobytes(),
            tuple(s.material_alpha(m) for m in range(c.materials)), tuple(s.material_transmission(m) for m in range(c.materials)),
            tuple(tuple(s.material_emission(m)[0].tolist()) + (s.material_emission(m)[1],) for m in range(c.materials)), tuple(s.material_normal_map(m) for m in range(c.materials)))


# ---------------------------------------------------------------- scene API
def test_set_get_round_trip_and_none_removes_the_map():
    s = lp.Scene()
    m = s.add_material((1, 1, 1, 1), 0.5, 0.0)
    img = s.add_image(image4())
    assert s.material_normal_map(0) == NONE and s.material_normal_map(m) == NONE
    before = s.materials.tobytes()
    s.set_material_normal_map(m, img, 2.5)
    assert s.material_normal_map(m) == (img, 2.5) and s.get_material_normal_map(m) == (img, 2.5) and s.material_normal_map(0) == NONE
    s.set_material_normal_map(m, img)                               # scale defaults to 1
    assert s.material_normal_map(m) == (img, 1.0)
    for scale in (0.0, -1.0, float(F(1e30)), float(F(0.1))):                  # any finite float
        s.set_material_normal_map(m, img, scale)
        assert s.material_normal_map(m) == (img, scale)
    m2 = s.add_material((1, 1, 1, 1), 1.0, 0.0)                     # a material added after the table was first written
    assert s.material_normal_map(m2) == NONE
    s.set_material_normal_map(m, None, 7.0)                         # removed: the scale goes with it
    assert s.material_normal_map(m) == NONE
    s.set_material_normal_map(m2, None)                             # removing what is not there is fine
    assert s.materials[:2].tobytes() == before and A.MATERIAL_DT.itemsize == 32


@pytest.mark.parametrize("args", [(9, 0, 1.0), (1, 1, 1.0), (1, 12345, 1.0), (1, 0, float("nan")), (1, 0, float("inf")), (1, 0, float("-inf")), (1, None, float("nan"))])
def test_invalid_arguments_leave_the_scene_untouched(args):
    s = lp.Scene()
    m = s.add_material((1, 1, 1, 1), 1.0, 0.0)
    img = s.add_image(image4())
    assert (m, img) == (1, 0)
    s.set_material_normal_map(m, img, 2.0)
    with pytest.raises(lp.Error) as e:
        s.set_material_normal_map(*args)
    assert e.value.kind == "InvalidArg" and "lpt_scene_set_material_normal_map" in str(e.value)
    assert s.material_normal_map(m) == (img, 2.0)
    with pytest.raises(lp.Error) as e:
        s.material_normal_map(2)
    assert e.value.kind == "InvalidArg"


def test_bindings_agree_on_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "lpt.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "loupiote_hip", "src", "ffi.rs")).read()
    safe = open(os.path.join(ROOT, "bindings", "rust", "loupiote_hip", "src", "lib.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "loupiote.hpp")).read()
    for n in ("lpt_scene_set_material_normal_map", "lpt_scene_get_material_normal_map", "lpt_scene_gpu_shading_normal"):
        m = re.search(r"\bint %s\(([^;]*)\);" % n, header)
        assert m, n
        n_args = len(m.group(1).split(","))
        assert n in A.SIGNATURES and len(A.SIGNATURES[n][1]) == n_args, n
        m = re.search(r"pub fn %s\(([^;]*)\) -> c_int;" % n, ffi)
        assert m and len(m.group(1).split(",")) == n_args, n
        assert "%s(" % n in hpp, n
        assert hasattr(A.lib(), n)
    assert "ffi::lpt_scene_set_material_normal_map(" in safe and "ffi::lpt_scene_get_material_normal_map(" in safe
    assert A.lib().lpt_abi_version() == 6      # new entry points only: no layout changed
    assert "SPEC.md §24" in header and "lpt_scene_set_material_normal_map" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


# ---------------------------------------------------------------- loader (SPEC §14(10))
def test_the_fixture_values_arrive():
    s = _load(normal_glb())
    assert s.counts().materials == 2 and s.counts().images == 1
    assert s.material_normal_map(0) == NONE and s.material_normal_map(1) == (0, 2.0)      # the dummy; the image through textures[].source, the scale
    _load(normal_glb(), s)                                          # appended to a scene that already has an image and materials: the offsets apply
    assert s.counts().materials == 3 and s.material_normal_map(2) == (1, 2.0) and s.material_normal_map(1) == (0, 2.0)


def test_defaults_and_the_ignored_texcoord():
    assert _load(normal_glb(normal={"index": 0})).material_normal_map(1) == (0, 1.0)                       # scale defaults to 1
    assert _load(normal_glb(normal={"index": 0, "scale": -0.5, "texCoord": 3})).material_normal_map(1) == (0, -0.5)      # texCoord is not read
    assert _load(normal_glb(normal={"index": 0, "scale": 0})).material_normal_map(1) == (0, 0.0)
    assert _load(normal_glb(normal={"index": 0, "scale": 0.1})).material_normal_map(1) == (0, float(F(0.1)))


@pytest.mark.parametrize("normal", [{"index": 1}, {"index": -1}, {"index": 7, "scale": 1.0}, {"scale": 2.0}, {"index": 0, "scale": 1e999}, {"index": 0, "scale": -1e999},
                                    {"index": 0, "scale": 1e39}, {"index": 0, "scale": "2"}, {"index": 0, "scale": [1.0]}])
def test_rejected_input_leaves_the_scene_untouched(normal):
    s = _load(normal_glb())
    before = _snapshot(s)
    with pytest.raises(lp.Error) as e:
        _load(normal_glb(normal=normal), s)
    assert e.value.kind == "FileNotFound"
    assert _snapshot(s) == before


def test_a_file_without_the_key_loads_as_before(cornell_glb):
    s = _load(cornell_glb)
    assert all(s.material_normal_map(m) == NONE for m in range(s.counts().materials))
    from oracle import gltf_oracle as G
    o = G.Scene()
    G.load_gltf(cornell_glb, o)
    for name in ("materials", "instances", "vertices", "indices", "entries"):
        assert getattr(s, name).tobytes() == np.ascontiguousarray(getattr(o, name)).tobytes(), name
    # the same file with and without the key: everything but the side table is the same bytes
    a, b = _snapshot(_load(normal_glb())), _snapshot(_load(normal_glb(normal=None)))
    assert a[:-1] == b[:-1] and a[-1] != b[-1] and all(t == NONE for t in b[-1])


def test_the_committed_fixture_is_the_writers_output():
    with open(os.path.join(ROOT, "tests", "golden", "normal-map.glb"), "rb") as f:
        data = f.read()
    assert data == normal_glb() and len(data) < 8192


# ---------------------------------------------------------------- launch plan
def test_nmap_keeps_a_wavefront_off_the_path_kernel_and_changes_nothing_else(tmp_path):
    exe = str(tmp_path / "plan_fact_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "tools", "plan_fact_check.cpp")], check=True)
    p = subprocess.run([exe, "nmap"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = json.loads(p.stdout)
    assert out["cases"] == 9 * 256 * 3 * 2 and 0 < out["with_path"] < out["cases"]      # the grid does reach plans that would have taken the path kernel


# ---------------------------------------------------------------- the reference's self-checks
def _one(pos, nrm, uv, bary, d, image, scale, **kw):
    g = lambda a, sh: np.broadcast_to(np.asarray(a, F), (len(bary),) + sh)
    return N.shading_normal(g(pos, (3, 3)), g(nrm, (3, 3)), g(uv, (3, 2)), np.asarray(bary, F), g(d, (3,)), image, scale, **kw)


FLAT = dict(pos=[[0, 0, 0], [1, 0, 0], [0, 0, -1]], nrm=[[0, 1, 0]] * 3, uv=[[0, 0], [1, 0], [0, -1]])      # normal +y, uv = (x, z)
DOWN = [0.0, -1.0, 0.0]
BARY = np.random.default_rng(7).dirichlet((1, 1, 1), 64)[:, :2].astype(F)


def test_reference_frame_is_orthonormal():
    sh = hook_shapes()[6]                                           # the tilted normals: the frame is re-orthogonalised against the interpolated normal
    t, b, d = hook_cases(6, sh)
    r = hook_reference(sh, t, b, d)
    Tp, Bp, Nv = r["Tp"], r["Bp"], r["Nv"]
    for x, y in ((Tp, Bp), (Tp, Nv), (Bp, Nv)):
        assert np.abs(np.sum(x * y, 1)).max() < 1e-14
    for x in (Tp, Bp, Nv, r["Ns"]):
        assert np.abs(np.linalg.norm(x, axis=1) - 1).max() < 1e-14
    assert np.abs(np.sum(Nv * r["Ngf"], 1)).min() > 0.7 and r["mapped"].any() and not r["mapped"].all()


def test_reference_a_uniform_texel_on_an_axis_aligned_quad_is_the_closed_form():
    for rgb, scale in (((200, 90, 230), 1.0), ((10, 250, 140), 2.5), ((128, 128, 255), 1.0), ((77, 201, 160), -1.0)):
        img = np.array([[rgb + (255,)]], np.uint8)
        r = _one(image=img, scale=scale, bary=BARY, d=DOWN, **FLAT)
        n = np.array(rgb) / 255.0 * 2 - 1
        want = np.array([n[0] * scale, n[2], n[1] * scale])         # T = +x, B = +z (v grows with z), N = +y
        want /= np.linalg.norm(want)
        assert r["mapped"].all() and np.abs(r["Ns"] - want[None]).max() < 1e-15, (rgb, scale)
        # seen from below, the reversed normal (glTF's rule for double-sided materials)
        r = _one(image=img, scale=scale, bary=BARY, d=[0.0, 1.0, 0.0], **FLAT)
        assert r["mapped"].all() and r["flip"].all() and np.abs(r["Ns"] + want[None]).max() < 1e-15


def test_reference_mirrored_u_mirrors_nx_and_leaves_ny():
    img = image4()
    uv = np.asarray(FLAT["uv"], F)
    mir = uv * F([-1, 1])                                            # u -> -u: det changes sign
    a = _one(FLAT["pos"], FLAT["nrm"], uv, BARY, DOWN, img, 1.0)
    b = _one(FLAT["pos"], FLAT["nrm"], mir, BARY, DOWN, img, 1.0)
    assert (a["q"]["det"][0] * b["q"]["det"][0] < 0).all()                  # one of the two is the mirrored parametrisation (det < 0)
    assert np.allclose(a["Tp"], -b["Tp"], atol=1e-15) and np.allclose(a["Bp"], b["Bp"], atol=1e-15)
    # the same texel seen through both: a 1x1 image removes the lookup position from the comparison
    a = _one(FLAT["pos"], FLAT["nrm"], uv, BARY, DOWN, IMAGE1, 1.0)
    b = _one(FLAT["pos"], FLAT["nrm"], mir, BARY, DOWN, IMAGE1, 1.0)
    assert np.allclose(a["Ns"] * [-1, 1, 1], b["Ns"], atol=1e-15) and np.abs(a["Ns"][:, 0]).min() > 0.1 and np.abs(a["Ns"][:, 2]).min() > 0.1


def test_reference_fallbacks():
    img = image4()
    plain = _one(image=None, scale=1.0, bary=BARY, d=DOWN, **FLAT)["Ns"]
    assert np.array_equal(plain, np.tile([0.0, 1.0, 0.0], (len(BARY), 1)))
    for dtype in (np.float64, np.float32):
        # det = 0: all uv equal
        r = _one(FLAT["pos"], FLAT["nrm"], [[0.3, 0.6]] * 3, BARY, DOWN, img, 1.0, dtype=dtype)
        assert not r["mapped"].any() and np.array_equal(r["Ns"], plain) and (r["q"]["det"][0] == 0).all() and (r["q"]["det"][1] == 0).all()
        # a zero Tp: the vertex normals lie along the tangent (uv = (x, y) on a triangle in the xy plane, normals +x)
        r = _one([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[1, 0, 0]] * 3, [[0, 0], [1, 0], [0, 1]], BARY, [0, 0, -1.0], img, 1.0, dtype=dtype)
        assert not r["mapped"].any() and (r["q"]["tl2"][0] == 0).all() and np.array_equal(r["Ns"], np.tile([1.0, 0.0, 0.0], (len(BARY), 1)))
        # nz = -1 with scale 0: Nm = -Nv, under the surface
        r = _one(image=np.array([[[37, 99, 0, 255]]], np.uint8), scale=0.0, bary=BARY, d=DOWN, dtype=dtype, **FLAT)
        assert not r["mapped"].any() and np.array_equal(r["Ns"], plain) and (r["q"]["under"][0] < -0.99).all() and (r["q"]["m2"][0] > 0.99).all()
        # ... and nz = 0 with scale 0: m2 = 0 needs tex.b = 1/2 exactly, which no byte gives; a scale of 0 with nz > 0 is the interpolated normal itself
        r = _one(image=np.array([[[37, 99, 200, 255]]], np.uint8), scale=0.0, bary=BARY, d=DOWN, dtype=dtype, **FLAT)
        assert r["mapped"].all() and np.abs(r["Ns"] - plain).max() < 1e-6


def test_reference_binary32_restatement_lies_within_the_running_bound():
    """the bound is checked against the one binary32 evaluation that needs no GPU: numpy's, operation by operation in the SPEC's order"""
    worst = 0.0
    for k, sh in enumerate(hook_shapes()):
        t, b, d = hook_cases(k, sh)
        r64, r32 = hook_reference(sh, t, b, d), hook_reference(sh, t, b, d, dtype=np.float32)
        c = ~N.undecided(r64)
        assert np.array_equal(r64["mapped"][c], r32["mapped"][c]) and np.array_equal(r64["flip"][c], r32["flip"][c]), sh["name"]
        err, bound = np.abs(r32["Ns"].astype(np.float64) - r64["Ns"])[c], r64["Ns_err"][c]
        assert np.all(err <= bound), (sh["name"], float((err - bound).max()))
        for name, (v, e) in r64["q"].items():
            m = c & r64.get("reached", {name: c})[name]
            assert np.all(np.abs(r32["q"][name][0].astype(np.float64) - v)[m] <= e[m]), (sh["name"], name)
        worst = max(worst, float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0))))
    print("binary32 restatement: largest error / bound %.3g" % worst)
    assert worst > 0.01      # the bound is not vacuous either


def test_decisions_left_to_rounding_stay_under_the_cap():
    """for the committed inputs of the GPU hook test: the elements one of whose deciding quantities (det, tl2, m2, dot(Bp, B), dot(Nv, Ngf), dot(Ns, Ngf), and §12's
    dot(Ng, d)) lies within its derived bound of its threshold are at most 2 % per shape — counted from the binary64 reference alone"""
    total = 0
    for k, sh in enumerate(hook_shapes()):
        t, b, d = hook_cases(k, sh)
        assert len(t) == N_HOOK == 64 * 64 + 4
        r = hook_reference(sh, t, b, d)
        u = N.undecided(r)
        print("%-26s undecided %d of %d; mapped %d; flipped %d" % (sh["name"], u.sum(), N_HOOK, r["mapped"].sum(), r["flip"].sum()))
        assert u.sum() <= 0.02 * N_HOOK, (sh["name"], int(u.sum()))
        assert 0.3 < (r["q"]["geo"][0] > 0).mean() < 0.7             # directions on both sides
        assert (np.abs(r["q"]["geo"][0]) < 0.01).mean() > 0.15       # some grazing
        total += int(u.sum())
    assert total <= 0.02 * N_HOOK * 8
