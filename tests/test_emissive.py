"""CPU: emissive materials (SPEC.md §22) on the host — the scene API's side table, what the glTF loader reads (emissiveFactor, emissiveTexture,
KHR_materials_emissive_strength; SPEC §14(9)), the launch plan's `emis` fact through tests/tools/plan_fact_check.cpp, the bindings' agreement on the new entry points,
and tests/emissive_ref.py against what it restates."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import _abi as A

import emissive_ref as E
from test_gpu_emissive import emissive_glb, texture4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _load(glb, into=None):
    s = lp.Scene() if into is None else into
    lp.loaders.load_gltf(glb, s)
    return s


def _emission(s, m):
    le, image = s.material_emission(m)
    return tuple(float(x) for x in le), image


def _snapshot(s):
    c = s.counts()
    return (tuple(getattr(c, f) for f, _ in c._fields_), s.materials.tobytes(), s.instances.tobytes(), s.vertices.tobytes(), s.indices.tobytes(), s.punctual_lights.tobytes(),
            tuple(s.material_alpha(m) for m in range(c.materials)), tuple(s.material_transmission(m) for m in range(c.materials)), tuple(_emission(s, m) for m in range(c.materials)))


NONE = ((0.0, 0.0, 0.0), None)


# ---------------------------------------------------------------- scene API
def test_set_get_round_trip_and_zero_drops_the_record():
    s = lp.Scene()
    m = s.add_material((1, 1, 1, 1), 0.5, 0.0)
    img = s.add_image(texture4())
    assert _emission(s, 0) == NONE and _emission(s, m) == NONE
    before = s.materials.tobytes()
    s.set_material_emission(m, (0.9, 0.5, 0.1), 3.0, img)
    le, image = s.material_emission(m)
    assert np.array_equal(le, F((0.9, 0.5, 0.1)) * F(3.0)) and le.dtype == np.float32 and image == img      # one binary32 product per channel
    s.set_material_emission(m, (0.0, 2.5, 0.0))                     # strength 1, no image; a factor above 1 is the caller's business
    assert _emission(s, m) == ((0.0, 2.5, 0.0), None) and _emission(s, 0) == NONE
    m2 = s.add_material((1, 1, 1, 1), 1.0, 0.0)                     # a material added after the table was first written
    assert _emission(s, m2) == NONE
    s.set_material_emission(m, (0.9, 0.5, 0.1), 0.0, img)           # a product of 0: the record is dropped, the image with it
    assert _emission(s, m) == NONE
    s.set_material_emission(m, (0.0, 0.0, 0.0), 7.0, img)
    assert _emission(s, m) == NONE
    assert s.materials[:2].tobytes() == before and A.MATERIAL_DT.itemsize == 32


@pytest.mark.parametrize("args", [(9, (1, 1, 1), 1.0, None), (1, (-0.1, 1, 1), 1.0, None), (1, (1, float("nan"), 1), 1.0, None), (1, (1, 1, float("inf")), 1.0, None),
                                  (1, (1, 1, 1), -1.0, None), (1, (1, 1, 1), float("nan"), None), (1, (1, 1, 1), float("inf"), None), (1, (1, 1, 1), 1.0, 1),
                                  (1, (1, 1, 1), 1.0, 12345), (1, (3e38, 1, 1), 3e38, None)])
def test_invalid_arguments_leave_the_scene_untouched(args):
    s = lp.Scene()
    m = s.add_material((1, 1, 1, 1), 1.0, 0.0)
    img = s.add_image(texture4())
    assert (m, img) == (1, 0)
    s.set_material_emission(m, (0.25, 0.5, 1.0), 2.0, img)
    with pytest.raises(lp.Error) as e:
        s.set_material_emission(*args)
    assert e.value.kind == "InvalidArg" and "lpt_scene_set_material_emission" in str(e.value)
    assert _emission(s, m) == ((0.5, 1.0, 2.0), img)
    with pytest.raises(lp.Error) as e:
        s.material_emission(2)
    assert e.value.kind == "InvalidArg"


def test_bindings_agree_on_the_new_entry_points():
    names = ("lpt_scene_set_material_emission", "lpt_scene_get_material_emission")
    header = open(os.path.join(ROOT, "include", "lpt.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "loupiote_hip", "src", "ffi.rs")).read()
    safe = open(os.path.join(ROOT, "bindings", "rust", "loupiote_hip", "src", "lib.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "loupiote.hpp")).read()
    for n in names:
        m = re.search(r"\bint %s\(([^;]*)\);" % n, header)
        assert m, n
        n_args = len(m.group(1).split(","))
        assert n in A.SIGNATURES and len(A.SIGNATURES[n][1]) == n_args, n
        m = re.search(r"pub fn %s\(([^;]*)\) -> c_int;" % n, ffi)
        assert m and len(m.group(1).split(",")) == n_args, n
        assert "ffi::%s(" % n in safe and "%s(" % n in hpp, n
        assert hasattr(A.lib(), n)
    assert A.lib().lpt_abi_version() == 6      # new entry points only: no layout changed
    assert "SPEC.md §22" in header and "lpt_scene_set_material_emission" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


# ---------------------------------------------------------------- loader (SPEC §14(9))
def test_the_fixture_values_arrive():
    s = _load(emissive_glb())
    assert s.counts().materials == 3 and s.counts().images == 1
    assert _emission(s, 0) == NONE and _emission(s, 1) == NONE                                   # the dummy, the floor
    le, image = s.material_emission(2)
    assert np.array_equal(le, F((1.0, 0.8, 0.6)) * F(5.0)) and image == 0                          # factor x strength, the image through textures[].source
    # appended to a scene that already has an image and materials: the offsets apply
    _load(emissive_glb(), s)
    assert s.counts().materials == 5 and s.material_emission(4)[1] == 1 and _emission(s, 3) == NONE


def test_defaults():
    assert _emission(_load(emissive_glb(panel={"emissiveFactor": [0.5, 0.25, 1.0]})), 2) == ((0.5, 0.25, 1.0), None)          # strength 1, no image
    assert _emission(_load(emissive_glb(panel={"emissiveTexture": {"index": 0}})), 2) == NONE                                  # no factor: (0, 0, 0), non-emissive
    assert _emission(_load(emissive_glb(panel={"extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": 9.0}}})), 2) == NONE
    assert _emission(_load(emissive_glb(panel={"emissiveFactor": [1, 1, 1], "extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": 0}}, "emissiveTexture": {"index": 0}})), 2) == NONE
    assert _emission(_load(emissive_glb(panel={"emissiveFactor": [0, 0, 0], "emissiveTexture": {"index": 0}})), 2) == NONE
    s = _load(emissive_glb(panel={"emissiveFactor": [0.0, 1.0, 0.0], "emissiveTexture": {"index": 0, "texCoord": 0}, "extensions": {"KHR_materials_emissive_strength": {}}}))
    assert _emission(s, 2) == ((0.0, 1.0, 0.0), 0)


@pytest.mark.parametrize("panel", [{"emissiveFactor": [1.0, 1.0]}, {"emissiveFactor": [1, 1, 1, 1]}, {"emissiveFactor": 1.0}, {"emissiveFactor": "white"},
                                   {"emissiveFactor": [1, "1", 1]}, {"emissiveFactor": [-0.1, 0, 0]}, {"emissiveFactor": [0, 1.5, 0]}, {"emissiveFactor": [0, 0, 1e999]},
                                   {"emissiveFactor": [1, 1, 1], "emissiveTexture": {"index": 1}}, {"emissiveFactor": [1, 1, 1], "emissiveTexture": {"index": -1}},
                                   {"emissiveFactor": [0, 0, 0], "emissiveTexture": {"index": 7}},
                                   {"emissiveFactor": [1, 1, 1], "extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": -1}}},
                                   {"extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": 1e999}}},
                                   {"extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": 1e39}}},
                                   {"extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": "5"}}}])
def test_rejected_input_leaves_the_scene_untouched(panel):
    s = _load(emissive_glb())
    before = _snapshot(s)
    with pytest.raises(lp.Error) as e:
        _load(emissive_glb(panel=panel), s)
    assert e.value.kind == "FileNotFound"
    assert _snapshot(s) == before


def test_a_file_without_the_three_members_loads_as_before(cornell_glb):
    s = _load(cornell_glb)
    c = s.counts()
    assert all(_emission(s, m) == NONE for m in range(c.materials))
    from oracle import gltf_oracle as G
    o = G.Scene()
    G.load_gltf(cornell_glb, o)
    for name in ("materials", "instances", "vertices", "indices", "entries"):
        assert getattr(s, name).tobytes() == np.ascontiguousarray(getattr(o, name)).tobytes(), name
    # the same file with and without the members: everything but the side table is the same bytes
    a, b = _snapshot(_load(emissive_glb())), _snapshot(_load(emissive_glb(panel=None)))
    assert a[:-1] == b[:-1] and a[-1] != b[-1] and all(t == NONE for t in b[-1])


def test_the_committed_fixture_is_the_writers_output():
    with open(os.path.join(ROOT, "tests", "golden", "emissive-panel.glb"), "rb") as f:
        data = f.read()
    assert data == emissive_glb() and len(data) < 8192


# ---------------------------------------------------------------- launch plan
def test_emis_keeps_a_wavefront_off_the_path_kernel_and_changes_nothing_else(tmp_path):
    exe = str(tmp_path / "plan_fact_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "tools", "plan_fact_check.cpp")], check=True)
    p = subprocess.run([exe, "emis"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = json.loads(p.stdout)
    assert out["cases"] == 9 * 128 * 3 * 2 and 0 < out["with_path"] < out["cases"]      # the grid does reach plans that would have taken the path kernel


# ---------------------------------------------------------------- the reference's self-checks
def test_reference_a_1x1_image_is_a_constant():
    img = np.array([[[200, 90, 30, 255]]], np.uint8)
    rng = np.random.default_rng(3)
    tu, tv = rng.uniform(-3, 3, 200), rng.uniform(-3, 3, 200)
    got = E.lookup(img, tu, tv)
    assert np.allclose(got, E.srgb_table()[img[0, 0, :3]][None], rtol=1e-15, atol=0)
    rec = E.record((0.5, 0.5, 0.5), 2.0, 0)
    assert np.allclose(E.emitted(rec, [img], tu, tv), E.srgb_table()[img[0, 0, :3]][None], rtol=1e-15)


def test_reference_uv_outside_the_unit_square_wraps():
    img = texture4()
    rng = np.random.default_rng(4)
    tu, tv = rng.uniform(0, 1, 300), rng.uniform(0, 1, 300)
    base = E.lookup(img, tu, tv)
    for du, dv in ((1, 0), (0, 1), (-2, 3), (5, -4)):
        assert np.allclose(E.lookup(img, tu + du, tv + dv), base, rtol=0, atol=1e-12)
    # texel centres return the texel, and the lookup across the border blends the last texel with the first
    lin = E.srgb_table()[img[..., :3]]
    assert np.allclose(E.lookup(img, np.array([0.125 + 0.25 * 2]), np.array([0.125 + 0.25 * 1])), lin[1, 2][None], atol=1e-15)
    assert np.allclose(E.lookup(img, np.array([0.0]), np.array([0.125])), 0.5 * (lin[0, 3] + lin[0, 0])[None], atol=1e-15)
    t = E.srgb_table()
    assert t[0] == 0.0 and t[255] == 1.0 and np.all(np.diff(t) > 0) and abs(t[10] - 10 / 255 / 12.92) < 1e-9 and abs(t[128] - ((128 / 255 + 0.055) / 1.055) ** 2.4) < 1e-7


def test_reference_strength_scales_linearly_and_zero_is_no_record():
    img = texture4()
    tu, tv = np.linspace(0, 2.5, 50), np.linspace(2.5, 0, 50)
    one = E.emitted(E.record((0.5, 0.25, 1.0), 1.0, 0), [img], tu, tv)
    four = E.emitted(E.record((0.5, 0.25, 1.0), 4.0, 0), [img], tu, tv)
    assert np.array_equal(four, 4.0 * one) and one.max() > 0.1
    assert E.record((0.5, 0.25, 1.0), 0.0, 0) is None and E.record((0, 0, 0), 3.0) is None
    assert E.record((0.9, 0.5, 0.1), 3.0)[0].dtype == np.float32 and np.array_equal(E.record((0.9, 0.5, 0.1), 3.0)[0], F((0.9, 0.5, 0.1)) * F(3.0))
    # a depth-1 frame: a miss is 0, a hit is E at the interpolated uv
    tri_uv = np.array([[(0, 0), (2.5, 0), (2.5, 2.5)], [(0, 0), (2.5, 2.5), (0, 2.5)]])
    rec = E.record((1, 1, 1), 2.0, 0)
    f = E.depth1_frame([-1, 0, 1], [0.0, 0.25, 0.5], [0.0, 0.5, 0.25], tri_uv, [rec, rec], [img])
    assert not f[0].any() and np.allclose(f[1], 2.0 * E.lookup(img, np.array([2.5 * 0.75]), np.array([2.5 * 0.5]))[0]) and np.allclose(f[2], 2.0 * E.lookup(img, np.array([2.5 * 0.5]), np.array([2.5 * 0.75]))[0])
