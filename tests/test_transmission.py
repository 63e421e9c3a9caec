"""CPU: transmissive materials (SPEC.md §21) on the host — what the glTF loader reads (KHR_materials_transmission, _ior, _volume), the scene API's
side table, the bindings' agreement on the new entry points, and tests/transmission_ref.py against the physics it restates."""
import os
import re

import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import _abi as A

import transmission_ref as R
from test_gpu_transmission import glass_glb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPAQUE = (0.0, 1.5, True)


def _load(glb, into=None):
    s = lp.Scene() if into is None else into
    lp.loaders.load_gltf(glb, s)
    return s


def _snapshot(s):
    c = s.counts()
    return (tuple(getattr(c, f) for f, _ in c._fields_), s.materials.tobytes(), s.instances.tobytes(), s.vertices.tobytes(), s.indices.tobytes(), s.punctual_lights.tobytes(),
            tuple(s.material_alpha(m) for m in range(c.materials)), tuple(s.material_transmission(m) for m in range(c.materials)))


# ---------------------------------------------------------------- loader
def test_the_three_extensions_and_their_defaults():
    s = _load(glass_glb())
    assert s.counts().materials == 4
    assert s.material_transmission(0) == OPAQUE and s.material_transmission(1) == OPAQUE      # the dummy, the floor
    assert s.material_transmission(2) == (1.0, 1.5, True)                                      # the pane: no ior, no volume -> 1.5, thin-walled
    f, ior, thin = s.material_transmission(3)                                                  # the cube: ior 1.33, thicknessFactor 0.5 -> solid
    assert (f, ior, thin) == (float(np.float32(0.9)), float(np.float32(1.33)), False)
    # thin versus solid is glTF's own rule: thicknessFactor > 0
    assert _load(glass_glb(cube_thickness=0.0)).material_transmission(3)[2] is True
    assert _load(glass_glb(cube_thickness=None)).material_transmission(3)[2] is True
    assert _load(glass_glb(pane={"KHR_materials_transmission": {"transmissionFactor": 0.25}, "KHR_materials_volume": {"thicknessFactor": 2}})).material_transmission(2) == (0.25, 1.5, False)
    # a factor of 0 (stated or by default) is opaque, whatever else the material states
    assert _load(glass_glb(pane={"KHR_materials_transmission": {}, "KHR_materials_ior": {"ior": 2.0}})).material_transmission(2) == OPAQUE
    assert _load(glass_glb(pane={"KHR_materials_transmission": {"transmissionFactor": 0}})).material_transmission(2) == OPAQUE


def test_appends_with_the_scene_offsets():
    s = _load(glass_glb())
    _load(glass_glb(), s)
    assert s.counts().materials == 7
    assert s.material_transmission(2) == s.material_transmission(5) == (1.0, 1.5, True) and s.material_transmission(4) == OPAQUE and s.material_transmission(6)[2] is False


@pytest.mark.parametrize("pane", [{"KHR_materials_transmission": {"transmissionFactor": -0.1}}, {"KHR_materials_transmission": {"transmissionFactor": 1.5}},
                                  {"KHR_materials_transmission": {"transmissionFactor": "1"}}, {"KHR_materials_transmission": {"transmissionFactor": 1e999}},
                                  {"KHR_materials_transmission": {"transmissionFactor": 1}, "KHR_materials_ior": {"ior": 0.9}},
                                  {"KHR_materials_ior": {"ior": 0.5}}, {"KHR_materials_ior": {"ior": 1e999}}, {"KHR_materials_ior": {"ior": [1.5]}},
                                  {"KHR_materials_transmission": {"transmissionFactor": 1}, "KHR_materials_volume": {"thicknessFactor": "thick"}}])
def test_rejected_input_leaves_the_scene_untouched(pane):
    s = _load(glass_glb())
    before = _snapshot(s)
    with pytest.raises(lp.Error) as e:
        _load(glass_glb(pane=pane), s)
    assert e.value.kind == "FileNotFound"
    assert _snapshot(s) == before


def test_a_file_without_the_extensions_loads_as_before(cornell_glb):
    s = _load(cornell_glb)
    c = s.counts()
    assert all(s.material_transmission(m) == OPAQUE for m in range(c.materials))
    from oracle import gltf_oracle as G
    o = G.Scene()
    G.load_gltf(cornell_glb, o)
    for name in ("materials", "instances", "vertices", "indices", "entries"):
        assert getattr(s, name).tobytes() == np.ascontiguousarray(getattr(o, name)).tobytes(), name
    # the same file with and without the extensions: everything but the side table is the same bytes
    a, b = _snapshot(_load(glass_glb())), _snapshot(_load(glass_glb(pane=None, cube=None)))
    assert a[:-1] == b[:-1] and a[-1] != b[-1] and all(t == OPAQUE for t in b[-1])


# ---------------------------------------------------------------- scene API
def test_set_get_round_trip_and_factor_zero_is_opaque():
    s = lp.Scene()
    m = s.add_material((1, 1, 1, 1), 0.5, 0.0)
    assert s.material_transmission(0) == OPAQUE and s.material_transmission(m) == OPAQUE
    before = s.materials.tobytes()
    s.set_material_transmission(m, 0.75)
    assert s.material_transmission(m) == (0.75, 1.5, True) and s.material_transmission(0) == OPAQUE
    s.set_material_transmission(m, 1.0, ior=1.0, thin_walled=False)
    assert s.material_transmission(m) == (1.0, 1.0, False)
    m2 = s.add_material((1, 1, 1, 1), 1.0, 0.0)      # a material added after the table was first written
    assert s.material_transmission(m2) == OPAQUE
    s.set_material_transmission(m, 0.0, ior=2.0, thin_walled=False)
    assert s.material_transmission(m)[0] == 0.0      # opaque again: the table entry of its triangles is 0 (material_tables.h trans_state reads factor > 0)
    assert s.materials[:2].tobytes() == before and A.MATERIAL_DT.itemsize == 32


@pytest.mark.parametrize("args", [(9, 0.5, 1.5, 1), (1, -0.1, 1.5, 1), (1, 1.1, 1.5, 1), (1, float("nan"), 1.5, 1), (1, 0.5, 0.99, 1), (1, 0.5, float("inf"), 1),
                                  (1, 0.5, float("nan"), 0), (1, float("inf"), 1.5, 0)])
def test_invalid_arguments_leave_the_scene_untouched(args):
    s = lp.Scene()
    m = s.add_material((1, 1, 1, 1), 1.0, 0.0)
    s.set_material_transmission(m, 0.25, 1.25, False)
    with pytest.raises(lp.Error) as e:
        s.set_material_transmission(*args)
    assert e.value.kind == "InvalidArg"
    assert s.material_transmission(m) == (0.25, 1.25, False)
    with pytest.raises(lp.Error) as e:
        s.material_transmission(2)
    assert e.value.kind == "InvalidArg"


def test_bindings_agree_on_the_new_entry_points():
    names = ("lpt_scene_set_material_transmission", "lpt_scene_get_material_transmission", "lpt_interface_sample")
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


# ---------------------------------------------------------------- the reference against the physics it restates (float64 unless stated)
def _dirs(n, seed, cmin=0.02):
    rng = np.random.default_rng(seed)
    c = rng.uniform(cmin, 1.0, n)
    phi = rng.uniform(0, 2 * np.pi, n)
    s = np.sqrt(1 - c * c)
    return np.c_[s * np.cos(phi), s * np.sin(phi), -c], c     # towards the plane z = 0 from above; N = +z


N_UP = np.array([0.0, 0.0, 1.0])


def test_snells_law_and_unit_directions():
    d, c = _dirs(2000, 1)
    for ior, entering in ((1.5, True), (1.33, True), (2.4, True), (1.5, False)):
        wi, w, tr = R.interface_sample(d, N_UP, N_UP, entering, (1, 1, 1), ior, False, 2.0, dtype=np.float64)      # r4 = 2: never reflects (unless Fr = 1: then r4 < 1 fails too)
        eta = 1 / ior if entering else ior
        tir = eta * eta * (1 - c * c) >= 1
        assert tr.all()          # r4 >= Fr always
        ok = ~tir
        sin_i, sin_t = np.sqrt(1 - c[ok] ** 2), np.linalg.norm(wi[ok][:, :2], axis=1)
        assert np.allclose(sin_t, eta * sin_i, atol=1e-12) and np.allclose(np.linalg.norm(wi[ok], axis=1), 1.0, atol=1e-12) and (wi[ok][:, 2] < 0).all()
        # the refracted ray stays in the plane of incidence
        assert np.allclose(np.cross(wi[ok], d[ok]) @ N_UP, 0.0, atol=1e-12)
    # reflection: mirror about N
    wi, w, tr = R.interface_sample(d, N_UP, N_UP, True, (0.2, 0.3, 0.4), 1.5, False, -1.0, dtype=np.float64)
    assert not tr.any() and np.allclose(wi, d * (1, 1, -1), atol=1e-12) and (w == 1).all()


def test_fresnel_range_reciprocity_and_normal_incidence():
    c = np.linspace(1e-4, 1.0, 4001)
    for ior in (1.0, 1.1, 1.5, 2.4):
        for eta in (1 / ior, ior):
            Fr, ct = R.fresnel(c, np.full_like(c, eta))
            assert ((Fr >= 0) & (Fr <= 1)).all()
            ok = Fr < 1
            back, _ = R.fresnel(ct[ok], np.full(ok.sum(), 1 / eta))           # Fr(theta_i, eta) = Fr(theta_t, 1 / eta)
            assert np.allclose(back, Fr[ok], rtol=1e-9, atol=1e-15)
        F0, _ = R.fresnel(np.array([1.0]), np.array([1 / ior]))
        assert np.isclose(F0[0], ((ior - 1) / (ior + 1)) ** 2, rtol=1e-12, atol=1e-18)
    Ff, _ = R.fresnel(c.astype(np.float32), np.full(c.size, 1 / 1.5, np.float32))
    assert Ff.dtype == np.float32 and ((Ff >= 0) & (Ff <= 1)).all()


def test_total_internal_reflection_exactly_from_the_critical_angle():
    """exiting (eta = ior): s2 = eta^2 (1 - c^2) >= 1 is total reflection — in float32, decided by that very comparison: the reference's Fr is exactly 1 on one side
    and below 1 on the other, with no band in between"""
    f = np.float32
    ior = f(1.5)
    cc = np.sqrt(1 - 1 / (1.5 * 1.5))
    c = (cc + np.linspace(-1e-5, 1e-5, 2001)).astype(f)
    s2 = (ior * ior) * np.maximum(f(0), f(1) - c * c)
    Fr, ct = R.fresnel(c, np.full(c.size, ior, f))
    assert np.array_equal(Fr == 1, s2 >= 1) and (s2 >= 1).any() and (s2 < 1).any()
    assert (ct[s2 >= 1] == 0).all() and (Fr[s2 < 1] < 1).all()
    d = np.c_[np.sqrt(np.maximum(0, 1 - c.astype(np.float64) ** 2)), np.zeros(c.size), -c.astype(np.float64)]
    wi, w, tr = R.interface_sample(d, N_UP, N_UP, False, (1, 1, 1), 1.5, False, 0.999999, dtype=np.float64)
    c64 = np.minimum(-d[:, 2], 1.0)
    tir = 2.25 * (1 - c64 * c64) >= 1
    assert np.array_equal(~tr, tir | (R.fresnel(c64, np.full(c.size, 1.5))[0] > 0.999999))
    # entering never reflects totally
    assert (R.fresnel(np.linspace(0, 1, 1001), np.full(1001, 1 / 1.5))[1][1:] > 0).all()


def test_ior_one_is_no_interface():
    d, c = _dirs(2000, 3, cmin=0.1)
    Fr, ct = R.fresnel(c, np.ones_like(c))
    assert (Fr <= 1e-24).all()                     # ct = sqrt(1 - (1 - c^2)) = c to a few ulp: rs, rp ~ 1e-15 / c
    wi, w, tr = R.interface_sample(d, N_UP, N_UP, True, (0.5, 0.6, 0.7), 1.0, False, 1e-12, dtype=np.float64)      # (r4 = 0 would still reflect where rounding leaves Fr = 1e-30)
    assert tr.all() and np.allclose(wi, d, atol=1e-14) and np.array_equal(w, np.tile((0.5, 0.6, 0.7), (2000, 1)))
    # float32: within the format's precision (Fr is a square of ~2^-24 / c^2 terms)
    wi, w, tr = R.interface_sample(d, N_UP, N_UP, True, (0.5, 0.6, 0.7), 1.0, False, 1e-6)
    assert tr.all() and np.abs(wi - d.astype(np.float32)).max() <= 4 * 2.0 ** -24


def test_thin_walled_goes_straight_on_and_the_fallback_normal():
    d, c = _dirs(500, 4)
    for entering in (True, False):
        wi, w, tr = R.interface_sample(d, N_UP, N_UP, entering, (0.5, 1, 0.25), 1.5, True, 2.0)
        assert tr.all() and np.array_equal(wi, d.astype(np.float32)) and np.array_equal(w, np.tile(np.float32((0.5, 1, 0.25)), (500, 1)))
    # a shading normal that faces away from V is replaced by Ngf; one that puts the result on the wrong side is, too
    away = np.array([0.0, 0.0, -1.0])
    a = R.interface_sample(d, away, N_UP, True, (1, 1, 1), 1.5, False, -1.0)
    b = R.interface_sample(d, N_UP, N_UP, True, (1, 1, 1), 1.5, False, -1.0)
    assert np.array_equal(a[0], b[0])
    g = np.array([[0.995, 0.0, -0.0998749]])       # grazing; Ns tilted along the ray: mirroring about it sends the ray below the surface
    g /= np.linalg.norm(g)
    tilted = np.array([0.09, 0.0, 0.996]) / np.linalg.norm([0.09, 0.0, 0.996])      # dot(V, Ns) = 0.01 > 0, and 2 c Ns.z < V.z
    wi, _, tr = R.interface_sample(g, tilted, N_UP, True, (1, 1, 1), 1.5, False, -1.0, dtype=np.float64)
    assert not tr[0] and wi[0, 2] > 0 and np.allclose(wi[0], g[0] * (1, 1, -1), atol=1e-12)


def test_expectation_of_a_thin_pane_is_its_closed_form():
    """one pane before a constant probe, depth 2: E = L (Fr + (1 - Fr) base), the zero mass is 0; depth 1: every pane sample is truncated"""
    from loupiote_amd import testing as T
    view = T.look((0, 0, 0), (0, 0, -1))
    pane = R.rect((0, 0, -2), (1, 0, 0), (0, 1, 0), 0.4, 0.4, kind="thin", ior=1.5, base=(0.5, 1.0, 0.25))
    px = np.array([[32, 32], [20, 40], [0, 0]])
    mean, var, pz = R.expectation([pane], (1, 1, 1), view, 0.6, 64, 64, 2, 4, px)
    _, d = R.camera_rays(view, 0.6, 64, 64, (np.arange(4) + 0.5) / 4)
    for k in range(2):
        Fr = R.fresnel(-d[px[k, 0], px[k, 1]][:, 2], np.full(16, 1 / 1.5))[0]
        assert np.allclose(mean[k], (Fr[:, None] + (1 - Fr)[:, None] * np.array([0.5, 1.0, 0.25])).mean(0), rtol=1e-12)
        assert var[k, 1] < 1e-24 and var[k, 0] > 0 and pz[k] == 0
    assert np.array_equal(mean[2], (1, 1, 1)) and (var[2] == 0).all()        # beside the pane: the probe
    mean, var, pz = R.expectation([pane], (1, 1, 1), view, 0.6, 64, 64, 1, 2, px)
    assert (pz[:2] == 1).all() and (mean[:2] == 0).all() and pz[2] == 0
