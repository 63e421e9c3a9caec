"""CPU: volume attenuation (SPEC.md §28) on the host — the scene API's state and the absorption coefficient it derives, tests/volume_ref.py against binary64
exp(-sigma t) within its own rounding model, what the glTF loader reads from KHR_materials_volume, the bindings' agreement on the new entry points, and the
transmission table's sigma rows (tests/tools/volume_tables_check.cpp, a stand-alone program under AddressSanitizer + UBSan)."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import _abi as A

import volume_ref as V
from test_gpu_transmission import glass_glb
from test_gpu_volume import TINT, TINT_D, tinted_glb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF = float("inf")
FLT_MAX = float(np.finfo(F).max)
NONE = ((1.0, 1.0, 1.0), INF, (0.0, 0.0, 0.0))


def _state(s, m):
    c, d, sg = s.material_attenuation(m)
    return tuple(float(x) for x in c), d, tuple(float(x) for x in sg)


def _bits(x):
    return np.asarray(x, F).view(np.uint32).astype(np.int64)


# ---------------------------------------------------------------- 1. the scene API
def test_set_get_round_trip_and_defaults():
    s = lp.Scene()
    m = s.add_material((1, 1, 1, 1), 0.5, 0.0)
    assert _state(s, 0) == NONE and _state(s, m) == NONE
    before = s.materials.tobytes()
    s.set_material_attenuation(m, TINT, TINT_D)
    c, d, sg = s.material_attenuation(m)
    assert np.array_equal(c, F(TINT)) and d == 0.5 and c.dtype == sg.dtype == F and _state(s, 0) == NONE
    assert (np.abs(_bits(sg) - _bits(V.sigma(TINT, TINT_D))) <= 1).all() and (sg > 0).all()
    m2 = s.add_material((1, 1, 1, 1), 1.0, 0.0)          # a material added after the table was first written
    assert _state(s, m2) == NONE
    s.set_material_attenuation(m, (1.0, 1.0, 1.0))       # the default distance is +inf: none
    assert _state(s, m) == NONE
    assert s.materials[:2].tobytes() == before and s.material_transmission(m) == (0.0, 1.5, True)       # beside the transmission state and independent of it
    # NULL out-pointers
    assert A.lib().lpt_scene_get_material_attenuation(s._h, m, None, None, None) == 0


def test_the_state_survives_factor_zero_and_back():
    s = lp.Scene()
    m = s.add_material((1, 1, 1, 1), 0.5, 0.0)
    s.set_material_transmission(m, 1.0, 1.5, False)
    s.set_material_attenuation(m, TINT, TINT_D)
    want = _state(s, m)
    s.set_material_transmission(m, 0.0)
    assert _state(s, m) == want
    s.set_material_transmission(m, 0.5, 1.33, True)
    assert _state(s, m) == want and s.material_transmission(m) == (0.5, float(F(1.33)), True)


@pytest.mark.parametrize("args", [(9, (0.5, 0.5, 0.5), 1.0), (1, (1.5, 0.5, 0.5), 1.0), (1, (0.5, -0.1, 0.5), 1.0), (1, (0.5, 0.5, float("nan")), 1.0), (1, (INF, 0.5, 0.5), 1.0),
                                  (1, (0.5, 0.5, 0.5), 0.0), (1, (0.5, 0.5, 0.5), -1.0), (1, (0.5, 0.5, 0.5), float("nan")), (1, (0.5, 0.5, 0.5), -INF), (1, (0.5, 0.5, 0.5), -0.0)])
def test_invalid_arguments_leave_the_state_untouched(args):
    s = lp.Scene()
    m = s.add_material((1, 1, 1, 1), 1.0, 0.0)
    s.set_material_attenuation(m, (0.25, 0.5, 1.0), 2.0)
    want = _state(s, m)
    with pytest.raises(lp.Error) as e:
        s.set_material_attenuation(*args)
    assert e.value.kind == "InvalidArg"
    assert _state(s, m) == want and _state(s, 0) == NONE
    with pytest.raises(lp.Error) as e:
        s.material_attenuation(2)
    assert e.value.kind == "InvalidArg"


SIGMA_CASES = [((0.0, 1.0, 0.5), 0.5), ((1.0, 1.0, 1.0), 0.5), (TINT, INF), ((0.0, 0.5, 1.0), INF), ((0.5, 0.9, 0.999), 1e-40), ((0.2, 0.8, 0.4), 0.5), ((1e-45, 1e-30, 0.99999994), 3e38),
               ((0.5, 0.25, 0.125), 1e-38), ((0.99999994, 0.5, 0.1), 1e30), ((0.3, 0.6, 0.9), 7.25)]


@pytest.mark.parametrize("color,distance", SIGMA_CASES)
def test_sigma_equals_the_reference_within_one_ulp(color, distance):
    s = lp.Scene()
    m = s.add_material((1, 1, 1, 1), 1.0, 0.0)
    s.set_material_attenuation(m, color, distance)
    c, d, sg = s.material_attenuation(m)
    want = V.sigma(c, F(d))
    assert np.all(np.isfinite(sg)) and (sg >= 0).all() and not np.signbit(sg).any()
    assert (np.abs(_bits(sg) - _bits(want)) <= 1).all(), (sg, want)
    for k in range(3):
        if c[k] == 1 or np.isinf(d):
            assert sg[k] == 0
        elif c[k] == 0 or -np.log(float(c[k])) / d > FLT_MAX:
            assert sg[k] == F(FLT_MAX)         # c = 0, and a quotient that overflows
    if distance == 1e-40:
        assert sg[0] == sg[1] == F(FLT_MAX) and 0 < sg[2] < F(FLT_MAX)      # 0.69 / 1e-40 and 0.1 / 1e-40 overflow, 1e-3 / 1e-40 does not


def test_bindings_agree_on_the_new_entry_points():
    names = ("lpt_scene_set_material_attenuation", "lpt_scene_get_material_attenuation", "lpt_scene_gpu_attenuation")
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
        assert "%s(" % n in hpp, n
        assert hasattr(A.lib(), n)
    assert "ffi::lpt_scene_set_material_attenuation(" in safe and "ffi::lpt_scene_get_material_attenuation(" in safe
    assert A.lib().lpt_abi_version() == 6      # new entry points only: no layout changed


# ---------------------------------------------------------------- 2. the reference against binary64
def test_atten_against_binary64_within_the_rounding_model():
    rng = np.random.default_rng(28)
    n = 200000
    sig = np.exp(rng.uniform(np.log(1e-6), np.log(1e4), n)).astype(F)
    t = np.exp(rng.uniform(np.log(1e-6), np.log(1e4), n)).astype(F)
    a = V.atten(sig, t)
    x = sig.astype(np.float64) * t.astype(np.float64)
    y32 = (sig * t) * V.LOG2E
    below = y32 < F(125.0)
    assert np.array_equal(a == 0, ~below)                       # A = 0 from y >= 125 on, and nowhere below
    assert below.sum() > 100000 and (~below).sum() > 1000
    true = np.exp(-x[below])
    frac = np.abs(a[below].astype(np.float64) - true) / true / V.bound(x[below])
    print("atten: %d pairs below y = 125, the largest fraction of the bound (3x + 8) 2^-24 in use: %.3f (at x = %.4g)" % (below.sum(), frac.max(), x[below][frac.argmax()]))
    assert frac.max() <= 1.0
    assert not np.isnan(a).any() and ((a == 0) | (a >= np.finfo(F).tiny)).all() and (a <= 1).all()


def test_atten_at_the_edges():
    tiny = np.finfo(F).tiny
    fmax = F(FLT_MAX)
    # t = 0, sigma = 0: exactly 1
    assert V.atten(F(3.5), F(0)) == 1 and V.atten(F(0), F(3e38)) == 1 and V.atten(fmax, F(0)) == 1
    # FLT_MAX with t tiny: x is huge, or overflows: 0
    assert V.atten(fmax, F(1e-30)) == 0 and V.atten(fmax, F(2.0)) == 0 and V.atten(F(3e38), F(3e38)) == 0      # sigma t = +inf
    with np.errstate(invalid="ignore"):
        assert V.atten(F(0), F(INF)) == 0 and V.atten(F(np.nan), F(1)) == 0                                    # 0 x inf = NaN: !(y < 125)
    # y one ulp below 125, and at 125
    for sig in (F(1.0), F(3.218876), F(0.44628707), F(1.8325814), fmax, F(1e-3)):
        t = F(125.0 / (float(V.LOG2E) * float(sig)))
        y = lambda t: (sig * F(t)) * V.LOG2E
        while y(t) >= F(125.0):
            t = np.nextafter(t, F(0))
        while y(np.nextafter(t, F(INF))) < F(125.0):
            t = np.nextafter(t, F(INF))
        lo, hi = V.atten(sig, t), V.atten(sig, np.nextafter(t, F(INF)))
        assert hi == 0 and lo >= tiny and lo < 2.0 ** -124, (sig, t, lo, hi)
        x = float(sig) * float(t)
        assert abs(float(lo) - np.exp(-x)) / np.exp(-x) <= V.bound(x)
    k125 = V.atten(F(1.0), np.nextafter(F(125.0) / V.LOG2E, F(0)))
    assert k125 >= tiny
    # small arguments: 1 - x to the model
    for x in (1e-10, 1e-7, 1e-3, 0.3465, 0.3467, 0.5, 1.0):
        a = float(V.atten(F(1.0), F(x)))
        assert abs(a - np.exp(-float(F(x)))) / np.exp(-float(F(x))) <= V.bound(float(F(x)))
    # monotone in the large: more absorbing, darker
    assert V.atten(F(2.0), F(1.0)) < V.atten(F(1.0), F(1.0)) < V.atten(F(0.5), F(1.0))


def test_the_coefficients_are_the_series():
    want = [1.0, -1.0, 0.5, -1.0 / 6, 1.0 / 24, -1.0 / 120, 1.0 / 720, -1.0 / 5040]
    assert [float(c) for c in V.COEF] == [float(F(w)) for w in want]
    assert float(V.LOG2E) == float(F(1.4426950408889634)) and float(V.LN2) == float(F(0.6931471805599453))


def test_expectation_of_a_slab_is_its_closed_form():
    """a solid slab of index 1 seen head on: the one path crosses it once, E = L exp(-sigma h / cos); without sigma the reference is transmission_ref's"""
    import transmission_ref as R
    from loupiote_amd import testing as T
    view = T.look((0, 0, 0), (0, 0, -1))
    sig = np.array([3.0, 0.5, 0.0])
    mk = lambda **kw: [V.rect((0, 0, -2), (1, 0, 0), (0, 1, 0), 1.5, 1.5, kind="solid", ior=1.0, **kw), V.rect((0, 0, -2.5), (0, 1, 0), (1, 0, 0), 1.5, 1.5, kind="solid", ior=1.0, **kw)]
    px = np.array([[32, 32], [20, 40]])
    mean, var, pz = V.expectation(mk(sigma=sig), (1, 1, 1), view, 0.6, 64, 64, 4, 1, px)
    _, d = V.camera_rays(view, 0.6, 64, 64, np.array([0.5]))
    for k in range(2):
        cos = -d[px[k, 0], px[k, 1], 0, 2]
        assert np.allclose(mean[k], np.exp(-sig * 0.5 / cos), rtol=1e-12) and (pz[k] < 1e-20) and (var[k] < 1e-20).all()
    a, b = V.expectation(mk(), (1, 1, 1), view, 0.6, 64, 64, 4, 2, px), R.expectation(mk(), (1, 1, 1), view, 0.6, 64, 64, 4, 2, px)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # a front-face hit is not attenuated: a single face with sigma, hit from outside, passes the probe whole
    mean, _, _ = V.expectation(mk(sigma=sig)[:1], (1, 1, 1), view, 0.6, 64, 64, 4, 1, px)
    assert np.allclose(mean, 1.0, rtol=1e-12)


# ---------------------------------------------------------------- 3. the loader
def _load(glb, into=None):
    s = lp.Scene() if into is None else into
    lp.loaders.load_gltf(glb, s)
    return s


def _snapshot(s):
    c = s.counts()
    n = c.materials
    return (tuple(getattr(c, f) for f, _ in c._fields_), s.materials.tobytes(), s.instances.tobytes(), s.vertices.tobytes(), s.indices.tobytes(), s.punctual_lights.tobytes(),
            tuple(s.material_alpha(m) for m in range(n)), tuple(s.material_transmission(m) for m in range(n)),
            tuple((tuple(map(float, le)), im) for le, im in (s.material_emission(m) for m in range(n))), tuple(s.material_normal_map(m) for m in range(n)),
            tuple(_state(s, m) for m in range(n)))


def test_the_golden_file_and_the_defaults():
    with open(os.path.join(ROOT, "tests", "golden", "tinted-glass.glb"), "rb") as f:
        data = f.read()
    assert data == tinted_glb() and len(data) < 8192
    s = _load(data)
    assert s.counts().materials == 3 and _state(s, 0) == NONE and _state(s, 1) == NONE
    c, d, sg = s.material_attenuation(2)
    assert np.array_equal(c, F(TINT)) and d == TINT_D and (np.abs(_bits(sg) - _bits(V.sigma(TINT, TINT_D))) <= 1).all()
    assert s.material_transmission(2) == (1.0, 1.5, False)
    # either key alone: the other keeps its default
    assert _state(_load(tinted_glb(volume={"thicknessFactor": 0.5, "attenuationColor": [0.5, 1, 1]})), 2) == ((0.5, 1.0, 1.0), INF, (0.0, 0.0, 0.0))
    c, d, sg = _load(tinted_glb(volume={"thicknessFactor": 0.5, "attenuationDistance": 2})).material_attenuation(2)
    assert tuple(c) == (1.0, 1.0, 1.0) and d == 2.0 and (sg == 0).all()
    # stored whatever the factor and the thickness say: a thin-walled and an opaque material keep them
    assert _state(_load(tinted_glb(volume={"attenuationColor": list(TINT), "attenuationDistance": TINT_D})), 2) == _state(s, 2)
    g = _load(glass_glb(pane={"KHR_materials_volume": {"attenuationColor": list(TINT), "attenuationDistance": TINT_D}}))
    assert g.material_transmission(2)[0] == 0.0 and _state(g, 2) == _state(s, 2)
    # appended with the scene's offsets
    _load(data, s)
    assert s.counts().materials == 5 and _state(s, 4) == _state(s, 2) and _state(s, 3) == NONE


@pytest.mark.parametrize("volume", [{"attenuationColor": [0.2, 0.8]}, {"attenuationColor": [0.2, 1.5, 0.4]}, {"attenuationColor": [0.2, -0.1, 0.4]}, {"attenuationDistance": 0},
                                    {"attenuationDistance": -1.0}, {"attenuationDistance": "far"}, {"attenuationColor": [0.2, "0.8", 0.4]}, {"attenuationColor": 0.5},
                                    {"attenuationDistance": 1e999}, {"attenuationDistance": 1e39}, {"attenuationDistance": 1e-60}, {"attenuationColor": [0.2, 0.8, 0.4, 1.0]}])
def test_rejected_input_leaves_the_scene_untouched(volume):
    s = _load(tinted_glb())
    before = _snapshot(s)
    with pytest.raises(lp.Error) as e:
        _load(tinted_glb(volume=dict(volume, thicknessFactor=0.5)), s)
    assert e.value.kind == "FileNotFound"
    assert _snapshot(s) == before


def test_files_without_the_keys_load_as_before():
    with open(os.path.join(ROOT, "tests", "golden", "glass-pane.glb"), "rb") as f:
        glass = f.read()
    s = _load(glass)
    assert all(_state(s, m) == NONE for m in range(s.counts().materials))
    assert s.material_transmission(2) == (1.0, 1.5, True) and s.material_transmission(3) == (float(F(0.9)), float(F(1.33)), False)
    # the golden file with the two keys stripped loads equal to a load of itself that never saw them: everything but the attenuation state is the same bytes
    a, b = _snapshot(_load(tinted_glb())), _snapshot(_load(tinted_glb(volume={"thicknessFactor": 0.5})))
    assert a[:-1] == b[:-1] and a[-1] != b[-1] and all(t == NONE for t in b[-1])


# ---------------------------------------------------------------- 4. the side tables: the sigma rows beside the transmission records
def Fb(x):
    return int(np.float32(x).view(np.uint32))


def _row(color, distance):
    return [int(b) for b in _bits(V.sigma(color, distance))] + [0]


TWO = ["scene 4", "trans 1 1 1.5 0", "atten 1 0.2 0.8 0.4 0.5", "trans 2 0.5 1.25 0", "atten 2 0 1 0.5 2"]
TABLE_CASES = {
    "a solid attenuating material: .w = 1 and its row": (
        ["scene 2", "trans 1 1 1.5 0", "atten 1 0.2 0.8 0.4 0.5", "inst 1 0 2", "tris 2"], ([[Fb(1), Fb(1.5), 0, Fb(1)]], [_row(TINT, 0.5)], [1, 1])),
    "the same material thin-walled: .w = 0, no row anywhere": (
        ["scene 2", "trans 1 1 1.5 1", "atten 1 0.2 0.8 0.4 0.5", "inst 1 0 2", "tris 2"], ([[Fb(1), Fb(1.5), Fb(1), 0]], [], [1, 1])),
    "sigma = 0 by the colour": (["scene 2", "trans 1 1 1.5 0", "atten 1 1 1 1 0.5", "inst 1 0 2", "tris 2"], ([[Fb(1), Fb(1.5), 0, 0]], [], [1, 1])),
    "sigma = 0 by the distance": (["scene 2", "trans 1 1 1.5 0", "atten 1 0.2 0.8 0.4 inf", "inst 1 0 2", "tris 2"], ([[Fb(1), Fb(1.5), 0, 0]], [], [1, 1])),
    "an opaque material keeps its attenuation out of the table": (["scene 2", "atten 1 0.2 0.8 0.4 0.5", "inst 1 0 2", "tris 2"], ([], [], [])),
    "rows in first-use order, parallel to the records: 2, 1": (
        TWO + ["inst 2 0 1", "inst 1 1 2", "inst 0 3 1", "inst 2 4 1", "tris 5"],
        ([[Fb(0.5), Fb(1.25), 0, Fb(1)], [Fb(1), Fb(1.5), 0, Fb(1)]], [_row((0.0, 1.0, 0.5), 2.0), _row(TINT, 0.5)], [1, 2, 2, 0, 1])),
    "a clear solid beside a tinted one: a zero row stands in": (
        TWO + ["trans 3 1 1.5 0", "inst 3 0 1", "inst 1 1 1", "tris 2"], ([[Fb(1), Fb(1.5), 0, 0], [Fb(1), Fb(1.5), 0, Fb(1)]], [[0, 0, 0, 0], _row(TINT, 0.5)], [1, 2])),
    "a thin pane beside a tinted solid: .w = 0 and a zero row": (
        TWO + ["trans 3 1 1.5 1", "atten 3 0.5 0.5 0.5 1", "inst 1 0 1", "inst 3 1 1", "tris 2"],
        ([[Fb(1), Fb(1.5), 0, Fb(1)], [Fb(1), Fb(1.5), Fb(1), 0]], [_row(TINT, 0.5), [0, 0, 0, 0]], [1, 2])),
    "an unused attenuating material leaves no row": (TWO + ["trans 3 1 1.5 0", "inst 3 0 2", "tris 2"], ([[Fb(1), Fb(1.5), 0, 0]], [], [1, 1])),
}


@pytest.fixture(scope="module")
def table_results(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("voltab") / "volume_tables_check")
    src = [os.path.join(ROOT, "tests", "tools", "volume_tables_check.cpp"), os.path.join(ROOT, "loupiote_amd", "csrc", "scene.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include")] + src + ["-o", exe])
    lines = [l for cmds, _ in TABLE_CASES.values() for l in cmds + ["derive"]]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:allocator_may_return_null=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0 and not p.stderr, (p.stdout[-2000:], p.stderr[-4000:])       # clean under the sanitizers
    out = [json.loads(l) for l in p.stdout.splitlines()]
    assert len(out) == len(TABLE_CASES)
    return dict(zip(TABLE_CASES, out))


@pytest.mark.parametrize("name", list(TABLE_CASES))
def test_sigma_rows(table_results, name):
    got, (recs, more, tri) = table_results[name], TABLE_CASES[name][1]
    assert got["status"] == 0 and got["others"] == 0           # the other three kinds have no second record
    assert got["recs"] == recs and got["tri"] == tri
    assert len(got["more"]) == len(more)
    for g, w in zip(got["more"], more):                          # the rows: the reference's sigma within one ulp (bit for bit where it is 0 or FLT_MAX)
        assert all(abs(a - b) <= 1 for a, b in zip(g, w)) and g[3] == 0, (g, w)
    assert len(got["more"]) in (0, len(got["recs"]))
