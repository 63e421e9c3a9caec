"""CPU: rough transmission (SPEC.md §29) on the host — the sampler of tests/rough_ref.py against Walter et al.'s closed-form rough dielectric BSDF, its smooth
fallback against tests/transmission_ref.py bit for bit, the scene API's rough bit, what the glTF loader's LPT_GLTF_READ_ROUGH_TRANSMISSION marks, the bindings'
agreement on the new entry points, and the transmission table's rough bit (tests/tools/rough_tables_check.cpp, a stand-alone program under AddressSanitizer + UBSan).

THE SAMPLER AGAINST THE CLOSED FORM.  For a configuration (side, angle, roughness) 2^18 float64 events are drawn; the directions are binned on a 16 x 32
(theta, phi) grid about the normal, and a bin's estimate — the mean over ALL draws of weight x [wi in the bin] — is compared with the quadrature of f |cos| over
the bin (rough_ref.binned_bsdf).  The bound per bin is 6 standard errors of that estimate, from the draws' own per-bin variance, plus the quadrature's stated
error (its distance from the rule at half the resolution).  Bins with fewer than 64 draws may be left out, up to 5 % of the closed form's total mass, which
the reference alone decides (asserted).  Leaving out all of them would break that cap in one configuration — the thin pane at roughness 1, whose reflected
hemisphere holds 5 % of the weight spread over 256 bins of 4 to 60 draws each: 5.13 % —, so the test leaves out FEWER: only the bins with fewer than
MIN_DRAWS = 32 draws (at most 2.7 % of the mass in any configuration).  A bin of 32 draws has a standard error of some 18 % of its value, which the bound carries.
The total weight is at most 1 + 6 standard errors."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import _abi as A

import rough_ref as RR
import transmission_ref as TR
from test_gpu_transmission import glass_glb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
N_DRAWS = 1 << 18
MIN_DRAWS = 32
Z = np.array([0.0, 0.0, 1.0])
CRIT = float(np.degrees(np.arcsin(1 / 1.5)))       # 41.81 degrees
BASE = 0.8

# (name, entering, thin, the angle of V against the normal in degrees)
GEOMETRY = [("entering-0", True, False, 0.0), ("entering-60", True, False, 60.0), ("exiting-30", False, False, 30.0), ("exiting-past-critical", False, False, CRIT + 0.5),
            ("thin-45", True, True, 45.0)]
ROUGHNESS = [0.2, 0.5, 1.0]


def _view(deg):
    t = np.radians(deg)
    return np.array([np.sin(t), 0.0, np.cos(t)])


# ---------------------------------------------------------------- 1. the sampler against the closed form
@pytest.mark.parametrize("rough", ROUGHNESS)
@pytest.mark.parametrize("geometry", GEOMETRY, ids=[g[0] for g in GEOMETRY])
def test_sampler_against_the_closed_form(geometry, rough):
    name, entering, thin, deg = geometry
    V = _view(deg)
    eta = 1 / 1.5 if (thin or entering) else 1.5
    a2 = rough ** 4
    rng = np.random.default_rng(29)
    r4, u1, u2 = rng.random(N_DRAWS), rng.random(N_DRAWS), rng.random(N_DRAWS)
    wi, weight, kind = RR.interface_sample_rough(np.broadcast_to(-V, (N_DRAWS, 3)), Z, Z, entering, (BASE, BASE, BASE), 1.5, thin, rough, r4, u1, u2, dtype=np.float64)
    assert not (kind & RR.KIND_SMOOTH).any()
    w = weight[:, 0]
    live = kind != RR.KIND_ENDED
    assert np.all(np.isfinite(wi)) and np.all(np.isfinite(w)) and (w[~live] == 0).all() and (w >= 0).all() and (w <= 1).all()
    assert np.allclose(np.linalg.norm(wi[live], axis=1), 1.0, atol=1e-12)
    # the total weight: what one event keeps of the energy
    total, total_se = w.mean(), w.std(ddof=1) / np.sqrt(N_DRAWS)
    assert total <= 1 + 6 * total_se
    want, quad = RR.binned_bsdf(V, Z, eta, a2, BASE, thin)
    it, ip = RR.bin_of(wi[live], Z)
    flat = it * 32 + ip
    count = np.bincount(flat, minlength=512).reshape(16, 32)
    s1 = np.bincount(flat, weights=w[live], minlength=512).reshape(16, 32) / N_DRAWS
    s2 = np.bincount(flat, weights=w[live] ** 2, minlength=512).reshape(16, 32) / N_DRAWS
    se = np.sqrt(np.maximum(s2 - s1 * s1, 0.0) / (N_DRAWS - 1))
    kept = count >= MIN_DRAWS
    left_out = want[~kept].sum() / want.sum()
    assert left_out <= 0.05, left_out                    # decided by the closed form alone
    miss = np.abs(s1 - want) / (6 * se + quad + 1e-300)
    print("%s rough %.1f: total %.4f +- %.4f (closed form %.4f), reflected %.3f, ended %.4f, %d bins kept, %.2e of the mass left out, worst bin %.2f of its bound, "
          "quadrature error at most %.1e" % (name, rough, total, total_se, want.sum(), (kind == 0).mean(), (~live).mean(), kept.sum(), left_out, miss[kept].max(), quad.max()))
    assert (miss[kept] <= 1.0).all(), (np.argwhere(kept & (miss > 1)), s1[kept & (miss > 1)], want[kept & (miss > 1)])
    assert abs(total - want.sum()) <= 6 * total_se + quad.sum()
    if name == "exiting-past-critical" and rough == 0.2:
        assert (kind == 0).mean() > 0.4                  # a smooth interface would reflect it all; a frosted one still mostly does


def test_the_closed_form_conserves_energy_at_low_roughness():
    """Walter's BSDF, all by itself: a white interface of roughness 0.3 keeps nearly all of the light (single scattering loses a little to masking), and no more
    than all of it, within the quadrature's stated error"""
    for entering, deg in ((True, 0.0), (True, 60.0), (False, 30.0)):
        want, quad = RR.binned_bsdf(_view(deg), Z, 1 / 1.5 if entering else 1.5, 0.3 ** 4, 1.0, False)
        assert 0.97 < want.sum() <= 1.0 + quad.sum(), (entering, deg, want.sum(), quad.sum())


# ---------------------------------------------------------------- 2. the smooth fallback, and the float32 event's own sanity
def _rows(n, seed=7):
    rng = np.random.default_rng(seed)
    unit = lambda a: a / np.linalg.norm(a, axis=-1, keepdims=True)
    ngf = unit(rng.normal(size=(n, 3)))
    d = unit(rng.normal(size=(n, 3)))
    d = np.where(((d * ngf).sum(1) > 0)[:, None], -d, d)
    ns = unit(ngf + 0.4 * rng.normal(size=(n, 3)))
    ns = np.where(((ns * ngf).sum(1) < 0)[:, None], -ns, ns)
    return [a.astype(F) for a in (d, ns, ngf)] + [rng.random(n) < 0.5, rng.random((n, 3)).astype(F), rng.uniform(1.0, 2.5, n).astype(F), rng.random(n) < 0.3] + \
           [rng.random(n).astype(F) for _ in range(3)]


def test_below_the_threshold_the_event_is_the_smooth_one_bit_for_bit():
    d, ns, ngf, entering, base, ior, thin, r4, u1, u2 = _rows(4096)
    below = np.nextafter(F(0.045), F(0))
    for rough in (below, F(0.0449), F(0.0), F(-1.0)):
        wi, w, kind = RR.interface_sample_rough(d, ns, ngf, entering, base, ior, thin, rough, r4, u1, u2)
        swi, sw, st = TR.interface_sample(d, ns, ngf, entering, base, ior, thin, r4)
        assert np.array_equal(wi.view(np.uint32), swi.view(np.uint32)) and np.array_equal(w.view(np.uint32), sw.view(np.uint32))
        assert np.array_equal(kind, 4 + st.astype(np.uint32))
    wi, w, kind = RR.interface_sample_rough(d, ns, ngf, entering, base, ior, thin, F(0.045), r4, u1, u2)
    assert not (kind & 4).any() and not np.array_equal(wi, swi)           # at the threshold: the rough event


def test_sincos2pi32_is_the_polynomial_and_close_to_the_functions():
    u = np.concatenate([np.linspace(0, 1, 100001)[:-1], [0.25, 0.5, 0.75, 1 - 2.0 ** -24]]).astype(F)
    s, c = RR.sincos2pi32(u)
    assert s.dtype == c.dtype == F
    assert np.abs(s - np.sin(2 * np.pi * u.astype(np.float64))).max() < 5e-6 and np.abs(c - np.cos(2 * np.pi * u.astype(np.float64))).max() < 5e-6
    # fma32 rounds once: against exact rational arithmetic on cases built to round twice in binary64
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a, b = rng.random(2000).astype(F), rng.random(2000).astype(F)
    cc = (rng.random(2000) * 2.0 ** rng.integers(-30, 2, 2000)).astype(F)
    got = RR.fma32(a, b, cc)
    for i in range(0, 2000, 7):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(cc[i]))
        lo, hi = np.nextafter(got[i], F(-np.inf)), np.nextafter(got[i], F(np.inf))
        assert abs(Fraction(float(got[i])) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact))


def test_float32_event_agrees_with_float64():
    d, ns, ngf, entering, base, ior, thin, r4, u1, u2 = _rows(20000, seed=11)
    for rough in (0.2, 1.0):
        a = RR.interface_sample_rough(d, ns, ngf, entering, base, ior, thin, F(rough), r4, u1, u2)
        b = RR.interface_sample_rough(d, ns, ngf, entering, base, ior, thin, F(rough), r4, u1, u2, dtype=np.float64)
        same = a[2] == b[2]
        assert same.mean() > 0.999                       # the pick and the side tests fall alike but at their edges
        assert np.abs(a[0][same] - b[0][same]).max() < 2e-4 and np.abs(a[1][same] - b[1][same]).max() < 2e-4


# ---------------------------------------------------------------- 3. the scene API
def test_rough_bit_defaults_round_trip_and_independence():
    s = lp.Scene()
    m = s.add_material((1, 1, 1, 1), 0.5, 0.0)
    assert s.material_transmission_rough(0) is False and s.material_transmission_rough(m) is False
    before = s.materials.tobytes()
    s.set_material_transmission(m, 1.0, 1.5, False, rough=True)
    assert s.material_transmission_rough(m) is True and s.material_transmission(m) == (1.0, 1.5, False) and s.material_transmission_rough(0) is False
    assert s.materials.tobytes() == before
    m2 = s.add_material((1, 1, 1, 1), 1.0, 0.0)          # a material added after the table was first written
    assert s.material_transmission_rough(m2) is False
    # the C ABI keeps the bit apart from the three numbers: factor 0 and back keeps it
    L = A.lib()
    assert L.lpt_scene_set_material_transmission(s._h, m, 0.0, 1.5, 1) == 0 and s.material_transmission_rough(m) is True
    assert L.lpt_scene_set_material_transmission(s._h, m, 0.5, 1.33, 1) == 0 and s.material_transmission_rough(m) is True
    assert s.material_transmission(m) == (0.5, float(F(1.33)), True)
    # ... and a bit set on an opaque material waits for the factor
    assert L.lpt_scene_set_material_transmission_rough(s._h, m2, 1) == 0 and s.material_transmission_rough(m2) is True and s.material_transmission(m2)[0] == 0.0
    assert L.lpt_scene_set_material_transmission_rough(s._h, m2, 0) == 0 and s.material_transmission_rough(m2) is False
    # Python's setter states the whole state, the bit included
    s.set_material_transmission(m, 0.5, 1.33, True)
    assert s.material_transmission_rough(m) is False
    assert L.lpt_scene_get_material_transmission_rough(s._h, m, None) == 0      # a NULL out-pointer


@pytest.mark.parametrize("material,on", [(9, 1), (9, 0), (1, 2), (1, 0xFFFFFFFF), (0xFFFFFFFF, 1)])
def test_invalid_arguments_leave_the_scene_untouched(material, on):
    s = lp.Scene()
    m = s.add_material((1, 1, 1, 1), 1.0, 0.0)
    s.set_material_transmission(m, 0.7, 1.4, False, rough=True)
    want = [(s.material_transmission(k), s.material_transmission_rough(k)) for k in range(2)]
    assert A.lib().lpt_scene_set_material_transmission_rough(s._h, material, on) == A.LPT_ERR_INVALID_ARG
    assert [(s.material_transmission(k), s.material_transmission_rough(k)) for k in range(2)] == want
    with pytest.raises(lp.Error) as e:
        s.material_transmission_rough(2)
    assert e.value.kind == "InvalidArg"
    assert A.lib().lpt_scene_set_material_transmission_rough(None, 0, 1) == A.LPT_ERR_INVALID_ARG


def test_bindings_agree_on_the_new_entry_points():
    names = ("lpt_scene_set_material_transmission_rough", "lpt_scene_get_material_transmission_rough", "lpt_interface_sample_rough")
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
        assert "%s(" % n in hpp and "ffi::%s(" % n in safe, n
        assert hasattr(A.lib(), n)
    assert re.search(r"#define LPT_GLTF_READ_ROUGH_TRANSMISSION 4u", header) and "pub const LPT_GLTF_READ_ROUGH_TRANSMISSION: u32 = 4;" in ffi
    assert A.GLTF_READ_ROUGH_TRANSMISSION == 4
    assert A.lib().lpt_abi_version() == 6      # new entry points only: no layout changed


# ---------------------------------------------------------------- 4. the loader
def _snapshot(s):
    c = s.counts()
    n = c.materials
    return (tuple(getattr(c, f) for f, _ in c._fields_), s.materials.tobytes(), s.instances.tobytes(), s.vertices.tobytes(), s.indices.tobytes(), s.punctual_lights.tobytes(),
            tuple(s.material_alpha(m) for m in range(n)), tuple(s.material_transmission(m) for m in range(n)),
            tuple((tuple(map(float, le)), im) for le, im in (s.material_emission(m) for m in range(n))), tuple(s.material_normal_map(m) for m in range(n)),
            tuple((tuple(map(float, c_)), d, tuple(map(float, sg))) for c_, d, sg in (s.material_attenuation(m) for m in range(n))),
            tuple(s.material_transmission_rough(m) for m in range(n)))


def _load_ex(data, flags, into=None):
    s = lp.Scene() if into is None else into
    buf = np.frombuffer(bytes(data), np.uint8)
    return s, A.lib().lpt_load_gltf_ex(s._h, A.ptr(buf), buf.size, flags)


def _golden(name):
    with open(os.path.join(ROOT, "tests", "golden", name), "rb") as f:
        return f.read()


@pytest.mark.parametrize("name", ["glass-pane.glb", "tinted-glass.glb", "frosted-glass.glb"])
def test_the_flag_marks_every_transmissive_material_and_no_other(name):
    data = _golden(name)
    plain = lp.Scene()
    lp.loaders.load_gltf(data, plain)
    base = _snapshot(plain)
    assert not any(base[-1])
    for flags in (0, 1):
        s, st = _load_ex(data, flags)
        assert st == 0 and _snapshot(s) == base         # without the flag: the loader of before, byte for byte
    for flags in (4, 5):
        s, st = _load_ex(data, flags)
        assert st == 0
        snap = _snapshot(s)
        assert snap[:-1] == base[:-1]
        n = s.counts().materials
        assert snap[-1] == tuple(s.material_transmission(m)[0] > 0 for m in range(n)) and any(snap[-1]) and not all(snap[-1])
    for kw, flags in ((dict(rough_transmission=True), 4), (dict(blend=True, rough_transmission=True), 5), (dict(blend=True), 1), ({}, 0)):
        s = lp.Scene()
        lp.loaders.load_gltf(data, s, **kw)
        assert _snapshot(s) == _snapshot(_load_ex(data, flags)[0])
        p = lp.Scene()
        lp.loaders.load_gltf_path(os.path.join(ROOT, "tests", "golden", name), p, **kw)
        assert _snapshot(p) == _snapshot(s)


@pytest.mark.parametrize("flags", [2, 3, 6, 7, 8, 12, 0x80000004])
def test_unknown_flag_bits_are_rejected_and_leave_the_scene_untouched(flags):
    s, st = _load_ex(glass_glb(), 4)
    assert st == 0
    before = _snapshot(s)
    assert _load_ex(glass_glb(), flags, s)[1] == A.LPT_ERR_INVALID_ARG and _snapshot(s) == before
    path = os.path.join(ROOT, "tests", "golden", "glass-pane.glb").encode()
    assert A.lib().lpt_load_gltf_path_ex(s._h, path, flags) == A.LPT_ERR_INVALID_ARG and _snapshot(s) == before


def test_the_flag_on_a_file_the_loader_rejects_and_on_an_appended_file():
    s, st = _load_ex(glass_glb(), 4)
    before = _snapshot(s)
    assert _load_ex(glass_glb(pane={"KHR_materials_transmission": {"transmissionFactor": 1.5}}), 4, s)[1] == A.LPT_ERR_FILE_NOT_FOUND and _snapshot(s) == before
    # a transmission factor of 0 makes no glass, so the flag marks nothing; appended materials are marked at the scene's offsets
    _load_ex(glass_glb(pane={"KHR_materials_transmission": {"transmissionFactor": 0.0}}), 4, s)
    assert [s.material_transmission_rough(m) for m in range(7)] == [False, False, True, True, False, False, True]
    # the frosted file's roughness is the material's, as §10 reads it
    f, _ = _load_ex(_golden("frosted-glass.glb"), 4)
    assert [float(r) for r in f.materials["roughness"][2:4]] == [0.5, float(F(0.3))]


# ---------------------------------------------------------------- 5. the side table: the rough bit in the sign of `thin`
def Fb(x):
    return int(np.float32(x).view(np.uint32))


TWO = ["scene 4", "trans 1 1 1.5 1", "trans 3 0.5 1.33 0"]
TABLE_CASES = {
    "no rough bit: the records of before": (TWO + ["inst 1 0 1", "inst 3 1 1", "tris 2"], ([[Fb(1), Fb(1.5), Fb(1), 0], [Fb(0.5), Fb(1.33), 0, 0]], [1, 0], [0, 0], 0)),
    "a rough pane: thin = -1": (TWO + ["rough 1 1", "inst 1 0 1", "inst 3 1 1", "tris 2"], ([[Fb(1), Fb(1.5), Fb(-1), 0], [Fb(0.5), Fb(1.33), 0, 0]], [1, 0], [1, 0], 0)),
    "a rough solid: thin = -0": (TWO + ["rough 3 1", "inst 1 0 1", "inst 3 1 1", "tris 2"], ([[Fb(1), Fb(1.5), Fb(1), 0], [Fb(0.5), Fb(1.33), Fb(-0.0), 0]], [1, 0], [0, 1], 0)),
    "a rough tinted solid keeps its sigma flag": (TWO + ["rough 3 1", "atten 3 0.5 0.5 0.5 1", "inst 3 0 2", "tris 2"], ([[Fb(0.5), Fb(1.33), Fb(-0.0), Fb(1)]], [0], [1], 0)),
    "set and cleared again": (TWO + ["rough 1 1", "rough 1 0", "inst 1 0 2", "tris 2"], ([[Fb(1), Fb(1.5), Fb(1), 0]], [1], [0], 0)),
    "the bit on an opaque material leaves no record": (TWO + ["rough 2 1", "inst 2 0 1", "inst 1 1 1", "tris 2"], ([[Fb(1), Fb(1.5), Fb(1), 0]], [1], [0], 0)),
    "the bit survives factor 0 and back": (TWO + ["rough 1 1", "trans 1 0 1.5 1", "trans 1 0.25 2 0", "inst 1 0 2", "tris 2"], ([[Fb(0.25), Fb(2), Fb(-0.0), 0]], [0], [1], 0)),
    "rejected calls change nothing": (TWO + ["rough 1 2", "rough 9 1", "inst 1 0 2", "tris 2"], ([[Fb(1), Fb(1.5), Fb(1), 0]], [1], [0], 2)),
}


@pytest.fixture(scope="module")
def table_results(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("roughtab") / "rough_tables_check")
    src = [os.path.join(ROOT, "tests", "tools", "rough_tables_check.cpp"), os.path.join(ROOT, "loupiote_amd", "csrc", "scene.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include")] + src + ["-o", exe])
    lines = [l for cmds, _ in TABLE_CASES.values() for l in cmds + ["derive"]]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:allocator_may_return_null=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0 and not p.stderr, (p.stdout[-2000:], p.stderr[-4000:])       # clean under the sanitizers
    out = [json.loads(l) for l in p.stdout.splitlines()]
    assert len(out) == len(TABLE_CASES)
    return dict(zip(TABLE_CASES, out))


@pytest.mark.parametrize("name", list(TABLE_CASES))
def test_rough_bit_in_the_transmission_table(table_results, name):
    recs, thin, rough, rejected = TABLE_CASES[name][1]
    got = table_results[name]
    assert got["status"] == 0 and got["recs"] == recs and got["thin"] == thin and got["rough"] == rough and got["rejected"] == rejected
    assert got["more"] == [] or len(got["more"]) == len(recs)
