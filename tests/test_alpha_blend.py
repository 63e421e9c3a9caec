"""CPU: alpha-blended materials (SPEC.md §26) on the host — tests/blend_ref.py against values worked out by hand and as a fair coin, the scene API's
third alpha state, and what the glTF loader reads when it is asked to read BLEND."""
import io

import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import _abi as A

import blend_ref as B
from test_gpu_alpha_mask import alpha_glb, mask_texture, png_bytes

INVALID = A.INVALID_INDEX
F = np.float32


# ---------------------------------------------------------------- blend_ref against hand-computed values
def test_pcg_known_answers():
    """SPEC §4 by hand.  v = 0: s = 2891336453 = 0xAC564B05, s >> 28 = 10, so the shift is 14: s >> 14 = 176473 = 0x2B159;
    (0x2B159 ^ 0xAC564B05) = 0xAC54FA5C = 2891250268; x 277803737 mod 2^32 = 129708028 = 0x7BB2FFC; w >> 22 = 30; 0x7BB2FFC ^ 30 = 0x7BB2FE2 = 129708002"""
    s = 2891336453
    assert s >> 28 == 10 and s >> 14 == 176473 and (176473 ^ s) == 2891250268
    w = (2891250268 * 277803737) % 2 ** 32
    assert w >> 22 == 30 and (w ^ 30) == 129708002
    assert [int(x) for x in B.pcg([0, 1, 37, 0xFFFFFFFF, 0x3F000000])] == [129708002, 2831084092, 356461763, 3861530882, 1034895725]
    assert B.pcg(np.uint32(1)).dtype == np.uint32 and int(B.pcg(1)) == 2831084092


def test_xi_known_answers():
    """h = pcg(pcg(pcg(prim) ^ bits(u)) ^ bits(v)), xi = (h >> 8) / 2^24; the chain written out for each row: pcg(prim), the second hash, h"""
    rows = [   # prim, u, v, pcg(prim), pcg(. ^ bits(u)), h, h >> 8
        (0, 0.0, 0.0, 129708002, 817759070, 2145236065, 8379828),
        (0, -0.0, 0.0, 129708002, 1459943766, 173512251, 677782),          # bits(-0) = 0x80000000: the sign of a zero is part of the hit
        (0, 0.0, -0.0, 129708002, 817759070, 1482632797, 5791534),
        (1, 0.25, 0.5, 2831084092, 914338319, 4281245581, 16723615),       # bits 0x3E800000, 0x3F000000
        (37, 1.0, 0.0, 356461763, 3745129541, 4075674323, 15920602),
        (37, 0.3, 0.3, 356461763, 730263198, 3639169, 14215),              # bits(0.3f) = 0x3E99999A
        (0xFFFFFFFE, 0.5, 0.5, 2155513543, 2147146490, 3382009175, 13210973),
    ]
    assert int(B.bits(F(0.3))) == 0x3E99999A and int(B.bits(F(-0.0))) == 0x80000000 and int(B.bits(F(0.25))) == 0x3E800000
    for prim, u, v, h1, h2, h, top in rows:
        assert int(B.pcg(prim)) == h1 and int(B.pcg(h1 ^ int(B.bits(F(u))))) == h2 and int(B.pcg(h2 ^ int(B.bits(F(v))))) == h and h >> 8 == top
        x = B.xi(prim, u, v)
        assert x.dtype == F and float(x) == top / 2.0 ** 24 and 0.0 <= float(x) < 1.0
    got = B.xi([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])       # vectorised
    assert np.array_equal(got, np.array([r[6] / 2.0 ** 24 for r in rows], F))


def test_the_decision_at_its_ends():
    prim, u, v = np.arange(4096), np.linspace(0, 1, 4096, dtype=F), np.linspace(1, 0, 4096, dtype=F)
    assert B.counts(F(1.0), prim, u, v).all() and B.counts(F(1.5), prim, u, v).all()          # a >= 1 always counts: xi < 1
    assert not B.counts(F(0.0), prim, u, v).any() and not B.counts(F(-0.5), prim, u, v).any() and not B.counts(F(-0.0), prim, u, v).any()
    assert not B.counts(F(np.nan), prim, u, v).any()
    x = B.xi(prim, u, v)
    assert np.array_equal(B.counts(x, prim, u, v), np.zeros(4096, bool))                       # a == xi does not count (strictly greater)
    assert B.counts(np.nextafter(x, F(2.0)), prim, u, v).all()
    uv = np.array([[0, 0], [2, 0], [2, 2]], F)
    assert B.alpha(0.3, None, uv, F(0.25), F(0.5)) == F(0.3) and B.alpha(1.0, mask_texture(), uv, F(0.25), F(0.5)) == F(0.5)   # a is §20's


# ---------------------------------------------------------------- the reference alone is a fair coin
N = 1 << 20
PRIMS = (0, 1, 37)
ALPHAS = (0.1, 0.3, 0.5, 0.9)


def _uv_sets():
    rng = np.random.default_rng(26)
    u, v = rng.random(N, F), rng.random(N, F)
    g = (np.arange(1024, dtype=F) / F(1024.0))
    gu, gv = np.meshgrid(g, g)
    return {"uniform": (u, v), "grid": (gu.reshape(-1).copy(), gv.reshape(-1).copy()), "v=0": ((np.arange(N, dtype=F) / F(N)), np.zeros(N, F)),
            "scaled": (u * F(1e-6), v * F(1e-6))}


@pytest.fixture(scope="module")
def xi_sets():
    return {name: [B.xi(p, u, v) for p in PRIMS] for name, (u, v) in _uv_sets().items()}


def test_the_reference_is_a_fair_coin(xi_sets):
    """2^20 (u, v) pairs of four kinds x prims 0, 1, 37 x four alphas: the share with xi < a within 5 binomial standard deviations of a (48 statistics)"""
    worst = 0.0
    for name, xs in xi_sets.items():
        for p, x in zip(PRIMS, xs):
            assert x.shape == (N,) and x.min() >= 0.0 and x.max() < 1.0
            for a in ALPHAS:
                z = abs((x < F(a)).mean() - a) / np.sqrt(a * (1 - a) / N)
                worst = max(worst, z)
                assert z <= 5.0, (name, p, a, z)
    print("fair coin: largest deviation %.2f sigma over %d statistics" % (worst, len(xi_sets) * len(PRIMS) * len(ALPHAS)))


def test_prims_draw_independently(xi_sets):
    """the correlation of xi between two prims at equal (u, v) within 5 / sqrt(n): a stack of cards composites, it does not line up"""
    for name, xs in xi_sets.items():
        for i in range(len(PRIMS)):
            for j in range(i + 1, len(PRIMS)):
                r = np.corrcoef(xs[i].astype(np.float64), xs[j].astype(np.float64))[0, 1]
                assert abs(r) <= 5.0 / np.sqrt(N), (name, PRIMS[i], PRIMS[j], r)


# ---------------------------------------------------------------- scene API
def test_blend_round_trips_and_changes_back():
    s = lp.Scene()
    img = s.add_image(mask_texture())
    m = s.add_material((1, 1, 1, 0.75), 1.0, 0.0)
    before = s.materials.tobytes()
    assert A.ALPHA_BLEND == 2 and A.ALPHA_BLEND not in (A.ALPHA_OPAQUE, A.ALPHA_MASK)
    s.set_material_alpha(m, "BLEND", alpha_image=img)
    assert s.material_alpha(m) == (A.ALPHA_BLEND, 0.5, img) and s.material_alpha(0) == (A.ALPHA_OPAQUE, 0.5, INVALID)
    s.set_material_alpha(m, "BLEND")
    assert s.material_alpha(m) == (A.ALPHA_BLEND, 0.5, INVALID)
    s.set_material_alpha(m, "MASK", 0.125, img)
    assert s.material_alpha(m) == (A.ALPHA_MASK, 0.125, img)
    s.set_material_alpha(m, "BLEND", cutoff=0.9, alpha_image=img)          # BLEND has no cutoff: the stored one returns to 0.5
    assert s.material_alpha(m) == (A.ALPHA_BLEND, 0.5, img)
    s.set_material_alpha(m, "OPAQUE")
    assert s.material_alpha(m) == (A.ALPHA_OPAQUE, 0.5, INVALID)
    s.set_material_alpha(m, "BLEND", alpha_image=img)
    s.set_material_alpha(m, A.ALPHA_MASK, 0.25, img)
    assert s.material_alpha(m) == (A.ALPHA_MASK, 0.25, img)
    assert s.materials.tobytes() == before and A.MATERIAL_DT.itemsize == 32       # a side table: lpt_material keeps its layout and its bytes


def test_the_integer_mode_still_reaches_the_old_setter():
    s = lp.Scene()
    m = s.add_material((1, 1, 1, 1), 1.0, 0.0)
    with pytest.raises(lp.Error) as e:
        s.set_material_alpha(m, A.ALPHA_BLEND)
    assert e.value.kind == "InvalidArg" and s.material_alpha(m) == (A.ALPHA_OPAQUE, 0.5, INVALID)


@pytest.mark.parametrize("material, image", [(9, INVALID), (2, INVALID), (1, 1), (1, 0xFFFFFFFE)])
def test_bad_indices_are_refused_and_leave_the_scene(material, image):
    s = lp.Scene()
    img = s.add_image(mask_texture())
    m = s.add_material((1, 1, 1, 1), 1.0, 0.0)
    s.set_material_alpha(m, A.ALPHA_MASK, 0.25, img)
    with pytest.raises(lp.Error) as e:
        s.set_material_alpha(material, "BLEND", alpha_image=image)
    assert e.value.kind == "InvalidArg"
    assert s.material_alpha(m) == (A.ALPHA_MASK, 0.25, img) and s.material_alpha(0) == (A.ALPHA_OPAQUE, 0.5, INVALID)
    assert A.lib().lpt_scene_set_material_alpha_blend(None, 0, INVALID) == A.LPT_ERR_INVALID_ARG


# ---------------------------------------------------------------- loader
def _load(glb, **kw):
    s = lp.Scene()
    lp.loaders.load_gltf(glb, s, **kw)
    return s


def _snapshot(s):
    c = s.counts()
    return (tuple(getattr(c, f) for f, _ in c._fields_), s.materials.tobytes(), s.instances.tobytes(), s.vertices.tobytes(), s.indices.tobytes(), s.punctual_lights.tobytes(),
            tuple(s.material_alpha(m) for m in range(c.materials)))


def test_blend_sets_the_side_table_and_the_alpha_image():
    s = _load(alpha_glb(mode="BLEND"), blend=True)
    assert s.counts().materials == 3 and s.counts().images == 1
    assert s.material_alpha(0) == (A.ALPHA_OPAQUE, 0.5, INVALID) and s.material_alpha(1) == (A.ALPHA_OPAQUE, 0.5, INVALID)
    assert s.material_alpha(2) == (A.ALPHA_BLEND, 0.5, 0)
    assert s.materials["albedo_texture"][2] == 0 and np.array_equal(s.image(0), mask_texture())
    for cutoff in (0.25, None, 0):          # alphaCutoff is validated and ignored
        assert _load(alpha_glb(mode="BLEND", cutoff=cutoff), blend=True).material_alpha(2) == (A.ALPHA_BLEND, 0.5, 0)
    # everything but the side table is the plain load's
    assert _snapshot(s)[:-1] == _snapshot(_load(alpha_glb(mode="BLEND")))[:-1]
    assert _load(alpha_glb(mode="BLEND")).material_alpha(2) == (A.ALPHA_OPAQUE, 0.5, INVALID)       # by default BLEND loads as opaque


def test_blend_through_a_path(tmp_path):
    p = tmp_path / "blend.glb"
    p.write_bytes(alpha_glb(mode="BLEND"))
    s, t = lp.Scene(), lp.Scene()
    lp.loaders.load_gltf_path(p, s, blend=True)
    lp.loaders.load_gltf_path(p, t)
    assert s.material_alpha(2) == (A.ALPHA_BLEND, 0.5, 0) and t.material_alpha(2) == (A.ALPHA_OPAQUE, 0.5, INVALID)
    assert _snapshot(s) == _snapshot(_load(alpha_glb(mode="BLEND"), blend=True))


def test_an_image_without_an_alpha_channel_is_no_alpha_image():
    rgb = mask_texture()[..., :3]
    s = _load(alpha_glb(mode="BLEND", image=png_bytes(rgb)), blend=True)
    assert s.material_alpha(2) == (A.ALPHA_BLEND, 0.5, INVALID) and s.materials["albedo_texture"][2] == 0 and not s.image(0)[..., 3].any()
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb)).save(buf, format="JPEG", quality=90)
    s = _load(alpha_glb(mode="BLEND", image=buf.getvalue(), mime="image/jpeg"), blend=True)
    assert s.material_alpha(2) == (A.ALPHA_BLEND, 0.5, INVALID) and s.materials["albedo_texture"][2] == 0


@pytest.mark.parametrize("kw", [{"mode": "MASK"}, {"mode": "MASK", "cutoff": 0.25}, {"mode": "OPAQUE"}, {"mode": "OPAQUE", "cutoff": 0.3}, {"mode": None, "cutoff": None},
                                {"mode": None, "cutoff": 0.3}])
def test_the_flag_changes_nothing_for_a_file_without_blend(kw):
    assert _snapshot(_load(alpha_glb(**kw), blend=True)) == _snapshot(_load(alpha_glb(**kw)))


def test_flags_zero_is_the_plain_loader():
    for kw in ({"mode": "BLEND"}, {"mode": "MASK"}, {}):
        glb = np.frombuffer(alpha_glb(**kw), np.uint8)
        s = lp.Scene()
        assert A.lib().lpt_load_gltf_ex(s._h, A.ptr(glb), glb.size, 0) == A.LPT_OK
        assert _snapshot(s) == _snapshot(_load(alpha_glb(**kw)))


def test_blend_appends_with_the_scene_offsets():
    s = _load(alpha_glb(mode="BLEND"), blend=True)
    lp.loaders.load_gltf(alpha_glb(cutoff=0.75), s, blend=True)
    lp.loaders.load_gltf(alpha_glb(mode="BLEND"), s, blend=True)
    assert s.counts().materials == 7 and s.counts().images == 3
    assert s.material_alpha(2) == (A.ALPHA_BLEND, 0.5, 0) and s.material_alpha(4) == (A.ALPHA_MASK, 0.75, 1) and s.material_alpha(6) == (A.ALPHA_BLEND, 0.5, 2)
    assert s.material_alpha(3)[0] == A.ALPHA_OPAQUE and s.material_alpha(5)[0] == A.ALPHA_OPAQUE


@pytest.mark.parametrize("kw", [{"mode": "blend"}, {"mode": "CUTOUT"}, {"mode": 2}, {"mode": "BLEND", "cutoff": -0.1}, {"mode": "BLEND", "cutoff": "0.5"},
                                {"mode": "BLEND", "cutoff": 1e999}, {"mode": "OPAQUE", "cutoff": -1}])
def test_bad_alpha_fields_still_reject_the_file_and_leave_the_scene(kw):
    s = _load(alpha_glb(mode="BLEND"), blend=True)
    before = _snapshot(s)
    with pytest.raises(lp.Error) as e:
        lp.loaders.load_gltf(alpha_glb(**kw), s, blend=True)
    assert e.value.kind == "FileNotFound"
    assert _snapshot(s) == before


@pytest.mark.parametrize("flags", [2, 3, 0x80000000, 0xFFFFFFFF])
def test_an_unknown_flag_bit_is_an_invalid_argument(flags, tmp_path):
    s = _load(alpha_glb(mode="BLEND"), blend=True)
    before = _snapshot(s)
    glb = np.frombuffer(alpha_glb(mode="BLEND"), np.uint8)
    assert A.lib().lpt_load_gltf_ex(s._h, A.ptr(glb), glb.size, flags) == A.LPT_ERR_INVALID_ARG
    p = tmp_path / "blend.glb"
    p.write_bytes(glb.tobytes())
    assert A.lib().lpt_load_gltf_path_ex(s._h, str(p).encode(), flags) == A.LPT_ERR_INVALID_ARG
    assert _snapshot(s) == before
