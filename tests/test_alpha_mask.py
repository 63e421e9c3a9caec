"""CPU: alpha-masked materials (SPEC.md §20) on the host — what the glTF loader reads (alphaMode, alphaCutoff, which image carries alpha), the scene API's
side table, and tests/alpha_ref.py against values worked out by hand."""
import io

import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import _abi as A

import alpha_ref as R
from test_gpu_alpha_mask import PATTERN, alpha_glb, mask_texture, png_bytes

INVALID = A.INVALID_INDEX


def _load(glb):
    s = lp.Scene()
    lp.loaders.load_gltf(glb, s)
    return s


def _snapshot(s):
    c = s.counts()
    return (tuple(getattr(c, f) for f, _ in c._fields_), s.materials.tobytes(), s.instances.tobytes(), s.vertices.tobytes(), s.indices.tobytes(), s.punctual_lights.tobytes(),
            tuple(s.material_alpha(m) for m in range(c.materials)))


# ---------------------------------------------------------------- loader
def test_mask_sets_the_side_table_and_the_alpha_image():
    s = _load(alpha_glb())
    assert s.counts().materials == 3 and s.counts().images == 1
    assert s.material_alpha(0) == (A.ALPHA_OPAQUE, 0.5, INVALID)      # the dummy
    assert s.material_alpha(1) == (A.ALPHA_OPAQUE, 0.5, INVALID)      # the floor: no alphaMode
    assert s.material_alpha(2) == (A.ALPHA_MASK, 0.5, 0)
    assert s.materials["albedo_texture"][2] == 0 and np.array_equal(s.image(0), mask_texture())
    assert _load(alpha_glb(cutoff=0.25)).material_alpha(2) == (A.ALPHA_MASK, 0.25, 0)
    assert _load(alpha_glb(cutoff=None)).material_alpha(2) == (A.ALPHA_MASK, 0.5, 0)      # glTF's default
    assert _load(alpha_glb(cutoff=0)).material_alpha(2) == (A.ALPHA_MASK, 0.0, 0)


def test_mask_appends_with_the_scene_offsets():
    s = _load(alpha_glb())
    lp.loaders.load_gltf(alpha_glb(cutoff=0.75), s)
    assert s.counts().materials == 5 and s.counts().images == 2
    assert s.material_alpha(2) == (A.ALPHA_MASK, 0.5, 0) and s.material_alpha(4) == (A.ALPHA_MASK, 0.75, 1) and s.material_alpha(3)[0] == A.ALPHA_OPAQUE


@pytest.mark.parametrize("mode", ["OPAQUE", "BLEND", None])
def test_opaque_blend_and_absent_load_as_opaque(mode):
    """BLEND is SPEC §14 (7): loaded as opaque.  None of the three leaves a trace: the scene is the one of a file that says nothing about alpha"""
    s = _load(alpha_glb(mode=mode, cutoff=None))
    assert all(s.material_alpha(m) == (A.ALPHA_OPAQUE, 0.5, INVALID) for m in range(3))
    assert _snapshot(s) == _snapshot(_load(alpha_glb(mode=None, cutoff=None)))
    assert _snapshot(_load(alpha_glb(mode=mode, cutoff=0.3))) == _snapshot(s)           # a cutoff without MASK means nothing


def test_an_image_without_an_alpha_channel_is_no_alpha_image():
    """SPEC §14 (5) expands RGB with alpha 0, which must not cut everything away: the mask then tests color.w alone"""
    rgb = mask_texture()[..., :3]
    s = _load(alpha_glb(image=png_bytes(rgb)))
    assert s.material_alpha(2) == (A.ALPHA_MASK, 0.5, INVALID) and s.materials["albedo_texture"][2] == 0 and not s.image(0)[..., 3].any()
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb)).save(buf, format="JPEG", quality=90)
    s = _load(alpha_glb(image=buf.getvalue(), mime="image/jpeg"))
    assert s.material_alpha(2) == (A.ALPHA_MASK, 0.5, INVALID) and s.materials["albedo_texture"][2] == 0


@pytest.mark.parametrize("kw", [{"mode": "mask"}, {"mode": "CUTOUT"}, {"mode": 1}, {"cutoff": -0.1}, {"cutoff": "0.5"}, {"cutoff": 1e999}, {"mode": "OPAQUE", "cutoff": -1}])
def test_bad_alpha_fields_reject_the_file_and_leave_the_scene(kw):
    s = _load(alpha_glb())
    before = _snapshot(s)
    with pytest.raises(lp.Error) as e:
        lp.loaders.load_gltf(alpha_glb(**kw), s)
    assert e.value.kind == "FileNotFound"
    assert _snapshot(s) == before


def test_cornell_box_loads_as_before(cornell_glb):
    s = _load(cornell_glb)
    c = s.counts()
    assert (c.entries, c.instances, c.materials, c.images) == (6, 6, 4, 0) and c.indices == 34 * 3 and c.vertices == 103
    assert all(s.material_alpha(m) == (A.ALPHA_OPAQUE, 0.5, INVALID) for m in range(c.materials))
    from oracle import gltf_oracle as G
    o = G.Scene()
    G.load_gltf(cornell_glb, o)
    for name in ("materials", "instances", "vertices", "indices", "entries"):
        assert getattr(s, name).tobytes() == np.ascontiguousarray(getattr(o, name)).tobytes(), name


# ---------------------------------------------------------------- scene API
def test_set_get_round_trip_and_defaults():
    s = lp.Scene()
    assert s.material_alpha(0) == (A.ALPHA_OPAQUE, 0.5, INVALID)
    img = s.add_image(mask_texture())
    m = s.add_material((1, 1, 1, 0.75), 1.0, 0.0)
    assert s.material_alpha(m) == (A.ALPHA_OPAQUE, 0.5, INVALID)
    before = s.materials.tobytes()
    s.set_material_alpha(m, A.ALPHA_MASK, 0.125, img)
    assert s.material_alpha(m) == (A.ALPHA_MASK, 0.125, img) and s.material_alpha(0) == (A.ALPHA_OPAQUE, 0.5, INVALID)
    s.set_material_alpha(m, "MASK", 2.0)
    assert s.material_alpha(m) == (A.ALPHA_MASK, 2.0, INVALID)
    m2 = s.add_material((1, 1, 1, 1), 1.0, 0.0)                     # a material added after the table was first written
    assert s.material_alpha(m2) == (A.ALPHA_OPAQUE, 0.5, INVALID)
    s.set_material_alpha(m, "OPAQUE")
    assert s.material_alpha(m) == (A.ALPHA_OPAQUE, 0.5, INVALID)
    assert s.materials[:2].tobytes() == before and A.MATERIAL_DT.itemsize == 32       # a side table: lpt_material keeps its layout and its bytes


@pytest.mark.parametrize("args", [(9, 1, 0.5, INVALID), (1, 2, 0.5, INVALID), (1, 1, -0.5, INVALID), (1, 1, float("nan"), INVALID), (1, 1, float("inf"), INVALID),
                                  (1, 1, 0.5, 1), (1, 1, 0.5, 0xFFFFFFFE)])
def test_invalid_arguments_leave_the_scene_untouched(args):
    s = lp.Scene()
    img = s.add_image(mask_texture())
    m = s.add_material((1, 1, 1, 1), 1.0, 0.0)
    s.set_material_alpha(m, A.ALPHA_MASK, 0.25, img)
    with pytest.raises(lp.Error) as e:
        s.set_material_alpha(*args)
    assert e.value.kind == "InvalidArg"
    assert s.material_alpha(m) == (A.ALPHA_MASK, 0.25, img) and s.material_alpha(0) == (A.ALPHA_OPAQUE, 0.5, INVALID)
    with pytest.raises(lp.Error) as e:
        s.material_alpha(2)
    assert e.value.kind == "InvalidArg"


# ---------------------------------------------------------------- alpha_ref against hand-computed values
def test_alpha_ref_texel_centres_and_midpoints():
    img = mask_texture()
    f = np.float32
    # a texel centre is the texel: u = (x + 0.5) / 16 gives fx = x, weight 0
    for by in range(4):
        for bx in range(4):
            u, v = f((4 * bx + 1 + 0.5) / 16), f((4 * by + 2 + 0.5) / 16)
            assert R.tex_alpha(img, u, v) == f(PATTERN[by, bx])
    # the midpoint between two texels of different blocks: (255 * (1 / 255)) * 0.5 + 0 * 0.5
    assert R.tex_alpha(img, f(4 / 16), f(1.5 / 16)) == f(0.5)          # row 0: blocks 0 | 1 = 1 | 0
    assert R.tex_alpha(img, f(8 / 16), f(1.5 / 16)) == f(0.5)          # row 0: blocks 1 | 2 = 0 | 1
    assert R.tex_alpha(img, f(8 / 16), f(5.5 / 16)) == f(1.0)          # row 1: blocks 1 | 2 = 1 | 1
    assert R.tex_alpha(img, f(4 / 16), f(4 / 16)) == f(0.5)            # the corner of blocks (0,0) (0,1) (1,0) (1,1) = 1 0 0 1: 0.5 * 0.5 + 0.5 * 0.5
    assert R.tex_alpha(img, f(8.25 / 16), f(1.5 / 16)) == f(0.75)      # a quarter of a texel past the centre of texel 7 (alpha 0) towards texel 8 (alpha 1): fx = 7.75
    # repeat: one texel centre beyond either end is the other end's texel
    assert R.tex_alpha(img, f(1.0 + 0.5 / 16), f(1.5 / 16)) == f(PATTERN[0, 0]) and R.tex_alpha(img, f(-0.5 / 16), f(1.5 / 16)) == f(PATTERN[0, 3])
    assert R.tex_alpha(img, f(1.5 / 16), f(-0.5 / 16)) == f(PATTERN[3, 0]) and R.tex_alpha(img, f(2.0 + 5.5 / 16), f(1.0 + 9.5 / 16)) == f(PATTERN[2, 1])


def test_alpha_ref_interpolation_and_decision():
    f = np.float32
    uv = np.array([[0, 0], [2, 0], [2, 2]], f)
    tu, tv = R.interp_uv(uv, f(0.25), f(0.5))                           # bw = 0.25: (0 * 0.25 + 2 * 0.25) + 2 * 0.5, (0 + 0) + 2 * 0.5
    assert (tu, tv) == (f(1.5), f(1.0))
    img = mask_texture()
    # uv (1.5, 1.0) wraps to (0.5, 0.0): fx = 7.5 between texels 7 | 8, fy = -0.5 between rows 15 | 0 -> blocks (3,1) (3,2) (0,1) (0,2) = 0 1 0 1
    assert R.alpha(1.0, img, uv, f(0.25), f(0.5)) == f(0.5)
    assert R.alpha(0.5, img, uv, f(0.25), f(0.5)) == f(0.25)
    assert R.alpha(0.3, None, uv, f(0.25), f(0.5)) == f(0.3)
    assert R.counts(f(0.5), 0.5) and not R.counts(np.nextafter(f(0.5), f(0)), 0.5) and R.counts(f(0.0), 0.0) and not R.counts(f(1.0), 2.0)
    a = R.alpha(1.0, img, uv, np.array([0.25, 0.1], f), np.array([0.5, 0.1], f))   # vectorised over hits
    assert a.shape == (2,) and a[0] == f(0.5)
