"""-m gpu: rough transmission (SPEC.md §29) on the device.  The event the shading kernels run (lpt_interface_sample_rough) against the float32 restatement in
tests/rough_ref.py, bit for bit; bit-identity with clear glass where the roughness is 0 or the material is opaque; two furnace scenes against the float64
reference; bit-identity across the launch paths; and a glTF file's frosted glass end to end.

THE BOUNDS.  The hook is compared by bits.  The furnace means are compared within 6 combined standard errors — the device's from its own per-sample frames,
the reference's from its own draws, both computed here — plus, for the pane, the spread of the reference's expectation over the directions of the pixels that
are averaged.  Nothing is tuned on what the device returns."""
import json
import os
import struct

import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import testing as T

import rough_ref as RR
import transmission_ref as R
from test_gpu_env_sampling import _dark_light, const_probe
from test_gpu_transmission import (CUBE_C, CUBE_DIR, CUBE_EYE, CUBE_HALF, DIR, EYE, GLB_FLOOR, GLB_PANE, QUAD_IDX, VFOV, Rig, add_rect, cube_mesh, cube_rects, frame_of,
                                   glass_glb)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
W = H = 64
PANE_BASE = (0.8, 0.6, 0.4)
ONE_M = F(1.0 - 2.0 ** -24)


def _unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


# ---------------------------------------------------------------- 1. the hook against the float32 reference, bit for bit
def _hook_rows():
    """[n, 19] rows {d, Ns, Ngf, entering, base, ior, thin, roughness, r4, u1, u2}: 16384 random ones over every side, wall kind and roughness, then the edges"""
    rng = np.random.default_rng(29)
    n = 16384
    ngf = _unit(rng.normal(size=(n, 3)))
    d = _unit(rng.normal(size=(n, 3)))
    d = np.where(((d * ngf).sum(1) > 0)[:, None], -d, d)                       # Ngf is flipped against d
    ns = _unit(ngf + 0.4 * rng.normal(size=(n, 3)))
    ns = np.where(((ns * ngf).sum(1) < 0)[:, None], -ns, ns)                   # §12: Ns on Ngf's side (some still face away from V: N = Ngf)
    rough = rng.choice([0.0449, 0.045, 0.1, 0.3, 0.5, 0.8, 1.0, 1.7], n)
    rows = [np.column_stack([d, ns, ngf, rng.random(n) < 0.5, rng.random((n, 3)), rng.uniform(1.0, 2.5, n), rng.random(n) < 0.3, rough, rng.random(n), rng.random(n), rng.random(n)])]
    z = np.array([0.0, 0.0, 1.0])
    cc = float(np.sqrt(1 - 1 / 2.25))                                          # the cosine of the critical angle of ior 1.5
    edge = []
    for c in (1.0, 0.5, 1e-2, 1e-4, 1e-7, 0.0, cc - 1e-3, cc + 1e-3, cc - 0.2):  # head on ... grazing V ... V in the surface; about and past the critical angle
        for ns_e in (z, -z, _unit(np.array([-0.6, 0.0, 0.8])), _unit(np.array([0.8, 0.0, 0.6]))):      # -z and the tilted ones: dot(V, Ns) <= 0 at some c, so N = Ngf
            for entering, thin in ((True, False), (False, False), (True, True), (False, True)):
                for rough_e in (0.0449, 0.045, 0.5, 1.0):
                    for r4 in (0.0, 0.03, 0.5, float(ONE_M)):
                        for u1, u2 in ((0.0, 0.0), (0.37, float(ONE_M)), (0.25, 0.5), (float(ONE_M), 0.0), (0.625, 0.999), (0.5, float(ONE_M))):
                            dd = np.array([np.sqrt(max(0.0, 1 - c * c)), 0.0, -c])
                            edge.append(np.concatenate([dd, ns_e, z, [entering], PANE_BASE, [1.5, thin, rough_e, r4, u1, u2]]))
    rows.append(np.array(edge))
    return np.concatenate(rows).astype(F)


def test_the_hook_equals_the_reference_bit_for_bit(device):
    rows = _hook_rows()
    assert 20000 <= len(rows) <= 40000 and rows.shape[1] == 19
    wi, weight, kind = device.interface_sample_rough(rows)
    c = rows
    rwi, rweight, rkind = RR.interface_sample_rough(c[:, 0:3], c[:, 3:6], c[:, 6:9], c[:, 9] != 0, c[:, 10:13], c[:, 13], c[:, 14] != 0, c[:, 15], c[:, 16], c[:, 17], c[:, 18])
    assert np.all(np.isfinite(wi)) and np.all(np.isfinite(weight))
    counts = {k: int((rkind == k).sum()) for k in (0, 1, 2, 4, 5)}
    print("hook: %d rows, kinds" % len(rows), counts, "N = Ngf in %d" % int(((c[:, 0:3] * c[:, 3:6]).sum(1) >= 0).sum()))
    assert all(v > 100 for v in counts.values()), counts                        # reflected, transmitted, ended, and the smooth event's two
    assert np.array_equal(kind, rkind), (int((kind != rkind).sum()), np.flatnonzero(kind != rkind)[:8])
    bad = (wi.view(np.uint32) != rwi.view(np.uint32)).any(1) | (weight.view(np.uint32) != rweight.view(np.uint32)).any(1)
    assert not bad.any(), (int(bad.sum()), np.flatnonzero(bad)[:8], wi[bad][:4], rwi[bad][:4], weight[bad][:4], rweight[bad][:4])
    # below the threshold the hook is lpt_interface_sample itself
    s = (c[:, 15] < F(0.045))
    swi, sweight, skind = device.interface_sample(c[s, 0:3], c[s, 3:6], c[s, 6:9], c[s, 9] != 0, c[s, 10:13], c[s, 13], c[s, 14] != 0, c[s, 16])
    assert s.sum() > 2000 and wi[s].tobytes() == swi.tobytes() and weight[s].tobytes() == sweight.tobytes() and np.array_equal(kind[s], skind + 4)


# ---------------------------------------------------------------- the glass-pane.glb scene by hand, with the roughness and the bit as parameters
def hand_scene(pane_rough=0.1, cube_rough=0.1, floor_rough=0.6, bits=(False, False, False), light=None):
    """tests/golden/glass-pane.glb's scene built through the scene API (test_gpu_transmission.test_gltf_glass_end_to_end's): floor, thin pane, solid cube.
    bits: the rough bit of the three materials"""
    c = lp.Scene()
    mats = [c.add_material((0.8, 0.7, 0.6, 1.0), floor_rough, 0.1), c.add_material((0.5, 1.0, 0.25, 1.0), pane_rough, 0.0), c.add_material((1.0, 1.0, 1.0, 1.0), cube_rough, 0.0)]
    c.set_material_transmission(mats[1], 1.0, rough=bits[1])
    c.set_material_transmission(mats[2], 0.9, ior=1.33, thin_walled=False, rough=bits[2])
    if bits[0]:
        assert lp._abi.lib().lpt_scene_set_material_transmission_rough(c._h, mats[0], 1) == 0      # an opaque material with the bit
    up, front = np.tile(np.float32([[0, 1, 0]]), (4, 1)), np.tile(np.float32([[0, 0, 1]]), (4, 1))
    cp, cn, ci = cube_mesh(0.5)
    blas = [c.add_mesh(GLB_FLOOR.astype(np.float32), up, None, np.array([0, 2, 1, 0, 3, 2], np.uint32)), c.add_mesh(GLB_PANE.astype(np.float32), front, None, QUAD_IDX),
            c.add_mesh(cp, cn, None, ci)]

    def trs(t=(0, 0, 0), s=(1, 1, 1)):
        m = np.diag(list(s) + [1.0]).astype(np.float32)
        m[:3, 3] = t
        return m.T

    c.add_instance(blas[0], trs(s=(4, 1, 4)), mats[0])
    c.add_instance(blas[1], trs(t=(0, 0, 1)), mats[1])
    c.add_instance(blas[2], trs(t=(1.5, 0.5, -1.0)), mats[2])
    if light is not None:
        c.add_punctual_light(light)
    c.set_light(0, _dark_light())
    return c


GLB_VIEW = dict(depth=6, eye=(0.5, 1.2, 5.0), direction=(0.0, -0.15, -1.0), vfov=T.VFOV)


def test_the_bit_with_roughness_zero_and_on_an_opaque_material_changes_nothing(device):
    probe = const_probe(0.25)
    kw = dict(n=4, size=(W, H), **GLB_VIEW)
    clear = frame_of(device, hand_scene(0.0, 0.0), probe, **kw)
    assert np.all(np.isfinite(clear)) and clear[..., :3].any()
    assert frame_of(device, hand_scene(0.0, 0.0, bits=(False, True, True)), probe, **kw).tobytes() == clear.tobytes()
    # just below the threshold too, against the same roughness with the bit clear
    low = float(np.nextafter(F(0.045), F(0)))
    assert frame_of(device, hand_scene(low, low, bits=(False, True, True)), probe, **kw).tobytes() == frame_of(device, hand_scene(low, low), probe, **kw).tobytes()
    # the bit on a material that is not transmissive
    assert frame_of(device, hand_scene(0.0, 0.0, bits=(True, False, False)), probe, **kw).tobytes() == clear.tobytes()
    # ... and the bit is not idle: at the threshold the frame differs
    assert frame_of(device, hand_scene(0.045, 0.045, bits=(False, True, True)), probe, **kw).tobytes() != frame_of(device, hand_scene(0.045, 0.045), probe, **kw).tobytes()


# ---------------------------------------------------------------- 2. a thin rough pane before a constant probe
def rough_pane_scene(rough=0.5, tr=1.0, metal=0.0):
    """one 0.8 x 0.8 thin rough pane at z = -2 facing the camera at the origin (test_gpu_transmission.pane_scene's geometry)"""
    s = lp.Scene()
    s.set_light(0, _dark_light())
    m = s.add_material(PANE_BASE + (1.0,), rough, metal)
    s.set_material_transmission(m, tr, 1.5, True, rough=True)
    add_rect(s, (0, 0, -2), (1, 0, 0), (0, 1, 0), 0.4, 0.4, m)
    return s


def test_thin_rough_pane_before_a_constant_probe(device):
    SPP, REF = 64, 1 << 18
    centre = (slice(24, 40), slice(24, 40))
    rig = Rig(device, rough_pane_scene(), const_probe(0.5), depth=2)
    x = rig.samples(SPP).astype(np.float64)
    rig.close()
    E = x[0, 0, 0]                                   # beside the pane: the probe's radiance as the device decodes it
    assert (E > 0).all() and (x[:, 0, 0] == E).all() and E[0] == E[1] == E[2]
    block = x[(slice(None),) + centre]               # [spp, 16, 16, 3]
    got = block.mean((0, 1, 2))
    got_se = np.sqrt(block.var(0, ddof=1).sum((0, 1)) / SPP) / 256
    # the reference at the central direction, and at the block's corners and edge midpoints for the spread (common random numbers: the differences are smooth)
    view = T.look(EYE, DIR)
    o, dd = R.camera_rays(view, VFOV, W, H, np.array([0.0, 1.0]))
    n = np.array([0.0, 0.0, 1.0])
    want, want_se = RR.pane_expectation(np.array(DIR, np.float64), n, PANE_BASE, 1.5, 0.5, REF, seed=1)
    around = [dd[y, xx, k] for y, xx, k in ((24, 24, 0), (24, 39, 1), (39, 24, 2), (39, 39, 3), (24, 32, 0), (32, 24, 0), (39, 32, 2), (32, 39, 1))]
    spread = max(np.abs(RR.pane_expectation(a, n, PANE_BASE, 1.5, 0.5, REF, seed=1)[0] - want).max() for a in around)
    bound = 6 * np.sqrt(got_se ** 2 + (E * want_se) ** 2) + E * spread
    print("rough pane: mean / E", got / E, "expected", want, "device se / E", got_se / E, "reference se", want_se, "spread", spread, "|miss| / bound", np.abs(got - E * want) / bound)
    assert (np.abs(got - E * want) <= bound).all(), (got, E * want, bound)
    assert (want < np.array([1.0, 0.9, 0.8])).all() and (want > 0.3).all()      # a frosted, tinted pane: darker than a clear one, not black
    # every sample is a weight in [0, 1] times the probe, and the pane is frosted: the samples of one pixel take many values
    assert (block >= 0).all() and (block <= E * (1 + 1e-6)).all() and len(np.unique(block[:, 8, 8, 0])) > SPP // 2


# ---------------------------------------------------------------- 3. a closed rough solid cube in the same furnace
def rough_cube_scene(rough=0.5):
    s = lp.Scene()
    s.set_light(0, _dark_light())
    m = s.add_material((1.0, 1.0, 1.0, 1.0), rough, 0.0)
    s.set_material_transmission(m, 1.0, 1.5, False, rough=True)
    pos, nrm, idx = cube_mesh(CUBE_HALF)
    blas = s.add_mesh(pos, nrm, np.zeros((len(pos), 2), np.float32), idx)
    xf = np.eye(4, dtype=np.float32)
    xf[:3, 3] = CUBE_C
    s.add_instance(blas, xf.T, m)
    return s


def test_closed_rough_solid_cube_furnace(device):
    DEPTH, SPP, SIZE, REF = 12, 64, 32, 256
    pix = (slice(12, 20), slice(12, 20))             # test_gpu_transmission.CUBE_PIX at half the resolution
    ys, xs = np.meshgrid(np.arange(12, 20), np.arange(12, 20), indexing="ij")
    px = np.stack([ys.ravel(), xs.ravel()], 1)
    rects = cube_rects(CUBE_C, CUBE_HALF, kind="solid", ior=1.5)
    view = T.look(CUBE_EYE, CUBE_DIR)
    o, dd = R.camera_rays(view, VFOV, SIZE, SIZE, np.array([0.0, 1.0]))
    corner = dd[pix].reshape(-1, 3)
    assert (R._nearest(rects, np.broadcast_to(o, corner.shape), corner, np.full(len(corner), -1))[1] >= 0).all()      # the pixels lie on the cube
    o, d = RR.jittered_rays(view, VFOV, SIZE, SIZE, px, REF, seed=3)
    L = RR.scene_monte_carlo(rects, 1.0, o, d, DEPTH, 0.5, seed=4).reshape(len(px), REF)
    want, want_se = L.mean(), np.sqrt(L.var(1, ddof=1).sum() / REF) / len(px)
    assert (L >= 0).all() and (L <= 1 + 1e-12).all()
    rig = Rig(device, rough_cube_scene(), const_probe(0.5), size=(SIZE, SIZE), depth=DEPTH, eye=CUBE_EYE, direction=CUBE_DIR)
    x = rig.samples(SPP).astype(np.float64)
    rig.close()
    assert np.all(np.isfinite(x))
    E = x[0, 0, 0, 0]
    assert E > 0 and (x[:, 0, 0] == E).all()
    block = x[(slice(None),) + pix][..., 0]          # [spp, 8, 8]
    got, got_se = block.mean(), np.sqrt(block.var(0, ddof=1).sum() / SPP) / len(px)
    margin = 6 * np.sqrt(got_se ** 2 + (E * want_se) ** 2)
    print("rough cube: mean / E %.4f, reference %.4f, device se / E %.4f, reference se %.4f, |miss| / margin %.2f" % (got / E, want, got_se / E, want_se, abs(got - E * want) / margin))
    assert abs(got - E * want) <= margin, (got, E * want, margin)
    assert got <= E + margin and (block <= E * (1 + 1e-5)).all()       # white frosted glass in a furnace: nothing is gained
    assert 0.3 < want < 1.0                                          # ... and single scattering loses some of it


# ---------------------------------------------------------------- 4. launch independence
def test_launch_independence(device):
    """the 64 x 64 frosted frame over the launch paths of test_gpu_transmission.test_launch_independence"""
    scene, probe = rough_pane_scene(tr=0.7, metal=0.2), const_probe(0.5)
    size = (W, H)
    kw = dict(size=size, depth=4, n=4)
    want = frame_of(device, scene, probe, **kw)
    assert np.all(np.isfinite(want))
    clear = rough_pane_scene(tr=0.7, metal=0.2)
    clear.set_material_transmission(1, 0.7, 1.5, True)
    assert frame_of(device, clear, probe, **kw).tobytes() != want.tobytes()      # the frame is a frosted one
    for v in (dict(options={"coop_rays": 0}), dict(options={"path_rays": 0}), dict(options={"packet_primary": 0}), dict(options={"packet_primary": 1})):
        assert frame_of(device, scene, probe, **kw, **v).tobytes() == want.tobytes(), v
    acc = np.zeros_like(want)
    for rank in range(2):
        acc += frame_of(device, scene, probe, rank=rank, world=2, **kw)
    assert acc.tobytes() == want.tobytes()
    # the denoised mode and its sharded twin
    sg = lp.SceneGPU.new_from_scene(scene, device)
    mode = lp.BlitMode.DenoisedPathrace
    one = Rig(device, scene, probe, size=size, depth=4, mode=mode, sg=sg)
    ranks = [Rig(device, scene, probe, size=size, depth=4, mode=mode, sg=sg, rank=q, world=2) for q in range(2)]
    for f in range(2):
        view = T.look((0.02 * f, 0.01 * f, 0.0), DIR)
        one.r.raytrace(view)
        for r in ranks:
            r.r.raytrace(view)
        ranks[0].r.exchange_local([r.r for r in ranks[1:]])
        got, ref = ranks[0].r.read_radiance(), one.r.read_radiance()
        assert np.all(np.isfinite(ref)) and got.tobytes() == ref.tobytes(), "frame %d" % f
    for r in [one] + ranks:
        r.close()
    sg.close()


# ---------------------------------------------------------------- 5. glTF end to end
FROSTED_PANE_ROUGH, FROSTED_CUBE_ROUGH = 0.5, 0.3


def frosted_glb():
    """tests/golden/frosted-glass.glb: test_gpu_transmission.glass_glb's file — a floor, one thin pane, one solid cube, one directional light — with the pane's
    roughnessFactor 0.5 and the cube's 0.3; the binary chunk is taken over as it is, the JSON chunk written anew"""
    src = glass_glb()
    jlen = struct.unpack_from("<I", src, 12)[0]
    js = json.loads(src[20:20 + jlen])
    js["materials"][1]["pbrMetallicRoughness"]["roughnessFactor"] = FROSTED_PANE_ROUGH
    js["materials"][2]["pbrMetallicRoughness"]["roughnessFactor"] = FROSTED_CUBE_ROUGH
    j = json.dumps(js).encode()
    j += b" " * (-len(j) % 4)
    b = src[20 + jlen:]
    return struct.pack("<III", 0x46546C67, 2, 12 + 8 + len(j) + len(b)) + struct.pack("<II", len(j), 0x4E4F534A) + j + b


def test_gltf_frosted_glass_end_to_end(device):
    with open(os.path.join(HERE, "golden", "frosted-glass.glb"), "rb") as f:
        data = f.read()
    assert data == frosted_glb() and len(data) < 8192          # the committed copy is this writer's output
    frosted, clear = lp.Scene(), lp.Scene()
    lp.loaders.load_gltf(data, frosted, rough_transmission=True)
    lp.loaders.load_gltf(data, clear)
    assert [frosted.material_transmission_rough(m) for m in range(4)] == [False, False, True, True]
    assert not any(clear.material_transmission_rough(m) for m in range(4))
    light = frosted.punctual_lights[:1].copy()                # the loader's record (its fp32 rotation leaves 1e-8 in the axis)
    probe = const_probe(0.25)
    kw = dict(n=4, size=(96, 64), **GLB_VIEW)
    frames = {}
    for name, s in (("frosted", frosted), ("clear", clear), ("hand frosted", hand_scene(FROSTED_PANE_ROUGH, FROSTED_CUBE_ROUGH, bits=(False, True, True), light=light)),
                    ("hand clear", hand_scene(FROSTED_PANE_ROUGH, FROSTED_CUBE_ROUGH, light=light))):
        s.set_light(0, _dark_light())
        frames[name] = frame_of(device, s, probe, **kw)
        assert np.all(np.isfinite(frames[name])) and frames[name][..., :3].any()
    assert frames["frosted"].tobytes() == frames["hand frosted"].tobytes()
    assert frames["clear"].tobytes() == frames["hand clear"].tobytes()          # without the flag: the clear render of before, the bit clear
    assert frames["frosted"].tobytes() != frames["clear"].tobytes()
