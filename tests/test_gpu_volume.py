"""-m gpu: volume attenuation (SPEC.md §28) on the device.  The factor the shading kernels apply (lpt_scene_gpu_attenuation) against the float32 restatement in
tests/volume_ref.py, bit for bit; a cube of index 1 whose every sample must be the probe's radiance times exp(-sigma chord) of that sample's own ray; the tinted
furnace against the float64 expectation of the reference; bit-identity where the rule must not apply and across the forms of the frame pipeline; the tables through
the scene's update paths; and a glTF file's tinted glass end to end.

THE BOUNDS.  The hook is compared by bits.  A straight-through sample is compared with exp(-sigma chord) within the rounding model of volume_ref.atten and the
length the device's segment can differ from the binary64 chord by (stated at the test).  Means are compared with the reference's expectation within 5 standard
errors taken from the reference's own per-sample variance — derived, not tuned."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import scenes, testing as T

import volume_ref as V
from test_gpu_env_sampling import _dark_light, const_probe
from test_gpu_transmission import (CUBE_C, CUBE_DIR, CUBE_EYE, CUBE_HALF, CUBE_PIX, H, VFOV, W, Rig, _atrium_with_sealed_glass, _is, add_rect, cube_mesh, cube_rects,
                                   cube_scene, frame_of)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
TINT, TINT_D = (0.2, 0.8, 0.4), 0.5
U = 2.0 ** -24


def tinted_cube_scene(ior=1.5, color=TINT, distance=TINT_D, thin=False):
    """test_gpu_transmission.cube_scene with the volume attenuation set (material 1); color None: never set"""
    s = cube_scene()
    s.set_material_transmission(1, 1.0, ior, thin)
    if color is not None:
        s.set_material_attenuation(1, color, distance)
    return s


# ---------------------------------------------------------------- 1. the hook against the float32 reference, bit for bit
HOOK_QUADS = [((0, 0, -2), (1, 0, 0), (0, 1, 0)), ((2, 0, -2), (0, 1, 0), (1, 0, 0)), ((4, 0, -2), (0, 1, 0), (0, 0, 1)), ((6, 0, -2), (0, 0, 1), (1, 0, 0)),
              ((8, 0, -2), (1, 0, 0), (0, 0, 1))]      # (centre, u, v): normals +z, -z, +x, +y, -y
HOOK_KINDS = ["opaque", "thin", "clear", "tinted", "black-red"]


def _hook_scene():
    s = lp.Scene()
    s.set_light(0, _dark_light())
    mats = []
    for kind in HOOK_KINDS:
        m = s.add_material((1.0, 1.0, 1.0, 1.0), 0.3, 0.0)
        if kind != "opaque":
            s.set_material_transmission(m, 1.0, 1.5, kind == "thin")
        if kind in ("thin", "tinted"):
            s.set_material_attenuation(m, TINT, TINT_D)        # on the thin pane it is stored and does not act
        if kind == "black-red":
            s.set_material_attenuation(m, (0.0, 1.0, 0.5), 0.5)
        mats.append(m)
    for (c, u, v), m in zip(HOOK_QUADS, mats):
        add_rect(s, c, u, v, 0.4, 0.4, m)
    deg = s.add_mesh(np.array([[0, 5, 0], [1, 5, 0], [2, 5, 0]], F), np.tile(F([[0, 0, 1]]), (3, 1)), np.zeros((3, 2), F), np.array([0, 1, 2], np.uint32))
    s.add_instance(deg, np.eye(4, dtype=F), mats[3])                # a degenerate triangle of the attenuating material: prim 10
    return s, mats


def _either_side_of_125(sig):
    """the two adjacent float32 t with fl(fl(sig t) L) < 125 <= the next one's"""
    y = lambda t: (F(sig) * F(t)) * V.LOG2E
    t = F(125.0 / (float(V.LOG2E) * float(sig)))
    while y(t) >= F(125.0):
        t = np.nextafter(t, F(0))
    while y(np.nextafter(t, F(np.inf))) < F(125.0):
        t = np.nextafter(t, F(np.inf))
    return [t, np.nextafter(t, F(np.inf))]


def test_hook_equals_the_reference_bit_for_bit(device):
    s, mats = _hook_scene()
    sg = lp.SceneGPU.new_from_scene(s, device)
    prims, dirs, ts, want, applies = [], [], [], [], []
    c60, s60 = np.cos(np.pi / 3), np.sin(np.pi / 3)
    for q, ((_, u, v), m, kind) in enumerate(zip(HOOK_QUADS, mats, HOOK_KINDS)):
        u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
        n = np.cross(u, v)
        sig = s.material_attenuation(m)[2]
        acts = kind in ("tinted", "black-red")
        tt = [F(0), F(1e-30), F(1e-3), F(0.5), F(1), F(10), F(3e38)]
        for sc in sig[sig > 0] if acts else V.sigma(TINT, TINT_D):
            tt += _either_side_of_125(sc)
        for d in (n, -n, c60 * n + s60 * u, -c60 * n + s60 * v, u, -v, (u + v) / np.sqrt(2)):       # along, against, at 60 degrees either way, three in the plane
            d32 = d.astype(F)
            behind = float(d32.astype(np.float64) @ n) > 0      # entering is !(dot > 0): a direction in the plane (dot = 0) counts as entering
            for tri in range(2):
                for t in tt:
                    prims.append(2 * q + tri); dirs.append(d32); ts.append(t)
                    ok = acts and behind
                    applies.append(ok)
                    want.append(V.atten(sig, t) if ok else np.ones(3, F))
    for t in (F(0), F(0.5), F(3e38)):                               # the degenerate triangle: no surface hit
        prims.append(10); dirs.append(F([0, 0, 1])); ts.append(t); applies.append(False); want.append(np.ones(3, F))
    prims, dirs, ts, want, applies = np.array(prims, np.uint32), np.array(dirs, F), np.array(ts, F), np.array(want, F), np.array(applies)
    try:
        got = sg.attenuation(prims, dirs, ts)
        with pytest.raises(lp.Error) as e:
            sg.attenuation(np.array([11], np.uint32), F([[0, 0, 1]]), F([1.0]))      # beyond the baked triangles
        assert e.value.kind == "InvalidArg"
    finally:
        sg.close()
    print("hook: %d elements, %d apply; distinct factors %d" % (len(prims), applies.sum(), len(np.unique(want[applies].view(np.uint32)))))
    assert applies.sum() > 80 and (~applies).sum() > 400
    assert np.array_equal(got["applies"], applies), np.flatnonzero(got["applies"] != applies)[:8]
    bad = (got["A"].view(np.uint32) != want.view(np.uint32)).any(1)
    assert not bad.any(), (int(bad.sum()), prims[bad][:4], ts[bad][:4], got["A"][bad][:4], want[bad][:4])
    assert (got["A"][~applies] == 1).all()
    # the edges are among the factors: exactly 1 (t = 0, sigma = 0), exactly 0 (y >= 125, FLT_MAX x 1e-30), and the smallest values below the threshold are normal numbers
    a = want[applies]
    assert (a == 1).any() and (a == 0).any() and (a[a > 0] >= np.finfo(F).tiny).all() and (a[a > 0].min() < 1e-37)


# ---------------------------------------------------------------- 2. straight through a cube of index 1
STRAIGHT_PIX = (slice(24, 40), slice(16, 40))


def test_straight_through_a_cube_of_index_one(device):
    """At ior = 1 the Fresnel term is a rounding residue (asserted below from the reference, in float32: at most 1e-14 at cos >= 0.3), so every sample of a block pixel
    enters by one face, crosses the cube and leaves: its radiance is L exp(-sigma_c chord) per channel, chord being the binary64 slab-method chord of that sample's own
    ray.  The device's segment runs from the entry point moved eps = 1e-4 (1 + max |P|) along the face normal (§12) to the exit face, so its length differs from the
    chord by at most eps / cos(theta) at the entry, as much again for where the exit point lands, and the traversal's own error of a hit distance on either end:
    Delta = 2 eps / cos(theta) + 4 delta_t, delta_t the largest |t_device - t_float64| SceneGPU.trace_closest shows on these same rays (code this change does not
    touch; measured here and printed: 1.2e-07 on the MI355X when this was written, half an ulp of a distance of 3).  The tolerance is exp(+-sigma_c Delta) (1 +- (3 sigma_c chord + 8) 2^-24), the second
    factor volume_ref's rounding model."""
    S, DEPTH = 8, 4
    sig = V.sigma(TINT, TINT_D).astype(np.float64)
    lo, hi = np.asarray(CUBE_C, np.float64) - CUBE_HALF, np.asarray(CUBE_C, np.float64) + CUBE_HALF
    rig = Rig(device, tinted_cube_scene(ior=1.0), const_probe(0.5), depth=DEPTH, eye=CUBE_EYE, direction=CUBE_DIR)
    clear = Rig(device, tinted_cube_scene(ior=1.0, color=None), const_probe(0.5), depth=DEPTH, eye=CUBE_EYE, direction=CUBE_DIR)
    rig.r.accumulate = clear.r.accumulate = False
    worst = delta_t = 0.0
    n_checked = 0
    try:
        for f in range(S):
            o, d = rig.r.primary_rays(rig.view, 0)                # the rays of the frame the next raytrace() renders
            rig.r.raytrace(rig.view)
            x = rig.r.read_radiance()[..., :3].copy()
            clear.r.raytrace(clear.view)
            y = clear.r.read_radiance()[..., :3].copy()
            L = x[0, 0]
            assert (L > 0).all() and _is(y[0, 0], L)
            assert _is(y[STRAIGHT_PIX], L).all()                  # without the attenuation: the probe's radiance, bit for bit, in every block sample
            ob, db = o[STRAIGHT_PIX].reshape(-1, 3), d[STRAIGHT_PIX].reshape(-1, 3)
            o64, d64 = ob.astype(np.float64), db.astype(np.float64)
            with np.errstate(divide="ignore"):
                t0, t1 = (lo - o64) / d64, (hi - o64) / d64
            tn, tf = np.minimum(t0, t1), np.maximum(t0, t1)
            t_in, t_out = tn.max(1), tf.min(1)
            assert (t_in < t_out).all()                           # every ray of the block meets the cube
            cos_in = np.take_along_axis(np.abs(d64), tn.argmax(1)[:, None], 1)[:, 0]
            cos_out = np.take_along_axis(np.abs(d64), tf.argmin(1)[:, None], 1)[:, 0]
            cos = np.minimum(cos_in, cos_out)
            assert (cos >= 0.3).all(), cos.min()
            for c in (cos_in, cos_out):                           # the reference's own Fresnel term at these angles, in float32
                assert V.fresnel(c.astype(F), np.ones(len(c), F))[0].max() <= 1e-14
            hit = rig.sg.trace_closest(ob, db)
            assert (hit["prim"] < 12).all()
            delta_t = max(delta_t, float(np.abs(hit["t"].astype(np.float64) - t_in).max()))
            chord = t_out - t_in
            P = o64 + d64 * t_out[:, None]
            eps = 1e-4 * (1.0 + np.maximum(np.abs(P).max(1), np.abs(o64 + d64 * t_in[:, None]).max(1)))
            Delta = 2.0 * eps / cos + 4.0 * delta_t
            got = x[STRAIGHT_PIX].reshape(-1, 3).astype(np.float64)
            for c in range(3):
                b = (3.0 * sig[c] * chord + 8.0) * U
                low = L[c] * np.exp(-sig[c] * (chord + Delta)) * (1.0 - b)
                high = L[c] * np.exp(-sig[c] * (chord - Delta)) * (1.0 + b)
                inside = (got[:, c] >= low) & (got[:, c] <= high)
                assert inside.all(), (f, c, int((~inside).sum()), got[~inside][:3, c], low[~inside][:3], high[~inside][:3])       # no sample is left out
                mid = L[c] * np.exp(-sig[c] * chord)
                worst = max(worst, float((np.abs(got[:, c] - mid) / (high - low) * 2).max()))
            n_checked += len(chord)
    finally:
        rig.close()
        clear.close()
    print("straight: %d samples, delta_t %.3g, chords %.3f..%.3f, largest |got - L exp(-sigma chord)| / half width %.3f" % (n_checked, delta_t, chord.min(), chord.max(), worst))
    assert n_checked == S * 16 * 24 and delta_t < 1e-4


# ---------------------------------------------------------------- 3. the tinted furnace
def test_tinted_furnace(device):
    """test_closed_solid_cube_furnace's scene and pixel block with sigma from (0.2, 0.8, 0.4) / 0.5: the mean over block and samples against the reference's
    expectation (jitter integrated on a 2 x 2 sub-pixel grid), per channel, within 5 standard errors of the reference's own per-sample variance"""
    S, DEPTH, GRID = 16, 12, 2
    ys, xs = np.meshgrid(np.arange(24, 40), np.arange(24, 40), indexing="ij")
    px = np.stack([ys.ravel(), xs.ravel()], 1)
    sig = V.sigma(TINT, TINT_D).astype(np.float64)
    rects = cube_rects(CUBE_C, CUBE_HALF, kind="solid", ior=1.5, sigma=sig)
    view = T.look(CUBE_EYE, CUBE_DIR)
    mean, var, pz = V.expectation(rects, (1, 1, 1), view, VFOV, W, H, DEPTH, GRID, px)
    clear_mean, _, _ = V.expectation(cube_rects(CUBE_C, CUBE_HALF, kind="solid", ior=1.5), (1, 1, 1), view, VFOV, W, H, DEPTH, GRID, px)
    assert np.allclose(clear_mean, (1 - pz)[:, None], atol=1e-12) and (mean < clear_mean).all()       # the reference without sigma is the furnace of §21
    rig = Rig(device, tinted_cube_scene(), const_probe(0.5), depth=DEPTH, eye=CUBE_EYE, direction=CUBE_DIR)
    x = rig.samples(S)
    rig.close()
    assert np.all(np.isfinite(x))
    L = x[0, 0, 0]
    assert (L > 0).all() and _is(x[:, 0, 0], L).all()
    inner = x[(slice(None),) + CUBE_PIX].astype(np.float64)
    zero = (inner == 0).all(-1)
    want_z, sigma_z = S * pz.sum(), np.sqrt(S * (pz * (1 - pz)).sum())
    assert abs(int(zero.sum()) - want_z) <= 5 * sigma_z + 1e-9, (int(zero.sum()), want_z, sigma_z)       # the truncated paths, as in the furnace
    assert ((inner > 0).all(-1) | zero).all() and (inner <= L).all()
    got = inner.reshape(-1, 3).mean(0) / L.astype(np.float64)
    want = mean.mean(0)
    se = np.sqrt(var.sum(0) / S) / len(px)
    print("tinted furnace: mean %s, expected %s, standard error %s, |diff| / se %s; truncated %d (expected %.2g)" % (got, want, se, np.abs(got - want) / se, zero.sum(), want_z))
    assert np.all(np.abs(got - want) <= 5 * se), (got, want, se)
    assert got[0] < got[2] < got[1] and sig[0] > sig[2] > sig[1]      # red, blue, green: as sigma orders them


# ---------------------------------------------------------------- 4. unchanged where it must be
@pytest.mark.parametrize("variant", ["thin-walled", "distance-inf", "white"])
def test_a_material_that_does_not_attenuate_renders_as_before(device, variant):
    kw = dict(n=4, depth=6, eye=CUBE_EYE, direction=CUBE_DIR)
    thin = variant == "thin-walled"
    edited = tinted_cube_scene(thin=thin, color=(1.0, 1.0, 1.0) if variant == "white" else TINT, distance=float("inf") if variant == "distance-inf" else TINT_D)
    want = frame_of(device, tinted_cube_scene(thin=thin, color=None), const_probe(0.5), **kw)
    got = frame_of(device, edited, const_probe(0.5), **kw)
    assert np.all(np.isfinite(want)) and want[..., :3].any()
    assert got.tobytes() == want.tobytes()
    assert frame_of(device, tinted_cube_scene(thin=False), const_probe(0.5), **kw).tobytes() != want.tobytes()      # ... and the solid attenuating cube is another frame


def test_opaque_hits_beside_an_attenuating_material_are_unchanged(device):
    """the small atrium plus a sealed opaque box that holds a triangle of solid glass: no ray reaches it, so the frame of the TRANS kernels is the same with and
    without the attenuation — whose record and sigma row are on the device (the hook reads them)"""
    desc = scenes.synthetic_atrium(texture_size=128)
    kw = dict(size=(96, 64), depth=4, eye=desc["camera"]["origin"], direction=desc["camera"]["direction"], vfov=T.VFOV)
    frames = []
    for tinted in (False, True):
        s = _atrium_with_sealed_glass(desc, 1.0)
        glass = s.counts().materials - 1
        s.set_material_transmission(glass, 1.0, 1.5, False)
        if tinted:
            s.set_material_attenuation(glass, TINT, TINT_D)
        sg = lp.SceneGPU.new_from_scene(s, device)
        last = sg.stats().triangles - 1                          # the glass triangle is the last instance (geometric normal -y)
        a = sg.attenuation(np.array([last], np.uint32), F([[0, -1, 0]]), F([0.5]))
        assert bool(a["applies"][0]) is tinted and np.array_equal(a["A"][0], V.atten(V.sigma(TINT, TINT_D), F(0.5)) if tinted else np.ones(3, F))
        frames.append(frame_of(device, s, desc.get("probe"), n=2, sg=sg, **kw))
        frames.append(frame_of(device, s, desc.get("probe"), n=2, sg=sg, mode=lp.BlitMode.DenoisedPathrace, **kw))      # the GBUF forms
        sg.close()
    assert np.all(np.isfinite(frames[0])) and frames[0][..., :3].any()
    assert frames[0].tobytes() == frames[2].tobytes() and frames[1].tobytes() == frames[3].tobytes()


# ---------------------------------------------------------------- 5. one frame however it is launched
def test_launch_independence(device):
    scene, probe = tinted_cube_scene(), const_probe(0.5)
    kw = dict(size=(64, 64), depth=6, n=4, eye=CUBE_EYE, direction=CUBE_DIR)
    want = frame_of(device, scene, probe, **kw)
    assert np.all(np.isfinite(want))
    assert want.tobytes() != frame_of(device, tinted_cube_scene(color=None), probe, **kw).tobytes()
    for v in (dict(options={"coop_rays": 0}), dict(options={"path_rays": 0}), dict(options={"packet_primary": 0}), dict(options={"packet_primary": 1}),
              dict(options={"wavefront_rays": 64 * 64 // 2})):       # the last: the frame as two pieces
        assert frame_of(device, scene, probe, **kw, **v).tobytes() == want.tobytes(), v
    acc = np.zeros_like(want)
    for rank in range(2):
        acc += frame_of(device, scene, probe, rank=rank, world=2, **kw)
    assert acc.tobytes() == want.tobytes()
    # the denoised mode and its sharded twin
    sg = lp.SceneGPU.new_from_scene(scene, device)
    mode = lp.BlitMode.DenoisedPathrace
    rk = dict(size=(64, 64), depth=6, mode=mode, sg=sg, eye=CUBE_EYE, direction=CUBE_DIR)
    one = Rig(device, scene, probe, **rk)
    ranks = [Rig(device, scene, probe, rank=q, world=2, **rk) for q in range(2)]
    for f in range(2):
        view = T.look((CUBE_EYE[0] + 0.02 * f, CUBE_EYE[1] + 0.01 * f, CUBE_EYE[2]), CUBE_DIR)
        one.r.raytrace(view)
        for r in ranks:
            r.r.raytrace(view)
        ranks[0].r.exchange_local([r.r for r in ranks[1:]])
        got, ref = ranks[0].r.read_radiance(), one.r.read_radiance()
        assert np.all(np.isfinite(ref)) and got.tobytes() == ref.tobytes(), "frame %d" % f
    for r in [one] + ranks:
        r.close()
    sg.close()


# ---------------------------------------------------------------- 6. the tables follow the scene through an instance update and both arms of a rebuild
@pytest.mark.parametrize("big", [False, True], ids=["fewer-than-16-triangles", "16-triangles"])
def test_sigma_rows_follow_update_and_rebuild(device, big):
    def moved(dx):
        m = np.eye(4, dtype=F)
        m[0, 3] = dx
        return m.T

    s = lp.Scene()
    s.set_light(0, _dark_light())
    first = s.add_material((1.0, 1.0, 1.0, 1.0), 0.3, 0.0)
    s.set_material_transmission(first, 1.0, 1.5, False)
    add_rect(s, (2, 0, -2), (1, 0, 0), (0, 1, 0), 0.4, 0.4, first)                     # a clear solid first: the edited material's record is the second
    mat = s.add_material((1.0, 1.0, 1.0, 1.0), 0.3, 0.0)
    pane = add_rect(s, (0, 0, -2), (1, 0, 0), (0, 1, 0), 0.4, 0.4, mat)               # prims 2, 3; normal +z
    if big:
        pos, nrm, idx = cube_mesh(0.3)
        xf = np.eye(4, dtype=F)
        xf[:3, 3] = (-0.5, 0.1, -3.5)
        s.add_instance(s.add_mesh(pos, nrm, np.zeros((len(pos), 2), F), idx), xf.T, s.add_material((0.2, 0.8, 0.2, 1.0), 0.8, 0.0))
    sg = lp.SceneGPU.new_from_scene(s, device)
    assert (sg.stats().triangles >= 16) == big
    prim, d, t = np.array([2, 3, 0], np.uint32), F([[0, 0, 1]] * 3), F([0.25, 0.75, 0.25])

    def check(color, distance):
        got, fresh_sg = sg.attenuation(prim, d, t), lp.SceneGPU.new_from_scene(s, device)
        fresh = fresh_sg.attenuation(prim, d, t)
        fresh_sg.close()
        assert np.array_equal(got["A"].view(np.uint32), fresh["A"].view(np.uint32)) and np.array_equal(got["applies"], fresh["applies"])
        want = np.ones((3, 3), F)
        if color is not None:
            want[:2] = V.atten(V.sigma(color, distance)[None, :], t[:2, None])
        assert np.array_equal(got["A"].view(np.uint32), want.view(np.uint32)) and np.array_equal(got["applies"], [color is not None] * 2 + [False])

    try:
        check(None, None)                                               # opaque
        s.set_material_transmission(mat, 1.0, 1.5, False)               # opaque -> tinted solid glass, by an instance update
        s.set_material_attenuation(mat, TINT, TINT_D)
        s.set_instance_transform(pane, moved(0.05))
        assert sg.update_instances(s) == 1
        check(TINT, TINT_D)
        s.set_material_attenuation(mat, (0.9, 0.1, 0.5), 2.0)           # no instance changed: the rebuild alone carries the new row
        sg.rebuild(s)
        check((0.9, 0.1, 0.5), 2.0)
        s.set_material_attenuation(mat, (1.0, 1.0, 1.0))                # the attenuation removed, by an instance update: no row is left on the device
        s.set_instance_transform(pane, moved(0.0))
        assert sg.update_instances(s) == 1
        check(None, None)
        s.set_material_attenuation(mat, TINT, TINT_D)                   # ... and back, then the material opaque: the state is kept and does not act
        s.set_material_transmission(mat, 0.0)
        sg.rebuild(s)
        check(None, None)
        assert np.array_equal(s.material_attenuation(mat)[0], F(TINT))
    finally:
        sg.close()


# ---------------------------------------------------------------- 7. glTF end to end
GLB_FLOOR = np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], "<f4")
GLB_CUBE_AT = (1.5, 0.5, -1.0)
_DEFAULT = object()


def tinted_glb(volume=_DEFAULT):
    """a small .glb: a 8x8 floor, one solid cube (transmission 1, a volume of thickness 0.5 with attenuationColor (0.2, 0.8, 0.4) and attenuationDistance 0.5) and
    one directional light.  `volume`: another KHR_materials_volume object for the cube's material"""
    blob = bytearray()
    views, accessors = [], []

    def add(arr, ctype, atype):
        raw = np.ascontiguousarray(arr).tobytes()
        views.append({"buffer": 0, "byteOffset": len(blob), "byteLength": len(raw)})
        blob.extend(raw)
        blob.extend(b"\0" * (-len(blob) % 4))
        accessors.append({"bufferView": len(views) - 1, "componentType": ctype, "count": len(arr), "type": atype})
        return len(accessors) - 1

    up = np.tile(np.array([[0, 1, 0]], "<f4"), (4, 1))
    qi = add(np.array([0, 2, 1, 0, 3, 2], "<u2"), 5123, "SCALAR")
    cp, cn, ci = cube_mesh(0.5)
    meshes = [{"primitives": [{"attributes": {"POSITION": add(GLB_FLOOR, 5126, "VEC3"), "NORMAL": add(up, 5126, "VEC3")}, "indices": qi, "material": 0}]},
              {"primitives": [{"attributes": {"POSITION": add(cp.astype("<f4"), 5126, "VEC3"), "NORMAL": add(cn.astype("<f4"), 5126, "VEC3")},
                               "indices": add(ci.astype("<u2"), 5123, "SCALAR"), "material": 1}]}]
    if volume is _DEFAULT:
        volume = {"thicknessFactor": 0.5, "attenuationColor": list(TINT), "attenuationDistance": TINT_D}
    mats = [{"pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.7, 0.6, 1.0], "roughnessFactor": 0.6, "metallicFactor": 0.1}},
            {"pbrMetallicRoughness": {"baseColorFactor": [1.0, 1.0, 1.0, 1.0], "roughnessFactor": 0.1, "metallicFactor": 0.0},
             "extensions": {"KHR_materials_transmission": {"transmissionFactor": 1.0}, "KHR_materials_volume": volume}}]
    q = [float(np.sin(-np.pi / 4)), 0.0, 0.0, float(np.cos(-np.pi / 4))]     # -90 degrees about X: the light's -Z axis points straight down
    js = {"asset": {"version": "2.0"}, "meshes": meshes, "accessors": accessors, "bufferViews": views, "materials": mats,
          "nodes": [{"mesh": 0, "scale": [4.0, 1.0, 4.0]}, {"mesh": 1, "translation": list(GLB_CUBE_AT)}, {"rotation": q, "extensions": {"KHR_lights_punctual": {"light": 0}}}],
          "extensionsUsed": ["KHR_lights_punctual", "KHR_materials_transmission", "KHR_materials_volume"],
          "extensions": {"KHR_lights_punctual": {"lights": [{"type": "directional", "color": [1.0, 0.95, 0.9], "intensity": 3.0}]}},
          "buffers": [{"byteLength": len(blob)}]}
    j = json.dumps(js).encode()
    j += b" " * (-len(j) % 4)
    b = bytes(blob)
    return struct.pack("<III", 0x46546C67, 2, 12 + 8 + len(j) + 8 + len(b)) + struct.pack("<II", len(j), 0x4E4F534A) + j + struct.pack("<II", len(b), 0x004E4942) + b


GLB_EYE, GLB_BLOCK = (1.5, 0.15, 3.0), (slice(28, 36), slice(28, 36))
GLB_DIR = tuple(np.subtract(GLB_CUBE_AT, GLB_EYE))


def test_gltf_tinted_glass_end_to_end(device):
    """The golden file and the same file stripped of its attenuation, seen from below the cube's centre so that what is seen through the cube is the probe.  With the
    floor taken as black the reference gives E_t and E_c, the expectations of the paths that end in the probe, tinted and clear.  The frames add the paths by way of
    the floor, F_t and F_c, to them.  Both files draw the same random numbers and the attenuation only scales a path by factors <= 1, so 0 <= F_t <= F_c per channel,
    and F_c = D_c - E_c is read off the clear frame D_c.  Hence for the tinted block D_t: green >= E_t[g], red <= E_t[r] + F_c[r], and so
    D_t[g] / D_t[r] >= (E_t[g] - 5 se) / (E_t[r] + max(0, D_c[r] - E_c[r]) + 10 se): the reference's margin, the standard errors its own."""
    path = os.path.join(HERE, "golden", "tinted-glass.glb")
    with open(path, "rb") as f:
        assert f.read() == tinted_glb()                      # the committed copy is this writer's output
    S, DEPTH = 32, 6
    kw = dict(depth=DEPTH, eye=GLB_EYE, direction=GLB_DIR)
    frames = []
    for glb in (tinted_glb(), tinted_glb(volume={"thicknessFactor": 0.5})):
        s = lp.Scene()
        lp.loaders.load_gltf(glb, s)
        s.set_light(0, _dark_light())
        frames.append(frame_of(device, s, const_probe(0.25), n=S, **kw)[..., :3].astype(np.float64))
    tinted, clear = frames
    assert np.all(np.isfinite(tinted)) and tinted.any()
    L = clear[0, 0]
    assert L[0] > 0 and L[0] == L[1] == L[2] and np.array_equal(tinted[0, 0], L)          # the corner sees the probe
    assert (tinted <= clear).all()                                                         # the same paths, scaled by factors <= 1
    ys, xs = np.meshgrid(np.arange(GLB_BLOCK[0].start, GLB_BLOCK[0].stop), np.arange(GLB_BLOCK[1].start, GLB_BLOCK[1].stop), indexing="ij")
    px = np.stack([ys.ravel(), xs.ravel()], 1)
    view = T.look(GLB_EYE, GLB_DIR)
    floor = V.rect((0, 0, 0), (0, 0, 1), (1, 0, 0), 4.0, 4.0, kind="black")
    sig = V.sigma(TINT, TINT_D).astype(np.float64)
    o, dd = V.camera_rays(view, VFOV, W, H, np.array([0.0, 1.0]))
    corner = dd[GLB_BLOCK].reshape(-1, 3)
    cube = cube_rects(GLB_CUBE_AT, 0.5, kind="solid", ior=1.5, sigma=sig)
    assert (V._nearest(cube, np.broadcast_to(o, corner.shape), corner, np.full(len(corner), -1))[1] == 0).all()      # the block lies on the cube's +z face
    Et, vt, _ = V.expectation(cube + [floor], L, view, VFOV, W, H, DEPTH, 2, px)
    Ec, vc, _ = V.expectation(cube_rects(GLB_CUBE_AT, 0.5, kind="solid", ior=1.5) + [floor], L, view, VFOV, W, H, DEPTH, 2, px)
    Et, Ec = Et.mean(0), Ec.mean(0)
    se_t, se_c = np.sqrt(vt.sum(0) / S) / len(px), np.sqrt(vc.sum(0) / S) / len(px)
    Dt, Dc = tinted[GLB_BLOCK].reshape(-1, 3).mean(0), clear[GLB_BLOCK].reshape(-1, 3).mean(0)
    margin = (Et[1] - 5 * se_t[1]) / (Et[0] + max(0.0, Dc[0] - Ec[0]) + 5 * se_t[0] + 5 * se_c[0])
    print("gltf: tinted block %s, clear block %s; reference E_t %s, E_c %s; green / red %.3f, the reference's margin %.3f" % (Dt, Dc, Et, Ec, Dt[1] / Dt[0], margin))
    assert margin > Dc[1] / Dc[0]                            # the bound says something: it lies above the stripped file's own green / red
    assert Dt[1] / Dt[0] >= margin, (Dt, margin)


def test_bench_renders_the_tinted_file():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "1", "--frames-per-step", "2", "--width", "256", "--height", "256", "--no-extras",
                        "--camera", "1.5,0.15,3,0,0.35,-4", "--gltf", os.path.join(HERE, "golden", "tinted-glass.glb")], capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    j = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert j["data"] == "real" and "tinted-glass.glb" in j["config"]["workload"] and j["config"]["frame_complete"] is True and j["value"] > 0
