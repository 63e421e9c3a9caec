"""-m gpu: punctual lights (SPEC.md §19) on the device.  The function the shading kernels run (lpt_scene_gpu_sample_punctual) against the float64
restatement in tests/punctual_ref.py; rendered frames against closed forms — a delta light has no Monte-Carlo error beyond the pixel jitter and
the pick of the light —; shadows, cones and ranges that are EXACTLY black where they must be; the pick probabilities beside rectangle lights
and the probe; bit-identity across every form of the frame pipeline; and a glTF file's lights end to end.

THE BOUNDS (not tuned on any output; every float32 operation is taken as one relative rounding of 2^-24, first order, worst case = the sum):
  punctual_sample (kernels.h), point / spot: w = pos - Po (1), d2 = dot(w, w) (2 more per component squared and summed: 5, the subtraction's error
  enters twice: 2), dist = sqrt (1), 1 / dist (1), wi = w * inv (1), att = 1 / d2 (1), q = d2 / (r * r) (2), 1 - q * q (2; the q^2 doubles q's error: 2 x 9),
  g = (att * wr) * (s * s) (3), E = col * g (1).  Away from the clamp corners that is fewer than 48 roundings for E, 12 for wi and dist:
  REL_E = 48 * 2^-24, REL_W = 12 * 2^-24.  Two terms are not relative.  The range window 1 - q^2 loses relative accuracy where it nears 0: its
  error is absolute, 20 * 2^-24 of the unwindowed value.  The cone window subtracts two cosines: c = dot(-wi, dir) carries 12 + 5 roundings of a
  number <= 1, so s = (c - cos_outer) * inv_span is off by at most 20 * inv_span * 2^-24 ABSOLUTE, and s^2 by twice that (s <= 1).  A point whose
  float64 s or range window lies within those distances of 0 or 1 may clamp differently in float32 and is left out of test 1 (under 1 % of the points,
  asserted on the CPU from the reference alone before the GPU is asked).  Cancellation in pos - Po costs nothing here: the kernel and the reference read
  the SAME float32 position and points, so the subtraction is one rounding of its own result however close the point is to the light.
  A rendered pixel adds the shading chain on top: the primary hit and P (about 16 roundings and 3e-7 (|o| + t) of §7), Po (3), bsdf_eval (about 40:
  SPEC §10 has that many operations for one channel), NoL (5), the contribution (5) and the accumulation of up to 64 samples (64): REL_PIXEL =
  REL_E + 144 * 2^-24 = 192 * 2^-24 = 1.1e-5.

WHAT A PIXEL IS COMPARED WITH.  Every scene made through the API holds the dummy rectangle light 0 (Scene::default), so with one punctual light the
punctual share of the light samples is p_p = 1/2, not 1: besides the jitter, WHICH samples of a pixel picked the punctual light is random — and known,
because the pick is r0 of SPEC §4, a pure function of pixel and seed that tests/punctual_ref.py restates.  A pixel of which k_l of the spp samples picked
light l is therefore bounded by sum_l k_l / (spp p_pick_l) x [min, max] of light l's closed form over the pixel (a sub-pixel grid that includes the
pixel's border), widened by REL_PIXEL and the absolute terms above; the image mean is tested in the project's form against the full expectation."""
import json
import struct

import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import scenes, testing as T

import punctual_ref as R
from test_gpu_env_sampling import ALBEDO, DIR, EYE, PATH, PER_BOUNCE, VFOV, _bsdf_quadrature, _dark_light, _mean_sigma, const_probe, quad_scene, render, sun_probe

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
REL_W, REL_E, ABS_WINDOW, REL_PIXEL = 12 * U, 48 * U, 20 * U, 192 * U
N_UP = np.array([0.0, 1.0, 0.0])


# ---------------------------------------------------------------- 1. the unit kernel against float64
def _unit_points(rng, light, n):
    """points around the light at distances from 1e-3 to 1e3 (log-uniform), every direction: behind a spot, beyond a range and inside both included"""
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dist = 10.0 ** rng.uniform(-3, 3, n)
    dist[:8] = (1e-3, 1e3, 1e-3, 1e3, 0.5, 2.0, 7.9, 8.1)
    return (light["position"][None] + d * dist[:, None]).astype(np.float32)


@pytest.mark.parametrize("kind", ["point", "point_range", "spot", "spot_range", "directional"])
def test_sample_punctual_matches_float64(device, kind):
    rng = np.random.default_rng(5)
    rec = {"point": lp.point_light((0.5, -1.0, 2.0), color=(1.0, 0.5, 0.25), intensity=40.0),
           "point_range": lp.point_light((0.5, -1.0, 2.0), intensity=3.0, range=8.0),
           "spot": lp.spot_light((1.0, 2.0, -0.5), (0.3, -1.0, 0.2), intensity=10.0, inner_angle=0.3, outer_angle=0.8),
           "spot_range": lp.spot_light((1.0, 2.0, -0.5), (0.3, -1.0, 0.2), color=(0.2, 1.0, 0.6), intensity=10.0, range=8.0, inner_angle=0.1, outer_angle=0.4),
           "directional": lp.directional_light((0.3, -1.0, 0.2), color=(0.9, 0.8, 0.7), intensity=2.5)}[kind]
    light = R.from_record(rec)           # the float32 record as stored, widened: the reference and the kernel read the same numbers
    pts = _unit_points(rng, light, 4096)
    ok, wi, dist, E = R.incident(light, pts.astype(np.float64))
    # which points sit within the float32 bound of a clamp corner — from the reference alone, before the GPU is asked
    near = np.zeros(len(pts), bool)
    w = light["position"][None] - pts.astype(np.float64)
    d2 = (w * w).sum(1)
    if light["type"] == R.SPOT:
        s = (-(wi @ light["direction"]) - light["cos_outer"]) * light["inv_span"]
        tol = ABS_WINDOW * light["inv_span"]
        near |= (np.abs(s) <= tol) | (np.abs(s - 1.0) <= tol)
    if light["range"] > 0:
        q = d2 / light["range"] ** 2
        near |= np.abs(1.0 - q * q) <= ABS_WINDOW
    assert ok.all() and near.mean() < 0.01, near.mean()
    s = quad_scene()
    s.add_punctual_light(lp.point_light((9, 9, 9)))     # light 0 is another one: the index is honoured
    s.add_punctual_light(rec)
    sg = lp.SceneGPU.new_from_scene(s, device)
    gw, gd, gE = sg.sample_punctual(1, pts)
    with pytest.raises(lp.Error) as e:
        sg.sample_punctual(2, pts)
    assert e.value.kind == "InvalidArg"
    sg.close()
    keep = ~near
    assert np.all(np.isfinite(gw)) and np.all(np.isfinite(gE))
    assert np.all(np.abs(gw[keep] - wi[keep]) <= REL_W), np.abs(gw[keep] - wi[keep]).max()
    if light["type"] == R.DIRECTIONAL:
        assert np.all(gd == np.float32(1e30))
    else:
        assert np.all(np.abs(gd[keep] - dist[keep]) <= REL_W * dist[keep])
    # E: relative, plus the two absolute terms in units of the unwindowed value
    unwin = light["color"][None] * (np.ones(len(pts)) if light["type"] == R.DIRECTIONAL else 1.0 / d2)[:, None]
    bound = REL_E * E + unwin * (ABS_WINDOW * (1.0 if light["range"] > 0 else 0.0) + 2.0 * ABS_WINDOW * light["inv_span"] * (1.0 if light["type"] == R.SPOT else 0.0))
    err = np.abs(gE.astype(np.float64) - E)
    assert np.all(err[keep] <= bound[keep]), (err[keep] / np.maximum(bound[keep], 1e-300)).max()
    # exact zeros where the reference has a zero well inside a clamp: behind a spot, beyond a range
    assert np.all(gE[keep & (E.sum(1) == 0)] == 0)
    assert (E.sum(1) == 0).any() or light["type"] != R.SPOT


def test_sample_punctual_at_the_light_has_no_sample(device):
    s = quad_scene()
    s.add_punctual_light(lp.point_light((1, 2, 3), intensity=5.0))
    sg = lp.SceneGPU.new_from_scene(s, device)
    wi, dist, E = sg.sample_punctual(0, np.array([[1, 2, 3], [1, 2, 4]], np.float32))
    sg.close()
    assert not wi[0].any() and dist[0] == 0 and not E[0].any()
    assert tuple(wi[1]) == (0, 0, -1) and dist[1] == 1 and tuple(E[1]) == (5, 5, 5)


# ---------------------------------------------------------------- rendered frames against closed forms
W = H = 64
SPP = 64


def _camera(eye, direction, vfov, w, h, sub):
    """SPEC §11 in float64 from the view matrix the product is given: ray directions [h, w, len(sub)^2, 3] for sub-pixel offsets `sub` in x and y"""
    v = np.asarray(T.look(eye, direction), np.float64).reshape(4, 4)   # columns (rows here: column-major): right, up, direction, origin
    right, up, fwd, origin = v[0, :3], v[1, :3], v[2, :3], v[3, :3]
    th = np.tan(vfov / 2)
    jx, jy = np.meshgrid(sub, sub)
    x = np.arange(w)[None, :, None] + jx.reshape(-1)[None, None, :]
    y = np.arange(h)[:, None, None] + jy.reshape(-1)[None, None, :]
    cx = (2 * x / w - 1) * (w / h * th)
    cy = (1 - 2 * y / h) * th
    d = right * cx[..., None] + up * cy[..., None] + fwd
    return origin, d / np.linalg.norm(d, axis=-1, keepdims=True)


def _floor(eye, direction, vfov, w=W, h=H, g=5):
    """floor points (the plane y = 0) and view vectors of a sub-pixel grid: `edge` includes the pixel's border (for [min, max]), `mid` are midpoints (for the mean)"""
    out = {}
    for name, sub in (("edge", np.linspace(0, 1, g)), ("mid", (np.arange(g) + 0.5) / g)):
        o, d = _camera(eye, direction, vfov, w, h, sub)
        t = -o[1] / d[..., 1]
        out[name] = (o + d * t[..., None], -d)
    return out


def _lum_of(light, P, V, lit=None):
    """luminance of the closed form at floor points P[..., 3] seen along V[..., 3]; `lit(P)`: False where an occluder shadows the point"""
    sh = P.shape[:-1]
    Pf, Vf = P.reshape(-1, 3), V.reshape(-1, 3)
    out = _radiance_per_point(light, Pf, Vf)
    if lit is not None:
        out = np.where(lit(Pf), out, 0.0)
    return out.reshape(sh)


def _radiance_per_point(light, P, V):
    """luminance of punctual_ref.radiance for the floor's material (base ALBEDO, roughness 1, metallic 0, normal +Y) with a view vector PER POINT:
    SPEC §10 written out over arrays of V, since R.bsdf takes one V (test_per_point_bsdf_is_the_reference_bsdf holds the two together)"""
    Po = P + N_UP[None] * (1e-4 * (1.0 + np.abs(P).max(1)))[:, None]
    ok, wi, _, E = R.incident(light, Po)
    NoL = wi @ N_UP
    NoV = np.maximum(V @ N_UP, 1e-4)
    Hh = wi + V
    hn = np.linalg.norm(Hh, axis=1, keepdims=True)
    Hh = Hh / np.where(hn > 0, hn, 1.0)
    NoH = np.maximum(Hh @ N_UP, 0.0)
    VoH = np.maximum((Hh * V).sum(1), 0.0)
    a2 = 1.0
    D = a2 / (np.pi * ((NoH * NoH) * (a2 - 1.0) + 1.0) ** 2)
    k = 0.5
    vis = 1.0 / (4.0 * (NoL * (1 - k) + k) * (NoV * (1 - k) + k))
    F = 0.04 + 0.96 * (1.0 - VoH) ** 5
    f = (ALBEDO / np.pi) * (1.0 - F) + D * vis * F
    return np.where(ok & (NoL > 0), f * NoL * R.luminance(E), 0.0)


def test_per_point_bsdf_is_the_reference_bsdf():
    """the vectorised-over-V evaluation above against R.bsdf (one V at a time) — CPU only, but it belongs to this file's helpers"""
    rng = np.random.default_rng(2)
    light = R.make(R.POINT, position=(0.3, 1.2, -0.2), intensity=3.0)
    P = np.c_[rng.uniform(-1, 1, 16), np.zeros(16), rng.uniform(-1, 1, 16)]
    V = rng.normal(size=(16, 3))
    V[:, 1] = np.abs(V[:, 1]) + 0.5
    V /= np.linalg.norm(V, axis=1, keepdims=True)
    got = _radiance_per_point(light, P, V)
    want = [R.luminance(R.radiance(light, P[i:i + 1], N_UP, V[i], (ALBEDO,) * 3, 1.0, 0.0))[0] for i in range(16)]
    assert np.allclose(got, want, rtol=1e-12)


def _picks(n_punctual, n_rect, spp, bounces, env=False, w=W, h=H):
    """k[l][h, w]: how many of the spp samples of a pixel picked punctual light l — SPEC §19's pick from r0 (SPEC §4), in the float32 the product uses"""
    pix = np.arange(w * h, dtype=np.uint64)
    p_p = np.float32(n_punctual) / np.float32(n_punctual + n_rect)
    k = np.zeros((n_punctual, h * w), np.int64)
    for j in range(spp):
        r0 = R.r0_of(pix, 1 + j * bounces).astype(np.float32)
        rl = (r0 - np.float32(0.5)) / np.float32(0.5) if env else r0
        sel = (rl < p_p) & ((r0 >= 0.5) if env else True)
        li = np.minimum(((rl / p_p) * np.float32(n_punctual)).astype(np.int64), n_punctual - 1)
        for l in range(n_punctual):
            k[l] += sel & (li == l)
    return k.reshape(n_punctual, h, w)


def _check_pixels(img, lights, eye=EYE, direction=DIR, vfov=VFOV, lit=None, skip=None, spp=SPP, n_rect=1, abs_terms=None):
    """every pixel inside its bound (module docstring), the image mean in the project's form; returns the per-pixel expectation"""
    fl = _floor(eye, direction, vfov)
    lum = R.luminance(img[..., :3].astype(np.float64))
    picks = _picks(len(lights), n_rect, spp, 1)
    _, p_pick, _ = R.pick(len(lights), n_rect, False)
    lo = np.zeros((H, W))
    hi = np.zeros((H, W))
    want = np.zeros((H, W))
    for l, light in enumerate(lights):
        e = _lum_of(light, *fl["edge"], lit=lit)
        m = _lum_of(light, *fl["mid"], lit=lit)
        scale = picks[l] / (spp * p_pick)
        a = 0.0 if abs_terms is None else abs_terms[l]
        lo += scale * np.maximum(e.min(-1) * (1 - REL_PIXEL) - a, 0.0)
        hi += scale * (e.max(-1) * (1 + REL_PIXEL) + a)
        want += m.mean(-1)
    keep = np.ones((H, W), bool) if skip is None else ~skip
    assert np.all(np.isfinite(img))
    bad = keep & ((lum < lo) | (lum > hi))
    assert not bad.any(), (int(bad.sum()), lum[bad][:4], lo[bad][:4], hi[bad][:4])
    m, s = float(lum[keep].mean()), float(lum[keep].std(ddof=1) / np.sqrt(keep.sum()))
    w_mean = float(want[keep].mean())
    print("mean %.6g want %.6g sigma %.3g" % (m, w_mean, s))
    assert abs(m - w_mean) <= 4 * s + 2e-4 * w_mean, (m, w_mean, s)
    return want


def _scene(records, extra=None, light=None):
    s = quad_scene(light)
    for r in records:
        s.add_punctual_light(r)
    if extra is not None:
        extra(s)
    return s


def _occluder(x0, x1, y=0.5):
    """an opaque quad at height y over x0..x1 (z from -5 to 5), facing up and down alike (shadow rays test triangles from either side)"""
    def add(s):
        pos = np.array([[x0, y, -5], [x1, y, -5], [x1, y, 5], [x0, y, 5]], np.float32)
        nrm = np.tile(np.array([[0, 1, 0]], np.float32), (4, 1))
        blas = s.add_mesh(pos, nrm, np.zeros((4, 2), np.float32), np.array([0, 2, 1, 0, 3, 2], np.uint32))
        s.add_instance(blas, np.eye(4, dtype=np.float32), 1)
    return add


def _edge_band(x_edge, eye=EYE, direction=DIR, vfov=VFOV):
    """pixels within one pixel of the floor line x = x_edge (float64, from the pixel corners)"""
    o, d = _camera(eye, direction, vfov, W, H, np.array([0.0, 1.0]))
    P = o + d * (-o[1] / d[..., 1])[..., None]
    x = P[..., 0]
    pix = np.abs(x.max(-1) - x.min(-1)).max()
    return (x.min(-1) - pix <= x_edge) & (x_edge <= x.max(-1) + pix), x


# 2. ---------------------------------------------------------------------------------------------------------------
def test_point_light_depth_1(device):
    rec = lp.point_light((0.01, 0.7, -0.005), color=(1.0, 0.8, 0.6), intensity=3.0)
    img = render(device, _scene([rec]), None, W, H, 1, SPP, env=False)
    _check_pixels(img, [R.from_record(rec)])


# 3. ---------------------------------------------------------------------------------------------------------------
def test_shadow_is_exactly_black(device):
    """light at x = 0.3004, height 1; an occluder at height 0.5 over x in [0.15, 0.6] shadows the floor from x = 2 * 0.15 - 0.3004 = -0.0004 (the middle of a pixel
    column: the band of one pixel either side is then three columns, 4.7 % of the frame) to 0.9; the camera's own rays pass height 0.5 within |x| < 0.013 and never see it"""
    rec = lp.point_light((0.3004, 1.0, 0.0), intensity=5.0)
    light = R.from_record(rec)
    x_edge = 2.0 * float(np.float32(0.15)) - light["position"][0]
    band, x = _edge_band(x_edge)
    assert band.mean() <= 0.05      # seen to hold before anything is rendered
    img = render(device, _scene([rec], _occluder(0.15, 0.6)), None, W, H, 1, SPP, env=False)
    umbra = ~band & (x.min(-1) > x_edge)
    assert umbra.sum() > 0.4 * W * H and (~band & ~umbra).sum() > 0.4 * W * H
    assert np.all(img[umbra][:, :3] == 0.0)
    _check_pixels(img, [light], lit=lambda P: P[:, 0] < x_edge, skip=band | umbra)


# 4. ---------------------------------------------------------------------------------------------------------------
WIDE = 0.6   # a frame that spans a cone's or a range's footprint on the floor


def test_spot_cone(device):
    inner, outer, h = 0.05, 0.1, 2.0
    rec = lp.spot_light((0, h, 0), (0, -1, 0), intensity=9.0, inner_angle=inner, outer_angle=outer)
    light = R.from_record(rec)
    img = render(device, _scene([rec]), None, W, H, 1, SPP, env=False, vfov=WIDE)
    fl = _floor(EYE, DIR, WIDE)
    P = fl["edge"][0]
    c = h / np.sqrt(P[..., 0] ** 2 + h * h + P[..., 2] ** 2)       # the cosine at the light between its axis and the floor point
    tol = ABS_WINDOW * light["inv_span"]
    s = (c - light["cos_outer"]) * light["inv_span"]
    outside, inside = s.max(-1) < -tol, s.min(-1) > 1 + tol
    assert outside.sum() > 500 and inside.sum() > 100 and (~outside & ~inside).sum() > 100
    assert np.all(img[outside][:, :3] == 0.0)
    peak = _lum_of(R.make(R.POINT, position=(0, h, 0), intensity=9.0), *fl["edge"]).max(-1)
    _check_pixels(img, [light], vfov=WIDE, abs_terms=[2 * tol * peak])                                     # the band against s^2, everything else too
    point = R.make(R.POINT, position=(0, h, 0), intensity=9.0)                                             # inside the inner cone: the point light's expectation
    _check_pixels(img, [point], vfov=WIDE, skip=~inside)


def test_directional_and_its_shadow(device):
    d = np.array([0.3, -1.0, 0.2])
    rec = lp.directional_light(d, color=(1.0, 0.9, 0.8), intensity=2.0)
    light = R.from_record(rec)
    # unoccluded: the constant f · NoL · E (f varies with the view by 1e-4 across the frame; the closed form carries that)
    img = render(device, _scene([rec]), None, W, H, 1, SPP, env=False)
    want = _check_pixels(img, [light])
    assert want.max() / want.min() < 1.001
    # the occluder at height 0.5 over x in [-1, -0.1504]: its shadow is displaced ALONG the light's direction, by 0.5 * 0.3 / 1 in x: the floor from -0.85 to -0.0004
    x_edge = float(np.float32(-0.1504)) + 0.5 * (light["direction"][0] / -light["direction"][1])
    band, x = _edge_band(x_edge)
    assert band.mean() <= 0.05 and abs(x_edge + 0.0004) < 1e-6
    img = render(device, _scene([rec], _occluder(-1.0, -0.1504)), None, W, H, 1, SPP, env=False)
    umbra = ~band & (x.max(-1) < x_edge)
    assert umbra.sum() > 0.4 * W * H
    assert np.all(img[umbra][:, :3] == 0.0)
    _check_pixels(img, [light], lit=lambda P: P[:, 0] > x_edge, skip=band | umbra)


def test_range_cuts_to_exactly_zero(device):
    h, r = 0.2, 0.3
    rec = lp.point_light((0, h, 0), intensity=0.5, range=r)
    light = R.from_record(rec)
    img = render(device, _scene([rec]), None, W, H, 1, SPP, env=False, vfov=WIDE)
    fl = _floor(EYE, DIR, WIDE)
    P = fl["edge"][0]
    d2 = P[..., 0] ** 2 + (h - 1e-4 * (1 + np.abs(P).max(-1))) ** 2 + P[..., 2] ** 2
    beyond = (d2 / light["range"] ** 2).min(-1) > 1 + ABS_WINDOW
    assert beyond.sum() > 500 and (~beyond).sum() > 500
    assert np.all(img[beyond][:, :3] == 0.0)
    unwin = _lum_of(R.make(R.POINT, position=(0, h, 0), intensity=0.5), *fl["edge"]).max(-1)
    _check_pixels(img, [light], vfov=WIDE, abs_terms=[ABS_WINDOW * unwin])


# 5. ---------------------------------------------------------------------------------------------------------------
def test_two_point_lights_sum(device):
    recs = [lp.point_light((0.01, 0.7, -0.005), intensity=3.0), lp.point_light((-0.2, 1.5, 0.1), color=(0.2, 0.4, 1.0), intensity=0.7)]
    img = render(device, _scene(recs), None, W, H, 1, SPP, env=False)
    _check_pixels(img, [R.from_record(r) for r in recs])     # per pixel with the picks of BOTH lights (p_p = 2/3), and the mean = the sum of the two closed forms


def _rect_light():
    """the rectangle light of test_light_plus_probe_matches_quadrature: in the sun's direction, facing the quad's centre"""
    sun = np.array([0.35, 0.8, 0.25])
    sun /= np.linalg.norm(sun)
    c, n = 6.0 * sun, -sun
    t = np.cross(n, [0, 0, 1.0])
    t /= np.linalg.norm(t)
    b = np.cross(n, t)
    hw, Le = 0.6, 3.0
    light = np.zeros(1, lp._abi.LIGHT_DT)
    light["normal"] = tuple(n) + (0,)
    light["tangent"] = tuple(t) + (hw,)
    light["bitangent"] = tuple(b) + (hw,)
    light["origin"] = tuple(c) + (Le,)

    def covers(L):
        dn = L @ n
        tt = np.where(dn < 0, c @ n / np.where(dn < 0, dn, -1.0), -1.0)
        hit = L * tt[:, None] - c[None]
        return (dn < 0) & (tt > 0) & (np.abs(hit @ t) <= hw) & (np.abs(hit @ b) <= hw)
    return light, covers, Le, sun


@pytest.mark.parametrize("env", [False, True])
def test_point_light_beside_a_rectangle_light_and_the_probe(device, env):
    """depth 2, every strategy in play: the rectangle light by the env test's quadrature (NEE + BSDF rays, MIS), the probe likewise when env sampling is on, the point
    light in closed form (weight 1; nothing of it arrives over a BSDF ray).  A wrong p_pick, or a rectangle pdf without its (1 - p_p), shifts the mean by tens of per cent."""
    light, covers, Le, _ = _rect_light()
    rec = lp.point_light((-1.5, 2.0, 0.5), intensity=6.0)
    V = -np.asarray(DIR, np.float64)
    V /= np.linalg.norm(V)
    want_light = _bsdf_quadrature(const_probe(1.0), V, light_mask=lambda L: ~covers(L)) * Le
    want_point = float(R.luminance(R.radiance(R.from_record(rec), np.zeros((1, 3)), N_UP, V, (ALBEDO,) * 3, 1.0, 0.0))[0])
    rgbe = sun_probe() if env else None
    want_env = _bsdf_quadrature(rgbe, V, light_mask=covers) if env else 0.0
    img = render(device, _scene([rec], light=light), rgbe, 64, 64, 2, 64, env=env, vfov=0.01)
    m, s = _mean_sigma(img)
    want = want_light + want_point + want_env
    print("mean %.6g = light %.6g + point %.6g + env %.6g ? sigma %.3g" % (m, want_light, want_point, want_env, s))
    assert want_point > 0.2 * want
    assert abs(m - want) <= 4 * s + 1e-3 * want, (m, want_light, want_point, want_env, s)


def test_point_light_behind_a_rectangle_lights_front_contributes_nothing(device):
    light, _, _, sun = _rect_light()
    light["origin"][0][3] = 0.0                                    # the rectangle emits nothing; its front still stops what comes from behind it
    rec = lp.point_light(tuple(7.0 * sun), intensity=50.0)         # one unit behind the rectangle's centre, seen from the quad's centre
    img = render(device, _scene([rec], light=light), None, 64, 64, 2, 16, env=False, vfov=0.01)
    assert not img[..., :3].any()
    free = render(device, _scene([rec]), None, 64, 64, 2, 16, env=False, vfov=0.01)     # the same light with the rectangle out of the way
    assert free[..., :3].mean() > 0


# 6. ---------------------------------------------------------------------------------------------------------------
def _atrium_lights():
    return [lp.point_light((0.0, 2.5, 0.0), color=(1.0, 0.8, 0.6), intensity=30.0, range=20.0),
            lp.spot_light((2.0, 4.0, 1.0), (-0.3, -1.0, -0.2), intensity=80.0, inner_angle=0.3, outer_angle=0.6),
            lp.directional_light((0.4, -1.0, 0.3), color=(1.0, 0.95, 0.9), intensity=1.5)]


@pytest.fixture(scope="module")
def atrium_small():
    return scenes.synthetic_atrium(texture_size=128)


def _atrium_scene(desc, lights=True):
    s = scenes.to_product(desc)
    for r in (_atrium_lights() if lights else []):
        s.add_punctual_light(r)
    return s


def _atrium(device, desc, lights=True, **kw):
    return render(device, _atrium_scene(desc, lights), desc.get("probe"), 96, 64, 4, 2, False, eye=desc["camera"]["origin"], direction=desc["camera"]["direction"],
                  vfov=T.VFOV, **kw)


def test_atrium_bit_identical_inside_the_feature(device, atrium_small):
    desc = atrium_small
    ref = _atrium(device, desc, options=PER_BOUNCE)
    off = _atrium(device, desc, lights=False, options=PER_BOUNCE)
    assert np.all(np.isfinite(ref)) and ref.tobytes() != off.tobytes() and ref[..., :3].mean() > off[..., :3].mean()
    assert _atrium(device, desc, options=PER_BOUNCE).tobytes() == ref.tobytes()          # run to run
    assert _atrium(device, desc, options=PATH).tobytes() == ref.tobytes()                # k_path
    assert _atrium(device, desc, options=dict(PER_BOUNCE, packet_primary=0)).tobytes() == ref.tobytes()
    assert _atrium(device, desc, options=dict(PER_BOUNCE, packet_primary=1)).tobytes() == ref.tobytes()
    assert _atrium(device, desc, options=PER_BOUNCE, lanes=2).tobytes() == ref.tobytes()
    assert _atrium(device, desc, options=PATH, lanes=2).tobytes() == ref.tobytes()
    acc = np.zeros_like(ref)
    for rank in range(2):
        acc += _atrium(device, desc, options=PATH, world=2, rank=rank)
    assert acc.tobytes() == ref.tobytes()


def _renderer(device, sg, desc, w=96, h=64, rank=0, world=1, mode=None, options=PER_BOUNCE):
    r = lp.Renderer(device, (w, h))
    r.downsample_factor = 1.0
    r.resize(device, sg, None, (w, h))
    r.set_max_bounces(4)
    r.set_vfov(T.VFOV)
    for k, v in options.items():
        r.set_option(k, v)
    if world > 1:
        r.set_shard(rank, world)
        r.set_resources(device, sg, None)
    if mode is not None:
        r.set_blit_mode(mode)
    r.reset_accumulation()
    return r


def test_update_punctual_and_its_ordering(device, atrium_small):
    """unchanged data: the same frame bit for bit.  Changed data: a frame that was RECORDED before the update shows the lights the record saw — the rule of
    update_instances (recorded calls are submitted first) — and the next frame shows the new ones: the frame of a scene uploaded with them."""
    desc = atrium_small
    view = T.look(desc["camera"]["origin"], desc["camera"]["direction"])
    scene = _atrium_scene(desc)
    sg = lp.SceneGPU.new_from_scene(scene, device)

    def record(r, n=2):
        r.reset_accumulation()
        r.accumulate = True
        for _ in range(n):
            r.raytrace(view)

    def shot(sg_):   # a fresh renderer every time: a renderer's seed counter counts its frames
        r = _renderer(device, sg_, desc)
        record(r)
        img = r.read_radiance()
        r.close()
        return img

    old = shot(sg)
    assert np.all(np.isfinite(old)) and old[..., :3].any()
    sg.update_punctual(scene)                              # unchanged data
    assert shot(sg).tobytes() == old.tobytes()
    moved = lp.point_light((1.0, 3.0, -1.0), color=(0.3, 1.0, 0.3), intensity=60.0)
    scene.set_punctual_light(0, moved)
    r = _renderer(device, sg, desc)
    record(r)                                              # recorded, not submitted ...
    assert r.submission_stats()[2] > 0
    sg.update_punctual(scene)                              # ... submitted by the update, with the old lights
    assert r.submission_stats()[2] == 0
    assert r.read_radiance().tobytes() == old.tobytes()
    r.close()
    new = shot(sg)
    sg2 = lp.SceneGPU.new_from_scene(scene, device)
    assert new.tobytes() == shot(sg2).tobytes() and new.tobytes() != old.tobytes()
    # another number of lights is a rebuild's business, which carries them
    scene.add_punctual_light(lp.point_light((0, 1, 0), intensity=20.0))
    with pytest.raises(lp.Error) as e:
        sg.update_punctual(scene)
    assert e.value.kind == "InvalidArg"
    sg.rebuild(scene)
    sg3 = lp.SceneGPU.new_from_scene(scene, device)
    more = shot(sg)
    assert more.tobytes() == shot(sg3).tobytes() and more.tobytes() != new.tobytes()
    for x in (sg, sg2, sg3):
        x.close()


def test_denoised_sharded_equals_single(device, atrium_small):
    """SPEC §15.5 with punctual lights: lights are scene data, so the sharded denoised frame is the single one bit for bit"""
    desc = atrium_small
    sg = lp.SceneGPU.new_from_scene(_atrium_scene(desc), device)
    mode = lp.BlitMode.DenoisedPathrace
    one = _renderer(device, sg, desc, mode=mode)
    ranks = [_renderer(device, sg, desc, rank=q, world=2, mode=mode) for q in range(2)]
    for f in range(3):
        o = np.asarray(desc["camera"]["origin"], np.float64) + (0.05 * f, 0.02 * f, 0.0)
        view = T.look(tuple(o), desc["camera"]["direction"])
        one.raytrace(view)
        for r in ranks:
            r.raytrace(view)
        ranks[0].exchange_local(ranks[1:])
        got, want = ranks[0].read_radiance(), one.read_radiance()
        assert np.all(np.isfinite(want)) and got.tobytes() == want.tobytes(), "frame %d" % f
    for r in [one] + ranks:
        r.close()
    sg.close()


# 7. ---------------------------------------------------------------------------------------------------------------
def spot_glb():
    """a small .glb: a floor, an occluder above half of it and one spot light on a rotated, translated node (KHR_lights_punctual)"""
    blob = bytearray()
    views, accessors = [], []

    def add(arr, ctype, atype):
        raw = np.ascontiguousarray(arr).tobytes()
        views.append({"buffer": 0, "byteOffset": len(blob), "byteLength": len(raw)})
        blob.extend(raw)
        blob.extend(b"\0" * (-len(blob) % 4))
        accessors.append({"bufferView": len(views) - 1, "componentType": ctype, "count": len(arr), "type": atype})
        return len(accessors) - 1

    quad = np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], "<f4")
    nrm = np.tile(np.array([[0, 1, 0]], "<f4"), (4, 1))
    prim = {"attributes": {"POSITION": add(quad, 5126, "VEC3"), "NORMAL": add(nrm, 5126, "VEC3")}, "indices": add(np.array([0, 2, 1, 0, 3, 2], "<u2"), 5123, "SCALAR"),
            "material": 0}
    q = [np.sin(-np.pi / 4), 0.0, 0.0, np.cos(-np.pi / 4)]     # -90 degrees about X: the light's -Z axis points straight down
    js = {"asset": {"version": "2.0"}, "meshes": [{"primitives": [prim]}], "accessors": accessors, "bufferViews": views,
          "materials": [{"pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.7, 0.6, 1.0], "roughnessFactor": 0.6, "metallicFactor": 0.1}}],
          "nodes": [{"mesh": 0, "scale": [4.0, 1.0, 4.0]}, {"mesh": 0, "translation": [1.0, 0.8, 0.0], "scale": [0.5, 1.0, 0.5]},
                    {"translation": [0.2, 2.5, 0.1], "rotation": q, "extensions": {"KHR_lights_punctual": {"light": 0}}}],
          "extensionsUsed": ["KHR_lights_punctual"],
          "extensions": {"KHR_lights_punctual": {"lights": [{"type": "spot", "color": [1.0, 0.9, 0.8], "intensity": 40.0, "range": 30.0,
                                                              "spot": {"innerConeAngle": 0.4, "outerConeAngle": 0.9}}]}},
          "buffers": [{"byteLength": len(blob)}]}
    j = json.dumps(js).encode()
    j += b" " * (-len(j) % 4)
    b = bytes(blob)
    return struct.pack("<III", 0x46546C67, 2, 12 + 8 + len(j) + 8 + len(b)) + struct.pack("<II", len(j), 0x4E4F534A) + j + struct.pack("<II", len(b), 0x004E4942) + b


def test_gltf_lights_end_to_end(device):
    a = lp.Scene()
    lp.loaders.load_gltf(spot_glb(), a)
    assert a.punctual_count() == 1
    # the committed copy (tests/golden/spot-light.glb: the file `python bench.py --gltf` can be pointed at) is this writer's output
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spot-light.glb"), "rb") as f:
        assert f.read() == spot_glb()
    # the same scene through the API: meshes, material and instances added by hand, the light from the constructor
    rec = a.punctual_lights[0]
    built = lp.spot_light((0.2, 2.5, 0.1), (0, -1, 0), color=(1.0, 0.9, 0.8), intensity=40.0, range=30.0, inner_angle=0.4, outer_angle=0.9)
    assert np.allclose(rec["direction"][:3], (0, -1, 0), atol=1e-6) and np.array_equal(rec["cone"], built["cone"][0]) and np.array_equal(rec["color"], built["color"][0])
    built["direction"] = rec["direction"]      # the loader's fp32 T·R·S leaves 1e-8 of the rotation in the axis; everything else is the constructor's
    c = lp.Scene()
    for s in (c,):
        pos = np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], np.float32)
        nrm = np.tile(np.array([[0, 1, 0]], np.float32), (4, 1))
        blas = s.add_mesh(pos, nrm, None, np.array([0, 2, 1, 0, 3, 2], np.uint32))
        mat = s.add_material((0.8, 0.7, 0.6, 1.0), 0.6, 0.1)
        s.add_instance(blas, np.diag([4.0, 1.0, 4.0, 1.0]).astype(np.float32).T, mat)
        m = np.diag([0.5, 1.0, 0.5, 1.0]).astype(np.float32)
        m[:3, 3] = (1.0, 0.8, 0.0)
        s.add_instance(blas, m.T, mat)
        s.add_punctual_light(built)
    assert c.punctual_lights.tobytes() == a.punctual_lights.tobytes()
    eye, direction = (0.0, 3.0, 4.0), (0.0, -0.6, -0.8)
    frames = []
    for s in (a, c):
        s.set_light(0, _dark_light())
        frames.append(render(device, s, None, 96, 64, 3, 4, False, eye=eye, direction=direction, vfov=T.VFOV))
    assert frames[0].tobytes() == frames[1].tobytes()
    lum = R.luminance(frames[0][..., :3].astype(np.float64))
    assert lum.max() > 0.1 and (lum == 0).any()       # lit with no probe and no emitting rectangle, and the occluder's shadow is black
