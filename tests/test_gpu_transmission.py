"""-m gpu: transmissive materials (SPEC.md §21) on the device.  The interface event the shading kernels run (lpt_interface_sample) against the float32
restatement in tests/transmission_ref.py, bit for bit; frames of a few triangles whose every sample must be one of a handful of exactly known values, with the
shares of those values against the float64 expectation of the reference; bit-identity with the opaque kernels where no glass is hit and across the forms of
the frame pipeline; and a glTF file's glass end to end.

THE BOUNDS.  A sample of these scenes is a product of exactly representable factors (the probe's radiance, base colours of 0.5 / 0.25 / 1, weight 1), so its
VALUE is compared by bits.  WHICH value a sample takes is a Bernoulli draw whose probability the reference enumerates (Fresnel terms, in float64, jitter
integrated on a sub-pixel grid); a count over pixels and samples is compared with its expectation within 5 sigma, sigma^2 = sum p (1 - p) — derived, not tuned."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import scenes, testing as T

import transmission_ref as R
from test_gpu_env_sampling import _dark_light, const_probe

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
W = H = 64
VFOV = 0.6
EYE, DIR = (0.0, 0.0, 0.0), (0.0, 0.0, -1.0)
BASE = (0.5, 1.0, 0.25)
QUAD_IDX = np.array([0, 1, 2, 0, 2, 3], np.uint32)


# ---------------------------------------------------------------- scenes of a few triangles
def add_rect(s, center, u, v, hu, hv, mat):
    """the rectangle center +- hu u +- hv v as two triangles wound so that the geometric normal is u x v; flat shading normals"""
    c, u, v = (np.asarray(a, np.float64) for a in (center, u, v))
    pos = np.array([c - hu * u - hv * v, c + hu * u - hv * v, c + hu * u + hv * v, c - hu * u + hv * v], np.float32)
    nrm = np.tile(np.cross(u, v).astype(np.float32)[None], (4, 1))
    blas = s.add_mesh(pos, nrm, np.zeros((4, 2), np.float32), QUAD_IDX)
    return s.add_instance(blas, np.eye(4, dtype=np.float32), mat)


CUBE_FACES = [((0, 0, 1), (1, 0, 0), (0, 1, 0)), ((0, 0, -1), (0, 1, 0), (1, 0, 0)), ((1, 0, 0), (0, 1, 0), (0, 0, 1)), ((-1, 0, 0), (0, 0, 1), (0, 1, 0)),
              ((0, 1, 0), (0, 0, 1), (1, 0, 0)), ((0, -1, 0), (1, 0, 0), (0, 0, 1))]      # (outward normal, u, v) with u x v = normal


def cube_mesh(half=1.0):
    pos, nrm, idx = [], [], []
    for n, u, v in CUBE_FACES:
        n, u, v = (np.asarray(a, np.float64) * half for a in (n, u, v))
        k = len(pos)
        pos += [n - u - v, n + u - v, n + u + v, n - u + v]
        nrm += [n / half] * 4
        idx += [k, k + 1, k + 2, k, k + 2, k + 3]
    return np.array(pos, np.float32), np.array(nrm, np.float32), np.array(idx, np.uint32)


def cube_rects(center, half, **kw):
    return [R.rect(np.asarray(center, np.float64) + half * np.asarray(n, np.float64), u, v, half, half, **kw) for n, u, v in CUBE_FACES]


def pane_scene(tr=1.0, base=BASE, metal=0.0, thin=True, ior=1.5, mask_cutoff=None):
    """one 0.8 x 0.8 pane at z = -2 facing the camera at the origin; mask_cutoff: a masked opaque quad half way, over the whole pane"""
    s = lp.Scene()
    s.set_light(0, _dark_light())
    m = s.add_material(tuple(base) + (1.0,), 0.3, metal)
    if tr is not None:
        s.set_material_transmission(m, tr, ior, thin)
    add_rect(s, (0, 0, -2), (1, 0, 0), (0, 1, 0), 0.4, 0.4, m)
    if mask_cutoff is not None:
        mm = s.add_material((0.8, 0.2, 0.2, 1.0), 1.0, 0.0)
        s.set_material_alpha(mm, "MASK", mask_cutoff)
        add_rect(s, (0, 0, -1), (1, 0, 0), (0, 1, 0), 0.3, 0.3, mm)
    return s


PANE = dict(center=(0, 0, -2), u=(1, 0, 0), v=(0, 1, 0), hu=0.4, hv=0.4)
INTERIOR = (slice(16, 48), slice(16, 48))      # pixels wholly on the pane (asserted from the reference where it is used)


class Rig:
    """a scene on the device with one renderer"""

    def __init__(self, device, scene, probe, size=(W, H), depth=2, eye=EYE, direction=DIR, vfov=VFOV, options=None, env=False, mode=None, rank=0, world=1, sg=None):
        self.own_sg = sg is None
        self.sg = lp.SceneGPU.new_from_scene(scene, device) if sg is None else sg
        self.pr = lp.ProbeGPU(device, probe, probe.shape[1], probe.shape[0]) if probe is not None else None
        self.r = r = lp.Renderer(device, size)
        r.downsample_factor = 1.0
        r.resize(device, self.sg, self.pr, size)
        r.set_max_bounces(depth)
        r.set_vfov(vfov)
        for k, v in (options or {}).items():
            r.set_option(k, v)
        if world > 1:
            r.set_shard(rank, world)
            r.set_resources(device, self.sg, self.pr)
        if env:
            r.set_env_sampling(True)
        if mode is not None:
            r.set_blit_mode(mode)
        self.view = T.look(eye, direction)
        r.reset_accumulation()

    def samples(self, n):
        """n single-sample frames [n, h, w, 3] (accumulate off: every frame is one sample per pixel with its own seed)"""
        self.r.accumulate = False
        out = []
        for _ in range(n):
            self.r.raytrace(self.view)
            out.append(self.r.read_radiance()[..., :3].copy())
        return np.stack(out)

    def frame(self, n):
        self.r.reset_accumulation()
        self.r.accumulate = True
        for _ in range(n):
            self.r.raytrace(self.view)
        return self.r.read_radiance()

    def close(self):
        self.r.close()
        if self.pr is not None:
            self.pr.close()
        if self.own_sg:
            self.sg.close()


def frame_of(device, scene, probe, n=4, **kw):
    rig = Rig(device, scene, probe, **kw)
    img = rig.frame(n)
    rig.close()
    return img


def _is(x, value):
    return (x.view(np.uint32) == np.asarray(value, np.float32).view(np.uint32)).all(-1)


# ---------------------------------------------------------------- 1. the hook against the float32 reference, bit for bit
def _unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def _hook_inputs():
    rng = np.random.default_rng(21)
    n = 4096
    ngf = _unit(rng.normal(size=(n, 3)))
    d = _unit(rng.normal(size=(n, 3)))
    d = np.where(((d * ngf).sum(1) > 0)[:, None], -d, d)                       # Ngf is flipped against d
    ns = _unit(ngf + 0.4 * rng.normal(size=(n, 3)))
    ns = np.where(((ns * ngf).sum(1) < 0)[:, None], -ns, ns)                   # §12: Ns on Ngf's side
    rows = [(d, ns, ngf, rng.random(n) < 0.5, rng.random((n, 3)), rng.uniform(1.0, 2.5, n), rng.random(n) < 0.3, rng.random(n))]
    z = np.array([0.0, 0.0, 1.0])

    def at(c, **kw):        # a ray with cosine c against N = Ngf = +z
        e = dict(d=np.array([np.sqrt(max(0.0, 1 - c * c)), 0.0, -c]), ns=z, ngf=z, entering=True, base=(0.5, 1.0, 0.25), ior=1.5, thin=False)
        e.update(kw)
        return [(e["d"][None], np.asarray(e["ns"], float)[None], np.asarray(e["ngf"], float)[None], np.array([e["entering"]]), np.array([e["base"]], float),
                 np.array([e["ior"]]), np.array([e["thin"]]), np.array([r4])) for r4 in (0.0, 0.02, 0.04, 0.05, 0.5, 0.999, 1.0)]

    cc = float(np.sqrt(1 - 1 / 2.25))
    for kw in (dict(c=1.0), dict(c=1e-4), dict(c=1e-4, entering=False), dict(c=cc - 1e-6, entering=False), dict(c=cc + 1e-6, entering=False),
               dict(c=float(np.float32(cc)), entering=False), dict(c=0.7, ior=1.0), dict(c=0.3, ior=1.0, entering=False), dict(c=0.5, thin=True),
               dict(c=0.5, thin=True, entering=False), dict(c=0.2, ns=(0, 0, -1)), dict(c=0.1, ns=_unit(np.array([0.09, 0.0, 0.996]))), dict(c=0.1, ns=_unit(np.array([-0.6, 0.0, 0.8]))),
               dict(c=0.1, ns=_unit(np.array([0.8, 0.0, 0.6])), entering=False), dict(c=0.0)):
        rows += at(**kw)
    return [np.concatenate([r[k] for r in rows]) for k in range(8)]


def test_interface_sample_equals_the_reference_bit_for_bit(device):
    d, ns, ngf, entering, base, ior, thin, r4 = _hook_inputs()
    f = np.float32
    d, ns, ngf, base, ior, r4 = d.astype(f), ns.astype(f), ngf.astype(f), base.astype(f), ior.astype(f), r4.astype(f)
    wi, weight, kind = device.interface_sample(d, ns, ngf, entering, base, ior, thin, r4)
    rwi, rweight, rtr = R.interface_sample(d, ns, ngf, entering, base, ior, thin, r4)
    assert np.all(np.isfinite(wi)) and len(d) > 4096 + 90
    assert np.array_equal(kind.astype(bool), rtr), int((kind.astype(bool) != rtr).sum())
    assert np.array_equal(wi.view(np.uint32), rwi.view(np.uint32)), int((wi.view(np.uint32) != rwi.view(np.uint32)).any(1).sum())
    assert np.array_equal(weight.view(np.uint32), rweight.view(np.uint32))
    assert 0.05 < rtr.mean() < 0.95        # both branches are exercised


# ---------------------------------------------------------------- 2. a thin tinted pane before a constant probe
def _pane_fresnel(grid=4):
    """the jitter-averaged Fresnel term per pixel of the pane scene, from the reference's expectation: with a unit probe and depth 2 the red channel of a
    pane pixel is Fr + (1 - Fr) * 0.5; also asserts that INTERIOR lies on the pane (the borders of its pixels hit it)"""
    view = T.look(EYE, DIR)
    pane = R.rect(PANE["center"], PANE["u"], PANE["v"], PANE["hu"], PANE["hv"], kind="thin", ior=1.5, base=BASE)
    mean, _, pz = R.expectation([pane], (1, 1, 1), view, VFOV, W, H, 2, grid)
    o, dd = R.camera_rays(view, VFOV, W, H, np.array([0.0, 1.0]))
    hit = R._nearest([pane], np.broadcast_to(o, (W * H * 4, 3)), dd.reshape(-1, 3), np.full(W * H * 4, -1))[1].reshape(H, W, 4)
    assert (hit[INTERIOR] == 0).all() and (pz == 0).all()
    return (2.0 * mean[:, 0] - 1.0).reshape(H, W)


def test_thin_tinted_pane_before_a_constant_probe(device):
    S = 32
    rig = Rig(device, pane_scene(), const_probe(0.5), depth=2)
    x = rig.samples(S)
    rig.close()
    L = x[0, 0, 0]                                   # beside the pane: the probe's radiance as the device decodes it
    assert (L > 0).all() and _is(x[:, 0, 0], L).all() and _is(x[:, H - 1, W - 1], L).all()
    refl, trans = _is(x, L), _is(x, L * np.float32(BASE))
    inner_r, inner_t = refl[(slice(None),) + INTERIOR], trans[(slice(None),) + INTERIOR]
    assert (inner_r ^ inner_t).all(), int((~(inner_r ^ inner_t)).sum())       # exactly one of the two values, every sample
    Fr = _pane_fresnel()[INTERIOR]
    want, sigma = S * Fr.sum(), np.sqrt(S * (Fr * (1 - Fr)).sum())
    got = int(inner_r.sum())
    print("pane: reflect samples %d, expected %.1f +- %.1f" % (got, want, sigma))
    assert abs(got - want) <= 5 * sigma, (got, want, sigma)
    assert (x[1:] != x[:-1]).any()                   # the frames are different samples


# ---------------------------------------------------------------- 3. a closed solid cube: the furnace
CUBE_EYE, CUBE_C, CUBE_HALF = (1.2, 0.9, 0.0), (0.0, 0.0, -3.0), 0.5
CUBE_DIR = tuple(np.subtract(CUBE_C, CUBE_EYE))
CUBE_PIX = (slice(24, 40), slice(24, 40))


def cube_scene():
    s = lp.Scene()
    s.set_light(0, _dark_light())
    m = s.add_material((1.0, 1.0, 1.0, 1.0), 0.3, 0.0)
    s.set_material_transmission(m, 1.0, 1.5, False)
    pos, nrm, idx = cube_mesh(CUBE_HALF)
    blas = s.add_mesh(pos, nrm, np.zeros((len(pos), 2), np.float32), idx)
    xf = np.eye(4, dtype=np.float32)
    xf[:3, 3] = CUBE_C
    s.add_instance(blas, xf.T, m)
    return s


@pytest.mark.parametrize("DEPTH", [12, 4])      # 12: the truncated mass is ~1e-9, every sample is the probe's radiance; 4: 1.1 % of the samples are truncated paths
def test_closed_solid_cube_furnace(device, DEPTH):
    S = 16
    ys, xs = np.meshgrid(np.arange(24, 40), np.arange(24, 40), indexing="ij")
    px = np.stack([ys.ravel(), xs.ravel()], 1)
    rects = cube_rects(CUBE_C, CUBE_HALF, kind="solid", ior=1.5)
    view = T.look(CUBE_EYE, CUBE_DIR)
    mean, var, pz = R.expectation(rects, (1, 1, 1), view, VFOV, W, H, DEPTH, 1, px)      # the pixel centres
    o, dd = R.camera_rays(view, VFOV, W, H, np.array([0.0, 1.0]))
    corner = dd[CUBE_PIX].reshape(-1, 3)
    assert (R._nearest(rects, np.broadcast_to(o, corner.shape), corner, np.full(len(corner), -1))[1] >= 0).all()      # the pixels lie on the cube
    assert pz.mean() < 0.05, pz.mean()
    assert np.allclose(mean[:, 0], 1 - pz, atol=1e-12)                                    # white glass loses nothing but the truncated paths
    rig = Rig(device, cube_scene(), const_probe(0.5), depth=DEPTH, eye=CUBE_EYE, direction=CUBE_DIR)
    x = rig.samples(S)
    rig.close()
    assert np.all(np.isfinite(x))
    L = x[0, 0, 0]
    assert (L > 0).all() and _is(x[:, 0, 0], L).all()
    inner = x[(slice(None),) + CUBE_PIX]
    zero, full = _is(inner, np.zeros(3, np.float32)), _is(inner, L)
    assert (zero ^ full).all(), int((~(zero ^ full)).sum())
    want, sigma = S * pz.sum(), np.sqrt(S * (pz * (1 - pz)).sum())
    print("cube: truncated samples %d of %d, expected %.2f +- %.2f (mass %.4f)" % (zero.sum(), zero.size, want, sigma, pz.mean()))
    assert abs(int(zero.sum()) - want) <= 5 * sigma + 1e-9, (int(zero.sum()), want, sigma)


# ---------------------------------------------------------------- 4. slab refraction and delta MIS
SLAB_H, SLAB_LE = 0.5, 4.0
SLAB_DIR = (1.0, 0.0, -1.0)                     # 45 degrees onto a slab whose faces are z = -2 and z = -2 - h
SLAB_EMIT_X = 2.0 + SLAB_H * (np.sin(np.pi / 4) / np.sqrt(2.25 - 0.5)) + (2.0 - SLAB_H)      # where the central ray, shifted by the slab, meets z = -4
SLAB_ROWS = slice(28, 36)


def slab_scene():
    s = lp.Scene()
    l = np.zeros(1, lp._abi.LIGHT_DT)
    l["normal"], l["tangent"], l["bitangent"], l["origin"] = (0, 0, 1, 0), (1, 0, 0, 0.15), (0, 1, 0, 1.0), (SLAB_EMIT_X, 0, -4.0, SLAB_LE)
    s.set_light(0, l)
    m = s.add_material((1.0, 1.0, 1.0, 1.0), 0.3, 0.0)
    s.set_material_transmission(m, 1.0, 1.5, False)
    add_rect(s, (2, 0, -2), (1, 0, 0), (0, 1, 0), 1.5, 1.5, m)                  # outward normal +z
    add_rect(s, (2, 0, -2 - SLAB_H), (0, 1, 0), (1, 0, 0), 1.5, 1.5, m)         # outward normal -z
    return s


def slab_rects():
    return [R.rect((2, 0, -2), (1, 0, 0), (0, 1, 0), 1.5, 1.5, kind="solid", ior=1.5), R.rect((2, 0, -2 - SLAB_H), (0, 1, 0), (1, 0, 0), 1.5, 1.5, kind="solid", ior=1.5),
            R.rect((SLAB_EMIT_X, 0, -4.0), (1, 0, 0), (0, 1, 0), 0.15, 1.0, kind="emitter", Le=SLAB_LE)]


def test_slab_refraction_and_delta_mis(device):
    """the emitter is seen through the slab where the lateral shift h sin(t) (1 - cos(t) / sqrt(n^2 - sin^2(t))) puts it, with weight 1.  The bound per pixel column: 5 sigma of the
    reference's own per-sample variance over rows x spp samples, plus the reference's quadrature error (4x4 against 8x8 sub-pixel grids), plus 256 x 2^-24 relative for the float32
    accumulation of 256 samples"""
    DEPTH, SPP = 4, 256
    rig = Rig(device, slab_scene(), const_probe(0.25), depth=DEPTH, direction=SLAB_DIR)
    one = rig.samples(8)
    img = rig.frame(SPP)[..., :3].astype(np.float64)
    rig.close()
    Lp = one[:, 0, 0].max(0)                                 # the corner looks through the slab too: the probe's radiance, or 0 for a truncated path
    le = np.full(3, SLAB_LE, np.float32)
    ok = _is(one, Lp) | _is(one, le) | _is(one, np.zeros(3, np.float32))
    assert ok.all(), int((~ok).sum())                        # the probe, exactly Le (weight 1, no MIS), or a truncated path
    assert _is(one, le).any()
    ys, xs = np.meshgrid(np.arange(SLAB_ROWS.start, SLAB_ROWS.stop), np.arange(W), indexing="ij")
    px = np.stack([ys.ravel(), xs.ravel()], 1)
    view = T.look(EYE, SLAB_DIR)
    probe = np.asarray(Lp, np.float64)
    m8, v8, _ = R.expectation(slab_rects(), probe, view, VFOV, W, H, DEPTH, 8, px)
    m4, _, _ = R.expectation(slab_rects(), probe, view, VFOV, W, H, DEPTH, 4, px)
    rows = SLAB_ROWS.stop - SLAB_ROWS.start
    want = m8[:, 0].reshape(rows, W).mean(0)
    quad = np.abs(m8[:, 0] - m4[:, 0]).reshape(rows, W).mean(0)
    sigma = np.sqrt(v8[:, 0].reshape(rows, W).sum(0) / SPP) / rows
    got = img[SLAB_ROWS, :, 0].mean(0)
    bound = 5 * sigma + quad + SPP * 2.0 ** -24 * want
    lit = want > 2 * probe[0]
    print("slab: columns seeing the emitter", np.flatnonzero(lit), "max |got - want| / bound %.3f" % (np.abs(got - want) / bound).max())
    assert 3 <= lit.sum() <= 12
    assert np.all(np.abs(got - want) <= bound), (np.flatnonzero(np.abs(got - want) > bound), got, want)


# ---------------------------------------------------------------- 5. opaque hits in the TRANS kernels are unchanged
@pytest.fixture(scope="module")
def atrium_small():
    return scenes.synthetic_atrium(texture_size=128)


def _atrium_with_sealed_glass(desc, factor, punctual=False):
    """the atrium plus one transmissive triangle inside a closed opaque box far outside the building: no ray reaches it"""
    s = scenes.to_product(desc)
    box = s.add_material((0.5, 0.5, 0.5, 1.0), 1.0, 0.0)
    pos, nrm, idx = cube_mesh(0.5)
    blas = s.add_mesh(pos, nrm, np.zeros((len(pos), 2), np.float32), idx)
    xf = np.eye(4, dtype=np.float32)
    xf[:3, 3] = (0.0, -400.0, 0.0)
    s.add_instance(blas, xf.T, box)
    glass = s.add_material((1.0, 1.0, 1.0, 1.0), 0.2, 0.0)
    s.set_material_transmission(glass, factor, 1.5, True)
    tri = s.add_mesh(np.array([[-0.1, -400, -0.1], [0.1, -400, -0.1], [0, -400, 0.1]], np.float32), np.tile(np.float32([[0, 1, 0]]), (3, 1)), np.zeros((3, 2), np.float32),
                     np.array([0, 1, 2], np.uint32))
    s.add_instance(tri, np.eye(4, dtype=np.float32), glass)
    if punctual:
        s.add_punctual_light(lp.point_light((0.0, 2.5, 0.0), color=(1.0, 0.8, 0.6), intensity=30.0, range=20.0))
    return s


@pytest.mark.parametrize("variant", ["plain", "env", "punctual"])
def test_opaque_hits_in_the_trans_kernels_are_unchanged(device, atrium_small, variant):
    desc = atrium_small
    kw = dict(size=(96, 64), depth=4, eye=desc["camera"]["origin"], direction=desc["camera"]["direction"], vfov=T.VFOV, env=variant == "env")
    frames = [frame_of(device, _atrium_with_sealed_glass(desc, f, variant == "punctual"), desc.get("probe"), n=2, **kw) for f in (0.0, 1.0)]
    assert np.all(np.isfinite(frames[0])) and frames[0][..., :3].any()
    assert frames[0].tobytes() == frames[1].tobytes()
    # the same through the denoiser's primary pass (the GBUF instantiations)
    g = [frame_of(device, _atrium_with_sealed_glass(desc, f, variant == "punctual"), desc.get("probe"), n=2, mode=lp.BlitMode.DenoisedPathrace, **kw) for f in (0.0, 1.0)]
    assert g[0].tobytes() == g[1].tobytes()


# ---------------------------------------------------------------- 6. launch independence
@pytest.mark.parametrize("size", [(64, 64), (256, 256)], ids=lambda s: "%dx%d" % s)
def test_launch_independence(device, size):
    """64x64 x 4 samples is a wavefront of the cooperative range, 256x256 x 1 sample one of the path kernel's range (which a glass scene leaves to the per-bounce launches)"""
    scene, probe = pane_scene(tr=0.7, metal=0.2), const_probe(0.5)
    kw = dict(size=size, depth=4, n=4 if size[0] == 64 else 1)
    want = frame_of(device, scene, probe, **kw)
    assert np.all(np.isfinite(want))
    variants = [dict(options={"coop_rays": 0}), dict(options={"path_rays": 0}), dict(options={"packet_primary": 0}), dict(options={"packet_primary": 1})]
    if size[0] == 256:
        variants.append(dict(options={"wavefront_rays": size[0] * size[1] // 2}))       # the frame as two pieces
    for v in variants:
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


# ---------------------------------------------------------------- 7. tr = 0.5, metallic 0 and 1
def test_half_transmission_metallic_zero_and_one(device):
    probe = const_probe(0.5)
    opaque = frame_of(device, pane_scene(tr=None, metal=1.0), probe, depth=2)
    assert frame_of(device, pane_scene(tr=0.5, metal=1.0), probe, depth=2).tobytes() == opaque.tobytes()       # pt = 0: the opaque material's frame
    S = 32
    rig = Rig(device, pane_scene(tr=0.5, metal=0.0), probe, depth=2)
    x = rig.samples(S)
    rig.close()
    L = x[0, 0, 0]
    inner = x[(slice(None),) + INTERIOR]
    in_set = _is(inner, L) | _is(inner, L * np.float32(BASE))
    n = in_set.size
    got, want, sigma = int(in_set.sum()), 0.5 * n, np.sqrt(0.25 * n)
    print("half: interface samples %d of %d" % (got, n))
    assert abs(got - want) <= 5 * sigma, (got, want, sigma)


# ---------------------------------------------------------------- 8. mask and glass together
def test_a_cut_away_mask_in_front_of_the_pane_changes_nothing(device):
    probe = const_probe(0.5)
    want = Rig(device, pane_scene(), probe, depth=3)
    got = Rig(device, pane_scene(mask_cutoff=2.0), probe, depth=3)       # cutoff 2: color.w = 1 never reaches it, the quad is cut away everywhere
    a, b = want.samples(4), got.samples(4)
    want.close()
    got.close()
    assert a.tobytes() == b.tobytes()
    solid = Rig(device, pane_scene(mask_cutoff=0.5), probe, depth=3)     # ... and a mask that keeps the quad does change the frame
    c = solid.samples(1)
    solid.close()
    assert c.tobytes() != a[:1].tobytes()


# ---------------------------------------------------------------- 9. glTF end to end
GLB_FLOOR = np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], "<f4")
GLB_PANE = np.array([[-1, 0, 0], [1, 0, 0], [1, 2, 0], [-1, 2, 0]], "<f4")           # vertical, normal +z
_DEFAULT = object()


def glass_glb(pane=_DEFAULT, cube=_DEFAULT, cube_thickness=0.5):
    """a small .glb: a 8x8 floor, one thin pane (KHR_materials_transmission alone), one solid cube (transmission 0.9, ior 1.33, a volume) and one directional
    light.  `pane` / `cube`: other `extensions` objects for the two materials (None: none at all)"""
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
    front = np.tile(np.array([[0, 0, 1]], "<f4"), (4, 1))
    qi = add(np.array([0, 2, 1, 0, 3, 2], "<u2"), 5123, "SCALAR")
    pi = add(np.array([0, 1, 2, 0, 2, 3], "<u2"), 5123, "SCALAR")
    cp, cn, ci = cube_mesh(0.5)
    meshes = [{"primitives": [{"attributes": {"POSITION": add(GLB_FLOOR, 5126, "VEC3"), "NORMAL": add(up, 5126, "VEC3")}, "indices": qi, "material": 0}]},
              {"primitives": [{"attributes": {"POSITION": add(GLB_PANE, 5126, "VEC3"), "NORMAL": add(front, 5126, "VEC3")}, "indices": pi, "material": 1}]},
              {"primitives": [{"attributes": {"POSITION": add(cp.astype("<f4"), 5126, "VEC3"), "NORMAL": add(cn.astype("<f4"), 5126, "VEC3")},
                               "indices": add(ci.astype("<u2"), 5123, "SCALAR"), "material": 2}]}]
    if pane is _DEFAULT:
        pane = {"KHR_materials_transmission": {"transmissionFactor": 1.0}}
    if cube is _DEFAULT:
        cube = {"KHR_materials_transmission": {"transmissionFactor": 0.9}, "KHR_materials_ior": {"ior": 1.33}}
        if cube_thickness is not None:
            cube["KHR_materials_volume"] = {"thicknessFactor": cube_thickness}
    mats = [{"pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.7, 0.6, 1.0], "roughnessFactor": 0.6, "metallicFactor": 0.1}},
            {"pbrMetallicRoughness": {"baseColorFactor": [0.5, 1.0, 0.25, 1.0], "roughnessFactor": 0.1, "metallicFactor": 0.0}},
            {"pbrMetallicRoughness": {"baseColorFactor": [1.0, 1.0, 1.0, 1.0], "roughnessFactor": 0.1, "metallicFactor": 0.0}}]
    if pane is not None:
        mats[1]["extensions"] = pane
    if cube is not None:
        mats[2]["extensions"] = cube
    q = [float(np.sin(-np.pi / 4)), 0.0, 0.0, float(np.cos(-np.pi / 4))]     # -90 degrees about X: the light's -Z axis points straight down
    js = {"asset": {"version": "2.0"}, "meshes": meshes, "accessors": accessors, "bufferViews": views, "materials": mats,
          "nodes": [{"mesh": 0, "scale": [4.0, 1.0, 4.0]}, {"mesh": 1, "translation": [0.0, 0.0, 1.0]}, {"mesh": 2, "translation": [1.5, 0.5, -1.0]},
                    {"rotation": q, "extensions": {"KHR_lights_punctual": {"light": 0}}}],
          "extensionsUsed": ["KHR_lights_punctual", "KHR_materials_transmission", "KHR_materials_ior", "KHR_materials_volume"],
          "extensions": {"KHR_lights_punctual": {"lights": [{"type": "directional", "color": [1.0, 0.95, 0.9], "intensity": 3.0}]}},
          "buffers": [{"byteLength": len(blob)}]}
    j = json.dumps(js).encode()
    j += b" " * (-len(j) % 4)
    b = bytes(blob)
    return struct.pack("<III", 0x46546C67, 2, 12 + 8 + len(j) + 8 + len(b)) + struct.pack("<II", len(j), 0x4E4F534A) + j + struct.pack("<II", len(b), 0x004E4942) + b


def test_gltf_glass_end_to_end(device):
    path = os.path.join(HERE, "golden", "glass-pane.glb")
    with open(path, "rb") as f:
        assert f.read() == glass_glb()                       # the committed copy is this writer's output
    a = lp.Scene()
    lp.loaders.load_gltf(glass_glb(), a)
    assert a.material_transmission(2) == (1.0, 1.5, True) and a.material_transmission(3)[2] is False and a.material_transmission(1)[0] == 0.0
    c = lp.Scene()
    mats = [c.add_material((0.8, 0.7, 0.6, 1.0), 0.6, 0.1), c.add_material((0.5, 1.0, 0.25, 1.0), 0.1, 0.0), c.add_material((1.0, 1.0, 1.0, 1.0), 0.1, 0.0)]
    c.set_material_transmission(mats[1], 1.0)
    c.set_material_transmission(mats[2], 0.9, ior=1.33, thin_walled=False)
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
    c.add_punctual_light(a.punctual_lights[:1].copy())      # the loader's record (its fp32 rotation leaves 1e-8 in the axis)
    assert [c.material_transmission(m) for m in range(4)] == [a.material_transmission(m) for m in range(4)]
    frames = []
    for s in (a, c):
        s.set_light(0, _dark_light())
        frames.append(frame_of(device, s, const_probe(0.25), n=4, size=(96, 64), depth=6, eye=(0.5, 1.2, 5.0), direction=(0.0, -0.15, -1.0), vfov=T.VFOV))
    assert np.all(np.isfinite(frames[0])) and frames[0][..., :3].any()
    assert frames[0].tobytes() == frames[1].tobytes()
    # ... and the glass is there: the same file without the extensions renders another frame
    b = lp.Scene()
    lp.loaders.load_gltf(glass_glb(pane=None, cube=None), b)
    b.set_light(0, _dark_light())
    assert frame_of(device, b, const_probe(0.25), n=4, size=(96, 64), depth=6, eye=(0.5, 1.2, 5.0), direction=(0.0, -0.15, -1.0), vfov=T.VFOV).tobytes() != frames[0].tobytes()


def test_bench_renders_the_glass_file():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "1", "--frames-per-step", "2", "--width", "256", "--height", "256", "--no-extras",
                        "--camera", "0.5,1.2,5,0,-0.15,-1", "--gltf", os.path.join(HERE, "golden", "glass-pane.glb")], capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    j = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert j["data"] == "real" and "glass-pane.glb" in j["config"]["workload"] and j["config"]["frame_complete"] is True and j["value"] > 0


# ---------------------------------------------------------------- 10. the tables follow the scene through an instance update and both arms of a rebuild
@pytest.mark.parametrize("big", [False, True], ids=["fewer-than-16-triangles", "16-triangles"])
def test_tables_follow_update_and_rebuild(device, big):
    """a pane whose material turns into glass by an instance update, is edited again by a rebuild alone, and turns opaque again by an instance update: after each
    step the frame is the frame of a fresh upload of the scene as edited.  A scene of fewer than 16 triangles takes the rebuild's refit arm, one of 16 its GPU build"""
    probe = const_probe(0.5)
    kw = dict(n=4, size=(64, 36), depth=3)

    def moved(dx):
        m = np.eye(4, dtype=np.float32)
        m[0, 3] = dx
        return m.T

    s = lp.Scene()
    s.set_light(0, _dark_light())
    pane_mat = s.add_material(BASE + (1.0,), 0.3, 0.0)
    pane = add_rect(s, (0, 0, -2), (1, 0, 0), (0, 1, 0), 0.4, 0.4, pane_mat)
    add_rect(s, (0.3, 0.1, -3), (1, 0, 0), (0, 1, 0), 0.5, 0.5, s.add_material((0.8, 0.2, 0.2, 1.0), 1.0, 0.0))       # behind the pane: seen through the glass only
    if big:
        pos, nrm, idx = cube_mesh(0.3)
        xf = np.eye(4, dtype=np.float32)
        xf[:3, 3] = (-0.5, 0.1, -3.5)
        s.add_instance(s.add_mesh(pos, nrm, np.zeros((len(pos), 2), np.float32), idx), xf.T, s.add_material((0.2, 0.8, 0.2, 1.0), 0.8, 0.0))
    sg = lp.SceneGPU.new_from_scene(s, device)
    assert (sg.stats().triangles >= 16) == big

    def check(other_than=None):
        got, fresh = frame_of(device, s, probe, sg=sg, **kw), frame_of(device, s, probe, **kw)
        assert np.all(np.isfinite(fresh)) and got.tobytes() == fresh.tobytes()
        assert other_than is None or fresh.tobytes() != other_than.tobytes()
        return fresh

    opaque = check()
    s.set_material_transmission(pane_mat, 1.0, 1.5, True)         # opaque -> glass, by an instance update
    s.set_instance_transform(pane, moved(0.05))
    assert sg.update_instances(s) == 1
    glass = check(other_than=opaque)
    s.set_material_transmission(pane_mat, 0.6, 1.33, False)       # no instance changed: the rebuild alone carries the new record
    sg.rebuild(s)
    check(other_than=glass)
    s.set_material_transmission(pane_mat, 0.0)                    # ... and opaque again, by an instance update
    s.set_instance_transform(pane, moved(0.0))
    assert sg.update_instances(s) == 1
    assert check(other_than=glass).tobytes() == opaque.tobytes()
    sg.close()
