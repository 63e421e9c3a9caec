"""-m gpu: environment importance sampling in next-event estimation (SPEC.md §18, lpt_renderer_set_env_sampling).  The sampler the shading
kernels run (lpt_probe_sample / lpt_probe_pdf) against its own density and the float64 restatement in tests/env_ref.py; rendered means
against numpy quadrature and against the off mode (both unbiased); the variance it buys; bit-identity across every form of the frame
pipeline inside the mode; and that the mode off — or without a distribution to sample — leaves every frame as it was."""
import numpy as np
import pytest
from scipy import stats

import loupiote_amd as lp
from loupiote_amd import scenes, testing as T

import env_ref

pytestmark = pytest.mark.gpu

EYE, DIR = (0.0, 1.0, 0.0), (0.0, -1.0, 0.02)   # straight down (nearly: the camera needs a horizontal right vector) onto the quad
VFOV = 0.05
ALBEDO = 0.5


def sun_probe():
    return scenes.sky_probe(64, 32)


def const_probe(level=0.5):
    e = int(np.floor(np.log2(level))) + 1   # level = m / 256 * 2^e, m in [128, 256)
    m = int(round(level / 2.0 ** e * 256))
    return np.array([[[m, m, m, e + 128]]], np.uint8)


def _dark_light():
    """the scene's one rectangle light switched off, far below the quad and facing away from it: n_lights = 1, nothing emitted"""
    l = np.zeros(1, lp._abi.LIGHT_DT)
    l["normal"] = (0, -1, 0, 0)
    l["tangent"] = (1, 0, 0, 0.1)
    l["bitangent"] = (0, 0, 1, 0.1)
    l["origin"] = (0, -50.0, 0, 0.0)
    return l


def quad_scene(light=None):
    s = lp.Scene()
    pos = np.array([[-200, 0, -200], [200, 0, -200], [200, 0, 200], [-200, 0, 200]], np.float32)
    nrm = np.tile(np.array([[0, 1, 0]], np.float32), (4, 1))
    uv = np.zeros((4, 2), np.float32)
    blas = s.add_mesh(pos, nrm, uv, np.array([0, 2, 1, 0, 3, 2], np.uint32))
    mat = s.add_material((ALBEDO, ALBEDO, ALBEDO, 1.0), 1.0, 0.0)
    s.add_instance(blas, np.eye(4, dtype=np.float32), mat)
    s.set_light(0, _dark_light() if light is None else light)
    return s


def render(device, scene, probe, w, h, bounces, frames, env, eye=EYE, direction=DIR, vfov=VFOV, options=None, world=1, rank=0,
           lanes=None, toggle=False, destroy_probe=False):
    sg = lp.SceneGPU.new_from_scene(scene, device)
    pr = lp.ProbeGPU(device, probe, probe.shape[1], probe.shape[0]) if probe is not None else None
    r = lp.Renderer(device, (w, h))
    r.downsample_factor = 1.0
    r.resize(device, sg, pr, (w, h))
    r.set_max_bounces(bounces)
    r.set_vfov(vfov)
    for k, v in (options or {}).items():
        r.set_option(k, v)
    if lanes is not None:
        r.set_lanes(lanes)
    if world > 1:
        r.set_shard(rank, world)
        r.set_resources(device, sg, pr)
    if toggle:
        r.set_env_sampling(True)
    r.set_env_sampling(env)
    assert r.get_env_sampling() == bool(env)
    if destroy_probe:
        pr.close()
        pr = None
    view = T.look(eye, direction)
    r.reset_accumulation()
    r.accumulate = True
    for _ in range(frames):
        r.raytrace(view)
    img = r.read_radiance()
    r.close()
    if pr is not None:
        pr.close()
    sg.close()
    return img


# ---------------------------------------------------------------- 1. the sampler against its own density
@pytest.mark.parametrize("which", ["sky", "sun"])
def test_sampler_matches_its_pdf(device, which):
    rgbe = scenes.sky_probe(64, 32) if which == "sky" else scenes.sky_probe(64, 32, sun_power=400.0)
    H, W = rgbe.shape[:2]
    pr = lp.ProbeGPU(device, rgbe, W, H)
    n = 1 << 20
    u = np.random.default_rng(11).random((n, 6), dtype=np.float32)
    dirs, ps, rad = pr.sample(u)
    ok = ps > 0
    assert ok.mean() > 0.999
    assert np.all(np.isfinite(dirs)) and np.all(np.abs(np.linalg.norm(dirs[ok], axis=1) - 1) < 1e-5)
    # the sampled cell, from the direction and the in-cell uniforms r1, r2
    uu, vv = env_ref.uv_of(dirs[ok])
    col = np.mod(np.rint(uu * W - u[ok, 4]).astype(np.int64), W)
    row = np.clip(np.rint(vv * H - u[ok, 5]).astype(np.int64), 0, H - 1)
    dist = lp.env_distribution(rgbe)
    # p_s = p_e(d) away from the cell borders (the approximations env_lookup's (u, v) go through may put a point on the border into the next cell)
    pe = pr.pdf(dirs[ok])
    fx, fy = uu * W, vv * H
    inner = (np.abs(fx - np.rint(fx)) > 1e-3) & (np.abs(fy - np.rint(fy)) > 1e-3)
    assert inner.mean() > 0.99
    # the approximations are good to ~1e-4 rad, so a few points per ten thousand still land one cell over (the border band SPEC §18 allows)
    same = np.isclose(pe[inner], ps[ok][inner], rtol=1e-3, atol=0)
    assert same.mean() > 0.998, same.mean()
    # p_e on the GPU is the reference's (exact atan2 / acos there: the same border band)
    ref = env_ref.pdf_e(dist["pdf_uv"].astype(np.float64), dirs[ok][inner])
    assert np.isclose(pe[inner], ref, rtol=1e-4, atol=0).mean() > 0.998
    # the cells are drawn in proportion to pdf_uv: chi-square, sparse cells pooled
    expect = dist["pdf_uv"].astype(np.float64).ravel() / (W * H) * ok.sum()
    got = np.bincount(row * W + col, minlength=W * H).astype(np.float64)
    assert np.all(got[expect == 0] == 0)
    big = expect >= 5
    e2 = np.append(expect[big], expect[~big].sum())
    g2 = np.append(got[big], got[~big].sum())
    if e2[-1] < 5:
        e2, g2 = e2[:-1], g2[:-1]
    chi = float(((g2 - e2) ** 2 / e2).sum())
    assert stats.chi2.sf(chi, len(e2) - 1) > 1e-4, chi
    # the density integrates to one over the sphere (midpoint quadrature of p_e)
    grid, dw = env_ref.sphere_grid(1024, 2048)
    pg = pr.pdf(grid.astype(np.float32)).astype(np.float64)
    assert abs(float((pg * dw).sum()) - 1.0) < 0.01
    # the estimator of the probe's luminance integral
    want = float((env_ref.luminance(env_ref.lookup(rgbe, grid)) * dw).sum())
    est = float((env_ref.luminance(rad[ok].astype(np.float64)) / ps[ok]).sum() / n)
    assert est == pytest.approx(want, rel=0.01)
    pr.close()


def test_black_probe_samples_nothing(device):
    pr = lp.ProbeGPU(device, np.zeros((8, 16, 4), np.uint8), 16, 8)
    dirs, ps, rad = pr.sample(np.full((64, 6), 0.5, np.float32))
    assert not dirs.any() and not ps.any() and not rad.any()
    assert not pr.pdf(np.tile(np.array([[0, 1, 0]], np.float32), (4, 1))).any()
    pr.close()


# ---------------------------------------------------------------- 2. / 3. rendered means
def _bsdf_quadrature(rgbe, V, light_mask=None, n_theta=512, n_phi=1024):
    """outgoing radiance of the diffuse-metallic-roughness quad (roughness 1, metal 0, base ALBEDO) towards V under the probe (SPEC §10 in float64)"""
    th = (np.arange(n_theta) + 0.5) * (0.5 * np.pi) / n_theta
    ph = (np.arange(n_phi) + 0.5) * 2.0 * np.pi / n_phi - np.pi
    Tg, Pg = np.meshgrid(th, ph, indexing="ij")
    L = np.stack([np.sin(Tg) * np.cos(Pg), np.cos(Tg), np.sin(Tg) * np.sin(Pg)], axis=-1).reshape(-1, 3)
    dw = (np.sin(Tg) * (0.5 * np.pi / n_theta) * (2.0 * np.pi / n_phi)).reshape(-1)
    V = np.asarray(V, np.float64) / np.linalg.norm(V)
    NoV, NoL = max(V[1], 1e-4), L[:, 1]
    Hh = L + V
    Hh /= np.linalg.norm(Hh, axis=1, keepdims=True)
    VoH = np.maximum(Hh @ V, 0.0)
    alpha = 1.0
    D = 1.0 / np.pi   # a2 = 1
    k = alpha * 0.5
    vis = 1.0 / (4.0 * ((NoL * (1 - k) + k) * (NoV * (1 - k) + k)))
    F = 0.04 + 0.96 * (1.0 - VoH) ** 5
    f = (ALBEDO / np.pi) * (1.0 - F) + D * vis * F
    Le = env_ref.luminance(env_ref.lookup(rgbe, L))
    if light_mask is not None:
        Le = np.where(light_mask(L), 0.0, Le)
    return float((f * Le * NoL * dw).sum())


def _mean_sigma(img):
    lum = env_ref.luminance(img[..., :3].astype(np.float64)).ravel()
    return float(lum.mean()), float(lum.std(ddof=1) / np.sqrt(lum.size))


@pytest.mark.parametrize("probe_name", ["const", "sun"])
@pytest.mark.parametrize("bounces", [1, 2])
def test_quad_matches_quadrature(device, probe_name, bounces):
    rgbe = const_probe() if probe_name == "const" else sun_probe()
    V = -np.asarray(DIR, np.float64)
    want = _bsdf_quadrature(rgbe, V)
    img = render(device, quad_scene(), rgbe, 64, 64, bounces, 32, env=True)
    m, s = _mean_sigma(img)
    assert abs(m - want) <= 4 * s + 2e-4 * want, (m, want, s)
    if bounces == 2:
        off = render(device, quad_scene(), rgbe, 64, 64, bounces, 256, env=False)
        mo, so = _mean_sigma(off)
        assert abs(mo - m) <= 4 * np.hypot(s, so), (m, mo, s, so)


def test_light_plus_probe_matches_quadrature(device):
    """one rectangle light facing the quad and the sun probe at depth 2: every strategy fully MIS-weighted.  The light sits in the
    sun's direction, so the probe's samples it covers are dropped — and the light's own irradiance is added by quadrature."""
    rgbe = sun_probe()
    sun = np.array([0.35, 0.8, 0.25])
    sun /= np.linalg.norm(sun)
    c = 6.0 * sun   # the light's centre, its normal towards the quad's centre point below the camera
    n = -sun
    t = np.cross(n, [0, 0, 1.0])
    t /= np.linalg.norm(t)
    b = np.cross(n, t)
    hw, Le = 0.6, 3.0
    light = np.zeros(1, lp._abi.LIGHT_DT)
    light["normal"] = tuple(n) + (0,)
    light["tangent"] = tuple(t) + (hw,)
    light["bitangent"] = tuple(b) + (hw,)
    light["origin"] = tuple(c) + (Le,)
    P = np.zeros(3)

    def covers(L):   # directions from P that hit the light's front
        dn = L @ n
        tt = np.where(dn < 0, (c - P) @ n / np.where(dn < 0, dn, -1.0), -1.0)
        hit = P[None] + L * tt[:, None] - c[None]
        return (dn < 0) & (tt > 0) & (np.abs(hit @ t) <= hw) & (np.abs(hit @ b) <= hw)

    V = -np.asarray(DIR, np.float64)
    V /= np.linalg.norm(V)
    want_env = _bsdf_quadrature(rgbe, V, light_mask=covers)
    # the light's part: the same BSDF quadrature with Le inside the light's solid angle (luminance of a white emitter = Le)
    want_light = _bsdf_quadrature(const_probe(1.0), V, light_mask=lambda L: ~covers(L)) * Le
    img = render(device, quad_scene(light), rgbe, 64, 64, 2, 64, env=True, vfov=0.01)
    m, s = _mean_sigma(img)
    want = want_env + want_light
    assert abs(m - want) <= 4 * s + 1e-3 * want, (m, want_env, want_light, s)


# ---------------------------------------------------------------- 4. variance
def test_variance_drops_on_the_sun_probe(device):
    rgbe = sun_probe()
    on = render(device, quad_scene(), rgbe, 64, 64, 2, 8, env=True)
    off = render(device, quad_scene(), rgbe, 64, 64, 2, 8, env=False)
    v_on = env_ref.luminance(on[..., :3].astype(np.float64)).var()
    v_off = env_ref.luminance(off[..., :3].astype(np.float64)).var()
    print("per-pixel variance at 8 spp: on %.4g off %.4g ratio %.4g" % (v_on, v_off, v_on / v_off))
    # the issue's expectation was 0.1 (from the sun's solid angle); measured on an MI355X: 0.185 (the 64 x 32 probe spreads the sun over a
    # 5.6-degree cell and the sky's gradient stays).  The bar: the measured ratio with a third of margin
    assert v_on <= 0.25 * v_off


# ---------------------------------------------------------------- 5. bit-identity inside the mode
@pytest.fixture(scope="module")
def atrium_small():
    desc = scenes.synthetic_atrium(texture_size=128)
    desc["probe"] = scenes.sky_probe(128, 64)
    return desc


def _atrium(device, desc, env, **kw):
    w, h, bounces, frames = 96, 64, 4, 2
    return render(device, scenes.to_product(desc), desc["probe"], w, h, bounces, frames, env, eye=desc["camera"]["origin"],
                  direction=desc["camera"]["direction"], vfov=T.VFOV, **kw)


PATH = {"path_rays": 0x7FFFFFFF, "packet_primary": 1, "coop_rays": 0}
PER_BOUNCE = {"path_rays": 0, "step_budget": 16, "tail_lanes": 0, "coop_rays": 0}


def test_atrium_bit_identical_inside_the_mode(device, atrium_small):
    desc = atrium_small
    ref = _atrium(device, desc, True, options=PER_BOUNCE)
    off = _atrium(device, desc, False, options=PER_BOUNCE)
    assert np.all(np.isfinite(ref)) and ref.tobytes() != off.tobytes()
    assert _atrium(device, desc, True, options=PER_BOUNCE).tobytes() == ref.tobytes()          # run to run
    assert _atrium(device, desc, True, options=PATH).tobytes() == ref.tobytes()                # k_path
    assert _atrium(device, desc, True, options=dict(PER_BOUNCE, packet_primary=0)).tobytes() == ref.tobytes()
    assert _atrium(device, desc, True, options=PER_BOUNCE, lanes=2).tobytes() == ref.tobytes()
    assert _atrium(device, desc, True, options=PATH, lanes=2).tobytes() == ref.tobytes()
    acc = np.zeros_like(ref)
    for rank in range(2):
        acc += _atrium(device, desc, True, options=PATH, world=2, rank=rank)
    assert acc.tobytes() == ref.tobytes()


# ---------------------------------------------------------------- 6. off means off
def test_off_means_off(device, atrium_small):
    desc = atrium_small
    off = _atrium(device, desc, False, options=PATH)
    assert _atrium(device, desc, False, options=PATH, toggle=True).tobytes() == off.tobytes()
    black = dict(desc, probe=np.zeros((8, 16, 4), np.uint8))
    assert _atrium(device, black, True, options=PATH).tobytes() == _atrium(device, black, False, options=PATH).tobytes()
    # the bound probe destroyed while the mode is on: the renderer falls back to the black default probe, no fault
    gone_on = _atrium(device, desc, True, options=PATH, destroy_probe=True)
    gone_off = _atrium(device, desc, False, options=PATH, destroy_probe=True)
    assert gone_on.tobytes() == gone_off.tobytes()
