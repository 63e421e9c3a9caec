"""-m gpu: the thin-lens camera (SPEC.md §25) on the device.  The renderer's own ray generation (lpt_renderer_primary_rays: k_raygen compacted at 61x37, dense at
64x32) against the binary64 restatement of tests/lens_ref.py; a closed lens is the renderer that never heard of one, bit for bit; an open lens gives one frame
however it is launched or sharded; a plane in focus renders as the pinhole renders it; a small emitter out of focus spreads over the stated disc and keeps its
energy; invalid arguments change nothing.  Tolerances, the board's edge distance and the spot's numbers are lens_ref's, derived there and not from a run."""
import math

import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import _abi as A, api, testing as T

import lens_ref as L
import primary_ref as P
from conftest import PIPELINES
from test_gpu_env_sampling import _dark_light
from test_gpu_transmission import QUAD_IDX

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("pipeline")]

BLACK = np.zeros((1, 1, 4), np.uint8)          # RGBE 0: a black probe
DEPTH = 4
VIEWS = [P.view_matrix(o, fw, roll) for o, fw, roll in L.RAY_VIEWS]
OPEN = (0.15, 5.5)                              # a lens that blurs the reference scene visibly: its surfaces lie 6 to 8 units away


@pytest.fixture(scope="module")
def world(device):
    scene = lp.Scene()
    P.build_scene(scene, scene.add_image, lambda l: scene.set_light(0, P.light_record(A.LIGHT_DT)))
    sg = lp.SceneGPU.new_from_scene(scene, device)
    pr = lp.ProbeGPU(device, np.array([[[64, 64, 64, 128]]], np.uint8), 1, 1)
    yield sg, pr
    pr.close()
    sg.close()


def make(device, sg, pr, size, depth=DEPTH, vfov=L.RAY_VFOV, mode=None, lens=None, rank=0, n_ranks=1, seed=L.USER_SEED, noise=False, timings=False):
    r = lp.Renderer(device, size)
    r.downsample_factor = 1.0
    r.resize(device, sg, pr, size)
    r.set_max_bounces(depth)
    r.set_vfov(vfov)
    r.set_seed(seed)
    if noise:
        nz = P.noise_texture()
        r.upload_noise_texture(nz, nz.shape[1], nz.shape[0], nz.shape[1] * 4)
        r.use_noise_texture(True)
    if n_ranks > 1:
        r.set_shard(rank, n_ranks)
        r.set_resources(device, sg, pr)
    if mode is not None:
        r.set_blit_mode(mode)
    if lens is not None:
        r.set_lens(*lens)
    if timings:
        r.enable_timings(True)
    r.reset_accumulation()
    return r


def bits(a):
    return np.ascontiguousarray(a).tobytes()


# ---------------------------------------------------------------- 1. rays against the reference
@pytest.mark.parametrize("size", P.SIZES, ids=lambda s: "%dx%d" % s)
def test_primary_rays_match_the_float64_reference(device, world, size):
    sg, pr = world
    w, h = size
    worst = {"origin": 0.0, "direction": 0.0, "|off| - R": 0.0, "off . fwd": 0.0, "focus": 0.0}
    lines = []
    for noise in (False, True):
        r = make(device, sg, pr, size, noise=noise)
        try:
            for vi, view in enumerate(VIEWS):
                r.raytrace(view)                                        # the seed state moves between the views
                fc, seed = r.frame_state()
                for R, Fd in L.RAY_LENSES:
                    r.set_lens(R, Fd)
                    assert r.lens == (float(np.float32(R)), float(np.float32(Fd)))
                    for sample in L.RAY_SAMPLES:
                        o, d = r.primary_rays(view, sample)
                        assert r.frame_state() == (fc, seed)            # the hook leaves the frame state alone
                        o, d = o.reshape(-1, 3).astype(np.float64), d.reshape(-1, 3).astype(np.float64)
                        ref = L.primary_rays(view, w, h, L.RAY_VFOV, R, Fd, L.USER_SEED, seed + sample * DEPTH, P.noise_texture() if noise else None)
                        assert np.max(np.abs(ref.cx)) <= 1.5 and np.max(np.abs(ref.cy)) <= 1.5      # what the tolerances assume
                        e = {}
                        e["origin"] = float(np.max(np.abs(o - ref.o) / L.tol_origin(R, ref.o)))
                        e["direction"] = float(np.max(np.abs(d - ref.d)) / L.tol_direction(R, Fd))
                        o_max = float(np.max(np.abs(ref.o)))
                        slack = math.sqrt(3.0) * float(np.max(L.tol_origin(R, o_max)))
                        off = o - ref.cam.origin[None]
                        e["|off| - R"] = float(np.max(np.linalg.norm(off, axis=1) - R) / slack)
                        e["off . fwd"] = float(np.max(np.abs(off @ ref.cam.fwd)) / L.tol_perpendicular(ref.cam, R, o_max))
                        dist = np.linalg.norm(np.cross(ref.focus - o, d), axis=1) / np.linalg.norm(d, axis=1)
                        e["focus"] = float(np.max(dist) / L.tol_focus(R, Fd, o_max, float(np.max(np.linalg.norm(ref.dir, axis=1)))))
                        assert np.linalg.norm(off, axis=1).max() > 0.9 * R  # the lens is used to its rim
                        for k, v in e.items():
                            worst[k] = max(worst[k], v)
                        lines.append("%dx%d noise %d view %d R %g F %g sample %d: error / tolerance %s" % (w, h, noise, vi, R, Fd, sample, {k: "%.3g" % v for k, v in e.items()}))
        finally:
            r.close()
    print("\n".join(lines))
    print("largest error / tolerance: %s" % {k: "%.3g" % v for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


# ---------------------------------------------------------------- 2. a closed lens is today's renderer
def frames(device, sg, pr, size, lens, timings=False, n_ranks=1):
    """radiance of two accumulated path-traced frames, and G-buffer / motion / filtered radiance of a DenoisedPathrace frame behind a camera move; the ranks' buffers
    summed (they are zero outside a rank's tiles: SPEC §13, §15.5) -> ({name: array}, {stage: launches} of the path-traced renderer)"""
    out, launches = {}, {}
    for rank in range(n_ranks):
        r = make(device, sg, pr, size, lens=lens, rank=rank, n_ranks=n_ranks, timings=timings)
        r.accumulate = True
        r.raytrace(VIEWS[0])
        r.raytrace(VIEWS[0])
        part = {"radiance": r.read_radiance()}
        if timings:
            launches = {k: v[1] for k, v in r.timings().items()}
        r.close()
        r = make(device, sg, pr, size, lens=lens, rank=rank, n_ranks=n_ranks, mode=lp.BlitMode.DenoisedPathrace)
        r.raytrace(VIEWS[0])
        r.raytrace(VIEWS[1])
        g, m, rad, _ = r.read_denoiser()
        part.update({"gbuffer": g, "motion": m})
        if n_ranks == 1:
            part["denoised"] = rad
        r.close()
        for k, v in part.items():
            out[k] = v if k not in out else out[k] + v
    return out, launches


@pytest.mark.parametrize("size", P.SIZES, ids=lambda s: "%dx%d" % s)
def test_a_closed_lens_is_the_renderer_without_one(device, world, size, monkeypatch):
    sg, pr = world
    for arm, options in PIPELINES.items():                              # all three arms here, whichever the fixture picked (it skips `default` outside the full-size modules)
        monkeypatch.setattr(api, "DEFAULT_OPTIONS", dict(options))
        want, launches = frames(device, sg, pr, size, None, timings=True)
        assert want["radiance"][..., :3].max() > 0.05 and np.any(want["motion"] != 0)
        for lens in ((0.0, 1.0), (0.0, 0.25), (0.0, 77.0)):
            got, l2 = frames(device, sg, pr, size, lens, timings=True)
            for k in want:
                assert bits(got[k]) == bits(want[k]), (arm, lens, k)
            assert l2 == launches, (arm, lens, l2, launches)            # and the same launches
    view = VIEWS[1]
    a, b = make(device, sg, pr, size), make(device, sg, pr, size, lens=(0.0, 3.5))
    try:
        (oa, da), (ob, db) = a.primary_rays(view, 2), b.primary_rays(view, 2)
        assert bits(oa) == bits(ob) and bits(da) == bits(db)
        assert np.all(oa.reshape(-1, 3) == np.asarray(view, np.float32)[12:15][None])       # the shared origin, as it was given
        ref = L.primary_rays(view, size[0], size[1], L.RAY_VFOV, 0.0, 1.0, L.USER_SEED, a.frame_state()[1] + 2 * DEPTH)
        err = float(np.max(np.abs(da.reshape(-1, 3) - ref.d)) / L.tol_direction(0.0, 1.0))
        print("closed lens, direction error / tolerance %.3g" % err)
        assert err <= 1.0
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- 3. the arms agree with the lens open
@pytest.mark.parametrize("size", P.SIZES, ids=lambda s: "%dx%d" % s)
def test_an_open_lens_gives_one_frame_however_it_is_launched(device, world, size, monkeypatch):
    sg, pr = world
    got = {}
    for arm, options in PIPELINES.items():
        monkeypatch.setattr(api, "DEFAULT_OPTIONS", dict(options))
        got[arm], launches = frames(device, sg, pr, size, OPEN, timings=True)
        assert launches["path"] == 0 and launches["primary intersection"] == 0, (arm, launches)     # the plan keeps a lens frame off k_path and the packets
        assert launches["ray generation"] > 0 and launches["shading"] > 0 and launches["intersection"] > 0
        if arm == "path":                                               # ... which this arm does take with the lens closed
            _, pin = frames(device, sg, pr, size, None, timings=True)
            assert pin["path"] > 0 and pin["primary intersection"] > 0, pin
    pinhole, _ = frames(device, sg, pr, size, None)
    assert bits(got["default"]["radiance"]) != bits(pinhole["radiance"]) and bits(got["default"]["gbuffer"]) != bits(pinhole["gbuffer"])
    for arm in PIPELINES:
        for k in got["default"]:
            assert bits(got[arm][k]) == bits(got["default"][k]), (arm, k)
    sharded, _ = frames(device, sg, pr, size, OPEN, n_ranks=3)
    for k in sharded:
        assert bits(sharded[k]) == bits(got["default"][k]), ("three ranks", k)


# ---------------------------------------------------------------- 4. a plane in focus renders as the pinhole renders it
def board_scene(size):
    """the checkerboard of lens_ref: one mesh per parity, two triangles per cell, the diagonal from the cell's low corner; black base, two emissive materials"""
    s = lp.Scene()
    s.set_light(0, _dark_light())
    nx, ny = L.board_cells(*size)
    c, z = L.BOARD_CELL, -L.BOARD_F
    for parity in (0, 1):
        m = s.add_material((0.0, 0.0, 0.0, 1.0), 1.0, 0.0)
        s.set_material_emission(m, L.BOARD_LE[parity])
        pos, idx = [], []
        for j in range(-ny, ny):
            for i in range(-nx, nx):
                if (i + j) & 1 != parity:
                    continue
                idx += list(QUAD_IDX + len(pos))
                pos += [(i * c, j * c, z), ((i + 1) * c, j * c, z), ((i + 1) * c, (j + 1) * c, z), (i * c, (j + 1) * c, z)]
        pos = np.array(pos, np.float32)
        nrm = np.tile(np.array([[0, 0, 1]], np.float32), (len(pos), 1))
        blas = s.add_mesh(pos, nrm, np.zeros((len(pos), 2), np.float32), np.array(idx, np.uint32))
        s.add_instance(blas, np.eye(4, dtype=np.float32), m)
    return s


@pytest.mark.parametrize("size", P.SIZES, ids=lambda s: "%dx%d" % s)
def test_a_plane_in_focus_renders_as_the_pinhole_renders_it(device, size):
    w, h = size
    view = T.look(L.BOARD_EYE, L.BOARD_DIR)
    sg = lp.SceneGPU.new_from_scene(board_scene(size), device)
    pr = lp.ProbeGPU(device, BLACK, 1, 1)
    out = {}
    try:
        for name, lens in (("pinhole", None), ("lens", (L.BOARD_R, L.BOARD_F))):
            r = make(device, sg, pr, size, depth=1, vfov=L.BOARD_VFOV, lens=lens)
            assert r.frame_state()[1] == 0                              # the same seed for both
            r.raytrace(view)
            rad = r.read_radiance()[..., :3].reshape(-1, 3)
            r.close()
            r = make(device, sg, pr, size, depth=1, vfov=L.BOARD_VFOV, lens=lens, mode=lp.BlitMode.DenoisedPathrace)
            r.raytrace(view)
            g = r.read_denoiser()[0].reshape(-1, 4)
            r.close()
            out[name] = (rad, g[:, 0], g[:, 1].copy().view(np.float32))
    finally:
        pr.close()
        sg.close()
    parity, tri, _, _, cmp, ref = L.board_reference(view, w, h, L.USER_SEED, 0)
    left = 1.0 - float(np.mean(cmp))
    print("%dx%d: %.3f %% of the pixels left out (within %.3g of an edge)" % (w, h, 100.0 * left, L.board_edge_eps()))
    assert left <= 0.01
    (rad_p, prim_p, t_p), (rad_l, prim_l, t_l) = out["pinhole"], out["lens"]
    assert np.all(prim_p != P.INVALID) and np.all(prim_l != P.INVALID)       # the board fills the frame
    assert np.array_equal(prim_l[cmp], prim_p[cmp]) and bits(rad_l[cmp]) == bits(rad_p[cmp])
    le = np.asarray(L.BOARD_LE, np.float32)[parity]
    assert bits(rad_p[cmp]) == bits(le[cmp])                            # ... and both are the material the reference's focal point falls on
    assert len(np.unique(prim_p[cmp] & 1)) == 2 and np.array_equal(prim_p[cmp] & 1, tri[cmp].astype(np.uint32))      # the triangle of the cell's quad, too
    assert not np.array_equal(t_l, t_p)                                 # the lens rays are other rays: the depths along them differ


# ---------------------------------------------------------------- 5. out of focus blurs by the stated disc
def test_out_of_focus_blurs_by_the_stated_disc_and_keeps_the_energy(device):
    half, rho, half_diag, centre, hits = L.spot_numbers()
    s = lp.Scene()
    s.set_light(0, _dark_light())
    m = s.add_material((0.0, 0.0, 0.0, 1.0), 1.0, 0.0)
    s.set_material_emission(m, L.SPOT_LE)
    z = -L.SPOT_Z
    pos = np.array([(-half, -half, z), (half, -half, z), (half, half, z), (-half, half, z)], np.float32)
    blas = s.add_mesh(pos, np.tile(np.array([[0, 0, 1]], np.float32), (4, 1)), np.zeros((4, 2), np.float32), QUAD_IDX)
    s.add_instance(blas, np.eye(4, dtype=np.float32), m)
    sg = lp.SceneGPU.new_from_scene(s, device)
    pr = lp.ProbeGPU(device, BLACK, 1, 1)
    view = T.look((0.0, 0.0, 0.0), (0.0, 0.0, -1.0))
    img = {}
    try:
        for name, lens in (("pinhole", None), ("lens", (L.SPOT_R, L.SPOT_F))):
            r = make(device, sg, pr, (L.SPOT_W, L.SPOT_H), depth=1, vfov=L.SPOT_VFOV, lens=lens)
            r.accumulate = True
            for _ in range(L.SPOT_SAMPLES // 64):
                r.raytrace_n(view, 64)
            img[name] = r.read_radiance()[..., :3].astype(np.float64)
            r.close()
    finally:
        pr.close()
        sg.close()
    y, x = np.mgrid[0:L.SPOT_H, 0:L.SPOT_W]
    dist = np.hypot(x + 0.5 - centre[0], y + 0.5 - centre[1])
    le = np.asarray(L.SPOT_LE, np.float64)
    sigma = math.sqrt(hits)                                             # a sum of independent hits of mean `hits`: its variance is at most its mean
    for name in ("pinhole", "lens"):
        lit = np.any(img[name] != 0.0, axis=-1)
        reach = (rho if name == "lens" else 0.0) + half_diag + 1.0
        count = img[name].sum(axis=(0, 1)) * L.SPOT_SAMPLES / le         # the frame is the mean over the samples: per channel, the number of hits
        print("%s: %d lit pixels, farthest %.2f px (allowed %.2f), hits %s (expected %.0f, 5 sigma %.0f)" % (name, lit.sum(), dist[lit].max(), reach, np.round(count, 2), hits, 5 * sigma))
        assert lit.any() and dist[lit].max() <= reach
        assert np.allclose(count, count[0], rtol=1e-5) and abs(count[0] - hits) <= 5.0 * sigma
    lit = np.any(img["lens"] != 0.0, axis=-1)
    assert dist[lit].max() > 0.5 * rho and lit.sum() > 0.5 * math.pi * rho * rho     # the disc fills


# ---------------------------------------------------------------- 6. invalid arguments
BAD = [(-1.0, 1.0), (-1e-30, 1.0), (float("nan"), 1.0), (float("inf"), 1.0), (0.1, 0.0), (0.1, -2.0), (0.1, float("nan")), (0.1, float("inf")), (0.1, -float("inf"))]


@pytest.mark.parametrize("before", [None, OPEN], ids=["default", "open"])
def test_invalid_arguments_change_nothing(device, world, before):
    sg, pr = world
    size = P.SIZES[0]
    a, b = make(device, sg, pr, size, lens=before), make(device, sg, pr, size, lens=before)
    try:
        assert a.lens == ((0.0, 1.0) if before is None else tuple(float(np.float32(v)) for v in before))
        for bad in BAD:
            with pytest.raises(lp.Error) as e:
                a.set_lens(*bad)
            assert e.value.kind == "InvalidArg" and "lpt_renderer_set_lens" in str(e.value)
            assert a.lens == b.lens
        with pytest.raises(lp.Error) as e:
            a.primary_rays(VIEWS[0], 64)
        assert e.value.kind == "InvalidArg"
        for r in (a, b):
            r.raytrace(VIEWS[0])
        assert a.frame_state() == b.frame_state() and bits(a.read_radiance()) == bits(b.read_radiance())
    finally:
        a.close()
        b.close()
