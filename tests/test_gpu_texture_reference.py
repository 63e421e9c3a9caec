"""-m gpu: what a hit reads from its textures (SPEC §9, §20; `texture_lookup` over the 8x4-tiled atlas, `texture_lookup_pair` over the apron tiles, `alpha_rejects`' own copy
of the addressing) and the environment lookup (`env_lookup`), through the device probes `SceneGPU.sample_textures` and `ProbeGPU.lookup`, against the binary64 reference
tests/texture_ref.py and against the oracle's lookups bit for bit.  Every image size of the reference, each way an image can be stored: alone in the atlas as albedo, mra,
emissive image, normal map and mask; as a pair; as half of a pair that other materials also sample alone.  Coordinates are placed exactly by CARRIER triangles: a small
triangle whose three vertices carry three wanted coordinates, probed at the barycentrics (0, 0), (1, 0), (0, 1), where §12's interpolation returns the vertex's own value
(the weight of the other two is an exact 0); a few hundred ordinary triangles with spread uv and interior barycentrics exercise the interpolation itself.
Every bound is texture_ref's (derived; none measured).  The tests print their reports: run with -s.

Measured on an MI355X, worst |error| / bound (limit 1), images alone in the atlas (the worst of albedo, mra, emissive, normal map) / as a pair (resident halves or not: the
same figure): 1x1 0 / 0, 1x7 0.64 / 0.64, 7x1 0.64 / 0.64, 2x2 0.29 / 0.27, 3x3 0.50 / 0.50, 4x4 0.40 / 0.40, 5x3 0.50 / 0.50, 8x4 0.52 / 0.52, 9x5 0.50 / 0.50,
16x16 0.71 / 0.63, 23x17 0.61 / 0.61, 64x64 0.85 / 0.81; the interpolated coordinate 0.42; beyond int32 0.06 (the one axis that is not pinned); probes 2x1 0.67, 1x2 0.66,
2x2 0.42, 5x3 0.46, 8x4 0.52, 16x8 0.56.  Every row equals the oracle's bit for bit, pairing on, off and gpu_build answer the same bytes, and both frame pins are bit-equal."""
import numpy as np
import pytest

import texture_ref as R
import test_texture_reference as CPU
import loupiote_amd as lp

pytestmark = pytest.mark.gpu
F = np.float32
IDENTITY = np.eye(4, dtype=F).reshape(16)
N_ORDINARY = 300
CUTOFF = 0.5


def dark_light():
    l = np.zeros(1, lp._abi.LIGHT_DT)
    l["normal"], l["tangent"], l["bitangent"], l["origin"] = (0, 0, 1, 0), (1, 0, 0, 0.5), (0, 1, 0, 0.5), (0, 0, -50.0, 0.0)
    return l


def carrier_mesh(tu, tv, per_triangle=3):
    """carriers of the coordinates (tu, tv) on a grid in z = 0, `per_triangle` coordinates each (1: vertex 0 carries it, the others 0), then N_ORDINARY ordinary triangles
    -> (mesh, probes {prim, bary} of the carriers in the order of (tu, tv), probes of the ordinary triangles with their vertex uv)"""
    n = len(tu)
    nt = -(-n // per_triangle)
    uv = np.zeros((nt * 3, 2), F)
    slot = np.arange(n) // per_triangle * 3 + np.arange(n) % per_triangle
    uv[slot, 0], uv[slot, 1] = tu, tv
    rs = np.random.RandomState(11)
    ord_uv = rs.uniform(-3, 4, (N_ORDINARY * 3, 2)).astype(F)
    uv = np.concatenate([uv, ord_uv])
    t = np.arange(nt + N_ORDINARY)
    side = int(np.ceil(np.sqrt(len(t))))
    corner = np.stack([(t % side).astype(F), (t // side).astype(F), np.zeros(len(t), F)], axis=1)
    pos = (corner[:, None, :] + np.array([(0, 0, 0), (0.5, 0, 0), (0, 0.5, 0)], F)[None]).reshape(-1, 3)
    nrm = np.tile(F([0, 0, 1]), (len(pos), 1))
    bary = np.array([(0, 0), (1, 0), (0, 1)], F)[np.arange(n) % per_triangle]
    hu = rs.uniform(0.05, 0.9, N_ORDINARY).astype(F)
    hv = (rs.uniform(0.05, 0.95, N_ORDINARY) * (1 - hu)).astype(F)
    mesh = {"pos": pos, "nrm": nrm, "uv": uv, "tris": nt + N_ORDINARY}
    return mesh, {"prim": (np.arange(n) // per_triangle).astype(np.uint32), "bary": bary}, \
        {"prim": (nt + np.arange(N_ORDINARY)).astype(np.uint32), "bary": np.stack([hu, hv], axis=1), "uv": ord_uv.reshape(N_ORDINARY, 3, 2)}


ROLES = ("alone-a", "alone-b", "pair-resident", "pair-only")


def build_scene(W, H, mesh):
    """four instances of the mesh, one per material:
    alone-a        image 0 alone in the atlas as albedo, as emissive image and as mask (color.w 1); image 1 alone as normal map
    alone-b        image 1 alone in the atlas as mra, as emissive image and as mask (color.w 0.7)
    pair-resident  (image 0, image 1) as a pair whose halves the two materials above also sample alone
    pair-only      (image 2, image 3) — copies of images 0 and 1 — as a pair and nothing else: they live in the pair's texels only"""
    s = lp.Scene()
    s.set_light(0, dark_light())
    im = [s.add_image(R.image(W, H, k % 2)) for k in range(4)]
    a = s.add_material((1.0, 1.0, 1.0, 1.0), 1.0, 1.0, albedo_texture=im[0])
    s.set_material_emission(a, (1.0, 1.0, 1.0), 1.0, im[0])
    s.set_material_normal_map(a, im[1], 1.0)
    s.set_material_alpha(a, "MASK", CUTOFF, im[0])
    b = s.add_material((1.0, 1.0, 1.0, 0.7), 1.0, 1.0, mra_texture=im[1])
    s.set_material_emission(b, (1.0, 1.0, 1.0), 1.0, im[1])
    s.set_material_alpha(b, "MASK", CUTOFF, im[1])
    c = s.add_material((1.0, 1.0, 1.0, 1.0), 1.0, 1.0, albedo_texture=im[0], mra_texture=im[1])
    d = s.add_material((1.0, 1.0, 1.0, 1.0), 1.0, 1.0, albedo_texture=im[2], mra_texture=im[3])
    blas = s.add_mesh(mesh["pos"], mesh["nrm"], mesh["uv"])
    for m in (a, b, c, d):
        s.add_instance(blas, IDENTITY, m)
    return s


def probe_roles(sg, mesh, q):
    """sample_textures of the probes q under each of the four instances -> {role: outputs}"""
    return {role: sg.sample_textures(q["prim"] + np.uint32(k * mesh["tris"]), q["bary"]) for k, role in enumerate(ROLES)}


def as_bytes(out):
    return b"".join(out[r][k].tobytes() for r in ROLES for k in ("albedo", "mra", "emissive", "normal", "rejected", "uv"))


def resident_bytes(W, H, plain, pairs):
    return plain * (-(-W // 8)) * (-(-H // 4)) * 128 + pairs * (-(-W // 3)) * (-(-H // 3)) * 128


def check_rows(W, H, tu, tv, out, rep):
    """the four roles' outputs at the coordinates (tu, tv) against the reference and the oracle"""
    i0, i1 = R.image(W, H, 0), R.image(W, H, 1)
    ref = {"srgb0": R.lookup(i0, tu, tv, True), "lin1": R.lookup(i1, tu, tv, False), "srgb1": R.lookup(i1, tu, tv, True), "pair": R.pair(i0, i1, tu, tv)}
    orc = {"srgb0": CPU.oracle_lookup(W, H, 0, tu, tv, True), "lin0": CPU.oracle_lookup(W, H, 0, tu, tv, False), "lin1": CPU.oracle_lookup(W, H, 1, tu, tv, False),
           "srgb1": CPU.oracle_lookup(W, H, 1, tu, tv, True)}
    one3, zero3 = np.ones((len(tu), 3), F), np.zeros((len(tu), 3), F)

    def held(what, got, key, cols):
        val, bound, exact = ref[key]
        r = R.ratios(val[:, cols], bound[:, cols], got)
        rep[what] = max(rep.get(what, 0.0), float(r.max()))
        assert np.all(r <= 1.0), (W, H, what, float(r.max()), int(np.argmax(r.max(axis=1))))
        assert np.array_equal(got[exact], val[exact][:, cols].astype(F)), (W, H, what, "an exact row is the tap itself")
        assert got.tobytes() == np.ascontiguousarray(orc[key][:, cols]).tobytes(), (W, H, what, "the oracle's lookup, bit for bit")

    a, b = out["alone-a"], out["alone-b"]
    held("atlas albedo", a["albedo"], "srgb0", [0, 1, 2])
    held("atlas emissive", a["emissive"], "srgb0", [0, 1, 2])
    held("atlas normal", a["normal"], "lin1", [0, 1, 2])
    held("atlas mra", b["mra"], "lin1", [1, 2])
    held("atlas emissive", b["emissive"], "srgb1", [0, 1, 2])
    assert np.array_equal(a["mra"], one3[:, :2]) and np.array_equal(b["albedo"], one3) and np.array_equal(b["normal"], zero3)
    for role in ("pair-resident", "pair-only"):
        o = out[role]
        got = np.concatenate([o["albedo"], o["mra"]], axis=1)
        val, bound, exact = ref["pair"]
        r = R.ratios(val, bound, got)
        rep[role] = max(rep.get(role, 0.0), float(r.max()))
        assert np.all(r <= 1.0), (W, H, role, float(r.max()), int(np.argmax(r.max(axis=1))))
        assert np.array_equal(got[exact], val[exact].astype(F))
        assert got.tobytes() == np.concatenate([orc["srgb0"][:, :3], orc["lin1"][:, 1:3]], axis=1).tobytes(), (W, H, role)
        assert np.array_equal(o["emissive"], one3) and np.array_equal(o["normal"], zero3) and not o["rejected"].any()
    # §20: the reference's decision outside the band it leaves out, and on EVERY row the decision of texture_lookup's own alpha (the mask's copy must not drift from it)
    for o, k, cw, lin in ((a, 0, 1.0, orc["lin0"]), (b, 1, 0.7, orc["lin1"])):
        al, ab = R.alpha(R.image(W, H, k), cw, tu, tv)
        keep = R.mask_compared(al, ab, CUTOFF)
        assert np.array_equal(o["rejected"][keep], al[keep] < CUTOFF), (W, H, cw)
        assert np.array_equal(o["rejected"], ~((F(cw) * lin[:, 3]).astype(F) >= F(CUTOFF))), (W, H, cw)
        rep["mask rows left out"] = rep.get("mask rows left out", 0) + int((~keep).sum())


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: "%dx%d" % s)
def test_every_storage_path_against_float64_and_the_oracle(device, size):
    """within the bound, bit-equal on the exact rows, bit-equal to the oracle; pair_textures on / off and gpu_build answer the same bytes; the stats count the tiles"""
    W, H = size
    tu, tv = R.coords(W, H)
    mesh, q, qo = carrier_mesh(tu, tv)
    scene = build_scene(W, H, mesh)
    first, rep = None, {}
    for name, kw in (("paired", {}), ("unpaired", {"pair_textures": False}), ("gpu_build", {"gpu_build": True})):
        sg = lp.SceneGPU.new_from_scene(scene, device, **kw)
        st = sg.stats()
        out, ordinary = probe_roles(sg, mesh, q), probe_roles(sg, mesh, qo)
        sg.close()
        assert st.triangles == 4 * mesh["tris"]
        if name == "unpaired":
            assert (st.texture_pairs, st.texture_bytes_resident) == (0, resident_bytes(W, H, 4, 0))
        else:
            assert (st.texture_pairs, st.texture_bytes_resident) == (2, resident_bytes(W, H, 2, 2))
        got = as_bytes(out) + as_bytes(ordinary)
        first = first or got
        assert got == first, "%s differs from the paired upload" % name
        if name != "paired":
            continue
        for role in ROLES:      # a carrier returns its vertex' coordinate itself
            assert np.array_equal(out[role]["uv"], np.stack([tu, tv], axis=1)), role
        check_rows(W, H, tu, tv, out, rep)
        # the ordinary triangles: §12's interpolation within its bound, and every lookup at the coordinate the device reports
        uv, ub = R.interpolate(qo["uv"][:, 0], qo["uv"][:, 1], qo["uv"][:, 2], qo["bary"][:, 0], qo["bary"][:, 1])
        got_uv = ordinary["alone-a"]["uv"]
        assert R.passes(uv, ub, got_uv) and all(np.array_equal(ordinary[r]["uv"], got_uv) for r in ROLES)
        rep["interpolated uv"] = float(R.ratios(uv, ub, got_uv).max())
        check_rows(W, H, got_uv[:, 0].copy(), got_uv[:, 1].copy(), ordinary, rep)
    print("\ndevice %dx%d, %d rows + %d interpolated: worst |error| / bound (must stay at or below 1) %s" % (W, H, len(tu), N_ORDINARY, "  ".join("%s %.3f" % kv for kv in rep.items())))


@pytest.mark.parametrize("size", R.OUTSIDE_SIZES, ids=lambda s: "%dx%d" % s)
def test_beyond_int32_the_saturation_rule_decides(device, size):
    """|t·size| from 2^31 to LPT_UV_MAX (SPEC §9: x0 = wrap(sat(floor(fx))), the texel after it for x1): every output is finite, lies within [min, max] of the image's
    channel values, equals the oracle's bit for bit, and is the texel the rule names.  (Every index goes through wrap, which keeps it inside the image: kernels.h
    texture_lookup, texture_lookup_pair and alpha_rejects compute x0 = wrap_i((int)x0f, W) and x1 = wrap_next(x0, W) and index with nothing else.)  What no mesh may
    carry — NaN, infinities, beyond LPT_UV_MAX — never reaches a kernel: tests/test_abi.py."""
    W, H = size
    tu, tv = R.outside(W, H)
    mesh, q, _ = carrier_mesh(tu, tv, per_triangle=1)
    scene = build_scene(W, H, mesh)
    first = None
    for kw in ({}, {"pair_textures": False}):
        sg = lp.SceneGPU.new_from_scene(scene, device, **kw)
        out = probe_roles(sg, mesh, q)
        sg.close()
        first = first or as_bytes(out)
        assert as_bytes(out) == first
    rep = {}
    check_rows(W, H, tu, tv, out, rep)
    for role, key, k, srgb, cols in (("alone-a", "albedo", 0, True, [0, 1, 2]), ("alone-a", "normal", 1, False, [0, 1, 2]), ("alone-b", "mra", 1, False, [1, 2]),
                                     ("pair-only", "albedo", 0, True, [0, 1, 2]), ("pair-only", "mra", 1, False, [1, 2]), ("pair-resident", "albedo", 0, True, [0, 1, 2])):
        vals = R.texel_values(R.image(W, H, k), srgb).reshape(-1, 4)[:, cols]
        got = out[role][key]
        assert np.all(np.isfinite(got)) and np.all(got >= vals.min(axis=0).astype(F)) and np.all(got <= vals.max(axis=0).astype(F)), (role, key)
    print("\ndevice %dx%d beyond int32: %d rows, worst |error| / bound %s" % (W, H, len(tu), "  ".join("%s %.3f" % kv for kv in rep.items())))


# ------------------------------------------------------------------ the environment lookup
@pytest.mark.parametrize("size", R.PROBES, ids=lambda s: "%dx%d" % s)
def test_probe_lookup_against_float64_and_the_oracle(device, size):
    W, H = size
    rgbe = R.probe(W, H)
    pr = lp.ProbeGPU(device, rgbe, W, H)
    rep = {}
    sets = R.directions(W, H)
    for name, d in sets.items():
        got = pr.lookup(d)
        val, bound = R.env(rgbe, d)
        r = R.ratios(val, bound, got)
        rep[name] = float(r.max())
        assert np.all(r <= 1.0), (size, name, float(r.max()), int(np.argmax(r.max(axis=1))))
        assert got.tobytes() == CPU.oracle_env(rgbe, d).tobytes(), (size, name, "the oracle's lookup, bit for bit")
    # the poles: u = 1/2 whatever the signs of the zeros — the reference's value there, and one value per pole
    poles = pr.lookup(sets["poles"])
    up = R.env(rgbe, np.array([(0, 1, 0)], F))
    assert R.passes(np.repeat(up[0], 3, axis=0), np.repeat(up[1], 3, axis=0), poles[[0, 2, 4]]) and np.all(poles[[2, 4]] == poles[0]) and np.all(poles[3] == poles[1])
    # the seam: the two sides differ by no more than the two bounds allow (the lookup wraps continuously)
    seam = sets["seam"]
    got, (val, bound) = pr.lookup(seam), R.env(rgbe, seam)
    plus, minus = np.arange(0, len(seam), 4), np.arange(2, len(seam), 4)        # (y 0, +z) and (y 0, −z) of each magnitude, then the same at y 0.25
    for p, m in ((plus, minus), (plus + 1, minus + 1)):
        assert np.all(np.abs(got[p].astype(np.float64) - got[m]) <= bound[p] + bound[m] + np.abs(val[p] - val[m])), size
    # sample() of the existing API reports the radiance lookup() returns at the direction it reports
    u = np.random.RandomState(3).uniform(0, 1, (2000, 6)).astype(F)
    dirs, pdf, rad = pr.sample(u)
    ok = pdf > 0
    assert ok.sum() > 1000 and pr.lookup(dirs[ok]).tobytes() == rad[ok].tobytes()
    pr.close()
    print("\ndevice probe %dx%d: worst |error| / bound %s" % (W, H, "  ".join("%s %.3f" % kv for kv in rep.items())))


def test_a_1x1_probe_is_constant_for_every_direction(device):
    rgbe = np.array([[[200, 100, 50, 130]]], np.uint8)
    pr = lp.ProbeGPU(device, rgbe, 1, 1)
    d = np.concatenate([R.all_directions(2, 2), np.array([(np.nan, 0, 0), (0, np.nan, 0), (0, 0, 0), (np.inf, -np.inf, 1), (np.nan, np.nan, np.nan)], F)])
    got = pr.lookup(d)
    pr.close()
    assert np.all(got == R.env(rgbe, d[:1])[0].astype(F))


# ------------------------------------------------------------------ two frame-level pins: shade_hit reads what the probe reads
FW, FH = 64, 48
PIN_VFOV = 0.6
PIN_SIZE = (7, 5)
BLACK = np.zeros((1, 1, 4), np.uint8)
QUAD_POS = np.array([(-0.5, -0.3, -2.0), (0.5, -0.3, -2.0), (0.5, 0.3, -2.0), (-0.5, 0.3, -2.0)], F)
QUAD_UV = np.array([(-0.7, -0.4), (2.3, -0.4), (2.3, 1.9), (-0.7, 1.9)], F)       # wraps: three periods in u, more than two in v
QUAD_NRM = np.tile(F([0, 0, 1]), (4, 1))
QUAD_IDX = np.array([0, 1, 2, 0, 2, 3], np.uint32)
EYE, DIRECTION = (0.11, 0.04, 0.0), (-0.03, 0.02, -1.0)


def _renderer(device, sg, pr, bounces, seed):
    r = lp.Renderer(device, (FW, FH))
    r.downsample_factor = 1.0
    r.resize(device, sg, pr, (FW, FH))
    r.set_max_bounces(bounces)
    r.set_vfov(PIN_VFOV)
    r.set_seed(seed)
    r.reset_accumulation()
    r.accumulate = True
    r.reset_ray_counts()
    return r


@pytest.mark.usefixtures("pipeline")
def test_emissive_frame_is_the_probes_texel_times_le(device):
    """an emissive quad (black base, the 7x5 image, uv from (−0.7, −0.4) to (2.3, 1.9)) before a black probe, light 0 dark, depth 1, one frame at 64x48: at every pixel
    whose primary ray hits the quad the radiance is float32(Le) · sample_textures(prim, (u, v)).emissive, bit for bit — the weight is 1, `E *= tex` is one multiply, and
    T·E with T = 1, 0 + x and the division by one sample are exact"""
    from loupiote_amd import testing as T
    s = lp.Scene()
    s.set_light(0, dark_light())
    img = s.add_image(R.image(*PIN_SIZE))
    m = s.add_material((0.0, 0.0, 0.0, 1.0), 1.0, 0.0)
    s.set_material_emission(m, (0.9, 0.5, 0.25), 3.0, img)
    s.add_instance(s.add_mesh(QUAD_POS, QUAD_NRM, QUAD_UV, QUAD_IDX), IDENTITY, m)
    le = s.material_emission(m)[0]
    sg = lp.SceneGPU.new_from_scene(s, device)
    pr = lp.ProbeGPU(device, BLACK, 1, 1)
    r = _renderer(device, sg, pr, 1, 11)
    view = T.look(EYE, DIRECTION)
    o, d = r.primary_rays(view)
    r.raytrace(view)
    got = r.read_radiance()[..., :3].reshape(-1, 3)
    hit = sg.trace_closest(o.reshape(-1, 3), d.reshape(-1, 3))
    on = hit["prim"] < 2
    tex = sg.sample_textures(hit["prim"][on], np.stack([hit["u"][on], hit["v"][on]], axis=1))
    r.close(); pr.close(); sg.close()
    assert 300 < on.sum() < FW * FH - 300 and np.all(got[~on] == 0)
    want = le.astype(F)[None, :] * tex["emissive"]
    assert want.dtype == F and got[on].tobytes() == want.tobytes()
    val, bound, _ = R.lookup(R.image(*PIN_SIZE), tex["uv"][:, 0].copy(), tex["uv"][:, 1].copy(), True)
    assert R.passes(val[:, :3], bound[:, :3], tex["emissive"]) and np.ptp(tex["uv"][:, 0]) > 2.5 and np.ptp(tex["uv"][:, 1]) > 1.9


@pytest.mark.usefixtures("pipeline")
def test_paired_npot_frame_is_the_oracles_with_and_without_pairing(device):
    """the same quad under a paired 7x5 albedo + mra material, lit by the rectangle light, depth 2, two frames at 64x48: the frame uploaded with pair_textures=True, the one
    with False and the oracle's are the same bytes with equal ray counts — the non-power-of-two, wrapping-uv counterpart of test_gpu_edge's 64x64 texture-pair frame"""
    from loupiote_amd import scenes, testing as T
    from oracle import harness, orc
    light = np.zeros(1, lp._abi.LIGHT_DT)
    light["normal"], light["tangent"], light["bitangent"], light["origin"] = (0, 0, -1, 0), (1, 0, 0, 0.4), (0, 1, 0, 0.3), (0.1, 0.1, -0.8, 9.0)
    desc = {"meshes": [{"positions": QUAD_POS, "normals": QUAD_NRM, "uvs": QUAD_UV, "indices": QUAD_IDX}], "instances": [(1, IDENTITY, 1)],
            "materials": [((0.9, 0.8, 0.7, 1.0), 0.8, 0.6, 0, 1)], "images": [R.image(*PIN_SIZE, 0), R.image(*PIN_SIZE, 1)], "lights": [light]}
    view = T.look(EYE, DIRECTION)
    osc = orc.OracleScene.from_scene(harness.to_oracle(desc), probe=BLACK)
    acc, oc = osc.render(FW, FH, view, PIN_VFOV, 2, frames=2, user_seed=11, want_counters=True)
    want = orc.resolve(acc)
    assert want[..., :3].max() > 0
    for pair in (True, False):
        sg = lp.SceneGPU.new_from_scene(scenes.to_product(desc), device, pair_textures=pair)
        pr = lp.ProbeGPU(device, BLACK, 1, 1)
        r = _renderer(device, sg, pr, 2, 11)
        for _ in range(2):
            r.raytrace(view)
        c, img = r.ray_counts(), r.read_radiance()
        assert sg.stats().texture_pairs == (1 if pair else 0)
        r.close(); pr.close(); sg.close()
        assert (c.closest, c.shadow, c.shaded) == (oc.closest, oc.shadow, oc.shaded), pair
        assert img.tobytes() == want.tobytes(), pair
