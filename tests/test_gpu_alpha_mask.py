"""-m gpu: alpha-masked (cutout) materials, SPEC.md §20 — glTF alphaMode MASK down to the traversal.

The reference of tests 1-3 never sees the masked scene: every masked quad ALONE, as an opaque scene, goes through the oracle's brute-force
trace_closest, which gives the candidate (t, u, v, prim) per layer exactly as §7 accepts it; tests/alpha_ref.py (numpy float32, written from the
SPEC) decides each candidate; the nearest accepted one, or the wall behind, wins.  The product must return that hit bit for bit.  A ray whose
reference alpha lies within 1e-6 of the cutoff may be left out (EXCLUDE_CAP = 1 % at the most, asserted from the reference alone): the texels are
0 / 255 and the cutoff 0.5, so alpha passes the cutoff only in the one-texel ramps between blocks, with a slope of a whole texel.

Frames (tests 3-5) are compared with frames only, bit for bit: cutoff 0 keeps everything (= the opaque scene), cutoff 2 cuts everything (= the
scene without the masked instances, which come last so that prim ids agree), and every launch path gives one frame."""
import json
import os
import struct
import zlib

import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import _abi as A, testing as T

import alpha_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID = A.INVALID_INDEX
MISS = 0xFFFFFFFF
EXCLUDE_CAP = 0.01
NEAR_CUTOFF = 1e-6

# alpha 255 / 0 in 4x4-texel blocks of a 16x16 image: PATTERN[by][bx]; no row or column is uniform, no symmetry
PATTERN = np.array([[1, 0, 1, 0], [0, 1, 1, 0], [1, 1, 0, 0], [0, 0, 1, 1]], np.uint8)


def mask_texture():
    img = np.zeros((16, 16, 4), np.uint8)
    img[..., 0], img[..., 1], img[..., 2] = 200, 180, 90
    img[..., 3] = np.kron(PATTERN, np.ones((4, 4), np.uint8)) * 255
    return img


def png_bytes(img):
    """an 8-bit PNG of img[H, W, 3 | 4] (colour type 2 | 6), filter 0"""
    h, w, c = img.shape

    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)

    raw = b"".join(b"\0" + np.ascontiguousarray(img[y]).tobytes() for y in range(h))
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6 if c == 4 else 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 9))
            + chunk(b"IEND", b""))


def alpha_glb(mode="MASK", cutoff=0.5, with_quad=True, image=None, mime="image/png"):
    """a small .glb: a 8x8 floor at y = 0, a 2x2 quad one unit above it whose material has the 16x16 RGBA mask texture (alphaMode `mode`, None: not
    stated; alphaCutoff `cutoff`, None: not stated) and one directional light that shines straight down.  `image`: other bytes for the texture"""
    blob = bytearray()
    views, accessors = [], []

    def view(raw):
        views.append({"buffer": 0, "byteOffset": len(blob), "byteLength": len(raw)})
        blob.extend(raw)
        blob.extend(b"\0" * (-len(blob) % 4))
        return len(views) - 1

    def add(arr, ctype, atype):
        accessors.append({"bufferView": view(np.ascontiguousarray(arr).tobytes()), "componentType": ctype, "count": len(arr), "type": atype})
        return len(accessors) - 1

    quad = np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], "<f4")
    nrm = np.tile(np.array([[0, 1, 0]], "<f4"), (4, 1))
    uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], "<f4")
    ipos, inrm, iidx = add(quad, 5126, "VEC3"), add(nrm, 5126, "VEC3"), add(np.array([0, 2, 1, 0, 3, 2], "<u2"), 5123, "SCALAR")
    floor = {"attributes": {"POSITION": ipos, "NORMAL": inrm}, "indices": iidx, "material": 0}
    leaf = {"attributes": {"POSITION": ipos, "NORMAL": inrm, "TEXCOORD_0": add(uv, 5126, "VEC2")}, "indices": iidx, "material": 1}
    masked = {"pbrMetallicRoughness": {"baseColorFactor": [1.0, 1.0, 1.0, 1.0], "roughnessFactor": 0.9, "metallicFactor": 0.0, "baseColorTexture": {"index": 0}}}
    if mode is not None:
        masked["alphaMode"] = mode
    if cutoff is not None:
        masked["alphaCutoff"] = cutoff
    q = [np.sin(-np.pi / 4), 0.0, 0.0, np.cos(-np.pi / 4)]     # -90 degrees about X: the light's -Z axis points straight down
    nodes = [{"mesh": 0, "scale": [4.0, 1.0, 4.0]}]
    if with_quad:
        nodes.append({"mesh": 1, "translation": [0.0, 1.0, 0.0]})
    nodes.append({"rotation": q, "extensions": {"KHR_lights_punctual": {"light": 0}}})
    js = {"asset": {"version": "2.0"}, "meshes": [{"primitives": [floor]}, {"primitives": [leaf]}], "accessors": accessors,
          "materials": [{"pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.7, 0.6, 1.0], "roughnessFactor": 0.6, "metallicFactor": 0.1}}, masked],
          "textures": [{"source": 0}], "images": [{"bufferView": view(png_bytes(mask_texture()) if image is None else image), "mimeType": mime}],
          "nodes": nodes, "extensionsUsed": ["KHR_lights_punctual"],
          "extensions": {"KHR_lights_punctual": {"lights": [{"type": "directional", "color": [1.0, 0.95, 0.9], "intensity": 3.0}]}}}
    js["bufferViews"] = views
    js["buffers"] = [{"byteLength": len(blob)}]
    j = json.dumps(js).encode()
    j += b" " * (-len(j) % 4)
    b = bytes(blob)
    return struct.pack("<III", 0x46546C67, 2, 12 + 8 + len(j) + 8 + len(b)) + struct.pack("<II", len(j), 0x4E4F534A) + j + struct.pack("<II", len(b), 0x004E4942) + b


# ---------------------------------------------------------------- the layered scene of tests 1-3 and 5
LAYER_Z = (0.0, -0.5, -1.0, -1.5)
LAYER_UV_SCALE = (1.0, 0.5, 2.5, 1.0)       # 2.5: the texture repeats
LAYER_IMAGE = (True, True, True, False)     # the last layer has no image and color.w = 0.3
WALL_Z, WALL_N = -3.0, 4                    # a 4x4-cell wall (32 triangles, so that the scene is large enough for the GPU builder and a real rebuild)
QUAD_IDX = np.array([0, 1, 2, 0, 2, 3], np.uint32)


def _wall_mesh():
    g = np.linspace(-3.0, 3.0, WALL_N + 1, dtype=np.float32)
    pos = np.array([[x, y, WALL_Z] for y in g for x in g], np.float32)
    idx = []
    for j in range(WALL_N):
        for i in range(WALL_N):
            a = j * (WALL_N + 1) + i
            idx += [a, a + 1, a + WALL_N + 2, a, a + WALL_N + 2, a + WALL_N + 1]
    return pos, np.array(idx, np.uint32)


def _layer_mesh(k):
    z, s = LAYER_Z[k], LAYER_UV_SCALE[k]
    pos = np.array([[-1, -1, z], [1, -1, z], [1, 1, z], [-1, 1, z]], np.float32)
    uv = np.array([[0, 0], [s, 0], [s, s], [0, s]], np.float32)
    return pos, uv


def layered_scene(cutoff=0.5, masks=True, quads=True):
    """the wall first (prims 0..31), then the four quads (prims 32..39).  masks False: the same materials, all opaque"""
    s = lp.Scene()
    img = s.add_image(mask_texture())
    nrm = lambda n: np.tile(np.array([[0, 0, 1]], np.float32), (n, 1))
    wpos, widx = _wall_mesh()
    wall = s.add_mesh(wpos, nrm(len(wpos)), None, widx)
    s.add_instance(wall, np.eye(4, dtype=np.float32), s.add_material((0.7, 0.7, 0.7, 1.0), 0.8, 0.0))
    for k in range(len(LAYER_Z) if quads else 0):
        pos, uv = _layer_mesh(k)
        blas = s.add_mesh(pos, nrm(4), uv, QUAD_IDX)
        mat = s.add_material((0.9, 0.8, 0.7, 1.0 if LAYER_IMAGE[k] else 0.3), 0.7, 0.0, albedo_texture=img if LAYER_IMAGE[k] else INVALID)
        if masks:
            s.set_material_alpha(mat, A.ALPHA_MASK, cutoff, img if LAYER_IMAGE[k] else INVALID)
        s.add_instance(blas, np.eye(4, dtype=np.float32), mat)
    light = np.zeros(1, A.LIGHT_DT)
    light["normal"], light["tangent"], light["bitangent"], light["origin"] = (0, -1, 0, 0), (1, 0, 0, 0.8), (0, 0, 1, 0.8), (0, 2.5, 1.0, 12.0)
    s.set_light(0, light)
    return s


class Reference:
    """per layer ALONE through the oracle's brute force, §20 by alpha_ref, the nearest accepted layer or the wall"""

    def __init__(self):
        from oracle import gltf_oracle as G, orc
        mat = np.zeros(1, G.MATERIAL_DT)
        mat["color"], mat["roughness"], mat["albedo_texture"], mat["mra_texture"] = 1.0, 1.0, INVALID, INVALID
        dark = np.zeros(1, G.LIGHT_DT)
        dark["normal"], dark["tangent"], dark["bitangent"], dark["origin"] = (0, -1, 0, 0), (1, 0, 0, 0.1), (0, 0, 1, 0.1), (0, -50.0, 0, 0.0)

        def soup(pos, idx):
            v = np.zeros(len(idx), G.VERTEX_DT)
            v["position"][:, :3] = pos[idx]
            v["normal"][:, 2] = 1.0
            return orc.OracleScene(v, np.zeros(len(idx) // 3, np.uint32), mat, dark)

        self.wall = soup(*_wall_mesh())
        self.layers = []
        for k in range(len(LAYER_Z)):
            pos, uv = _layer_mesh(k)
            self.layers.append((soup(pos, QUAD_IDX), uv[QUAD_IDX].reshape(2, 3, 2)))
        self.image = mask_texture()

    def closest(self, o, d, cutoff=0.5):
        """-> (hits as HIT_DT, near: rays with a layer's alpha within NEAR_CUTOFF of the cutoff, accepted layer hits [n, layers] as t or inf)"""
        best = self.wall.trace_closest(o, d, brute_force=True).copy()
        best_is_wall = np.ones(len(o), bool)
        near = np.zeros(len(o), bool)
        ts = np.full((len(o), len(self.layers)), np.inf)
        for k, (sc, uv) in enumerate(self.layers):
            h = sc.trace_closest(o, d, brute_force=True)
            hit = h["prim"] < 2
            a = np.zeros(len(o), np.float32)
            for tri in range(2):
                m = hit & (h["prim"] == tri)
                a[m] = R.alpha(1.0 if LAYER_IMAGE[k] else 0.3, self.image if LAYER_IMAGE[k] else None, uv[tri], h["u"][m], h["v"][m])
            near |= hit & (np.abs(a.astype(np.float64) - cutoff) <= NEAR_CUTOFF)
            ok = hit & R.counts(a, cutoff)
            ts[ok, k] = h["t"][ok]
            take = ok & ((h["t"] < best["t"]) | (best["prim"] == MISS))
            best["t"][take], best["u"][take], best["v"][take] = h["t"][take], h["u"][take], h["v"][take]
            best["prim"][take] = 2 * WALL_N * WALL_N + 2 * k + h["prim"][take]
            best_is_wall &= ~take
        return best, near, ts


@pytest.fixture(scope="module")
def reference():
    return Reference()


def _rays(n=4096, seed=11):
    """half aimed at random points of the quads, half at their edges and at the borders of the texel blocks"""
    rng = np.random.default_rng(seed)
    o = (np.array([0.0, 0.0, 3.0]) + rng.uniform(-0.4, 0.4, (n, 3))).astype(np.float32)
    k = rng.integers(0, len(LAYER_Z), n)
    z = np.array(LAYER_Z)[k]
    xy = rng.uniform(-1.1, 1.1, (n, 2))
    half = n // 2
    # borders: uv multiples of 1/4 (the blocks) — x = 2 uv / scale - 1 — and the quad's own edges; one coordinate snapped
    s = np.array(LAYER_UV_SCALE)[k[half:]]
    m = rng.integers(0, 11, n - half)
    snap = np.where(m < 9, np.minimum(2.0 * (0.25 * m) / s - 1.0, 1.0), np.where(m == 9, -1.0, 1.0))
    axis = rng.integers(0, 2, n - half)
    # ... beside the border by 1e-5 .. 2e-3 of the quad (alpha leaves the cutoff by 8 x scale x that: well past NEAR_CUTOFF), and 16 rays (0.4 %) exactly on it
    jitter = rng.choice([1e-5, -1e-5, 1e-4, -1e-4, 3e-4, -3e-4, 2e-3, -2e-3], n - half)
    jitter[:16] = 0.0
    xy[half:][np.arange(n - half), axis] = snap + jitter
    target = np.c_[xy, z]
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d.astype(np.float32)


@pytest.fixture(scope="module")
def ray_reference(reference):
    o, d = _rays()
    hits, near, ts = reference.closest(o, d)
    wall_t = reference.wall.trace_closest(o, d, brute_force=True)["t"]
    return o, d, hits, near, ts, wall_t


pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- 1. closest hit
@pytest.mark.parametrize("gpu_build", [False, True])
def test_closest_hit_matches_the_layered_reference(device, ray_reference, gpu_build):
    o, d, want, near, ts, _ = ray_reference
    assert near.mean() <= EXCLUDE_CAP, near.mean()
    layer = (want["prim"] >= 32) & (want["prim"] != MISS)
    assert layer.sum() > 1000 and (np.isfinite(ts).sum(1) < (ts.shape[1] - 1)).sum() > 1000     # hits on quads, and cut-away candidates in front of them
    sg = lp.SceneGPU.new_from_scene(layered_scene(), device, gpu_build=gpu_build)
    got = sg.trace_closest(o, d)
    sg.close()
    keep = ~near
    for f in ("prim", "t", "u", "v"):
        bad = keep & (got[f].view(np.uint32) != want[f].view(np.uint32))
        assert not bad.any(), (f, int(bad.sum()), got[bad][:4], want[bad][:4])


# ---------------------------------------------------------------- 2. any hit
@pytest.mark.parametrize("gpu_build", [False, True])
def test_any_hit_matches_the_layered_reference(device, ray_reference, gpu_build):
    o, d, _, near, ts, wall_t = ray_reference
    tmax = np.where(wall_t < 1e29, np.float32(0.999) * wall_t, np.float32(100.0)).astype(np.float32)    # the segment ends in front of the wall
    want = (ts <= tmax[:, None].astype(np.float64)).any(1)
    assert 0.2 < want.mean() < 0.9
    sg = lp.SceneGPU.new_from_scene(layered_scene(), device, gpu_build=gpu_build)
    got = sg.trace_occluded(o, d, tmax).astype(bool)
    sg.close()
    keep = ~near
    assert np.array_equal(got[keep], want[keep]), int((got[keep] != want[keep]).sum())


# ---------------------------------------------------------------- 3. the launch paths
EYE, DIR = (0.15, 0.1, 3.0), (0.0, 0.0, -1.0)
BOUNCES, SPP = 3, 2
SIZES = [(64, 36), (256, 144)]
VARIANTS = ["default", "packet", "lanes", "raytrace_n", "shards"]


def _renderer(device, sg, size, variant, mode=None):
    r = lp.Renderer(device, size)
    r.downsample_factor = 1.0
    r.resize(device, sg, None, size)
    r.set_max_bounces(BOUNCES)
    r.set_vfov(T.VFOV)
    if variant == "packet":
        r.set_option("packet_primary", 1)
    if variant == "lanes":
        r.set_lanes(2)
    if mode is not None:
        r.set_blit_mode(mode)
    return r


def _frame(device, scene, size, variant="default", gbuffer=False):
    """SPP samples of the frame (path-traced: the radiance; gbuffer: SPP denoised frames, -> the last one's G-buffer and main target)"""
    sg = lp.SceneGPU.new_from_scene(scene, device)
    view = T.look(EYE, DIR)
    out = None
    for rank in range(2 if variant == "shards" else 1):
        r = _renderer(device, sg, size, variant, lp.BlitMode.DenoisedPathrace if gbuffer else None)
        if variant == "shards":
            r.set_shard(rank, 2)
            r.set_resources(device, sg, None)
        r.reset_accumulation()
        r.accumulate = True
        if variant == "raytrace_n":
            r.raytrace_n(view, SPP)
        else:
            for _ in range(SPP):
                r.raytrace(view)
        part = r.read_denoiser()[0] if gbuffer else r.read_radiance()
        out = part if out is None else out + part       # the ranks' buffers are zero outside their tiles (SPEC §13, §15.5)
        r.close()
    sg.close()
    return out


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_cutoff_zero_is_the_opaque_frame(device, size):
    want = _frame(device, layered_scene(masks=False), size)
    assert want[..., :3].max() > 0.05
    for v in VARIANTS:
        got = _frame(device, layered_scene(cutoff=0.0), size, v)
        assert got.tobytes() == want.tobytes(), v


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_cutoff_two_is_the_frame_without_the_masked_instances(device, size):
    want = _frame(device, layered_scene(quads=False), size)
    for v in VARIANTS:
        got = _frame(device, layered_scene(cutoff=2.0), size, v)
        assert got.tobytes() == want.tobytes(), v


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_primary_prim_ids_and_one_frame_on_every_launch_path(device, reference, size):
    from oracle import orc
    w, h = size
    view = T.look(EYE, DIR)
    seed = BOUNCES * (SPP - 1)      # a denoised frame is one sample; the seed counter moves by the depth per frame (SPEC §1)
    o, d = np.zeros((h * w, 3), np.float32), np.zeros((h * w, 3), np.float32)
    for y in range(h):
        for x in range(w):
            o[y * w + x], d[y * w + x] = orc.raygen(w, h, view, T.VFOV, x, y, 0, seed)
    want, near, _ = reference.closest(o, d)
    assert near.mean() <= EXCLUDE_CAP, near.mean()
    prims = want["prim"].reshape(h, w)
    assert ((prims >= 32) & (prims != MISS)).mean() > 0.05 and (prims < 32).mean() > 0.05
    scene = layered_scene()
    frames = [_frame(device, scene, size, v) for v in VARIANTS]
    for v, f in zip(VARIANTS, frames):
        assert f.tobytes() == frames[0].tobytes(), v
    for v in VARIANTS:
        g = _frame(device, scene, size, v, gbuffer=True)
        got = g[..., 0]
        keep = ~near.reshape(h, w)
        assert np.array_equal(got[keep], prims[keep]), (v, int((got[keep] != prims[keep]).sum()))


# ---------------------------------------------------------------- 4. the point of it: a cut-away block casts no shadow
def _glb_frame(device, glb, size=(96, 64)):
    s = lp.Scene()
    lp.loaders.load_gltf(glb, s)
    dark = np.zeros(1, A.LIGHT_DT)
    dark["normal"], dark["tangent"], dark["bitangent"], dark["origin"] = (0, -1, 0, 0), (1, 0, 0, 0.1), (0, 0, 1, 0.1), (0, -50.0, 0, 0.0)
    s.set_light(0, dark)
    sg = lp.SceneGPU.new_from_scene(s, device)
    r = lp.Renderer(device, size)
    r.downsample_factor = 1.0
    r.resize(device, sg, None, size)
    r.set_max_bounces(1)            # the primary hit and its shadow ray: nothing else reaches the quad from a floor pixel
    r.set_vfov(T.VFOV)
    r.reset_accumulation()
    r.accumulate = True
    for _ in range(8):
        r.raytrace(T.look(GLB_EYE, GLB_DIR))
    img = r.read_radiance()
    r.close()
    sg.close()
    return img


GLB_EYE, GLB_DIR = (0.0, 0.9, 3.0), (0.0, -0.3, -1.0)       # below the quad's height: no camera ray meets the quad on its way to the floor


def _floor_blocks(w, h):
    """per pixel: the mask block (by, bx) its WHOLE footprint on the floor lies under, between the centres of the block's outer texels (where the bilinear alpha is the block's own 0 or 1) with a tenth of a texel to spare, or -1 (SPEC §11 in float64)"""
    v = np.asarray(T.look(GLB_EYE, GLB_DIR), np.float64).reshape(4, 4)
    right, up, fwd, origin = v[0, :3], v[1, :3], v[2, :3], v[3, :3]
    th = np.tan(T.VFOV / 2)
    block = None
    for jx in (0.0, 1.0):
        for jy in (0.0, 1.0):
            x, y = np.meshgrid(np.arange(w) + jx, np.arange(h) + jy)
            d = right * ((2 * x / w - 1) * (w / h * th))[..., None] + up * ((1 - 2 * y / h) * th)[..., None] + fwd
            t = np.where(d[..., 1] < -1e-9, -origin[1] / np.minimum(d[..., 1], -1e-9), np.inf)
            P = origin + d * t[..., None]
            tex = np.stack([(P[..., 0] + 1) / 2, (P[..., 2] + 1) / 2], -1) * 16          # texel coordinates under the quad (uv = (x + 1) / 2, (z + 1) / 2)
            inside = np.isfinite(t) & (tex.min(-1) > 0) & (tex.max(-1) < 16)
            b = np.floor(np.where(inside[..., None], tex, 0) / 4).astype(int)
            frac = np.where(inside[..., None], tex, 0) - 4 * b
            ok = inside & (frac.min(-1) > 0.6) & (frac.max(-1) < 3.4)
            code = np.where(ok, b[..., 1] * 4 + b[..., 0], -1)
            block = code if block is None else np.where(block == code, block, -1)
    return block


def test_a_cut_away_block_casts_no_shadow(device):
    with open(os.path.join(HERE, "golden", "alpha-mask.glb"), "rb") as f:
        committed = f.read()
    assert committed == alpha_glb() and len(committed) < 16384       # the committed copy is this writer's output
    w, h = 96, 64
    masked = _glb_frame(device, committed, (w, h))
    opaque = _glb_frame(device, alpha_glb(mode="OPAQUE"), (w, h))
    without = _glb_frame(device, alpha_glb(with_quad=False), (w, h))
    block = _floor_blocks(w, h)
    kept = (block >= 0) & (PATTERN.reshape(-1)[np.maximum(block, 0)] == 1)
    cut = (block >= 0) & (PATTERN.reshape(-1)[np.maximum(block, 0)] == 0)
    assert kept.sum() >= 8 and cut.sum() >= 8, (int(kept.sum()), int(cut.sum()))
    assert np.array_equal(masked[cut], without[cut]) and masked[cut][:, :3].mean() > 0.01         # lit, exactly as if the quad were not there
    assert np.array_equal(masked[kept], opaque[kept]) and masked[kept][:, :3].max() == 0          # shadowed, exactly as under the solid quad: no probe, depth 1
    assert not np.array_equal(opaque[cut], without[cut])


# ---------------------------------------------------------------- 5. refit and rebuild
def test_refit_and_rebuild_keep_the_mask(device):
    size = (64, 36)
    moved = np.eye(4, dtype=np.float32)
    moved[:3, 3] = (0.35, -0.2, 0.4)          # column-major below: the translation goes to elements 12..14
    scene = layered_scene()
    inst = scene.counts().instances - 4       # the first masked quad
    fresh_scene = layered_scene()
    fresh_scene.set_instance_transform(inst, moved.T)
    want = _frame(device, fresh_scene, size)
    assert want.tobytes() != _frame(device, scene, size).tobytes()

    sg = lp.SceneGPU.new_from_scene(scene, device)
    scene.set_instance_transform(inst, moved.T)
    view = T.look(EYE, DIR)

    def frame():
        r = _renderer(device, sg, size, "default")
        r.reset_accumulation()
        r.accumulate = True
        for _ in range(SPP):
            r.raytrace(view)
        img = r.read_radiance()
        r.close()
        return img

    sg.update_instances(scene)
    assert frame().tobytes() == want.tobytes()
    sg.rebuild(scene)
    assert frame().tobytes() == want.tobytes()
    # a material that stops masking: the rebuild re-derives the table (cutoff 0.5 -> opaque)
    for m in range(scene.counts().materials):
        scene.set_material_alpha(m, A.ALPHA_OPAQUE)
    sg.rebuild(scene)
    opaque = layered_scene(masks=False)
    opaque.set_instance_transform(inst, moved.T)
    assert frame().tobytes() == _frame(device, opaque, size).tobytes()
    sg.close()
