"""-m gpu: the per-element device probes (`Device.interface_sample` / `bsdf_probe`, `SceneGPU.sample_punctual` / `sample_emitter` / `shading_normal` / `sample_textures` /
`trace_closest` / `trace_occluded`, `ProbeGPU.sample` / `pdf` / `lookup`) share one upload / launch / read-back path.  For each of the eleven, a batch of 257 elements —
one 256-thread block and one element, four 64-lane traversal blocks and one lane — must equal, bit for bit, the three calls on its elements [0:1], [1:256] and
[256:257] put together: an element's answer depends on neither the size of its batch nor its place in it, which pins the strides, the rows and the grid arithmetic of that
path.  An empty batch succeeds and returns empty arrays of the same trailing shape, and a scene or an environment probe handed to a device that does not own it is
refused.  Nothing here is about values: the reference modules of each probe hold those."""
import numpy as np
import pytest

import emitter_scenes as ES
import texture_ref as TR
import loupiote_amd as lp

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("pipeline")]
F = np.float32
N = 257
CUTS = ((0, 1), (1, 256), (256, 257))
PROBE_SIZE = (8, 4)


def build_scene():
    """three quads in y = 0, 1, 2 under a point light: a textured pair, a normal-mapped material whose albedo image stands alone in the atlas, and a textured emitter
    (the scene's emitter distribution); prims 0..5"""
    b = ES.Built()
    i0, i1 = b.image(TR.image(5, 3, 0)), b.image(TR.image(5, 3, 1))
    pair = b.s.add_material((1.0, 1.0, 1.0, 1.0), 1.0, 1.0, albedo_texture=i0, mra_texture=i1)
    bumpy = b.s.add_material((0.8, 0.8, 0.8, 1.0), 1.0, 0.0, albedo_texture=i0)
    b.s.set_material_normal_map(bumpy, i1, 1.0)
    lamp = b.material((2.0, 1.0, 4.0), i0)
    uv = F([(0.0, 0.0), (2.5, 0.0), (2.5, 1.7), (0.0, 1.7)])
    for k, mat in enumerate(((pair, None), (bumpy, None), lamp)):
        b.mesh(ES.QUAD + F([0, k - 1.0, 0]), ES.QUAD_IDX, mat, uv=uv)
    b.s.add_punctual_light(lp.point_light((0.3, 3.0, -2.5), (1.0, 0.9, 0.8), 5.0))
    return b.s, 6


def build_probe():
    """texture_ref's 8x4 probe with its edge exponents (0 .. 10: black or nearly, 255: the largest) drawn back into 120 .. 136, so that no one texel holds the whole
    distribution and the draws spread over the alias table"""
    p = TR.probe(*PROBE_SIZE)
    p[..., 3] = np.clip(p[..., 3], 120, 136)
    return p


def unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


@pytest.fixture(scope="module")
def probes(device):
    """name -> (the entry point, its per-element inputs), all of N elements from one fixed seed"""
    rs = np.random.RandomState(257)
    scene, n_tris = build_scene()
    assert lp.env_distribution(build_probe())["total"] > 0.0       # the environment probes run their kernels, not the fill of a probe without a distribution
    sg = lp.SceneGPU.new_from_scene(scene, device)
    env = lp.ProbeGPU(device, build_probe(), *PROBE_SIZE)
    u = lambda *shape: rs.uniform(0.0, 1.0, (N,) + shape).astype(F)
    dirs = lambda: unit(rs.normal(size=(N, 3)))
    points = (rs.uniform(-1.0, 1.0, (N, 3)) + [0.0, 0.5, -3.0]).astype(F)
    prim = rs.randint(0, n_tris, N).astype(np.uint32)
    bary = (u(2) * F(0.5)).astype(F)
    normal = dirs()
    about = lambda: unit(normal + 0.9 * rs.normal(size=(N, 3)) / np.sqrt(3.0))       # mostly in the normal's hemisphere: the BSDF has something to say
    bsdf_rows = np.concatenate([u(3), u(2), normal, about(), about(), about(), u(3)], axis=1)
    origins = (points + F([0.0, 2.5, 0.0])).astype(F)
    table = {
        "sample_punctual": (lambda p: sg.sample_punctual(0, p), [points]),
        "sample_emitter": (sg.sample_emitter, [points, u(4)]),
        "shading_normal": (sg.shading_normal, [prim, bary, dirs()]),
        "sample_textures": (sg.sample_textures, [prim, bary]),
        "interface_sample": (device.interface_sample, [dirs(), dirs(), dirs(), rs.randint(0, 2, N), u(3), (F(1.0) + u()).astype(F), rs.randint(0, 2, N), u()]),
        "bsdf_probe": (device.bsdf_probe, [bsdf_rows]),
        "probe_sample": (env.sample, [u(6)]),
        "probe_pdf": (env.pdf, [dirs()]),
        "probe_lookup": (env.lookup, [dirs()]),
        "trace_closest": (sg.trace_closest, [origins, unit(rs.normal(size=(N, 3)) + [0.0, -3.0, 0.0])]),
        "trace_occluded": (sg.trace_occluded, [origins, unit(rs.normal(size=(N, 3)) + [0.0, -3.0, 0.0]), (u() * F(4.0)).astype(F)]),
    }
    yield table
    env.close()
    sg.close()


NAMES = ("sample_punctual", "sample_emitter", "shading_normal", "sample_textures", "interface_sample", "bsdf_probe", "probe_sample", "probe_pdf", "probe_lookup",
         "trace_closest", "trace_occluded")


def arrays(out):
    """what an entry point returns — an array, a tuple of arrays or a dict of arrays — as a list of arrays in a fixed order"""
    if isinstance(out, dict):
        return [np.asarray(out[k]) for k in sorted(out)]
    return [np.asarray(a) for a in (out if isinstance(out, tuple) else (out,))]


@pytest.mark.parametrize("name", NAMES)
def test_a_batch_equals_its_pieces(probes, name):
    fn, inputs = probes[name]
    assert all(len(a) == N for a in inputs)
    whole = arrays(fn(*inputs))
    pieces = [arrays(fn(*[a[lo:hi] for a in inputs])) for lo, hi in CUTS]
    assert all(len(a) == N for a in whole)
    for k, w in enumerate(whole):
        joined = np.concatenate([p[k] for p in pieces])
        assert joined.dtype == w.dtype and joined.shape == w.shape, (name, k)
        assert joined.tobytes() == w.tobytes(), (name, k, "an element's answer depends on its batch")


@pytest.mark.parametrize("name", NAMES)
def test_an_empty_batch_succeeds(probes, name):
    fn, inputs = probes[name]
    one = arrays(fn(*[a[:1] for a in inputs]))
    none = arrays(fn(*[a[:0] for a in inputs]))
    assert len(none) == len(one)
    for e, o in zip(none, one):
        assert e.dtype == o.dtype and e.shape == (0,) + o.shape[1:], (name, e.shape, o.shape)


def test_a_scene_or_probe_of_another_device_is_refused(device):
    """every probe that takes a scene or an environment probe answers LPT_ERR_INVALID_ARG to a device that does not own it — the two ray queries as well, which used to
    launch with the other device's pointers"""
    scene, _ = build_scene()
    sg = lp.SceneGPU.new_from_scene(scene, device)
    env = lp.ProbeGPU(device, build_probe(), *PROBE_SIZE)
    other = lp.Device(0)
    p, b, d = np.zeros((1, 3), F), np.zeros((1, 2), F), F([[0.0, 0.0, -1.0]])
    calls = [lambda: sg.sample_punctual(0, p), lambda: sg.sample_emitter(p, np.zeros((1, 4), F)), lambda: sg.shading_normal([0], b, d), lambda: sg.sample_textures([0], b),
             lambda: sg.trace_closest(p, d), lambda: sg.trace_occluded(p, d, F([1.0])), lambda: env.sample(np.zeros((1, 6), F)), lambda: env.pdf(d), lambda: env.lookup(d)]
    sg._dev = env._dev = other           # the wrappers pass the device they were made with: hand them the other one
    try:
        for k, call in enumerate(calls):
            with pytest.raises(lp.Error) as e:
                call()
            assert e.value.status == lp._abi.LPT_ERR_INVALID_ARG and "another device" in str(e.value), (k, str(e.value))
    finally:
        sg._dev = env._dev = device
    for call in calls:
        call()                           # and to its own device each still answers
    env.close()
    sg.close()
    other.close()
