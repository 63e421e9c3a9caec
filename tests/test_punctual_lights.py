"""CPU: punctual lights (SPEC.md §19) on the host side — the scene array and its checks, lpt_punctual_light_make against float64, the
KHR_lights_punctual loader (SPEC.md §14(6)), and the float64 reference (tests/punctual_ref.py) at its corners by hand."""
import base64
import json
import os
import struct

import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import _abi as A

import punctual_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- scene array
def test_default_scene_has_no_punctual_lights_and_the_old_counts():
    s = lp.Scene()
    assert s.punctual_count() == 0 and s.punctual_lights.shape == (0,)
    c = s.counts()
    assert (c.materials, c.entries, c.vertices, c.instances, c.lights, c.images, c.indices) == (1, 1, 1, 1, 1, 0, 0)
    s.add_punctual_light(lp.point_light((1, 2, 3)))
    c = s.counts()   # lpt_scene_counts keeps its layout: the punctual lights have a count of their own
    assert (c.materials, c.entries, c.vertices, c.instances, c.lights, c.images, c.indices) == (1, 1, 1, 1, 1, 0, 0)
    assert A.PUNCTUAL_DT.itemsize == 64 and A.lib().lpt_abi_version() == 6


def test_round_trip_add_set_get_count():
    s = lp.Scene()
    i0 = s.add_punctual_light(lp.point_light((1, 2, 3), color=(1, 0.5, 0.25), intensity=8.0, range=5.0))
    i1 = s.add_punctual_light(lp.spot_light((0, 4, 0), (0, -3, 4), intensity=2.0, inner_angle=0.2, outer_angle=0.6))
    i2 = s.add_punctual_light(lp.directional_light((2, -2, 1), color=(0.5, 0.5, 1.0), intensity=3.0))
    assert (i0, i1, i2) == (0, 1, 2) and s.punctual_count() == 3
    L = s.punctual_lights
    assert tuple(L[0]["position"]) == (1, 2, 3, 0) and tuple(L[0]["color"]) == (8, 4, 2, 0) and L[0]["direction"][3] == 5.0
    assert tuple(L[0]["cone"]) == (-2, 1, 0, 0)      # a point light's cone window is neutral
    assert L[1]["position"][3] == 1 and np.allclose(L[1]["direction"][:3], (0, -0.6, 0.8), atol=1e-7)   # normalised on entry
    assert L[2]["position"][3] == 2 and np.allclose(L[2]["direction"][:3], np.array([2, -2, 1]) / 3.0, atol=1e-7)
    # the derived cone fields against float64
    assert L[1]["cone"][0] == np.float32(np.cos(np.float64(np.float32(0.6))))
    assert L[1]["cone"][1] == np.float32(1.0 / (np.cos(np.float64(np.float32(0.2))) - np.cos(np.float64(np.float32(0.6)))))
    # a direction given unnormalised by hand is normalised by add and set alike
    rec = L[1].copy()
    rec["direction"][:3] = (0, 0, -7)
    s.set_punctual_light(0, rec)
    assert tuple(s.punctual_lights[0]["direction"][:3]) == (0, 0, -1) and s.punctual_count() == 3
    # inner == outer is refused by the constructor; the span's floor of 1e-6 is there for outer barely above inner
    tight = lp.spot_light((0, 0, 0), (0, 0, -1), inner_angle=0.5, outer_angle=np.nextafter(np.float32(0.5), np.float32(1)))
    assert np.isfinite(tight["cone"][0][1]) and tight["cone"][0][1] <= 1.0000001e6


def _bad_records():
    ok = lp.spot_light((0, 1, 0), (0, -1, 0), intensity=2.0, range=3.0)
    out = []
    for field, idx, value in (("position", 0, np.nan), ("direction", 1, np.inf), ("color", 2, np.nan), ("cone", 0, np.inf), ("cone", 3, np.nan),
                              ("position", 3, 3.0), ("position", 3, 0.5), ("position", 3, -1.0),   # unknown types
                              ("direction", 3, -1.0),                                             # negative range
                              ("color", 1, -0.5)):                                                # negative colour
        r = ok.copy()
        r[field][0][idx] = value
        out.append(r)
    for kind in (1.0, 2.0):   # zero direction for a spot / a directional light
        r = ok.copy()
        r["position"][0][3] = kind
        r["direction"][0][:3] = 0
        out.append(r)
    return out


def test_rejected_inputs_report_invalid_arg_and_append_nothing():
    s = lp.Scene()
    s.add_punctual_light(lp.point_light((0, 0, 0)))
    before = s.punctual_lights.tobytes()
    for rec in _bad_records():
        with pytest.raises(lp.Error) as e:
            s.add_punctual_light(rec)
        assert e.value.kind == "InvalidArg"
        with pytest.raises(lp.Error) as e:
            s.set_punctual_light(0, rec)
        assert e.value.kind == "InvalidArg"
    with pytest.raises(lp.Error) as e:
        s.set_punctual_light(1, lp.point_light((0, 0, 0)))
    assert e.value.kind == "InvalidArg"
    assert s.punctual_count() == 1 and s.punctual_lights.tobytes() == before
    for kw in (dict(intensity=-1.0), dict(intensity=np.inf), dict(range=-2.0), dict(inner_angle=0.5, outer_angle=0.5), dict(inner_angle=0.6, outer_angle=0.5),
               dict(outer_angle=2.0), dict(inner_angle=-0.1), dict(direction=(0, 0, 0)), dict(color=(1, -1, 1)), dict(position=(np.nan, 0, 0))):
        args = dict(position=(0, 1, 0), direction=(0, -1, 0))
        args.update(kw)
        with pytest.raises(lp.Error) as e:
            lp.spot_light(**args)
        assert e.value.kind == "InvalidArg", kw
    # a point light has no direction to get wrong
    assert tuple(lp.point_light((0, 0, 0))["direction"][0]) == (0, 0, -1, 0)


# ---------------------------------------------------------------- loader
def make_gltf(nodes, lights=None, glb=False, with_mesh=True):
    """the tiny glTF writer of tests/test_loader.py (its idea, cut down to one triangle mesh) plus the KHR_lights_punctual extension"""
    blob = bytearray()
    views, accessors = [], []
    meshes = []
    if with_mesh:
        raw = np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0]], "<f4").tobytes()
        views.append({"buffer": 0, "byteOffset": 0, "byteLength": len(raw)})
        blob.extend(raw)
        accessors.append({"bufferView": 0, "componentType": 5126, "count": 3, "type": "VEC3"})
        meshes.append({"primitives": [{"attributes": {"POSITION": 0}}]})
    js = {"asset": {"version": "2.0"}, "meshes": meshes, "nodes": list(nodes), "accessors": accessors, "bufferViews": views, "materials": [], "images": [],
          "textures": []}
    if lights is not None:
        js["extensions"] = {"KHR_lights_punctual": {"lights": list(lights)}}
        js["extensionsUsed"] = ["KHR_lights_punctual"]
    if glb:
        js["buffers"] = [{"byteLength": len(blob)}]
        j = json.dumps(js).encode()
        j += b" " * (-len(j) % 4)
        b = bytes(blob) + b"\0" * (-len(blob) % 4)
        return struct.pack("<III", 0x46546C67, 2, 12 + 8 + len(j) + 8 + len(b)) + struct.pack("<II", len(j), 0x4E4F534A) + j + struct.pack("<II", len(b), 0x004E4942) + b
    js["buffers"] = [{"byteLength": len(blob), "uri": "data:application/octet-stream;base64," + base64.b64encode(bytes(blob)).decode()}]
    return json.dumps(js).encode()


def light_node(index, **trs):
    return dict({"extensions": {"KHR_lights_punctual": {"light": index}}}, **trs)


def _quat(axis, angle):
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    return np.append(a * np.sin(angle / 2), np.cos(angle / 2))


def _rotate(q, v):
    """float64 quaternion algebra: q v q*"""
    u, w = q[:3], q[3]
    v = np.asarray(v, np.float64)
    return v + 2.0 * np.cross(u, np.cross(u, v) + w * v)


LIGHTS = [{"type": "point", "color": [1.0, 0.5, 0.25], "intensity": 40.0, "range": 12.5},
          {"type": "spot", "intensity": 7.0, "spot": {"innerConeAngle": 0.3, "outerConeAngle": 0.7}},
          {"type": "directional", "color": [0.9, 0.8, 0.7], "intensity": 2.5},
          {"type": "spot"}]   # every default: white, intensity 1, unlimited, inner 0, outer pi/4


def _nodes():
    q1, q2, q3 = _quat((1, 2, 3), 0.9), _quat((0, 1, 0), 2.2), _quat((1, 0, 0), -np.pi / 2)
    nodes = [light_node(0, translation=[1.5, -2.0, 3.25], rotation=list(q1), scale=[2.0, 0.5, 3.0]),
             {"mesh": 0},
             light_node(1, translation=[-4.0, 6.0, 0.5], rotation=list(q2), scale=[1.0, 1.0, 0.25]),
             light_node(2, rotation=list(q3), scale=[3.0, 3.0, 3.0]),
             light_node(3)]
    return nodes, (q1, q2, q3)


@pytest.mark.parametrize("glb", [False, True])
def test_loader_places_the_three_types(glb):
    nodes, (q1, q2, q3) = _nodes()
    s = lp.Scene()
    lp.loaders.load_gltf(make_gltf(nodes, LIGHTS, glb=glb), s)
    L = s.punctual_lights
    assert len(L) == 4 and s.counts().instances == 2
    assert [int(l["position"][3]) for l in L] == [0, 1, 2, 1]
    # position = the node's translation; direction = R·S applied to (0, 0, -1), normalised (a uniform or z-only scale leaves R·(0,0,-1))
    assert np.allclose(L[0]["position"][:3], (1.5, -2.0, 3.25), atol=1e-6) and np.allclose(L[2]["position"][:3], 0, atol=1e-6)
    for l, q in ((L[0], q1), (L[1], q2), (L[2], q3)):
        assert np.allclose(l["direction"][:3], _rotate(q, (0, 0, -1)), atol=1e-6)
    assert np.allclose(L[2]["direction"][:3], (0, -1, 0), atol=1e-6)          # -Z turned by -90 degrees about X: straight down
    assert np.allclose(L[1]["position"][:3], (-4.0, 6.0, 0.5), atol=1e-6)
    assert np.allclose(L[0]["color"], (40.0, 20.0, 10.0, 0)) and L[0]["direction"][3] == 12.5
    assert np.allclose(L[1]["color"], (7, 7, 7, 0)) and L[1]["direction"][3] == 0
    assert np.allclose(L[1]["cone"][:2], (np.cos(0.7), 1.0 / (np.cos(0.3) - np.cos(0.7))), rtol=1e-6)
    assert np.allclose(L[2]["color"], (2.25, 2.0, 1.75, 0), rtol=1e-6) and tuple(L[2]["cone"]) == (-2, 1, 0, 0)
    # the defaults
    assert tuple(L[3]["position"]) == (0, 0, 0, 1) and tuple(L[3]["direction"]) == (0, 0, -1, 0) and tuple(L[3]["color"]) == (1, 1, 1, 0)
    assert np.allclose(L[3]["cone"][:2], (np.cos(np.pi / 4), 1.0 / (1.0 - np.cos(np.pi / 4))), rtol=1e-6)
    # append semantics: a second load adds to the first
    lp.loaders.load_gltf(make_gltf(nodes[:2], LIGHTS[:1], glb=glb), s)
    L2 = s.punctual_lights
    assert len(L2) == 5 and L2[:4].tobytes() == L.tobytes() and L2[4].tobytes() == L[0].tobytes()


def test_loader_uses_an_explicit_matrix_like_a_mesh_node():
    m = np.eye(4)
    m[:3, :3] = [[0, 0, 1], [0, 1, 0], [-1, 0, 0]]   # +90 degrees about Y: -Z goes to -X
    m[:3, 3] = (7, 8, 9)
    s = lp.Scene()
    lp.loaders.load_gltf(make_gltf([light_node(0, matrix=list(m.T.reshape(-1)))], [{"type": "directional"}]), s)
    l = s.punctual_lights[0]
    assert np.allclose(l["direction"][:3], (-1, 0, 0), atol=1e-7) and np.allclose(l["position"][:3], (7, 8, 9))


MALFORMED = [
    ([light_node(1)], [{"type": "point"}]),                                                # light index out of range
    ([light_node(-1)], [{"type": "point"}]),
    ([light_node(0.5)], [{"type": "point"}]),
    ([light_node(0)], [{"type": "area"}]),                                                 # unknown type
    ([light_node(0)], [{}]),
    ([light_node(0)], [{"type": "spot", "spot": {"innerConeAngle": 0.5, "outerConeAngle": 0.5}}]),   # outer <= inner
    ([light_node(0)], [{"type": "spot", "spot": {"innerConeAngle": 0.9}}]),                # ... against the default outer
    ([light_node(0)], [{"type": "point", "intensity": 1e999}]),                            # non-finite
    ([light_node(0)], [{"type": "point", "intensity": -1.0}]),
    ([light_node(0)], [{"type": "point", "range": -1.0}]),
    ([light_node(0)], [{"type": "point", "color": [1.0, 1.0]}]),
    ([light_node(0, translation=[1e39, 0, 0])], [{"type": "point"}]),                      # overflows fp32
    ([light_node(0, scale=[1, 1, 0])], [{"type": "spot"}]),                                # no direction left
    ([light_node(0)], None),                                                               # a node names a light the file does not carry
]


@pytest.mark.parametrize("case", range(len(MALFORMED)))
def test_loader_rejects_malformed_lights(case):
    nodes, lights = MALFORMED[case]
    s = lp.Scene()
    s.add_punctual_light(lp.point_light((1, 1, 1)))
    before = (s.punctual_lights.tobytes(), s.instances.tobytes(), s.vertices.tobytes())
    with pytest.raises(lp.Error) as e:
        lp.loaders.load_gltf(make_gltf([{"mesh": 0}] + nodes, lights), s)
    assert e.value.kind == "FileNotFound"
    assert (s.punctual_lights.tobytes(), s.instances.tobytes(), s.vertices.tobytes()) == before


def test_files_without_the_extension_load_as_before():
    s = lp.Scene()
    lp.loaders.load_gltf(make_gltf([{"mesh": 0}]), s)
    assert s.punctual_count() == 0 and s.counts().instances == 2
    # lights the file declares but no node uses add nothing
    lp.loaders.load_gltf(make_gltf([{"mesh": 0}], LIGHTS), s)
    assert s.punctual_count() == 0 and s.counts().instances == 3
    # the committed Cornell box: no punctual lights, and the arrays the oracle's independent loader reads from the same bytes
    from oracle import gltf_oracle as G
    data = open(os.path.join(ROOT, "tests", "golden", "cornell-box.glb"), "rb").read()
    c = lp.Scene()
    lp.loaders.load_gltf(data, c)
    assert c.punctual_count() == 0
    o = G.Scene()
    G.load_gltf(data, o)
    for name in ("materials", "entries", "vertices", "indices", "instances", "lights"):
        assert getattr(c, name).tobytes() == getattr(o, name).tobytes(), name


# ---------------------------------------------------------------- the float64 reference at its corners, by hand
def test_reference_corners():
    spot = R.make(R.SPOT, position=(0, 2, 0), direction=(0, -1, 0), intensity=3.0, inner=0.2, outer=0.5)
    below = np.array([[0.0, 0.0, 0.0]])
    ok, wi, dist, E = R.incident(spot, below)
    assert ok[0] and np.allclose(wi[0], (0, 1, 0)) and dist[0] == 2.0 and np.allclose(E[0], 3.0 / 4.0)      # inside the inner cone: window 1
    on_outer = np.array([[2.0 * np.tan(0.5), 0.0, 0.0]])
    assert np.all(np.abs(R.incident(spot, on_outer)[3]) < 1e-25)                                           # exactly on the outer cone: 0 (to rounding of tan)
    assert R.cone_window(np.cos(0.5), np.cos(0.5), 5.0) == 0.0 and R.cone_window(np.cos(0.2), np.cos(0.5), 1.0 / (np.cos(0.2) - np.cos(0.5))) == 1.0
    half = 0.5 * (np.cos(0.2) + np.cos(0.5))
    assert R.cone_window(half, np.cos(0.5), 1.0 / (np.cos(0.2) - np.cos(0.5))) == pytest.approx(0.25)      # s = 1/2 -> s^2
    assert np.all(R.incident(spot, np.array([[0.0, 5.0, 0.0]]))[3] == 0)                                   # behind the spot
    point = R.make(R.POINT, position=(0, 0, 0), intensity=16.0, range=4.0)
    assert np.all(R.incident(point, np.array([[4.0, 0, 0]]))[3] == 0)                                      # d = range
    assert np.allclose(R.incident(point, np.array([[0, 2.0, 0]]))[3], 16.0 / 4.0 * 15.0 / 16.0)            # d = range / 2: 15/16
    assert np.all(R.incident(point, np.array([[0, 9.0, 0]]))[3] == 0)
    assert not R.incident(point, np.zeros((1, 3)))[0][0]                                                   # the point IS the light: no sample
    sun = R.make(R.DIRECTIONAL, direction=(1, -1, 0), color=(1, 0.5, 0.25), intensity=2.0, range=3.0)
    pts = np.array([[0, 0, 0], [1e3, -5, 7], [-3, 1e-3, 2]], np.float64)
    ok, wi, dist, E = R.incident(sun, pts)
    assert ok.all() and np.all(dist == R.T_INF) and np.all(E == np.array([2.0, 1.0, 0.5])) and np.allclose(wi, np.array([-1, 1, 0]) / np.sqrt(2))
    # pick probabilities: the shares add up to one
    for n_p, n, env in ((1, 1, False), (3, 1, False), (2, 5, True), (1, 0, True)):
        p_p, pp, pr = R.pick(n_p, n, env)
        assert p_p == n_p / (n_p + n) and (0.5 if env else 0.0) + n_p * pp + n * pr == pytest.approx(1.0)
    # the BSDF: a white Lambertian (roughness 1, metallic 0) seen and lit along the normal is (1 - F)/pi + D·Vis·F with F = 0.04
    f = R.bsdf((1, 1, 1), 1.0, 0.0, (0, 1, 0), (0, 1, 0), (0, 1, 0), np.array([[0, 1.0, 0]]))[0]
    assert np.allclose(f, (0.96 / np.pi) + (1.0 / np.pi) * (1.0 / 4.0) * 0.04)
    assert np.all(R.bsdf((1, 1, 1), 0.3, 0.5, (0, 1, 0), (0, 1, 0), (0, 1, 0), np.array([[0, -1.0, 0]])) == 0)
    # r0 of SPEC §4 is a uniform in [0, 1)
    r0 = R.r0_of(np.arange(4096), 1)
    assert r0.min() >= 0 and r0.max() < 1 and abs(r0.mean() - 0.5) < 0.03
