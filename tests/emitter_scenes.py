"""Scenes for the tests of SPEC.md §23 (emitter sampling), shared by tests/test_emitter_sampling.py (host) and tests/test_gpu_emitter_sampling.py (device): scenes of
explicit meshes that keep what tests/emitter_ref.py needs of them.  Test infrastructure only."""
import numpy as np

import loupiote_amd as lp
from loupiote_amd import _abi as A

import emitter_ref as R

F = np.float32
QUAD_IDX = np.array([0, 1, 2, 0, 2, 3], np.uint32)


def dark_light():
    """the scene's one rectangle light switched off, far below everything and facing away: n_lights = 1, nothing emitted, nothing hidden"""
    l = np.zeros(1, A.LIGHT_DT)
    l["normal"], l["tangent"], l["bitangent"], l["origin"] = (0, -1, 0, 0), (1, 0, 0, 0.1), (0, 0, 1, 0.1), (0, -50.0, 0, 0.0)
    return l


def scaled(s, t=(0.0, 0.0, 0.0)):
    m = np.diag([s, s, s, 1.0]).astype(F)
    m[:3, 3] = t
    return m.T                       # the API takes model_to_world column-major


class Built:
    """a scene of explicit meshes, and what the reference needs of it: every baked triangle in prim-id order (binary32), its vertex uv and its material's record"""

    def __init__(self):
        self.s = lp.Scene()
        self.s.set_light(0, dark_light())
        self.tris, self.uv, self.rec, self.images = [], [], [], []

    def material(self, le=None, image=None, base=(0.0, 0.0, 0.0, 1.0)):
        m = self.s.add_material(base, 1.0, 0.0)
        rec = None
        if le is not None:
            self.s.set_material_emission(m, le, 1.0, image)
            le32 = np.broadcast_to(np.asarray(le, F), (3,)) * F(1.0)
            rec = (le32, image) if le32.any() else None
        return m, rec

    def image(self, img):
        self.images.append(img)
        return self.s.add_image(img)

    def mesh(self, pos, idx, mat, uv=None, m2w=None):
        pos, idx = np.asarray(pos, F), np.asarray(idx, np.uint32)
        uv = np.zeros((len(pos), 2), F) if uv is None else np.asarray(uv, F)
        m2w = np.eye(4, dtype=F) if m2w is None else m2w
        n = np.tile(F([[0, 0, 1]]), (len(pos), 1))
        inst = self.s.add_instance(self.s.add_mesh(pos, n, uv, idx), m2w, mat[0])
        self.tris += list(R.bake(pos, idx, m2w))
        self.uv += list(uv[idx.astype(np.int64)].reshape(-1, 3, 2))
        self.rec += [mat[1]] * (len(idx) // 3)
        return inst

    def reference(self):
        return R.distribution(np.array(self.tris, F), [None if r is None else r[0] for r in self.rec])


QUAD = F([[-0.5, 1.0, -3.5], [0.5, 1.0, -3.5], [0.5, 1.0, -2.5], [-0.5, 1.0, -2.5]])


def mixed_scene(scale=1.0):
    """a non-emissive quad (prims 0, 1), an emissive triangle of zero area (prim 2), an emissive quad (prims 3, 4), and an emissive material that no instance uses"""
    b = Built()
    plain, lamp, _unused = b.material(), b.material((2.0, 1.0, 4.0)), b.material((9.0, 9.0, 9.0))
    b.mesh(QUAD - F([0, 1, 0]), QUAD_IDX, plain)
    b.mesh(F([[0, 0, 0], [1, 1, 1], [2, 2, 2]]), [0, 1, 2], lamp)
    b.mesh(QUAD, QUAD_IDX, lamp, m2w=scaled(scale))
    return b


def many_scene(n_e, image=None):
    """n_e emissive triangles of different areas over three materials (the second one textured when an image is given), as one instance per material, behind two
    non-emissive triangles; n_e = 2: equal areas with Le 1 : 10^6"""
    b = Built()
    b.mesh(QUAD - F([0, 1, 0]), QUAD_IDX, b.material())
    rs = np.random.RandomState(230 + n_e)
    if n_e == 2:
        for le in (1.0, 1.0e6):
            b.mesh(F([[0, 1, -3], [1, 1, -3], [0, 1, -2]]), [0, 1, 2], b.material((le, le, le)))
        return b
    img = None if image is None else b.image(image)
    mats = [b.material((2.0, 1.0, 4.0)), b.material((0.5, 3.0, 0.25), img), b.material((0.0, 0.0, 7.0))][:min(n_e, 3)]
    share = [n_e - 2 * (n_e // 3), n_e // 3, n_e // 3] if n_e >= 3 else [n_e]
    for mat, k in zip(mats, share):
        pos = (rs.uniform(-1.0, 1.0, (3 * k, 3)) * rs.uniform(0.05, 1.0, (k, 1)).repeat(3, 0) + F([0.0, 1.5, -3.0])).astype(F)
        b.mesh(pos, np.arange(3 * k), mat, uv=rs.uniform(0.0, 2.5, (3 * k, 2)).astype(F))
    return b
