"""-m gpu: interactive instance edits (reference Instance::set_transform, standalone/src/lib.rs:118-121).

`SceneGPU.update_instances` re-bakes only the moved instances and refits the wide BVH on the GPU.  Hits do not
depend on the tree (SPEC §7), so the refitted scene must give exactly what a fresh upload of the edited scene —
and the oracle, which rebuilds from scratch — gives."""
import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import scenes, testing as T

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("pipeline")]   # every test body over the three arms of tests/conftest.py PIPELINES: k_path, the per-bounce launches, the shipped defaults


def _trs(angle, t, s=1.0):
    c, sn = np.cos(angle), np.sin(angle)
    m = np.eye(4, dtype=np.float32)
    m[:3, :3] = np.array([[c, 0, sn], [0, 1, 0], [-sn, 0, c]], np.float32) * np.float32(s)
    m[:3, 3] = t
    return np.ascontiguousarray(m.T).reshape(-1)      # column-major


def _render(device, sg, w, h, bounces, frames):
    pr = lp.ProbeGPU(device, T.CORNELL_PROBE, 1, 1)
    r = lp.Renderer(device, (w, h))
    r.downsample_factor = 1.0
    r.resize(device, sg, pr, (w, h))
    r.set_max_bounces(bounces)
    r.set_vfov(T.VFOV)
    r.reset_accumulation()
    r.accumulate = True
    r.reset_ray_counts()
    view = T.look(T.CORNELL_EYE, T.CORNELL_DIR)
    for _ in range(frames):
        r.raytrace(view)
    img, counts = r.read_radiance(), r.ray_counts()
    r.close(); pr.close()
    return img, counts


def test_moved_instances_refit_equals_fresh_upload_and_oracle(device, cornell_glb):
    from oracle import gltf_oracle as G, orc
    scene = lp.Scene()
    lp.loaders.load_gltf(cornell_glb, scene)
    scene.set_light(0, T.cornell_light())
    sg = lp.SceneGPU.new_from_scene(scene, device)
    before, _ = _render(device, sg, 128, 128, 4, 2)
    assert sg.update_instances(scene) == 0                      # nothing moved: nothing to do
    n_inst = scene.counts().instances
    moves = {n_inst - 1: _trs(0.5, (0.8, 0.9, 0.6), 0.8), n_inst - 2: _trs(-0.3, (-0.9, 0.0, -0.5))}
    osc = G.Scene()
    G.load_gltf(cornell_glb, osc)
    osc.lights[0] = T.cornell_light()[0]
    for idx, m in moves.items():
        base = scene.instances[idx]["model_to_world"].reshape(-1).copy()
        new = (m.reshape(4, 4).T @ base.reshape(4, 4).T).T.astype(np.float32).reshape(-1)   # move in world space
        scene.set_instance_transform(idx, new)
        osc.instances[idx]["model_to_world"] = new.reshape(osc.instances[idx]["model_to_world"].shape)
    assert sg.update_instances(scene) == 2
    refit, c_refit = _render(device, sg, 128, 128, 4, 2)
    assert refit.tobytes() != before.tobytes()
    fresh_sg = lp.SceneGPU.new_from_scene(scene, device)
    fresh, c_fresh = _render(device, fresh_sg, 128, 128, 4, 2)
    assert refit.tobytes() == fresh.tobytes()
    assert (c_refit.closest, c_refit.shadow, c_refit.shaded) == (c_fresh.closest, c_fresh.shadow, c_fresh.shaded)
    sc = orc.OracleScene.from_scene(osc, probe=T.CORNELL_PROBE)
    acc, oc = sc.render(128, 128, T.look(T.CORNELL_EYE, T.CORNELL_DIR), T.VFOV, 4, frames=2, want_counters=True)
    assert refit.tobytes() == orc.resolve(acc).tobytes()
    assert (c_refit.closest, c_refit.shadow, c_refit.shaded) == (oc.closest, oc.shadow, oc.shaded)
    # random rays: closest hits of the refitted tree == those of the rebuilt tree
    rng = np.random.default_rng(5)
    o = np.zeros((20000, 4), np.float32); d = np.zeros((20000, 4), np.float32)
    o[:, :3] = rng.uniform(-2.5, 2.5, (20000, 3))
    v = rng.normal(size=(20000, 3)); d[:, :3] = v / np.linalg.norm(v, axis=1, keepdims=True)
    assert sg.trace_closest(o, d).tobytes() == fresh_sg.trace_closest(o, d).tobytes()
    # moving back restores the original picture (the refit is not cumulative)
    lp.loaders  # noqa
    scene2 = lp.Scene()
    lp.loaders.load_gltf(cornell_glb, scene2)
    scene2.set_light(0, T.cornell_light())
    for idx in moves:
        scene.set_instance_transform(idx, scene2.instances[idx]["model_to_world"].reshape(-1))
    assert sg.update_instances(scene) == 2
    again, _ = _render(device, sg, 128, 128, 4, 2)
    assert again.tobytes() == before.tobytes()
    fresh_sg.close(); sg.close()


def test_refit_rejects_a_changed_instance_list(device, cornell_glb):
    scene = lp.Scene()
    lp.loaders.load_gltf(cornell_glb, scene)
    sg = lp.SceneGPU.new_from_scene(scene, device)
    scene.add_instance(1, np.eye(4, dtype=np.float32).reshape(-1), 0)
    with pytest.raises(lp.Error) as e:
        sg.update_instances(scene)
    assert e.value.kind == "InvalidArg"
    sg.close()


def test_non_finite_transform_raises_and_the_scene_recovers(device, cornell_glb):
    """A NaN / inf transform is an AccelBuild error from update_instances, rebuild and a GPU-built upload (the bake checks every vertex before
    any kernel reads the triangles); the flag is reset, so the next valid edit of the same instance works: the scene then traces and renders
    like a fresh upload"""
    scene = lp.Scene()
    lp.loaders.load_gltf(cornell_glb, scene)
    scene.set_light(0, T.cornell_light())
    sg = lp.SceneGPU.new_from_scene(scene, device)
    idx = scene.counts().instances - 1
    base = scene.instances[idx]["model_to_world"].reshape(-1).copy()
    bad = base.copy()
    bad[12], bad[13] = np.nan, np.inf
    rng = np.random.default_rng(11)
    o = np.zeros((20000, 4), np.float32); d = np.zeros((20000, 4), np.float32)
    o[:, :3] = rng.uniform(-2.5, 2.5, (20000, 3))
    v = rng.normal(size=(20000, 3)); d[:, :3] = v / np.linalg.norm(v, axis=1, keepdims=True)

    def raises_accel_build(call):
        with pytest.raises(lp.Error) as e:
            call()
        assert e.value.kind == "AccelBuild"

    def same_as_fresh():
        fresh = lp.SceneGPU.new_from_scene(scene, device)
        assert sg.trace_closest(o, d).tobytes() == fresh.trace_closest(o, d).tobytes()
        img, c = _render(device, sg, 96, 96, 3, 1)
        ref, c_ref = _render(device, fresh, 96, 96, 3, 1)
        assert img.tobytes() == ref.tobytes() and (c.closest, c.shadow) == (c_ref.closest, c_ref.shadow)
        fresh.close()

    scene.set_instance_transform(idx, bad)
    raises_accel_build(lambda: sg.update_instances(scene))
    scene.set_instance_transform(idx, (_trs(0.5, (0.8, 0.9, 0.6), 0.8).reshape(4, 4).T @ base.reshape(4, 4).T).T.astype(np.float32).reshape(-1))
    assert sg.update_instances(scene) == 1                       # the failed edit was recorded: the valid one re-bakes the instance
    same_as_fresh()

    scene.set_instance_transform(idx, bad)
    raises_accel_build(lambda: sg.rebuild(scene))
    scene.set_instance_transform(idx, (_trs(-0.3, (-0.9, 0.0, -0.5)).reshape(4, 4).T @ base.reshape(4, 4).T).T.astype(np.float32).reshape(-1))
    sg.rebuild(scene)
    assert sg.update_instances(scene) == 0
    same_as_fresh()

    scene.set_instance_transform(idx, bad)
    raises_accel_build(lambda: lp.SceneGPU.new_from_scene(scene, device, gpu_build=True))
    sg.close()

def test_refit_large_scene_statue_moves(device):
    """atrium: move one ~7k-triangle instance; refit == fresh upload on 100k random rays and a 480x270 frame"""
    desc = scenes.synthetic_atrium(textures=False)
    scene = scenes.to_product(desc)
    sg = lp.SceneGPU.new_from_scene(scene, device)
    counts = scene.counts()
    idx = counts.instances - 2
    m = scene.instances[idx]["model_to_world"].reshape(-1).copy()
    m[12] += 1.5; m[13] += 0.25; m[14] -= 2.0
    scene.set_instance_transform(idx, m)
    assert sg.update_instances(scene) == 1
    fresh = lp.SceneGPU.new_from_scene(scene, device)
    rng = np.random.default_rng(9)
    n = 100000
    o = np.zeros((n, 4), np.float32); d = np.zeros((n, 4), np.float32)
    o[:, :3] = rng.uniform((-12, 0.2, -6), (12, 9, 6), (n, 3))
    v = rng.normal(size=(n, 3)); d[:, :3] = v / np.linalg.norm(v, axis=1, keepdims=True)
    a, b = sg.trace_closest(o, d), fresh.trace_closest(o, d)
    assert a.tobytes() == b.tobytes() and (a["prim"] != 0xFFFFFFFF).mean() > 0.5
    fresh.close(); sg.close()


# ---------------------------------------------------------------- the four material side tables (SPEC §20, §21, §22, §24) and the emitter distribution (§23) follow the edits
def _quad(scene, x, mat, z=-3.0, half=0.35):
    pos = np.array([[x - half, -half, z], [x + half, -half, z], [x + half, half, z], [x - half, half, z]], np.float32)
    nrm = np.tile(np.float32([[0, 0, 1]]), (4, 1))
    uv = np.array([(0, 0), (1.5, 0), (1.5, 1.5), (0, 1.5)], np.float32)
    return scene.add_instance(scene.add_mesh(pos, nrm, uv, np.array([0, 1, 2, 0, 2, 3], np.uint32)), np.eye(4, dtype=np.float32), mat)


def _nudged(dy):
    m = np.eye(4, dtype=np.float32)
    m[1, 3] = dy
    return m.T


def _table_frame(device, sg, probe):
    """64x36 pixels, 4 samples, a fixed seed, emitter sampling on"""
    r = lp.Renderer(device, (64, 36))
    r.downsample_factor = 1.0
    r.resize(device, sg, probe, (64, 36))
    r.set_max_bounces(3)
    r.set_vfov(0.6)
    r.set_seed(11)
    r.set_emissive_sampling(True)
    r.reset_accumulation()
    r.accumulate = True
    view = T.look((0.0, 0.0, 0.0), (0.0, 0.0, -1.0))
    for _ in range(4):
        r.raytrace(view)
    img = r.read_radiance()
    r.close()
    return img


@pytest.mark.parametrize("big", [False, True], ids=["fewer-than-16-triangles", "16-triangles-and-more"])
def test_material_tables_follow_update_and_rebuild(device, big):
    """a masked, a glass, an emissive (with an image) and a normal-mapped material on four instances; the features change places by an instance update, then by a
    rebuild (its refit arm below 16 triangles, its GPU build from 16 on): every frame is that of a fresh upload of the scene as edited.  An edit that names an image
    uploaded only as half of a pair is InvalidArg and leaves the scene on the device as it was"""
    rng = np.random.RandomState(31)
    mask = rng.randint(0, 256, (4, 4, 4)).astype(np.uint8)
    glow = rng.randint(0, 256, (4, 4, 4)).astype(np.uint8)
    bump = rng.randint(64, 192, (5, 3, 4)).astype(np.uint8)
    bump[..., 2] = 230
    s = lp.Scene()
    dark = np.zeros(1, lp._abi.LIGHT_DT)
    dark["normal"], dark["tangent"], dark["bitangent"], dark["origin"] = (0, -1, 0, 0), (1, 0, 0, 0.1), (0, 0, 1, 0.1), (0, -50.0, 0, 0.0)
    s.set_light(0, dark)
    i_mask, i_glow, i_bump = s.add_image(mask), s.add_image(glow), s.add_image(bump)
    i_pa, i_pb = s.add_image(rng.randint(0, 256, (4, 4, 4)).astype(np.uint8)), s.add_image(rng.randint(0, 256, (4, 4, 4)).astype(np.uint8))
    mats = [s.add_material((0.9, 0.8, 0.7, 1.0), 0.6, 0.0) for _ in range(4)]
    inst = [_quad(s, x, m) for x, m in zip((-1.2, -0.4, 0.4, 1.2), mats)]
    _quad(s, 0.0, s.add_material((0.7, 0.7, 0.9, 1.0), 0.9, 0.0), z=-4.0, half=2.5)                 # a backdrop: what the cut-away texels and the glass show
    _quad(s, 0.0, s.add_material((1.0, 1.0, 1.0, 1.0), 1.0, 0.0, i_pa, i_pb), z=-3.5, half=0.2)    # (i_pa, i_pb) is a pair: neither image is resident on its own
    if big:
        g = np.linspace(-2.5, 2.5, 4, dtype=np.float32)
        pos = np.array([[x, -0.8, z - 3.0] for z in g for x in g], np.float32)
        idx = np.array([[a, a + 1, a + 5, a, a + 5, a + 4] for a in (j * 4 + i for j in range(3) for i in range(3))], np.uint32).reshape(-1)
        s.add_instance(s.add_mesh(pos, np.tile(np.float32([[0, 1, 0]]), (16, 1)), None, idx), np.eye(4, dtype=np.float32), s.add_material((0.5, 0.5, 0.5, 1.0), 1.0, 0.0))

    def assign(order):
        """material mats[order[k]] gets feature k (mask, glass, emission, normal map) and no other"""
        for m in mats:
            s.set_material_alpha(m, "OPAQUE")
            s.set_material_transmission(m, 0.0)
            s.set_material_emission(m, 0.0)
            s.set_material_normal_map(m, None)
        s.set_material_alpha(mats[order[0]], "MASK", 0.5, i_mask)
        s.set_material_transmission(mats[order[1]], 1.0, 1.5, True)
        s.set_material_emission(mats[order[2]], (1.0, 0.5, 0.25), 2.0, i_glow)
        s.set_material_normal_map(mats[order[3]], i_bump, 2.0)

    assign((0, 1, 2, 3))
    sg = lp.SceneGPU.new_from_scene(s, device)
    assert (sg.stats().triangles >= 16) == big and sg.stats().texture_pairs == 1
    probe = lp.ProbeGPU(device, np.array([[[128, 128, 128, 128]]], np.uint8), 1, 1)
    seen = []

    def check():
        fresh_sg = lp.SceneGPU.new_from_scene(s, device)
        got, fresh = _table_frame(device, sg, probe), _table_frame(device, fresh_sg, probe)
        fresh_sg.close()
        assert np.all(np.isfinite(fresh)) and got.tobytes() == fresh.tobytes()
        assert all(fresh.tobytes() != f.tobytes() for f in seen)      # every edit shows
        seen.append(fresh)

    check()
    assign((1, 2, 3, 0))                                  # the features move one instance on, by an instance update
    for i in inst:
        s.set_instance_transform(i, _nudged(0.02))
    assert sg.update_instances(s) == 4
    check()
    assign((3, 0, 1, 2))                                  # ... and again, by a rebuild that finds no instance changed
    sg.rebuild(s)
    check()
    before = seen[-1]
    # a pair-only image: each of the three kinds that name an image refuses it, by an update and by a rebuild, before anything on the device changed
    edits = [lambda: s.set_material_alpha(mats[3], "MASK", 0.5, i_pa), lambda: s.set_material_emission(mats[1], (1.0, 0.5, 0.25), 2.0, i_pb),
             lambda: s.set_material_normal_map(mats[2], i_pa, 2.0)]
    for edit in edits:
        for call in (sg.update_instances, sg.rebuild):
            edit()
            s.set_instance_transform(inst[0], _nudged(0.3))
            with pytest.raises(lp.Error) as e:
                call(s)
            assert e.value.kind == "InvalidArg" and "only as half of an (albedo, mra) pair" in str(e.value)
            assert _table_frame(device, sg, probe).tobytes() == before.tobytes()
            s.set_instance_transform(inst[0], _nudged(0.02))
            assign((3, 0, 1, 2))
    assert sg.update_instances(s) == 0
    assert _table_frame(device, sg, probe).tobytes() == before.tobytes()
    probe.close()
    sg.close()
