"""CPU: the emitter distribution of SPEC.md §23 through the host hook lpt_scene_emitter_distribution (no GPU): which triangles are entries and in which order, the
weights following an instance's scale, the alias table against the weights and against tests/emitter_ref.py, a scene without a distribution, and the switch's null
arguments.  The scenes come from tests/emitter_scenes.py."""
import ctypes as C

import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import _abi as A

import emitter_ref as R

from emitter_scenes import F, QUAD, QUAD_IDX, Built, dark_light, many_scene, mixed_scene, scaled  # noqa: F401


# ---------------------------------------------------------------- 1. entries and order
def test_entries_are_the_emissive_triangles_with_an_area_in_prim_order():
    b = mixed_scene()
    d = b.s.emitter_distribution()
    assert d["prim"].tolist() == [3, 4] and len(d["q"]) == 2 and d["sum_w"] > 0
    assert np.array_equal(d["prim_alias"], d["prim"][d["alias"]])
    ref = b.reference()
    assert ref["prim"].tolist() == [3, 4] and d["sum_w"] == ref["sum_w"]
    # the quad is 1 x 1: each half has area 1/2, weight 1/2 lum(Le)
    assert abs(d["sum_w"] - float(R.lum(F([2.0, 1.0, 4.0])))) <= 4 * 2.0 ** -24 * d["sum_w"]


def test_an_instance_scaled_by_two_has_four_times_the_weight():
    one, two = mixed_scene(1.0).s.emitter_distribution(), mixed_scene(2.0).s.emitter_distribution()
    assert two["prim"].tolist() == [3, 4]
    assert two["sum_w"] == 4.0 * one["sum_w"]                # a power of two: exact in binary32 and binary64
    w1, w2 = R.pmf(one["q"], one["alias"]) * one["sum_w"], R.pmf(two["q"], two["alias"]) * two["sum_w"]
    assert np.allclose(w2, 4.0 * w1, rtol=2 * 2.0 ** -24, atol=0)


# ---------------------------------------------------------------- 2. the alias table
@pytest.mark.parametrize("n_e", [1, 2, 130])
def test_alias_table_reproduces_the_weights(n_e):
    """THE BOUND, derived: q is the binary32 rounding of a number in [0, 1], so a column's kept share q/n is off by at most 2^-25/n absolutely.  Entry i gets its own
    column's share and (1 - q_s)/n of every column s whose alias it is — at most n columns in all, 2^-25 absolutely; an entry that is some column's alias was `large`
    (p_i >= 1/n), so that is n 2^-25 <= n 2^-24 relative, and an entry that is no column's alias has its own q alone, 2^-24 relative.  The binary64 build adds one
    rounding per scaled weight, per subtraction (at most n of them on a value of at most n, in units of 1/n of the pmf) and per term of the sum: 4 n 2^-53 absolutely."""
    b = many_scene(n_e)
    d, ref = b.s.emitter_distribution(), b.reference()
    assert len(d["q"]) == n_e == len(ref["prim"])
    assert np.array_equal(d["prim"], ref["prim"]) and np.array_equal(d["alias"], ref["alias"]) and np.all(np.diff(d["prim"].astype(np.int64)) > 0)
    assert np.array_equal(d["prim_alias"], ref["prim"][ref["alias"]])
    ulp = np.spacing(np.maximum(np.abs(ref["q"]), np.finfo(F).tiny).astype(F))
    assert np.all(np.abs(d["q"].astype(np.float64) - ref["q"].astype(np.float64)) <= ulp)
    assert np.all((d["q"] >= 0) & (d["q"] <= 1)) and np.all(d["alias"] < n_e)
    want = ref["w"] / ref["sum_w"]
    got = R.pmf(d["q"], d["alias"])
    tol = n_e * 2.0 ** -24 * want + 4 * n_e * 2.0 ** -53
    print("n_e %d: largest |pmf - w/W| / bound %.3g, smallest share %.3g" % (n_e, float((np.abs(got - want) / tol).max()), want.min()))
    assert np.all(np.abs(got - want) <= tol)
    assert abs(d["sum_w"] - ref["sum_w"]) <= 2.0 ** -52 * ref["sum_w"]
    if n_e == 2:
        assert abs(want[1] / want[0] - 1.0e6) < 1.0


# ---------------------------------------------------------------- 3. no distribution
def test_no_emission_means_no_distribution():
    b = Built()
    b.mesh(QUAD, QUAD_IDX, b.material())
    b.mesh(QUAD + F([0, 1, 0]), QUAD_IDX, b.material((0.0, 0.0, 0.0)))
    d = b.s.emitter_distribution()
    assert len(d["q"]) == 0 and d["sum_w"] == 0.0 and b.reference() is None
    e = lp.Scene().emitter_distribution()                     # Scene::default()
    assert len(e["prim"]) == 0 and e["sum_w"] == 0.0
    z = Built()                                               # an emissive material on a triangle without an area alone
    z.mesh(F([[0, 0, 0], [1, 1, 1], [2, 2, 2]]), [0, 1, 2], z.material((1.0, 1.0, 1.0)))
    assert len(z.s.emitter_distribution()["q"]) == 0


# ---------------------------------------------------------------- 4. null arguments
def test_null_arguments_are_rejected():
    L, f, n = A.lib(), C.c_int(7), C.c_uint32()
    assert L.lpt_renderer_set_emissive_sampling(None, 1) == A.LPT_ERR_INVALID_ARG
    assert L.lpt_renderer_get_emissive_sampling(None, C.byref(f)) == A.LPT_ERR_INVALID_ARG and f.value == 7
    assert L.lpt_scene_emitter_distribution(None, 0, None, None, None, None, C.byref(n), None) == A.LPT_ERR_INVALID_ARG
    s = lp.Scene()
    assert L.lpt_scene_emitter_distribution(s._h, 0, None, None, None, None, None, None) == A.LPT_ERR_INVALID_ARG
    assert L.lpt_scene_gpu_sample_emitter(None, None, 0, None, None, None, None, None, None, None, None, None, None) == A.LPT_ERR_INVALID_ARG


# ---------------------------------------------------------------- 5. the reference's own path estimator against its quadrature
def test_the_path_estimator_of_the_reference_reproduces_its_quadrature():
    """emitter_ref.last_bounce_shift at depth 1 is the direct light on what the camera sees: over the lamp-and-floor scene of tests/test_gpu_emitter_sampling.py it must give
    floor_window_mean's integral, within 5 of its standard errors plus the quadrature's stated error.  (The GPU test of depth 3 uses the estimator to size a wrong rule.)"""
    from loupiote_amd import testing as T
    view = T.look((0.0, 1.0, 0.5), (0.0, -0.7, -1.0))
    rows, cols = slice(8, 28), slice(12, 52)
    lamp = R.rect((0.0, 1.5, -3.0), (1, 0, 0), (0, 0, 1), 0.5, 0.5, 0.0, 8.0)
    floor = R.rect((0.0, 0.0, -3.0), (0, 0, 1), (1, 0, 0), 4.0, 4.0, 1.0)
    got, se = R.last_bounce_shift(view, 0.6, 64, 36, rows, cols, [lamp, floor], lamp, depth=1, spp=16)
    want, qerr = R.floor_window_mean(view, 0.6, 64, 36, rows, cols, 0.0, 1.0, dict(center=(0.0, 1.5, -3.0), eu=(1, 0, 0), ev=(0, 0, 1), hu=0.5, hv=0.5), 8.0, sub=2, order=16)
    assert se < 1.0e-3 * want and abs(got - want) <= 5 * se + qerr, (got, se, want, qerr)
