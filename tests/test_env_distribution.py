"""CPU: lpt_env_distribution (SPEC.md §18, the environment probe's sampling distribution built on the host) against the float64
restatement in tests/env_ref.py — pdf_uv, the probabilities the two alias tables imply, and the empty distribution of a black probe."""
import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import scenes

import env_ref


def _bright(w, h, x, y, e=140):
    a = np.zeros((h, w, 4), np.uint8)
    a[..., :3] = 40
    a[..., 3] = 128
    a[y, x] = (250, 240, 200, e)
    return a


def _random(w, h, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    a[..., 3] = rng.integers(120, 140, (h, w))
    return a


PROBES = {
    "sky": lambda: scenes.sky_probe(64, 32),
    "random": lambda: _random(48, 24, 3),
    "bright_x0": lambda: _bright(32, 16, 0, 7),
    "bright_xlast": lambda: _bright(32, 16, 31, 9),
    "bright_row0": lambda: _bright(32, 16, 5, 0),
    "bright_rowlast": lambda: _bright(32, 16, 20, 15),
    "low_exponents": lambda: np.dstack([_random(16, 8, 4)[..., :3], np.random.default_rng(6).integers(0, 14, (8, 16)).astype(np.uint8)]),
    "strip_w1": lambda: _random(1, 16, 7),
    "strip_h1": lambda: _random(16, 1, 8),
    "one_texel": lambda: np.array([[[10, 20, 30, 130]]], np.uint8),
}


@pytest.mark.parametrize("name", list(PROBES))
def test_distribution_matches_reference(name):
    rgbe = PROBES[name]()
    got = lp.env_distribution(rgbe)
    want, total = env_ref.distribution(rgbe)
    assert total > 0.0
    assert got["total"] == pytest.approx(total, rel=1e-12)
    np.testing.assert_allclose(got["pdf_uv"], want, rtol=1e-6, atol=1e-6 * want.max())
    # zero-weight texels stay at zero: the sampler must never pick them
    assert np.all(got["pdf_uv"][want == 0.0] == 0.0)
    w = env_ref.weights(rgbe)
    H, W = w.shape
    rows = w.sum(axis=1)
    np.testing.assert_allclose(env_ref.alias_probabilities(got["row_q"], got["row_alias"]), rows / rows.sum(), rtol=0, atol=1e-6)
    assert np.all(got["row_alias"] < H)
    for y in range(H):
        if rows[y] > 0:
            np.testing.assert_allclose(env_ref.alias_probabilities(got["col_q"][y], got["col_alias"][y]), w[y] / rows[y], rtol=0, atol=1e-6)
    assert np.all(got["col_alias"] < W)
    assert np.all((got["row_q"] >= 0) & (got["row_q"] <= 1)) and np.all((got["col_q"] >= 0) & (got["col_q"] <= 1))


def test_neighbourhood_max_wraps_and_clamps():
    """a bright texel at x = 0 lifts the weights of column W - 1 (wrap), one in row 0 only rows 0 and 1 (clamp)"""
    got = lp.env_distribution(_bright(32, 16, 0, 7))["pdf_uv"]
    assert got[7, 31] > 10 * got[7, 16] and got[6, 31] > 10 * got[7, 16]
    got = lp.env_distribution(_bright(32, 16, 5, 0))["pdf_uv"]
    assert got[1, 5] > 10 * got[2, 5]


def test_black_probe_has_no_distribution():
    for rgbe in (np.zeros((1, 1, 4), np.uint8), np.zeros((8, 16, 4), np.uint8), np.dstack([np.full((4, 8, 3), 200, np.uint8), np.full((4, 8, 1), 9, np.uint8)])):
        got = lp.env_distribution(rgbe)
        assert got["total"] == 0.0
        assert np.all(got["pdf_uv"] == 0.0)


def test_null_outputs_are_skipped():
    import ctypes as C
    from loupiote_amd import _abi as A
    rgbe = scenes.sky_probe(16, 8)
    total = C.c_double()
    assert A.lib().lpt_env_distribution(A.ptr(rgbe), 16, 8, None, None, None, None, None, C.byref(total)) == 0
    assert total.value > 0
    assert A.lib().lpt_env_distribution(None, 16, 8, None, None, None, None, None, None) == A.LPT_ERR_INVALID_ARG
