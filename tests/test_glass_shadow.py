"""SPEC.md §27 (shadows through thin glass), the reference alone (tests/glass_shadow_ref.py; no device): the threshold xi is uniform enough that a pane passes
a channel with probability tau, it is independent of §26's xi at the same hit, the binary32 tau stays within its derived bound of the binary64 one, and the
Fresnel term is the textbook's.

THE BOUNDS.  A share over n hits is a binomial count: 5 standard deviations, sqrt(tau (1 - tau) / n).  A sample correlation of n independent pairs has standard
deviation 1/sqrt(n): 5 of them.  binary32 against binary64: glass_shadow_ref.tau_bound, derived there from the count of roundings.  None is tuned."""
import numpy as np
import pytest

import blend_ref
import glass_shadow_ref as G

F = np.float32
N = 1 << 20
PRIMS = (0, 1, 37)
TAUS = (0.04, 0.25, 0.5, 0.9216, 0.999)


def _hits(kind):
    rng = np.random.default_rng(27)
    if kind == "uniform":
        u = rng.random(N, F)
        v = (rng.random(N, F) * (F(1) - u)).astype(F)
    elif kind == "grid":
        g = (np.arange(1024, dtype=F) + F(0.5)) / F(2048)
        u, v = (a.reshape(-1).astype(F) for a in np.meshgrid(g, g))
    else:       # an edge of the triangle: v = 0
        u, v = ((np.arange(N, dtype=F) + F(0.5)) / F(N)).astype(F), np.zeros(N, F)
    assert u.shape == (N,) and v.shape == (N,)
    return u, v


@pytest.fixture(scope="module", params=["uniform", "grid", "v0"])
def hits(request):
    return _hits(request.param)


def test_xi_is_one_of_the_2_24_fractions_in_0_1(hits):
    u, v = hits
    x = G.xi(5, u, v)
    assert x.dtype == F and x.min() >= 0 and x.max() < 1
    assert np.array_equal(x * F(2.0 ** 24), np.floor(x * F(2.0 ** 24)))


@pytest.mark.parametrize("prim", PRIMS)
def test_a_channel_passes_with_probability_tau(hits, prim):
    u, v = hits
    x = G.xi(prim, u, v)
    for t in TAUS:
        share = float((F(t) > x).mean())
        sigma = np.sqrt(float(F(t)) * (1.0 - float(F(t))) / N)
        print("prim %d tau %.4f: share %.6f (%.2f sigma)" % (prim, t, share, (share - float(F(t))) / sigma))
        assert abs(share - float(F(t))) <= 5 * sigma, (prim, t, share)
    assert not (F(0.0) > x).any() and (F(1.0) > x).all()        # tau <= 0 never passes, tau >= 1 always


@pytest.mark.parametrize("prim", PRIMS)
def test_xi_is_uncorrelated_with_the_alpha_blend_xi_of_the_same_hit(hits, prim):
    u, v = hits
    a, b = G.xi(prim, u, v).astype(np.float64), blend_ref.xi(prim, u, v).astype(np.float64)
    r = float(np.corrcoef(a, b)[0, 1])
    print("prim %d: correlation %.2e (bound %.2e)" % (prim, r, 5 / np.sqrt(N)))
    assert abs(r) <= 5 / np.sqrt(N), r
    assert (a != b).mean() > 0.999          # the salt: not the same number


def test_two_prims_get_unrelated_thresholds(hits):
    u, v = hits
    r = float(np.corrcoef(G.xi(0, u, v).astype(np.float64), G.xi(1, u, v).astype(np.float64))[0, 1])
    assert abs(r) <= 5 / np.sqrt(N), r


def test_fresnel_at_normal_incidence_is_the_textbook_value():
    t64 = G.tau([[1.0, 1.0, 1.0]], 0.0, 1.0, 1.5, 1.0, np.float64)
    assert np.allclose(1.0 - t64, 0.04, rtol=0, atol=1e-15)          # ((1 - 1/1.5) / (1 + 1/1.5))^2 = 0.04
    t32 = G.tau([[1.0, 1.0, 1.0]], 0.0, 1.0, 1.5, 1.0, F)
    assert np.all(np.abs(t32.astype(np.float64) - 0.96) <= G.tau_bound([[1.0, 1.0, 1.0]], 1.5, 1.0))      # (1.5 is a binary32 number)
    # ior 1 is no interface, metallic 1 and grazing incidence pass nothing, and the tint is the base colour's
    assert np.array_equal(G.tau([[0.5, 1.0, 0.25]], 0.0, 1.0, 1.0, 0.7, np.float64), [[0.5, 1.0, 0.25]])
    assert not G.tau([[0.5, 1.0, 0.25]], 1.0, 1.0, 1.5, 1.0, F).any() and not G.tau([[0.5, 1.0, 0.25]], 0.0, 1.0, 1.5, 0.0, F).any()
    assert np.array_equal(G.tau([[0.5, 1.0, 0.25]], 0.5, 0.25, 1.5, 1.0, np.float64), 0.25 * 0.5 * 0.96 * np.array([[0.5, 1.0, 0.25]]))


def test_binary32_tau_stays_within_the_derived_bound_of_binary64():
    rng = np.random.default_rng(3)
    n = 1 << 16
    c = np.concatenate([rng.random(n - 6, F), np.array([1.0, 0.5, 1e-3, 1e-4, 0.0, 0.999999], F)])
    base = rng.random((n, 3), F)
    metal = rng.uniform(-0.2, 1.2, n).astype(F)
    tr = rng.choice(np.array([0.25, 1.0], F), n)
    for ior in (1.0, 1.5, 2.4):
        t32 = G.tau(base, metal, tr, F(ior), c, F).astype(np.float64)
        t64 = G.tau(base, metal, tr, F(ior), c, np.float64)
        bound = G.tau_bound(base, float(F(ior)), c.astype(np.float64))
        err = np.abs(t32 - t64)
        assert np.all(np.isfinite(t32)) and np.all(err <= bound), (ior, float((err / bound).max()))
        well = c > 0.05
        print("ior %.1f: max |tau32 - tau64| %.2e, largest bound where c > 0.05: %.2e" % (ior, err.max(), bound[well].max()))
        if ior > 1.0:
            assert bound[well].max() < 1e-4       # the bound means something away from grazing incidence


def test_bits_and_the_and_of_a_stack():
    t = np.array([[0.5, 1.0, 0.25], [0.0, 0.0, 0.0], [np.nan, 0.9, 0.1]], F)
    assert G.bits(t, np.array([0.3, 0.0, 0.5], F)).tolist() == [0b011, 0b000, 0b010]
    # the alive mask of a ray through two panes is the AND of their bits, whatever the order and however often one is tested
    rng = np.random.default_rng(9)
    a, b = rng.integers(0, 8, 1000), rng.integers(0, 8, 1000)
    assert np.array_equal(7 & a & b, 7 & b & a & b & a)
