"""CPU: the oracle's BSDF (SPEC §10: make_surface, spec_probability, bsdf_eval, bsdf_sample, through the batched orc_bsdf_probe) against the binary64
reference and the error model of tests/bsdf_ref.py, on the edge set the device is held to in tests/test_gpu_bsdf_reference.py: pointwise within
`tolerance`, the checker's own mutation tests, what every surviving sample satisfies bit for bit, the sampling against its density and the mean
weight against the directional albedo.  Every bound is bsdf_ref's (the model's, or 4 standard errors of a fixed-seed mean); figures are printed
before they are asserted (pytest -s)."""
import numpy as np
import pytest

import bsdf_ref as R
import kat_scenes as K
from oracle import orc

_CACHE = {}


def _edge():
    rows, n_edge = R.edge_set(orc.bsdf_probe)
    if "out" not in _CACHE:
        _CACHE["out"] = orc.bsdf_probe(rows)
    return rows, n_edge, _CACHE["out"]


def test_the_error_model_walks_the_reference():
    """`tolerance` evaluates SPEC §10 in the SPEC's operation order, `reference` from the formulas: two float64 evaluations that may differ by float64
    roundings only — 2^-29 of the binary32 ones the tolerance is made of; a millionth of the tolerance is asked"""
    rows, _, _ = _edge()
    want, wok = R.reference(rows)
    tol, aux = R.tolerance(rows)
    got = aux["values"][:, :5]
    t = np.concatenate([tol["pspec"], tol["f"], tol["pdf"]], axis=1)
    fin = np.isfinite(t) & ~aux["near_eval"][:, None]
    assert fin.mean() > 0.99
    assert np.all(np.abs(got - want[:, :5])[fin] <= 1e-6 * t[fin])
    both = ~aux["near_sample"]
    assert np.array_equal(aux["ok"][both], wok[both])
    Ls = R.sample_direction(R.surface(*(R.split(rows)[k] for k in ("base", "rough", "metal"))), R.split(rows)["N"], R.split(rows)["V"],
                            R.split(rows)["r3"] < want[:, 0], R.split(rows)["r4"], R.split(rows)["r5"])
    fin = np.isfinite(tol["L_s"])
    assert np.all(np.abs(aux["L_s"] - Ls)[fin] <= 1e-6 * tol["L_s"][fin])


def test_oracle_meets_the_error_model_on_the_edge_set():
    rows, n_edge, (out, ok) = _edge()
    assert np.all(np.isfinite(out)) and set(np.unique(ok)) <= {0, 1}
    assert np.all(out[ok == 0, 5:] == 0.0)
    R.assert_not_negative(out)
    c = R.check(rows, out, ok, _CACHE.setdefault("check", {}))
    print("\noracle, %d edge + %d random elements: error / tolerance %s; left out: eval %.4f %%, sample %.4f %%; ok mismatches %d"
          % (n_edge, rows.shape[0] - n_edge, {k: round(v, 3) for k, v in c["ratio"].items()}, 100 * c["left_out_eval"], 100 * c["left_out_sample"], c["ok_mismatch"]))
    assert c["left_out_eval"] <= 0.02 and c["left_out_sample"] <= 0.02
    assert not c["bad"].any(), np.flatnonzero(c["bad"])[:10]


# the share of the set a mutation must be rejected on, from what it touches: k and the diffuse factor change f wherever the gate at L is open or a sample
# survives (about two thirds of the set; less the surfaces with alpha = 1, where alpha^2 / 2 = alpha / 2, and those without a diffuse lobe), the swapped pdf every
# pdf likewise; r4 for sqrt(r4) only moves the cosine-lobe samples (1 - pspec of the draws, less r4 in {0, 1})
@pytest.mark.parametrize("mutation,share", [("k_alpha2", 0.5), ("diffuse_without_1mF", 0.5), ("pdf_s_swapped", 0.5), ("cosine_r4", 0.2)])
def test_the_checker_rejects_a_wrong_bsdf(mutation, share):
    rows, _, _ = _edge()
    out, ok = R.reference(rows, mutation)
    c = R.check(rows, out.astype(np.float32), ok, dict(_CACHE.get("check", {})))      # same rows, same lobe picks: the reference is the cached one
    print("\n%s: rejected on %.1f %% of the set" % (mutation, 100 * c["bad"].mean()))
    assert c["bad"].mean() >= share


def test_every_surviving_sample_is_consistent_bit_for_bit():
    rows, _, (out, ok) = _edge()
    n = R.sample_invariants(rows, out, ok, orc.bsdf_probe)
    assert n > rows.shape[0] // 3


def test_r3_at_pspec_takes_the_cosine_lobe():
    """`r3 < pspec`: the draw AT the oracle's own pspec is a cosine-lobe sample (the direction of r3 = 1 - 2^-24), the float below it a GGX one"""
    rows, n_edge, (out, ok) = _edge()
    at = (rows[:n_edge, 17] == out[:n_edge, 0]) & (out[:n_edge, 0] < 1.0)
    assert at.sum() > 100
    r = rows[:n_edge][at].copy()
    r[:, 17] = R.ONE_M
    o2, k2 = orc.bsdf_probe(r)
    assert np.array_equal(o2.view(np.uint32), out[:n_edge][at].view(np.uint32)) and np.array_equal(k2, ok[:n_edge][at])


@pytest.mark.parametrize("name", R.DENSITY_CONFIGS)
def test_samples_follow_the_density(name):
    for label, got, want, se in R.density_estimates(name, orc.bsdf_probe):
        print("\n%s, %s: %.6f against %.6f, %.2f standard errors" % (name, label, got, want, (got - want) / se))
        assert abs(got - want) <= 4.0 * se, (name, label, got, want, se)


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_mean_weight_is_the_directional_albedo(name):
    got, want, se = R.weight_estimates(name, orc.bsdf_probe)
    print("\n%s: %s against %s, %s standard errors" % (name, got, want, (got - want) / se))
    assert np.all(np.abs(got - want) <= 4.0 * se), (name, got, want, se)


def test_no_sample_loses_its_specular_density():
    got, bound = R.grazing_weights(orc.bsdf_probe)
    print("\nlargest weight at NoV 1e-4, minimum roughness: %.4g (bound %.4g)" % (got, bound))
    assert got <= bound


def test_the_albedo_agrees_with_the_furnace_quadrature():
    """at the two furnace materials the grid of kat_scenes.directional_albedo resolves, the two quadratures agree to a tenth of that test's 0.4 %"""
    eye = np.array([0.9, 1.3, 2.2])
    for base, rough, metal in (((0.8, 0.6, 0.4), 0.5, 0.0), ((0.95, 0.9, 0.8), 0.25, 1.0)):
        old = K.directional_albedo(base, rough, metal, eye)
        new = R.directional_albedo(base, rough, metal, (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), eye)
        print("\n%s %s %s: %s against %s, relative difference %s" % (base, rough, metal, new, old, np.abs(new - old) / old))
        assert np.all(np.abs(new - old) <= 0.0004 * old)
