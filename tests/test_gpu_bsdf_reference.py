"""-m gpu: the device's BSDF (SPEC §10: device_math.h make_surface, spec_probability, bsdf_eval, bsdf_sample, set up as shade_hit sets them up, through
the hook lpt_bsdf_probe) on the edge set of tests/bsdf_ref.py: bit for bit the oracle's — the project's bar: -ffp-contract=off, explicit fmaf only,
correctly rounded divide and square root —, and held to the binary64 reference by the same checker and the same two integral tests as the oracle in
tests/test_bsdf_reference.py, where the bounds are explained.  One launch each."""
import numpy as np
import pytest

import bsdf_ref as R
from oracle import orc

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("pipeline")]

_CACHE = {}


def _edge(device):
    rows, n_edge = R.edge_set(orc.bsdf_probe)
    return rows, n_edge, device.bsdf_probe(rows)


def test_hook_equals_the_oracle_bit_for_bit(device):
    rows, n_edge, (out, ok) = _edge(device)
    want, wok = orc.bsdf_probe(rows)
    assert np.all(np.isfinite(out))
    diff = np.any(out.view(np.uint32) != want.view(np.uint32), axis=1) | (ok != wok)
    if diff.any():          # the float64 reference says which side is wrong
        i = np.flatnonzero(diff)
        cd, co = R.check(rows[i], out[i], ok[i]), R.check(rows[i], want[i], wok[i])
        pytest.fail("%d of %d elements differ (first: %s); of those the device misses the reference on %d, the oracle on %d"
                    % (i.size, rows.shape[0], i[:5], cd["bad"].sum(), co["bad"].sum()))


def test_hook_meets_the_error_model_on_the_edge_set(device):
    rows, n_edge, (out, ok) = _edge(device)
    assert np.all(np.isfinite(out)) and np.all(out[ok == 0, 5:] == 0.0)
    R.assert_not_negative(out)
    c = R.check(rows, out, ok, _CACHE)
    print("\ndevice, %d edge + %d random elements: error / tolerance %s; left out: eval %.4f %%, sample %.4f %%; ok mismatches %d"
          % (n_edge, rows.shape[0] - n_edge, {k: round(v, 3) for k, v in c["ratio"].items()}, 100 * c["left_out_eval"], 100 * c["left_out_sample"], c["ok_mismatch"]))
    assert c["left_out_eval"] <= 0.02 and c["left_out_sample"] <= 0.02
    assert not c["bad"].any(), np.flatnonzero(c["bad"])[:10]
    assert R.sample_invariants(rows, out, ok, device.bsdf_probe) > rows.shape[0] // 3


@pytest.mark.parametrize("name", R.DENSITY_CONFIGS)
def test_samples_follow_the_density(device, name):
    for label, got, want, se in R.density_estimates(name, device.bsdf_probe):
        print("\n%s, %s: %.6f against %.6f, %.2f standard errors" % (name, label, got, want, (got - want) / se))
        assert abs(got - want) <= 4.0 * se, (name, label, got, want, se)


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_mean_weight_is_the_directional_albedo(device, name):
    got, want, se = R.weight_estimates(name, device.bsdf_probe)
    print("\n%s: %s against %s, %s standard errors" % (name, got, want, (got - want) / se))
    assert np.all(np.abs(got - want) <= 4.0 * se), (name, got, want, se)


def test_no_sample_loses_its_specular_density(device):
    got, bound = R.grazing_weights(device.bsdf_probe)
    print("\nlargest weight at NoV 1e-4, minimum roughness: %.4g (bound %.4g)" % (got, bound))
    assert got <= bound
