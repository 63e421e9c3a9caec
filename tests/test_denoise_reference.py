"""The oracle's denoiser passes (oracle/lpt_oracle.c orc_denoise_filter, SPEC §15.2-15.4) against an independent binary64
restatement of the SPEC (tests/denoise_ref.py), stage by stage, on seeded edge inputs: sizes 1x1 to 3840x2160, miss and emitter
pixels, albedo bytes 0 and 255, zero and non-zero variance, normals and depths at the reuse thresholds, NaN / inf / huge /
sub-pixel / border motions, and static runs past the history cap.

Tolerance, per value: twice the first-order bound of the float32 evaluation that the reference carries next to each of its
values (the bound formulas are in the docstrings of denoise_ref.Temporal and denoise_ref.atrous); the history must be equal.
The mutation check makes the claim that this would catch a misreading checkable: every mutant of the reference in
denoise_ref.MUTANTS must leave the tolerance somewhere on the same inputs."""
import functools

import numpy as np
import pytest

import denoise_ref as R


@functools.lru_cache(maxsize=None)
def oracle_run(w, h, mode):
    """the oracle over the edge sequence of one size: per frame the inputs, temporal radiance, moments, history, main target"""
    from oracle import orc
    seq = R.sequence(w, h)
    den = orc.Denoiser(None, w, h)
    frames = []
    for k in range(len(seq)):
        inputs = seq.frame(k)
        main = den.filter(*inputs, mode=mode)
        _, _, rad, hist = den.read()
        frames.append((inputs, rad, den.read_moments(), hist, main))
    return frames


def run_checker(w, h, mode, mutant=None, stop_when_rejected=False):
    from oracle import orc
    chk = R.Checker(w, h, mode, mutant)
    worst = {}
    for inputs, rad, mom, hist, main in oracle_run(w, h, mode):
        for key, v in chk.frame(inputs, rad, hist, main, orc.atrous_pass, mom=mom).items():
            worst[key] = max(worst.get(key, 0.0), v)
        if stop_when_rejected and max(worst.values()) > 1.0:
            break
    return worst


CASES = [(w, h, mode) for (w, h) in R.SIZES for mode in (1, 2)] + [R.BIG + (1,)]


@pytest.mark.parametrize("w,h,mode", CASES, ids=["%dx%d-mode%d" % c for c in CASES])
def test_oracle_matches_float64_reference(w, h, mode):
    worst = run_checker(w, h, mode)
    print("%dx%d mode %d: largest error / tolerance per stage %s" % (w, h, mode, {k: "%.3g" % v for k, v in worst.items()}))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, "stages beyond the tolerance: %s" % bad


def test_edge_inputs_reach_the_edges():
    """the committed sequences reach what they are there for (a guard against a generator change that quietly drops a case)"""
    seq = R.sequence(19, 13)
    ev = [seq.frame(k) for k in range(seq.static, len(seq))]
    mo = np.concatenate([m.reshape(-1, 2) for _, _, m in ev])
    assert np.isnan(mo).any() and np.isposinf(mo).any() and np.isneginf(mo).any() and (np.abs(mo[np.isfinite(mo)]) * 19 > 2.0 ** 31).any()
    g = ev[0][1].reshape(-1, 4)
    assert (g[:, 0] == R.INVALID).any() and (((g[:, 0] & 0x80000000) != 0) & (g[:, 0] != R.INVALID)).any()
    alb = g[:, 3]
    assert ((alb & 0xFF) == 0).any() and ((alb & 0xFF) == 255).any()
    na, nb = R.threshold_normals()
    d = [R.dot32(R.oct_decode32(na), R.oct_decode32(nb[k])) for k in ("eq", "above", "below")]
    assert d[0] == np.float32(0.9) and d[1] > np.float32(0.9) > d[2]
    frames = oracle_run(19, 13, 1)
    hist = np.stack([f[3] for f in frames])
    assert hist.max() == R.CAP and (hist[seq.static - 1] == R.CAP).any()
    var = np.stack([f[1][..., 3] for f in frames[8:]])
    assert (var == 0).any() and (var > 0).any()


@pytest.mark.parametrize("mutant", list(R.MUTANTS))
def test_mutant_is_rejected(mutant):
    """a misreading of SPEC §15 in the reference (denoise_ref.MUTANTS) must disagree with the oracle beyond the tolerance"""
    worst = {}
    for w, h in R.SIZES:
        for mode in (1, 2):
            for k, v in run_checker(w, h, mode, mutant, stop_when_rejected=True).items():
                worst[k] = max(worst.get(k, 0.0), v)
            if max(worst.values()) > 1.0:
                break
        if max(worst.values()) > 1.0:
            break
    print("%s: largest error / tolerance %s" % (mutant, {k: "%.3g" % v for k, v in worst.items()}))
    assert max(worst.values()) > 1.0, "mutant %r (%s) is not rejected: %s" % (mutant, R.MUTANTS[mutant], worst)
