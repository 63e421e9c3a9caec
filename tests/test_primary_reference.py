"""The oracle's primary pass (oracle/lpt_oracle.c: ray generation, the primary hit, the G-buffer and the motion vectors of
orc_denoise_frame; SPEC §4, §11, §15.1) against an independent binary64 restatement of the SPEC and of plain geometry
(tests/primary_ref.py), over the scene and the camera sequence of that module: first frame against the identity, static, translation,
yaw, roll, a vfov change, a move past part of the scene and back; at 61x37 and 64x32, in both denoising modes, with and without the
blue-noise texture.

Tolerance, per value: the bound the reference carries next to it (derived in primary_ref.py; prim id, the depth of a miss and the
albedo byte away from a rounding boundary must be equal).  A pixel is left out only below the edge distance primary_ref.EDGE_EPS:
at most 1 % of a frame, and every frame still compares each class of pixel it was built to contain.  The mutation check makes the
claim that this would catch a misreading checkable: every mutant of the reference in primary_ref.MUTANTS must put the oracle's
output beyond the tolerance on some frame."""
import functools

import numpy as np
import pytest

import primary_ref as R

CASES = [(w, h, mode, False) for (w, h) in R.SIZES for mode in (1, 2)] + [(R.SIZES[0] + (1, True))]
IDS = ["%dx%d-mode%d%s" % (w, h, m, "-noise" if nz else "") for w, h, m, nz in CASES]


@functools.lru_cache(maxsize=None)
def scene():
    return R.scene_data()


@functools.lru_cache(maxsize=None)
def oracle_run(w, h, mode, noise):
    """the oracle over the sequence: per frame (view, vfov, seed counter before the call, G-buffer, motion)"""
    from oracle import orc
    gs, _ = scene()
    osc = orc.OracleScene.from_scene(gs, noise=R.noise_texture() if noise else None)
    den = orc.Denoiser(osc, w, h, 0.9, R.BOUNCES, R.USER_SEED)
    out = []
    for what, view, vfov, need in R.frames():
        seed = den.seed_counter
        den.frame(view, mode, vfov=vfov, use_noise=noise)
        g, m, _, _ = den.read()
        out.append((view, vfov, seed, g, m))
    return out


def run_checker(w, h, mode, noise, mutant=None, stop_when_rejected=False):
    ref = R.Reference(scene()[1], w, h, R.noise_texture() if noise else None, mutant)
    report = []
    for (what, _, _, need), (view, vfov, seed, g, m) in zip(R.frames(), oracle_run(w, h, mode, noise)):
        f = ref.frame(view, vfov, seed)
        report.append((what, need, R.coverage(f), R.check(f, g, m)))
        if stop_when_rejected and max(report[-1][3].values()) > 1.0:
            break
    return report


@pytest.mark.parametrize("w,h,mode,noise", CASES, ids=IDS)
def test_oracle_matches_float64_reference(w, h, mode, noise):
    lines, bad = [], []
    for k, (what, need, (excluded, classes), worst) in enumerate(run_checker(w, h, mode, noise)):
        lines.append("frame %d (%s): excluded %.2f %%, compared per class %s, largest error / tolerance %s"
                     % (k, what, 100.0 * excluded, classes, {s: "%.3g" % v for s, v in worst.items()}))
        if excluded > 0.01:
            bad.append("frame %d: %.2f %% of the pixels excluded" % (k, 100.0 * excluded))
        bad += ["frame %d compares no %s pixel" % (k, c) for c in need if classes[c] == 0]
        bad += ["frame %d: %s beyond the tolerance (%.3g)" % (k, s, v) for s, v in worst.items() if not v <= 1.0]
    print("\n".join(lines))
    assert not bad, "\n".join(bad + lines)


def test_sequence_reaches_what_it_is_there_for():
    """a guard against a scene or camera change that quietly drops a case: seam normals, a clamped and a textured albedo, motion in
    every kind of frame, a zero motion for the points behind the previous camera"""
    ref = R.Reference(scene()[1], 61, 37)
    fr = [ref.frame(view, vfov, R.BOUNCES * k) for k, (_, view, vfov, _) in enumerate(R.frames())]
    n = np.concatenate([f.n[f.compared & f.surf] for f in fr])
    for seam in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, -1)):
        assert np.any(np.all(n == np.array(seam, np.float64), axis=1)), "no pixel with the normal %s" % (seam,)
    assert np.any((n[:, 2] == 0) & (n[:, 0] != 0) & (n[:, 1] != 0)), "no pixel with n.z = 0 off the axes"
    alb = np.concatenate([f.alb[f.compared & f.surf] for f in fr])
    assert np.any(alb[:, 0] == 1.0) and np.any((alb[:, 0] < 1.0) & (alb[:, 0] > 0.0)) and len(np.unique(alb[:, 1])) > 20
    for k in (0, 2, 3, 4, 5, 6, 7):
        assert np.abs(fr[k].motion[fr[k].compared]).max() > 1e-3, "frame %d: no motion" % k
    for k in (1, 8):
        assert np.abs(fr[k].motion[fr[k].compared]).max() < 1e-9, "frame %d: static" % k
    for k in (0, 7):
        b = fr[k].behind & fr[k].compared
        assert b.any() and np.all(fr[k].motion[b] == 0) and np.abs(fr[k].motion[fr[k].compared & ~fr[k].miss & ~b]).min() > 0


@pytest.mark.parametrize("mutant", list(R.MUTANTS))
def test_mutant_is_rejected(mutant):
    """a misreading of SPEC §4 / §11 / §15.1 in the reference (primary_ref.MUTANTS) must put the oracle beyond the tolerance"""
    worst = {}
    for case in CASES:
        for _, _, _, w in run_checker(*case, mutant=mutant, stop_when_rejected=True):
            for s, v in w.items():
                worst[s] = max(worst.get(s, 0.0), v)
        if max(worst.values()) > 1.0:
            break
    print("%s: DETECTED, largest error / tolerance %s" % (mutant, {s: "%.3g" % v for s, v in worst.items()}))
    assert max(worst.values()) > 1.0, "mutant %r (%s) is not rejected: %s" % (mutant, R.MUTANTS[mutant], worst)
