"""SPEC.md §26 (alpha blend as stochastic coverage) restated in numpy, from the SPEC: §4's pcg on uint32, the threshold xi of a candidate hit
(prim, u, v), and the decision on top of tests/alpha_ref.py's alpha.  Test infrastructure only."""
import numpy as np

import alpha_ref as R

F = R.F
U = np.uint32


def pcg(v):
    """SPEC §4: s = v·747796405 + 2891336453; w = ((s >> ((s >> 28) + 4)) ^ s)·277803737; (w >> 22) ^ w — all modulo 2^32"""
    v = np.asarray(v).astype(np.uint64) & 0xFFFFFFFF
    s = (v * 747796405 + 2891336453) & 0xFFFFFFFF
    w = (((s >> ((s >> 28) + 4)) ^ s) * 277803737) & 0xFFFFFFFF
    return ((w >> 22) ^ w).astype(U)


def bits(x):
    """the binary32 pattern of x (so +0 and -0 differ)"""
    return np.asarray(x, F).view(U)


def xi(prim, u, v):
    """h = pcg(pcg(pcg(prim) ^ bits(u)) ^ bits(v)); xi = float(h >> 8)·2^-24, in [0, 1): exact in binary32"""
    prim, u, v = np.broadcast_arrays(np.asarray(prim).astype(U), np.asarray(u, F), np.asarray(v, F))
    h = pcg(pcg(pcg(prim) ^ bits(u)) ^ bits(v))
    return ((h >> U(8)).astype(F) * F(2.0 ** -24)).astype(F)


def counts(a, prim, u, v):
    """the hit counts iff a > xi (a NaN a does not count, a >= 1 always counts, a <= 0 never counts)"""
    return np.asarray(a, F) > xi(prim, u, v)


def alpha(color_w, image, uv, hu, hv):
    """a is §20's: alpha_ref.alpha"""
    return R.alpha(color_w, image, uv, hu, hv)
