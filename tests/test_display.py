"""CPU: the display transform and the meter of SPEC §30 without a device.  The new entry points and the ABI version (a renderer cannot be created without a
device, so the display state's round trip, its defaults and its refusals run in tests/test_gpu_display.py; here every entry point refuses a null handle); the curves
of csrc/display_math.h, compiled by g++ into tests/tools/display_check, against tests/display_ref.py's binary32 bit for bit; binary32 against binary64 inside the
bound display_ref derives term by term; the curves' properties in binary64; lpt_meter_from_histogram against the reference, exactly."""
import os
import subprocess

import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import _abi as A

import display_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVS = (-3.0, 0.0, 2.5)
OPS = (D.CLAMP, D.PBR_NEUTRAL, D.ACES)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------- the ABI
def test_abi_version_operators_and_header():
    assert A.lib().lpt_abi_version() == 6
    assert A.DISPLAY_OPERATORS == D.OPERATORS == {"clamp": 0, "pbr_neutral": 1, "aces": 2}
    header = open(os.path.join(ROOT, "include", "lpt.h")).read()
    assert "enum { LPT_DISPLAY_CLAMP = 0, LPT_DISPLAY_PBR_NEUTRAL = 1, LPT_DISPLAY_ACES = 2 };" in header
    assert "#define LPT_ABI_VERSION 6u" in header
    for name in ("lpt_renderer_set_display", "lpt_renderer_get_display", "lpt_renderer_meter", "lpt_meter_from_histogram", "lpt_display_probe", "lpt_meter_probe"):
        assert name in A.SIGNATURES and hasattr(A.lib(), name)
    assert lp.Renderer.set_display and lp.Renderer.meter and isinstance(lp.Renderer.display, property)


def test_null_handles_are_invalid_arguments_not_crashes():
    L = A.lib()
    ev, op = A.C.c_float(7.0), A.C.c_uint32(9)
    assert L.lpt_renderer_set_display(None, 0.0, 0) == A.LPT_ERR_INVALID_ARG
    assert L.lpt_renderer_get_display(None, A.C.byref(ev), A.C.byref(op)) == A.LPT_ERR_INVALID_ARG and (ev.value, op.value) == (7.0, 9)
    assert L.lpt_renderer_meter(None, 0.5, 0.02, A.C.byref(ev), None, None, None) == A.LPT_ERR_INVALID_ARG
    assert L.lpt_display_probe(None, 0, None, 0.0, 0, None) == A.LPT_ERR_INVALID_ARG
    assert L.lpt_meter_probe(None, 0, None, None, None) == A.LPT_ERR_INVALID_ARG
    with pytest.raises(lp.Error) as e:
        lp.api._display_operator("filmic")
    assert e.value.kind == "InvalidArg"


# ---------------------------------------------------------------------------- the curves on the CPU
@pytest.fixture(scope="module")
def display_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("display") / "display_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "loupiote_amd", "csrc"),
                           os.path.join(ROOT, "tests", "tools", "display_check.cpp"), "-o", exe])

    def run(lines):
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
        return p.stdout.split("\n")[:-1]
    return run


@pytest.fixture(scope="module")
def cases():
    return D.edge_accumulators()


def test_cpu_curves_equal_the_binary32_reference_bit_for_bit(display_check, cases):
    m = D.mean32(cases)
    mb = bits(m)
    lines, want = [], []
    for op in OPS:
        for ev in EVS:
            g = int(D.gain(ev).view(np.uint32))
            lines += ["%d %08x %08x %08x %08x" % (op, g, r[0], r[1], r[2]) for r in mb]
            want.append(bits(D.transform32(cases, ev, op)))
    out = display_check(lines)
    got = np.array([[int(w, 16) for w in l.split()] for l in out], np.uint32)
    want = np.concatenate(want)
    assert got.shape == want.shape
    nan = np.isnan(want.view(np.float32))
    assert not nan.any()                                       # no curve lets a NaN through: the bits can be compared as they are
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, (bad[:8], got[bad[:4]], want[bad[:4]])


def test_cpu_meter_bins_equal_the_reference(display_check):
    acc = D.meter_accumulators()
    Y = D.luminance32(D.mean32(acc))
    out = np.array([int(l) for l in display_check(["bin %08x" % b for b in bits(Y)])])
    with np.errstate(invalid="ignore"):
        ok = (Y >= np.float32(2.0 ** -24)) & (Y < np.float32(2.0 ** 24))
    want = np.where(ok, (bits(Y) >> 20).astype(np.int64) - (103 << 3), -1)
    assert np.array_equal(out, want)
    # by hand: 8 bins per octave from 2^-24, an octave's bins splitting the mantissa linearly; the range is half open; NaN and infinity have no bin
    by_hand = [(1.0, 192), (1.5, 196), (1.9999999, 199), (2.0 ** -24, 0), (D._ulps(2.0 ** -24, -1), -1), (2.0 ** 24, -1), (D._ulps(2.0 ** 24, -1), 383), (0.0, -1),
               (-1.0, -1), (np.nan, -1), (np.inf, -1), (0.18, 8 * 21 + 3)]
    assert [int(l) for l in display_check(["bin %08x" % int(np.float32(y).view(np.uint32)) for y, _ in by_hand])] == [b for _, b in by_hand]


# ---------------------------------------------------------------------------- binary32 against binary64
def finite_colours():
    rng = np.random.default_rng(3)
    c = [D.expose32(D.mean32(D.edge_accumulators()), ev) for ev in EVS]
    c.append((2.0 ** rng.uniform(-30, 60, (20000, 3))).astype(np.float32))
    c.append(rng.uniform(0, 2, (20000, 3)).astype(np.float32))
    g = np.linspace(0, 4, 4001, dtype=np.float32)
    c.append(np.stack([g, g, g], 1))
    c = np.concatenate(c)
    return c[np.isfinite(c).all(1)]


@pytest.mark.parametrize("op", [D.PBR_NEUTRAL, D.ACES])
def test_binary32_curves_stay_inside_the_derived_bound(op):
    """SPEC §30.4 records the largest fraction of the bound seen here (printed below)."""
    c = finite_colours()
    t32, dec = D.curve32(op, c)
    t64, bound = D.curve64(op, c, replay=dec)
    err = np.abs(t32.astype(np.float64) - t64)
    frac = err / bound
    print("op %d: max |binary32 - binary64| = %.3g, largest fraction of the bound = %.3f over %d colours" % (op, err.max(), frac.max(), c.shape[0]))
    assert np.all(err <= bound)
    # the bound is worth something: where the result matters (values the encoding does not clamp away) it stays below a tenth of one sRGB code's narrowest step
    inside = (np.abs(t64) <= 2.0) & (c.max(1) <= 2.0 ** 20)[:, None]
    assert bound[inside].max() < 0.1 * float(np.diff(D.THR.astype(np.float64)).min())


# ---------------------------------------------------------------------------- the curves' properties, in binary64
def pbr64(c):
    return D.curve64(D.PBR_NEUTRAL, c)[0]


def test_pbr_neutral_stays_in_the_unit_cube_and_is_monotone_and_continuous():
    rng = np.random.default_rng(4)
    c = np.concatenate([2.0 ** rng.uniform(-30, 60, (50000, 3)), rng.uniform(0, 3, (50000, 3)), np.zeros((1, 3)), np.full((1, 3), float(np.finfo(np.float32).max))])
    out = pbr64(c)
    assert out.min() >= 0.0 and out.max() <= 1.0
    g = np.concatenate([np.linspace(0, 4, 40001), 2.0 ** np.linspace(2, 100, 2000)])
    ramp = pbr64(np.stack([g, g, g], 1))[:, 0]
    assert np.all(np.diff(ramp) >= 0) and ramp[0] == 0.0 and ramp[-1] <= 1.0
    # continuity: across x = 0.08 (the offset's two forms) and across p = 0.76 (the compression's start) the value moves no more than the input does
    h = 2.0 ** -30
    for lo, hi in (((0.08 - h, 0.5, 0.9), (0.08 + h, 0.5, 0.9)), ((0.08 - h,) * 3, (0.08 + h,) * 3), ((0.76 - h, 0.0, 0.3), (0.76 + h, 0.0, 0.3)), ((0.8 - h,) * 3, (0.8 + h,) * 3)):
        a, b = pbr64(np.array([lo])), pbr64(np.array([hi]))
        assert np.abs(a - b).max() <= 4 * h
    off = lambda x: x - 6.25 * x * x
    assert abs(off(0.08) - 0.04) < 1e-15                       # the two forms of the offset meet
    # the rule for p = +inf: (1, 1, 1)
    assert np.array_equal(D.transform32(np.array([[np.inf, 1.0, 0.0, 1.0]], np.float32), 0.0, D.PBR_NEUTRAL), np.ones((1, 3), np.float32))


def test_aces_maps_black_to_code_0_and_infinity_to_a_finite_value():
    black = D.curve64(D.ACES, np.zeros((1, 3)))[0]
    assert np.all(black < 0) and np.all(D.encode_srgb8(black.astype(np.float32)) == 0)
    assert np.array_equal(D.display_bytes(np.array([[0, 0, 0, 1]], np.float32), 0.0, D.ACES), [[0, 0, 0, 255]])
    t = D.transform32(np.array([[np.inf, np.inf, np.inf, 1.0], [np.inf, 0.0, 0.0, 1.0], [3.4e38, 3.4e38, 3.4e38, 1.0]], np.float32), 2.5, D.ACES)
    assert np.isfinite(t).all()
    assert np.array_equal(D.display_bytes(np.array([[np.inf, np.inf, np.inf, 1.0]], np.float32), 0.0, D.ACES), [[255, 255, 255, 255]])


def test_clamp_at_exposure_0_is_the_old_encoding():
    """(0, CLAMP) through the reference is §13.2: code = round(255 * OETF(clamp(mean))) away from rounding boundaries"""
    acc = D.edge_accumulators()
    got = D.display_bytes(acc, 0.0, D.CLAMP)[:, :3].astype(int)
    m = np.clip(np.nan_to_num(D.mean32(acc).astype(np.float64), nan=0.0, posinf=1.0, neginf=0.0), 0.0, 1.0)
    s = np.where(m <= 0.0031308, 12.92 * m, 1.055 * m ** (1 / 2.4) - 0.055) * 255.0
    off = got != np.floor(s + 0.5).astype(int)
    assert np.all(np.abs(s[off] + 0.5 - np.round(s[off] + 0.5)) < 2e-3)


# ---------------------------------------------------------------------------- the evaluation of a histogram
def hist_cases():
    rng = np.random.default_rng(5)
    out = []
    for k in range(12):
        h = np.zeros(D.BINS, np.uint32)
        idx = rng.integers(0, D.BINS, rng.integers(1, 200))
        np.add.at(h, idx, rng.integers(1, 5000, idx.size).astype(np.uint32))
        out.append(h)
    for b in (0, 1, 191, 383):
        h = np.zeros(D.BINS, np.uint32)
        h[b] = 1 + 999 * (b & 1)
        out.append(h)
    out.append(np.zeros(D.BINS, np.uint32))                   # N = 0
    h = np.zeros(D.BINS, np.uint32)
    h[[10, 20, 30, 40]] = [25, 25, 40, 10]                    # N = 100: low = 0.25 and 0.5, high = 0.1 land exactly on bin boundaries
    out.append(h)
    out.append(np.full(D.BINS, 2 ** 23 - 1, np.uint32))       # a large one: N just below 2^32, the most pixels a frame can have
    return out


@pytest.mark.parametrize("low,high", [(0.5, 0.02), (0.0, 0.0), (0.25, 0.1), (0.5, 0.1), (0.0, 0.9990000128746033), (0.9, 0.05), (0.3333333432674408, 0.3333333432674408), (0.5, 0.4999999701976776)])
def test_meter_from_histogram_equals_the_reference_exactly(low, high):
    for h in hist_cases():
        want_ev, want_n = D.evaluate(h, low, high)
        ev, n = lp.meter_from_histogram(h, low, high)
        assert n == want_n and np.float32(ev).view(np.uint32) == np.float32(want_ev).view(np.uint32), (low, high, ev, want_ev, n, want_n)
    # one value by hand: everything in the bin that starts at 2^0, centre 1/16 of an octave above: ev = log2(0.18) - 1/16
    h = np.zeros(D.BINS, np.uint32)
    h[24 * 8] = 7
    assert lp.meter_from_histogram(h, 0.0, 0.0) == (float(np.float32(D.LOG2_018 - 0.0625)), 7)
    assert abs(D.LOG2_018 - np.log2(0.18)) < 1e-15


@pytest.mark.parametrize("low,high", [(-0.1, 0.0), (0.0, -0.1), (1.0, 0.0), (0.0, 1.0), (0.5, 0.5), (0.75, 0.5), (np.nan, 0.0), (0.0, np.nan), (np.inf, 0.0)])
def test_meter_rejects_fractions_outside_the_domain(low, high):
    h = np.ones(D.BINS, np.uint32)
    ev, n = A.C.c_float(5.0), A.C.c_uint32(5)
    assert A.lib().lpt_meter_from_histogram(A.ptr(h), low, high, A.C.byref(ev), A.C.byref(n)) == A.LPT_ERR_INVALID_ARG
    assert (ev.value, n.value) == (5.0, 5)
    assert A.lib().lpt_meter_from_histogram(None, 0.5, 0.02, A.C.byref(ev), A.C.byref(n)) == A.LPT_ERR_INVALID_ARG


def test_meter_refuses_a_histogram_whose_count_does_not_fit_32_bits():
    """`counted` is 32 bits wide: a histogram that sums to 2^32 or more is refused with nothing written; 2^32 - 1 is evaluated"""
    ev, n = A.C.c_float(5.0), A.C.c_uint32(5)
    h = np.zeros(D.BINS, np.uint32)
    h[[7, 300]] = [2 ** 31, 2 ** 31]
    assert A.lib().lpt_meter_from_histogram(A.ptr(h), 0.0, 0.0, A.C.byref(ev), A.C.byref(n)) == A.LPT_ERR_INVALID_ARG
    assert (ev.value, n.value) == (5.0, 5) and b"2^32" in A.lib().lpt_last_error()
    h[300] -= 1
    want_ev, want_n = D.evaluate(h, 0.25, 0.25)
    got_ev, got_n = lp.meter_from_histogram(h, 0.25, 0.25)
    assert got_n == want_n and np.float32(got_ev).view(np.uint32) == np.float32(want_ev).view(np.uint32)
    assert lp.meter_from_histogram(h, 0.0, 0.0)[1] == 2 ** 32 - 1
