"""CPU: the thin lens (SPEC.md §25) without a GPU — tests/lens_ref.py against hand-worked values and against tests/primary_ref.py with the lens closed, what the
reference alone says about the scenes of tests/test_gpu_lens.py (the board's excluded share, the spot's numbers), the launch plan's `lens` fact through
tests/tools/plan_fact_check.cpp, and the bindings' agreement on the three new entry points with the argument checks that need no device."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import _abi as A

from loupiote_amd import testing as T

import lens_ref as L
import primary_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEW = P.view_matrix((0.3, 1.25, -5.7), (0.12, 0.0, 1.0), 0.35)


def _cam(view=VIEW, W=61, H=37, vfov=0.9):
    return P.basis(view, W, H, vfov)


# ---------------------------------------------------------------- the reference against hand-worked values
def test_the_derivation_prints_its_terms_and_the_tolerances_are_a_few_dozen_u(capsys):
    terms, K = L.derivation()
    for name, val in terms.items():
        print("%-72s %8.3f u" % (name, val))
    assert len(capsys.readouterr().out.splitlines()) == len(terms) >= 8
    # one rounding each at the least, and nothing in the chain amplifies: a bound of hundreds of u would mean a mistake in the derivation
    assert 3.0 < K["k_sc"] < 12.0 and 10.0 < K["k_off"] < 40.0
    for R, Fd in L.RAY_LENSES:
        assert P.K_D * L.U < L.tol_direction(R, Fd) < 120.0 * L.U
    assert L.tol_direction(0.0, 3.0) == P.K_D * L.U


def test_sincos2pi_is_the_polynomial_of_section_5():
    u = np.linspace(0.0, 1.0, 4097)[:-1]
    s, c = L.sincos2pi(u)
    assert np.max(np.abs(s - np.sin(2 * np.pi * u))) < 4e-6 and np.max(np.abs(c - np.cos(2 * np.pi * u))) < 4e-6      # the truncation of x^9 / x^10 at pi/2, not rounding
    s, c = L.sincos2pi(np.array([0.0, 0.25, 0.5, 0.75]))
    assert s.tolist() == [0.0, 1.0, 0.0, -1.0] and c.tolist() == [1.0, 0.0, -1.0, 0.0]


def test_lens_points_by_hand():
    cam = _cam()
    rn, un = L.unit(cam.right), L.unit(cam.up)
    R = 0.25
    z = L.lens_offset(cam, R, np.array([0.0, 0.0]), np.array([0.3, 0.9]))
    assert np.all(z == 0.0)                                             # lx = 0: o' = origin
    off = L.lens_offset(cam, R, np.array([1.0, 1.0, 1.0, 0.25]), np.array([0.0, 0.25, 0.5, 0.0]))
    assert np.array_equal(off[0], rn * R) and np.array_equal(off[1], un * R) and np.array_equal(off[2], -rn * R)      # ly = 0, 1/4, 1/2: +rn, +un, −rn
    assert np.array_equal(off[3], rn * (R * 0.5))                       # rr = sqrt(1/4)
    r = L.primary_rays(VIEW, 61, 37, 0.9, R, 3.0, 7, 12)
    assert np.array_equal(r.o, cam.origin[None] + r.off) and np.all(np.linalg.norm(r.off, axis=1) <= R * (1 + 1e-12))
    assert np.max(np.abs(r.off @ cam.fwd)) < 1e-6 * R                    # in the lens plane, up to the view's own rounding


def test_every_ray_passes_through_the_focal_point():
    for R, Fd in L.RAY_LENSES:
        r = L.primary_rays(VIEW, 61, 37, 0.9, R, Fd, 7, 12)
        w = r.focus - r.o
        dist = np.linalg.norm(np.cross(w, r.d), axis=1)
        assert np.max(dist) < 1e-12 and np.all(np.sum(w * r.d, axis=1) > 0)
        # ... which lies on the plane at F along fwd, where the pinhole ray of the same pixel crosses it
        pin = L.primary_rays(VIEW, 61, 37, 0.9, 0.0, Fd, 7, 12)
        t = Fd * (r.cam.fwd @ r.cam.fwd) / (pin.d @ r.cam.fwd)
        assert np.max(np.abs(pin.o + pin.d * t[:, None] - r.focus)) < 1e-6       # the view's columns are orthogonal to binary32's precision, no better


def test_equal_area_annuli_receive_equal_shares():
    n, K = 64, 8
    g = (np.arange(n) + 0.5) / n
    lx, ly = (a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij"))
    off = L.lens_offset(_cam(), 0.4, lx, ly)
    r2 = np.sum(off * off, axis=1) / 0.4 ** 2
    counts = np.bincount(np.floor(r2 * K).astype(np.int64), minlength=K)
    assert counts.tolist() == [n * n // K] * K
    # and the angle is uniform: equal sectors about the axis
    cam = _cam()
    ang = np.arctan2(off @ L.unit(cam.up), off @ L.unit(cam.right)) % (2 * np.pi)
    assert np.bincount(np.floor(ang / (2 * np.pi) * K).astype(np.int64) % K, minlength=K).tolist() == [n * n // K] * K


@pytest.mark.parametrize("noise", [False, True])
def test_a_closed_lens_is_the_pinhole_of_primary_ref(noise):
    nz = P.noise_texture() if noise else None
    for (W, H) in P.SIZES:
        cam = P.basis(VIEW, W, H, 0.9)
        jx, jy = P.jitter(W, H, 7, 12, nz)
        want = P.primary_rays(cam, W, H, jx, jy)
        for Fd in (1.0, 0.37, 55.0):
            r = L.primary_rays(VIEW, W, H, 0.9, 0.0, Fd, 7, 12, nz)
            assert np.array_equal(r.d, want) and np.array_equal(r.o, np.broadcast_to(cam.origin, want.shape))
    a = L.draws(61, 37, 7, 12, 4)
    b = P.jitter(61, 37, 7, 12)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])     # the lens draws FOLLOW the jitter's
    assert not np.array_equal(a[2], a[0]) and 0.0 <= a[2].min() and a[3].max() < 1.0


def test_the_noise_texture_does_not_move_the_lens_draws():
    a = L.primary_rays(VIEW, 61, 37, 0.9, 0.2, 2.0, 7, 12)
    b = L.primary_rays(VIEW, 61, 37, 0.9, 0.2, 2.0, 7, 12, P.noise_texture())
    assert np.array_equal(a.off, b.off) and not np.array_equal(a.d, b.d)


# ---------------------------------------------------------------- what the reference says about the GPU test's scenes
def test_the_board_leaves_out_less_than_one_per_cent_by_the_reference_alone():
    view = T.look(L.BOARD_EYE, L.BOARD_DIR)
    for (W, H) in P.SIZES:
        parity, tri, i, j, cmp, r = L.board_reference(view, W, H, L.USER_SEED, 0)
        nx, ny = L.board_cells(W, H)
        assert i.min() >= -nx and i.max() < nx and j.min() >= -ny and j.max() < ny          # the board fills the frame
        assert np.max(np.linalg.norm(r.dir, axis=1)) <= L.BOARD_DIR_LEN
        assert np.max(np.abs(r.focus[:, 2] + L.BOARD_F)) < 1e-6                              # the focal points lie on the board
        left = 1.0 - float(np.mean(cmp))
        print("%dx%d: %.3f %% of the pixels within %.3g of an edge" % (W, H, 100.0 * left, L.board_edge_eps()))
        assert left <= 0.01
        assert 0.3 < parity.mean() < 0.7 and 0.3 < tri.mean() < 0.7                          # both materials and both triangles of a quad are seen


def test_the_spot_is_two_pixels_wide_and_its_disc_at_least_six():
    half, rho, half_diag, centre, hits = L.spot_numbers()
    px = L.SPOT_W / (2.0 * (L.SPOT_W / L.SPOT_H) * math.tan(0.5 * float(np.float32(L.SPOT_VFOV))))
    assert abs(2.0 * half / L.SPOT_Z * px - 2.0) < 1e-12 and rho >= 6.0 and hits == 4.0 * L.SPOT_SAMPLES
    assert centre[1] - (rho + half_diag + 1.0) > 1.0 and centre[0] - (rho + half_diag + 1.0) > 1.0      # the whole disc lies inside the frame: nothing is lost at a border


# ---------------------------------------------------------------- launch plan
def test_lens_keeps_a_wavefront_off_packets_and_the_path_kernel_and_changes_nothing_else(tmp_path):
    exe = str(tmp_path / "plan_fact_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "tools", "plan_fact_check.cpp")], check=True)
    p = subprocess.run([exe, "lens"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = json.loads(p.stdout)
    assert out["cases"] == 9 * 512 * 3 * 2 * 3
    assert 0 < out["with_path"] < out["cases"] and 0 < out["with_packet"] < out["cases"] and 0 < out["with_quads"]      # the grid reaches the plans the lens takes away


# ---------------------------------------------------------------- bindings
NEW = ("lpt_renderer_set_lens", "lpt_renderer_get_lens", "lpt_renderer_primary_rays")


def test_bindings_agree_on_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "lpt.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "loupiote_hip", "src", "ffi.rs")).read()
    safe = open(os.path.join(ROOT, "bindings", "rust", "loupiote_hip", "src", "lib.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "loupiote.hpp")).read()
    for n in NEW:
        m = re.search(r"\bint %s\(([^;]*)\);" % n, header)
        assert m, n
        n_args = len(m.group(1).split(","))
        assert n in A.SIGNATURES and len(A.SIGNATURES[n][1]) == n_args, n
        m = re.search(r"pub fn %s\(([^;]*)\) -> c_int;" % n, ffi)
        assert m and len(m.group(1).split(",")) == n_args, n
        assert "%s(" % n in hpp and "ffi::%s(" % n in safe, n
        assert hasattr(A.lib(), n)
    assert A.lib().lpt_abi_version() == 6      # new entry points only: no layout changed
    assert "SPEC.md §25" in header and "lpt_renderer_set_lens" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("set_lens", "lens", "primary_rays"):
        assert hasattr(lp.Renderer, name)
    assert isinstance(lp.Renderer.lens, property)


def test_null_handles_are_refused_before_anything_else():
    lib = A.lib()
    r, f = C.c_float(-1.0), C.c_float(-1.0)
    buf = np.zeros(3, np.float32)
    view = np.eye(4, dtype=np.float32).reshape(16)
    assert lib.lpt_renderer_set_lens(None, 0.1, 1.0) == A.LPT_ERR_INVALID_ARG and b"lpt_renderer_set_lens" in lib.lpt_last_error()
    assert lib.lpt_renderer_get_lens(None, C.byref(r), C.byref(f)) == A.LPT_ERR_INVALID_ARG and (r.value, f.value) == (-1.0, -1.0)
    assert lib.lpt_renderer_primary_rays(None, A.ptr(view), 0, A.ptr(buf), A.ptr(buf)) == A.LPT_ERR_INVALID_ARG and b"lpt_renderer_primary_rays" in lib.lpt_last_error()
    assert np.all(buf == 0.0)
