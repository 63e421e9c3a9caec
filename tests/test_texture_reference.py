"""CPU: the oracle's texture and environment lookups (SPEC.md §9; `orc_texture_lookup`, `orc_env_lookup`) against the binary64 reference tests/texture_ref.py over the whole
case set — every image size, every coordinate class, the rows beyond the int32 range that §9's saturation rule decides, every probe and direction.  Every row must lie
within the reference's DERIVED bound (none is measured), the exact rows must be equal bit for bit (all 256 entries of both decode tables are such rows on the 16x16
image), every mutant of texture_ref.MUTANTS must be rejected, and the rows the alpha decision leaves out stay under their cap.  Run with -s for the reports.

Measured, the oracle's worst |error| / bound (limit 1), sRGB image / linear image: 1x1 0 / 0, 1x7 0.64 / 0.59, 7x1 0.62 / 0.64, 2x2 0.27 / 0.27, 3x3 0.50 / 0.50,
4x4 0.40 / 0.38, 5x3 0.50 / 0.50, 8x4 0.52 / 0.38, 9x5 0.50 / 0.50, 16x16 0.72 / 0.70, 23x17 0.61 / 0.54, 64x64 0.91 / 0.83; probes 2x1 0.67, 1x2 0.66, 2x2 0.42, 5x3 0.46,
8x4 0.52, 16x8 0.56 (0 at the exact poles); the rows beyond int32 are decided by the saturation rule alone.  Mask rows left out: at most 1.8 % (3x3, color.w 0.7)."""
import functools

import numpy as np
import pytest

import texture_ref as R
from oracle import gltf_oracle as G, orc

F = np.float32


@functools.lru_cache(maxsize=None)
def oracle_scene(W, H):
    """images 0, 1 of the size and the probe of no size in particular"""
    v = np.zeros(3, G.VERTEX_DT)
    v["position"][1, 0] = v["position"][2, 1] = 1.0
    return orc.OracleScene(v, np.zeros(1, np.uint32), G.default_material(), G.default_light(), images=[R.image(W, H, 0), R.image(W, H, 1)])


def oracle_lookup(W, H, k, tu, tv, srgb):
    uv = np.ascontiguousarray(np.stack([tu, tv], axis=1), F)
    out = np.zeros((len(uv), 4), F)
    orc.lib().orc_texture_lookup_n(oracle_scene(W, H).h, k, orc._p(uv), len(uv), int(srgb), orc._p(out))
    return out


@functools.lru_cache(maxsize=None)
def oracle_rows(W, H):
    tu, tv = R.coords(W, H)
    return tu, tv, oracle_lookup(W, H, 0, tu, tv, True), oracle_lookup(W, H, 1, tu, tv, False)


def oracle_env(rgbe, d):
    v = np.zeros(3, G.VERTEX_DT)
    sc = orc.OracleScene(v, np.zeros(1, np.uint32), G.default_material(), G.default_light(), probe=rgbe)
    d = np.ascontiguousarray(d, F)
    out = np.zeros((len(d), 3), F)
    orc.lib().orc_env_lookup_n(sc.h, orc._p(d), len(d), orc._p(out))
    return out


def test_tables_and_the_storage_models():
    """the sRGB table is the oracle's, entry by entry; the models of the two storage layouts return the image's own texels at every size (so only a mutant misreads them)"""
    assert np.array_equal(R.SRGB_LUT, np.array([orc.lib().orc_srgb_lut(b) for b in range(256)], F))
    assert R.SRGB_LUT[0] == 0 and R.SRGB_LUT[255] == 1 and R.LINEAR_LUT[255] == 1
    for W, H in R.SIZES:
        tu, tv = R.coords(W, H)
        tu, tv = tu[::7], tv[::7]
        a = R.lookup(R.image(W, H), tu, tv, True)[0]
        for storage in ("atlas", "apron"):
            assert np.array_equal(a, R.lookup(R.image(W, H), tu, tv, True, storage)[0]), (W, H, storage)


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: "%dx%d" % s)
def test_oracle_lookup_within_the_bound_and_exact_rows_bit_equal(size):
    W, H = size
    tu, tv, got_s, got_l = oracle_rows(W, H)
    rep = {}
    for name, k, srgb, got in (("srgb", 0, True, got_s), ("linear", 1, False, got_l)):
        val, bound, exact = R.lookup(R.image(W, H, k), tu, tv, srgb)
        r = R.ratios(val, bound, got)
        rep[name] = float(r.max())
        assert np.all(r <= 1.0), (size, name, float(r.max()), int(np.argmax(r.max(axis=1))))
        assert exact.sum() >= 0.01 * len(tu) and np.all(bound[exact] == 0)
        assert np.array_equal(got[exact], val[exact].astype(F)), "an exact row is the tap itself"
    pv, pb, _ = R.pair(R.image(W, H, 0), R.image(W, H, 1), tu, tv)
    assert R.passes(pv, pb, np.concatenate([got_s[:, :3], got_l[:, 1:3]], axis=1))
    print("\noracle %dx%d: %d rows, %d exact; worst |error| / bound %s" % (W, H, len(tu), int(exact.sum()), "  ".join("%s %.3f" % kv for kv in rep.items())))


def test_every_table_entry_is_an_exact_row_of_the_16x16_image():
    """the texel centres of the 16x16 images return all 256 entries of the sRGB table and of b·(1/255), bit for bit"""
    y, x = np.mgrid[0:16, 0:16]
    tu, tv = ((x.reshape(-1) + 0.5) / 16).astype(F), ((y.reshape(-1) + 0.5) / 16).astype(F)
    for k, srgb, table in ((0, True, R.SRGB_LUT), (1, False, R.LINEAR_LUT)):
        img = R.image(16, 16, k)
        val, bound, exact = R.lookup(img, tu, tv, srgb)
        got = oracle_lookup(16, 16, k, tu, tv, srgb)
        assert exact.all() and np.array_equal(got, val.astype(F))
        assert np.array_equal(got[:, 0], table[img[..., 0].reshape(-1)]) and sorted(img[..., 0].reshape(-1)) == list(range(256))
        assert np.array_equal(got[:, 3], R.LINEAR_LUT[img[..., 3].reshape(-1)])


@pytest.mark.parametrize("size", R.OUTSIDE_SIZES, ids=lambda s: "%dx%d" % s)
def test_oracle_beyond_int32_follows_the_saturation_rule(size):
    """|t·size| from 2^31 to the end of the domain: every row is exact, x0 = wrap(sat(floor(fx))) names the texel, and the oracle returns it"""
    W, H = size
    tu, tv = R.outside(W, H)
    for k, srgb in ((0, True), (1, False)):
        val, bound, exact = R.lookup(R.image(W, H, k), tu, tv, srgb)
        got = oracle_lookup(W, H, k, tu, tv, srgb)
        pinned = np.all(bound == 0, axis=1)
        assert pinned.sum() >= len(tu) // 2 and R.passes(val, bound, got)
        assert np.array_equal(got[pinned], val[pinned].astype(F))
        assert np.all(np.isfinite(got))


@pytest.mark.parametrize("mutant", R.TEXTURE_MUTANTS)
def test_texture_mutant_is_rejected(mutant):
    """a misreading of §9 or of a storage layout in the reference must put the oracle beyond the bound; prints the share of rows that catch it per size"""
    storage = {"tile_stride_floor": "atlas", "apron_column": "apron", "apron_row": "apron"}.get(mutant, "linear")
    share = {}
    for W, H in R.SIZES:
        tu, tv, got_s, got_l = oracle_rows(W, H)
        val, bound, _ = R.pair(R.image(W, H, 0), R.image(W, H, 1), tu, tv, storage, mutant)
        share["%dx%d" % (W, H)] = R.caught(val, bound, np.concatenate([got_s[:, :3], got_l[:, 1:3]], axis=1))
    print("\n%s (%s): share of rows beyond the bound %s" % (mutant, R.MUTANTS[mutant], "  ".join("%s %.3f" % kv for kv in share.items())))
    assert max(share.values()) > 0, "mutant %r is not rejected" % mutant
    # the stride shows only where a width that is no multiple of 8 meets more than one row of tiles; an apron's wrapped column wherever a lookup crosses the border
    must = {"tile_stride_floor": ("1x7", "9x5", "23x17"), "apron_column": ("3x3", "4x4", "23x17", "64x64"), "apron_row": ("3x3", "4x4", "23x17", "64x64")}.get(mutant, ("23x17", "64x64", "9x5"))
    assert all(share[s] > 0 for s in must), (mutant, share)


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: "%dx%d" % s)
def test_alpha_rows_left_out_stay_under_the_cap(size):
    """from the reference alone: at most 2 % of a size's mask rows lie within the bound of the cutoff, and every texel cell keeps a compared row"""
    W, H = size
    tu, tv = R.coords(W, H)
    for cw in (1.0, 0.7):
        a, b = R.alpha(R.image(W, H), cw, tu, tv)
        keep = R.mask_compared(a, b, 0.5)
        assert 1.0 - keep.mean() <= 0.02, (size, cw, 1.0 - keep.mean())
        cx = np.mod(np.floor(tu.astype(np.float64) * W - 0.5), W).astype(int)
        cy = np.mod(np.floor(tv.astype(np.float64) * H - 0.5), H).astype(int)
        cells = np.zeros((H, W), bool)
        cells[cy[keep], cx[keep]] = True
        assert cells.all(), (size, cw)
        print("\nalpha %dx%d color.w %.1f: %d of %d rows left out; kept %d, cut %d" % (W, H, cw, int((~keep).sum()), len(keep), int((a[keep] >= 0.5).sum()), int((a[keep] < 0.5).sum())))


def test_interpolate_is_exact_at_a_vertex_and_bounded_inside():
    rs = np.random.RandomState(5)
    uv = rs.uniform(-3, 4, (3, 500, 2)).astype(F)
    hu = rs.uniform(0, 1, 500).astype(F)
    hv = (rs.uniform(0, 1, 500) * (1 - hu)).astype(F)
    v, b = R.interpolate(uv[0], uv[1], uv[2], np.zeros(500, F), np.zeros(500, F))
    assert np.array_equal(v, uv[0].astype(np.float64))
    v, b = R.interpolate(uv[0], uv[1], uv[2], hu, hv)
    bw = (F(1) - hu) - hv
    got = (uv[0] * bw[:, None] + uv[1] * hu[:, None]) + uv[2] * hv[:, None]
    assert got.dtype == F and R.passes(v, b, got) and b.max() < 2e-6


@pytest.mark.parametrize("size", R.PROBES + ((1, 1),), ids=lambda s: "%dx%d" % s)
def test_oracle_env_lookup_within_the_bound(size):
    W, H = size
    rgbe = R.probe(W, H)
    rep = {}
    for name, d in R.directions(W, H).items():
        val, bound = R.env(rgbe, d)
        got = oracle_env(rgbe, d)
        r = R.ratios(val, bound, got)
        rep[name] = float(r.max())
        assert np.all(r <= 1.0), (size, name, float(r.max()))
    print("\noracle probe %dx%d: worst |error| / bound %s" % (W, H, "  ".join("%s %.3f" % kv for kv in rep.items())))
    if size != (1, 1):
        poles = R.directions(W, H)["poles"]
        u = np.full(len(poles), 0.5)
        assert np.array_equal(R.env_uv(poles)[0], u), "u = 1/2 at the poles whatever the zeros' signs"
    else:
        d = np.array([(np.nan, 0, 0), (0, 0, 0), (np.inf, 1, 0)], F)
        assert np.array_equal(oracle_env(rgbe, d), np.repeat(R.env(rgbe, d[:1])[0].astype(F), 3, axis=0)), "a 1x1 probe is constant, NaN included"


@pytest.mark.parametrize("mutant", R.ENV_MUTANTS)
def test_env_mutant_is_rejected(mutant):
    share = {}
    for W, H in R.PROBES:
        rgbe, d = R.probe(W, H), R.all_directions(W, H)
        val, bound = R.env(rgbe, d, mutant)
        share["%dx%d" % (W, H)] = R.caught(val, bound, oracle_env(rgbe, d))
    print("\n%s (%s): share of rows beyond the bound %s" % (mutant, R.MUTANTS[mutant], "  ".join("%s %.3f" % kv for kv in share.items())))
    assert all(share[s] > 0 for s in ("5x3", "8x4", "16x8")), (mutant, share)
