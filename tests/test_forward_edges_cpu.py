"""The forward edge builders of tests/hgtest/fwd_edges.py, checked without a GPU: every case reaches the classes it claims, has the
admission code it claims from hg_forward_tiles_admissible itself (which pins each host limit at its value and just past it), and the
classifier's own last-writer resolution equals the oracle's bytes on an image that names every source pixel -- two independent
statements of the reference loops agree before either judges a kernel.  A few answers are checked by hand."""
import numpy as np
import pytest

from hgtest import fwd_edges as F
from hgtest import hip
from hgtest import oracle as O

HG = hip.load()
GEO = F.geometric_cases()
PW = F.piecewise_cases()
FUZZ_SEED, FUZZ_DRAWS = 2025, 420          # (tests/test_gpu_forward_edges.py runs the same draws)


def _floor(counts, claims, what):
    print(what, {k: v for k, v in counts.items() if k not in ("alias_left", "alias_right")})
    short = {k: (counts[k], v) for k, v in claims.items() if counts[k] < v}
    assert not short, (what, short)


def _geo_claims(name, c):
    """Least counts per class, by builder (G1 .. G7)."""
    if name.startswith("ties_s1_"):
        return {"tie_x": 130 * c["W"], "tie_y": 130 * c["W"]}, 130      # every writer is a tie on both axes; per tile side: 130 rows
    if name.startswith("ties_s15_"):
        return {"tie_x": 32 * 45, "tie_y": 32 * 45, "overwritten": 32}, 32 if c["admit"] else 0      # (width 63: its last column is no tie)
    if name.startswith("slope_") and "_aff_" in name:
        return {"tie_x": 100, "tie_y": 100}, 0
    if name.startswith("slope_") and "_proj_" in name:
        return {"tie_x": 100, "overwritten": 1000, "writers_max": 3}, 0
    if name.startswith("near_singular"):
        return {"writers_max": 32, "tie_x": 1000}, 0
    if name.startswith("minify"):
        return {"writers_max": c["writers"]}, 0
    if name.startswith("passes"):
        return {"pass_rows": 80, "writers_max": 8}, 0
    if name == "tall_65535":
        return {"pass_rows": 8000, "tie_y": 65535 * 16}, 0
    if name.startswith("wide_"):
        return {"tie_x": 65535 * 16, "written": 65535 * 16}, 0
    return {"written": 1}, 0


@pytest.mark.parametrize("name", list(GEO))
def test_geometric_builders_hit_their_classes(name):
    c = GEO[name]
    assert HG.forward_tiles_admissible(c["kind"], c["m"], c["W"], c["H"], c["geom"]) == c["admit"], (name, c["geom"])
    counts, win = F.classify_geometric(c)
    claims, per_side = _geo_claims(name, c)
    _floor(counts, claims, name)
    assert min(counts["border_tie"].values()) >= per_side, (name, counts["border_tie"])
    img = F.rank_image(c["W"], c["H"])
    assert np.array_equal(O.warp_forward_geometric(c["kind"], c["m"], img, *c["geom"]), F.expected_geometric(c, img, win)), name


def test_every_admission_code_occurs_near_singular():
    codes = {GEO[f"near_singular_{d:g}"]["admit"] for d in F.NEAR_SINGULAR_DIFFS}
    assert codes == {1, 2}
    m = GEO["near_singular_3e-12"]["m"]
    assert abs(m[0] * m[3] - m[2] * m[1]) > F.DET_MIN                 # refused by the round trip, not by the determinant ...
    m = GEO["near_singular_1e-13"]["m"]
    assert abs(m[0] * m[3] - m[2] * m[1]) < F.DET_MIN                 # ... and by the determinant


@pytest.mark.parametrize("name", [n for n in GEO if n.startswith("alias_")])
def test_alias_limit_reaches_every_column(name):
    """At least 16 writers at each of d = 1..30 on the side(s) the case names, writers from v = -1 into row 0 and from v = objH into the
    last row; nothing beyond column 30 (31 on the right: u = objW - 1 + d) where the case is admitted, something beyond in its twin."""
    c = GEO[name]
    counts, _ = F.classify_geometric(c)
    left, right = counts["alias_left"], counts["alias_right"]
    if "left" in name or "both" in name:
        assert min(left[1:F.ALIAS + 1]) >= 16 and counts["alias_last_row"] >= F.ALIAS, (name, left)
        assert (left[F.ALIAS + 1] == 0) == (c["admit"] != 0 or "30.5" in name), (name, left)
    if "right" in name or "both" in name:
        assert min(right[1:F.ALIAS + 2]) >= 16 and counts["alias_row0"] >= F.ALIAS, (name, right)
        assert (right[F.ALIAS + 2] == 0) == (c["admit"] != 0), (name, right)


def test_limits_are_pinned_on_both_sides():
    """The remaining terms of fwd_tile_param at their exact values: window width 64 / 63, source 65535 / 65536 in both directions."""
    ident = np.float64([1, 0, 0, 1, 0, 0])
    assert HG.forward_tiles_admissible(0, ident, 64, 8, (0, 0, F.WIN_MIN, 8)) == 2
    assert HG.forward_tiles_admissible(0, ident, 64, 8, (0, 0, F.WIN_MIN - 1, 8)) == 0
    assert HG.forward_tiles_admissible(0, ident, 64, 8, (0, 0, F.WIN_MIN, 0)) == 0
    t = np.float64([0, 1, 1, 0, 0, 0])
    assert HG.forward_tiles_admissible(0, t, 16, F.SRC_MAX, (0, 0, F.SRC_MAX, 16)) == 2
    assert HG.forward_tiles_admissible(0, t, 16, F.SRC_MAX + 1, (0, 0, F.SRC_MAX + 1, 16)) == 0
    for kind in (0, 1):                                                # |corner image| < 1e7 (affine) resp. 1e5, exclusive
        lim = F.IMAGE_MAX[kind]
        m = [1, 0, 0, 1, 0, 0] if kind == 0 else [1, 0, 0, 0, 1, 0, 0, 0]
        for W, admit in ((10, 2), (11, 0)):                            # x' = (largest entry) x: the corner image of W = 11 is the limit itself
            mm = np.float64(m)
            mm[0] = F.ENTRY_MAX[kind]
            x1 = float(mm[0] * (W - 1))
            assert (x1 < lim) == (admit == 2) and x1 <= lim
            assert HG.forward_tiles_admissible(kind, mm, W, 4, (0, 0, int(x1) + 1, 4)) == admit, (kind, W)


def test_geometric_known_answers():
    """Rank 0: one pixel written, with the last source pixel.  Both slopes 0: source row y lands on one pixel, the winner is x = W - 1.
    The 64-wide window with 30 columns outside on both sides: columns below 34 keep the direct writer of the row below the aliased
    one, columns from 34 take the pixel that aliased in from the left of the NEXT source row (it is later in raster order)."""
    c = GEO["rank0"]
    img = F.image(c)
    out = O.warp_forward_geometric(c["kind"], c["m"], img, *c["geom"])
    assert np.count_nonzero(out.any(-1)) == 1 and np.array_equal(out[4 - 2, 41 - 10], img[-1, -1])
    c = GEO["slope_both_0"]
    img = F.image(c)
    out = O.warp_forward_geometric(c["kind"], c["m"], img, *c["geom"])
    for y in (0, 1, 7, 148, 149):                                      # (y + 1, round(y / 4)); rows y = 4 k + 2 are ties and round up
        assert np.array_equal(out[int(F.js_round(np.float64(y / 4))), y + 1], img[y, c["W"] - 1]), y
    c = GEO["alias_both_w64"]
    img = F.image(c)
    out = O.warp_forward_geometric(c["kind"], c["m"], img, *c["geom"])
    H = c["H"]
    for r in range(H - 2):
        assert np.array_equal(out[r, :34], img[r + 1, 30:64]), r
        assert np.array_equal(out[r, 34:], img[r + 2, 0:30]), r


def test_absorbed_slope_lands_whole_rows_on_a_tile_border():
    """From row 53688 on every x of a row is the same tie, which rounds to the first column of the tile at 64; several pixels of that
    column are won by x = 1 .. 3 of such rows: pixels a candidate interval cut by the slope's sign would hand to x = 0, or leave empty."""
    c = GEO["slope_absorbed"]
    counts, win = F.classify_geometric(c)
    assert counts["border_tie"]["left"] >= 100000 and counts["tie_x"] == counts["border_tie"]["left"], counts["border_tie"]
    col = win.reshape(c["geom"][3], c["geom"][2])[:, F.TILE]
    assert ((col >= 53688 * c["W"]) & (col % c["W"] >= 1)).sum() >= 3, col


def _pw_claims(name, c):
    if name == "shifts_5":
        return {"tie_x": 64}, {k: 64 for k in range(-2, 3)}
    if name == "shifts_7":
        return {}, {k: 64 for k in range(-3, 4)}
    if name.startswith("collapsed"):
        return {"writers_max": 64, "overwritten": 64}, {}
    if name.startswith("rotated"):
        return {"tie_x": 30000, "tie_y": 30000}, {}
    if name.startswith("minify_64"):
        return {"writers_max": 320, "tie_x": 1000}, {}
    if name.startswith("dense"):
        return {"overwritten": 2000}, {}
    if name == "off_image":
        return {"lost_to_zero": 64, "zero_over_earlier": 32, "src_wrapped": 64}, {}
    return {"written": 600}, {}


@pytest.mark.parametrize("name", list(PW))
def test_piecewise_builders_hit_their_classes(name):
    c = PW[name]
    maps = F.piecewise_maps(c)
    counts, win, sidx = F.classify_piecewise(c, maps)
    claims, shift = _pw_claims(name, c)
    _floor(counts, claims, name)
    assert all(counts["shift"][k] >= v for k, v in shift.items()), (name, counts["shift"])
    if name == "shifts_5":
        assert counts["shift"][-3] == 0 and counts["shift"][3] == 0 and counts["shift_beyond"] == 0
    img = F.rank_image(c["W"], c["H"])
    assert np.array_equal(F.piecewise_oracle(c, img), F.expected_piecewise(c, img, win, sidx)), name
    fwd = maps[1].astype(np.float64)
    det = fwd[:, 0] * fwd[:, 3] - fwd[:, 2] * fwd[:, 1]
    if name in ("collapsed_collinear", "collapsed_coincident"):
        assert det[0] == 0.0 and np.isfinite(fwd).all()
    if name == "collapsed_tiny_det":
        assert 0.0 < abs(det[0]) < 1e-4
    if name == "rotated_90":
        assert (fwd[:, 0] == 0).all() and (fwd[:, 3] == 0).all()
    if name == "rotated_90_ulp":
        assert 0 < np.count_nonzero(fwd[:, 0]) < fwd.shape[0]
    if name == "entry_2e6":
        assert np.abs(fwd).max() > F.PW_ENTRY_MAX
    if name == "nan_vertex":
        assert np.isnan(fwd).any() and not np.isnan(fwd).all()
    if name.startswith("many_"):
        ids = maps[0].astype(np.int64)
        first = c["first_id"]
        if first + 64 < 65536:                                         # ids first .. 32767 own cells as themselves, 32768 .. as negative values (skipped)
            assert (ids >= first).sum() >= 1000 and (ids < -1).sum() >= 1000 and ids.max() == 32767 and ids[ids < -1].min() == -32768
        else:                                                          # ids .. 65534 are negative, 65536 .. select the padding's matrices 0 .. 31
            assert (ids < -1).sum() >= 1000 and ((ids >= 0) & (ids < 32)).sum() >= 1000 and ids[ids < -1].max() == -2 and ids.max() == 31
            assert not np.array_equal(fwd[0], fwd[first])             # ... which is another map than the real triangles'
    if "entries" in c:                                                # every triangle's destination box crosses the tile at the origin
        dp, tr = c["dp"].reshape(-1, 2), c["tris"].reshape(-1, 3)
        lo, hi = dp[tr].min(1) - c["geom"][:2], dp[tr].max(1) - c["geom"][:2]
        assert ((lo < F.TILE).all(1) & (hi >= 0).all(1)).sum() == c["entries"] == tr.shape[0]
        assert (np.floor(lo[:, 0]) - 2 >= 0).all() and (np.ceil(hi[:, 0]) + 2 < c["geom"][2]).all()     # one aliasing shift only


def test_dense_meshes_fill_the_capacity_steps():
    n = [F.dense(s)["entries"] for s in F.DENSE.values()]
    assert F.PW_CAP0 < n[0] <= 2 * F.PW_CAP0 < n[1] <= F.PW_CAP_MAX < n[2]
    c = PW["minify_64_8x8"]
    assert c["entries"] == 2 * F.PW_CAP0
    rows = c["My"] - c["msy"]
    assert c["entries"] * rows // 8 > F.PW_RECORDS and (c["Mx"] - c["msx"]) // F.PW_SEG_W * 2 > F.PW_SEGMENTS // 4
    c = PW["minify_64_1x1"]
    assert 2 * (c["My"] - c["msy"]) > F.PW_RECORDS and (c["Mx"] - c["msx"]) // F.PW_SEG_W * F.PW_RECORDS > F.PW_SEGMENTS


def test_box_limits():
    assert PW["box_65535"]["Mx"] - PW["box_65535"]["msx"] == F.SRC_MAX and PW["box_65536"]["Mx"] - PW["box_65536"]["msx"] == F.SRC_MAX + 1


def test_fuzz_yields_enough_admitted_frames():
    cases, refused, skipped = F.fuzz(FUZZ_SEED, FUZZ_DRAWS, HG.forward_tiles_admissible)
    print(len(cases), "admitted,", refused, "refused,", skipped, "windows too large")
    assert len(cases) >= 300 and refused <= FUZZ_DRAWS // 2
    assert sum(c["admit"] == 1 for c in cases) >= 3 and sum(c["kind"] == 1 for c in cases) >= 100
    for c in cases[::15]:                                              # (the whole set is compared on the GPU; a sample of it here)
        img = F.rank_image(c["W"], c["H"])
        assert np.array_equal(O.warp_forward_geometric(c["kind"], c["m"], img, *c["geom"]), F.expected_geometric(c, img)), c["name"]
