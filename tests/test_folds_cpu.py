"""The folded and degenerate meshes of tests/hgtest/folds.py, checked without a GPU: the oracle's triangle map is the "largest covering
id" model on every pixel (every triangle rasterised alone, the covers stacked), the oracle agrees with the second model of the nearest
rule, every case has the overlap, holes, depth and pieces per row it claims (counts printed per case), and a few pictures are known
without the oracle."""
import numpy as np
import pytest

from hgtest import edges as E
from hgtest import folds as FO

# what each case claims: conditions below what the reference alone gives (tests/hgtest/folds.classify)
AT_LEAST = {
    "fold_over": {"overlap": 6000, "holes": 1500},
    "fold_over_neg": {"overlap": 6000, "holes": 1500},
    "fold_under": {"overlap": 6000},
    "fold_over_rev": {"overlap": 6000},
    "nan_last": {"nan_holes": 3000},
    "nan_collinear": {"nan_holes": 3000},
    "sliver_last": {"overlap": 16, "holes": 1},
    "inner_over": {"overlap": 6000, "holes": 1000},
    "inner_nan": {"nan_holes": 2000},
}
EXACTLY = {
    "fold_under": {"holes": 0, "nan_holes": 0},
    "fold_over_rev": {"holes": 0, "nan_holes": 0},
    "nan_first": {"holes": 0, "nan_holes": 0},
    "none_collinear": {"depth": 1, "overlap": 0},
    "none_coincident": {"depth": 1, "overlap": 0},
}
EXACTLY.update({name: {"depth": K, "pieces": 4 * K} for name, K in FO.DEEP.items()})
EXACTLY.update({name: {"depth": K, "pieces": 4 * K + 2} for name, K in FO.DEEP_WIDE.items()})


@pytest.mark.parametrize("name,twin", FO.all_cases(), ids=lambda v: v if isinstance(v, str) else ("two_round" if v else "base"))
def test_fold_cases_meet_their_claims(name, twin):
    c = FO.case(name, twin)
    sp, tris, msx, msy, dp, geom, img = c
    out, wmap, fwd, inv, sx, sy, valid = FO.taps(name, twin)
    cl = FO.classify(c, inv)
    top = cl.pop("top")
    print(name, twin, "T", tris.size // 3, "geom", geom, "minSrc", (msx, msy), cl)
    assert np.array_equal(top, wmap.reshape(top.shape)), "the map is not 'largest covering id'"
    assert np.array_equal(out, E.nearest(img, sx, sy, valid, msx, msy))
    if name in FO.FOLDS:
        exact = bool(np.all(inv[:, :4] == np.float32([0.5, 0, 0, 0.5])))
        assert exact != twin, "the base mesh has exact half-scale inverses; its twin does not"
    if name in FO.NANS:
        t = 0 if name == "nan_first" else tris.size // 3 - 1
        assert np.isnan(inv[t]).all(), inv[t]
    short = {k: (cl[k], v) for k, v in AT_LEAST.get(name, {}).items() if cl[k] < v}
    wrong = {k: (cl[k], v) for k, v in EXACTLY.get(name, {}).items() if cl[k] != v}
    assert not short and not wrong, (name, twin, short, wrong)
    if cl["overlap"]:
        assert cl["discriminating"] * 10 >= cl["overlap"] * 9, cl


def _block_alone(block, geom, img, where):
    """The picture of one tie_mesh block by its formula (source = (dst - t) / 2 + origin, exact in f64) on the cells `where`."""
    x0, y0, _, _, _, _, (ox, oy) = block
    x = np.arange(geom[2], dtype=np.float64)[None, :] + geom[0]
    y = np.arange(geom[3], dtype=np.float64)[:, None] + geom[1]
    sx = np.broadcast_to((x - ox) / 2 + x0, where.shape).copy()
    sy = np.broadcast_to((y - oy) / 2 + y0, where.shape).copy()
    return E.nearest(img, sx, sy, where)


def _cover_of(c, ids):
    """Cells that the triangles `ids` of a case fill when rasterised alone."""
    sp, tris, msx, msy, dp, geom, img = c
    t3 = np.asarray(tris).reshape(-1, 3)[ids].ravel()
    return FO.covers(dp, t3, geom).any(0)


@pytest.mark.parametrize("name", ["fold_under", "nan_first", "none_collinear", "none_coincident"])
def test_what_lies_under_or_rasterises_nothing_leaves_block_a_alone(name):
    c = FO.case(name)
    sp, tris, msx, msy, dp, geom, img = c
    T = tris.size // 3
    a_ids = np.arange(T - 160, T) if name in ("fold_under", "nan_first") else np.arange(160)
    on_a = _cover_of(c, a_ids)
    assert on_a.sum() >= 512 * 40 - 600
    out = FO.taps(name)[0]
    want = _block_alone(FO.A, geom, img, on_a)
    assert want.any() and np.array_equal(out[on_a], want[on_a])


def test_fold_over_shows_the_upper_block_alone_inside_the_overlap():
    c = FO.case("fold_over")
    sp, tris, msx, msy, dp, geom, img = c
    inside = _cover_of(c, np.arange(160)) & _cover_of(c, np.arange(160, 208))
    assert inside.sum() >= 6000
    out, under = FO.taps("fold_over")[0], FO.taps("fold_under")[0]
    want = _block_alone(FO.BLK, geom, img, inside)
    assert np.array_equal(out[inside], want[inside])
    # ... whose columns from 255 on are outside the source: holes over block A's pixels
    assert (~want[inside].any(-1)).sum() >= 1500 and under[inside].any(-1).sum() >= 6000
    differ = (out != under).any(-1)
    assert np.array_equal(differ, differ & inside) and differ.sum() >= 5500
    assert np.array_equal(FO.taps("fold_over_rev")[0], under)


def test_a_nan_triangle_listed_last_blanks_its_interior():
    c = FO.case("nan_last")
    sp, tris, msx, msy, dp, geom, img = c
    T = tris.size // 3
    out, wmap = FO.taps("nan_last")[:2]
    tri = _cover_of(c, [T - 1])
    assert tri.sum() >= 3000
    assert (wmap.reshape(tri.shape)[tri] == T - 1).all() and not out[tri].any()
    assert np.array_equal(out[~tri], FO.taps("nan_first")[0][~tri])
