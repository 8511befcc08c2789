"""The edge-case builders of tests/hgtest/edges.py, checked without a GPU: every case reaches the edge classes it claims (pixel counts
printed per builder), the oracle agrees with a second, independent model of the nearest rule on every pixel, and a few answers are
checked by hand, so that a mistake shared by the oracle and a kernel cannot pass."""
import numpy as np
import pytest

from hgtest import edges as E
from hgtest import oracle as O

# what each case claims: class -> least number of covered pixels (spans for E5)
PIECEWISE_CLAIMS = {
    "pos": {"E1 tie x>=0": 32, "E1 tie y>=0": 32, "E2 low in": 32, "E2 low out": 32, "E3 high in, next row": 32, "E3 high in, past the end": 2,
            "E3 high in y": 32, "E3 high out": 32, "E5 first past limit": 32, "E5 last past limit": 32},
    "exact": {"E1 tie x>=0": 32, "E2 low in": 32, "E3 high in, next row": 32, "E3 high in, past the end": 2, "E5 first on limit": 32,
              "E5 last on limit": 32},
    "neg": {"E1 tie x<0": 32, "E1 tie y<0": 32, "E1 -0.5": 32, "E2 low out": 32, "E3 high in, same row": 32, "E4 rx<0, index>=0": 32,
            "E4 index<0": 32, "E5 last past limit": 32},
    "dense": {"E1 tie x>=0": 32, "E2 low out": 32, "E3 high in, next row": 32, "E3 high out": 32, "E5 last past limit": 32},
    "negy": {"E1 tie y<0": 32, "E3 high in, next row": 32, "E4 index<0": 32, "E4 ry<0, index>=0": 16},
}
GEOMETRIC_CLAIMS = {
    "affine_half": {"E1 tie x>=0": 32, "E1 tie y>=0": 32, "E2 low in": 32, "E2 low out": 32, "E3 high in, next row": 32,
                    "E3 high in, past the end": 2, "E3 high out": 32},
    "affine_q1": {"E1 tie x>=0": 32, "E6 Q1": 32, "E3 high in, next row": 16},
    "affine_q1_neg": {"E1 tie x>=0": 32, "E6 -Q1": 32, "E3 high in, next row": 16},
    "affine_below": {"E3 high in, next row": 16, "E3 high in, past the end": 1, "E2 low out": 32},
    "proj_q1": {"E1 tie x>=0": 32, "E6 Q1": 32, "E3 high in, next row": 16},
    "proj_ieee": {"E1 tie x>=0": 32, "E2 low out": 32, "E3 high in, next row": 32, "E3 high out": 32},
}


def _claims_met(counts, claims, what):
    print(what, counts)
    short = {k: (counts[k], v) for k, v in claims.items() if counts[k] < v}
    assert not short, (what, short)


@pytest.mark.parametrize("twin", [False, True], ids=["one_fma", "two_round"])
@pytest.mark.parametrize("name", list(E.PIECEWISE))
def test_piecewise_builders_hit_their_edges(name, twin):
    case = E.piecewise(name, twin)
    sp, tris, msx, msy, dp, geom, img = case
    out, wmap, inv, sx, sy, valid = E.piecewise_taps(case)
    exact = np.all(inv[:, :4] == np.float32([0.5, 0, 0, 0.5]), axis=1)
    assert exact.all() != twin, "the base mesh has exact half-scale inverses; its twin does not"
    assert np.array_equal(out, E.nearest(img, sx, sy, valid, msx, msy))
    _claims_met(E.classify(sx, sy, valid, img.shape[1], img.shape[0], msx, msy, wmap), PIECEWISE_CLAIMS[name], (name, twin))


@pytest.mark.parametrize("name", list(E.GEOMETRIC))
def test_geometric_builders_hit_their_edges(name):
    case = E.GEOMETRIC[name]()
    kind, m, img, geom = case
    sx, sy, cov = E.geometric_coords(case)
    assert np.array_equal(O.warp_inverse_geometric(kind, m, img, *geom), E.nearest(img, sx, sy, cov))
    _claims_met(E.classify(sx, sy, cov, img.shape[1], img.shape[0]), GEOMETRIC_CLAIMS[name], name)


def test_known_answers_without_the_oracle():
    """Q1: s = 0.49999999999999994 reads column / row 0, not 1; 1 + Q1 is the tie 1.5 and reads 2.  E3: s in [W - 0.5, W) on row r
    reads pixel (0, r + 1); on the last row it reads nothing.  -Q1 fails the bounds test although Math.round gives 0."""
    kind, m, img, geom = E.GEOMETRIC["affine_q1"]()
    out = O.warp_inverse_geometric(kind, m, img, *geom)
    x0, y0 = geom[0], geom[1]
    assert np.array_equal(out[0 - y0, 0 - x0], img[0, 0])           # (Q1, Q1) -> (0, 0)
    assert np.array_equal(out[1 - y0, 0 - x0], img[2, 0])           # (Q1, 1.5) -> (0, 2)
    assert np.array_equal(out[0 - y0, 3 - x0], img[0, 4])           # (3.5, Q1) -> (4, 0)
    kind, m, img, geom = E.GEOMETRIC["affine_q1_neg"]()
    out = O.warp_inverse_geometric(kind, m, img, *geom)
    assert not out[:, 0 - geom[0]].any() and not out[0 - geom[1]].any()  # s = -Q1: outside
    assert np.array_equal(out[1 - geom[1], 1 - geom[0]], img[1, 1])     # 1 - Q1 == 0.5 exactly: rounds up
    kind, m, img, geom = E.GEOMETRIC["affine_half"]()
    H, W = img.shape[:2]
    out = O.warp_inverse_geometric(kind, m, img, *geom)
    xe = 2 * W - 1 - geom[0]                                         # s_x = W - 0.5
    for r in range(H - 1):
        assert np.array_equal(out[2 * r - geom[1], xe], img[r + 1, 0]), r
    assert not out[2 * (H - 1) - geom[1], xe].any()                   # last row: index W * H
    assert not out[:, xe + 1].any()                                   # s_x = W: outside
    assert np.array_equal(out[-1 - geom[1] + 0, 0 - geom[0]], np.zeros(4, np.uint8))   # s = (0, -0.5): outside
    assert np.array_equal(out[0 - geom[1], 0 - geom[0]], img[0, 0])


def test_piecewise_known_answers_without_the_oracle():
    """Negative minima: a pixel at round(sx) = -1 reads the previous row's last pixel; on row 0 it reads nothing.  minSrcY < 0 with
    round(sx) >= W: row -1 plus W + k reads pixel k of row 0."""
    case = E.piecewise("neg")
    sp, tris, msx, msy, dp, geom, img = case
    out, wmap, inv, sx, sy, valid = E.piecewise_taps(case)
    H, W = img.shape[:2]
    hit = valid & (sx == -1.0) & (sy >= 0) & (sy < H + msy)
    assert hit.sum() >= 8
    for r, c in zip(*np.nonzero(hit)):
        ry = int(E.js_round(sy[r, c]))
        want = img[ry - 1, W - 1] if ry > 0 else np.zeros(4, np.uint8)
        assert np.array_equal(out[r, c], want), (r, c, ry)
    case = E.piecewise("negy")
    sp, tris, msx, msy, dp, geom, img = case
    out, wmap, inv, sx, sy, valid = E.piecewise_taps(case)
    hit = valid & (sy == -1.0) & (sx >= W) & (sx < W + msx)
    assert hit.sum() >= 8
    for r, c in zip(*np.nonzero(hit)):
        assert np.array_equal(out[r, c], img[0, int(E.js_round(sx[r, c])) - W]), (r, c)
