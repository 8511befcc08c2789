"""Edge-case inputs for the inverse warps, built from exact arithmetic, and a classifier of the pixels they produce.  CPU only.

Piecewise builders return (sp, tris, minSrcX, minSrcY, dst_pts, geom, image) and geometric builders (kind, m, image, geom): the
argument lists of tests/hgtest/oracle.py and tests/hgtest/bilinear.py.

The piecewise meshes are grids of half-integer source points whose destination is 2 * (src - origin) + t: every triangle's f32
inverse is then exactly [0.5, 0, 0, 0.5, c, d], so the source coordinate of every output pixel lies on the half-integer grid and
every other column and row is an exact Math.round tie.  A grid whose first column sits at minSrcX - 0.5 and whose last sits at
W + minSrcX + 0.5 puts pixels on both sides of both bounds (:1047) and makes the spans of its last cells end one pixel past a limit.

The classifier takes per-pixel (sx, sy) in f64 and counts the covered pixels of each class:
  E1 tie        s = k + 0.5 exactly, inside the bounds; k >= 0 and k < 0, each axis
  E2 low limit  s = minSrc exactly (in); s in [minSrc - 0.5, minSrc) (out, though it rounds into the window)
  E3 high limit s in [W + minSrc - 0.5, W + minSrc) (in): pixel minSrcX of the next row (minSrcX >= 0) or column W + minSrcX of
                the same row (minSrcX < 0), or an index >= W*H (-> 0) on the last row; s = W + minSrc exactly (out)
  E4 signed     in-bounds pixels with round(sx) < 0: the previous row's tail, or an index < 0 (-> 0); round(sy) < 0 with a
                non-negative index
  E5 span ends  spans (runs of one triangle id along a row) whose first or last pixel sits on a limit, or one pixel past it
  E6 Q1         |s| = 0.49999999999999994 (the f64 matrices of the geometric kinds)"""
import numpy as np

from . import bilinear as B
from . import oracle as O
from . import workloads as WL

Q1 = 0.49999999999999994                 # the largest double below 0.5: Math.round gives 0, floor(v + 0.5) in f64 gives 1


def js_round(v):
    """Math.round of f64 values, exactly (v - floor(v) is exact for |v| < 2^52)."""
    f = np.floor(v)
    return f + ((v - f) >= 0.5)


# ------------------------------------------------------------------------------------------------ piecewise builders

def tie_mesh(blocks):
    """Grid blocks (x0, y0, nx, ny, cw, ch, (ox, oy)): source points (x0 + i cw, y0 + j ch), destination 2 (src - (x0, y0)) + (ox, oy).
    Returns (sp, tris, dp) of the union (triangle ids in block order)."""
    sps, dps, trs, base = [], [], [], 0
    for x0, y0, nx, ny, cw, ch, (ox, oy) in blocks:
        i, j = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1))
        s = np.stack([x0 + i * cw, y0 + j * ch], -1).reshape(-1, 2).astype(np.float64)
        d = 2.0 * (s - [x0, y0]) + [ox, oy]
        assert np.array_equal(s.astype(np.float32), s) and np.array_equal(d.astype(np.float32), d), "points must be exact in f32"
        sps.append(s); dps.append(d)
        trs.append(WL.grid_triangles(nx, ny).astype(np.int64) + base)
        base += (nx + 1) * (ny + 1)
    sp = np.concatenate(sps).astype(np.float32).ravel()
    dp = np.concatenate(dps).astype(np.float32).ravel()
    return sp, np.concatenate(trs).astype(np.uint32), dp


def nudge(dp, vertex, ulps):
    """The two-rounding twin of a mesh: one destination vertex moved by `ulps` f32 units in the last place along x.  The triangles
    around it get an inverse whose :1383 sums are no longer exact (HG.affine_one_fma_form is false for the frame)."""
    d = np.array(dp, np.float32).reshape(-1, 2)
    for _ in range(ulps):
        d[vertex, 0] = np.nextafter(d[vertex, 0], np.float32(np.inf), dtype=np.float32)
    return d.ravel()


def piecewise_case(W, H, blocks, image=None, seed=1, geom=None):
    sp, tris, dp = tie_mesh(blocks)
    msx, msy = WL.src_min(sp)
    img = O.lcg_image(W, H, seed) if image is None else image
    return sp, tris, msx, msy, dp, WL.piecewise_geom(dp) if geom is None else geom, img


# name -> (W, H, blocks, seed).  The first column of "pos" / "neg" / "negy" is at minSrc - 0.5 and the last at W + minSrc + 0.5
# (W + 1 a multiple of the cell width): spans start one pixel before the low limit and end one pixel past the high one.  "exact"
# starts on minSrc and ends on W + minSrc: every span's first and last pixel sit on the limits.
PIECEWISE = {
    "pos": (255, 19, [(-0.5, -0.5, 16, 5, 16, 4, (2, 2))], 11),                  # minSrc (0, 0): the high-dword bounds form applies
    "exact": (256, 20, [(0.0, 0.0, 16, 5, 16, 4, (2, 2))], 12),                  # every span ends on a limit
    "neg": (255, 19, [(-3.5, -2.5, 16, 5, 16, 4, (2, 2))], 13),                  # minSrc (-3, -2): negative round(sx), round(sy)
    "negy": (255, 19, [(4.5, -2.5, 16, 5, 16, 4, (2, 2))], 14),                  # minSrc (5, -2): round(sy) < 0 with round(sx) >= W
    "dense": (255, 19, [(-0.5, -0.5, 64, 5, 4, 4, (2, 2))], 15),                 # "pos" in 4-pixel cells: rows of more than 200 spans
}


def piecewise(name, twin=False):
    W, H, blocks, seed = PIECEWISE[name]
    sp, tris, msx, msy, dp, geom, img = piecewise_case(W, H, blocks, seed=seed)
    if twin:
        dp = nudge(dp, 2 * (blocks[0][2] + 1) + 3, 2)                           # an interior vertex: the window stays the same
        assert WL.piecewise_geom(dp) == geom
    return sp, tris, msx, msy, dp, geom, img


def pad_triangles(sp, tris, dp, geom, n_total=32769):
    """The mesh with triangles appended up to n_total, all one triangle placed far below the window: they fill no cell of the map, and
    a mesh of more than 32767 triangles is outside the fast kernels' range (k_pw_fused runs in nearest mode too)."""
    far = geom[1] + geom[3] + 1000.0
    sp2 = np.concatenate([sp, np.float32([0, 0, 4, 0, 0, 4])])
    dp2 = np.concatenate([dp, np.float32([0, far, 8, far, 0, far + 8])])
    n = sp.size // 2
    extra = np.tile(np.uint32([n, n + 1, n + 2]), n_total - tris.size // 3)
    return sp2, np.concatenate([tris, extra]), dp2


# ------------------------------------------------------------------------------------------------ geometric builders

def _geo(kind, m, W, H, geom, seed):
    return kind, np.asarray(m, np.float64), O.lcg_image(W, H, seed), tuple(geom)


# name -> builder; the kernel that k_geo_fast instantiates for it (KIND of hg_last_geometric_kernel) is in GEOMETRIC_KIND
GEOMETRIC = {
    # f32-valued affine: half scale, the window reaches 1.5 pixels past every side: ties on every odd column and row
    "affine_half": lambda: _geo(0, [0.5, 0, 0, 0.5, 0, 0], 256, 24, (-3, -3, 2 * 256 + 6, 2 * 24 + 6), 21),
    # affine with doubles: column and row 0 need Q1's special case, every other column and row is an exact tie
    "affine_q1": lambda: _geo(0, [1, 0, 0, 1, Q1, Q1], 256, 24, (-2, -2, 256 + 4, 24 + 4), 22),
    # ... and its negative: s = -Q1 fails the bounds test although it rounds to 0; s = 1 - Q1 rounds to the tie 0.5
    "affine_q1_neg": lambda: _geo(0, [1, 0, 0, 1, -Q1, -Q1], 256, 24, (-2, -2, 256 + 4, 24 + 4), 23),
    # just below every integer (one unit in the last place below 256): at x = W = 256, s = W - 2^-45 is inside and s + 0.5 is a rounding tie
    # (the 2^-80 makes the offsets f64-only: KIND 2)
    "affine_below": lambda: _geo(0, [1, 0, 0, 1, -(2.0 ** -45 + 2.0 ** -80), -(2.0 ** -48 + 2.0 ** -80)], 256, 32, (-2, -2, 256 + 4, 32 + 4), 24),
    # projective in the plain division range (denominator 1): Q1 offsets
    "proj_q1": lambda: _geo(1, [1, 0, Q1, 0, 1, Q1, 0, 0], 256, 24, (-2, -2, 256 + 4, 24 + 4), 25),
    # projective with an entry below 2^-100 (IEEE divisions): the denominator still rounds to 1, half scale
    "proj_ieee": lambda: _geo(1, [0.5, 0, 0, 0, 0.5, 0, 2.0 ** -110, 0], 256, 24, (-3, -3, 2 * 256 + 6, 2 * 24 + 6), 26),
}
GEOMETRIC_KIND = {"affine_half": 0, "affine_q1": 2, "affine_q1_neg": 2, "affine_below": 2, "proj_q1": 3, "proj_ieee": 1}


# ------------------------------------------------------------------------------------------------ the nearest rule, written again

def nearest(img, sx, sy, covered, msx=0, msy=0):
    """The per-pixel rule of :1001 / :1047 without the oracle: bounds on the unrounded coordinate, Math.round, flat index
    round(sy) * W + round(sx) into the source, anything outside the array reads 0."""
    img = np.asarray(img, np.uint8)
    H, W = img.shape[:2]
    with np.errstate(invalid="ignore"):
        inb = covered & (sx >= msx) & (sx < W + msx) & (sy >= msy) & (sy < H + msy)
    out = np.zeros(sx.shape + (4,), np.uint8)
    idx = js_round(sy[inb]).astype(np.int64) * W + js_round(sx[inb]).astype(np.int64)
    ok = (idx >= 0) & (idx < W * H)
    vals = np.zeros((idx.size, 4), np.uint8)
    flat = img.reshape(-1, 4)
    vals[ok] = flat[idx[ok]]
    out[inb] = vals
    return out


def piecewise_taps(case):
    """(rgba, map, inv, sx, sy, covered) of a piecewise case through the oracle."""
    sp, tris, msx, msy, dp, geom, img = case
    out, wmap, _, inv = O.warp_inverse_piecewise(sp, dp, tris, img, msx, msy, *geom, taps=True)
    sx, sy, valid = B.piecewise_coords(wmap, inv, *geom)
    return out, wmap, inv, sx, sy, valid


def geometric_coords(case):
    kind, m, img, geom = case
    sx, sy = B.geometric_coords(kind, m, *geom)
    return sx, sy, np.ones(sx.shape, bool)


# ------------------------------------------------------------------------------------------------ classifier

def classify(sx, sy, covered, W, H, msx=0, msy=0, wmap=None):
    """Counts of the covered pixels in each edge class (see the module docstring).  wmap (piecewise): the Int16 map, for E5."""
    with np.errstate(invalid="ignore"):
        fin = covered & np.isfinite(sx) & np.isfinite(sy)
        inx = (sx >= msx) & (sx < W + msx)
        iny = (sy >= msy) & (sy < H + msy)
        inb = fin & inx & iny
        rx = np.where(inb, js_round(np.where(inb, sx, 0)), 0).astype(np.int64)
        ry = np.where(inb, js_round(np.where(inb, sy, 0)), 0).astype(np.int64)
        idx = ry * W + rx
        tie_x, tie_y = (sx - np.floor(sx)) == 0.5, (sy - np.floor(sy)) == 0.5
        c = {}
        n = lambda a: int(np.count_nonzero(a))
        c["E1 tie x>=0"] = n(inb & tie_x & (sx >= 0)); c["E1 tie x<0"] = n(inb & tie_x & (sx < 0))
        c["E1 tie y>=0"] = n(inb & tie_y & (sy >= 0)); c["E1 tie y<0"] = n(inb & tie_y & (sy < 0))
        c["E1 -0.5"] = n(inb & ((sx == -0.5) | (sy == -0.5)))
        c["E2 low in"] = n(inb & ((sx == msx) | (sy == msy)))
        c["E2 low out"] = n(fin & (((sx >= msx - 0.5) & (sx < msx) & iny) | ((sy >= msy - 0.5) & (sy < msy) & inx)))
        hix = inb & (sx >= W + msx - 0.5)
        # round(sx) = W + minSrcX: index (ry + 1) W + minSrcX, pixel minSrcX of the next row -- of the same row, column W + minSrcX, when minSrcX < 0
        c["E3 high in, next row"] = n(hix & (idx < W * H) & (idx >= 0)) if msx >= 0 else 0
        c["E3 high in, same row"] = n(hix & (idx < W * H) & (idx >= 0)) if msx < 0 else 0
        c["E3 high in, past the end"] = n(hix & (idx >= W * H))
        c["E3 high in y"] = n(inb & (sy >= H + msy - 0.5))
        c["E3 high out"] = n(fin & (((sx == W + msx) & iny) | ((sy == H + msy) & inx)))
        c["E4 rx<0, index>=0"] = n(inb & (rx < 0) & (idx >= 0))
        c["E4 index<0"] = n(inb & (idx < 0))
        c["E4 ry<0, index>=0"] = n(inb & (ry < 0) & (idx >= 0))
        c["E6 Q1"] = n(fin & ((np.abs(sx) == Q1) | (np.abs(sy) == Q1)))
        c["E6 -Q1"] = n(fin & ((sx == -Q1) | (sy == -Q1)))
    if wmap is not None:
        c.update(span_ends(sx, sy, wmap, W, msx))
    return c


def span_ends(sx, sy, wmap, W, msx):
    """E5: spans (runs of one id along a row) whose first / last pixel is on the x limit (in) or one pixel past it (out, while the
    pixel next to it is in)."""
    ids = np.asarray(wmap).reshape(sx.shape).astype(np.int64)
    lo, hi = float(msx), float(W + msx)
    at = {"E5 first on limit": 0, "E5 first past limit": 0, "E5 last on limit": 0, "E5 last past limit": 0}
    for r in range(ids.shape[0]):
        row = ids[r]
        cut = np.flatnonzero(np.diff(row)) + 1
        starts, ends = np.r_[0, cut], np.r_[cut, row.size]
        for a, b in zip(starts, ends):
            if row[a] < 0 or b - a < 2:
                continue
            f0, f1, l0, l1 = sx[r, a], sx[r, a + 1], sx[r, b - 1], sx[r, b - 2]
            at["E5 first on limit"] += int(f0 == lo)
            at["E5 first past limit"] += int(f0 < lo <= f1)
            at["E5 last on limit"] += int(hi - 0.5 <= l0 < hi)
            at["E5 last past limit"] += int(l0 >= hi > l1)
    return at
