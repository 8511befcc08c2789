"""Folded and degenerate meshes for the inverse piecewise warps, and a classifier of the pixels where their triangles overlap.  CPU only.

The reference rasterises the triangle map in list order (fillTriangle, :852-858), so where destination triangles overlap the LARGEST covering
id wins, and the pixel loop :1042-1056 reads that winner alone: a winner whose coordinate fails the bounds test :1047 or is NaN leaves the
pixel 0, whatever lies under it.  The meshes here are unions of edges.tie_mesh blocks: every inverse is exactly [0.5, 0, 0, 0.5, c, d] and
the blocks' source offsets differ by tens of pixels, so a kernel that resolves an overlap to another triangle reads another source pixel.

A builder returns (sp, tris, minSrcX, minSrcY, dst_pts, geom, image) like edges.piecewise.  All cases use a 255 x 19 source."""
import functools

import numpy as np

from . import bilinear as B
from . import edges as E
from . import field as FM
from . import oracle as O
from . import workloads as WL

W, H = 255, 19
A = (-0.5, -0.5, 16, 5, 16, 4, (2, 2))                       # edges.PIECEWISE["pos"]: 160 triangles, window 512 x 40
BLK = (159.5, 3.5, 8, 3, 16, 4, (130, 10))                   # 48 triangles inside A's window, from source columns 160 .. 287
A_NEG = (-3.5, -2.5, 16, 5, 16, 4, (2, 2))
BLK_NEG = (156.5, 1.5, 8, 3, 16, 4, (130, 10))
A_POINTS = 17 * 6
A_VERTEX = 2 * 17 + 3                                        # an interior vertex of A (row 2, column 3): moving it keeps the window

# a block whose every span has both ends inside the source (k_pw_rows' "safe" spans), and a block that leaves the source inside its first window
INNER = (0.0, 0.0, 15, 4, 16, 4, (2, 2))
BLK_LEFT = (159.5, 3.5, 8, 3, 16, 4, (10, 6))
NAN_DST = [100, 6, 300, 10, 180, 38]
SLIVER_SRC = [40, 4, 80, 8, 60, 16]


def _add(mesh, src3, dst3, first=False):
    """The mesh with one triangle on three points of its own, listed last (id T) or first (id 0, every other id moves up)."""
    sp, tris, dp = mesh
    s3, d3 = np.float32(src3), np.float32(dst3)
    if first:
        return np.concatenate([s3, sp]), np.concatenate([np.uint32([0, 1, 2]), tris + np.uint32(3)]), np.concatenate([d3, dp])
    n = sp.size // 2
    return np.concatenate([sp, s3]), np.concatenate([tris, np.uint32([n, n + 1, n + 2])]), np.concatenate([dp, d3])


def deep_blocks(K):
    """K blocks of 2 x 5 cells, 96 x 4 source pixels each, stacked on one another with source offsets 16 (k mod 4): depth K."""
    return [(-0.5 + 16.0 * (k % 4), -0.5, 2, 5, 96, 4, (2 + 2 * k, 2)) for k in range(K)]


# name -> (mesh builder, index of A's first point or None, image seed)
_MESHES = {
    "fold_over": (lambda: E.tie_mesh([A, BLK]), 0, 11),
    "fold_under": (lambda: E.tie_mesh([BLK, A]), 9 * 4, 11),
    "fold_over_neg": (lambda: E.tie_mesh([A_NEG, BLK_NEG]), 0, 13),
    "fold_over_rev": (lambda: _reversed(E.tie_mesh([A, BLK])), 0, 11),
    "nan_last": (lambda: _add(E.tie_mesh([A]), [40, 8] * 3, NAN_DST), None, 11),
    "nan_first": (lambda: _add(E.tie_mesh([A]), [40, 8] * 3, NAN_DST, first=True), None, 11),
    "nan_collinear": (lambda: _add(E.tie_mesh([A]), [40, 8, 80, 8, 120, 8], NAN_DST), None, 11),
    "sliver_last": (lambda: _add(E.tie_mesh([A]), SLIVER_SRC, [100.25, 4, 101.5, 4, 300.75, 40]), None, 11),
    "none_collinear": (lambda: _add(E.tie_mesh([A]), SLIVER_SRC, [10, 5, 200, 24, 390, 43]), None, 11),
    "none_coincident": (lambda: _add(E.tie_mesh([A]), SLIVER_SRC, [100, 20] * 3), None, 11),
    # not in A's window: the first 256-pixel window of every row is covered by safe spans of INNER alone, under an out-of-bounds / NaN winner
    "inner_over": (lambda: E.tie_mesh([INNER, BLK_LEFT]), None, 11),
    "inner_nan": (lambda: _add(E.tie_mesh([INNER]), [40, 8] * 3, [20, 6, 230, 10, 120, 30]), None, 11),
}
FOLDS = ["fold_over", "fold_under", "fold_over_neg", "fold_over_rev"]
NANS = ["nan_last", "nan_first", "nan_collinear", "inner_nan"]
DEEP = {"deep12": 12, "deep20": 20, "deep40": 40, "deep70": 70}
# ... and the same stacks with one cell far to the right of them (two triangles more in rows 0 .. 7): windows of 530 columns, because
# k_pw_tile takes windows of 512 columns or more
DEEP_WIDE = {"deep12_wide": 12, "deep20_wide": 20, "deep40_wide": 40}
WIDENER = (15.5, -0.5, 1, 1, 16, 4, (500, 2))
SINGLE = list(_MESHES)                                       # every case of one frame but the deep stacks


def _reversed(mesh):
    sp, tris, dp = mesh
    return sp, tris.reshape(-1, 3)[::-1].ravel().copy(), dp


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def case(name, twin=False):
    """(sp, tris, minSrcX, minSrcY, dst_pts, geom, image), built once and read-only.  twin (fold_* only): A's interior vertex moved by two
    f32 units in the last place, which takes the frame out of the one-fma form."""
    if name in DEEP or name in DEEP_WIDE:
        assert not twin
        blocks = deep_blocks(DEEP[name]) if name in DEEP else deep_blocks(DEEP_WIDE[name]) + [WIDENER]
        mesh, a0, seed = E.tie_mesh(blocks), None, 11
    else:
        build, a0, seed = _MESHES[name]
        mesh = build()
    sp, tris, dp = mesh
    geom = WL.piecewise_geom(dp)
    if twin:
        assert a0 is not None, name
        dp = E.nudge(dp, a0 + A_VERTEX, 2)
        assert WL.piecewise_geom(dp) == geom
    msx, msy = WL.src_min(sp)
    return _frozen(sp, tris, msx, msy, dp, geom, O.lcg_image(W, H, seed))


def all_cases(deep=True):
    """(name, twin) of every case: the fold_* cases with their twins."""
    out = [(n, t) for n in SINGLE for t in ((False, True) if n in FOLDS else (False,))]
    return out + ([(n, False) for n in list(DEEP) + list(DEEP_WIDE)] if deep else [])


@functools.lru_cache(maxsize=None)
def taps(name, twin=False):
    """(rgba, map, fwd, inv, sx, sy, valid) of a case on the oracle, computed once and read-only."""
    sp, tris, msx, msy, dp, geom, img = case(name, twin)
    out, wmap, fwd, inv = O.warp_inverse_piecewise(sp, dp, tris, img, msx, msy, *geom, taps=True)
    sx, sy, valid = B.piecewise_coords(wmap, inv, *geom)
    return _frozen(out, wmap, fwd, inv, sx, sy, valid)


# ------------------------------------------------------------------------------------------------ the cover classifier

def covers(dp, tris, geom):
    """(T, h, w) bool: the cells every triangle fills when it is rasterised ALONE through the oracle's fillTriangle."""
    x0, y0, w, h = geom
    tris = np.asarray(tris, np.uint32)
    T = tris.size // 3
    cov = np.zeros((T, h, w), bool)
    for t in range(T):
        cov[t] = O.build_tri_map(dp, tris[3 * t:3 * t + 3], w, y0, w * h).reshape(h, w) >= 0
    return cov


def stack(cov):
    """(top, second, depth): the largest and the second largest covering id per cell (-1: none), and how many cover it."""
    top = np.full(cov.shape[1:], -1, np.int64)
    second = top.copy()
    for t in range(cov.shape[0]):
        second = np.where(cov[t], top, second)
        top = np.where(cov[t], t, top)
    return top, second, cov.sum(0)


def classify(c, inv):
    """Counts over the output window of a case, from the per-triangle covers and the oracle's inverse matrices `inv`:
         overlap         pixels covered by two or more triangles
         discriminating  overlap pixels where the winner and the next lower covering triangle read different flat source indices, or
                         exactly one of the two is a hole (fails :1047, NaN, or an index outside the array)
         holes           finite winners that fail the bounds test over a lower covering triangle that passes it
         nan_holes       NaN winners over such a triangle
         depth           the largest number of triangles on one pixel
         pieces          the largest number of triangles with a span in one output row
    and the model map `top` (largest covering id, -1 where none)."""
    sp, tris, msx, msy, dp, geom, img = c
    cov = covers(dp, tris, geom)
    top, second, depth = stack(cov)
    sx, sy, valid = B.piecewise_coords(top, inv, *geom)
    sx2, sy2, valid2 = B.piecewise_coords(second, inv, *geom)
    idx = FM.index_field(sx, sy, valid, W, H, msx, msy)
    idx2 = FM.index_field(sx2, sy2, valid2, W, H, msx, msy)
    over = depth >= 2
    live_top = FM.covered(sx, sy, valid, W, H, msx, msy)
    live_lower = np.zeros(top.shape, bool)
    x = np.arange(geom[2], dtype=np.float64)[None, :] + geom[0]
    y = np.arange(geom[3], dtype=np.float64)[:, None] + geom[1]
    for t in range(cov.shape[0]):
        m = np.asarray(inv[t], np.float64)
        with np.errstate(all="ignore"):
            tx, ty = (m[0] * x + m[2] * y) + m[4], (m[1] * x + m[3] * y) + m[5]
            ok = (tx >= msx) & (tx < W + msx) & (ty >= msy) & (ty < H + msy)
        live_lower |= cov[t] & ok & (t < top)
    nan_top = valid & ~(np.isfinite(sx) & np.isfinite(sy))
    n = lambda a: int(np.count_nonzero(a))
    return {"overlap": n(over), "discriminating": n(over & (idx != idx2)), "holes": n(valid & ~nan_top & ~live_top & live_lower),
            "nan_holes": n(nan_top & live_lower), "depth": int(depth.max()), "pieces": int(cov.any(2).sum(0).max()), "top": top}


# ------------------------------------------------------------------------------------------------ frame sets

F = 8
NO_OVERLAP, NO_SPANS = 3, 6


@functools.lru_cache(maxsize=None)
def moving_fold():
    """Mesh [A, BLK] in eight frames: BLK's destination moves over A by the frame, so the overlap region moves; frame 3 puts it below A
    (no overlap), frame 6 puts all its vertices on x = 200 (no spans, non-finite inverses); odd frames are the two-rounding twin.
    Returns (sp, tris, minSrcX, minSrcY, [dst_pts per frame], [geom per frame])."""
    sp, tris, dp = E.tie_mesh([A, BLK])
    base = dp.reshape(-1, 2).astype(np.float64)
    frames = []
    for f in range(F):
        d = base.copy()
        d[A_POINTS:] += [12 * f - 30, 2 * (f % 4) - 4] if f != NO_OVERLAP else [0, 34]
        if f == NO_SPANS:
            d[A_POINTS:, 0] = 200.0
        d = d.astype(np.float32).ravel()
        frames.append(E.nudge(d, A_VERTEX, 2) if f % 2 else d)
    msx, msy = WL.src_min(sp)
    return _frozen(sp, tris, msx, msy) + (tuple(_frozen(*frames)), tuple(WL.piecewise_geom(d) for d in frames))


NAN_FRAMES, TWIN_FRAMES = (1, 5), (3, 7)
HALF_SRC = [40, 2, 140, 4, 80, 18]                           # (NAN_DST - (100, 6)) / 2 + (40, 2): inside the source


@functools.lru_cache(maxsize=None)
def moving_nan():
    """Mesh A plus one triangle listed last, eight frames with their own source points.  The triangle's source is HALF_SRC, half its
    destination of frame 0 (an exact half-scale inverse in every frame: its destination moves right by 8 pixels a frame), but coincident
    in frames 1 and 5: NaN matrices in those frames only.  Frames 3 and 7 are the two-rounding twin with finite matrices (A's interior
    vertex moved), so the one-fma frames are 0, 2, 4 and 6 and the coordinate form differs from frame to frame within the set.
    Returns (tris, [src_pts per frame], [dst_pts per frame], [geom per frame], [minSrc per frame])."""
    srcs, dsts = [], []
    for f in range(F):
        src3 = [40, 8] * 3 if f in NAN_FRAMES else HALF_SRC
        dst3 = (np.float64(NAN_DST).reshape(3, 2) + [8 * f, 0]).ravel()
        sp, tris, dp = _add(E.tie_mesh([A]), src3, dst3)
        if f in TWIN_FRAMES:
            dp = E.nudge(dp, A_VERTEX, 2)
        srcs.append(sp); dsts.append(dp)
    _frozen(tris, *srcs, *dsts)
    return tris, tuple(srcs), tuple(dsts), tuple(WL.piecewise_geom(d) for d in dsts), tuple(WL.src_min(s) for s in srcs)
