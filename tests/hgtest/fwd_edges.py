"""Edge-case inputs for the FORWARD warps (scatter semantics: the last writer in raster order wins), built from the constants of the
tile kernels' candidate bounds and of their host admission (fwd_tile_param), and a classifier of the writers they produce.  CPU only.

Geometric cases are dicts {name, kind, m, W, H, seed, geom, admit}: admit is the code hg_forward_tiles_admissible must give (0 = scatter +
gather, 1 = k_fwd_tiles without a trusted inverse, 2 = with one).  Piecewise cases are dicts {name, sp, tris, dp, W, H, seed, geom, msx, msy,
Mx, My, ...}: the source-point bounding box (msx, msy) .. (Mx, My) is part of the case because some cases pass a box that is not the mesh's.

The classifier restates the reference loops (_geometricWarp :911-932, _piecewiseAffineWarp :948-972) in numpy f64, in the reference's
operation order, and resolves the last writer itself; tests/test_forward_edges_cpu.py checks it against the oracle's bytes before either
judges a kernel.  Its counts (per case):
  tie_x, tie_y     landing writers whose destination coordinate minus the offset has fraction exactly 0.5
  border_tie       {left, right, top, bottom}: such ties that land on the first / last column / row of a 64 x 64 output tile
  alias_left[d]    landing writers with u = -d (they land one row up, column objW - d), d = 1..32; alias_last_row: those from v = objH
  alias_right[d]   landing writers with u = objW - 1 + d (one row down, column d - 1); alias_row0: those from v = -1
  shift[k]         landing writers with k objW <= u < (k + 1) objW, k = -3..3
  writers_max      most writers on one output pixel; overwritten: pixels with two or more
  lost_to_zero     pixels whose LAST writer reads outside the source array (a 0 stored over earlier writers); zero_over_earlier: those with
                   an earlier writer that read a pixel; src_wrapped: pixels whose last writer has a valid flat source index with x outside
                   0..W-1 (it reads the neighbouring source row)
  pass_rows        winners whose source row is the last of a 256-row pass counted from row 0, or the first of the next"""
import numpy as np

from . import oracle as O
from . import workloads as WL
from .edges import js_round

WRAP, TILE, PASS = 32, 64, 256             # kFwdWrap, kFwdTileW == kFwdTileH, source rows per pass of k_fwd_tiles
ALIAS = WRAP - 2                           # fwd_tile_param: no corner image further than this outside the window
DEN_MIN, PERSP_MAX = 1.0e-2, 0.1           # fwd_tile_param: denominator at the source corners, |m6| and |m7|
ENTRY_MAX = {0: 1.0e6, 1: 1.0e4}           # ... |m0..m5| (affine, projective)
IMAGE_MAX = {0: 1.0e7, 1: 1.0e5}           # ... |corner image|, exclusive
SRC_MAX, WIN_MIN = 65535, 2 * WRAP         # ... source width and height; window width
SLOPE_SWITCH, DET_MIN, ROUND_TRIP = 1.0e-9, 1.0e-12, 1.0e-3
PW_ENTRY_MAX, PW_SHIFT_MAX = 1.0e6, 2      # k_fwd_pw_bins
PW_CAP0, PW_CAP_MAX = 64, 256              # entries per tile: first and largest capacity
PW_RECORDS, PW_SEGMENTS, PW_SEG_W = 512, 1024, 16
UP = 1.0 + 2.0 ** -20                      # "just past a limit": a factor far above rounding error, far below anything else


# ------------------------------------------------------------------------------------------------ the reference loops, written again

def apply_affine(m, x, y):
    return (m[0] * x) + (m[2] * y) + m[4], (m[1] * x) + (m[3] * y) + m[5]                       # :1383-1384


def apply_projective(m, x, y):
    den = m[6] * x + m[7] * y + 1
    return (m[0] * x + m[1] * y + m[2]) / den, (m[3] * x + m[4] * y + m[5]) / den               # :1402-1403


def _shl2(u):
    """`u << 2` of JS on f64 values: ToInt32 (non-finite -> 0), shift, back to int32."""
    fin = np.isfinite(u)
    t = np.where(fin, np.trunc(np.where(fin, u, 0.0)), 0.0)
    w = np.mod(t, 4294967296.0).astype(np.uint64)
    w = (w << np.uint64(2)) & np.uint64(0xFFFFFFFF)
    return w.astype(np.uint32).view(np.int32).astype(np.float64)


def _resolve(nx, ny, rank, geom, src_row, src_ok=None, src_wrapped=None):
    """Counts and winners of the writers (nx, ny) in raster order `rank` (1-D arrays), window geom."""
    xo, yo, ow, oh = geom
    n_px = max(ow, 0) * max(oh, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        uh, vh = nx - xo, ny - yo                                                             # :924 / :962
        u, v = js_round(uh), js_round(vh)
        idx = (v * float(ow << 2)) + _shl2(u)                                                 # :926 / :964
        lands = (idx >= 0) & (idx + 3 < n_px * 4)
    p = (idx[lands] / 4).astype(np.int64)
    ul, vl, rk = u[lands], v[lands], rank[lands]
    col, row = p % max(ow, 1), p // max(ow, 1)
    tx = (uh[lands] - np.floor(uh[lands])) == 0.5
    ty = (vh[lands] - np.floor(vh[lands])) == 0.5
    n = lambda a: int(np.count_nonzero(a))
    first_c, last_c = (col % TILE) == 0, ((col % TILE) == TILE - 1) | (col == ow - 1)
    first_r, last_r = (row % TILE) == 0, ((row % TILE) == TILE - 1) | (row == oh - 1)
    c = {"tie_x": n(tx), "tie_y": n(ty),
         "border_tie": {"left": n(tx & first_c), "right": n(tx & last_c), "top": n(ty & first_r), "bottom": n(ty & last_r)}}
    c["alias_left"] = [0] + [n(ul == -d) for d in range(1, WRAP + 1)]
    c["alias_right"] = [0] + [n(ul == ow - 1 + d) for d in range(1, WRAP + 1)]
    c["alias_last_row"] = n((ul < 0) & (ul >= -WRAP) & (vl == oh))
    c["alias_row0"] = n((ul >= ow) & (ul < ow + WRAP) & (vl == -1))
    k = np.floor(ul / max(ow, 1))
    c["shift"] = {s: n(k == s) for s in range(-3, 4)}
    c["shift_beyond"] = n(np.abs(k) > 3)
    writers = np.bincount(p, minlength=n_px) if n_px else np.zeros(0, np.int64)
    c["writers_max"] = int(writers.max()) if n_px else 0
    c["overwritten"] = n(writers >= 2)
    win = np.full(n_px, -1, np.int64)
    np.maximum.at(win, p, rk)
    has = win >= 0
    c["written"] = n(has)
    wr = src_row[np.where(has, win, 0)]
    c["pass_rows"] = n(has & (((wr % PASS) == PASS - 1) | (((wr % PASS) == 0) & (wr > 0))))
    if src_ok is not None:
        lost = has & ~src_ok[np.where(has, win, 0)]
        good = np.bincount(p, weights=src_ok[rk].astype(np.float64), minlength=n_px) > 0
        c["lost_to_zero"] = n(lost)
        c["zero_over_earlier"] = n(lost & good)
        c["src_wrapped"] = n(has & src_wrapped[np.where(has, win, 0)])
    return c, win


def geometric_writers(case):
    kind, m, W, H = case["kind"], case["m"], case["W"], case["H"]
    ys, xs = np.mgrid[0:H, 0:W]
    x, y = xs.ravel().astype(np.float64), ys.ravel().astype(np.float64)
    with np.errstate(all="ignore"):
        nx, ny = apply_affine(m, x, y) if kind == 0 else apply_projective(m, x, y)
    return nx, ny, ys.ravel()


def classify_geometric(case):
    """(counts, winners): winners[p] = raster rank y * W + x of the last writer of output pixel p, -1 where nobody writes."""
    nx, ny, rows = geometric_writers(case)
    return _resolve(nx, ny, np.arange(nx.size), case["geom"], rows)


def expected_geometric(case, img, win=None):
    """The output the winners give: the classifier's own statement of the reference result."""
    if win is None:
        win = classify_geometric(case)[1]
    flat = np.asarray(img, np.uint8).reshape(-1, 4)
    out = np.zeros((win.size, 4), np.uint8)
    out[win >= 0] = flat[win[win >= 0]]
    return out.reshape(case["geom"][3], case["geom"][2], 4)


def piecewise_maps(case):
    """(forward map as Int16 (map_h, map_w), f32 forward matrices) of a piecewise case, from the oracle's rasteriser and solver."""
    mw, mh = case["Mx"] - case["msx"], case["My"] - case["msy"]
    fmap = O.build_tri_map(case["sp"], case["tris"], mw, case["msy"], mw * mh)
    return fmap.reshape(mh, mw), O.piecewise_matrices(case["sp"], case["dp"], case["tris"])


def piecewise_oracle(case, img):
    fmap, fwd = piecewise_maps(case)
    return O.warp_forward_piecewise(fmap.ravel(), fwd, img, case["msx"], case["msy"], case["Mx"], case["My"], *case["geom"])


def classify_piecewise(case, maps=None):
    """(counts, winners, flat source index per map cell): winners[p] = map cell of the last writer of output pixel p, -1 where none."""
    fmap, fwd = piecewise_maps(case) if maps is None else maps
    mh, mw = fmap.shape
    W, H = case["W"], case["H"]
    t16 = fmap.ravel().astype(np.int64)
    used = t16 > -1                                                                            # :957
    cells = np.flatnonzero(used)
    my, mx = cells // mw, cells % mw
    x, y = (mx + case["msx"]).astype(np.float64), (my + case["msy"]).astype(np.float64)
    m = fwd[t16[cells]].astype(np.float64).T
    with np.errstate(all="ignore"):
        nx, ny = apply_affine(m, x, y)                                                         # :961 (the f32 matrix the Int16 value selects)
    sidx = np.full(mh * mw, -1, np.int64)
    sidx[cells] = (my + case["msy"]) * W + (mx + case["msx"])                                   # :960
    src_ok = (sidx >= 0) & (sidx < W * H)
    xs = np.zeros(mh * mw, np.int64)
    xs[cells] = mx + case["msx"]
    wrapped = src_ok & ((xs < 0) | (xs >= W))
    rows = np.arange(mh * mw) // mw
    c, win = _resolve(nx, ny, cells, case["geom"], rows, src_ok, wrapped)
    c["ids"] = (int(t16[cells].min()), int(t16[cells].max())) if cells.size else (0, 0)
    return c, win, sidx


def expected_piecewise(case, img, win=None, sidx=None):
    if win is None:
        _, win, sidx = classify_piecewise(case)
    flat = np.asarray(img, np.uint8).reshape(-1, 4)
    out = np.zeros((win.size, 4), np.uint8)
    s = sidx[np.where(win >= 0, win, 0)]
    ok = (win >= 0) & (s >= 0) & (s < flat.shape[0])
    out[ok] = flat[s[ok]]
    return out.reshape(case["geom"][3], case["geom"][2], 4)


def rank_image(W, H):
    """An image whose pixel i (raster order) holds i + 1 as a little-endian uint32: a warp of it names every winner."""
    return (np.arange(W * H, dtype=np.uint32) + 1).view(np.uint8).reshape(H, W, 4).copy()


def image(case):
    return O.lcg_image(case["W"], case["H"], case["seed"])


# ------------------------------------------------------------------------------------------------ geometric builders

def _g(name, kind, m, W, H, geom, admit, seed=61):
    return {"name": name, "kind": kind, "m": np.asarray(m, np.float64), "W": int(W), "H": int(H), "seed": seed,
            "geom": tuple(int(v) for v in geom), "admit": admit}


def _hull(kind, m, W, H):
    """Rounded bounds of the images of the four source corners (x0, y0, x1, y1): what the windows below are cut from."""
    x, y = np.float64([0, W - 1, 0, W - 1]), np.float64([0, 0, H - 1, H - 1])
    fx, fy = apply_affine(m, x, y) if kind == 0 else apply_projective(m, x, y)
    return int(js_round(fx.min())), int(js_round(fy.min())), int(js_round(fx.max())), int(js_round(fy.max()))


def _fit(kind, m, W, H, grow=(0, 0, 0, 0)):
    """The window that holds every rounded corner image, grown by (left, top, right, bottom) pixels (negative: shrunk)."""
    x0, y0, x1, y1 = _hull(kind, m, W, H)
    return (x0 - grow[0], y0 - grow[1], x1 - x0 + 1 + grow[0] + grow[2], y1 - y0 + 1 + grow[1] + grow[3])


def _fit0(kind, m, W, H):
    """A window at offset (0, 0) that holds every rounded corner image and one pixel more."""
    x0, y0, x1, y1 = _hull(kind, m, W, H)
    assert x0 >= 0 and y0 >= 0
    return (0, 0, x1 + 2, y1 + 2)


def tile_border_ties():
    """G1: scale 1 and 1.5 with half-integer translations: every destination x (and y) of scale 1, every other one of scale 1.5, is a
    Math.round tie, and the windows put them on the first and last column and row of full and ragged tiles."""
    out = []
    for wn in (63, 64, 65, 96, 127, 128, 129, 193):
        for t, tag in (((0.5, 0.5), "pos"), ((-20.5, -10.5), "neg")):
            xo, yo = int(np.floor(t[0])) + 1, int(np.floor(t[1])) + 1          # u = x, v = y: the window is the source
            out.append(_g(f"ties_s1_{tag}_w{wn}", 0, [1, 0, 0, 1, t[0], t[1]], wn, 130, (xo, yo, wn, 130), 2 if wn >= WIN_MIN else 0, 62))
        ws = int(np.ceil(wn / 1.5)) + 1                                        # u = round(1.5 x - 0.5) covers 0 .. wn - 1 and a little more
        out.append(_g(f"ties_s15_w{wn}", 0, [1.5, 0, 0, 1.5, 0.5, -2.5], ws, 90, (1, -2, wn, 134), 2 if wn >= WIN_MIN else 0, 63))
    return out


def alias_limit():
    """G2: identity maps whose window is shifted and narrowed so that a corner image lies exactly kFwdWrap - 2 = 30 columns outside on the
    left, on the right and on both, and is one row shorter than the image above and below (writers from v = -1 and v = objH exist);
    the twins at 30.5 and 31 columns are refused."""
    W, H = 200, 40
    out = []
    for kind, ident in ((0, [1, 0, 0, 1, 0, 0]), (1, [1, 0, 0, 0, 1, 0, 0, 0])):
        k = "aff" if kind == 0 else "proj"
        out.append(_g(f"alias_left_{k}", kind, ident, W, H, (ALIAS, 1, W - ALIAS, H - 2), 2, 64))
        out.append(_g(f"alias_right_{k}", kind, ident, W, H, (0, 1, W - ALIAS - 1, H - 2), 2, 64))
        out.append(_g(f"alias_both_{k}", kind, ident, W, H, (ALIAS, 1, W - 2 * ALIAS - 1, H - 2), 2, 64))
        out.append(_g(f"alias_left_31_{k}", kind, ident, W, H, (ALIAS + 1, 1, W - ALIAS - 1, H - 2), 0, 64))
        out.append(_g(f"alias_right_31_{k}", kind, ident, W, H, (0, 1, W - ALIAS - 2, H - 2), 0, 64))
    half = [1, 0, 0, 1, -0.5, 0]                                               # x' = x - 0.5: the left corner image is 30.5 columns outside
    out.append(_g("alias_left_30.5_aff", 0, half, W, H, (ALIAS, 1, W - ALIAS, H - 2), 0, 64))
    out.append(_g("alias_right_30.5_aff", 0, [1, 0, 0, 1, 0.5, 0], W, H, (0, 1, W - ALIAS - 1, H - 2), 0, 64))
    out.append(_g("alias_both_w64", 0, [1, 0, 0, 1, 0, 0], WIN_MIN + 2 * ALIAS + 1, H, (ALIAS, 1, WIN_MIN, H - 2), 2, 65))
    return out


SLOPES = [0.0] + [s * v for v in (1e-10, 0.99 * SLOPE_SWITCH, 1.01 * SLOPE_SWITCH, 1e-8, 1e-6) for s in (1, -1)]


def slopes():
    """G3: the x slope (a[0], a[1] of k_fwd_tiles: m0, or m0 - L m6 for the tile edge L) and the y slope (m1, or m3 - L m6) on both sides of
    the 1e-9 switch, the other axis regular; both slopes 0; matrices of rank 1 and rank 0."""
    out = []
    W, H = 100, 150
    for s in SLOPES:
        mx = [s, 1, 1, 0, 0.5, 0.5]                                            # x' = s x + y + 0.5, y' = x + 0.5: ties, x slope s
        out.append(_g(f"slope_x_aff_{s:g}", 0, mx, W, H, _fit(0, mx, W, H, (1, 1, 1, 1)), 2, 66))
        my = [1, s, 0, 1, 0.5, 0.5]                                            # x' = x + 0.5, y' = s x + y + 0.5: y slope s
        out.append(_g(f"slope_y_aff_{s:g}", 0, my, W, H, _fit(0, my, W, H, (1, 1, 1, 1)), 2, 66))
        # projective: num_x - L den = s x + y + (m2 - L) for the left edge L of the tile at column 64 of a window at offset 0
        m6 = 2.0 ** -10
        L = TILE - 0.5 - 1.0 / 64
        px = [L * m6 + s, 1, 0.5, 1, 0, 0.5, m6, 0]
        out.append(_g(f"slope_x_proj_{s:g}", 1, px, W, H, _fit0(1, px, W, H), 2, 67))
        py = [1, 0, 0.5, L * m6 + s, 1, 0.5, m6, 0]                            # the same for the top edge L of the tile row at 64
        out.append(_g(f"slope_y_proj_{s:g}", 1, py, W, H, _fit0(1, py, W, H), 2, 67))
    # A slope just past the switch that the reference's own sums absorb: x' = (m0 x + L m7 y + L) / (m7 y + 1) with L = 9999.5 and
    # m7 = 1/16.  From row 2^25 / (L m7) = 53688 on, |m0 x| < ulp(L m7 y) / 2 for x <= 3, so the numerator rounds to L (m7 y + 1) and
    # x' is the tie L for EVERY x of the row, while the kernel's constraint (m0 - L m6) x + ... >= 0 still has the slope m0 < 0 in it:
    # only the 1/64-pixel widening keeps x = 1 .. 3 among the candidates of the tile whose first column that tie rounds to.
    Lt = 9999.5
    # (y' = (4000 x + 10 y) / (m7 y + 1) puts x = 0 .. 3 of those rows about one pixel apart; the window holds only those output rows)
    ab = [-1.01 * SLOPE_SWITCH, Lt / 16, Lt, 4000, 10, 0, 0, 1 / 16]
    out.append(_g("slope_absorbed", 1, ab, 4, SRC_MAX, (int(Lt) - TILE + 1, 150, 2 * TILE, 30), 1, 67))
    out.append(_g("slope_both_0", 0, [0, 0, 1, 0.25, 0.5, 0], W, H, (0, 0, H + 1, H // 4 + 2), 1, 68))     # row y lands on (y + 1, round(y / 4))
    out.append(_g("rank1", 0, [1, 0.5, 2, 1, 0, 0], 60, 40, (0, 0, 60 + 80, 72), 1, 68))                   # y' = x' / 2
    out.append(_g("rank0", 0, [0, 0, 0, 0, 40.5, 3.5], 60, 40, (10, 2, WIN_MIN, 4), 1, 68))               # everything lands on (41 - 10, 4 - 2)
    return out


NEAR_SINGULAR_DIFFS = [1e-6, 1e-8, 1e-9, 1e-10, 1e-11, 3e-12, 1e-12, 1e-13]


def near_singular():
    """G4: second row = 0.75 x first row + (d, -d): det = -1.5 d straddles |det| > 1e-12, and the inverse stops bringing the corners
    back within 1e-3 px on the way down.  Admission 2 while the inverse is trusted, 1 below (never 0)."""
    out = []
    W, H = 80, 60
    for d in NEAR_SINGULAR_DIFFS:
        m = [1, 0.75 + d, 0.5, 0.375 - d, 0.5, 0.25]
        out.append(_g(f"near_singular_{d:g}", 0, m, W, H, _fit(0, m, W, H, (1, 1, 1, 1)), 2 if d >= 1e-11 else 1, 69))
    return out


def minify():
    """G5: many writers per pixel."""
    out = []
    for sx, sy, W, H in ((1 / 16, 1 / 16, 1040, 320), (1 / 64, 1 / 64, 4160, 128), (1 / 32, 4, 2080, 20), (4, 1 / 32, 20, 2080)):
        m = [sx, 0, 0, sy, 0.25, 0.25]
        c = _g(f"minify_{1 / sx:g}_{1 / sy:g}", 0, m, W, H, _fit(0, m, W, H), 2, 70)
        c["writers"] = int(round(max(1 / sx, 1) * max(1 / sy, 1)))
        out.append(c)
    return out


def projective_limits():
    """G6: each admission limit of a projective frame at its value and just past it (small sources keep the windows small)."""
    out = []
    W, H, s = 21, 16, 0.2
    for corner, (cx, cy) in (("x", (1, 0)), ("y", (0, 1)), ("xy", (1, 1))):
        for den, admit, tag in ((DEN_MIN * UP, 2, "in"), (DEN_MIN * (2 - UP), 0, "out")):
            g = (den - 1) / (cx * (W - 1) + cy * (H - 1))
            m = [s, 0, 0, 0, s, 0, g * cx, g * cy]
            out.append(_g(f"den_{corner}_{tag}", 1, m, W, H, _fit(1, m, W, H, (1, 1, 1, 1)), admit, 71))
    for k, (W, H) in ((6, (70, 8)), (7, (8, 70))):                             # |m6|, |m7| = 0.1, the denominator growing
        for v, admit, tag in ((PERSP_MAX, 2, "in"), (0.1000001, 0, "out"), (-PERSP_MAX, 2, "neg_in"), (-0.1000001, 0, "neg_out")):
            m = [40, 0, 0, 0, 40, 0, 0, 0]
            m[k] = v
            if v < 0:                                                          # the denominator falls to 0.1 at the far corner: a short source
                Wn, Hn = (10, 8) if k == 6 else (8, 10)
                m[0] = m[4] = 8
            else:
                Wn, Hn = W, H
            out.append(_g(f"m{k}_{tag}", 1, m, Wn, Hn, _fit(1, m, Wn, Hn, (1, 1, 1, 1)), admit, 72))
    for v, admit, tag in ((ENTRY_MAX[1], 2, "in"), (ENTRY_MAX[1] * UP, 0, "out")):
        m = [1, 0, v, 0, 1, -v, 0, 0]
        out.append(_g(f"entry_proj_{tag}", 1, m, 90, 20, _fit(1, m, 90, 20, (1, 1, 1, 1)), admit, 73))
    for v, admit, tag in ((ENTRY_MAX[0], 2, "in"), (ENTRY_MAX[0] * UP, 0, "out")):
        m = [1, 0, 0, 1, v, -v]
        out.append(_g(f"entry_aff_{tag}", 0, m, 90, 20, _fit(0, m, 90, 20, (1, 1, 1, 1)), admit, 73))
    for m2, admit, tag in ((9990.9, 2, "in"), (9991.0, 0, "out")):             # corner image (9 + m2) / 0.1 against 1e5
        m = [1, 0, m2, 0, 0.05, 0, -0.1, 0]
        out.append(_g(f"image_proj_{tag}", 1, m, 10, 3, _fit(1, m, 10, 3, (1, 1, 1, 1)), admit, 74))
    return out


def source_limits():
    """G7: the largest sources (65535 wide; 65535 tall under a transposition), one column more (scatter), and sources a few rows around one
    and two passes under a map that folds 8 source rows and 8 columns into one output row: a tile's source rows span several passes, and
    every source row wins somewhere."""
    out = [_g("wide_65535", 0, [1, 0, 0, 1, 0.5, 0], SRC_MAX, 16, (1, 0, SRC_MAX, 16), 2, 75),
           _g("tall_65535", 0, [0, 1, 1, 0, 0, 0.5], 16, SRC_MAX, (0, 1, SRC_MAX, 16), 2, 75),
           _g("wide_65536", 0, [1, 0, 0, 1, 0.5, 0], SRC_MAX + 1, 16, (1, 0, SRC_MAX + 1, 16), 0, 75)]
    for H in (256, 257, 512, 513):
        m = [1, 0.125, 0, 0.125, 0, 0.375]
        out.append(_g(f"passes_h{H}", 0, m, 80, H, _fit(0, m, 80, H, (0, 1, 0, 1)), 2, 76))
        ms = [1, 0.125, 1 - 1e-13, 0.125, 0, 0.375]                            # ... |det| below 1e-12: no inverse, every tile scans all rows, passes from row 0
        out.append(_g(f"passes_all_rows_h{H}", 0, ms, 80, H, _fit(0, ms, 80, H, (1, 1, 1, 1)), 1, 76))
    return out


def batch():
    """G8: five frames of one affine batch on one source size (two images: frame f reads image f mod 2): a 64-wide window with 30 columns
    outside on both sides, a single-row window, an empty one in the middle, one that needs both aliasing regions, a 1.5 scale with ties."""
    W, H = WIN_MIN + 2 * ALIAS + 1, 40
    ident = [1, 0, 0, 1, 0, 0, 0, 0]
    frames = [(ident, (ALIAS, 1, WIN_MIN, H - 2)), (ident, (0, 20, W, 1)), (ident, (0, 0, 0, H)), (ident, (20, 1, W - 40, H - 2)),
              ([1.5, 0, 0, 1.5, 0.5, 0.5, 0, 0], (1, 1, 186, 60))]
    return {"kind": 0, "W": W, "H": H, "seeds": (77, 78), "frames": [(np.float64(m), g) for m, g in frames]}


def fuzz(seed, n, admissible):
    """G9: n draws from the ranges of the builders above; returns (admitted cases, draws that admission refused, draws whose window was too large to use).  `admissible` is hg_forward_tiles_admissible."""
    rng = np.random.default_rng(seed)
    sizes = [(96, 40), (140, 100), (70, 270), (300, 64), (200, 130), (64, 64)]
    out, refused, skipped = [], 0, 0
    for trial in range(n):
        W, H = sizes[trial % len(sizes)]
        kind, mode = trial % 2, trial % 7
        ang = rng.choice([0, np.pi / 2, np.pi, -np.pi / 2, rng.uniform(-3.2, 3.2)])
        sx, sy = 10 ** rng.uniform(-1.0, 0.7, 2)
        A = np.array([[np.cos(ang) * sx, -np.sin(ang) * sy], [np.sin(ang) * sx, np.cos(ang) * sy]])
        if mode == 1: A[0, 0] = rng.choice(SLOPES)
        if mode == 2: A[1] = A[0] * rng.uniform(0.5, 2) + rng.uniform(-1, 1, 2) * 10 ** rng.uniform(-13, -6)
        if mode == 3: A[1, 0] = rng.choice(SLOPES)
        t = np.floor(rng.uniform(-300, 300, 2)) + rng.choice([0, 0.5, 0.25, rng.uniform()])
        if mode == 4: t = np.floor(rng.uniform(-9e5, 9e5, 2) if kind == 0 else rng.uniform(-9e3, 9e3, 2)) + 0.5
        if kind == 0:
            m = np.array([A[0, 0], A[1, 0], A[0, 1], A[1, 1], t[0], t[1]])
            if trial % 3: m = m.astype(np.float32).astype(np.float64)
        else:
            g = rng.uniform(-1, 1, 2) * 10 ** rng.uniform(-5, -1, 2) * [70 / W, 70 / H]
            if mode == 5:                                                      # a denominator close to its floor at one corner
                d = DEN_MIN * rng.uniform(1.01, 5)
                g = np.array([(d - 1) / (W - 1), 0.0]) if trial % 2 else np.array([0.0, (d - 1) / (H - 1)])
                if np.abs(g).max() > PERSP_MAX: g *= PERSP_MAX / np.abs(g).max()
                A *= 0.05
            m = np.array([A[0, 0], A[0, 1], t[0], A[1, 0], A[1, 1], t[1], g[0], g[1]])
        with np.errstate(all="ignore"):
            x0, y0, x1, y1 = _hull(kind, m, W, H) if np.all(np.isfinite(m)) else (0, 0, 0, 0)
        ow, oh = x1 - x0 + 1, y1 - y0 + 1
        if not (WIN_MIN <= ow <= 2500 and 1 <= oh <= 2500 and ow * oh <= 400_000):
            if ow < WIN_MIN and oh >= 1 and oh <= 2500:
                x0, ow = x0 - (WIN_MIN - ow) // 2, WIN_MIN                         # a thin image in the narrowest window
            else:
                skipped += 1; continue
        geom = (x0, y0, ow, oh)
        if mode == 6 and ow > WIN_MIN + 2 * ALIAS:                             # columns outside on both sides, up to the limit
            a, b = int(rng.integers(1, ALIAS + 1)), int(rng.integers(1, ALIAS + 1))
            geom = (x0 + a, y0 + 1, ow - a - b, max(oh - 2, 1))
        code = admissible(kind, m, W, H, geom)
        if code: out.append(_g(f"fuzz{trial}", kind, m, W, H, geom, code, 5000 + trial))
        else: refused += 1
    return out, refused, skipped


def geometric_cases():
    cases = tile_border_ties() + alias_limit() + slopes() + near_singular() + minify() + projective_limits() + source_limits()
    return {c["name"]: c for c in cases}


# ------------------------------------------------------------------------------------------------ piecewise builders

def _p(name, sp, tris, dp, W, H, geom, seed=81, box=None, **extra):
    sp, dp = np.ascontiguousarray(sp, np.float32).ravel(), np.ascontiguousarray(dp, np.float32).ravel()
    if box is None:
        ms = O.minmax_xy(sp)
        box = (int(ms[0]), int(ms[1]), int(ms[2]), int(ms[3]))
    c = {"name": name, "sp": sp, "tris": np.ascontiguousarray(tris, np.uint32).ravel(), "dp": dp, "W": int(W), "H": int(H), "seed": seed,
         "geom": tuple(int(v) for v in geom), "msx": box[0], "msy": box[1], "Mx": box[2], "My": box[3],
         "flagged": 0, "kernel": 2}                # frames redone on the first call; the kernel code that call reports
    c.update(extra)
    return c


def _grid(x0, y0, x1, y1, nx, ny):
    xs, ys = np.linspace(x0, x1, nx + 1), np.linspace(y0, y1, ny + 1)
    gx, gy = np.meshgrid(xs, ys)
    return np.stack([gx, gy], -1).reshape(-1, 2), WL.grid_triangles(nx, ny)


def _dst_geom(dp):
    md = O.minmax_xy(np.ascontiguousarray(dp, np.float32).ravel())
    return (int(md[0]), int(md[1]), int(md[2] - md[0]), int(md[3] - md[1]))


def shifts():
    """P1: a window one FIFTH as wide as the destination box (five aliasing shifts need five window widths), placed so that every
    k = -2..2 has writers in one frame and k_fwd_pw_bins' padded bounds (+-2 pixels) stay inside +-2; the twin's box reaches k = +-3."""
    s, tris = _grid(0, 0, 312, 64, 6, 2)
    d = s + [0.5, 0.5]
    return [_p("shifts_5", s, tris, d, 320, 64, (126, 0, TILE, 64), 82),
            _p("shifts_7", s, tris, d, 320, 64, (140, 0, 40, 64), 82, flagged=1)]


def collapsed():
    """P2: destination triangles with three collinear vertices, three coincident ones (forward determinant 0) and a tiny non-zero
    determinant, next to regular ones."""
    out = []
    s, tris = _grid(0, 0, 256, 128, 4, 2)                 # vertex j * 5 + i; triangle 0 = (0, 1, 5), triangle 1 = (1, 6, 5)
    for tag in ("collinear", "coincident", "tiny_det"):
        d = s * 1.0 + [3.5, 2.5]
        if tag == "coincident":
            d[1] = d[0]; d[5] = d[0]                      # triangle 0 is a point, triangle 1 a segment
        else:
            d[5] = (d[0] + d[1]) / 2 + ([0, 2.0 ** -10] if tag == "tiny_det" else [0, 0])
        out.append(_p(f"collapsed_{tag}", s, tris, d, 256, 128, _dst_geom(d), 83))
    return out


def rotated():
    """P3: destination = source turned by exactly 90 degrees (m0 == 0, m3 == 0), and the same with one vertex moved by one f32 ulp."""
    s, tris = _grid(0, 0, 256, 192, 4, 3)
    d = np.stack([200.5 - s[:, 1], s[:, 0] + 0.5], -1)
    d1 = d.astype(np.float32)
    d1[7, 0] = np.nextafter(d1[7, 0], np.float32(np.inf))
    return [_p("rotated_90", s, tris, d, 256, 192, _dst_geom(d), 84), _p("rotated_90_ulp", s, tris, d1, 256, 192, _dst_geom(d), 84)]


def scaled():
    """P4: 1/64 horizontally (one tile holds more than 1024 segments; with 1/5 vertically more than 512 (entry, row) records) and 16 x."""
    out = []
    for nx, ny in ((1, 1), (8, 8)):
        s, tris = _grid(0, 0, 4160, 320, nx, ny)
        d = s * [1 / 64, 1 / 5] + [0.5, 0.25]
        # (3 free columns and rows on every side: k_fwd_pw_bins' padded bounds stay in k = 0, so the 8 x 8 mesh files exactly its 128
        # triangles under the tile at the origin: one overflow at capacity 64, none at 128)
        out.append(_p(f"minify_64_{nx}x{ny}", s, tris, d, 4160, 320, (-3, -3, 72, 71), 85, flagged=1 if nx == 8 else 0, entries=2 * nx * ny))
        s, tris = _grid(0, 0, 40, 32, nx, ny)
        d = s * 16.0 + [0.5, 0.5]
        out.append(_p(f"magnify_16_{nx}x{ny}", s, tris, d, 40, 32, _dst_geom(d), 85))
    return out


def dense(strips):
    """P5: 2 * strips thin triangles (source strips two rows tall, 64 wide) squeezed into 60 output rows: every one of them crosses
    the tile at the origin, so that tile holds 2 * strips entries (k = 0 only: the window leaves 3 columns free on both sides)."""
    s, tris = _grid(0, 0, 64, 2 * strips, 1, strips)
    d = s * [1.0, 60.0 / (2 * strips)]
    return _p(f"dense_{2 * strips}", s, tris, d, 64, 2 * strips, (-3, 0, 70, 60), 86, entries=2 * strips)


DENSE = {"65-128": 48, "129-256": 100, ">256": 140}


def many_triangles(n_pad):
    """P6: an 8 x 4 grid (64 triangles) behind n_pad copies of one padding triangle, so that the real triangles carry the ids n_pad ..
    n_pad + 63.  The padding's source triangle lies below the source box the case passes (its rows fall outside the forward map); its
    destination is a regular triangle, because ids past 65535 wrap and select ITS matrix (id - 65536)."""
    s, tris = _grid(0, 0, 256, 128, 8, 4)
    d = s * 0.75 + [2.5, 1.5]
    pad_s = np.float64([[0, 200], [8, 200], [0, 208]])
    pad_d = pad_s * 0.5 + [20.0, -90.0]             # ids >= 65536 use this map: (x, y) -> (x / 2 + 20, y / 2 - 90)
    sp, dp = np.concatenate([pad_s, s]), np.concatenate([pad_d, d])
    t = np.concatenate([np.tile(np.uint32([0, 1, 2]), n_pad), tris + np.uint32(3)])
    return _p(f"many_{n_pad + 64}", sp, t, dp, 256, 128, (0, -30, 200, 130), 87, box=(0, 0, 256, 128), first_id=n_pad)


def off_image():
    """P7: source points left of, above, right of and below the image, half scale: writers that read outside the source (0) or the
    neighbouring source row land over writers that read a pixel."""
    s, tris = _grid(-8, -6, 136, 102, 4, 4)
    d = s * 0.5 + [10.25, 8.25]
    return _p("off_image", s, tris, d, 128, 96, _dst_geom(d), 88)


def limits():
    """P8: a source box 65535 wide (tiles) and 65536 wide (scatter); a forward matrix entry above 1e6; a NaN destination vertex."""
    out = []
    for w in (SRC_MAX, SRC_MAX + 1):
        s, tris = _grid(0, 0, w, 8, 1, 1)
        d = s * [1 / 64, 1.0] + [0.5, 0.5]
        out.append(_p(f"box_{w}", s, tris, d, SRC_MAX, 8, _dst_geom(d), 89, kernel=2 if w <= SRC_MAX else 1))
    s, tris = _grid(0, 0, 128, 128, 2, 2)
    far = float(1 << 21)
    assert far > PW_ENTRY_MAX
    out.append(_p("entry_2e6", s, tris, s + [far, 0.0], 128, 128, (1 << 21, 0, 128, 128), 89, flagged=1))
    d = s + [0.5, 0.5]
    d[4] = np.nan                                    # the centre vertex: six of the eight matrices
    out.append(_p("nan_vertex", s, tris, d, 128, 128, (0, 0, 129, 129), 89, flagged=1))
    return out


def piecewise_batch():
    """P9: one mesh, frames of mixed windows with an empty one, one source per frame."""
    s, tris = _grid(0, 0, 192, 96, 6, 3)
    sp = s.astype(np.float32).ravel()
    frames = []
    for f, (sc, t, g) in enumerate([((1.0, 1.0), (0.5, 0.5), None), ((0.5, 0.5), (-20.5, 3.5), None), ((1.0, 1.0), (0, 0), (0, 0, 0, 50)),
                                    ((1.5, 0.75), (4.25, -7.5), None), ((1.0, 1.0), (0.5, 0.5), (40, 1, 100, 94))]):
        d = (s * sc + t).astype(np.float32).ravel()
        frames.append((d, _dst_geom(d) if g is None else g))
    return {"sp": sp, "tris": tris, "W": 192, "H": 96, "box": (0, 0, 192, 96), "frames": frames, "seeds": [90 + f for f in range(len(frames))]}


def piecewise_cases():
    cases = shifts() + collapsed() + rotated() + scaled() + [dense(n) for n in DENSE.values()] + \
        [many_triangles(32767 - 32), many_triangles(65536 - 32)] + [off_image()] + limits()
    return {c["name"]: c for c in cases}
