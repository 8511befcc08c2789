"""Numpy model of the point lists (include/hgwarp.h, hg_points_*).  Test infrastructure only: f64 in the reference's operation order (numpy
never fuses a*b+c; bilinear.geometric_coords' order), one rounding to f32 at the end, over the CPU oracle's maps and matrices
(oracle.build_tri_map / piecewise_matrices / inverse_affine), never the library's.

    cell          (Math.round(x), Math.round(y)), ties toward +Infinity, as doubles: NaN / +-Inf / 1e30 stay what they are and fail every
                  range test, so no integer is ever formed from them
    to source     (u, v) in window coordinates; mapped iff the cell lies in [0, objW) x [0, objH) and the coordinate of the point itself
                  passes the loop's coverage test (:1001; :1045-1047 with the id the map holds at the cell)
    to output     (px, py) in source pixels; mapped iff the cell lies in the loop's domain (:919-920; :955-958 through the forward map);
                  the result is the forward transform of the point itself minus the window's offsets, wherever it falls
An unmapped point is 0x7fc00000 in both words.  Every function returns an (n, 2) float32 array."""
import numpy as np

from . import oracle as O

F32 = np.float32
NAN_BITS = np.uint32(0x7FC00000)


def _round(v):
    with np.errstate(invalid="ignore"):
        f = np.floor(v)
        return f + ((v - f) >= 0.5)


def cells(pts):
    """(cx, cy) as float64 arrays (non-finite where the input is)."""
    p = np.asarray(pts, F32).reshape(-1, 2).astype(np.float64)
    return _round(p[:, 0]), _round(p[:, 1])


def _inside(cx, cy, x0, y0, w, h):
    with np.errstate(invalid="ignore"):
        return (cx - x0 >= 0) & (cx - x0 < w) & (cy - y0 >= 0) & (cy - y0 < h)


def _result(x, y, mapped):
    out = np.full((x.size, 2), NAN_BITS, np.uint32).view(F32)
    with np.errstate(all="ignore"):
        out[mapped, 0] = x[mapped].astype(F32)
        out[mapped, 1] = y[mapped].astype(F32)
    return out


def _geometric(kind, m, x, y):
    m = np.asarray(m, np.float64)
    with np.errstate(all="ignore"):
        if kind == 0:
            return (m[0] * x + m[2] * y) + m[4], (m[1] * x + m[3] * y) + m[5]
        den = (m[6] * x + m[7] * y) + 1.0
        return ((m[0] * x + m[1] * y) + m[2]) / den, ((m[3] * x + m[4] * y) + m[5]) / den


def _affine_rows(mats, ids, x, y):
    mm = np.asarray(mats, F32).reshape(-1, 6).astype(np.float64)[ids]
    with np.errstate(all="ignore"):
        return (mm[:, 0] * x + mm[:, 2] * y) + mm[:, 4], (mm[:, 1] * x + mm[:, 3] * y) + mm[:, 5]


def to_source_geometric(kind, m, pts, geom, W, H):
    """m: the INVERSE matrix (6 / 8 doubles)."""
    xoff, yoff, objw, objh = geom
    p = np.asarray(pts, F32).reshape(-1, 2).astype(np.float64)
    cx, cy = cells(pts)
    sx, sy = _geometric(kind, m, p[:, 0] + xoff, p[:, 1] + yoff)
    with np.errstate(invalid="ignore"):
        ok = _inside(cx, cy, 0, 0, objw, objh) & (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)      # :1001
    return _result(sx, sy, ok)


def to_source_piecewise(map16, inv, pts, geom, W, H, msx, msy):
    """map16: the Int16 map of the window (objw * objh cells); inv: (T, 6) float32 inverse matrices."""
    xoff, yoff, objw, objh = geom
    p = np.asarray(pts, F32).reshape(-1, 2).astype(np.float64)
    cx, cy = cells(pts)
    ins = _inside(cx, cy, 0, 0, objw, objh)
    ids = np.full(p.shape[0], -1, np.int64)
    if ins.any():
        ids[ins] = np.asarray(map16).astype(np.int64)[cy[ins].astype(np.int64) * objw + cx[ins].astype(np.int64)]
    has = ids >= 0                                                                                  # :1045
    sx, sy = _affine_rows(inv, np.where(has, ids, 0), p[:, 0] + xoff, p[:, 1] + yoff)
    with np.errstate(invalid="ignore"):
        ok = has & (sx >= msx) & (sx < W + msx) & (sy >= msy) & (sy < H + msy)                      # :1047
    return _result(sx, sy, ok)


def to_source_piecewise_mesh(sp, dp, tris, pts, geom, W, H, msx, msy):
    """The same from the mesh: the oracle's map of the window and its inverse matrices."""
    objw, objh = max(geom[2], 0), max(geom[3], 0)
    if objw * objh == 0:
        return _result(np.zeros(np.asarray(pts).size // 2), np.zeros(np.asarray(pts).size // 2), np.zeros(np.asarray(pts).size // 2, bool))
    wmap = O.build_tri_map(dp, tris, objw, geom[1], objw * objh)
    fwd = O.piecewise_matrices(sp, dp, tris)
    inv = np.stack([O.inverse_affine(f) for f in fwd]) if len(fwd) else np.zeros((0, 6), F32)
    return to_source_piecewise(wmap, inv, pts, geom, W, H, msx, msy)


def to_output_geometric(kind, m, pts, geom, W, H, raw=False):
    """m: the FORWARD matrix.  raw: (x, y, mapped) in f64 instead, before the rounding to f32."""
    xoff, yoff = geom[0], geom[1]
    p = np.asarray(pts, F32).reshape(-1, 2).astype(np.float64)
    cx, cy = cells(pts)
    nx, ny = _geometric(kind, m, p[:, 0], p[:, 1])                                                  # :923
    ok = _inside(cx, cy, 0, 0, W, H)                                                                # :919-920
    with np.errstate(invalid="ignore"):
        return (nx - xoff, ny - yoff, ok) if raw else _result(nx - xoff, ny - yoff, ok)             # :924


def to_output_piecewise(fmap16, fwd, pts, geom, msx, msy, maxx, maxy, raw=False):
    """fmap16: the Int16 forward map over the source box (:817-832); fwd: (T, 6) float32 forward matrices.  raw: as to_output_geometric."""
    xoff, yoff = geom[0], geom[1]
    mw, mh = max(maxx - msx, 0), max(maxy - msy, 0)
    p = np.asarray(pts, F32).reshape(-1, 2).astype(np.float64)
    cx, cy = cells(pts)
    ins = _inside(cx, cy, msx, msy, mw, mh)
    ids = np.full(p.shape[0], -1, np.int64)
    if ins.any():
        ids[ins] = np.asarray(fmap16).astype(np.int64)[(cy[ins] - msy).astype(np.int64) * mw + (cx[ins] - msx).astype(np.int64)]
    has = ids > -1                                                                                  # :958
    nx, ny = _affine_rows(fwd, np.where(has, ids, 0), p[:, 0], p[:, 1])                             # :961
    with np.errstate(invalid="ignore"):
        return (nx - xoff, ny - yoff, has) if raw else _result(nx - xoff, ny - yoff, has)           # :962


def forward_map(sp, tris, msx, msy, maxx, maxy):
    """The forward triangle map of :817-832: the source triangles over the source box, width maxSrcX - minSrcX, y offset minSrcY."""
    mw, mh = max(maxx - msx, 0), max(maxy - msy, 0)
    return O.build_tri_map(sp, tris, mw, msy, mw * mh)


def paint_at(u, v, values, objw, objh):
    """The forward loops' painting (:926-928 / :964-967) of `values` (n, 4 uint8) at the ROUNDED positions (u, v) (f64 arrays; NaN rows are
    not painted), last writer in list order: flat index (v * objw + u) * 4 as the reference forms it (u outside [0, objw) aliases into the
    neighbouring rows), dropped where it leaves the array.  Returns (objh, objw, 4) uint8."""
    out = np.zeros((max(objh, 0) * max(objw, 0), 4), np.uint8)
    with np.errstate(invalid="ignore"):
        idx = v * objw + u
        keep = (idx >= 0) & (idx < out.shape[0])
    out[idx[keep].astype(np.int64)] = np.asarray(values)[keep]            # (numpy assigns in order: the last writer stays)
    return out.reshape(max(objh, 0), max(objw, 0), 4)


def paint(res, values, objw, objh, exact=None):
    """paint_at Math.round of the results (n, 2 float32).  exact = (x, y) f64: the rows of rounding_outliers are painted at Math.round of
    the exact value instead; returns (picture, number of such rows)."""
    r = np.asarray(res, F32).astype(np.float64)
    u, v = _round(r[:, 0]), _round(r[:, 1])
    if exact is None:
        return paint_at(u, v, values, objw, objh)
    out = rounding_outliers(res, exact[0], exact[1]) & ~np.isnan(r).any(1)
    u, v = np.where(out, _round(exact[0]), u), np.where(out, _round(exact[1]), v)
    return paint_at(u, v, values, objw, objh), int(out.sum())


def rounding_outliers(res, exact_x, exact_y):
    """Rows whose f32-rounded value rounds to another integer than the f64 value, in either coordinate (what the raster anchors may leave out)."""
    r = np.asarray(res, F32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (_round(r[:, 0]) != _round(exact_x)) | (_round(r[:, 1]) != _round(exact_y))
