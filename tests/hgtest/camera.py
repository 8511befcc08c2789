"""A numpy model of the camera models, written from the text of include/hgwarp.h ("camera models") alone: float64 in the written operation
order, a longdouble variant (dtype=LD) that the tolerances are taken around, the first-order error bound `delta` of the canvas -> source
chain, and the checks tests/test_camera_cpu.py (on the host program's output) and tests/test_gpu_camera.py (on the device's) both make."""
import math

import numpy as np

F64, LD = np.float64, np.longdouble
PLANE, CYLINDER, SPHERE = 0, 1, 2
RECORD, ITERS = 32, 20
FX, FY, CX, CY, K1, K2, P1, P2, K3, R2MAX, AC = range(9, 20)
TWO_PI = 6.283185307179586
TOL = 1e-9
EPS = 2.0 ** -52                             # one ulp of float64, relative
NANP = 0x7FC00000
WORST = [0.0]                                # the largest |device - model| / delta any check has seen
STORED = [0, 0]                              # coordinates compared, and those that were not float32(the longdouble model)
EXCUSED = [0]                                # decisions (covered / valid) that differed from the model's within delta of a bound


# ------------------------------------------------------------------------------------------------ rotations
def rot(yaw=0.0, pitch=0.0, roll=0.0):
    """camera <- world for a camera turned by yaw about y (to the right), then pitch about x (up is positive: y grows downwards), then roll about z: the
    optical axis of rot(yaw) lies at azimuth yaw."""
    cy, sy, cp, sp, cr, sr = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])                # world <- camera of a yaw
    rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    return (ry @ rx @ rz).T


# ------------------------------------------------------------------------------------------------ the two maps
def lens(rec, xn, yn):
    k1, k2, p1, p2, k3 = rec[K1], rec[K2], rec[P1], rec[P2], rec[K3]
    r2 = xn * xn + yn * yn
    rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
    tx = ((2 * p1) * xn) * yn + p2 * (r2 + (2 * xn) * xn)
    ty = p1 * (r2 + (2 * yn) * yn) + ((2 * p2) * xn) * yn
    return rad, tx, ty, r2


def ray_terms(surface, scale, u0, v0, U, V, dtype=F64):
    """(sa, ca, yb, cb, a, b): the ray is (sa cb, yb, ca cb)."""
    U, V = np.asarray(U, dtype), np.asarray(V, dtype)
    a, b = (U - dtype(u0)) / dtype(scale), (V - dtype(v0)) / dtype(scale)
    one = np.ones_like(a)
    with np.errstate(invalid="ignore"):
        sa, ca = (a, one) if surface == PLANE else (np.sin(a), np.cos(a))
        yb, cb = (np.sin(b), np.cos(b)) if surface == SPHERE else (b, np.ones_like(b))
    return sa, ca, yb, cb, a, b


def to_source(rec, surface, scale, u0, v0, U, V, dtype=F64):
    """Canvas -> source: (sx, sy, cz, r2) in `dtype`; the rule c.z > 0 && r2 <= r2_max is `inside`."""
    rec = np.asarray(rec, F64).astype(dtype)
    sa, ca, yb, cb, _, _ = ray_terms(surface, scale, u0, v0, U, V, dtype)
    with np.errstate(all="ignore"):
        x, y, z = sa * cb, yb, ca * cb
        c0 = (rec[0] * x + rec[1] * y) + rec[2] * z
        c1 = (rec[3] * x + rec[4] * y) + rec[5] * z
        c2 = (rec[6] * x + rec[7] * y) + rec[8] * z
        xn, yn = c0 / c2, c1 / c2
        rad, tx, ty, r2 = lens(rec, xn, yn)
        xd, yd = xn * rad + tx, yn * rad + ty
        return rec[FX] * xd + rec[CX], rec[FY] * yd + rec[CY], c2, r2


def inside(rec, cz, r2):
    with np.errstate(invalid="ignore"):
        return (cz > 0) & (r2 <= rec[R2MAX])


def covered(rec, sx, sy, cz, r2, W, H):
    with np.errstate(invalid="ignore"):
        return inside(rec, cz, r2) & (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)


def undistort(rec, xd, yd):
    with np.errstate(all="ignore"):
        xn, yn = xd, yd
        for _ in range(ITERS):
            rad, tx, ty, _ = lens(rec, xn, yn)
            xn, yn = (xd - tx) / rad, (yd - ty) / rad
        rad, tx, ty, r2 = lens(rec, xn, yn)
        xe, ye = xn * rad + tx, yn * rad + ty
        ok = (np.abs(xe - xd) <= TOL) & (np.abs(ye - yd) <= TOL) & (r2 <= rec[R2MAX])
    return xn, yn, r2, ok


_remainder = np.vectorize(math.remainder, otypes=[F64])


def to_canvas(rec, surface, scale, u0, v0, x, y):
    """Source -> canvas in float64: (U, V, valid)."""
    rec = np.asarray(rec, F64)
    x, y = np.asarray(x, F64), np.asarray(y, F64)
    with np.errstate(all="ignore"):
        xd, yd = (x - rec[CX]) / rec[FX], (y - rec[CY]) / rec[FY]
        xn, yn, _, ok = undistort(rec, xd, yd)
        wx = (rec[0] * xn + rec[3] * yn) + rec[6]
        wy = (rec[1] * xn + rec[4] * yn) + rec[7]
        wz = (rec[2] * xn + rec[5] * yn) + rec[8]
        if surface == PLANE:
            ok = ok & (wz > 0)
            a, b = wx / wz, wy / wz
        else:
            h = np.sqrt(wx * wx + wz * wz)
            a = np.arctan2(wx, wz)
            b = wy / h if surface == CYLINDER else np.arctan2(wy, h)
            d = a - rec[AC]
            a = rec[AC] + np.where(np.isfinite(d), _remainder(np.where(np.isfinite(d), d, 0.0), TWO_PI), np.nan)
        return u0 + scale * a, v0 + scale * b, ok


# ------------------------------------------------------------------------------------------------ the host calls
def pack_record(R, fx, fy, cx, cy, dist, W, H):
    R = np.asarray(R, F64).reshape(9)
    vals = [fx, fy, cx, cy, *R, *(dist if dist is not None else [])]
    if W < 1 or H < 1 or not np.isfinite(vals).all() or fx <= 0 or fy <= 0:
        raise ValueError("refused")
    m = R.reshape(3, 3)
    if (np.abs(m.T @ m - np.eye(3)) > 1e-6).any():
        raise ValueError("not orthonormal")
    rec = np.zeros(RECORD)
    rec[:9] = R
    rec[FX:CY + 1] = fx, fy, cx, cy
    if dist is not None:
        rec[K1:K3 + 1] = dist
    rec[R2MAX] = np.inf
    rec[AC] = math.atan2(R[6], R[8])
    if dist is not None:
        px = np.array([0, W, 0, W, W / 2, W / 2, 0, W], F64)
        py = np.array([0, 0, H, H, 0, H, H / 2, H / 2], F64)
        _, _, r2, ok = undistort(rec, (px - cx) / fx, (py - cy) / fy)
        if not ok.all():
            raise ValueError("the distortion is too strong")
        rec[R2MAX] = 1.05 * r2.max()
    return rec


def border(W, H):
    i, j = np.arange(W + 1, dtype=F64), np.arange(H + 1, dtype=F64)
    return (np.concatenate([i, i, np.zeros(H + 1), np.full(H + 1, float(W))]), np.concatenate([np.zeros(W + 1), np.full(W + 1, float(H)), j, j]))


def limits(rec, W, H, surface, scale, u0, v0):
    U, V, ok = to_canvas(rec, surface, scale, u0, v0, *border(W, H))
    ok = ok & np.isfinite(U) & np.isfinite(V)
    if not ok.any():
        raise ValueError("no valid border position")
    lo_u, hi_u, lo_v, hi_v = U[ok].min(), U[ok].max(), V[ok].min(), V[ok].max()
    if surface != PLANE:
        for s in (-1.0, 1.0):
            c = np.asarray(rec[:9]).reshape(3, 3) @ np.array([0.0, s, 0.0])
            with np.errstate(all="ignore"):
                xn, yn = c[0] / c[2], c[1] / c[2]
                rad, tx, ty, r2 = lens(rec, xn, yn)
                sx, sy = rec[FX] * (xn * rad + tx) + rec[CX], rec[FY] * (yn * rad + ty) + rec[CY]
            if c[2] > 0 and r2 <= rec[R2MAX] and 0 <= sx < W and 0 <= sy < H:
                if surface == CYLINDER:
                    raise ValueError("a pole inside a cylinder's picture")
                lo_u, hi_u = min(lo_u, u0 + scale * (rec[AC] - TWO_PI / 2)), max(hi_u, u0 + scale * (rec[AC] + TWO_PI / 2))
                vp = v0 + scale * (s * (TWO_PI / 4))
                lo_v, hi_v = min(lo_v, vp), max(hi_v, vp)
    x0, x1, y0, y1 = math.floor(lo_u) - 1, math.ceil(hi_u) + 1, math.floor(lo_v) - 1, math.ceil(hi_v) + 1
    return x0, y0, x1 - x0 + 1, y1 - y0 + 1


def first_image(rec, scale, u0, v0, U, V):
    """Sphere positions brought back to their first image: the canvas is periodic (the same direction one turn further) and shows a
    direction again across a pole (elevation b beyond +-pi/2 is the direction (a + pi, pi - b)); the result has its azimuth within
    a_c +- pi and its elevation within +-pi/2."""
    a, b = (np.asarray(U, F64) - u0) / scale, (np.asarray(V, F64) - v0) / scale
    b = _remainder(b, TWO_PI)
    over, under = b > math.pi / 2, b < -math.pi / 2
    b = np.where(over, math.pi - b, np.where(under, -math.pi - b, b))
    a = rec[AC] + _remainder(np.where(over | under, a + math.pi, a) - rec[AC], TWO_PI)
    return u0 + scale * a, v0 + scale * b


# ------------------------------------------------------------------------------------------------ the tolerance
def delta(rec, surface, scale, u0, v0, U, V):
    """(dsx, dsy, dcz, dr2): the first-order bound of the float64 chain canvas -> source against exact arithmetic on the same inputs, every
    elementary operation at EPS relative and sin, cos at 4 EPS (the formula is written out in tests/test_gpu_camera.py).  Evaluated at the
    float64 model's own intermediate values."""
    rec = np.asarray(rec, F64)
    A = np.abs
    sa, ca, yb, cb, a, b = ray_terms(surface, scale, u0, v0, U, V)
    with np.errstate(all="ignore"):
        da, db = 2 * EPS * A(a), 2 * EPS * A(b)
        dsa, dca = (da, 0 * da) if surface == PLANE else (da + 4 * EPS, da + 4 * EPS)
        dyb, dcb = (db + 4 * EPS, db + 4 * EPS) if surface == SPHERE else (db, 0 * db)
        x, y, z = sa * cb, yb, ca * cb
        dx, dy, dz = A(cb) * dsa + A(sa) * dcb + EPS * A(x), dyb, A(cb) * dca + A(ca) * dcb + EPS * A(z)
        c, dc = [], []
        for i in range(3):
            r0, r1, r2_ = rec[3 * i], rec[3 * i + 1], rec[3 * i + 2]
            c.append((r0 * x + r1 * y) + r2_ * z)
            dc.append((A(r0) * dx + A(r1) * dy + A(r2_) * dz) + 3 * EPS * (A(r0 * x) + A(r1 * y) + A(r2_ * z)))
        xn, yn = c[0] / c[2], c[1] / c[2]
        dxn = (dc[0] + A(xn) * dc[2]) / A(c[2]) + EPS * A(xn)
        dyn = (dc[1] + A(yn) * dc[2]) / A(c[2]) + EPS * A(yn)
        rad, tx, ty, r2 = lens(rec, xn, yn)
        dr2 = 2 * A(xn) * dxn + 2 * A(yn) * dyn + 2 * EPS * r2
        k1, k2, p1, p2, k3 = (A(rec[k]) for k in (K1, K2, P1, P2, K3))
        drad = (k1 + 2 * k2 * r2 + 3 * k3 * r2 * r2) * dr2 + 6 * EPS * (1 + r2 * (k1 + r2 * (k2 + r2 * k3)))
        dtx = 2 * p1 * (A(yn) * dxn + A(xn) * dyn) + p2 * (dr2 + 4 * A(xn) * dxn) + 4 * EPS * (2 * p1 * A(xn * yn) + p2 * (r2 + 2 * xn * xn))
        dty = 2 * p2 * (A(yn) * dxn + A(xn) * dyn) + p1 * (dr2 + 4 * A(yn) * dyn) + 4 * EPS * (2 * p2 * A(xn * yn) + p1 * (r2 + 2 * yn * yn))
        dxd = A(rad) * dxn + A(xn) * drad + dtx + 2 * EPS * (A(xn * rad) + A(tx))
        dyd = A(rad) * dyn + A(yn) * drad + dty + 2 * EPS * (A(yn * rad) + A(ty))
        xd, yd = xn * rad + tx, yn * rad + ty
        dsx = A(rec[FX]) * dxd + 2 * EPS * (A(rec[FX] * xd) + A(rec[CX]))
        dsy = A(rec[FY]) * dyd + 2 * EPS * (A(rec[FY] * yd) + A(rec[CY]))
    return dsx, dsy, dc[2], dr2


def window_positions(g):
    x_off, y_off, w, h = g
    c, r = np.meshgrid(np.arange(max(w, 0)), np.arange(max(h, 0)))
    return (c + x_off).astype(F64), (r + y_off).astype(F64)


def pack256(geoms, px):
    """(offsets, total) of windows packed at the 256-byte grain."""
    offs, off = [], 0
    for g in geoms:
        offs.append(off)
        if g[2] > 0 and g[3] > 0:
            off += (g[2] * g[3] * px + 255) // 256 * 256
    return offs, off


def js_round(v):
    f = np.floor(v)
    return np.where(v - f >= 0.5, f + 1, f)


def model_field(rec, g, W, H, surface, scale, u0, v0, fmt_index):
    """The float64 model's field of one window, as the stored values: int32 indices (flat) or float32 pairs (n, 2)."""
    U, V = window_positions(g)
    if np.isnan(rec).any():
        n = U.size
        return np.full(n, -1, np.int32) if fmt_index else np.full((n, 2), NANP, np.uint32).view(np.float32)
    sx, sy, cz, r2 = (v.ravel() for v in to_source(rec, surface, scale, u0, v0, U, V))
    cov = covered(rec, sx, sy, cz, r2, W, H)
    if fmt_index:
        with np.errstate(invalid="ignore"):
            idx = js_round(np.where(cov, sy, 0)) * W + js_round(np.where(cov, sx, 0))
        return np.where(cov & (idx >= 0) & (idx < W * H), idx, -1).astype(np.int32)
    out = np.full((sx.size, 2), NANP, np.uint32).view(np.float32)
    out[cov, 0], out[cov, 1] = sx[cov].astype(np.float32), sy[cov].astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------ the checks both test files make
def _f32_between(v, lo, hi):
    with np.errstate(over="ignore"):
        return (v >= lo.astype(np.float32)) & (v <= hi.astype(np.float32))


def _note(got, v, d):
    """Record the largest |stored - model| / delta.  The stored value is a float32 and delta is some 1e-12 px, so the figure is the float32
    rounding over delta, about 1e6 to 1e7; what it hides is counted beside it: the stored values that are NOT float32(model)."""
    with np.errstate(all="ignore"):
        if got.size:
            WORST[0] = max(WORST[0], float(np.max(np.abs(got.astype(LD) - v) / d)))
            STORED[0] += int(got.size)
            STORED[1] += int((got != v.astype(np.float32)).sum())


def check_to_source(got, rec, surface, scale, u0, v0, U, V, W=None, H=None, fmt_index=False, what="", cap=0.001):
    """Stored values of canvas positions (U, V) -- a field's frame (W, H given: tested against the picture) or point results (W None) --
    against the longdouble model v: the decision (covered / valid) may differ from the model's only where sx, sy, c.z or r2 lies within its
    delta of its bound, and such excused positions are at most `cap` of the frame; a stored coordinate lies between float32(v - delta) and
    float32(v + delta); an index equals the model's unless a value lies within delta of a rounding tie.  Returns the excused count."""
    U, V = np.asarray(U, F64).ravel(), np.asarray(V, F64).ravel()
    n = U.size
    if np.isnan(rec).any():
        assert (np.frombuffer(got, np.int32) == -1).all() if fmt_index else (np.frombuffer(got, np.uint32) == NANP).all(), (what, "a NaN record")
        return 0
    sx, sy, cz, r2 = to_source(rec, surface, scale, u0, v0, U, V, LD)
    dx, dy, dcz, dr2 = delta(rec, surface, scale, u0, v0, U, V)
    with np.errstate(invalid="ignore"):
        near = (np.abs(cz) <= dcz) | (np.abs(r2 - rec[R2MAX]) <= dr2)
        cov = inside(rec, cz, r2)
        if W is not None:
            near |= (np.abs(sx) <= dx) | (np.abs(sx - W) <= dx) | (np.abs(sy) <= dy) | (np.abs(sy - H) <= dy)
            cov &= (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
        cov &= ~(np.isnan(sx) | np.isnan(sy))
        near |= ~(np.isfinite(dx) & np.isfinite(dy))         # (where the first-order bound itself has no value, nothing is pinned)
    if fmt_index:
        v = np.frombuffer(got, np.int32)
        assert v.size == n and ((v >= -1) & (v < W * H)).all(), (what, "an index outside the source")
        with np.errstate(invalid="ignore"):
            idx = js_round(np.where(cov, sy, 0)) * W + js_round(np.where(cov, sx, 0))
            want = np.where(cov & (idx >= 0) & (idx < W * H), idx, -1).astype(np.int32)
            tie = (np.abs(sx - np.floor(sx) - 0.5) <= dx) | (np.abs(sy - np.floor(sy) - 0.5) <= dy)
        bad = (v != want) & ~near & ~tie
        assert not bad.any(), (what, "index", int(bad.sum()), np.flatnonzero(bad)[:4], v[bad][:4], want[bad][:4])
        excused = int((near & ((v >= 0) != cov)).sum())
    else:
        v = np.frombuffer(got, np.float32).reshape(-1, 2)
        nanp = np.frombuffer(got, np.uint32).reshape(-1, 2) == NANP
        gcov = ~nanp[:, 0]
        assert v.shape[0] == n and (nanp[:, 0] == nanp[:, 1]).all() and not np.isnan(v[gcov]).any(), (what, "an invalid position is the NaN pattern in both words")
        bad = (gcov != cov) & ~near
        assert not bad.any(), (what, "coverage", int(bad.sum()), np.flatnonzero(bad)[:4])
        m = gcov & cov & np.isfinite(dx) & np.isfinite(dy)
        _note(v[m, 0], sx[m], dx[m]); _note(v[m, 1], sy[m], dy[m])
        okx = _f32_between(v[m, 0], (sx[m] - dx[m]), (sx[m] + dx[m]))
        oky = _f32_between(v[m, 1], (sy[m] - dy[m]), (sy[m] + dy[m]))
        assert okx.all() and oky.all(), (what, "coords", int((~okx).sum() + (~oky).sum()), v[m][~(okx & oky)][:4], sx[m][~(okx & oky)][:4], sy[m][~(okx & oky)][:4])
        excused = int((near & (gcov != cov)).sum())
    EXCUSED[0] += excused
    assert excused <= max(cap * n, 0) or W is None, (what, "excused positions", excused, n)
    return excused


def check_field_frame(got, rec, g, W, H, surface, scale, u0, v0, fmt_index, what):
    U, V = window_positions(g)
    return check_to_source(got, rec, surface, scale, u0, v0, U, V, W, H, fmt_index, what)


# ------------------------------------------------------------------------------------------------ the fixtures both test files use
SRC_W, SRC_H = 180, 120
CANVAS = (140.0, 13.37, 7.77)                # scale, u0, v0: nothing lands on an integer


def cameras(n, distort, W=SRC_W, H=SRC_H):
    """n cameras that differ per frame: generic rotations fanned over yaw (no axis-aligned one, where sx would be exactly 0 on a whole column),
    unequal focal lengths, principal points off the centre, with or without lens terms."""
    recs = []
    for k in range(n):
        R = rot(0.35 * k - 0.8 + 0.013, 0.11 - 0.07 * k, 0.05 * k - 0.1)
        f = 150.0 + 7.0 * k
        dist = (-0.12 + 0.01 * k, 0.03, 0.001, -0.0015, 0.002) if distort else None
        recs.append(pack_record(R, f, f * 1.02, 90.3 + 0.21 * k, 60.7 - 0.17 * k, dist, W, H))
    return np.stack(recs)


def windows(band):
    """Windows around the 256-column piece and the band of `band` rows, with negative and large offsets and an empty one."""
    return [(-3, -2, 1, 1), (5, 7, 3, band - 1), (-100, -50, 255, band), (-120, -40, 256, band + 1), (-130, -45, 257, 1), (-300, -20, 513, band + 1),
            (0, 0, 0, 4)]


def near_count(rec, g, W, H, surface, scale, u0, v0):
    """How many pixels of a window the model itself puts within delta of a coverage bound (the CPU check that fixtures stay under the cap)."""
    U, V = (a.ravel() for a in window_positions(g))
    sx, sy, cz, r2 = to_source(rec, surface, scale, u0, v0, U, V, LD)
    dx, dy, dcz, dr2 = delta(rec, surface, scale, u0, v0, U, V)
    with np.errstate(invalid="ignore"):
        near = (np.abs(cz) <= dcz) | (np.abs(r2 - rec[R2MAX]) <= dr2) | (np.abs(sx) <= dx) | (np.abs(sx - W) <= dx) | (np.abs(sy) <= dy) | (np.abs(sy - H) <= dy)
    return int(near.sum())


