"""Numpy model of the thin-plate splines (include/hgwarp.h, "thin-plate splines"), written from the header text.  Test infrastructure only.

    solve(frm, to, lam)          the record (16 + 4 N doubles) and the status of one frame: the header's normalisation, system and partial-pivot
                                 elimination (largest magnitude, lowest row among equals), so the statuses follow the stated rule
    evaluate(rec, X, Y, dtype)   the spline of a record at positions, in float64 or np.longdouble
    delta(rec, X, Y)             the header-independent evaluation tolerance of the issue: (N + 16) 2^-52 (sum |w| q (|log q| + 1) + |a0| +
                                 |a1 x'| + |a2 y'| + |t|), per axis
    residual(rec, frm, to)       max_i |spline(from_i) - to_i| in longdouble (the solve's metric at lambda = 0)
    system_residual(...)         the largest residual of the linear system itself (the metric at lambda > 0)
    nodes / blend                the lattice of a stepped field and the blend of four nodes, as the header writes them
    field_values                 coverage and storage of evaluated positions by the rules of the other fields (hgtest.field)"""
import numpy as np

from . import field as FM

F64, LD = np.float64, np.longdouble
OK, SINGULAR, BAD_INPUT = 0, 1, 2
HEAD = 16
NAN64 = np.uint64(0x7FF8000000000000)


def record_doubles(n):
    return HEAD + 4 * n


def failed_record(n):
    return np.full(record_doubles(n), NAN64, np.uint64).view(F64)


def _seq_sum(v):
    """The sum in index order."""
    return np.cumsum(np.asarray(v, F64))[-1]


def normalise(frm, to):
    frm = np.asarray(frm, np.float32).reshape(-1, 2).astype(F64)
    to = np.asarray(to, np.float32).reshape(-1, 2).astype(F64)
    n = frm.shape[0]
    c = np.array([_seq_sum(frm[:, 0]) / n, _seq_sum(frm[:, 1]) / n])
    t = np.array([_seq_sum(to[:, 0]) / n, _seq_sum(to[:, 1]) / n])
    a = frm - c
    md = _seq_sum(np.sqrt(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1])) / n
    return frm, to, c, t, md


def U(q):
    q = np.asarray(q)
    with np.errstate(all="ignore"):
        return q * np.log(np.where(q > 0, q, q.dtype.type(1)))


def system(d, lam):
    n = d.shape[0]
    ex = d[:, None, 0] - d[None, :, 0]
    ey = d[:, None, 1] - d[None, :, 1]
    A = np.zeros((n + 3, n + 3), F64)
    A[:n, :n] = U(ex * ex + ey * ey)
    A[np.arange(n), np.arange(n)] = lam
    A[:n, n] = 1.0
    A[:n, n + 1:] = d
    A[n:, :n] = A[:n, n:].T
    return A


def eliminate(A, B):
    """Gaussian elimination with partial pivoting as the header states it, on copies.  Returns (solution (M, 2), ok)."""
    A, B = A.copy(), B.copy()
    M = A.shape[0]
    with np.errstate(all="ignore"):
        for k in range(M):
            mag = np.abs(A[k:, k])
            mag = np.where(np.isnan(mag), -1.0, mag)
            p = k + int(np.argmax(mag))                      # (argmax: the first of equals, the lowest row)
            piv = A[p, k]
            if not (abs(piv) > 0.0) or not np.isfinite(piv):
                return None, False
            if p != k:
                A[[k, p]] = A[[p, k]]
                B[[k, p]] = B[[p, k]]
            f = A[k + 1:, k] / piv
            A[k + 1:, k + 1:] = A[k + 1:, k + 1:] - f[:, None] * A[k, k + 1:][None, :]
            B[k + 1:] = B[k + 1:] - f[:, None] * B[k][None, :]
        for k in range(M - 1, -1, -1):
            B[k] = B[k] / A[k, k]
            B[:k] = B[:k] - A[:k, k][:, None] * B[k][None, :]
    return B, bool(np.isfinite(B).all())


def solve(frm, to, lam=0.0):
    """(record, status) of one frame."""
    f32 = np.asarray(frm, np.float32).ravel()
    t32 = np.asarray(to, np.float32).ravel()
    n = f32.size // 2
    if not (np.isfinite(f32).all() and np.isfinite(t32).all()):
        return failed_record(n), BAD_INPUT
    frm, to, c, t, md = normalise(f32, t32)
    if not (md > 0.0) or not np.isfinite(md):
        return failed_record(n), SINGULAR
    s = np.sqrt(2.0) / md
    d = (frm - c) * s
    B = np.zeros((n + 3, 2), F64)
    B[:n] = to - t
    x, ok = eliminate(system(d, float(lam)), B)
    if not ok:
        return failed_record(n), SINGULAR
    rec = np.zeros(record_doubles(n), F64)
    rec[0:2], rec[2], rec[3:5] = c, s, t
    rec[8:14] = x[n:].ravel()                                # a0x a0y a1x a1y a2x a2y
    pts = rec[HEAD:].reshape(n, 4)
    pts[:, 0:2] = d
    pts[:, 2:4] = x[:n]
    return rec, OK


def _parts(rec, X, Y, dtype):
    rec = np.asarray(rec, F64).astype(dtype)
    n = (rec.size - HEAD) // 4
    pts = rec[HEAD:].reshape(n, 4)
    X, Y = np.asarray(X, F64).astype(dtype), np.asarray(Y, F64).astype(dtype)
    xn, yn = (X - rec[0]) * rec[2], (Y - rec[1]) * rec[2]
    return rec, pts, xn, yn


def evaluate(rec, X, Y, dtype=F64):
    """(sx, sy) at from-space positions (any shape), the sum in index order."""
    rec, pts, xn, yn = _parts(rec, X, Y, dtype)
    ax, ay = np.zeros(xn.shape, dtype), np.zeros(xn.shape, dtype)
    with np.errstate(all="ignore"):
        for dx, dy, wx, wy in pts:
            ex, ey = xn - dx, yn - dy
            u = U(ex * ex + ey * ey)
            ax = ax + wx * u
            ay = ay + wy * u
        sx = rec[3] + (((rec[8] + rec[10] * xn) + rec[12] * yn) + ax)
        sy = rec[4] + (((rec[9] + rec[11] * xn) + rec[13] * yn) + ay)
    return sx, sy


def delta(rec, X, Y):
    """(dx, dy): the tolerance of an evaluation in float64 from a given record, any summation order, any logarithm good to a few ulp."""
    rec, pts, xn, yn = _parts(rec, X, Y, F64)
    n = pts.shape[0]
    mx, my = np.zeros(xn.shape), np.zeros(xn.shape)
    with np.errstate(all="ignore"):
        for dx, dy, wx, wy in pts:
            ex, ey = xn - dx, yn - dy
            q = ex * ex + ey * ey
            g = q * (np.abs(np.log(np.where(q > 0, q, 1.0))) + 1.0)
            mx = mx + abs(wx) * g
            my = my + abs(wy) * g
        mx = mx + abs(rec[8]) + np.abs(rec[10] * xn) + np.abs(rec[12] * yn) + abs(rec[3])
        my = my + abs(rec[9]) + np.abs(rec[11] * xn) + np.abs(rec[13] * yn) + abs(rec[4])
    k = (n + 16) * 2.0 ** -52
    return k * mx, k * my


def residual(rec, frm, to):
    """max_i |spline(from_i) - to_i| in px, evaluated in longdouble."""
    frm = np.asarray(frm, np.float32).reshape(-1, 2).astype(F64)
    to = np.asarray(to, np.float32).reshape(-1, 2).astype(LD)
    sx, sy = evaluate(rec, frm[:, 0], frm[:, 1], LD)
    return float(np.max(np.hypot(sx - to[:, 0], sy - to[:, 1])))


def system_residual(rec, frm, to, lam):
    """The largest |row of [[K + lam I, P], [P^T, 0]] [w; a] - [b; 0]| over both right-hand sides, in longdouble, with the record's own d, c, s and t."""
    rec = np.asarray(rec, F64)
    n = (rec.size - HEAD) // 4
    pts = rec[HEAD:].reshape(n, 4)
    to = np.asarray(to, np.float32).reshape(-1, 2).astype(LD)
    A = system(pts[:, 0:2].copy(), 0.0).astype(LD)
    d = pts[:, 0:2].astype(LD)
    ex, ey = d[:, None, 0] - d[None, :, 0], d[:, None, 1] - d[None, :, 1]
    A[:n, :n] = U(ex * ex + ey * ey)
    A[np.arange(n), np.arange(n)] = LD(lam)
    x = np.concatenate([pts[:, 2:4], rec[8:14].reshape(3, 2)]).astype(LD)
    b = np.zeros((n + 3, 2), LD)
    b[:n] = to - rec[3:5].astype(LD)
    return float(np.max(np.abs(A @ x - b)))


def nodes(n, step):
    return max(2, (n + step - 2) // step + 1)


def blend(n00, n01, n10, n11, fx, fy):
    with np.errstate(all="ignore"):
        return (n00 * (1.0 - fx) + n01 * fx) * (1.0 - fy) + (n10 * (1.0 - fx) + n11 * fx) * fy


def lattice_cells(w, h, step):
    """Per pixel of a w x h window: (ky, kx, fy, fx, on_node) of the stepped field."""
    c, r = np.meshgrid(np.arange(w), np.arange(h))
    kx = np.minimum(c // step, nodes(w, step) - 2)
    ky = np.minimum(r // step, nodes(h, step) - 2)
    fx = (c - kx * step) / float(step)
    fy = (r - ky * step) / float(step)
    return ky, kx, fy, fx, (c % step == 0) & (r % step == 0)


def blend_nodes(nd, w, h, step):
    """nd: (nodes_y, nodes_x) float64 of one axis -> the (h, w) pixels the header defines."""
    ky, kx, fy, fx, on = lattice_cells(w, h, step)
    v = blend(nd[ky, kx], nd[ky, kx + 1], nd[ky + 1, kx], nd[ky + 1, kx + 1], fx, fy)
    c, r = np.meshgrid(np.arange(w), np.arange(h))
    return np.where(on, nd[np.minimum(r // step, nd.shape[0] - 1), np.minimum(c // step, nd.shape[1] - 1)], v)


def window_positions(g):
    x_off, y_off, w, h = g
    c, r = np.meshgrid(np.arange(max(w, 0)), np.arange(max(h, 0)))
    return (c + x_off).astype(F64), (r + y_off).astype(F64)


def field_values(sx, sy, W, H, fmt_index):
    """The stored field of evaluated positions: int32 indices or float32 pairs, flat in row order."""
    sx, sy = np.asarray(sx, F64).ravel(), np.asarray(sy, F64).ravel()
    valid = np.ones(sx.shape, bool)
    return FM.index_field(sx, sy, valid, W, H) if fmt_index else FM.coords_field(sx, sy, valid, W, H)


# ------------------------------------------------------------------------------------------------ the checks both test files make
def pack256(geoms, px):
    """(offsets, total) of windows packed at the 256-byte grain."""
    offs, off = [], 0
    for g in geoms:
        offs.append(off)
        if g[2] > 0 and g[3] > 0:
            off += (g[2] * g[3] * px + 255) // 256 * 256
    return offs, off


def solve_base(frm, to, lam):
    """(model record, status, base): the metric of the model's own float64 solve -- the interpolation residual at lambda == 0, else the residual of
    the linear system."""
    rec, st = solve(frm, to, lam)
    if st != OK:
        return rec, st, None
    return rec, st, (residual(rec, frm, to) if lam == 0 else system_residual(rec, frm, to, lam))


def check_record(got, status, frm, to, lam, floor, what):
    """One frame's record and status against the model: the status exactly, the normalisation bit for bit (the same IEEE operations in the same
    order), the coefficients by the metric, which may reach 16 x the model's own (floor: what replaces a base of 0).  Returns metric / base."""
    want, st, base = solve_base(frm, to, lam)
    assert status == st, (what, "status", int(status), st)
    if st != OK:
        assert (np.asarray(got).view(np.uint64) == NAN64).all(), (what, "a failed frame's record is all NaN")
        return 0.0
    assert np.array_equal(got[:8].view(np.uint64), want[:8].view(np.uint64)) and (got[14:16] == 0).all(), (what, "normalisation", got[:8], want[:8])
    n = (got.size - HEAD) // 4
    assert np.array_equal(got[HEAD:].reshape(n, 4)[:, :2].view(np.uint64), want[HEAD:].reshape(n, 4)[:, :2].view(np.uint64)), (what, "d")
    base = base if base > 0 else floor
    m = residual(got, frm, to) if lam == 0 else system_residual(got, frm, to, lam)
    assert m <= 16 * base, (what, "metric", m, "base", base)
    return m / base


def _f32_between(v, lo, hi):
    with np.errstate(over="ignore"):
        return (v >= lo.astype(np.float32)) & (v <= hi.astype(np.float32))


def check_values(got, sx, sy, dx, dy, W, H, fmt_index, what):
    """A stored field (flat bytes) against positions' values (sx, sy) known to (dx, dy): the coverage decision may differ only where a value
    lies within its tolerance of a bound; a covered coordinate lies between float32(v - d) and float32(v + d); an index equals the model's
    unless a value lies within its tolerance of a rounding tie."""
    sx, sy, dx, dy = (np.asarray(a, F64).ravel() for a in (sx, sy, dx, dy))
    with np.errstate(invalid="ignore"):
        near = (np.abs(sx) <= dx) | (np.abs(sx - W) <= dx) | (np.abs(sy) <= dy) | (np.abs(sy - H) <= dy)
        cov = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    if fmt_index:
        v = np.frombuffer(got, np.int32)
        want = field_values(sx, sy, W, H, True)
        with np.errstate(invalid="ignore"):
            tie = (np.abs(sx - np.floor(sx) - 0.5) <= dx) | (np.abs(sy - np.floor(sy) - 0.5) <= dy)
        bad = (v != want) & ~near & ~tie
        assert not bad.any(), (what, "index", int(bad.sum()), np.flatnonzero(bad)[:4], v[bad][:4], want[bad][:4])
        assert ((v >= -1) & (v < W * H)).all(), (what, "an index outside the source")
        return
    v = np.frombuffer(got, np.float32).reshape(-1, 2)
    nanp = np.frombuffer(got, np.uint32).reshape(-1, 2) == 0x7FC00000
    gcov = ~nanp[:, 0]
    assert (nanp[:, 0] == nanp[:, 1]).all() and not np.isnan(v[gcov]).any(), (what, "an uncovered pixel is the NaN pattern in both words")
    bad = (gcov != cov) & ~near
    assert not bad.any(), (what, "coverage", int(bad.sum()), np.flatnonzero(bad)[:4])
    m = gcov & cov
    okx = _f32_between(v[m, 0], (sx - dx)[m], (sx + dx)[m])
    oky = _f32_between(v[m, 1], (sy - dy)[m], (sy + dy)[m])
    assert okx.all() and oky.all(), (what, "coords", int((~okx).sum() + (~oky).sum()), v[m][~(okx & oky)][:4], sx[m][~(okx & oky)][:4], sy[m][~(okx & oky)][:4])


def check_field_frame(got, rec, ok, g, W, H, fmt_index, what):
    """One frame of a step-1 field against the model's evaluation of the frame's own record."""
    if not ok:
        assert (np.frombuffer(got, np.int32) == -1).all() if fmt_index else (np.frombuffer(got, np.uint32) == 0x7FC00000).all(), (what, "a failed frame")
        return
    X, Y = window_positions(g)
    sx, sy = evaluate(rec, X, Y)
    dx, dy = delta(rec, X, Y)
    check_values(got, sx, sy, dx, dy, W, H, fmt_index, what)


def check_lattice_frame(got, got_step1, nodes_raw, rec, ok, g, W, H, fmt_index, step, what):
    """One frame of a stepped field: the device's own nodes against the model (to delta), every pixel against the model's blend of the device's
    nodes (to the largest delta of its four nodes plus 8 x 2^-53 x the largest |node|), and the pixels on nodes against the step-1 field, bit
    for bit."""
    w, h = g[2], g[3]
    ny, nx = nodes(h, step), nodes(w, step)
    nd = np.frombuffer(nodes_raw, F64, ny * nx * 2).reshape(ny, nx, 2)
    px = 4 if fmt_index else 8
    if not ok:
        assert np.isnan(nd).all(), (what, "a failed frame's nodes")
        assert (np.frombuffer(got, np.int32) == -1).all() if fmt_index else (np.frombuffer(got, np.uint32) == 0x7FC00000).all(), (what, "a failed frame")
        return
    c, r = np.meshgrid(np.arange(nx) * step + g[0], np.arange(ny) * step + g[1])
    X, Y = c.astype(F64), r.astype(F64)
    sx, sy = evaluate(rec, X, Y)
    dx, dy = delta(rec, X, Y)
    assert (np.abs(nd[..., 0] - sx) <= dx).all() and (np.abs(nd[..., 1] - sy) <= dy).all(), (what, "nodes")
    ky, kx, fy, fx, on = lattice_cells(w, h, step)
    bx, by = blend_nodes(nd[..., 0], w, h, step), blend_nodes(nd[..., 1], w, h, step)

    def four(a, red):
        return red(red(a[ky, kx], a[ky, kx + 1]), red(a[ky + 1, kx], a[ky + 1, kx + 1]))
    tx = four(dx, np.maximum) + 8 * 2.0 ** -53 * four(np.abs(nd[..., 0]), np.maximum)
    ty = four(dy, np.maximum) + 8 * 2.0 ** -53 * four(np.abs(nd[..., 1]), np.maximum)
    check_values(got, bx, by, tx, ty, W, H, fmt_index, what)
    a = np.frombuffer(got, np.uint8).reshape(h, w, px)
    b = np.frombuffer(got_step1, np.uint8).reshape(h, w, px)
    assert np.array_equal(a[on], b[on]), (what, "pixels on nodes equal the step-1 field bit for bit")


def check_points_frame(got, rec, ok, pts, what):
    """One frame's point results (n, 2) float32 against the model: the NaN pattern for a position that is not finite and for a failed frame;
    else the value to delta (where the model's own numbers are finite and below 1e30: a position of 1e30 is legal but pins nothing)."""
    p = np.asarray(pts, np.float32).astype(F64)
    fin = np.isfinite(p).all(1) & bool(ok)
    assert (np.ascontiguousarray(got[~fin]).view(np.uint32) == 0x7FC00000).all(), (what, "NaN / NaN")
    if fin.any():
        sx, sy = evaluate(rec, p[fin, 0], p[fin, 1])
        dx, dy = delta(rec, p[fin, 0], p[fin, 1])
        with np.errstate(invalid="ignore"):
            small = np.isfinite(dx) & np.isfinite(dy) & (np.abs(sx) < 1e30) & (np.abs(sy) < 1e30)
        v = got[fin][small]
        assert _f32_between(v[:, 0], (sx - dx)[small], (sx + dx)[small]).all() and _f32_between(v[:, 1], (sy - dy)[small], (sy + dy)[small]).all(), (what, "points")
