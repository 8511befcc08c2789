"""Numpy model of the multi-band mosaic (include/hgwarp.h, hg_mosaic_multiband_device) and of its work area (hg_mosaic_multiband_layout).
Test infrastructure only, built on hgtest.mosaic.  One np.float32 operation per step the header writes (numpy does not fuse); the arrays of
a frame live on its own grid and are 0.0f outside it, which the model gets by padding with zeros.

    grids                  per frame its level-0 grid (x, y, width, height) in canvas-relative coordinates, or None if it takes no part
    labels                 step 1: the label map (int32) and, per taking-part frame, where it contributes on its grid
    reduce / expand        steps 4 and 5 on one array (rows, columns[, channels])
    multiband              (canvas pixels (h, w, C), weight plane (h, w) float32, labels (h, w) int32) of a frame list
    layout                 the parts of the work area in their order, each 256-byte aligned, and the total"""
import numpy as np

from . import mosaic as MM

F32 = np.float32
MAX_BANDS = 8


def stat_channels(channels):
    return 3 if channels == 4 else channels


def _cdiv(a, b):
    return -((-a) // b)


def grids(geoms, canvas, n_bands):
    A = 1 << (n_bands - 1)
    cx, cy, cw, ch = (int(v) for v in canvas)
    out = []
    for g in geoms:
        x, y, w, h = (int(v) for v in g)
        a0, a1, b0, b1 = max(x, cx) - cx, min(x + w, cx + cw) - cx, max(y, cy) - cy, min(y + h, cy + ch) - cy
        if w <= 0 or h <= 0 or cw <= 0 or ch <= 0 or a0 >= a1 or b0 >= b1:
            out.append(None)
            continue
        gx, gy = A * (a0 // A - 1), A * (b0 // A - 1)
        out.append((gx, gy, A * (_cdiv(a1, A) + 1) - gx, A * (_cdiv(b1, A) + 1) - gy))
    return out


def canvas_grid(canvas, n_bands):
    """(width, height) of level 0 of the canvas grid; its origin is (-A, -A)."""
    A = 1 << (n_bands - 1)
    return A * _cdiv(int(canvas[2]), A) + 2 * A, A * _cdiv(int(canvas[3]), A) + 2 * A


def _window(g, canvas):
    """(frame slices, canvas slices) of window ∩ canvas of a taking-part frame."""
    cx, cy, cw, ch = (int(v) for v in canvas)
    x, y, w, h = (int(v) for v in g)
    x0, x1, y0, y1 = max(x, cx), min(x + w, cx + cw), max(y, cy), min(y + h, cy + ch)
    return (slice(y0 - y, y1 - y), slice(x0 - x, x1 - x)), (slice(y0 - cy, y1 - cy), slice(x0 - cx, x1 - cx))


def labels(geoms, fields, W, H, feather, canvas):
    """Step 1.  (label map (ch, cw) int32, cover[f]: bool (ch, cw) where frame f contributes)."""
    cw, ch = int(canvas[2]), int(canvas[3])
    label = np.full((ch, cw), -1, np.int32)
    best = np.zeros((ch, cw), F32)                                 # every rank is >= 2^-10
    covers = []
    for f, g in enumerate(geoms):
        cov = np.zeros((ch, cw), bool)
        covers.append(cov)
        if grids([g], canvas, 1)[0] is None:
            continue
        fs, cs = _window(g, canvas)
        co = np.asarray(fields[f], F32).reshape(int(g[3]), int(g[2]), 2)[fs]
        c = np.isfinite(co).all(-1)
        rank = MM.feather_weight(np.where(c[..., None], co, F32(0)), W, H, feather)
        cov[cs] = c
        win = c & (rank > best[cs])                                # strictly larger: the lowest f among equals stays
        label[cs] = np.where(win, f, label[cs])
        best[cs] = np.where(win, rank, best[cs])
    return label, covers


def _pad(a, n):
    return np.pad(a, [(n, n), (n, n)] + [(0, 0)] * (a.ndim - 2))


def reduce(a):
    """Step 4: level k + 1 (rows / 2, columns / 2) of level k; rows and columns are even."""
    h, w = a.shape[:2]
    assert h % 2 == 0 and w % 2 == 0 and a.dtype == F32
    p = _pad(a, 2)
    t = [p[:, i:i + w:2] for i in range(5)]
    with np.errstate(all="ignore"):
        r = ((t[0] + t[4]) + (t[1] + t[3]) * F32(4)) + t[2] * F32(6)
        s = [r[j:j + h:2] for j in range(5)]
        out = (((s[0] + s[4]) + (s[1] + s[3]) * F32(4)) + s[2] * F32(6)) * F32(0.00390625)
    assert out.dtype == F32 and out.shape[:2] == (h // 2, w // 2)
    return out


def _expand_axis(p, n):
    """The 1-D rule along axis 0 of p, which is T padded by one zero on both sides: 2 n results."""
    out = np.empty((2 * n,) + p.shape[1:], F32)
    with np.errstate(all="ignore"):
        out[0::2] = ((p[0:n] + p[2:n + 2]) + p[1:n + 1] * F32(6)) * F32(0.125)
        out[1::2] = (p[1:n + 1] + p[2:n + 2]) * F32(0.5)
    return out


def expand(t):
    """Step 5: the expansion of level k + 1 at every position of level k (2 rows x 2 columns)."""
    assert t.dtype == F32
    h, w = t.shape[:2]
    p = _pad(t, 1)
    hor = np.swapaxes(_expand_axis(np.swapaxes(p, 0, 1), w), 0, 1)        # horizontally, on every row (the padding rows give 0.0f)
    return _expand_axis(hor, h)


def multiband(geoms, fields, frames, W, H, feather, n_bands, canvas, gains=None, like=(np.uint8, 1)):
    """geoms, fields, frames, W, H, canvas as hgtest.mosaic.mosaic takes them; gains: one per frame or None; like: the (dtype, channels) of
    the canvas when no frame has a pixel."""
    L = int(n_bands)
    assert 1 <= L <= MAX_BANDS
    A = 1 << (L - 1)
    cx, cy, cw, ch = (int(v) for v in canvas)
    assert cw > 0 and ch > 0
    live = [f for f, g in enumerate(geoms) if g[2] > 0 and g[3] > 0]
    dtype = np.asarray(frames[live[0]]).dtype if live else np.dtype(like[0])
    C = np.asarray(frames[live[0]]).size // (int(geoms[live[0]][2]) * int(geoms[live[0]][3])) if live else like[1]
    k_stat = stat_channels(C)
    label, covers = labels(geoms, fields, W, H, feather, canvas)
    gr = grids(geoms, canvas, L)
    part = [f for f, g in enumerate(gr) if g is not None]
    # steps 2-4: the pyramids of every frame, on its grid
    I, M = {}, {}
    for f in part:
        gx, gy, gw, gh = gr[f]
        fs, cs = _window(geoms[f], canvas)
        px = np.asarray(frames[f]).reshape(int(geoms[f][3]), int(geoms[f][2]), C)[fs]
        assert px.dtype == dtype
        q = px.astype(F32)
        with np.errstate(all="ignore"):
            q[..., :k_stat] = F32(1.0 if gains is None else gains[f]) * q[..., :k_stat]
        i0 = np.zeros((gh, gw, C), F32)
        m0 = np.zeros((gh, gw), F32)
        gs = (slice(cs[0].start - gy, cs[0].stop - gy), slice(cs[1].start - gx, cs[1].stop - gx))
        i0[gs] = np.where(covers[f][cs][..., None], q, F32(0))
        m0[gs] = np.where(label[cs] == f, F32(1), F32(0))
        I[f], M[f] = [i0], [m0]
        for k in range(1, L):
            I[f].append(reduce(I[f][-1]))
            M[f].append(reduce(M[f][-1]))
    # step 6: blend and collapse, coarse to fine, on the canvas grid
    pw, ph = canvas_grid(canvas, L)
    R = None
    for k in range(L - 1, -1, -1):
        num = np.zeros((ph >> k, pw >> k, C), F32)
        den = np.zeros((ph >> k, pw >> k), F32)
        for f in part:
            gx, gy, gw, gh = gr[f]
            rect = (slice((gy + A) >> k, (gy + A + gh) >> k), slice((gx + A) >> k, (gx + A + gw) >> k))
            w = M[f][k]
            with np.errstate(all="ignore"):
                lap = I[f][k] - expand(I[f][k + 1]) if k < L - 1 else I[f][k]
                nnum = num[rect] + w[..., None] * lap
                nden = den[rect] + w
            assert nnum.dtype == F32 and nden.dtype == F32
            on = w != F32(0)
            num[rect] = np.where(on[..., None], nnum, num[rect])
            den[rect] = np.where(on, nden, den[rect])
        with np.errstate(all="ignore"):
            B = np.where((den > 0)[..., None], num / np.where(den > 0, den, F32(1))[..., None], F32(0))
            R = B + expand(R) if k < L - 1 else B
        assert R.dtype == F32
    # step 7
    r = R[A:A + ch, A:A + cw]
    has = label >= 0
    if dtype == np.uint8:
        with np.errstate(all="ignore"):
            r = np.minimum(F32(255), np.maximum(F32(0), np.floor(r + F32(0.5))))
    out = np.where(has[..., None], r, F32(0)).astype(dtype)
    return out, has.astype(F32), label


def _pad256(n):
    return (n + 255) // 256 * 256


def layout(geoms, canvas, channels, n_bands):
    """(parts, total): parts is a list of (name, offset, bytes) in the order of the work area: 'labels'; ('flags', f) per taking-part frame;
    per taking-part frame and level k = 1..L-1 ('I', f, k) then ('M', f, k); ('R', k) for k = 1..L-1.  An empty canvas needs nothing."""
    L = int(n_bands)
    cw, ch = int(canvas[2]), int(canvas[3])
    if cw <= 0 or ch <= 0:
        return [], 0
    parts, off = [], 0

    def add(name, n):
        nonlocal off
        parts.append((name, off, n))
        off += _pad256(n)

    add("labels", cw * ch * 4)
    gr = grids(geoms, canvas, L)
    for f, g in enumerate(gr):
        if g is not None:
            add(("flags", f), g[2] * g[3])
    for f, g in enumerate(gr):
        if g is None:
            continue
        for k in range(1, L):
            n = (g[2] >> k) * (g[3] >> k)
            add(("I", f, k), n * channels * 4)
            add(("M", f, k), n * 4)
    pw, ph = canvas_grid(canvas, L)
    for k in range(1, L):
        add(("R", k), (pw >> k) * (ph >> k) * channels * 4)
    return parts, off
