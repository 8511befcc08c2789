"""Numpy model of the anisotropic remap (include/hgwarp.h, hg_remap_aniso_frames_device).  Test infrastructure only.  One np.float32
operation per step the header writes (numpy does not fuse); the level choice, the per-level sample and the pyramids are those of
tests/hgtest/trilinear.py.

    steps                  (dx, dy, q) to the horizontal or the vertical neighbour of every pixel of a frame
    probe_plan             (mx, my, N, q') of every pixel: the major step, the probe count, the footprint the level is chosen from
    remap_aniso            one frame; aniso_frames: frame f reads pyramid f % n_planes"""
import numpy as np

from . import trilinear as TM

F32 = np.float32


def steps(co, fin, axis):
    """The step to the neighbour along axis (1: horizontal, 0: vertical): the next pixel if it exists and is finite, else the previous one
    under the same conditions, else none (all three 0)."""
    h, w, _ = co.shape
    nxt, prv = np.roll(co, -1, axis), np.roll(co, 1, axis)
    idx = np.arange(w)[None, :] if axis == 1 else np.arange(h)[:, None]
    n = co.shape[axis]
    a_ok = (idx + 1 < n) & np.roll(fin, -1, axis)
    b_ok = (idx >= 1) & np.roll(fin, 1, axis)
    nb = np.where(a_ok[..., None], nxt, prv)
    with np.errstate(all="ignore"):
        dx = nb[..., 0] - co[..., 0]
        dy = nb[..., 1] - co[..., 1]
        xx = dx * dx
        yy = dy * dy
        q = xx + yy
    assert q.dtype == F32 and dx.dtype == F32
    ok = a_ok | b_ok
    return np.where(ok, dx, F32(0)), np.where(ok, dy, F32(0)), np.where(ok, q, F32(0))


def probe_count(qM, qm, max_aniso):
    """Step 4: N of every pixel from the major and minor squared steps."""
    qM, qm = np.asarray(qM, F32), np.asarray(qm, F32)
    with np.errstate(all="ignore"):
        wants = (qM > F32(1)) & np.isfinite(qM)
        qmc = np.maximum(qm, F32(1))
        N = np.full(qM.shape, max_aniso, np.int32)
        for n in range(max_aniso, 0, -1):                      # descending: the smallest n that suffices is written last
            lhs = F32(n * n) * qmc
            assert lhs.dtype == F32
            N = np.where(lhs >= qM, n, N)
    return np.where(wants, N, 1).astype(np.int32)


def probe_plan(co, max_aniso):
    """co: (h, w, 2) float32.  (mx, my, N, q') per pixel (meaningless where the pixel itself is not finite)."""
    co = np.asarray(co, F32)
    fin = np.isfinite(co[..., 0]) & np.isfinite(co[..., 1])
    hx, hy, qh = steps(co, fin, 1)
    vx, vy, qv = steps(co, fin, 0)
    hmaj = qh >= qv
    mx, my = np.where(hmaj, hx, vx), np.where(hmaj, hy, vy)
    qM, qm = np.where(hmaj, qh, qv), np.where(hmaj, qv, qh)
    N = probe_count(qM, qm, max_aniso)
    with np.errstate(all="ignore"):
        q = qM / (N * N).astype(F32)
    assert q.dtype == F32
    return mx, my, N, q


def remap_aniso(co, pyr, max_aniso):
    """co: (h, w, 2) float32; pyr: TM.pyramid() of the (H, W, C) plane.  Returns (h * w, C) of the plane's type."""
    assert 1 <= max_aniso <= 16
    co = np.asarray(co, F32)
    h, w, _ = co.shape
    levels, C = len(pyr), pyr[0].shape[2]
    flat = co.reshape(-1, 2)
    fin = np.isfinite(flat[:, 0]) & np.isfinite(flat[:, 1])
    mx, my, N, q = (a.reshape(-1) for a in probe_plan(co, max_aniso))
    k, two, t = (a.reshape(-1) for a in TM.level_choice(q, levels))
    fN = N.astype(F32)
    acc = np.zeros((h * w, C), F32)
    for p in range(int(N[fin].max()) if fin.any() else 0):
        live = fin & (N > p)
        with np.errstate(all="ignore"):
            o = ((F32(p) + F32(0.5)) / fN) - F32(0.5)
            px = flat[:, 0] + mx * o
            py = flat[:, 1] + my * o
        assert o.dtype == F32 and px.dtype == F32
        pr = np.where((N > 1)[:, None], np.stack([px, py], -1), flat)
        r = np.zeros((h * w, C), F32)
        for L in range(levels):
            m = live & (k == L)
            if m.any():
                r[m] = TM._sample(pr[m], pyr[L], L)
            m = live & two & (k == L - 1)
            if m.any():
                hi = TM._sample(pr[m], pyr[L], L)
                d = hi - r[m]
                r[m] = r[m] + d * t[m][:, None]
        if p == 0:
            acc[live] = r[live]
        else:
            acc[live] = acc[live] + r[live]
    r = np.where(fin[:, None], acc / fN[:, None], F32(0))
    assert r.dtype == F32
    if pyr[0].dtype == np.uint8:
        return np.minimum(F32(255), np.floor(r + F32(0.5))).astype(np.uint8)
    return r


def aniso_frames(geoms, coords, pyrs, max_aniso):
    """coords[f]: (n_px, 2) float32 of frame f = (x_off, y_off, obj_w, obj_h); pyrs: one pyramid per plane.  Per frame (n_px, C)."""
    out = []
    for f, g in enumerate(geoms):
        w, h = max(g[2], 0), max(g[3], 0)
        pyr = pyrs[f % len(pyrs)]
        if w * h == 0:
            out.append(np.zeros((0, pyr[0].shape[2]), pyr[0].dtype))
        else:
            out.append(remap_aniso(np.asarray(coords[f], F32).reshape(h, w, 2), pyr, max_aniso))
    return out
