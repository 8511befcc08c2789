"""Numpy models of the mosaic's exposure entries (include/hgwarp.h: hg_mosaic_overlap_stats_device, hg_mosaic_solve_gains,
hg_mosaic_frames_gain_device).  Test infrastructure only, built on hgtest.mosaic.

    stat_channels          the channels that carry exposure: all, but not the alpha of a 4-channel frame
    overlap_stats          the (F, F, 2) uint64 statistics of a frame list: N_ab and S_ab, exact
    mosaic_gain            hgtest.mosaic.mosaic with one gain per frame: one np.float32 operation per step the header writes
    normal_equations       (A, b, live) of the gain solve in float64
    solve_gains            the reference solve: numpy.linalg.solve in float64 (frames without coverage: 1.0)
    gain_error             Brown & Lowe's error functional at a gain vector"""
import numpy as np

from . import mosaic as MM

F32 = np.float32


def stat_channels(channels):
    return 3 if channels == 4 else channels


def _windows(geoms, canvas):
    """Per live frame: (f, frame slices, canvas slices) of window ∩ canvas."""
    cx, cy, cw, ch = (int(v) for v in canvas)
    for f, g in enumerate(geoms):
        x, y, w, h = (int(v) for v in g)
        if w <= 0 or h <= 0 or cw <= 0 or ch <= 0:
            continue
        x0, x1, y0, y1 = max(x, cx), min(x + w, cx + cw), max(y, cy), min(y + h, cy + ch)
        if x0 >= x1 or y0 >= y1:
            continue
        yield f, (slice(y0 - y, y1 - y), slice(x0 - x, x1 - x)), (slice(y0 - cy, y1 - cy), slice(x0 - cx, x1 - cx))


def overlap_stats(geoms, fields, frames, channels, canvas):
    """stats[a, b] = (N_ab, S_ab): the canvas pixels frames a and b both contribute to, and the sum of a's intensity -- its stat channels
    added up -- over them.  uint8 frames; integers throughout."""
    F = len(geoms)
    cw, ch = max(int(canvas[2]), 0), max(int(canvas[3]), 0)
    cover = np.zeros((F, ch * cw), np.int64)
    value = np.zeros((F, ch * cw), np.int64)
    k = stat_channels(channels)
    for f, fs, cs in _windows(geoms, canvas):
        h, w = int(geoms[f][3]), int(geoms[f][2])
        px = np.asarray(frames[f])
        assert px.dtype == np.uint8
        co = np.asarray(fields[f], F32).reshape(h, w, 2)[fs]
        cov = np.isfinite(co).all(-1)
        v = px.reshape(h, w, channels)[fs][..., :k].astype(np.int64).sum(-1)
        c2, v2 = cover[f].reshape(ch, cw), value[f].reshape(ch, cw)
        c2[cs] = cov
        v2[cs] = np.where(cov, v, 0)
    out = np.zeros((F, F, 2), np.uint64)
    out[..., 0] = cover @ cover.T
    out[..., 1] = value @ cover.T
    return out


def _stored(q, dtype):
    """What LAST and a lone contributor store of q (float32): itself, or the byte min(255, floor(q + 0.5f))."""
    if dtype == np.uint8:
        with np.errstate(all="ignore"):
            r = np.minimum(F32(255), np.floor(q + F32(0.5)))
        assert r.dtype == F32
        return r.astype(np.uint8)
    return q


def mosaic_gain(geoms, fields, frames, W, H, mode, feather, canvas, gains):
    """hgtest.mosaic.mosaic where every p_c on a stat channel is q_c = g_f * p_c (one float32 multiply) before anything else."""
    cx, cy, cw, ch = (int(v) for v in canvas)
    assert cw > 0 and ch > 0
    live = [f for f, g in enumerate(geoms) if g[2] > 0 and g[3] > 0]
    dtype = np.asarray(frames[live[0]]).dtype if live else np.uint8
    C = np.asarray(frames[live[0]]).size // (geoms[live[0]][2] * geoms[live[0]][3]) if live else 1
    k = stat_channels(C)
    out = np.zeros((ch, cw, C), dtype)
    acc = np.zeros((ch, cw, C), F32)
    wsum = np.zeros((ch, cw), F32)
    count = np.zeros((ch, cw), np.int64)
    for f, fs, rect in _windows(geoms, canvas):
        h, w = int(geoms[f][3]), int(geoms[f][2])
        co = np.asarray(fields[f], F32).reshape(h, w, 2)[fs]
        px = np.asarray(frames[f]).reshape(h, w, C)[fs]
        assert px.dtype == dtype
        q = px.astype(F32)
        with np.errstate(all="ignore"):
            q[..., :k] = F32(gains[f]) * q[..., :k]
        assert q.dtype == F32
        one = _stored(q, dtype)
        cover = np.isfinite(co).all(-1)
        if mode == MM.LAST:
            out[rect] = np.where(cover[..., None], one, out[rect])
            wsum[rect] = np.where(cover, F32(1), wsum[rect])
            continue
        wf = MM.feather_weight(np.where(cover[..., None], co, F32(0)), W, H, feather) if mode == MM.FEATHER else np.ones(cover.shape, F32)
        with np.errstate(all="ignore"):
            prod = wf[..., None] * q
            nacc = acc[rect] + prod
            nsum = wsum[rect] + wf
        assert nacc.dtype == F32 and nsum.dtype == F32
        out[rect] = np.where((cover & (count[rect] == 0))[..., None], one, out[rect])
        acc[rect] = np.where(cover[..., None], nacc, acc[rect])
        wsum[rect] = np.where(cover, nsum, wsum[rect])
        count[rect] += cover
    if mode != MM.LAST:
        with np.errstate(all="ignore"):
            r = acc / wsum[..., None]
            if dtype == np.uint8:
                r = np.minimum(F32(255), np.floor(r + F32(0.5)))
        assert r.dtype == F32
        many = (count > 1)[..., None]
        out = np.where(many, np.where(many, r, F32(0)).astype(dtype), out)
    return out, wsum


def _means(stats, channels):
    st = np.asarray(stats, np.uint64).reshape(-1).reshape(int(round((np.asarray(stats).size // 2) ** 0.5)), -1, 2)
    N = st[..., 0].astype(np.float64)
    with np.errstate(all="ignore"):
        mean = np.where(N > 0, st[..., 1].astype(np.float64) / (stat_channels(channels) * N), 0.0)
    return N, mean


def normal_equations(stats, channels, sigma_n, sigma_g):
    """(A, b, live): the system over the frames with N_aa > 0 (their indices in `live`), float64."""
    N, mean = _means(stats, channels)
    live = np.flatnonzero(np.diag(N) > 0)
    N, mean = N[np.ix_(live, live)], mean[np.ix_(live, live)]
    alpha, beta = 1.0 / sigma_n ** 2, 1.0 / sigma_g ** 2
    off = ~np.eye(len(live), dtype=bool)
    A = np.where(off, -2.0 * alpha * N * mean * mean.T, 0.0)
    A[np.diag_indices(len(live))] = beta * N.sum(1) + 2.0 * alpha * (np.where(off, N * mean * mean, 0.0)).sum(1)
    return A, beta * N.sum(1), live


def solve_gains(stats, channels, sigma_n, sigma_g):
    """The reference: float64 gains, 1.0 for a frame that covers nothing."""
    A, b, live = normal_equations(stats, channels, sigma_n, sigma_g)
    g = np.ones(int(round((np.asarray(stats).size // 2) ** 0.5)), np.float64)
    if len(live):
        g[live] = np.linalg.solve(A, b)
    return g


def gain_error(stats, channels, sigma_n, sigma_g, gains):
    """1/2 sum_a sum_b N_ab [ (g_a I_ab - g_b I_ba)^2 / sigma_n^2 [a != b] + (1 - g_a)^2 / sigma_g^2 ] in float64."""
    N, mean = _means(stats, channels)
    g = np.asarray(gains, np.float64)
    off = ~np.eye(len(g), dtype=bool)
    d = g[:, None] * mean - g[None, :] * mean.T
    return 0.5 * float((N * (np.where(off, d * d, 0.0) / sigma_n ** 2 + ((1.0 - g) ** 2)[:, None] / sigma_g ** 2)).sum())
