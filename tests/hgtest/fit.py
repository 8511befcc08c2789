"""The numpy model of the fitting entries (include/hgwarp.h, "fitting transforms to matches"), written from the header's text: the sample
draw in Python integers, the minimal solve through the host functions whose bits the device solve equals (HG.solve_projective /
HG.solve_affine), the score in float64 with one numpy operation per rounded step, the total order of the best hypothesis, and the
normalised least-squares refit -- in float64 and, for the tolerance of the tests, once more in np.longdouble.  Everything but the refit is
compared bit for bit."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "homography.js_amd"))
import hgwarp as HG                          # noqa: E402

AFFINE, PROJECTIVE = 0, 1
M32 = 0xffffffff
QNAN_BITS = 0x7ff8000000000000
F64 = np.float64


def k_of(kind):
    return 4 if kind == PROJECTIVE else 3


def tile():
    """The scoring kernel's match tile T, read from the constant the shared header exposes."""
    import re
    text = open(os.path.join(ROOT, "homography.js_amd", "csrc", "hg_fit_dev.h")).read()
    return int(re.search(r"constexpr int kFitTile = (\d+);", text).group(1))


# ------------------------------------------------------------------------------------------------ samples
def mix(a):
    a &= M32
    a ^= a >> 16
    a = (a * 0x7feb352d) & M32
    a ^= a >> 15
    a = (a * 0x846ca68b) & M32
    a ^= a >> 16
    return a


def sample(kind, seed, f, h, count):
    """The four slots of hypothesis h of frame f: K distinct indices (-1 in the fourth for affine), or -1 everywhere when invalid."""
    K = k_of(kind)
    if count < K:
        return [-1] * 4
    k = mix(mix(mix((seed + 0x9e3779b9) & M32) + f) + h)
    got = []
    for t in range(16):
        i = (mix((k + t) & M32) * count) >> 32
        if i not in got:
            got.append(i)
            if len(got) == K:
                return got + [-1] * (4 - K)
    return [-1] * 4


def sample_indices(kind, seed, counts, n_hyp):
    return np.array([[sample(kind, seed, f, h, int(c)) for h in range(n_hyp)] for f, c in enumerate(counts)], np.int32).reshape(len(counts), n_hyp, 4)


def sample_ok(kind, idx, count):
    K = k_of(kind)
    ii = [int(v) for v in idx[:K]]
    return all(0 <= v < count for v in ii) and len(set(ii)) == K


# ------------------------------------------------------------------------------------------------ minimal solve, score, best
def minimal(kind, matches, idx):
    """(matrix of 8 doubles, valid) from the K matches idx of one frame's (N, 4) float32 list."""
    K = k_of(kind)
    p = matches[[int(v) for v in idx[:K]]]
    m = np.zeros(8, F64)
    if kind == PROJECTIVE:
        m[:] = HG.solve_projective(p[:, :2].ravel(), p[:, 2:].ravel())
    else:
        m[:6] = HG.solve_affine(p[:, :2].ravel(), p[:, 2:].ravel()).astype(F64)
    return m, bool(np.isfinite(m).all())


def project(kind, M, x, y):
    """apply_projective / apply_affine of hg_math.h for matrices M (H, 8) on points x, y (N,): (H, N) each, one rounding per step."""
    m = [M[:, k:k + 1] for k in range(8)]
    with np.errstate(all="ignore"):
        if kind == PROJECTIVE:
            den = ((m[6] * x) + (m[7] * y)) + 1.0
            return (((m[0] * x) + (m[1] * y)) + m[2]) / den, (((m[3] * x) + (m[4] * y)) + m[5]) / den
        return ((m[0] * x) + (m[2] * y)) + m[4], ((m[1] * x) + (m[3] * y)) + m[5]


def score(kind, M, matches, threshold):
    """(H, N) bool: is match i an inlier of matrix h?  matches = the frame's first counts[f] slots."""
    mt = np.asarray(matches, np.float32).reshape(-1, 4).astype(F64)
    M = np.asarray(M, F64).reshape(-1, 8)
    px, py = project(kind, M, mt[:, 0], mt[:, 1])
    with np.errstate(all="ignore"):
        dx, dy = px - mt[:, 2], py - mt[:, 3]
        e = (dx * dx) + (dy * dy)
        inl = e <= F64(threshold) * F64(threshold)
    return inl & np.isfinite(mt).all(1)


def best(counts, valid):
    """Index of the valid hypothesis with the highest count, the lowest index among equals; -1 without one."""
    bh, bc = -1, -1
    for h, (c, v) in enumerate(zip(counts, valid)):
        if v and c > bc:
            bh, bc = h, int(c)
    return bh


# ------------------------------------------------------------------------------------------------ refit
def gauss(A, n, r):
    """Partial-pivot elimination on the n x (n + r) augmented system, written out (no LAPACK: it must run in longdouble)."""
    A = A.copy()
    with np.errstate(all="ignore"):
        for k in range(n):
            pk = k
            for j in range(k + 1, n):
                if abs(A[pk, k]) < abs(A[j, k]):
                    pk = j
            if pk != k:
                A[[k, pk]] = A[[pk, k]]
            for i in range(k + 1, n):
                l = A[i, k] / A[k, k]
                A[i, k + 1:] = A[i, k + 1:] - l * A[k, k + 1:]
        for c in range(r):
            for i in range(n - 1, -1, -1):
                x = A[i, n + c]
                for j in range(i + 1, n):
                    x = x - A[i, j] * A[j, n + c]
                A[i, n + c] = x / A[i, i]
    return A[:, n:]


def refit(kind, inliers, dtype=F64):
    """The header's least-squares refit over the (n, 4) float32 inliers in `dtype`: 8 values (dtype), possibly not finite."""
    T = dtype
    q = np.asarray(inliers, np.float32).reshape(-1, 4).astype(T)
    n = T(len(q))
    with np.errstate(all="ignore"):
        c = q.sum(0) / n
        a = q - c
        sf = np.sqrt(T(2)) / (np.sqrt(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]).sum() / n)
        st = np.sqrt(T(2)) / (np.sqrt(a[:, 2] * a[:, 2] + a[:, 3] * a[:, 3]).sum() / n)
        x, y, u, v = a[:, 0] * sf, a[:, 1] * sf, a[:, 2] * st, a[:, 3] * st
        xx, xy, yy = x * x, x * y, y * y
        one = np.ones_like(x)
        base = (xx, xy, yy, x, y, one)
        s1 = [b.sum() for b in base]
        su = [(u * b).sum() for b in base]
        sv = [(v * b).sum() for b in base]
        S = np.array([[s1[0], s1[1], s1[3]], [s1[1], s1[2], s1[4]], [s1[3], s1[4], n]], T)
        g = np.zeros(9, T)
        g[8] = 1
        if kind == PROJECTIVE:
            w = u * u + v * v
            sw = [(w * b).sum() for b in base[:5]]
            U = np.array([[su[0], su[1]], [su[1], su[2]], [su[3], su[4]]], T)
            V = np.array([[sv[0], sv[1]], [sv[1], sv[2]], [sv[3], sv[4]]], T)
            A = np.zeros((8, 9), T)
            A[0:3, 0:3] = S
            A[3:6, 3:6] = S
            A[0:3, 6:8], A[6:8, 0:3] = -U, -U.T
            A[3:6, 6:8], A[6:8, 3:6] = -V, -V.T
            A[6:8, 6:8] = [[sw[0], sw[1]], [sw[1], sw[2]]]
            A[:, 8] = [su[3], su[4], su[5], sv[3], sv[4], sv[5], -sw[3], -sw[4]]
            g[:8] = gauss(A, 8, 1)[:, 0]
        else:
            A = np.zeros((3, 5), T)
            A[:, :3] = S
            A[:, 3] = [su[3], su[4], su[5]]
            A[:, 4] = [sv[3], sv[4], sv[5]]
            sol = gauss(A, 3, 2)
            g[0:3], g[3:6] = sol[:, 0], sol[:, 1]
        g = g.reshape(3, 3)
        gt = np.empty((3, 3), T)
        gt[:, 0], gt[:, 1] = g[:, 0] * sf, g[:, 1] * sf
        gt[:, 2] = (g[:, 2] - g[:, 0] * (sf * c[0])) - g[:, 1] * (sf * c[1])
        hm = np.empty((3, 3), T)
        hm[0], hm[1], hm[2] = gt[0] / st + c[2] * gt[2], gt[1] / st + c[3] * gt[2], gt[2]
        if kind == PROJECTIVE:
            return (hm.ravel() / hm[2, 2])[:8]
        return np.array([hm[0, 0], hm[1, 0], hm[0, 1], hm[1, 1], hm[0, 2], hm[1, 2], 0, 0], T)


def corner_displacement(kind, a, b, pts):
    """The refit metric: the largest distance, in pixels, between the images under a and under b of the four corners of pts' bounding box."""
    p = np.asarray(pts, np.longdouble).reshape(-1, 2)
    x = np.array([p[:, 0].min(), p[:, 0].max(), p[:, 0].min(), p[:, 0].max()])
    y = np.array([p[:, 1].min(), p[:, 1].min(), p[:, 1].max(), p[:, 1].max()])
    ax, ay = project(kind, np.asarray(a, np.longdouble).reshape(1, 8), x, y)
    bx, by = project(kind, np.asarray(b, np.longdouble).reshape(1, 8), x, y)
    return float(np.sqrt((ax - bx) ** 2 + (ay - by) ** 2).max())


# ------------------------------------------------------------------------------------------------ the whole call
class Fit:
    """What hg_fit_matches_frames_device leaves behind: mats, min_mats (F, 8) float64; counts, best (F,) int32; mask (F, N) uint8; and for
    the tolerance, refit_ld: per frame the longdouble refit (or None where d_mats is not a refit)."""


def fit(kind, matches, counts, threshold, n_hyp, seed=0, samples=None, refit_on=True):
    matches = np.asarray(matches, np.float32)                  # (F, N, 4)
    assert matches.ndim == 3 and matches.shape[2] == 4
    Fn, N = matches.shape[0], matches.shape[1]
    counts = [N] * Fn if counts is None else [int(c) for c in counts]
    K = k_of(kind)
    r = Fit()
    nan = np.array([QNAN_BITS] * 8, np.uint64).view(F64)
    r.mats, r.min_mats = np.tile(nan, (Fn, 1)), np.tile(nan, (Fn, 1))
    r.counts, r.best = np.zeros(Fn, np.int32), np.full(Fn, -1, np.int32)
    r.mask = np.zeros((Fn, N), np.uint8)
    r.refit_ld = [None] * Fn
    if samples is None and n_hyp:
        samples = sample_indices(kind, seed, counts, n_hyp)
    for f in range(Fn):
        mt = matches[f, :counts[f]]
        if n_hyp == 0:
            inl = np.isfinite(mt.astype(F64)).all(1)
        else:
            M, valid = np.zeros((n_hyp, 8), F64), np.zeros(n_hyp, bool)
            for h in range(n_hyp):
                if sample_ok(kind, samples[f, h], counts[f]):
                    M[h], valid[h] = minimal(kind, mt, samples[f, h])
            sc = score(kind, M, mt, threshold) if counts[f] else np.zeros((n_hyp, 0), bool)
            bh = best(sc.sum(1), valid)
            r.best[f] = bh
            if bh < 0:
                continue
            inl = sc[bh]
            r.min_mats[f] = M[bh]
            r.mats[f] = M[bh]
        r.counts[f] = int(inl.sum())
        r.mask[f, :counts[f]] = inl
        if refit_on and (r.counts[f] >= K if n_hyp == 0 else r.counts[f] > K):
            m = refit(kind, mt[inl])
            if np.isfinite(m).all():
                r.mats[f] = m
                r.refit_ld[f] = refit(kind, mt[inl], np.longdouble)
    return r


# ------------------------------------------------------------------------------------------------ what the CPU and the GPU tests share
F32 = np.float32
W_IMG, H_IMG = 640.0, 480.0
PLANT_H = np.array([1.1, 0.05, 3.0, -0.04, 0.95, -2.0, 1e-4, -2e-4])         # x' = (h0 x + h1 y + h2) / (h6 x + h7 y + 1) ...
PLANT_A = np.array([0.9, 0.1, -0.2, 1.05, 12.0, -7.0, 0.0, 0.0])              # x' = a0 x + a2 y + a4, y' = a1 x + a3 y + a5


def planted(kind, seed, F, N, specials=True):
    """(F, N, 4) float32 matches: per frame exactly ceil(0.6 N) follow the fixed map (noise-free in float64, then rounded), shuffled among
    uniform ones; with `specials`, frame 0 also holds a NaN, a +Inf and a 1e30 coordinate in its last three slots (N >= 8)."""
    rng = np.random.default_rng(seed)
    M = (PLANT_H if kind == PROJECTIVE else PLANT_A).reshape(1, 8)
    out = np.zeros((F, N, 4), F32)
    truth = np.zeros((F, N), bool)
    for f in range(F):
        xy = rng.uniform(0, [W_IMG, H_IMG], (N, 2))
        px, py = project(kind, M, xy[:, 0], xy[:, 1])
        uv = rng.uniform(0, [W_IMG, H_IMG], (N, 2))
        n_in = math.ceil(0.6 * N)
        who = rng.permutation(N)[:n_in]
        uv[who] = np.stack([px[0], py[0]], 1)[who]
        truth[f, who] = True
        out[f] = np.concatenate([xy, uv], 1).astype(F32)
    if specials and N >= 8:
        out[0, N - 1, 0], out[0, N - 2, 2], out[0, N - 3, 1] = np.nan, np.inf, 1e30
        truth[0, N - 3:] = False
    return out, truth


_BASES = {}


def base_floor(kind):
    """The smallest non-zero float64-against-longdouble displacement of the planted cases (seeds 1..6, 65 matches)."""
    if kind not in _BASES:
        vals = []
        for seed in range(1, 7):
            m, truth = planted(kind, seed, 1, 65, specials=False)
            inl = m[0][truth[0]]
            vals.append(corner_displacement(kind, refit(kind, inl), refit(kind, inl, np.longdouble), inl[:, :2]))
        _BASES[kind] = min(v for v in vals if v > 0)
        print(f"refit base, kind {kind}: float64 against longdouble on the planted cases: {min(vals):.3g} .. {max(vals):.3g} px")
    return _BASES[kind]


class Got:
    """A result as downloaded: mats, min_mats (F, 8) float64; counts, best int32; mask (F, N) uint8; raw: the bytes of each."""


def unpack(raw, F, N):
    """The outputs of one call laid end to end (d_mats, d_min_mats, d_counts, d_best, d_mask) as a Got."""
    raw = np.frombuffer(bytes(raw), np.uint8)
    sizes = (("mats", F * 64), ("min", F * 64), ("counts", F * 4), ("best", F * 4), ("mask", F * N))
    assert raw.size == sum(v for _, v in sizes)
    g, at = Got(), 0
    g.raw = {}
    for k, v in sizes:
        g.raw[k] = raw[at:at + v].copy()
        at += v
    g.mats, g.min_mats = g.raw["mats"].view(np.float64).reshape(F, 8), g.raw["min"].view(np.float64).reshape(F, 8)
    g.counts, g.best, g.mask = g.raw["counts"].view(np.int32), g.raw["best"].view(np.int32), g.raw["mask"].reshape(F, N)
    return g


def given_samples_case(kind):
    """Caller-given samples over three frames of 65 slots: (matches, the planted set, counts, samples (3, 8, 4))."""
    K = k_of(kind)
    m, truth = planted(kind, 41, 3, 65)
    counts = [65, 40, 65]
    # frame 0's list: four collinear points in slots 0..3, two coincident points in slots 4 and 5
    for k in range(4):
        m[0, k] = (10.0 + 20 * k, 30.0 + 10 * k, 50.0 + 20 * k, 5.0 + 10 * k)
    m[0, 5] = m[0, 4]
    truth[0, :6] = False
    good = [int(i) for i in np.flatnonzero(truth[0])[:4]]         # an all-inlier sample of frame 0
    s = np.zeros((3, 8, 4), np.int32)
    s[0] = [[6, 6, 7, 8],                                         # a repeated index
            [0, 1, 2, 3],                                         # collinear
            good,                                                 # h = 2: the best ...
            [4, 5, 7, 8],                                         # two coincident points, distinct indices
            [7, 8, 9, -1],                                        # -1 (affine ignores the fourth)
            good,                                                 # ... and h = 5 its twin
            [7, 8, 9, 10],
            [64, 63, 20, 21]]                                     # (slots 63, 64: the Inf and the NaN)
    s[1] = [[0, 1, 2, 40]] * 8                                    # an index equal to counts[f] (projective); affine: the third
    if K == 3:
        s[1, :, 2] = 40
    s[2] = [[-1, 0, 1, 2]] * 8                                    # every hypothesis invalid: the frame FAILS
    return m, truth, counts, s


def check(kind, g, w, matches, what, skip=()):
    """Device result g against the model's w: exact but for the refit."""
    assert np.array_equal(g.counts, w.counts), (what, "counts", g.counts.tolist(), w.counts.tolist())
    if "best" not in skip:
        assert np.array_equal(g.best, w.best), (what, "best", g.best.tolist(), w.best.tolist())
    if "mask" not in skip:
        assert np.array_equal(g.mask, w.mask), (what, "mask", np.argwhere(g.mask != w.mask)[:4].tolist())
    if "min" not in skip:
        assert np.array_equal(g.min_mats.view(np.uint64), w.min_mats.view(np.uint64)), (what, "minimal matrices", g.min_mats.tolist(), w.min_mats.tolist())
    for f in range(len(w.counts)):
        if w.refit_ld[f] is None:                                 # the minimal matrix, or the NaNs of a failed frame: bits
            assert np.array_equal(g.mats[f].view(np.uint64), w.mats[f].view(np.uint64)), (what, f, "d_mats", g.mats[f].tolist(), w.mats[f].tolist())
            continue
        pts = np.asarray(matches, F32)[f][w.mask[f] > 0][:, :2]
        base = corner_displacement(kind, w.mats[f], w.refit_ld[f], pts)
        if base == 0:
            base = base_floor(kind)
        dev = corner_displacement(kind, g.mats[f], w.mats[f], pts)
        print(f"{what} frame {f}: refit base {base:.3g} px, device {dev:.3g} px")
        assert np.isfinite(g.mats[f]).all() and dev <= 16 * base, (what, f, dev, base)


def counts_for(N):
    return [N, min(5, N), 0]
