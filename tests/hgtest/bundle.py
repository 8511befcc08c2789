"""The numpy model of hg_bundle_adjust_frames_device, written from the text of include/hgwarp.h ("adjusting a frame set over all pairs"):
float64 throughout, or with the sums and the solve in np.longdouble; the case builders and the tolerance recipe the CPU and the GPU tests
share.  The float64 model follows the header's order of operations in the pass (np.cumsum adds one term at a time) and in the solve."""
import os
import re
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from hgtest import align as AM

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
F64, LD = np.float64, np.longdouble
AFFINE, PROJECTIVE = 0, 1
CONVERGED, MAX_ITER, STALLED, SINGULAR = 0, 1, 2, 3
ADJUSTED, FIXED, UNANCHORED, BAD_INPUT = 0, 1, 2, 3
SUMS = 154
MAX_COORD = 16777216.0


def _const(name):
    text = open(os.path.join(ROOT, "homography.js_amd", "csrc", "hg_bundle_dev.h")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


def chunk():
    return _const("kBundleChunk")


def lds_cap():
    return _const("kBundleLdsCap")


def panel():
    return _const("kBundlePanel")


def p_of(kind):
    return 8 if kind == PROJECTIVE else 6


# ------------------------------------------------------------------------------------------------ matrices
def to3x3(kind, m, T=F64):
    m = np.asarray(m, T)
    if kind == PROJECTIVE:
        return np.array([[m[0], m[1], m[2]], [m[3], m[4], m[5]], [m[6], m[7], T(1)]], T)
    return np.array([[m[0], m[2], m[4]], [m[1], m[3], m[5]], [T(0), T(0), T(1)]], T)


def from3x3(kind, a):
    a = a / a[2, 2]
    if kind == PROJECTIVE:
        return a.ravel()[:8].copy()
    return np.array([a[0, 0], a[1, 0], a[0, 1], a[1, 1], a[0, 2], a[1, 2], 0, 0], a.dtype)


def normalise(kind, m, W, H, T=F64):
    """The iterate M' = T M T^-1 divided through by its last entry, row-major h0..h7, formed as the alignment forms H' (hgtest/align.py);
    all NaN where the input, or M', is not finite."""
    m = np.asarray(m, F64)
    if not np.isfinite(m[:p_of(kind)]).all():
        return np.full(8, np.nan, T)
    h = np.asarray(AM.normalise(kind, m, AM.geom(W, H, W, H, T), T), T)
    return h if np.isfinite(h).all() else np.full(8, np.nan, T)


def denormalise(kind, h, W, H):
    T = h.dtype.type
    return np.asarray(AM.denormalise(kind, h, AM.geom(W, H, W, H, T), T)).astype(F64)


def invert(kind, m):
    """hg_bundle_invert_matrix in longdouble."""
    return from3x3(kind, np.linalg.inv(to3x3(kind, m, F64)).astype(LD)).astype(F64)


def apply(kind, m, x, y):
    a = to3x3(kind, m, LD)
    x, y = np.asarray(x, LD), np.asarray(y, LD)
    d = a[2, 0] * x + a[2, 1] * y + a[2, 2]
    return (a[0, 0] * x + a[0, 1] * y + a[0, 2]) / d, (a[1, 0] * x + a[1, 1] * y + a[1, 2]) / d


def corner_displacement(kind, a, b, W, H):
    """The metric: the largest distance, in canvas pixels, between the images of the four frame corners under a and under b."""
    x, y = np.array([0, W - 1, 0, W - 1]), np.array([0, 0, H - 1, H - 1])
    ax, ay = apply(kind, a, x, y)
    bx, by = apply(kind, b, x, y)
    return float(np.sqrt((ax - bx) ** 2 + (ay - by) ** 2).max())


# ------------------------------------------------------------------------------------------------ one pass
def slots(kind, ha, hb, q, inside, W, H, huber, T):
    """The header's ONE SLOT over the (n, 4) float32 slots q of a pair: valid (n,), V (n, 2, 2 P + 1) rows, w (n,), rho (n,)."""
    P = p_of(kind)
    q = np.asarray(q, np.float32).astype(F64)
    s = F64(2) / F64(max(W, H))
    cx, cy = F64(W - 1) / 2, F64(H - 1) / 2
    with np.errstate(all="ignore"):
        ok = inside & (np.abs(q) <= MAX_COORD).all(1)
        x, y, u, v = (q[:, 0] - cx) * s, (q[:, 1] - cy) * s, (q[:, 2] - cx) * s, (q[:, 3] - cy) * s
        Da = (ha[6] * x + ha[7] * y) + 1 if kind == PROJECTIVE else np.ones_like(x)
        Db = (hb[6] * u + hb[7] * v) + 1 if kind == PROJECTIVE else np.ones_like(x)
        pax, pay = ((ha[0] * x + ha[1] * y) + ha[2]) / Da, ((ha[3] * x + ha[4] * y) + ha[5]) / Da
        pbx, pby = ((hb[0] * u + hb[1] * v) + hb[2]) / Db, ((hb[3] * u + hb[4] * v) + hb[5]) / Db
        ok = ok & np.isfinite(pax) & np.isfinite(pay) & np.isfinite(pbx) & np.isfinite(pby) & (Da > 0) & (Db > 0)
        rx, ry = pax - pbx, pay - pby
        e = np.sqrt(rx * rx + ry * ry) / s
        far = (e > huber) if huber > 0 else np.zeros_like(ok)
        w = np.where(far, huber / np.where(far, e, 1), 1.0)
        rho = np.where(far, 2 * huber * e - huber * huber, e * e)
        n = len(q)
        V = np.zeros((n, 2, 2 * P + 1), F64)
        z = np.zeros(n)
        if kind == PROJECTIVE:
            V[:, 0, :8] = np.stack([x / Da, y / Da, 1 / Da, z, z, z, -(pax * x) / Da, -(pax * y) / Da], 1)
            V[:, 1, :8] = np.stack([z, z, z, x / Da, y / Da, 1 / Da, -(pay * x) / Da, -(pay * y) / Da], 1)
            V[:, 0, 8:16] = -np.stack([u / Db, v / Db, 1 / Db, z, z, z, -(pbx * u) / Db, -(pbx * v) / Db], 1)
            V[:, 1, 8:16] = -np.stack([z, z, z, u / Db, v / Db, 1 / Db, -(pby * u) / Db, -(pby * v) / Db], 1)
        else:
            o = np.ones(n)
            V[:, 0, :6] = np.stack([x, z, y, z, o, z], 1)
            V[:, 1, :6] = np.stack([z, x, z, y, z, o], 1)
            V[:, 0, 6:12] = -np.stack([u, z, v, z, o, z], 1)
            V[:, 1, 6:12] = -np.stack([z, u, z, v, z, o], 1)
        V[:, 0, 2 * P], V[:, 1, 2 * P] = rx, ry
    V, w, rho = V[ok].astype(T), w[ok].astype(T), rho[ok].astype(T)
    return ok, V, w, rho


def tree_sum(v):
    """The decision's sum over pairs: lane l of 256 adds entries l, l + 256, .. in that order, then lane l += lane l + s for s = 128 .. 1."""
    lanes = np.zeros(256, v.dtype)
    for k in range(0, len(v), 256):
        part = v[k:k + 256]
        lanes[:len(part)] += part
    s = 128
    while s:
        lanes[:s] += lanes[s:2 * s]
        s //= 2
    return lanes[0]


def pair_record(kind, ha, hb, q, inside, W, H, huber, T):
    """The record of a pair in T: (2 P + 1)(P + 1) sums -- the last one the cost -- and the count; SUMS values, the tail zero.  The header's
    order: every entry over the slots of a chunk in ascending order, the chunks' sums in ascending order."""
    nv = 2 * p_of(kind) + 1
    iu = np.triu_indices(nv)
    ne = len(iu[0])
    rec = np.zeros(SUMS, T)
    CH = chunk()
    for k in range(0, len(q), CH):
        ok, V, w, rho = slots(kind, np.asarray(ha, F64), np.asarray(hb, F64), q[k:k + CH], inside[k:k + CH], W, H, huber, T)
        part = np.zeros(SUMS, T)
        if len(w):
            t = w[:, None] * ((V[:, 0, iu[0]] * V[:, 0, iu[1]]) + (V[:, 1, iu[0]] * V[:, 1, iu[1]]))
            t[:, ne - 1] = rho
            part[:ne] = np.cumsum(t, axis=0)[-1]
        part[ne] = int(ok.sum())
        rec += part
    return rec


def classify(c):
    """cls per frame (0 free, 1 fixed, 2 unanchored) by union-find over the pairs with counts > 0, and the free index of every frame."""
    F = c.F
    root = list(range(F))

    def find(f):
        while root[f] != f:
            root[f] = root[root[f]]
            f = root[f]
        return f
    for p, (a, b) in enumerate(c.pairs):
        if c.counts[p] > 0:
            ra, rb = find(a), find(b)
            if ra != rb:
                root[max(ra, rb)] = min(ra, rb)
    anch = {find(f) for f in range(F) if c.fixed[f]}
    cls = np.array([1 if c.fixed[f] else 0 if find(f) in anch else 2 for f in range(F)], np.int32)
    fidx = np.full(F, -1, np.int32)
    fidx[cls == 0] = np.arange(int((cls == 0).sum()))
    return cls, fidx


def evaluate(c, X, T):
    """One pass over the iterates X (F, 8): the records (n_pairs, SUMS) in T."""
    recs = np.zeros((len(c.pairs), SUMS), T)
    for p, (a, b) in enumerate(c.pairs):
        n = int(c.counts[p])
        inside = np.ones(n, bool) if c.mask is None else c.mask[p, :n] != 0
        recs[p] = pair_record(c.kind, X[a], X[b], c.matches[p, :n], inside, c.W, c.H, c.huber, T)
    return recs


def assemble(c, recs, cls, fidx):
    P = p_of(c.kind)
    nv = 2 * P + 1
    N = P * int((cls == 0).sum())
    T = recs.dtype.type
    Hm, g = np.zeros((N, N), T), np.zeros(N, T)
    iu = np.triu_indices(nv)
    for p, (a, b) in enumerate(c.pairs):
        G = np.zeros((nv, nv), T)
        G[iu] = recs[p, :len(iu[0])]
        G = G + np.triu(G, 1).T
        ia, ib = fidx[a], fidx[b]
        if ia >= 0:
            Hm[ia * P:ia * P + P, ia * P:ia * P + P] += G[:P, :P]
            g[ia * P:ia * P + P] -= G[:P, 2 * P]
        if ib >= 0:
            Hm[ib * P:ib * P + P, ib * P:ib * P + P] += G[P:2 * P, P:2 * P]
            g[ib * P:ib * P + P] -= G[P:2 * P, 2 * P]
        if ia >= 0 and ib >= 0:
            Hm[ia * P:ia * P + P, ib * P:ib * P + P] += G[:P, P:2 * P]
            Hm[ib * P:ib * P + P, ia * P:ia * P + P] += G[:P, P:2 * P].T
    return Hm, g


def solve_header(A, b, nb=32, rb=64):
    """The header's SOLVE to the letter: Cholesky with b as one more row, every entry a_ic -= l_ij l_cj one j at a time in ascending j (a
    product, then a difference: two roundings), then the back substitution.  Walked in panels of nb columns and blocks of rb rows so that
    numpy stays in cache; every entry still sees the same operations in the same order.  None at a pivot that is not positive and finite."""
    N = len(b)
    M = np.vstack([A, b[None, :]])
    pool = ThreadPoolExecutor(8) if N > 512 else None
    with np.errstate(all="ignore"):
        for k0 in range(0, N, nb):
            k1 = min(k0 + nb, N)
            S = M[k0:, k0:k1]
            for j in range(k1 - k0):
                d = S[j, j]
                if not (d > 0 and np.isfinite(d)):
                    if pool:
                        pool.shutdown()
                    return None
                l = np.sqrt(d)
                S[j + 1:, j] /= l
                S[j, j] = l
                if j + 1 < k1 - k0:
                    S[j + 1:, j + 1:] -= np.outer(S[j + 1:, j], S[j + 1:k1 - k0, j])
            def update(r0):
                r1 = min(r0 + rb, N + 1)
                c1 = min(N, r1)
                T, Li, Lj = M[r0:r1, k1:c1], M[r0:r1, k0:k1], np.ascontiguousarray(M[k1:c1, k0:k1].T)
                tmp = np.empty(T.shape)
                for k in range(k1 - k0):
                    np.multiply(Li[:, k:k + 1], Lj[k], out=tmp)
                    np.subtract(T, tmp, out=T)
            blocks = range(k1, N + 1, rb)
            if pool is None:
                for r0 in blocks:
                    update(r0)
            else:
                list(pool.map(update, blocks))                    # (row blocks are independent; numpy's loops release the interpreter)
        if pool:
            pool.shutdown()
        y = M[N].copy()
        for k in range(N - 1, -1, -1):
            y[k] = y[k] / M[k, k]
            y[:k] -= M[k, :k] * y[k]
    return y


def solve(A, b):
    """A x = b for a symmetric positive definite A; None where a pivot fails.  float64: the header's order.  longdouble: LAPACK's float64
    factor, then iterative refinement with longdouble residuals until the correction no longer registers."""
    T = A.dtype.type
    if T is F64:
        return solve_header(A, b)
    A64 = A.astype(F64)
    try:
        L = np.linalg.cholesky(A64)
    except np.linalg.LinAlgError:
        return None
    import scipy.linalg as SL

    def s64(r):
        return SL.solve_triangular(L.T, SL.solve_triangular(L, r, lower=True), lower=False)
    x = s64(b.astype(F64)).astype(T)
    if T is not F64:
        for _ in range(6):
            dx = s64((b - A @ x).astype(F64)).astype(T)
            x = x + dx
            if np.abs(dx).max() <= 1e-21 * max(np.abs(x).max(), 1e-300):
                break
    return x if np.isfinite(x.astype(F64)).all() else None


SLOT = {AFFINE: (0, 3, 1, 4, 2, 5), PROJECTIVE: (0, 1, 2, 3, 4, 5, 6, 7)}     # parameter k -> its slot in the row-major iterate


def adjust(c, T=F64):
    """The whole call in T.  Returns mats (F, 8) float64, info (dict), frames (F,) int32, pairs (dict of arrays), sums (n_pairs, SUMS) in T,
    and margin: the smallest relative distance of a decision (cost < c, displacement < eps, lambda > 1e12) from its tie."""
    kind, F, W, H, P = c.kind, c.F, c.W, c.H, p_of(c.kind)
    nv = 2 * P + 1
    ne = nv * (nv + 1) // 2
    cls, fidx = classify(c)
    N = P * int((cls == 0).sum())
    good = np.array([np.isfinite(normalise(kind, c.mats[f], W, H, F64)).all() for f in range(F)])
    X = np.stack([normalise(kind, c.mats[f], W, H, T) for f in range(F)]) if F else np.zeros((0, 8), T)
    out = types.SimpleNamespace(margin=np.inf)
    recs = evaluate(c, X, T)
    out.sums = recs.copy()
    cost, n = tree_sum(recs[:, ne - 1]), int(recs[:, ne].sum())
    first = (cost, n, recs.copy())
    lam, rounds, accepted, status = T(c.lambda0), 0, 0, MAX_ITER
    n_iter = c.n_iter if N > 0 else 0
    movers = [f for f in range(F) if cls[f] == 0 and good[f]]
    Hm = g = None
    for k in range(1, n_iter + 1):
        rounds = k
        if Hm is None:
            Hm, g = assemble(c, recs, cls, fidx)
        with np.errstate(all="ignore"):
            delta = solve(Hm + lam * np.eye(N, dtype=T), g)
        if delta is None:
            status = SINGULAR
            break
        Xn = X.copy()
        for f in range(F):
            if cls[f] == 0:
                for j in range(P):
                    Xn[f, SLOT[kind][j]] += delta[fidx[f] * P + j]
        rn = evaluate(c, Xn, T)
        cn, nn = tree_sum(rn[:, ne - 1]), int(rn[:, ne].sum())
        finite = all(np.isfinite(Xn[f].astype(F64)).all() for f in movers)
        if finite and nn >= n and cost > 0:
            out.margin = min(out.margin, abs(float((cn - cost) / cost)))
        if finite and nn >= n and cn < cost:
            disp = max([corner_displacement(kind, denormalise(kind, X[f], W, H), denormalise(kind, Xn[f], W, H), W, H) for f in movers] or [0.0])
            X, recs, cost, n, Hm = Xn, rn, cn, nn, None
            accepted += 1
            lam = max(lam / 10, T(1e-12))
            if c.eps > 0:
                out.margin = min(out.margin, abs(disp - c.eps) / c.eps)
            if disp < c.eps:
                status = CONVERGED
                break
        else:
            lam = lam * 10
            out.margin = min(out.margin, abs(float(lam) - 1e12) / 1e12)
            if lam > 1e12:
                status = STALLED
                break
    with np.errstate(all="ignore"):
        out.mats = np.stack([denormalise(kind, X[f], W, H) if (cls[f] == 0 and good[f] and accepted > 0) else np.asarray(c.mats[f], F64)
                             for f in range(F)]) if F else np.zeros((0, 8))
        out.info = dict(status=status, rounds=rounds, accepted=accepted, n_valid_first=first[1], n_valid_last=n,
                        rms_first=np.sqrt(first[0] / T(first[1])) if first[1] else T(np.nan), rms_last=np.sqrt(cost / T(n)) if n else T(np.nan),
                        lambda_last=lam, cost_first=first[0], cost_last=cost)
        out.frames = np.where(cls != 0, cls, np.where(good, ADJUSTED, BAD_INPUT)).astype(np.int32)
        nf, nl = first[2][:, ne].astype(np.int64), recs[:, ne].astype(np.int64)
        out.pairs = dict(n_valid_first=nf, n_valid_last=nl, rms_first=np.sqrt(first[2][:, ne - 1] / np.where(nf > 0, nf, np.nan).astype(T)),
                         rms_last=np.sqrt(recs[:, ne - 1] / np.where(nl > 0, nl, np.nan).astype(T)))
    return out


def rms_over_pairs(c, mats):
    """sqrt(cost / n_valid) of the matrices `mats` over all pairs of c, huber off, in longdouble: the number a caller cares about."""
    d = types.SimpleNamespace(**vars(c))
    d.huber = 0.0
    X = np.stack([normalise(c.kind, mats[f], c.W, c.H, LD) for f in range(c.F)])
    ne = (2 * p_of(c.kind) + 1) * (p_of(c.kind) + 1)
    r = evaluate(d, X, LD)
    return float(np.sqrt(r[:, ne - 1].sum() / r[:, ne].sum()))


# ------------------------------------------------------------------------------------------------ cases
def case(kind, W, H, mats, fixed, pairs, matches, counts=None, mask=None, n_iter=10, eps=0.01, lambda0=1e-3, huber=0.0):
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    matches = np.ascontiguousarray(matches, np.float32)
    matches = matches.reshape(len(pairs), -1, 4) if len(pairs) else matches.reshape(0, matches.shape[1] if matches.ndim == 3 else 0, 4)
    fx = np.zeros(len(mats), np.uint8)
    fx[list(fixed)] = 1
    return types.SimpleNamespace(kind=kind, W=W, H=H, F=len(mats), mats=np.ascontiguousarray(mats, F64).reshape(-1, 8), fixed=fx, pairs=pairs,
                                 matches=matches, n_points=matches.shape[1], counts_arg=counts,
                                 counts=np.full(len(pairs), matches.shape[1], np.int32) if counts is None else np.asarray(counts, np.int32),
                                 mask=None if mask is None else np.ascontiguousarray(mask, np.uint8), n_iter=n_iter, eps=eps, lambda0=lambda0,
                                 huber=huber)


def true_mats(kind, F, W, H, rng, cols=None):
    """Plausible frame -> canvas matrices: frame f shifted by 30 % of its width per column (rows of `cols` frames), so that next-but-one
    frames still overlap, a small turn and scale, for projective a small tilt.  Frame 0 is the identity."""
    cols = cols or F
    out = []
    for f in range(F):
        if f == 0:
            out.append(np.array([1, 0, 0, 0, 1, 0, 0, 0], F64) if kind == PROJECTIVE else np.array([1, 0, 0, 1, 0, 0, 0, 0], F64))
            continue
        ang, sc = rng.uniform(-0.05, 0.05), rng.uniform(0.97, 1.03)
        a = np.array([[sc * np.cos(ang), -sc * np.sin(ang), 0.3 * W * (f % cols) + rng.uniform(-3, 3)],
                      [sc * np.sin(ang), sc * np.cos(ang), 0.3 * H * (f // cols) + rng.uniform(-3, 3)],
                      [rng.uniform(-2e-4, 2e-4) if kind == PROJECTIVE else 0, rng.uniform(-2e-4, 2e-4) if kind == PROJECTIVE else 0, 1]])
        out.append(from3x3(kind, a))
    return np.stack(out)


def make_matches(kind, truth, pairs, n, W, H, rng, sigma=0.0):
    """n matches per pair: (x, y) uniform in frame a where its image lies inside frame b too (anywhere in a if the frames hardly overlap),
    (u, v) that image under the truth plus N(0, sigma) per coordinate, as float32."""
    M = np.zeros((len(pairs), n, 4), np.float32)
    for p, (a, b) in enumerate(pairs):
        x, y = rng.uniform(0, W - 1, 16 * n), rng.uniform(0, H - 1, 16 * n)
        cx, cy = apply(kind, truth[a], x, y)
        u, v = apply(kind, invert(kind, truth[b]), cx, cy)
        u, v = np.asarray(u, F64), np.asarray(v, F64)
        inside = (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
        k = np.concatenate([np.flatnonzero(inside), np.flatnonzero(~inside)])[:n]
        nu, nv = (rng.normal(0, sigma, n), rng.normal(0, sigma, n)) if sigma else (0.0, 0.0)
        M[p] = np.stack([x[k], y[k], u[k] + nu, v[k] + nv], 1)
    return M


def perturb(kind, truth, W, H, rng, px, keep=(0,)):
    """The truth with every frame outside `keep` moved so that its corners travel px pixels or so."""
    out = truth.copy()
    for f in range(len(truth)):
        if f in keep:
            continue
        a = to3x3(kind, truth[f])
        d = np.array([[1 + rng.uniform(-1, 1) * px / W, rng.uniform(-1, 1) * px / W, rng.uniform(-1, 1) * px],
                      [rng.uniform(-1, 1) * px / H, 1 + rng.uniform(-1, 1) * px / H, rng.uniform(-1, 1) * px], [0, 0, 1]])
        out[f] = from3x3(kind, d @ a)
    return out


def chain_pairs(F, extra=()):
    return [(f, f + 1) for f in range(F - 1)] + list(extra)


def planted_case(kind, F=5, n=40, seed=1, px=1.5, sigma=0.0, extra=((0, 2),), fixed=(0,), W=96, H=64, **kw):
    rng = np.random.default_rng(seed)
    truth = true_mats(kind, F, W, H, rng)
    pairs = chain_pairs(F, [e for e in extra if max(e) < F])
    M = make_matches(kind, truth, pairs, n, W, H, rng, sigma)
    c = case(kind, W, H, perturb(kind, truth, W, H, rng, px, keep=fixed), fixed, pairs, M, **kw)
    c.truth = truth
    return c


def count_case(kind, n):
    """Three frames, two pairs; the first pair uses n of its slots (n_iter = 0: one pass)."""
    npts = max(n, 8)
    c = planted_case(kind, F=3, n=npts, seed=100 + n, extra=(), n_iter=0)
    c.counts = np.array([n, min(npts, 8)], np.int32)
    c.counts_arg = c.counts
    return c


def free_case(kind, n_free, n=24, n_iter=3, seed=7):
    """n_free free frames behind one fixed frame: a chain with next-but-one pairs; N = P n_free."""
    F = n_free + 1
    return planted_case(kind, F=F, n=n, seed=seed + n_free, px=2.0, extra=[(f, f + 2) for f in range(F - 2)], n_iter=n_iter, eps=1e-3)


def big_case():
    """256 projective frames (N = 2040): a chain plus a handful of closing pairs, 8 matches per pair, two rounds."""
    F = 256
    rng = np.random.default_rng(256)
    truth = true_mats(PROJECTIVE, F, 96, 64, rng, cols=16)
    pairs = chain_pairs(F, [(f, f + 16) for f in (0, 17, 40, 100, 200, 239)])
    M = make_matches(PROJECTIVE, truth, pairs, 8, 96, 64, rng)
    c = case(PROJECTIVE, 96, 64, perturb(PROJECTIVE, truth, 96, 64, rng, 1.0), (0,), pairs, M, n_iter=2, eps=1e-6)
    c.truth = truth
    return c


def ring_case(seed=5):
    """The loop closure: 8 frames of 96 x 64 around a 3 x 3 block (the middle left out), matches with sigma = 0.5 px between ring neighbours,
    pairwise least-squares matrices (the model of the fit's n_hyp = 0 refit), chained WITHOUT the closing pair.  Returns the case started at
    the chain, over all 8 pairs."""
    from hgtest import fit as FM
    kind, W, H = PROJECTIVE, 96, 64
    rng = np.random.default_rng(seed)
    cells = [(0, 0), (1, 0), (2, 0), (2, 1), (2, 2), (1, 2), (0, 2), (0, 1)]
    truth = []
    for f, (i, j) in enumerate(cells):
        ang = 0.0 if f == 0 else rng.uniform(-0.03, 0.03)
        a = np.array([[np.cos(ang), -np.sin(ang), 0.6 * W * i], [np.sin(ang), np.cos(ang), 0.6 * H * j],
                      [0 if f == 0 else rng.uniform(-1e-4, 1e-4), 0 if f == 0 else rng.uniform(-1e-4, 1e-4), 1]])
        truth.append(from3x3(kind, a))
    truth = np.stack(truth)
    pairs = [(f, (f + 1) % 8) for f in range(8)]
    M = make_matches(kind, truth, pairs, 32, W, H, rng, 0.5)
    pm = np.stack([FM.refit(kind, M[p]) for p in range(8)]).astype(F64)
    start = chain(kind, 8, pairs[:7], pm[:7], 0)
    c = case(kind, W, H, start, (0,), pairs, M, n_iter=10, eps=0.01)
    c.truth, c.pair_mats = truth, pm
    return c


def huber_case(huber, kind=PROJECTIVE, seed=11):
    """Five frames, 10 % of the slots moved by 30 px, no mask."""
    c = planted_case(kind, F=5, n=60, seed=seed, px=2.0, sigma=0.2, extra=((0, 2), (1, 3), (2, 4)), n_iter=12, eps=1e-3, huber=huber)
    rng = np.random.default_rng(seed + 1)
    bad = rng.random(c.matches.shape[:2]) < 0.10
    ang = rng.uniform(0, 2 * np.pi, bad.sum())
    c.matches[bad, 2] += (30 * np.cos(ang)).astype(np.float32)
    c.matches[bad, 3] += (30 * np.sin(ang)).astype(np.float32)
    return c


def truth_error(c, mats):
    return max(corner_displacement(c.kind, mats[f], c.truth[f], c.W, c.H) for f in range(c.F))


def chain(kind, F, pairs, pair_mats, anchor):
    """hg_bundle_chain_from_pairs in longdouble."""
    M = [None] * F
    level = [-1] * F
    M[anchor], level[anchor] = np.eye(3, dtype=LD), 0
    ok = [np.isfinite(np.asarray(m, F64)[:p_of(kind)]).all() for m in pair_mats]
    lv = 0
    while True:
        grew = False
        for p, (a, b) in enumerate(pairs):
            if not ok[p]:
                continue
            q = to3x3(kind, pair_mats[p], LD)
            if level[b] == lv and level[a] < 0:
                t = M[b] @ q
                M[a], level[a], grew = t / t[2, 2], lv + 1, True
            elif level[a] == lv and level[b] < 0:
                qi = np.linalg.inv(q.astype(F64)).astype(LD)
                qi = qi + qi @ (np.eye(3, dtype=LD) - q @ qi)          # one Newton step: the inverse to longdouble
                t = M[a] @ (qi / qi[2, 2])
                M[b], level[b], grew = t / t[2, 2], lv + 1, True
        if not grew:
            break
        lv += 1
    return np.stack([np.full(8, np.nan) if M[f] is None else from3x3(kind, M[f]).astype(F64) for f in range(F)])


# ------------------------------------------------------------------------------------------------ the tolerance
def rel(a, b):
    """|a - b| / |b| entry by entry, 0 where both are 0 (or both NaN)."""
    a, b = np.asarray(a, LD), np.asarray(b, LD)
    with np.errstate(all="ignore"):
        r = np.abs(a - b) / np.abs(b)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    return np.where(same, 0, r).astype(F64)


_FLOOR = {}
HALF_ULP = 2.0 ** -53                        # a float64 cannot be asked to lie closer to a longdouble value than this, relatively


def floors():
    """The smallest non-zero bases of the planted cases: matrices (px), sums and rms (relative)."""
    if not _FLOOR:
        m, s, r = [], [], []
        for kind in (AFFINE, PROJECTIVE):
            c = planted_case(kind)
            a, b = adjust(c, F64), adjust(c, LD)
            m += [corner_displacement(kind, a.mats[f], b.mats[f], c.W, c.H) for f in range(c.F)]
            s += list(rel(a.sums, b.sums).max(1))
            r += [float(rel(a.info["rms_first"], b.info["rms_first"])), float(rel(a.info["rms_last"], b.info["rms_last"]))]
        for k, v in (("mats", m), ("sums", s), ("rms", r)):
            _FLOOR[k] = min(x for x in v if x > 0)
    return _FLOOR


def compare(c, got, m64, mld):
    """The device result `got` (mats (F, 8), sums (n_pairs, SUMS) or None, rms_first, rms_last, pair rms arrays) against the models by the
    recipe: 16 x the base (float64 model vs longdouble model), a base of 0 replaced by the floor.  Returns the largest device / base ratio."""
    fl = floors()
    worst = 0.0
    for f in range(c.F):
        if np.isnan(m64.mats[f]).any() or np.isnan(got.mats[f]).any():
            assert np.array_equal(np.asarray(got.mats[f]).view(np.uint64), m64.mats[f].view(np.uint64)), (f, "bits of a frame that is not finite")
            continue
        base = corner_displacement(c.kind, m64.mats[f], mld.mats[f], c.W, c.H) or fl["mats"]
        d = corner_displacement(c.kind, got.mats[f], m64.mats[f], c.W, c.H)
        assert d <= 16 * base, ("matrix", f, d, base)
        worst = max(worst, d / base)
    if got.sums is not None:
        for p in range(len(c.pairs)):
            base = max(rel(m64.sums[p], mld.sums[p]).max() or fl["sums"], HALF_ULP)
            d = rel(got.sums[p], mld.sums[p]).max()
            assert d <= 16 * base, ("sums", p, d, base)
            worst = max(worst, d / base)
    for k in ("rms_first", "rms_last"):
        for g, a, b in ((got.info[k], m64.info[k], mld.info[k]), (got.pairs[k], m64.pairs[k], mld.pairs[k])):
            base = np.maximum(np.where(rel(a, b) > 0, rel(a, b), fl["rms"]), HALF_ULP)
            d = rel(g, b)
            assert (d <= 16 * base).all(), (k, d, base)
            worst = max(worst, float((d / base).max()) if np.size(d) else 0.0)
    return worst


def decisions_clear(m64, mld):
    """No decision of the run (cost < c, displacement < eps, lambda > 1e12) lies within 16 x base of a tie, base being the relative error of
    the float64 model's costs against the longdouble model's: the condition under which status, rounds, accepted and n_valid may be compared
    exactly with the device's."""
    base = max(float(rel(m64.info["cost_first"], mld.info["cost_first"])), float(rel(m64.info["cost_last"], mld.info["cost_last"])), HALF_ULP)
    same = all(int(m64.info[k]) == int(mld.info[k]) for k in ("status", "rounds", "accepted", "n_valid_first", "n_valid_last"))
    return same and m64.margin > 16 * base


COUNTS = (0, 1, 3, 4, 255, 256, 257)          # (3 and 4: P / 2 of the two kinds)


def gpu_cases():
    """(name, case) of the cases tests/test_gpu_bundle.py compares exactly."""
    CH, CAP, PANEL = chunk(), lds_cap(), panel()
    for kind in (AFFINE, PROJECTIVE):
        for n in COUNTS + (CH - 1, CH, CH + 1, 2 * CH + 1):
            yield ("count", kind, n), count_case(kind, n)
        for huber in (0.0, 1.0):
            yield ("planted", kind, huber), planted_case(kind, sigma=0.3, huber=huber, n=70)
    for kind, n_free in free_counts():
        yield ("free", kind, n_free), free_case(kind, n_free)
    yield ("ring",), ring_case()


def free_counts():
    CAP, PANEL = lds_cap(), panel()
    return [(PROJECTIVE, CAP // 8 - 1), (PROJECTIVE, CAP // 8), (PROJECTIVE, CAP // 8 + 1), (PROJECTIVE, (CAP + 2 * PANEL) // 8), (AFFINE, CAP // 6),
            (AFFINE, CAP // 6 + 1), (AFFINE, 2), (PROJECTIVE, 1)]


def compare_exact(got, m64):
    """status, rounds, accepted and every n_valid: exactly the model's (tests/test_bundle_cpu.py fixes when this may be asked)."""
    for k in ("status", "rounds", "accepted", "n_valid_first", "n_valid_last"):
        assert int(got.info[k]) == int(m64.info[k]), (k, got.info[k], m64.info[k])
    assert np.array_equal(got.frames, m64.frames)
    for k in ("n_valid_first", "n_valid_last"):
        assert np.array_equal(np.asarray(got.pairs[k], np.int64), m64.pairs[k]), k


# ------------------------------------------------------------------------------------------------ the host check's files
INFO = np.dtype([("status", np.int32), ("rounds", np.int32), ("accepted", np.int32), ("n_valid_first", np.int32), ("n_valid_last", np.int32),
                 ("pad", np.int32), ("rms_first", np.float64), ("rms_last", np.float64), ("lambda_last", np.float64)])
PAIR_INFO = np.dtype([("n_valid_first", np.int32), ("n_valid_last", np.int32), ("rms_first", np.float64), ("rms_last", np.float64)])


def info_bytes(F, NP):
    return 48 + ((4 * F + 7) & ~7) + 24 * NP


def pack(c, large=False, want_sums=True):
    """The input file of tests/cpp/bundle_check.cpp (its layout is stated there)."""
    head = np.array([c.kind, c.W, c.H, c.F, len(c.pairs), c.n_points, c.n_iter, int(large), int(want_sums), int(c.mask is not None), 0, 0], np.int32)
    parts = [head.tobytes(), np.array([c.eps, c.lambda0, c.huber], F64).tobytes(), c.fixed.astype(np.int32).tobytes(), c.pairs.astype(np.int32).tobytes(),
             np.asarray(c.counts, np.int32).tobytes(), c.matches.tobytes()]
    if c.mask is not None:
        parts.append(c.mask.tobytes())
    parts.append(c.mats.tobytes())
    return b"".join(parts)


def unpack_host(raw, c, want_sums=True):
    """The output file of the host check as the GPU test's result object (raw: the file's bytes)."""
    F, NP = c.F, len(c.pairs)
    ib = info_bytes(F, NP)
    assert len(raw) == F * 64 + ib + (NP * SUMS * 8 if want_sums else 0), len(raw)
    buf = np.frombuffer(raw, np.uint8)
    info = buf[F * 64:F * 64 + 48].view(INFO)[0]
    o = F * 64 + 48 + ((4 * F + 7) & ~7)
    pairs = buf[o:o + 24 * NP].view(PAIR_INFO)
    return types.SimpleNamespace(mats=buf[:F * 64].view(F64).reshape(F, 8).copy(), sums=buf[F * 64 + ib:].view(F64).reshape(NP, SUMS).copy() if want_sums else None,
                                 info={k: info[k] for k in INFO.names}, frames=buf[F * 64 + 48:F * 64 + 48 + 4 * F].view(np.int32).copy(),
                                 pairs={k: pairs[k].copy() for k in PAIR_INFO.names}, raw=bytes(raw))
