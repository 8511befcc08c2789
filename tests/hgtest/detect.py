"""The numpy model of the keypoint feature (include/hgwarp.h, "detecting and describing keypoints"), written from the header's text: luma,
the Harris response in integers, the candidates under the total order, the per-cell selection, the orientation bin, the sampling pattern
and the 256-bit descriptor; model() returns what hg_detect_describe_frames_device writes, padding included.  Everything is integer
arithmetic in int64 (the header bounds every intermediate), so the comparison with the device is byte for byte.  Also the case builders
the CPU and GPU tests share."""
import hashlib
from types import SimpleNamespace

import numpy as np

MARGIN, DESC_BYTES, BINS = 16, 32, 32
PAD_WORD = 0x7FC00000
INFO = np.dtype([("R", "<i8"), ("bin", "<i4"), ("idx", "<i4")])
NO_R = np.iinfo(np.int64).min                     # "no response here": outside 4 <= x < W - 4, 4 <= y < H - 4

_C9 = (16384, 16069, 15137, 13623, 11585, 9102, 6270, 3196, 0)


def cos_table():
    c = [0] * 32
    for k in range(9):
        c[k] = _C9[k]
    for k in range(9):
        c[16 - k] = -_C9[k]
    for k in range(1, 16):
        c[32 - k] = c[k]
    return np.array(c, np.int64)


def sin_table():
    c = cos_table()
    return np.array([c[(k + 24) % 32] for k in range(32)], np.int64)


def mix(a):
    a &= 0xFFFFFFFF
    a ^= a >> 16
    a = (a * 0x7FEB352D) & 0xFFFFFFFF
    a ^= a >> 15
    a = (a * 0x846CA68B) & 0xFFFFFFFF
    a ^= a >> 16
    return a


def base_pattern():
    """256 x 4 int8 {ax, ay, bx, by}: per test the first kept point of its walk and the next kept point that differs."""
    out = np.zeros((256, 4), np.int8)
    root = mix(0x9E3779B9)
    for b in range(256):
        key = mix((root + b) & 0xFFFFFFFF)
        a = None
        t = 0
        while True:
            w = mix((key + t) & 0xFFFFFFFF)
            t += 1
            x = (w & 7) + ((w >> 3) & 7) + ((w >> 6) & 7) + ((w >> 9) & 7) - 14
            y = ((w >> 12) & 7) + ((w >> 15) & 7) + ((w >> 18) & 7) + ((w >> 21) & 7) - 14
            if x * x + y * y > 144:
                continue
            if a is None:
                a = (x, y)
            elif (x, y) != a:
                out[b] = (a[0], a[1], x, y)
                break
    return out


_PATTERN = None


def pattern():
    """BINS x 256 x 4 int8: the base pattern turned by every bin with arithmetic shifts."""
    global _PATTERN
    if _PATTERN is None:
        base = base_pattern().astype(np.int64)
        c, s = cos_table(), sin_table()
        out = np.zeros((BINS, 256, 4), np.int64)
        for k in range(BINS):
            for o in (0, 2):
                x, y = base[:, o], base[:, o + 1]
                out[k, :, o] = (x * c[k] - y * s[k] + 8192) >> 14
                out[k, :, o + 1] = (x * s[k] + y * c[k] + 8192) >> 14
        assert np.abs(out).max() <= 12
        _PATTERN = out.astype(np.int8)
    return _PATTERN


def tile():
    """T: the side of a sub-tile of k_detect_cells, read from the constant the shared header exposes."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    text = open(os.path.join(root, "homography.js_amd", "csrc", "hg_detect_dev.h")).read()
    return int(re.search(r"constexpr int kDetectTile = (\d+);", text).group(1))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def layout(W, H, cell, per_cell):
    cx, cy = -(-W // cell), -(-H // cell)
    return cx, cy, cx * cy * per_cell


def luma(plane, channels):
    """plane: H x W (1 channel) or H x W x 4 u8 -> H x W int64."""
    p = np.asarray(plane).astype(np.int64)
    if channels == 1:
        return p
    return (77 * p[..., 0] + 150 * p[..., 1] + 29 * p[..., 2] + 128) >> 8


def _box(a, r):
    """Sum over the (2r + 1)^2 window; valid (H - 2r) x (W - 2r) part."""
    H, W = a.shape
    n = 2 * r + 1
    h = sum(a[:, k:W - n + 1 + k] for k in range(n))
    return sum(h[k:H - n + 1 + k, :] for k in range(n))


def response(L):
    """H x W int64, NO_R where R is not defined."""
    H, W = L.shape
    R = np.full((H, W), NO_R, np.int64)
    if W < 9 or H < 9:
        return R
    ix = np.zeros((H, W), np.int64)
    iy = np.zeros((H, W), np.int64)
    ix[1:-1, 1:-1] = (L[:-2, 2:] + 2 * L[1:-1, 2:] + L[2:, 2:]) - (L[:-2, :-2] + 2 * L[1:-1, :-2] + L[2:, :-2])
    iy[1:-1, 1:-1] = (L[2:, :-2] + 2 * L[2:, 1:-1] + L[2:, 2:]) - (L[:-2, :-2] + 2 * L[:-2, 1:-1] + L[:-2, 2:])
    gx, gy = ix[1:-1, 1:-1], iy[1:-1, 1:-1]                       # rows, columns 1 .. -1
    A, Cc, B = _box(gx * gx, 3), _box(gy * gy, 3), _box(gx * gy, 3)     # centres 4 .. -4
    R[4:H - 4, 4:W - 4] = 16 * (A * Cc - B * B) - (A + Cc) * (A + Cc)
    return R


def candidates(R, min_response):
    """Flat indices (ascending) of the candidates of a plane."""
    H, W = R.shape
    if W < 33 or H < 33:
        return np.zeros(0, np.int64)
    c = R[16:H - 16, 16:W - 16]
    ok = c >= min_response
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy == 0 and dx == 0:
                continue
            q = R[16 + dy:H - 16 + dy, 16 + dx:W - 16 + dx]
            lower = dy < 0 or (dy == 0 and dx < 0)                # q has the lower flat index: it wins a tie
            ok &= (c > q) if lower else (c >= q)
    ys, xs = np.nonzero(ok)
    return (ys + 16) * W + (xs + 16)


def select(R, cand, cell, per_cell):
    """The keypoints of a plane in list order: by cell ascending, within a cell by (larger R, lower index)."""
    H, W = R.shape
    cx = -(-W // cell)
    y, x = cand // W, cand % W
    cid = (y // cell) * cx + x // cell
    r = R.reshape(-1)[cand]
    order = np.lexsort((cand, -r, cid))
    cid, cand = cid[order], cand[order]
    first = np.r_[True, cid[1:] != cid[:-1]] if len(cid) else np.zeros(0, bool)
    start = np.maximum.accumulate(np.where(first, np.arange(len(cid)), 0)) if len(cid) else np.zeros(0, np.int64)
    rank = np.arange(len(cid)) - start
    return cand[rank < per_cell]


_DISC = None


def disc():
    global _DISC
    if _DISC is None:
        d = np.arange(-15, 16)
        dy, dx = np.meshgrid(d, d, indexing="ij")
        keep = dx * dx + dy * dy <= 225
        _DISC = (dy[keep].astype(np.int64), dx[keep].astype(np.int64))
    return _DISC


def moments(L, kp):
    H, W = L.shape
    dy, dx = disc()
    y, x = kp // W, kp % W
    m10 = np.zeros(len(kp), np.int64)
    m01 = np.zeros(len(kp), np.int64)
    for s in range(0, len(kp), 2048):
        v = L[y[s:s + 2048, None] + dy[None, :], x[s:s + 2048, None] + dx[None, :]]
        m10[s:s + 2048] = (v * dx).sum(1)
        m01[s:s + 2048] = (v * dy).sum(1)
    return m10, m01


def choose_bin(m10, m01):
    c, s = cos_table(), sin_table()
    score = np.asarray(m10, np.int64)[:, None] * c[None, :] + np.asarray(m01, np.int64)[:, None] * s[None, :]
    return np.argmax(score, axis=1).astype(np.int32)              # (the first of equal maxima: the lowest k)


def describe(L, kp, bins):
    H, W = L.shape
    S = np.zeros((H, W), np.int64)
    S[2:H - 2, 2:W - 2] = _box(L, 2)
    out = np.zeros((len(kp), 32), np.uint8)
    for s in range(0, len(kp), 2048):
        tab = pattern().astype(np.int64)[bins[s:s + 2048]]        # n x 256 x 4
        y, x = (kp[s:s + 2048] // W)[:, None], (kp[s:s + 2048] % W)[:, None]
        bit = S[y + tab[:, :, 1], x + tab[:, :, 0]] < S[y + tab[:, :, 3], x + tab[:, :, 2]]
        out[s:s + 2048] = np.packbits(bit.astype(np.uint8), axis=1, bitorder="little")
    return out


def model_plane(plane, channels, cell, per_cell, min_response):
    L = luma(plane, channels)
    R = response(L)
    kp = select(R, candidates(R, min_response), cell, per_cell)
    if len(kp) == 0:
        return kp, np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros((0, 32), np.uint8), R
    bins = choose_bin(*moments(L, kp))
    return kp, R.reshape(-1)[kp], bins, describe(L, kp, bins), R


def model(planes, channels, cell, per_cell, min_response):
    """planes: P x H x W (x 4) u8.  -> counts (P int32), points (P x n_slots x 2 uint32: float32 words), desc (P x n_slots x 32 u8),
    info (P x n_slots INFO), each with the header's padding; `responses` keeps the R planes for the tests that need a threshold."""
    planes = np.asarray(planes)
    P, H, W = planes.shape[:3]
    _, _, n_slots = layout(W, H, cell, per_cell)
    counts = np.zeros(P, np.int32)
    points = np.full((P, n_slots, 2), PAD_WORD, np.uint32)
    desc = np.zeros((P, n_slots, 32), np.uint8)
    info = np.zeros((P, n_slots), INFO)
    info["bin"] = -1
    info["idx"] = -1
    resp = []
    for p in range(P):
        kp, r, bins, d, R = model_plane(planes[p], channels, cell, per_cell, min_response)
        n = len(kp)
        counts[p] = n
        points[p, :n, 0] = (kp % W).astype(np.float32).view(np.uint32)
        points[p, :n, 1] = (kp // W).astype(np.float32).view(np.uint32)
        desc[p, :n] = d
        info["R"][p, :n], info["bin"][p, :n], info["idx"][p, :n] = r, bins, kp
        resp.append(R)
    return SimpleNamespace(counts=counts, points=points, desc=desc, info=info, responses=resp, n_slots=n_slots)


# ------------------------------------------------------------------------------------------------ case builders (H x W u8 planes)
def _blur(a):
    p = np.pad(a.astype(np.int64), 1, mode="edge")
    return ((_box(p, 1) + 4) // 9).astype(np.uint8)


def scene(seed, W, H, rects=None, side=None):
    """Seeded rectangles of random grey (sides 4 .. side, by default a third of the plane) on a mid-grey ground, blurred once: many corners."""
    rng = np.random.default_rng(seed)
    a = np.full((H, W), 96, np.uint8)
    for _ in range(rects if rects is not None else max(6, W * H // 300)):
        w, h = int(rng.integers(4, side or max(6, W // 3))), int(rng.integers(4, side or max(6, H // 3)))
        x, y = int(rng.integers(-w // 2, W)), int(rng.integers(-h // 2, H))
        a[max(y, 0):y + h, max(x, 0):x + w] = rng.integers(0, 256)
    return _blur(a)


def noise(seed, W, H):
    return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)


def constant(W, H, v=137):
    return np.full((H, W), v, np.uint8)


def checker(W, H, lo=40, hi=210):
    y, x = np.mgrid[0:H, 0:W]
    return np.where(((x // 4) + (y // 4)) % 2 == 0, lo, hi).astype(np.uint8)


def margin_corners(W=80, H=80):
    """Black, with white 12 x 12 squares.  The response of a square's corner peaks two pixels inside it (quadrant()), so the squares are set
    so that corner peaks fall ON the margin and one pixel outside it:
      A at (14, 14): peak (16, 16), kept;              B at x 13, y 40: peak (15, 42), refused for x;   C at x 40, y 13: peak (42, 15), refused for y;
      D ending at (W - 15, H - 15): peak (W - 17, H - 17), the last legal position, kept;   E ending at x W - 14: peak x = W - 16, refused."""
    a = np.zeros((H, W), np.uint8)
    a[14:26, 14:26] = 255
    a[40:52, 13:25] = 255
    a[13:25, 40:52] = 255
    a[H - 26:H - 14, W - 26:W - 14] = 255
    a[H - 52:H - 40, W - 25:W - 13] = 255
    return a


def quadrant(first=14, W=33, H=33):
    """Black except for a white quadrant x >= first and y >= first.  The 7 x 7 window puts the peak of R two pixels inside the white, on the
    diagonal: at (first + 2, first + 2)."""
    a = np.zeros((H, W), np.uint8)
    a[first:, first:] = 255
    return a


def to_rgba(plane, seed=0):
    """A 4-channel plane whose luma differs from every channel: R, G, B are the plane under three different point maps, alpha is noise."""
    rng = np.random.default_rng(1000 + seed)
    p = np.asarray(plane)
    out = np.empty(p.shape + (4,), np.uint8)
    out[..., 0] = p
    out[..., 1] = 255 - p
    out[..., 2] = (p.astype(np.int64) * 3 // 4 + 17).astype(np.uint8)
    out[..., 3] = rng.integers(0, 256, p.shape, dtype=np.uint8)
    return out


def check(got, want, what, skip=()):
    """Byte-for-byte comparison of a result (counts, points as uint32 words, desc rows' first 32 bytes, info) with the model."""
    assert got.counts.tolist() == want.counts.tolist(), (what, "counts", got.counts.tolist(), want.counts.tolist())
    for k in ("points", "desc", "info"):
        if k in skip:
            continue
        g, w = getattr(got, k), getattr(want, k)
        if not np.array_equal(g, w):
            bad = np.argwhere(np.asarray(g != w).reshape(g.shape[0], g.shape[1], -1).any(-1))
            p, s = bad[0]
            raise AssertionError((what, k, f"{len(bad)} slots differ; first plane {p} slot {s}", g[p, s].tolist(), w[p, s].tolist(), int(want.counts[p])))


# ------------------------------------------------------------------------------------------------ the host check's files (tests/cpp/detect_check.cpp)
def pack_planes(planes, slack=0, fill=0xFF):
    """P planes back to back with `slack` bytes of `fill` behind each but the last: (bytes, plane_stride_bytes)."""
    planes = np.ascontiguousarray(planes, np.uint8)
    P = planes.shape[0]
    flat = planes.reshape(P, -1)
    out = np.full((P, flat.shape[1] + slack), fill, np.uint8)
    out[:, :flat.shape[1]] = flat
    raw = out.tobytes()
    return (raw[:len(raw) - slack] if slack else raw), flat.shape[1] + slack


def host_case(planes, channels, cell, per_cell, min_response, desc_stride=32, want=7, slack=0):
    import struct
    planes = np.asarray(planes)
    P, H, W = planes.shape[:3]
    raw, _ = pack_planes(planes, slack)
    return struct.pack("<10iq", W, H, P, channels, cell, per_cell, desc_stride, want, slack, 0, int(min_response)) + raw


def unpack(raw, P, n_slots, desc_stride):
    """The four outputs as the host check (and the GPU test) leave them: counts, points as words, the first 32 bytes of the descriptor rows, info;
    `rest` = the bytes 32..desc_stride of the rows."""
    o = 0
    counts = np.frombuffer(raw, np.int32, P, o); o += 4 * P
    points = np.frombuffer(raw, np.uint32, P * n_slots * 2, o).reshape(P, n_slots, 2); o += 8 * P * n_slots
    rows = np.frombuffer(raw, np.uint8, P * n_slots * desc_stride, o).reshape(P, n_slots, desc_stride); o += P * n_slots * desc_stride
    info = np.frombuffer(raw, INFO, P * n_slots, o).reshape(P, n_slots); o += 16 * P * n_slots
    assert o == len(raw)
    return SimpleNamespace(counts=counts, points=points, desc=rows[:, :, :32], rest=rows[:, :, 32:], info=info)


def filled(a, byte=0xA5):
    return bool((np.ascontiguousarray(a).view(np.uint8) == byte).all())


# ------------------------------------------------------------------------------------------------ the chain's pictures
def _bilinear(img, x, y):
    """img (H x W u8) sampled at float64 positions inside it, rounded to u8."""
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    fx, fy = x - x0, y - y0
    a = img.astype(np.float64)
    v = (a[y0, x0] * (1 - fx) + a[y0, x0 + 1] * fx) * (1 - fy) + (a[y0 + 1, x0] * (1 - fx) + a[y0 + 1, x0 + 1] * fx) * fy
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)


def _apply(M, x, y):
    w = M[2, 0] * x + M[2, 1] * y + M[2, 2]
    return (M[0, 0] * x + M[0, 1] * y + M[0, 2]) / w, (M[1, 0] * x + M[1, 1] * y + M[1, 2]) / w


CHAIN = dict(scene=(420, 380), key=(220, 180), key_off=(100, 100), frame=(192, 160), cell=16, per_cell=2, min_response=10 ** 10,
             threshold=1.5, n_hyp=512, fit_seed=7)
CHAIN_SEED = 4                                                    # (of the seeds 1..6 the one whose model chain meets chain_is_good)


def chain_case(seed):
    """A seeded scene, a keyframe crop of it and three frames resampled from it on the CPU (bilinear): an integer shift, a rotation of 20
    degrees, a rotation of 30 degrees with a mild perspective.  -> (key H x W u8, frames 3 x h x w u8, truth 3 x (3 x 3): frame pixel -> key pixel)."""
    SW, SH = CHAIN["scene"]
    kw, kh = CHAIN["key"]
    kx, ky = CHAIN["key_off"]
    w, h = CHAIN["frame"]
    sc = scene(seed, SW, SH, rects=2500, side=28)
    key = sc[ky:ky + kh, kx:kx + kw].copy()
    cx, cy = kx + kw / 2.0, ky + kh / 2.0                         # the frames look at the middle of the keyframe

    def about(angle, px=0.0, py=0.0, dx=0.0, dy=0.0):
        c, s = np.cos(np.radians(angle)), np.sin(np.radians(angle))
        to0 = np.array([[1, 0, -w / 2.0], [0, 1, -h / 2.0], [0, 0, 1]])
        rot = np.array([[c, -s, 0], [s, c, 0], [px, py, 1]])
        back = np.array([[1, 0, cx + dx], [0, 1, cy + dy], [0, 0, 1]])
        return back @ rot @ to0                                   # frame pixel -> scene position

    to_scene = [np.array([[1.0, 0, kx + 9], [0, 1.0, ky + 13], [0, 0, 1]]), about(20.0, dx=3.0, dy=-2.0), about(30.0, 2e-4, -1.5e-4, dx=-2.0, dy=4.0)]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    frames, truth = [], []
    for M in to_scene:
        sx, sy = _apply(M, xx, yy)
        assert sx.min() >= 0 and sy.min() >= 0 and sx.max() < SW - 1 and sy.max() < SH - 1
        frames.append(_bilinear(sc, sx, sy))
        truth.append(np.array([[1, 0, -kx], [0, 1, -ky], [0, 0, 1.0]]) @ M)
    return key, np.stack(frames), np.stack(truth)


def chain_is_good(frames, truth, wm, wt):
    """The condition on the chain's inputs, on the MODEL's results alone (wm: the match model's, wt: the fit model's without a refit): every
    frame has at least 30 accepted matches, at least 70 % of them lie within 1.5 px of the true transform, and the fitted matrix maps the
    frame's corners within 2 px of the truth.  -> per frame (matches, of them within 1.5 px, inliers of the fit, corner error)."""
    h, w = frames.shape[1:3]
    cs = np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]], np.float64)
    out = []
    for f in range(len(frames)):
        n = int(wm.counts[f])
        mt = wm.matches[f, :n].view(np.float32).astype(np.float64)
        tx, ty = _apply(truth[f], mt[:, 0], mt[:, 1])
        near = int((np.hypot(tx - mt[:, 2], ty - mt[:, 3]) <= 1.5).sum())
        M = np.append(wt.min_mats[f], 1.0).reshape(3, 3)
        ax, ay = _apply(M, cs[:, 0], cs[:, 1])
        bx, by = _apply(truth[f], cs[:, 0], cs[:, 1])
        err = float(np.hypot(ax - bx, ay - by).max())
        assert n >= 30 and near >= 0.7 * n and err <= 2.0, (f, n, near, err, "choose another seed")
        out.append((n, near, int(wt.counts[f]), err))
    return out
