"""Piecewise FORWARD frames under turns, mirrors, shears and slopes, for the tile kernels k_fwd_pw_bins + k_fwd_pw_tiles, and a numpy model
of k_fwd_pw_bins.  CPU only; the cases keep the shape of fwd_edges' piecewise cases ({name, sp, tris, dp, W, H, seed, geom, msx, msy, Mx, My,
kernel, flagged}), and tests/test_forward_turns_cpu.py checks the builders and the model before either judges a kernel.

What the cases aim at, by step of k_fwd_pw_tiles:
  (0) the source rows of a tile's pre-image under each entry's 2 x 2 matrix: det < 0 (T1 mirrors), oblique turns where m1 dx matters (T1),
      |det| from 1.5e-5 down to 1.4e-20 on both signs, through the evaluation-error guard and past it (T3);
  (1) the four half-planes a[j] x + b[j] >= 0, a = {m0, -m0, m1, -m1}: every sign pattern (T1), |a[j]| on both sides of the 1e-9 switch with
      both signs in one frame (T2);
  (2) the owner test and the last writer by (map row, map column): Math.round ties on every writer, folded rows and columns (T1 180 degrees),
      aliasing writers k = +-1 of an oblique triangle (T1 twin).
T4 puts six such frames into one launch; T5 draws them at random."""
import numpy as np

from . import oracle as O
from .fwd_edges import (PW_CAP0, PW_ENTRY_MAX, PW_SHIFT_MAX, TILE, _dst_geom, _grid, _p, apply_affine, classify_piecewise,  # noqa: F401
                        expected_piecewise, image, piecewise_maps, piecewise_oracle, rank_image)

PW_IMAGE_MAX, PW_PAD, PW_WIDTH_MAX = 1.0e7, 2, 1 << 24         # k_fwd_pw_bins: |corner image|, exclusive; padding of the bounds; window width
SLOPE_SWITCH = 1.0e-9                                          # k_fwd_pw_tiles step (1): |a[j]| below this is "no slope"
SHIFT = np.float64([300.5, 300.5])                             # T1: half-integer, so that an axis-aligned frame makes every writer a tie


# ------------------------------------------------------------------------------------------------ k_fwd_pw_bins, written again

def bins_model(case, maps=None):
    """(flag, max_entries, shifts): what k_fwd_pw_bins does with the frame.  flag: None, "fallback" (a triangle it cannot bound: the frame
    is redone through scatter + gather) or "overflow" (a tile with more than PW_CAP0 entries: the same, at the first capacity);
    max_entries: the most (triangle, k) entries filed under one 64 x 64 output tile; shifts: the set of aliasing shifts k filed."""
    fmap, fwd = piecewise_maps(case) if maps is None else maps
    xo, yo, ow, oh = case["geom"]
    if ow <= 0 or oh <= 0:
        return None, 0, set()
    mh, mw = fmap.shape
    ids = fmap.ravel().astype(np.int64)
    cells = np.flatnonzero((ids >= 0) & (ids < fwd.shape[0]))                                   # k_fmap_bbox: cur >= 0 && cur < T
    owners, inv = np.unique(ids[cells], return_inverse=True)
    box = np.empty((4, owners.size), np.int64)                                                   # cx0, cy0, cx1, cy1: from the map itself
    for row, (coord, fn, start) in enumerate(((cells % mw, np.minimum, mw), (cells // mw, np.minimum, mh),
                                              (cells % mw, np.maximum, -1), (cells // mw, np.maximum, -1))):
        box[row] = start
        fn.at(box[row], inv, coord)
    counts = np.zeros(((oh + TILE - 1) // TILE, (ow + TILE - 1) // TILE), np.int64)
    fallback, shifts = ow > PW_WIDTH_MAX, set()
    for i, t in enumerate(owners):
        m = fwd[t].astype(np.float64)
        bad = ow > PW_WIDTH_MAX or not bool(np.all(np.abs(m) <= PW_ENTRY_MAX))                   # (NaN fails the comparison, as on the device)
        x = np.float64([box[0, i], box[2, i], box[0, i], box[2, i]]) + case["msx"]
        y = np.float64([box[1, i], box[1, i], box[3, i], box[3, i]]) + case["msy"]
        with np.errstate(all="ignore"):
            fx, fy = apply_affine(m, x, y)
            if not bool(np.all((np.abs(fx) < PW_IMAGE_MAX) & (np.abs(fy) < PW_IMAGE_MAX))):
                bad = True
        if bad:
            fallback = True
            continue
        u, v = fx - float(xo), fy - float(yo)
        ua, ub = int(np.floor(u.min())) - PW_PAD, int(np.ceil(u.max())) + PW_PAD
        va, vb = int(np.floor(v.min())) - PW_PAD, int(np.ceil(v.max())) + PW_PAD
        kmin, kmax = ua // ow, ub // ow                                                          # (Python's // floors, like floordiv64)
        if kmin < -PW_SHIFT_MAX or kmax > PW_SHIFT_MAX:
            fallback = True
            continue
        for k in range(kmin, kmax + 1):
            c0, c1 = max(ua, k * ow) - k * ow, min(ub, (k + 1) * ow - 1) - k * ow
            r0, r1 = max(va + k, 0), min(vb + k, oh - 1)
            if c0 > c1 or r0 > r1:
                continue
            counts[r0 // TILE:r1 // TILE + 1, c0 // TILE:c1 // TILE + 1] += 1
            shifts.add(k)
    most = int(counts.max())
    return ("fallback" if fallback else "overflow" if most > PW_CAP0 else None), most, shifts


def dets(fwd):
    f = np.asarray(fwd, np.float64)
    return f[:, 0] * f[:, 3] - f[:, 2] * f[:, 1]


# ------------------------------------------------------------------------------------------------ T1: rigid motions, mirrors, shears

def _rot(deg):
    exact = {0: (1.0, 0.0), 90: (0.0, 1.0), 180: (-1.0, 0.0), 270: (0.0, -1.0)}
    c, s = exact[deg] if deg in exact else (np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg)))
    return np.float64([[c, -s], [s, c]])


MIRROR_X, MIRROR_Y = np.diag([-1.0, 1.0]), np.diag([1.0, -1.0])
RIGID = {"turn_180": _rot(180), "turn_270": _rot(270), "mirror_x": MIRROR_X, "mirror_y": MIRROR_Y, "transpose": np.float64([[0, 1], [1, 0]]),
         "turn_30": _rot(30), "turn_45": _rot(45), "turn_60": _rot(60), "turn_135_mirror_x": _rot(135) @ MIRROR_X,
         "shear_x_2": np.float64([[1, 2], [0, 1]]), "shear_y_-2": np.float64([[1, 0], [-2, 1]])}
AXIS_ALIGNED = ("turn_180", "turn_270", "mirror_x", "mirror_y", "transpose")
MIRRORED = ("mirror_x", "mirror_y", "transpose", "turn_135_mirror_x")
OBLIQUE = ("turn_30", "turn_45", "turn_60")
NARROW = 40


def rigid():
    """T1: destination = s A^T + (300.5, 300.5) on a 4 x 3 grid over a 256 x 192 source, the window the destination's own box (the bins
    kernel's +-2 padding files k = -1 and k = 1 beside k = 0); the 45 degree turn again in a window 40 columns narrower on each side."""
    s, tris = _grid(0, 0, 256, 192, 4, 3)
    out = []
    for name, A in RIGID.items():
        d = s @ A.T + SHIFT
        out.append(_p(name, s, tris, d, 256, 192, _dst_geom(d), 91))
    d = s @ RIGID["turn_45"].T + SHIFT
    g = _dst_geom(d)
    out.append(_p("turn_45_narrow", s, tris, d, 256, 192, (g[0] + NARROW, g[1], g[2] - 2 * NARROW, g[3]), 91))
    return out


# ------------------------------------------------------------------------------------------------ T2: the slope switch of step (1)

SLOPE_M0_V, SLOPE_M1_V = (0.0625, 0.25, 0.5, 1.5, 3.0), (0.0625, 0.5, 1.5)
SLOPE_VERTEX = 7                                               # source (128, 64) of the 4 x 3 grid on 256 x 192


def _ulp(d, vertex, axis, up):
    d = d.astype(np.float32)
    d[vertex, axis] = np.nextafter(d[vertex, axis], np.float32(np.inf if up else -np.inf))
    return d


def slope_switch():
    """T2: a 90 degree turn d = (64 + v - s_y, s_x + 0.5): vertex 7 has destination x = v, moved by one f32 ulp up or down, so that the
    triangles around it get m0 = +-ulp(v) / 64 (opposite signs on either side of the vertex) and every other triangle keeps m0 == 0;
    the same for m1 on the shift d = (s_x + 0.5, s_y - 64 + v) with destination y of vertex 7 moved; and the two m0 cases nearest the
    switch with the destination mirrored in y (m1 = -1, det < 0 beside the tiny m0)."""
    s, tris = _grid(0, 0, 256, 192, 4, 3)
    assert tuple(s[SLOPE_VERTEX]) == (128.0, 64.0)
    out = []
    for v in SLOPE_M0_V:
        d = np.stack([64.0 + v - s[:, 1], s[:, 0] + 0.5], -1)
        for up in (True, False):
            d1 = _ulp(d, SLOPE_VERTEX, 0, up)
            out.append(_p(f"slope_m0_{v:g}_{'up' if up else 'down'}", s, tris, d1, 256, 192, _dst_geom(d1), 92, slope=(0, v)))
        if v in (0.5, 1.5):
            d1 = _ulp(d, SLOPE_VERTEX, 0, True) * np.float32([1, -1])
            out.append(_p(f"slope_m0_{v:g}_up_mirror_y", s, tris, d1, 256, 192, _dst_geom(d1), 92, slope=(0, v)))
    for v in SLOPE_M1_V:
        d = np.stack([s[:, 0] + 0.5, s[:, 1] - 64.0 + v], -1)
        for up in (True, False):
            d1 = _ulp(d, SLOPE_VERTEX, 1, up)
            out.append(_p(f"slope_m1_{v:g}_{'up' if up else 'down'}", s, tris, d1, 256, 192, _dst_geom(d1), 92, slope=(1, v)))
    return out


# ------------------------------------------------------------------------------------------------ T3: the guard of step (0)

GUARD_E, GUARD_MIRRORED_E = (10, 20, 30, 36, 40, 44, 50, 60), (36, 44, 60)


def _flat(s, stride, e):
    """s + (3.5, 0) with the first vertex of the second row put 2^-e above the middle of the first cell's top edge: triangle 0 = (0, 1,
    stride) has |det| = 2^-e / (cell height), triangle 1 = (1, stride + 1, stride) is a sliver of the same grading."""
    d = s + [3.5, 0.0]
    d[stride] = (d[0] + d[1]) / 2 + [0.0, 2.0 ** -e]
    return d


def guard():
    """T3: fwd_edges.collapsed()'s 4 x 2 grid on 256 x 128; |det| of triangle 0 is 2^-e / 64 for e = 10 .. 60: the pre-image of a tile
    is trusted, then refused by the evaluation-error guard, with finite matrices throughout; e = 36, 44, 60 again mirrored in y (det < 0,
    the same magnitudes), in a window one row taller than the destination's box so that the flat triangle's writers land in it."""
    s, tris = _grid(0, 0, 256, 128, 4, 2)
    out = []
    for e in GUARD_E:
        d = _flat(s, 5, e)
        out.append(_p(f"guard_2^-{e}", s, tris, d, 256, 128, _dst_geom(d), 93, guard_e=e))
        if e in GUARD_MIRRORED_E:
            dm = d * [1.0, -1.0]                          # the flat triangle lies in (-1, 0] and rounds to row 0: one row below the box
            g = _dst_geom(dm)
            out.append(_p(f"guard_2^-{e}_mirror_y", s, tris, dm, 256, 128, (g[0], g[1], g[2], g[3] + 1), 93, guard_e=e))
    return out


def named_cases():
    return {c["name"]: c for c in rigid() + slope_switch() + guard()}


# ------------------------------------------------------------------------------------------------ T4: a batch

def turns_batch():
    """T4: one 6 x 3 mesh on 192 x 96, six frames in one launch (identity + 0.5, 180 degrees, mirror in x, 45 degrees, 90 degrees with an
    ulp slope, a flat triangle of T3), each in its own destination box; three sources, frame f reads source f mod 3."""
    s, tris = _grid(0, 0, 192, 96, 6, 3)
    turn = np.stack([32.25 - s[:, 1], s[:, 0] + 0.5], -1)                                       # vertex 9 = source (64, 32): destination x = 0.25
    assert tuple(s[9]) == (64.0, 32.0)
    ds = [s + [0.5, 0.5], s @ _rot(180).T + SHIFT, s @ MIRROR_X.T + SHIFT, s @ _rot(45).T + SHIFT, _ulp(turn, 9, 0, True), _flat(s, 7, 36)]
    frames = []
    for d in ds:
        d = np.ascontiguousarray(d, np.float32).ravel()
        frames.append((d, _dst_geom(d)))
    return {"sp": s.astype(np.float32).ravel(), "tris": tris, "W": 192, "H": 96, "box": (0, 0, 192, 96), "frames": frames, "seeds": [94, 95, 96]}


def batch_cases(b):
    box = b["box"]
    return [{"name": f"batch{f}", "sp": b["sp"], "tris": b["tris"], "dp": d, "W": b["W"], "H": b["H"], "msx": box[0], "msy": box[1], "Mx": box[2],
             "My": box[3], "geom": g} for f, (d, g) in enumerate(b["frames"])]


# ------------------------------------------------------------------------------------------------ T5: fuzz

FUZZ_SIZES = [(96, 64), (140, 100), (70, 200), (256, 64), (200, 130), (64, 64)]
FUZZ_PIXELS_MAX = 400_000


def fuzz(seed, n):
    """T5: n draws in the manner of fwd_edges.fuzz (G9) for piecewise frames: every multiple of 90 degrees and random angles, anisotropic
    scales, sx negated on every 3rd draw, and by mode = trial % 7: 2 a nearly rank-deficient matrix, 3 .. 5 jittered vertices, 5 also a
    shuffled triangle order and a fold, 6 a narrowed window.  Returns (cases, draws dropped); cases carry `ang`, `mode` and `A`."""
    rng = np.random.default_rng(seed)
    out, dropped = [], 0
    for trial in range(n):
        W, H = FUZZ_SIZES[trial % len(FUZZ_SIZES)]
        mode = trial % 7
        nx, ny = int(rng.integers(1, 7)), int(rng.integers(1, 6))
        s, tris = _grid(0, 0, W, H, nx, ny)
        if trial % 4 == 0: s = s * 0.9 + [0.05 * W, 0.05 * H]                                  # inside the image: minima > 0
        if trial % 5 == 0: s = (s - [W / 2, H / 2]) * 1.05 + [W / 2, H / 2]                    # past it on every side: off-image writers
        ang = float(rng.choice([0, np.pi / 2, np.pi, -np.pi / 2, rng.uniform(-3.2, 3.2)]))
        sx, sy = 10 ** rng.uniform(-0.6, 0.45, 2)
        if trial % 3 == 0: sx = -sx
        A = np.array([[np.cos(ang) * sx, -np.sin(ang) * sy], [np.sin(ang) * sx, np.cos(ang) * sy]])
        if mode == 2: A[1] = A[0] * rng.uniform(0.5, 2) + rng.uniform(-1, 1, 2) * 10 ** rng.uniform(-9, -2)
        p = s.copy()
        if mode in (3, 4, 5):
            p = p + rng.uniform(-0.45, 0.45, p.shape) * [W / nx, H / ny]
        if mode == 5:
            tris = tris.reshape(-1, 3)[rng.permutation(tris.size // 3)].ravel()
            p[int(rng.integers(0, p.shape[0]))] += rng.choice([-40.0, 40.0], 2)
        t = np.floor(rng.uniform(-300, 300, 2)) + rng.choice([0, 0.5, 0.25, rng.uniform()])
        d = p @ A.T + t
        geom = _dst_geom(d)
        if mode == 6 and geom[2] > 200:
            a, b = int(rng.integers(1, 40)), int(rng.integers(1, 40))
            geom = (geom[0] + a, geom[1], geom[2] - a - b, geom[3])
        if geom[2] <= 0 or geom[3] <= 0 or geom[2] * geom[3] > FUZZ_PIXELS_MAX:
            dropped += 1
            continue
        out.append(_p(f"fuzz{trial}", s, tris, d, W, H, geom, 6000 + trial, ang=ang, mode=mode, A=A))
    return out, dropped


def oblique(case):
    """More than 0.1 rad from every multiple of 90 degrees."""
    r = abs(case["ang"]) % (np.pi / 2)
    return min(r, np.pi / 2 - r) > 0.1


def fuzz_census(case, maps=None):
    """What a draw exercises: (flag, max_entries, shifts) of the bins model, and whether every triangle is mirrored, the frame is
    oblique, has landing writers at k = +-1, has a triangle with |det| < 1e-6."""
    maps = piecewise_maps(case) if maps is None else maps
    flag, most, shifts = bins_model(case, maps)
    counts, win, sidx = classify_piecewise(case, maps)
    det = dets(maps[1])
    return {"flag": flag, "entries": most, "shifts": shifts, "mirrored": bool((det < 0).all()), "oblique": oblique(case),
            "aliasing": counts["shift"][-1] + counts["shift"][1] > 0, "near_singular": bool((np.abs(det) < 1e-6).any())}, (counts, win, sidx)
