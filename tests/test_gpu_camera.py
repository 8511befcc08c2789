"""The camera models on the GPU against the numpy model of tests/hgtest/camera.py (written from the header's text; pinned by
tests/test_camera_cpu.py).  Shapes are the smallest at which the kernels can go wrong: a handful of frames whose cameras differ, windows
around the 256-column piece and around the band of rows (its height read from hg_camera_dev.h), point lists around the wave's 64 lanes.

Tolerance of canvas -> source (derived, not measured).  v = the model's longdouble value; the device's float32 must lie between
float32(v - delta) and float32(v + delta), and a coverage decision may differ from the model's only where sx, sy, c.z or r2 lies within its
delta of its bound -- at most 0.1 % of any frame (tests/test_camera_cpu.py shows on the model that this file's fixtures have none).  delta is
the first-order bound of the chain with e = 2^-52 per elementary operation and 4 e for sin and cos, written d(.) below, |.| taken of every
factor (tests/hgtest/camera.py, delta):
    d(a) = 2 e |a|  (the subtraction and the division);  d(sin a), d(cos a) = d(a) + 4 e;  on the plane d(a) alone and nothing for the 1
    d(b), d(sin b), d(cos b) alike, on the sphere only with the 4 e
    ray (x, y, z) = (sa cb, yb, ca cb):  d(x) = cb d(sa) + sa d(cb) + e x,  d(y) = d(yb),  d(z) = cb d(ca) + ca d(cb) + e z
    c_i = (r_i0 x + r_i1 y) + r_i2 z:  d(c_i) = sum_j r_ij d(ray_j) + 3 e sum_j |r_ij ray_j|     (a product and two sums over every term)
    xn = c_0 / c_2:  d(xn) = (d(c_0) + xn d(c_2)) / c_2 + e xn;  yn alike
    r2 = xn xn + yn yn:  d(r2) = 2 xn d(xn) + 2 yn d(yn) + 2 e r2
    rad = 1 + r2 (k1 + r2 (k2 + r2 k3)):  d(rad) = (k1 + 2 k2 r2 + 3 k3 r2^2) d(r2) + 6 e (1 + r2 (k1 + r2 (k2 + r2 k3)))
    tx = ((2 p1) xn) yn + p2 (r2 + (2 xn) xn):  d(tx) = 2 p1 (yn d(xn) + xn d(yn)) + p2 (d(r2) + 4 xn d(xn)) + 4 e (2 p1 xn yn + p2 (r2 + 2 xn^2)); ty alike
    xd = xn rad + tx:  d(xd) = rad d(xn) + xn d(rad) + d(tx) + 2 e (xn rad + tx)
    sx = fx xd + cx:  delta = fx d(xd) + 2 e (fx xd + cx);  sy alike;  d(c.z) = d(c_2) and d(r2) excuse the two other tests.
On this file's fixtures delta is some 1e-13 to 1e-11 px, a millionth of a float32 ulp of the coordinates: the stored value is float32(v) or
its neighbour.  The largest |device - model| / delta of this file is printed at teardown: it is the float32 rounding over delta, 7.96e7 on an
MI355X, where 0 of the 377 234 stored coordinates were not float32(v) (EXPERIMENTS.md, "Camera").

Round trip to-canvas(to-source(p)) of the point lists (derived; checked on the model in tests/test_camera_cpu.py, round_trip_bound).  The
source position s reaches the second call as a float32: e_s = 2^-24 |s| + f 1e-9 + delta per coordinate (its rounding; what the fixed-point
inverse of the distortion may leave, 1e-9 in normalised units, in pixels; the first call's own error).  Through the local magnification J of
source -> canvas (central differences of the model, step 1e-3 px; 1 % allowed for the second order) that is |J| e_s; the result is rounded to
float32 once more, 2^-24 |p|; the float64 arithmetic of source -> canvas adds 64 e (|p| + pi scale)."""
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "homography.js_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hgwarp as HG                          # noqa: E402
from hgtest import camera as CM              # noqa: E402
from hgtest import gpu_frames as GF          # noqa: E402
from hgtest.gpu_frames import FILL, INVALID  # noqa: E402
import test_camera_cpu as TC                 # noqa: E402  (limit_cases, covered_outside, round_trip_bound, round_trip_points, check_to_canvas)

pytestmark = pytest.mark.gpu
IX, CO = HG.FIELD_INDEX, HG.FIELD_COORDS
TAIL = 256                                   # canary bytes behind every output
W, H = CM.SRC_W, CM.SRC_H
SURFACES = (CM.PLANE, CM.CYLINDER, CM.SPHERE)
CSRC = os.path.join(ROOT, "homography.js_amd", "csrc")
BAND = int(re.search(r"kCamBandRows = (\d+);", open(os.path.join(CSRC, "hg_camera_dev.h")).read()).group(1))


@pytest.fixture(scope="module")
def ctx():
    c = HG.Context(0)
    yield c
    c.close()
    print(f"largest |device - model| / delta of this file: {CM.WORST[0]:.3g}; {CM.STORED[1]} of {CM.STORED[0]} stored coordinates are not float32(model); "
          f"{CM.EXCUSED[0]} decisions differ from the model's")


# ------------------------------------------------------------------------------------------------ run
def upload_records(ctx, recs):
    recs = np.ascontiguousarray(recs, np.float64).reshape(-1, CM.RECORD)
    d_r = ctx.alloc(max(recs.nbytes, 8))
    if recs.nbytes:
        ctx.to_device(d_r, recs.view(np.uint8).ravel())
    return d_r, recs


def field(ctx, recs, geoms, fmt, surface, canvas=CM.CANVAS, offs=None, w=W, h=H):
    """The field of the cameras into an allocation full of FILL; every byte outside the frames must still be FILL afterwards and the records
    must be unwritten.  Returns the per-frame bytes."""
    px = 4 if fmt == IX else 8
    fo = list(offs) if offs is not None else HG.pack_field_offsets(geoms, fmt)[0]
    assert offs is not None or fo == CM.pack256(geoms, px)[0]
    total = max([o + max(g[2], 0) * max(g[3], 0) * px for o, g in zip(fo, geoms)] + [0]) + TAIL
    d_r, recs = upload_records(ctx, recs)
    d_f = ctx.alloc(total)
    try:
        ctx.to_device(d_f, np.full(total, FILL, np.uint8))
        ctx.field_camera_frames_device(d_r, geoms, w, h, surface, *canvas, fmt, d_f, field_offsets=offs)
        ctx.sync()
        raw = ctx.to_host(d_f, total)
        if recs.nbytes:
            assert np.array_equal(ctx.to_host(d_r, recs.nbytes), recs.view(np.uint8).ravel()), "the records must not be written"
    finally:
        ctx.free(d_f)
        ctx.free(d_r)
    untouched = np.ones(total, bool)
    frames = []
    for o, g in zip(fo, geoms):
        k = max(g[2], 0) * max(g[3], 0) * px
        untouched[o:o + k] = False
        frames.append(raw[o:o + k].copy())
    assert (raw[untouched] == FILL).all(), "bytes between the frames, the padding and the tail must not be written"
    return frames


def points(ctx, recs, surface, pts, to_source, canvas=CM.CANVAS):
    pts = np.ascontiguousarray(pts, np.float32)
    n_sets, n_pts = pts.shape[0], pts.shape[1]
    d_r, recs = upload_records(ctx, recs)
    n_frames = recs.shape[0]
    out_b = n_frames * n_pts * 8
    d_p, d_o = ctx.alloc(max(pts.nbytes, 8)), ctx.alloc(out_b + TAIL)
    try:
        if pts.nbytes:
            ctx.to_device(d_p, pts.view(np.uint8).ravel())
        ctx.to_device(d_o, np.full(out_b + TAIL, FILL, np.uint8))
        fn = ctx.points_camera_to_source_frames_device if to_source else ctx.points_camera_to_canvas_frames_device
        fn(d_r, n_frames, surface, *canvas, d_p, n_pts, n_sets, d_o)
        ctx.sync()
        raw = ctx.to_host(d_o, out_b + TAIL)
        if pts.nbytes:
            assert np.array_equal(ctx.to_host(d_p, pts.nbytes), pts.view(np.uint8).ravel()), "the inputs must not be written"
    finally:
        for p in (d_r, d_p, d_o):
            ctx.free(p)
    assert (raw[out_b:] == FILL).all(), "the canary behind the point results"
    return raw[:out_b].view(np.float32).reshape(n_frames, n_pts, 2).copy()


def check_frames(frames, recs, geoms, fmt, surface, canvas=CM.CANVAS, w=W, h=H, what=""):
    for f, g in enumerate(geoms):
        px = 4 if fmt == IX else 8
        assert frames[f].size == max(g[2], 0) * max(g[3], 0) * px
        if frames[f].size:
            CM.check_field_frame(frames[f], recs[f], g, w, h, surface, *canvas, fmt == IX, (what, surface, fmt, f))


# ------------------------------------------------------------------------------------------------ the field's shapes
@pytest.mark.parametrize("distort", [False, True])
@pytest.mark.parametrize("surface", SURFACES)
@pytest.mark.parametrize("fmt", [IX, CO])
def test_windows_around_the_piece_and_the_band_with_gaps_between_the_frames(ctx, fmt, surface, distort):
    geoms = CM.windows(BAND)                                 # widths 1, 3, 255, 256, 257, 513; heights 1, band - 1, band, band + 1; an empty frame
    recs = CM.cameras(len(geoms), distort)
    frames = field(ctx, recs, geoms, fmt, surface)
    check_frames(frames, recs, geoms, fmt, surface, what="packed")
    # caller-given offsets: another order, gaps of odd sizes (multiples of the pixel size), which must keep their bytes
    px = 4 if fmt == IX else 8
    offs, o = [0] * len(geoms), 24
    for f in (4, 2, 6, 0, 5, 3, 1):
        offs[f] = o
        o += max(geoms[f][2], 0) * max(geoms[f][3], 0) * px + 8 * (f + 1)
    moved = field(ctx, recs, geoms, fmt, surface, offs=offs)
    for f in range(len(geoms)):
        assert np.array_equal(frames[f], moved[f]), (fmt, surface, f, "the same values wherever the frame is put")
    if fmt == CO:
        cov = sum(int((~np.isnan(fr.view(np.float32))).sum()) // 2 for fr in frames)
        n = sum(g[2] * g[3] for g in geoms if g[2] > 0)
        assert 0.05 * n < cov < 0.95 * n, (cov, n)           # the coverage test decides in both directions


@pytest.mark.parametrize("surface", SURFACES)
def test_large_offsets_heights_around_two_bands_and_no_work(ctx, surface):
    big = 1 << 26
    geoms = [(big - 64, -big, 64, 3), (-big, big - 2 * BAND - 1, 5, 2 * BAND + 1), (-60, -30, 260, 2 * BAND - 1), (0, 0, 4, 2 * BAND), (70000, -30, 33, 5)]
    recs = CM.cameras(len(geoms), True)
    for fmt in (IX, CO):
        check_frames(field(ctx, recs, geoms, fmt, surface), recs, geoms, fmt, surface, what="large offsets")
    empty = [(0, 0, 0, 8), (3, 3, 8, -1), (0, 0, 0, 0)]
    assert all(fr.size == 0 for fr in field(ctx, recs[:3], empty, CO, surface))             # empty windows: HG_OK, nothing is written
    assert field(ctx, np.zeros((0, CM.RECORD)), [], CO, surface) == []                      # no frames
    ctx.field_camera_frames_device(0, [], W, H, surface, *CM.CANVAS, CO, 0)                 # ... and no pointer is looked at
    ctx.field_camera_frames_device(0, empty, W, H, surface, *CM.CANVAS, CO, 0)


# ------------------------------------------------------------------------------------------------ the field's special cases
@pytest.mark.parametrize("surface", [CM.CYLINDER, CM.SPHERE])
def test_a_frame_looking_away_a_window_across_the_seam_and_one_a_turn_further(ctx, surface):
    turn = 880                                               # pixels of a full turn: scale = 880 / (2 pi), so that a turn is a whole number of columns
    canvas = (turn / CM.TWO_PI, 13.37, 7.77)
    seam = CM.pack_record(CM.rot(math.pi - 0.05, 0.1, 0.2), 150.0, 155.0, 90.3, 60.7, (-0.1, 0.02, 0.001, 0.001, 0.0), W, H)
    away = CM.pack_record(CM.rot(-0.05, 0.1, 0.2), 150.0, 155.0, 90.3, 60.7, None, W, H)
    x0 = 13 + turn // 2 - 70                                 # 140 columns around a = pi
    geoms = [(x0, -30, 140, 70), (x0 + turn, -30, 140, 70), (x0, -30, 140, 70), (x0 - 3 * turn, -30, 140, 70)]
    recs = np.stack([seam, seam, away, seam])
    frames = field(ctx, recs, geoms, CO, surface, canvas)
    check_frames(frames, recs, geoms, CO, surface, canvas, what="seam")
    v = [fr.view(np.float32).reshape(-1, 2) for fr in frames]
    assert np.isnan(v[2]).all(), "a frame looking away from its window is all uncovered"
    cov = ~np.isnan(v[0][:, 0])
    assert 0.3 * cov.size < cov.sum() and (cov.reshape(70, 140)[:, 60:80].sum(1) > 0).any(), "the seam runs through covered pixels"
    # the windows a turn further: the unshifted model's values within the sum of the two deltas
    U, V = (a.ravel() for a in CM.window_positions(geoms[0]))
    sx, sy, _, _ = CM.to_source(seam, surface, *canvas, U, V, CM.LD)
    d0 = CM.delta(seam, surface, *canvas, U, V)
    for k in (1, 3):
        Uk, Vk = (a.ravel() for a in CM.window_positions(geoms[k]))
        dk = CM.delta(seam, surface, *canvas, Uk, Vk)
        ck = ~np.isnan(v[k][:, 0])
        m = cov & ck
        assert (cov != ck).sum() <= 0.001 * cov.size and m.sum() > 0.3 * cov.size
        assert CM._f32_between(v[k][m, 0], (sx - (d0[0] + dk[0]))[m], (sx + (d0[0] + dk[0]))[m]).all()
        assert CM._f32_between(v[k][m, 1], (sy - (d0[1] + dk[1]))[m], (sy + (d0[1] + dk[1]))[m]).all()


def test_a_pole_inside_a_sphere_window(ctx):
    canvas = (40.0, 3.3, -2.7)
    pole = CM.pack_record(CM.rot(0.4, -(math.pi / 2 - 0.12), 0.3), 150.0, 150.0, 90.3, 60.7, None, W, H)
    win = HG.camera_limits(pole, W, H, CM.SPHERE, *canvas)
    geoms = [win, (win[0] - 5, win[1] + win[3] - 12, win[2] + 10, 30)]      # the window of the limits; a band of rows across the pole's row
    recs = np.stack([pole, pole])
    for fmt in (IX, CO):
        frames = field(ctx, recs, geoms, fmt, CM.SPHERE, canvas)
        check_frames(frames, recs, geoms, fmt, CM.SPHERE, canvas, what="pole")
    v = frames[0].view(np.float32).reshape(win[3], win[2], 2)
    row = int(round(-2.7 + 40.0 * math.pi / 2)) - win[1]     # the pole's row: covered at every azimuth
    assert (~np.isnan(v[row - 1, :, 0])).mean() > 0.95


def test_the_r2_max_cut_keeps_fold_back_pixels_out(ctx):
    """k1 = -0.3: the radial polynomial turns at r2 = 1 / 0.9, and rays beyond it land inside the picture again.  On a plane window that
    reaches far beyond the picture every covered pixel has r2 <= r2_max, and the pixels that would fold back are there to be refused."""
    rec = CM.pack_record(CM.rot(0.013, -0.02, 0.05), 220.0, 220.0, 90.3, 60.7, (-0.3, 0.0, 0.0, 0.0, 0.0), W, H)
    canvas = (220.0, 90.3, 60.7)
    g = (-310, -260, 800, 640)
    frames = field(ctx, [rec], [g], CO, CM.PLANE, canvas)
    check_frames(frames, [rec], [g], CO, CM.PLANE, canvas, what="fold")
    U, V = (a.ravel() for a in CM.window_positions(g))
    sx, sy, cz, r2 = CM.to_source(rec, CM.PLANE, *canvas, U, V)
    with np.errstate(invalid="ignore"):
        in_picture = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H) & (cz > 0)
    folded = in_picture & (r2 > rec[CM.R2MAX] * 1.01)
    assert folded.sum() > 1000, "the window shows the fold"
    cov = ~np.isnan(frames[0].view(np.float32).reshape(-1, 2)[:, 0])
    assert not (cov & folded).any() and (cov & in_picture).sum() > 10000
    assert (r2[cov] <= rec[CM.R2MAX] * (1 + 1e-12)).all()


@pytest.mark.parametrize("surface", SURFACES)
def test_a_nan_record_fails_alone_and_two_runs_give_the_same_bytes(ctx, surface):
    geoms = [(-100, -50, 130, BAND + 3)] * 5
    recs = CM.cameras(5, True)
    bad = recs.copy()
    bad[1, CM.K2] = np.nan                                   # a lens term
    bad[3, 27] = np.nan                                      # a slot nothing reads
    for fmt in (IX, CO):
        good = field(ctx, recs, geoms, fmt, surface)
        got = field(ctx, bad, geoms, fmt, surface)
        again = field(ctx, bad, geoms, fmt, surface)
        check_frames(got, bad, geoms, fmt, surface, what="NaN record")
        for f in range(5):
            assert np.array_equal(got[f], again[f]), (f, "two runs give the same bytes")
            if f in (1, 3):
                assert (got[f].view(np.int32) == -1).all() if fmt == IX else (got[f].view(np.uint32) == CM.NANP).all()
            else:
                assert np.array_equal(got[f], good[f]), (f, "the other frames are not affected")


# ------------------------------------------------------------------------------------------------ point lists
ODD = np.array([[np.nan, 1], [2, np.nan], [np.inf, 0], [0, -np.inf], [1e30, 5], [-1e30, 1e30], [13.5, 7.25], [-1000.75, 2000.5]], np.float32)


@pytest.mark.parametrize("surface", SURFACES)
@pytest.mark.parametrize("n_pts", [0, 1, 63, 64, 65, 1000])
def test_point_lists_around_the_wave_in_both_directions(ctx, surface, n_pts):
    recs = CM.cameras(5, True)
    rng = np.random.default_rng(n_pts + 7)
    lists = []
    for s in range(5):                                       # canvas positions around the frames, source positions around the picture, odd floats
        p = np.stack([rng.uniform(-300, 300, n_pts), rng.uniform(-120, 120, n_pts)], 1).astype(np.float32)
        p[:min(n_pts, 8)] = ODD[:min(n_pts, 8)] if s % 2 == 0 else ODD[::-1][:min(n_pts, 8)]
        lists.append(p)
    lists = np.stack(lists) if n_pts else np.zeros((5, 0, 2), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        sources = lists * np.float32(0.4) + np.float32(70.0)  # the same floats moved over the picture: source positions for the other direction
    for k in (1, 5):                                         # n_sets 1 and n_frames
        got = points(ctx, recs, surface, lists[:k], True)
        back = points(ctx, recs, surface, sources[:k], False)
        assert got.shape == (5, n_pts, 2) and back.shape == (5, n_pts, 2)
        for f in range(5):
            lst = lists[f % k]
            fin = np.isfinite(lst).all(1)
            assert (got[f][~fin].view(np.uint32) == CM.NANP).all()
            p = lst[fin].astype(np.float64)
            CM.check_to_source(np.ascontiguousarray(got[f][fin]).tobytes(), recs[f], surface, *CM.CANVAS, p[:, 0], p[:, 1], what=(surface, n_pts, f))
            TC.check_to_canvas(back[f], recs[f], surface, *CM.CANVAS, sources[f % k], (surface, n_pts, f))


@pytest.mark.parametrize("surface", SURFACES)
def test_points_on_pixels_repeat_the_coords_field_and_come_back_from_the_source(ctx, surface):
    g = (-100, -50, 257, BAND + 1)
    recs = CM.cameras(5, True)
    U, V = CM.window_positions(g)
    grid = np.stack([U.ravel(), V.ravel()], 1).astype(np.float32)[None]
    frames = field(ctx, recs, [g] * 5, CO, surface)
    got = points(ctx, recs, surface, grid, True)
    n_cov = 0
    for f in range(5):
        fld = frames[f].view(np.uint32).reshape(-1, 2)
        cov = fld[:, 0] != CM.NANP
        n_cov += int(cov.sum())
        assert np.array_equal(got[f].view(np.uint32)[cov], fld[cov]), (surface, f, "an integer position equals the coords field where it is covered, bit for bit")
    assert n_cov > 5000
    # the round trip on the device, frame by frame, inside the bound derived in the docstring
    for f in range(5):
        p = TC.round_trip_points(recs[f], surface, *CM.CANVAS)
        s = points(ctx, recs[f:f + 1], surface, p[None], True)
        assert not np.isnan(s).any()
        back = points(ctx, recs[f:f + 1], surface, s, False)[0]
        bU, bV = TC.round_trip_bound(recs[f], surface, *CM.CANVAS, p[:, 0].astype(np.float64), p[:, 1].astype(np.float64))
        eU, eV = np.abs(back[:, 0].astype(np.float64) - p[:, 0]), np.abs(back[:, 1].astype(np.float64) - p[:, 1])
        print(f"surface {surface} frame {f}: round trip error / bound {max((eU / bU).max(), (eV / bV).max()):.3g}")
        assert (eU <= bU).all() and (eV <= bV).all(), (surface, f, (eU / bU).max(), (eV / bV).max())


# ------------------------------------------------------------------------------------------------ limits, on device fields
def test_camera_limits_hold_every_covered_pixel_of_the_device_fields(ctx):
    """The property of tests/test_camera_cpu.py on the device's own fields: over the returned window grown by 8 pixels on each side, every
    covered pixel lies inside the window (a pole frame's pixels by their first image: covered_outside there)."""
    for name, rec, surface, scale, u0, v0 in TC.limit_cases():
        win = HG.camera_limits(rec, W, H, surface, scale, u0, v0)
        g = (win[0] - 8, win[1] - 8, win[2] + 16, win[3] + 16)
        fr = field(ctx, [rec], [g], CO, surface, (scale, u0, v0))[0]
        cov = ~np.isnan(fr.view(np.float32).reshape(g[3], g[2], 2)[..., 0])
        U, V = CM.window_positions(g)
        if name.startswith("pole"):
            U, V = CM.first_image(rec, scale, u0, v0, U, V)
        inside = (U >= win[0]) & (U <= win[0] + win[2] - 1) & (V >= win[1]) & (V <= win[1] + win[3] - 1)
        assert cov.sum() > 1000 and not (cov & ~inside).any(), (name, win, int((cov & ~inside).sum()))


# ------------------------------------------------------------------------------------------------ end to end
def texture(a, b):
    """A smooth texture on the sphere (azimuth a, elevation b), grey levels 28..228."""
    return 128.0 + 60.0 * np.sin(3.0 * a) * np.cos(2.0 * b) + 40.0 * np.cos(5.0 * b + a)


def test_five_frames_of_a_sphere_come_back_as_a_160_degree_mosaic(ctx):
    """Five 96 x 64 frames rendered from an analytic texture with yaw steps of 25 degrees; device field -> bilinear remap -> MEAN mosaic over a
    160 degree window, against the same pipeline fed the model's field: at most 1 grey level apart.  The RMS against the texture is printed."""
    fw, fh, f, scale = 96, 64, 80.0, 80.0
    recs = np.stack([CM.pack_record(CM.rot(math.radians(25.0 * (k - 2)) + 0.004, 0.02 * (k - 2), 0.01 * k), f, f, 47.6, 31.7, (-0.08, 0.01, 0.0, 0.0, 0.0), fw, fh)
                     for k in range(5)])
    x, y = np.meshgrid(np.arange(fw, dtype=np.float64), np.arange(fh, dtype=np.float64))
    planes = []
    for rec in recs:
        a, b, ok = CM.to_canvas(rec, CM.SPHERE, 1.0, 0.0, 0.0, x, y)
        assert ok.all()
        planes.append(np.clip(np.floor(texture(a, b) + 0.5), 0, 255).astype(np.uint8).reshape(fh, fw, 1))
    half = int(round(scale * math.radians(80.0)))
    canvas = (-half, -34, 2 * half, 68)
    geoms = [canvas] * 5
    want_fields = [CM.model_field(rec, canvas, fw, fh, CM.SPHERE, scale, 0.0, 0.0, False) for rec in recs]
    got_fields = [fr.view(np.float32).reshape(-1, 2) for fr in field(ctx, recs, geoms, CO, CM.SPHERE, (scale, 0.0, 0.0), w=fw, h=fh)]
    results = []
    for fields in (got_fields, want_fields):
        ran = GF.run_frames(ctx, geoms, fields, 8, planes, 1,
                            lambda b: ctx.remap_bilinear_frames_device(geoms, b.d_f, b.d_p, fw, fh, 5, b.stride, HG.ELEM_U8, 1, b.d_o))
        frames = [ran.raw[o:o + canvas[2] * canvas[3]].reshape(canvas[3], canvas[2], 1) for o in ran.oo]
        out, _ = GF.run_mosaic(ctx, geoms, fields, frames, HG.ELEM_U8, 1, fw, fh, HG.MOSAIC_MEAN, 0.0, canvas)
        results.append(out.reshape(canvas[3], canvas[2]).astype(np.int32))
    got, want = results
    assert np.abs(got - want).max() <= 1, int(np.abs(got - want).max())
    cov = ~np.all([np.isnan(fl[:, 0]) for fl in want_fields], axis=0).reshape(canvas[3], canvas[2])
    assert cov.mean() > 0.7 and cov[canvas[3] // 2, 4:-4].all()      # the middle row is covered from -77 to +77 degrees at least
    U, V = CM.window_positions(canvas)
    rms = math.sqrt(float(np.mean((got[cov] - texture(U / scale, V / scale)[cov]) ** 2)))
    print(f"end to end: {int(cov.sum())} covered canvas pixels, RMS against the analytic texture {rms:.3f} grey levels, device against model pipeline "
          f"{int(np.abs(got - want).max())} at most")


# ------------------------------------------------------------------------------------------------ refusals, state, the drop-in class
def test_refusals_on_the_device(ctx):
    recs = CM.cameras(1, False)
    d_r, _ = upload_records(ctx, recs)
    d_f = ctx.alloc(4096)
    try:
        g = [(0, 0, 8, 8)]
        code = lambda fn, *x, **k: GF.refusal_code(fn, *x, **k)
        fld, cv = ctx.field_camera_frames_device, CM.CANVAS
        assert code(fld, d_r, g, W, H, 2, *cv, CO, 0) == INVALID                             # d_field NULL
        assert code(fld, 0, g, W, H, 2, *cv, CO, d_f) == INVALID                             # d_records NULL
        assert code(fld, d_r + 4, g, W, H, 2, *cv, CO, d_f) == INVALID                       # misaligned records
        assert code(fld, d_r, g, W, H, 2, *cv, CO, d_f + 4) == INVALID                       # a coords field off its 8 bytes
        assert code(fld, d_r, g, W, H, 2, *cv, IX, d_f + 2) == INVALID
        assert code(fld, d_r, g, W, H, 3, *cv, CO, d_f) == INVALID
        assert code(fld, d_r, g, W, H, 2, 0.0, 0.0, 0.0, CO, d_f) == INVALID
        assert code(fld, d_r, g, W, H, 2, *cv, CO, d_f, field_offsets=[12]) == INVALID
        for fn in (ctx.points_camera_to_source_frames_device, ctx.points_camera_to_canvas_frames_device):
            assert code(fn, d_r, 1, 2, *cv, 0, 4, 1, d_f) == INVALID
            assert code(fn, d_r, 1, 2, *cv, d_f + 4, 4, 1, d_f) == INVALID
            assert code(fn, d_r, 1, 2, *cv, d_f, 4, 0, d_f) == INVALID
            assert code(fn, d_r, 1, 9, *cv, d_f, 4, 1, d_f) == INVALID
            fn(0, 0, 2, *cv, 0, 4, 1, 0)                                                   # no frames, no points: HG_OK, nothing is looked at
            fn(0, 1, 2, *cv, 0, 0, 1, 0)
        ctx.sync()
        assert np.array_equal(ctx.to_host(d_r, recs.nbytes).view(np.float64).view(np.uint64), recs.ravel().view(np.uint64)), "a refused call writes nothing"
    finally:
        ctx.free(d_r)
        ctx.free(d_f)


def test_a_camera_call_leaves_the_warp_state_alone(ctx):
    before = GF.tap_state(ctx)
    recs = CM.cameras(2, True)
    field(ctx, recs, [(0, 0, 20, 6)] * 2, CO, CM.SPHERE)
    points(ctx, recs, CM.CYLINDER, np.zeros((1, 3, 2), np.float32), True)
    points(ctx, recs, CM.PLANE, np.zeros((1, 3, 2), np.float32), False)
    assert GF.tap_state(ctx) == before


def test_js_warp_camera_equals_the_gather_through_its_own_index_field():
    """tests/js/camera_gpu.mjs: warpCamera(..., { output: 'image' }) on the real addon equals gathering the picture through the call's own
    index field; the default window is hg_camera_limits'."""
    GF.run_node_case("camera_gpu.mjs")
