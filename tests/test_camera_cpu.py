"""CPU-side checks of the camera models (include/hgwarp.h, "camera models"): the header declares and the library exports the entries and
enums, the numpy model of tests/hgtest/camera.py pinned by hand-worked cases and by its own round trip, every refusal that needs no device,
the four host calls, the window property of hg_camera_limits, the fixtures of the GPU test against their cap of excused pixels, the round-trip
bound of the point lists on the model, and the kernel text itself on the host under sanitizers.  tests/test_gpu_camera.py compares the
device with the model."""
import ctypes as C
import json
import math
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "homography.js_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hgwarp as HG                          # noqa: E402
from hgtest import camera as CM              # noqa: E402

NEW = ["hg_camera_pack_record", "hg_camera_limits", "hg_camera_focals_from_matrix", "hg_camera_rotation_from_matrix",
       "hg_field_camera_frames_device", "hg_points_camera_to_source_frames_device", "hg_points_camera_to_canvas_frames_device"]
INVALID = 1
SZ = C.c_size_t
CLANGXX = next((p for p in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("clang++")) if p and os.path.exists(p)), None)
CSRC = os.path.join(ROOT, "homography.js_amd", "csrc")
BAND = int(re.search(r"kCamBandRows = (\d+);", open(os.path.join(CSRC, "hg_camera_dev.h")).read()).group(1))
SURFACES = (CM.PLANE, CM.CYLINDER, CM.SPHERE)
W, H = CM.SRC_W, CM.SRC_H


def test_header_declares_and_library_exports_the_camera_entry_points():
    text = open(os.path.join(ROOT, "include", "hgwarp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hg_[a-z0-9_]+)\s*\(", code))
    L = HG.lib()
    for name in NEW:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in HG.EXPORTS, name
    assert "camera models\n" in text and "by the presence of hg_field_camera_frames_device" in text.split("enum {")[0]       # the section; the note beside HG_VERSION
    enums = dict(re.findall(r"\b(HG_(?:CAMERA|SURFACE)_[A-Z_]+) = (\d+)", code))
    assert enums == {"HG_CAMERA_RECORD_DOUBLES": "32", "HG_CAMERA_UNDISTORT_ITERS": "20", "HG_SURFACE_PLANE": "0", "HG_SURFACE_CYLINDER": "1", "HG_SURFACE_SPHERE": "2"}
    assert (HG.SURFACE_PLANE, HG.SURFACE_CYLINDER, HG.SURFACE_SPHERE) == SURFACES and HG.CAMERA_RECORD_DOUBLES == CM.RECORD and HG.CAMERA_UNDISTORT_ITERS == CM.ITERS
    for fn in ("camera_pack_record", "camera_limits", "camera_focals_from_matrix", "camera_rotation_from_matrix"):
        assert callable(getattr(HG, fn)), fn
    for m in ("field_camera_frames_device", "points_camera_to_source_frames_device", "points_camera_to_canvas_frames_device"):
        assert callable(getattr(HG.Context, m)), m
    for word in ("bundle adjustment", "fisheye", "estimating distortion", "anything but a field"):
        assert word in text.split("camera models\n")[1].split("dense optical flow\n")[0], word              # what is out of scope is said in the header
    assert BAND >= 4 and BAND % 4 == 0


# ------------------------------------------------------------------------------------------------ the model, by hand
def test_model_identity_on_the_plane_with_scale_f_is_the_identity_map():
    f = 200.0
    rec = CM.pack_record(np.eye(3), f, f, 64.0, 48.0, None, 128, 96)
    assert rec[CM.R2MAX] == np.inf and rec[CM.AC] == 0.0 and (rec[20:] == 0).all()
    U, V = np.meshgrid(np.arange(-5.0, 140.0, 7.0), np.arange(-3.0, 100.0, 5.0))
    sx, sy, cz, r2 = CM.to_source(rec, CM.PLANE, f, 64.0, 48.0, U, V)
    assert np.abs(sx - U).max() < 1e-12 and np.abs(sy - V).max() < 1e-12 and (cz == 1.0).all()
    cov = CM.covered(rec, sx, sy, cz, r2, 128, 96)
    assert np.array_equal(cov, (U >= 0) & (U < 128) & (V >= 0) & (V < 96))


def test_model_a_quarter_turn_of_yaw_puts_the_optical_axis_at_half_pi():
    rec = CM.pack_record(CM.rot(math.pi / 2), 100.0, 100.0, 50.0, 40.0, None, 100, 80)
    assert abs(rec[CM.AC] - math.pi / 2) < 1e-15
    scale = 70.0
    sx, sy, cz, _ = CM.to_source(rec, CM.SPHERE, scale, 0.0, 0.0, np.array([scale * math.pi / 2]), np.array([0.0]))
    assert abs(sx[0] - 50.0) < 1e-12 and abs(sy[0] - 40.0) < 1e-12 and abs(cz[0] - 1.0) < 1e-15
    # 10 degrees to the right of the axis and 5 up (y grows downwards): x' = tan(10) f, y' = -tan(5) f / cos(10)
    a, b = math.radians(100.0), math.radians(-5.0)
    sx, sy, _, _ = CM.to_source(rec, CM.SPHERE, scale, 0.0, 0.0, np.array([scale * a]), np.array([scale * b]))
    assert abs(sx[0] - (50.0 + 100.0 * math.tan(math.radians(10.0)))) < 1e-11
    assert abs(sy[0] - (40.0 - 100.0 * math.tan(math.radians(5.0)) / math.cos(math.radians(10.0)))) < 1e-11
    # the opposite direction is behind the camera
    _, _, cz, _ = CM.to_source(rec, CM.SPHERE, scale, 0.0, 0.0, np.array([-scale * math.pi / 2]), np.array([0.0]))
    assert cz[0] < 0


def test_model_pure_k1_worked_by_hand():
    """Identity, f = 100, c = 0, k1 = -0.2 on the plane at scale 1: the canvas position (0.5, 0) is the ray (0.5, 0, 1), xn = 0.5, r2 = 0.25,
    rad = 1 - 0.2 * 0.25 = 0.95, xd = 0.475, sx = 47.5; at (0.3, 0.4): r2 = 0.25 again, (sx, sy) = (28.5, 38)."""
    rec = np.zeros(CM.RECORD)
    rec[:9] = np.eye(3).ravel()
    rec[CM.FX], rec[CM.FY], rec[CM.K1], rec[CM.R2MAX] = 100.0, 100.0, -0.2, np.inf
    sx, sy, cz, r2 = CM.to_source(rec, CM.PLANE, 1.0, 0.0, 0.0, np.array([0.5, 0.3]), np.array([0.0, 0.4]))
    assert np.allclose(r2, 0.25, rtol=0, atol=1e-16) and np.allclose(sx, [47.5, 28.5], rtol=0, atol=1e-13) and np.allclose(sy, [0.0, 38.0], rtol=0, atol=1e-13)
    # and back: 0.95 xn' = 0.475 has the fixed point 0.5
    U, V, ok = CM.to_canvas(rec, CM.PLANE, 1.0, 0.0, 0.0, np.array([47.5, 28.5]), np.array([0.0, 38.0]))
    assert ok.all() and np.allclose(U, [0.5, 0.3], rtol=0, atol=1e-12) and np.allclose(V, [0.0, 0.4], rtol=0, atol=1e-12)
    # the fold: rad' = 0 at r2 = 1 / (3 * 0.2): far outside, xn = 4 lands at xd = 4 (1 - 3.2) < 0 -- inside a picture, were it not for r2_max
    rec2 = CM.pack_record(np.eye(3), 100.0, 100.0, 50.0, 50.0, (-0.2, 0, 0, 0, 0), 100, 100)
    assert 0.5 < rec2[CM.R2MAX] < 1 / 0.6
    sx, sy, cz, r2 = CM.to_source(rec2, CM.PLANE, 1.0, 0.0, 0.0, np.array([2.2]), np.array([0.0]))
    assert 0 <= sx[0] < 100 and not CM.covered(rec2, sx, sy, cz, r2, 100, 100)[0]


@pytest.mark.parametrize("surface", SURFACES)
@pytest.mark.parametrize("distort", [False, True])
def test_model_round_trip_source_canvas_source(surface, distort):
    recs = CM.cameras(6, distort)
    scale, u0, v0 = CM.CANVAS
    rng = np.random.default_rng(5)
    x, y = rng.uniform(0, W, 400), rng.uniform(0, H, 400)
    for rec in recs:
        U, V, ok = CM.to_canvas(rec, surface, scale, u0, v0, x, y)
        assert ok.all()
        sx, sy, cz, r2 = CM.to_source(rec, surface, scale, u0, v0, U, V)
        assert CM.inside(rec, cz, r2).all()
        assert np.abs(sx - x).max() < 1e-6 and np.abs(sy - y).max() < 1e-6          # (1e-9 of the inverse's tolerance times f, and change)
        if surface != CM.PLANE:
            assert (np.abs((U - u0) / scale - rec[CM.AC]) <= math.pi + 1e-12).all()  # unwrapped about the frame's own axis


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_without_a_device_in_the_documented_order():
    """Every shape check is made before the pointers and the context are looked at (all NULL throughout) and names itself in hg_last_error;
    a call that breaks two limits reports the one the header lists first."""
    L = HG.lib()
    err = lambda: L.hg_last_error(None).decode()
    G = (HG.Geom * 2)(HG.Geom(0, 0, 8, 8), HG.Geom(-3, 2, 5, 4))
    nan, inf = float("nan"), float("inf")

    def field(f=2, W=64, H=48, surface=2, scale=100.0, u0=0.0, v0=0.0, fmt=HG.FIELD_COORDS, geoms=G, offs=None):
        return L.hg_field_camera_frames_device(None, None, geoms, f, W, H, surface, scale, u0, v0, fmt, offs, None), err()

    big = (HG.Geom * 1)(HG.Geom(1 << 27, 0, 4, 4))
    offs = (SZ * 2)(0, 260)
    order = [(dict(surface=3), "unknown surface"), (dict(fmt=2), "unknown field format"), (dict(scale=0.0), "scale must"), (dict(u0=inf), "u0 and v0"),
             (dict(W=0), "W and H"), (dict(f=4097), "n_frames must"), (dict(geoms=big, f=1), "2^26"),
             (dict(fmt=HG.FIELD_INDEX, W=65536, H=32768), "2^31 pixels"), (dict(offs=offs), "multiples")]
    for k, (bad, word) in enumerate(order):
        code, msg = field(**bad)
        assert code == INVALID and word in msg, (bad, msg)
        for later, _ in order[k + 1:]:                       # the earlier limit wins
            both = dict(later, **bad)
            code, msg = field(**both)
            assert code == INVALID and word in msg, (both, msg)
    for bad, word in ((dict(surface=-1), "unknown surface"), (dict(fmt=-1), "unknown field format"), (dict(scale=-1.0), "scale must"), (dict(scale=nan), "scale must"),
                      (dict(scale=inf), "scale must"), (dict(v0=nan), "u0 and v0"), (dict(H=-1), "W and H"), (dict(f=-1), "n_frames must"), (dict(geoms=None), "geoms is NULL")):
        code, msg = field(**bad)
        assert code == INVALID and word in msg, (bad, msg)
    assert field(f=0)[0] == 0
    empty = (HG.Geom * 2)(HG.Geom(0, 0, 0, 8), HG.Geom(0, 0, 8, -1))
    assert field(geoms=empty)[0] == 0                        # a set of empty windows: nothing to do
    code, msg = field()
    assert code == INVALID and "is NULL" in msg              # the shape is legal: only the pointers are missing
    assert "is NULL" in field(fmt=HG.FIELD_COORDS, W=65536, H=32768)[1]      # the coords format has no 2^31 limit

    for name in ("hg_points_camera_to_source_frames_device", "hg_points_camera_to_canvas_frames_device"):
        def points(f=2, surface=1, scale=50.0, u0=0.0, v0=0.0, n_pts=10, n_sets=1):
            return getattr(L, name)(None, None, f, surface, scale, u0, v0, None, n_pts, n_sets, None), err()

        order = [(dict(surface=7), "unknown surface"), (dict(scale=-2.0), "scale must"), (dict(v0=-inf), "u0 and v0"), (dict(f=4097), "n_frames must"),
                 (dict(n_pts=(1 << 24) + 1), "n_pts must"), (dict(n_sets=0), "n_sets must")]
        for k, (bad, word) in enumerate(order):
            code, msg = points(**bad)
            assert code == INVALID and word in msg, (bad, msg)
            for later, _ in order[k + 1:]:
                code, msg = points(**dict(later, **bad))
                assert code == INVALID and word in msg, (bad, later, msg)
        assert points(n_pts=-1)[0] == INVALID and points(f=-3)[0] == INVALID
        assert points(n_pts=0)[0] == 0 and points(f=0)[0] == 0
        code, msg = points()
        assert code == INVALID and "is NULL" in msg

    rec = CM.cameras(1, False)[0]
    out = (C.c_int32 * 4)()
    rp = rec.ctypes.data_as(C.POINTER(C.c_double))
    for args, word in (((rp, W, H, 5, 100.0, 0.0, 0.0, out), "unknown surface"), ((rp, W, H, 2, 0.0, 0.0, 0.0, out), "scale must"),
                       ((rp, W, H, 2, 100.0, nan, 0.0, out), "u0 and v0"), ((rp, 0, H, 2, 100.0, 0.0, 0.0, out), "W and H"),
                       ((None, W, H, 2, 100.0, 0.0, 0.0, out), "is NULL"), ((rp, W, H, 2, 100.0, 0.0, 0.0, None), "is NULL")):
        assert L.hg_camera_limits(*args) == INVALID and word in err(), (word, err())
    with pytest.raises(HG.HgError) as e:
        HG.camera_limits(rec, W, H, 3, 100.0, 0, 0)
    assert e.value.code == INVALID


# ------------------------------------------------------------------------------------------------ the host calls
def test_camera_pack_record_matches_the_model_and_refuses_what_the_header_says():
    R = CM.rot(0.7, -0.2, 0.1)
    for dist in (None, (-0.2, 0.05, 0.001, -0.002, 0.0), (0.0, 0.0, 0.0, 0.0, 0.0), (0.1, -0.02, 0.0, 0.0, 0.01)):
        got = HG.camera_pack_record(R, (150.0, 140.0), (90.5, 60.25), W, H, dist)
        want = CM.pack_record(R, 150.0, 140.0, 90.5, 60.25, dist, W, H)
        assert got.shape == (32,) and np.array_equal(got.view(np.uint64), want.view(np.uint64)), dist
        assert (got[20:] == 0).all() and abs(got[CM.AC] - 0.7) < 1e-15
        if dist is None:
            assert got[CM.R2MAX] == np.inf
        else:
            # r2_max: 1.05 x the largest undistorted r2 of the corners and edge midpoints; every position of the picture stays valid
            far = max(((x - 90.5) / 150.0) ** 2 + ((y - 60.25) / 140.0) ** 2 for x in (0, W) for y in (0, H))
            assert 0.5 * far < got[CM.R2MAX] < 2.5 * far
            xs, ys = np.meshgrid(np.linspace(0, W, 37), np.linspace(0, H, 25))
            assert CM.to_canvas(got, CM.PLANE, 100.0, 0.0, 0.0, xs, ys)[2].all()
    code = lambda *a, **k: pytest.raises(HG.HgError, HG.camera_pack_record, *a, **k).value.code
    bad = R.copy(); bad[0, 0] += 2e-6
    assert code(bad, 150.0, (90, 60), W, H) == INVALID and "orthonormal" in HG.lib().hg_last_error(None).decode()
    ok = R.copy(); ok[0, 0] += 1e-7
    HG.camera_pack_record(ok, 150.0, (90, 60), W, H)        # inside 1e-6
    assert code(2.0 * R, 150.0, (90, 60), W, H) == INVALID
    for focal in (0.0, -1.0, (150.0, 0.0), float("nan"), float("inf")):
        assert code(R, focal, (90, 60), W, H) == INVALID, focal
    assert code(R, 150.0, (float("nan"), 60), W, H) == INVALID and code(R, 150.0, (90, 60), W, H, (0, 0, float("inf"), 0, 0)) == INVALID
    nanr = R.copy(); nanr[1, 1] = np.nan
    assert code(nanr, 150.0, (90, 60), W, H) == INVALID and code(R, 150.0, (90, 60), 0, H) == INVALID
    # too strong: k1 = -1.5 folds at r2 = 1 / 4.5, inside a picture whose corners lie at r2 = 0.52
    assert code(R, 150.0, (90, 60), W, H, (-1.5, 0, 0, 0, 0)) == INVALID and "too strong" in HG.lib().hg_last_error(None).decode()
    with pytest.raises(ValueError):
        CM.pack_record(R, 150.0, 150.0, 90, 60, (-1.5, 0, 0, 0, 0), W, H)


def limit_cases():
    """(name, record, surface, scale, u0, v0): plain frames on every surface, a frame across the +-pi seam and one holding a pole."""
    scale, u0, v0 = 60.0, 3.3, -2.7
    out = []
    for surface in SURFACES:
        for k, rec in enumerate(CM.cameras(3, True)):
            out.append((f"plain {surface} {k}", rec, surface, scale, u0, v0))
    seam = CM.pack_record(CM.rot(math.pi - 0.05, 0.1, 0.2), 150.0, 155.0, 90.3, 60.7, (-0.1, 0.02, 0.001, 0.001, 0.0), W, H)
    out.append(("seam, cylinder", seam, CM.CYLINDER, scale, u0, v0))
    out.append(("seam, sphere", seam, CM.SPHERE, scale, u0, v0))
    pole = CM.pack_record(CM.rot(0.4, -(math.pi / 2 - 0.12), 0.3), 150.0, 150.0, 90.3, 60.7, None, W, H)
    out.append(("pole, sphere", pole, CM.SPHERE, 40.0, u0, v0))
    return out


def covered_outside(rec, surface, scale, u0, v0, win, grow=8, sphere_turns=False):
    """The covered pixels of the model's field over `win` grown by `grow` pixels on each side that lie OUTSIDE win.  sphere_turns: the window
    is a full turn of the sphere, so the grown window shows positions of the window again -- the same direction one turn further, or seen
    across the pole (elevation b beyond +-pi/2 is the direction (a + pi, pi - b)): such a pixel is brought back to its first image, azimuth
    within a_c +- pi and elevation within +-pi/2, before it is asked whether the window holds it."""
    x, y, w, h = win
    g = (x - grow, y - grow, w + 2 * grow, h + 2 * grow)
    U, V = CM.window_positions(g)
    cov = CM.covered(rec, *CM.to_source(rec, surface, scale, u0, v0, U, V), W, H)
    if sphere_turns:
        U, V = CM.first_image(rec, scale, u0, v0, U, V)
    inside = (U >= x) & (U <= x + w - 1) & (V >= y) & (V <= y + h - 1)
    return int((cov & ~inside).sum()), int(cov.sum())


def test_camera_limits_hold_every_covered_pixel_of_the_model():
    """hg_camera_limits' property: every covered pixel of the field of the returned window grown by 8 pixels on each side lies inside the
    window.  A frame that holds a pole gets a full turn of columns, a_c +- pi, up to the pole's row; the canvas is periodic in both directions
    (the header: positions beyond +-pi scale are legal everywhere), so the 8 pixels around such a window ARE positions of the window again, and
    there the property is asked of every pixel's first image (covered_outside)."""
    for name, rec, surface, scale, u0, v0 in limit_cases():
        win = HG.camera_limits(rec, W, H, surface, scale, u0, v0)
        assert win == CM.limits(rec, W, H, surface, scale, u0, v0), name
        pole = name.startswith("pole")
        out, n_cov = covered_outside(rec, surface, scale, u0, v0, win, sphere_turns=pole)
        assert out == 0 and n_cov > 1000, (name, win, out, n_cov)
        if name.startswith("seam"):
            a0, a1 = (win[0] - u0) / scale, (win[0] + win[2] - u0) / scale
            assert a0 < math.pi < a1 and win[2] < 0.6 * CM.TWO_PI * scale, (name, win)       # one contiguous window across the seam
        if pole:
            assert win[2] >= CM.TWO_PI * scale and win[1] + win[3] - 1 >= v0 + scale * math.pi / 2, (name, win)     # (it looks down: the pole of +y)
    # no valid border position: a record whose r2_max shuts every border position out
    rec = CM.cameras(1, True)[0].copy()
    rec[CM.R2MAX] = 1e-6
    with pytest.raises(HG.HgError) as e:
        HG.camera_limits(rec, W, H, CM.SPHERE, 60.0, 0, 0)
    assert e.value.code == INVALID and "no border position" in str(e.value)
    pole = CM.pack_record(CM.rot(0.4, -(math.pi / 2 - 0.12), 0.3), 150.0, 150.0, 90.3, 60.7, None, W, H)
    with pytest.raises(HG.HgError) as e:
        HG.camera_limits(pole, W, H, CM.CYLINDER, 40.0, 0, 0)
    assert "pole" in str(e.value)


def random_rotation(rng, lo_deg=8.0, hi_deg=35.0):
    """A rotation by lo..hi degrees about an axis that is at least 25 degrees away from the optical axis: generic, and not near the case
    (a rotation about the optical axis) that carries no focal information."""
    while True:
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        if abs(ax[2]) < math.cos(math.radians(25.0)):
            break
    t = math.radians(rng.uniform(lo_deg, hi_deg)) * rng.choice([-1.0, 1.0])
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + math.sin(t) * Kx + (1 - math.cos(t)) * (Kx @ Kx)


def test_camera_focals_from_matrix_returns_both_focal_lengths():
    rng = np.random.default_rng(2024)
    K = lambda f: np.diag([f, f, 1.0])
    worst = 0.0
    for _ in range(50):
        R = random_rotation(rng)
        f_from, f_to = rng.uniform(300, 3000), rng.uniform(300, 3000)
        Hm = (K(f_to) @ R @ np.linalg.inv(K(f_from))) * rng.uniform(0.2, 5.0) * rng.choice([-1.0, 1.0])
        g0, g1, ok0, ok1 = HG.camera_focals_from_matrix(Hm)
        assert ok0 and ok1
        worst = max(worst, abs(g0 / f_from - 1), abs(g1 / f_to - 1))
    print(f"focals: worst relative error {worst:.3g}")
    assert worst <= 1e-9
    for t in (0.3, -1.1, 0.0):
        g0, g1, ok0, ok1 = HG.camera_focals_from_matrix(K(700.0) @ CM.rot(0, 0, t) @ np.linalg.inv(K(500.0)))
        assert not ok0 and not ok1 and g0 == 0 and g1 == 0
    with pytest.raises(HG.HgError):
        HG.camera_focals_from_matrix([1, 0, 0, 0, float("nan"), 0, 0, 0, 1])


def test_camera_rotation_from_matrix_gives_back_the_rotation():
    rng = np.random.default_rng(77)
    Km = lambda k: np.array([[k[0], 0, k[2]], [0, k[1], k[3]], [0, 0, 1.0]])
    for _ in range(20):
        R = random_rotation(rng, 1.0, 120.0)
        k_from = (rng.uniform(300, 2000), rng.uniform(300, 2000), rng.uniform(-50, 900), rng.uniform(-50, 700))
        k_to = (rng.uniform(300, 2000), rng.uniform(300, 2000), rng.uniform(-50, 900), rng.uniform(-50, 700))
        Hm = (Km(k_to).astype(np.longdouble) @ R.astype(np.longdouble) @ np.linalg.inv(Km(k_from)).astype(np.longdouble)).astype(np.float64) * rng.uniform(0.2, 5.0)
        got = HG.camera_rotation_from_matrix(Hm, k_from, k_to)
        assert np.abs(got - R).max() <= 1e-12, np.abs(got - R).max()
        noisy = Km(k_to) @ (R + rng.normal(0, 1e-3, (3, 3))) @ np.linalg.inv(Km(k_from))
        got = HG.camera_rotation_from_matrix(noisy, k_from, k_to)
        assert np.abs(got.T @ got - np.eye(3)).max() < 1e-12 and np.linalg.det(got) > 0.999 and np.abs(got - R).max() < 5e-3
    for bad in (-np.eye(3), np.zeros((3, 3)), np.diag([1.0, 1.0, 0.0])):
        with pytest.raises(HG.HgError) as e:
            HG.camera_rotation_from_matrix(bad, (1, 1, 0, 0), (1, 1, 0, 0))
        assert e.value.code == INVALID and "det" in str(e.value)
    with pytest.raises(HG.HgError):
        HG.camera_rotation_from_matrix(np.eye(3), (0, 1, 0, 0), (1, 1, 0, 0))


# ------------------------------------------------------------------------------------------------ what the GPU test rests on
@pytest.mark.parametrize("surface", SURFACES)
@pytest.mark.parametrize("distort", [False, True])
def test_the_gpu_fixtures_stay_under_the_cap_of_excused_pixels(surface, distort):
    """The model perturbed by +-delta: the pixels it puts within delta of a coverage bound are at most 0.1 % of any frame (here: none), the
    bound itself stays far below a float32 ulp of the coordinates, and both outcomes of the coverage test occur."""
    scale, u0, v0 = CM.CANVAS
    geoms = CM.windows(BAND)
    recs = CM.cameras(len(geoms), distort)
    n_cov = n_all = 0
    for rec, g in zip(recs, geoms):
        if g[2] <= 0 or g[3] <= 0:
            continue
        assert CM.near_count(rec, g, W, H, surface, scale, u0, v0) <= 0.001 * g[2] * g[3]
        U, V = CM.window_positions(g)
        sx, sy, cz, r2 = CM.to_source(rec, surface, scale, u0, v0, U, V)
        cov = CM.covered(rec, sx, sy, cz, r2, W, H)
        dx, dy, _, _ = CM.delta(rec, surface, scale, u0, v0, U, V)
        assert dx[cov].max(initial=0) < 1e-10 and dy[cov].max(initial=0) < 1e-10
        lx, ly, _, _ = CM.to_source(rec, surface, scale, u0, v0, U, V, CM.LD)
        assert (np.abs(sx - lx)[cov] <= dx[cov]).all() and (np.abs(sy - ly)[cov] <= dy[cov]).all()       # float64 against longdouble: inside delta
        n_cov += int(cov.sum()); n_all += cov.size
    assert 0.05 * n_all < n_cov < 0.95 * n_all, (n_cov, n_all)


def round_trip_bound(rec, surface, scale, u0, v0, U, V):
    """The bound of to-canvas(float32(to-source(p))) - p, per coordinate, derived in tests/test_gpu_camera.py: the source position s is known
    to e_s = 2^-24 |s| (its rounding to float32) + f 1e-9 (what the inverse of the distortion may leave, in pixels) + delta; that goes through
    the local magnification |J| of source -> canvas (central differences of the model, step 1e-3 px, 1 % allowed for the second order); the
    result is rounded to float32 once more, 2^-24 |p|; the float64 arithmetic of source -> canvas adds 64 EPS (|p| + pi scale)."""
    sx, sy, _, _ = CM.to_source(rec, surface, scale, u0, v0, U, V)
    dx, dy, _, _ = CM.delta(rec, surface, scale, u0, v0, U, V)
    ex = 2.0 ** -24 * np.abs(sx) + rec[CM.FX] * 1e-9 + dx
    ey = 2.0 ** -24 * np.abs(sy) + rec[CM.FY] * 1e-9 + dy
    h = 1e-3
    Uxp, Vxp, _ = CM.to_canvas(rec, surface, scale, u0, v0, sx + h, sy)
    Uxm, Vxm, _ = CM.to_canvas(rec, surface, scale, u0, v0, sx - h, sy)
    Uyp, Vyp, _ = CM.to_canvas(rec, surface, scale, u0, v0, sx, sy + h)
    Uym, Vym, _ = CM.to_canvas(rec, surface, scale, u0, v0, sx, sy - h)
    j = lambda p, m: np.abs(p - m) / (2 * h)
    bU = 1.01 * (j(Uxp, Uxm) * ex + j(Uyp, Uym) * ey) + 2.0 ** -24 * np.abs(U) + 64 * CM.EPS * (np.abs(U) + math.pi * scale)
    bV = 1.01 * (j(Vxp, Vxm) * ex + j(Vyp, Vym) * ey) + 2.0 ** -24 * np.abs(V) + 64 * CM.EPS * (np.abs(V) + math.pi * scale)
    return bU, bV


def round_trip_points(rec, surface, scale, u0, v0, n=300, seed=9):
    """Canvas positions (float32) whose source positions lie well inside the picture of `rec`."""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(5, W - 5, n), rng.uniform(5, H - 5, n)
    U, V, ok = CM.to_canvas(rec, surface, scale, u0, v0, x, y)
    assert ok.all()
    return np.stack([U, V], 1).astype(np.float32)


@pytest.mark.parametrize("surface", SURFACES)
def test_the_round_trip_bound_holds_on_the_model(surface):
    scale, u0, v0 = CM.CANVAS
    for rec in CM.cameras(5, True):
        p = round_trip_points(rec, surface, scale, u0, v0).astype(np.float64)
        sx, sy, cz, r2 = CM.to_source(rec, surface, scale, u0, v0, p[:, 0], p[:, 1])
        s32 = np.stack([sx, sy], 1).astype(np.float32).astype(np.float64)
        U, V, ok = CM.to_canvas(rec, surface, scale, u0, v0, s32[:, 0], s32[:, 1])
        bU, bV = round_trip_bound(rec, surface, scale, u0, v0, p[:, 0], p[:, 1])
        assert ok.all() and (np.abs(U.astype(np.float32) - p[:, 0]) <= bU).all() and (np.abs(V.astype(np.float32) - p[:, 1]) <= bV).all()
        assert bU.max() < 1e-3 and bV.max() < 1e-3           # (a bound that pins something)


# ------------------------------------------------------------------------------------------------ the kernel text on the host
def pack_case(recs, W, H, fmt, surface, scale, u0, v0, geoms, pts):
    pts = np.asarray(pts, np.float32)
    head = struct.pack("<8i3d", recs.shape[0], W, H, fmt, surface, pts.shape[1], pts.shape[0], 0, scale, u0, v0)
    return head + np.ascontiguousarray(recs, np.float64).tobytes() + np.asarray(geoms, np.int32).tobytes() + pts.tobytes()


def check_to_canvas(got, rec, surface, scale, u0, v0, pts, what):
    """Point results of source -> canvas against the float64 model: the NaN pattern where the position is not finite, the record holds a NaN,
    or the model says invalid (a point whose residual of the inverse lies within 1e-12 of the 1e-9 tolerance, or whose w.z lies within 1e-12 of
    0, may go either way); else within 64 EPS (|v| + pi scale) + a float32 rounding."""
    p = np.asarray(pts, np.float32).astype(np.float64)
    fin = np.isfinite(p).all(1) & (not np.isnan(rec).any())
    nanp = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 2) == CM.NANP
    assert (nanp[:, 0] == nanp[:, 1]).all() and nanp[~fin].all(), (what, "NaN / NaN")
    if not fin.any():
        return
    U, V, ok = CM.to_canvas(rec, surface, scale, u0, v0, p[:, 0], p[:, 1])
    with np.errstate(invalid="ignore"):
        ok = ok & ~np.isnan(U) & ~np.isnan(V) & fin
        sure = fin & (np.abs(p) < 1e6).all(1)               # (1e30 is a legal input but pins nothing)
    assert np.array_equal(~nanp[sure, 0], ok[sure]), (what, "validity", np.flatnonzero(sure & (~nanp[:, 0] != ok))[:4])
    m = sure & ok
    tol = lambda v: 64 * CM.EPS * (np.abs(v) + math.pi * scale) + 2.0 ** -23 * np.abs(v)
    assert (np.abs(got[m, 0] - U[m]) <= tol(U[m])).all() and (np.abs(got[m, 1] - V[m]) <= tol(V[m])).all(), (what, "to canvas")


ODD = np.array([[np.nan, 1], [2, np.nan], [np.inf, 0], [0, -np.inf], [1e30, 5], [-1e30, 1e30], [13.5, 7.25], [-1000.75, 2000.5]], np.float32)


@pytest.mark.skipif(CLANGXX is None, reason="clang++ (ROCm's) not available")
def test_kernel_source_text_on_the_host_under_sanitizers(tmp_path):
    """tests/cpp/camera_check.cpp: hg_k_camera.hip itself, compiled for the CPU behind the thread-index shim -- the field's workgroup as 256
    real threads, the point kernels lane after lane -- and run under ASan + UBSan on exact-size heap buffers: no byte outside a buffer is
    touched, and what the kernels compute is the model's by the GPU test's rules.  A stand-alone program; nothing is loaded into Python."""
    exe = str(tmp_path / "camera_check")
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wno-everything", "-pthread", "-I", os.path.join(cpp, "hip_stub"), "-I", CSRC, os.path.join(cpp, "camera_check.cpp"), "-o", exe],
                   check=True, cwd=str(tmp_path), timeout=600)
    scale, u0, v0 = CM.CANVAS
    geoms = [(-3, -2, 1, 1), (5, 7, 3, BAND - 1), (-120, -40, 256, BAND + 1), (-130, -45, 257, 2), (0, 0, 0, 4), (-300, -20, 513, 3)]
    worst0 = CM.WORST[0]
    k = 0
    for surface in SURFACES:
        for fmt, distort in ((HG.FIELD_COORDS, True), (HG.FIELD_INDEX, False)):
            recs = CM.cameras(len(geoms), distort)
            if fmt == HG.FIELD_COORDS:
                recs[3, CM.K2] = np.nan                      # frame 3 fails alone
            gU, gV = (a.ravel() for a in CM.window_positions(geoms[2]))
            gcov = CM.covered(recs[2], *CM.to_source(recs[2], surface, scale, u0, v0, gU, gV), W, H)
            pick = np.sort(np.concatenate([np.flatnonzero(gcov)[::7][:200], np.flatnonzero(~gcov)[::7][:100]]))     # pixels of frame 2, covered and not
            grid = np.stack([gU[pick], gV[pick]], 1).astype(np.float32)
            src = np.stack([np.linspace(-20, W + 20, 40), np.linspace(H + 10, -10, 40)], 1).astype(np.float32)
            pts = np.stack([np.concatenate([grid, ODD, src]), np.concatenate([grid, ODD[::-1], src[::-1]])])
            case = (recs, W, H, fmt, surface, scale, u0, v0, geoms, pts)
            fin, fout = tmp_path / f"case{k}.in", tmp_path / f"case{k}.out"
            fin.write_bytes(pack_case(*case))
            p = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=600)
            assert p.returncode == 0 and "host check ran" in p.stdout, (k, p.stdout[-2000:], p.stderr[-3000:])
            out = fout.read_bytes()
            px = 4 if fmt == HG.FIELD_INDEX else 8
            offs, _ = CM.pack256(geoms, px)
            fbytes = max(o + g[2] * g[3] * px for o, g in zip(offs, geoms) if g[2] > 0 and g[3] > 0)
            n_pts = pts.shape[1]
            assert len(out) == fbytes + 2 * len(geoms) * n_pts * 8
            raw = np.frombuffer(out, np.uint8, fbytes)
            untouched = np.ones(fbytes, bool)
            for f, g in enumerate(geoms):
                n = max(g[2], 0) * max(g[3], 0) * px
                untouched[offs[f]:offs[f] + n] = False
                if n:
                    CM.check_field_frame(out[offs[f]:offs[f] + n], recs[f], g, W, H, surface, scale, u0, v0, fmt == HG.FIELD_INDEX, (k, f))
            assert (raw[untouched] == 0xA5).all(), "bytes between the frames must not be written"
            to_src = np.frombuffer(out, np.float32, len(geoms) * n_pts * 2, fbytes).reshape(len(geoms), n_pts, 2)
            to_cnv = np.frombuffer(out, np.float32, len(geoms) * n_pts * 2, fbytes + len(geoms) * n_pts * 8).reshape(len(geoms), n_pts, 2)
            for f in range(len(geoms)):
                lst = pts[f % 2].astype(np.float64)
                fin_ = np.isfinite(lst).all(1)
                assert (to_src[f][~fin_].view(np.uint32) == CM.NANP).all()
                CM.check_to_source(np.ascontiguousarray(to_src[f][fin_]).tobytes(), recs[f], surface, scale, u0, v0, lst[fin_, 0], lst[fin_, 1], what=(k, f, "to source"))
                check_to_canvas(to_cnv[f], recs[f], surface, scale, u0, v0, pts[f % 2], (k, f))
            if fmt == HG.FIELD_COORDS:                       # a point on a pixel repeats the field's bits where the pixel is covered
                fld = np.frombuffer(out, np.uint32, geoms[2][2] * geoms[2][3] * 2, offs[2]).reshape(-1, 2)[pick]
                cov = fld[:, 0] != CM.NANP
                assert cov.sum() >= 100 and np.array_equal(to_src[2][:pick.size].view(np.uint32)[cov], fld[cov])
            k += 1
    print(f"largest |host kernel - model| / delta: {CM.WORST[0]:.3g}; {CM.STORED[1]} of {CM.STORED[0]} stored coordinates are not float32(model)")
    assert CM.WORST[0] >= worst0 and CM.STORED[0] > 10000


# ------------------------------------------------------------------------------------------------ the drop-in class
@pytest.mark.skipif(shutil.which("node") is None, reason="node is missing")
def test_js_class_warp_camera_over_the_recording_mock_addon():
    """tests/js/camera_class.mjs: h.warpCamera(cameras, options) and h.cameraFromMatrices(...) over a recording mock addon: the records it
    packs, the default windows, the option defaults and output codes, the bare strings it throws, the shape of the result."""
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "camera_class.mjs")], capture_output=True, text=True, timeout=300,
                       cwd=ROOT, env=dict(os.environ, HGWARP_ADDON=os.path.join(ROOT, "tests", "js", "mock_camera_addon.cjs")))
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads(line[-1])
    assert res["ok"] and res["fails"] == [] and p.returncode == 0, (res["fails"], p.stderr[-2000:])
    assert res["checks"] >= 30
