"""What the entry points that check before they bind refuse, and in which words: a table of bad argument lists with the (code, message)
pair each one gets -- the first failing check's, written out here.  No device is needed: the context is NULL, the device pointers are small
fake integers, and every case returns before anything is dereferenced (a legal list ends at "ctx is NULL", behind every check of its own).
HGWARP_LIB runs the same table against another build of the library."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "homography.js_amd"))
import hgwarp as HG                          # noqa: E402

OK, INVALID = 0, 1
SZ = C.c_size_t
INF, NAN = float("inf"), float("nan")
IDX, CO = HG.FIELD_INDEX, HG.FIELD_COORDS


def geoms(*g):
    return (HG.Geom * len(g))(*(HG.Geom(*w) for w in g))


def sizes(*v):
    return (SZ * len(v))(*v)


G2 = geoms((0, 0, 3, 2), (-1, 4, 0, 5))      # a 3 x 2 window and an empty one
EMPTY = geoms((0, 0, 0, 5), (0, 0, 3, -1))
FAR = geoms((1 << 27, 0, 3, 2))
NO_CTX = (INVALID, "ctx is NULL")
FMT = (INVALID, "unknown field format (HG_FIELD_INDEX or HG_FIELD_COORDS)")
LIMIT = (INVALID, "HG_FIELD_INDEX: the source has 2^31 pixels or more (an int32 cannot index it)")
OFFSET = (INVALID, "field offsets must be multiples of the field's pixel size (4 or 8 bytes)")
WINDOW = (INVALID, "output window offset beyond 2^26 pixels")
DONE = (OK, None)


def cam_field(rec=64, g=G2, n=2, W=64, H=48, surface=2, scale=100.0, u0=0.0, v0=0.0, fmt=CO, offs=None, field=256):
    return HG.lib().hg_field_camera_frames_device(None, rec, g, n, W, H, surface, scale, u0, v0, fmt, offs, field)


def cam_points(name):
    def call(rec=64, n=2, surface=1, scale=50.0, u0=0.0, v0=0.0, pts=128, n_pts=10, n_sets=1, out=256):
        return getattr(HG.lib(), name)(None, rec, n, surface, scale, u0, v0, pts, n_pts, n_sets, out)
    return call


def tps_field(rec=64, n_points=4, g=G2, n=2, W=64, H=48, fmt=CO, step=4, offs=None, field=256, scratch=512):
    return HG.lib().hg_field_tps_frames_device(None, rec, n_points, g, n, W, H, fmt, step, offs, field, scratch)


def tps_points(rec=64, n_points=4, n=2, pts=128, n_pts=10, n_sets=1, out=256):
    return HG.lib().hg_points_tps_frames_device(None, rec, n_points, n, pts, n_pts, n_sets, out)


def flow_layout(W=8, H=6, channels=1, n=2, n_to=1, levels=2, out=True):
    return HG.lib().hg_flow_layout(W, H, channels, n, n_to, levels, C.byref(SZ()) if out else None)


def tps_layout(g=G2, n=2, step=4, out=True):
    return HG.lib().hg_tps_field_layout(g, n, step, C.byref(SZ()) if out else None)


def mb_layout(g=G2, n=2, canvas=(0, 0, 2, 2), channels=3, bands=2, out=True):
    return HG.lib().hg_mosaic_multiband_layout(g, n, HG.Geom(*canvas), channels, bands, C.byref(SZ()) if out else None)


def fit_samples(kind=HG.HG_AFFINE, n=2, counts=None, n_points=8, n_hyp=3, out=True):
    cn = (C.c_int32 * len(counts))(*counts) if counts else None
    return HG.lib().hg_fit_sample_indices(kind, 7, n, cn, n_points, n_hyp, (C.c_int32 * (max(n, 1) * max(n_hyp, 1) * 4))() if out else None)


def pack_field(g=G2, n=2, fmt=CO, offs=True, total=True):
    return HG.lib().hg_pack_field_offsets(g, n, fmt, sizes(0, 0) if offs else None, C.byref(SZ()) if total else None)


def pack_plane(g=G2, n=2, px=3, offs=True, total=True):
    return HG.lib().hg_pack_plane_offsets(g, n, px, sizes(0, 0) if offs else None, C.byref(SZ()) if total else None)


def pyr_layout(W=5, H=3, elem=HG.ELEM_U8, channels=1, levels=2, offs=True, total=True):
    return HG.lib().hg_pyramid_layout(W, H, elem, channels, levels, (SZ * 32)() if offs else None, C.byref(SZ()) if total else None)


CAM, TPS = "hg_field_camera_frames_device: ", "hg_field_tps_frames_device: "
SURFACE = (INVALID, "camera: unknown surface (HG_SURFACE_PLANE, HG_SURFACE_CYLINDER or HG_SURFACE_SPHERE)")
SCALE = (INVALID, "camera: scale must be finite and > 0")
U0V0 = (INVALID, "camera: u0 and v0 must be finite")
CAM_FRAMES = (INVALID, "camera: n_frames must be 0..4096")
TPS_POINTS = (INVALID, "tps: n_points must be 3..1024")
TPS_FRAMES = (INVALID, "tps: n_frames must be 0..4096")
TPS_STEP = (INVALID, "tps: step must be 1, 2, 4, 8, 16 or 32")
FLOW_SHAPE = (INVALID, "flow: W and H must be 1..32768 and W * H <= 2^30")
MB = "hg_mosaic_multiband_layout: "

CASES = [
    # ------------------------------------------------------------------------------------------------ the camera's field
    (cam_field, dict(surface=3), SURFACE), (cam_field, dict(surface=-1), SURFACE),
    (cam_field, dict(fmt=2), FMT), (cam_field, dict(fmt=-1), FMT),
    (cam_field, dict(scale=0.0), SCALE), (cam_field, dict(scale=NAN), SCALE), (cam_field, dict(scale=INF), SCALE),
    (cam_field, dict(u0=INF), U0V0), (cam_field, dict(v0=NAN), U0V0),
    (cam_field, dict(W=0), (INVALID, CAM + "W and H must be >= 1")), (cam_field, dict(H=-1), (INVALID, CAM + "W and H must be >= 1")),
    (cam_field, dict(n=4097), CAM_FRAMES), (cam_field, dict(n=-1), CAM_FRAMES),
    (cam_field, dict(g=None), (INVALID, "camera: geoms is NULL")),
    (cam_field, dict(n=0), DONE), (cam_field, dict(n=0, g=None, rec=None, field=None), DONE),
    (cam_field, dict(g=FAR, n=1), WINDOW),
    (cam_field, dict(fmt=IDX, W=65536, H=32768), LIMIT), (cam_field, dict(fmt=IDX, W=65536, H=32767), NO_CTX), (cam_field, dict(W=65536, H=32768), NO_CTX),
    (cam_field, dict(offs=sizes(4, 0)), OFFSET), (cam_field, dict(offs=sizes(0, 4)), OFFSET),       # (an empty window's offset is checked too)
    (cam_field, dict(fmt=IDX, offs=sizes(2, 0)), OFFSET), (cam_field, dict(fmt=IDX, offs=sizes(4, 0)), NO_CTX),
    (cam_field, dict(g=EMPTY), DONE), (cam_field, dict(g=EMPTY, rec=None, field=None), DONE),
    (cam_field, dict(rec=None), (INVALID, CAM + "d_records / d_field is NULL")), (cam_field, dict(field=None), (INVALID, CAM + "d_records / d_field is NULL")),
    (cam_field, dict(rec=12), (INVALID, CAM + "d_records must be aligned to 8 bytes, d_field to its pixel size")),
    (cam_field, dict(field=12), (INVALID, CAM + "d_records must be aligned to 8 bytes, d_field to its pixel size")),
    (cam_field, dict(fmt=IDX, field=12), NO_CTX), (cam_field, dict(fmt=IDX, field=10), (INVALID, CAM + "d_records must be aligned to 8 bytes, d_field to its pixel size")),
    (cam_field, dict(), NO_CTX),
    # the earlier check wins
    (cam_field, dict(surface=3, fmt=2), SURFACE), (cam_field, dict(fmt=2, scale=0.0), FMT), (cam_field, dict(n=4097, g=None), CAM_FRAMES),
    (cam_field, dict(g=FAR, n=1, fmt=IDX, W=65536, H=32768), WINDOW), (cam_field, dict(fmt=IDX, W=65536, H=32768, offs=sizes(2, 0)), LIMIT),
    (cam_field, dict(offs=sizes(4, 0), rec=None), OFFSET), (cam_field, dict(rec=None, field=12), (INVALID, CAM + "d_records / d_field is NULL")),
    # ------------------------------------------------------------------------------------------------ the splines' field
    (tps_field, dict(n_points=2), TPS_POINTS), (tps_field, dict(n_points=1025), TPS_POINTS), (tps_field, dict(n_points=3), NO_CTX), (tps_field, dict(n_points=1024), NO_CTX),
    (tps_field, dict(n=4097), TPS_FRAMES), (tps_field, dict(n=-1), TPS_FRAMES),
    (tps_field, dict(step=3), TPS_STEP), (tps_field, dict(step=0), TPS_STEP), (tps_field, dict(step=64), TPS_STEP),
    (tps_field, dict(g=None), (INVALID, "tps: geoms is NULL")),
    (tps_field, dict(fmt=2), FMT),
    (tps_field, dict(W=0), (INVALID, TPS + "W and H must be >= 1")),
    (tps_field, dict(fmt=IDX, W=65536, H=32768), LIMIT), (tps_field, dict(W=65536, H=32768), NO_CTX),
    (tps_field, dict(n=0), DONE),
    (tps_field, dict(g=FAR, n=1), WINDOW),
    (tps_field, dict(offs=sizes(4, 0)), OFFSET), (tps_field, dict(offs=sizes(0, 12)), OFFSET), (tps_field, dict(fmt=IDX, offs=sizes(6, 0)), OFFSET),
    (tps_field, dict(fmt=IDX, offs=sizes(4, 0)), NO_CTX),
    (tps_field, dict(g=EMPTY), DONE),
    (tps_field, dict(rec=None), (INVALID, TPS + "d_records / d_field / d_scratch is NULL")),
    (tps_field, dict(scratch=None), (INVALID, TPS + "d_records / d_field / d_scratch is NULL")), (tps_field, dict(scratch=None, step=1), NO_CTX),
    (tps_field, dict(rec=12), (INVALID, TPS + "d_records must be aligned to 8 bytes, d_field to its pixel size, d_scratch to 16 bytes")),
    (tps_field, dict(field=12), (INVALID, TPS + "d_records must be aligned to 8 bytes, d_field to its pixel size, d_scratch to 16 bytes")),
    (tps_field, dict(fmt=IDX, field=12), NO_CTX),
    (tps_field, dict(scratch=520), (INVALID, TPS + "d_records must be aligned to 8 bytes, d_field to its pixel size, d_scratch to 16 bytes")),
    (tps_field, dict(), NO_CTX),
    (tps_field, dict(n_points=2, step=3), TPS_POINTS), (tps_field, dict(step=3, fmt=2), TPS_STEP), (tps_field, dict(fmt=2, W=0), FMT),
    (tps_field, dict(W=-65536, H=-32768, fmt=IDX), (INVALID, TPS + "W and H must be >= 1")), (tps_field, dict(fmt=IDX, W=65536, H=32768, n=0), LIMIT),
    # ------------------------------------------------------------------------------------------------ the splines' points
    (tps_points, dict(n_points=2), TPS_POINTS), (tps_points, dict(n_points=1025), TPS_POINTS), (tps_points, dict(n=4097), TPS_FRAMES),
    (tps_points, dict(n_pts=-1), (INVALID, "hg_points_tps_frames_device: n_pts must be 0..2^24")),
    (tps_points, dict(n_pts=(1 << 24) + 1), (INVALID, "hg_points_tps_frames_device: n_pts must be 0..2^24")),
    (tps_points, dict(n_sets=0), (INVALID, "hg_points_tps_frames_device: n_sets must be >= 1")),
    (tps_points, dict(n=0), DONE), (tps_points, dict(n_pts=0, rec=None), DONE),
    (tps_points, dict(pts=None), (INVALID, "hg_points_tps_frames_device: d_records / d_points / d_out is NULL")),
    (tps_points, dict(rec=12), (INVALID, "hg_points_tps_frames_device: d_records / d_points / d_out must be aligned to 8 bytes")),
    (tps_points, dict(pts=132), (INVALID, "hg_points_tps_frames_device: d_records / d_points / d_out must be aligned to 8 bytes")),
    (tps_points, dict(out=260), (INVALID, "hg_points_tps_frames_device: d_records / d_points / d_out must be aligned to 8 bytes")),
    (tps_points, dict(), NO_CTX),
    # ------------------------------------------------------------------------------------------------ the layouts
    (flow_layout, dict(W=0), FLOW_SHAPE), (flow_layout, dict(H=32769), FLOW_SHAPE), (flow_layout, dict(W=32768, H=32768), DONE),
    (flow_layout, dict(channels=3), (INVALID, "flow: channels must be 1 or 4")),
    (flow_layout, dict(levels=0), (INVALID, "flow: levels must be 1..min(hg_pyramid_levels(W, H), 12)")),
    (flow_layout, dict(levels=5), (INVALID, "flow: levels must be 1..min(hg_pyramid_levels(W, H), 12)")), (flow_layout, dict(levels=4), DONE),
    (flow_layout, dict(n=4097), (INVALID, "flow: n_frames must be 0..4096")), (flow_layout, dict(n=-1), (INVALID, "flow: n_frames must be 0..4096")),
    (flow_layout, dict(n_to=0), (INVALID, "flow: n_to_sets must be 1..max(n_frames, 1)")), (flow_layout, dict(n_to=3), (INVALID, "flow: n_to_sets must be 1..max(n_frames, 1)")),
    (flow_layout, dict(n=0, n_to=1), DONE),
    (flow_layout, dict(out=False), (INVALID, "hg_flow_layout: scratch_bytes is NULL")), (flow_layout, dict(), DONE),
    (tps_layout, dict(n=4097), TPS_FRAMES), (tps_layout, dict(step=3), TPS_STEP), (tps_layout, dict(g=None), (INVALID, "tps: geoms is NULL")),
    (tps_layout, dict(out=False), (INVALID, "hg_tps_field_layout: scratch_bytes is NULL")), (tps_layout, dict(), DONE), (tps_layout, dict(n=0, g=None), DONE),
    (mb_layout, dict(out=False), (INVALID, MB + "work_bytes is NULL")),
    (mb_layout, dict(n=65536), (INVALID, MB + "n_frames must be 0..65535")), (mb_layout, dict(n=-1), (INVALID, MB + "n_frames must be 0..65535")),
    (mb_layout, dict(channels=0), (INVALID, MB + "channels must be 1..4")), (mb_layout, dict(channels=5), (INVALID, MB + "channels must be 1..4")),
    (mb_layout, dict(bands=0), (INVALID, MB + "n_bands must be 1..8")), (mb_layout, dict(bands=9), (INVALID, MB + "n_bands must be 1..8")),
    (mb_layout, dict(g=None), (INVALID, MB + "NULL pointer")), (mb_layout, dict(g=None, n=0), DONE),
    (mb_layout, dict(canvas=(1 << 27, 0, 2, 2)), WINDOW), (mb_layout, dict(g=FAR, n=1), WINDOW),
    (mb_layout, dict(), DONE), (mb_layout, dict(canvas=(0, 0, 0, 5)), DONE),
    # ------------------------------------------------------------------------------------------------ host-only entries
    (fit_samples, dict(kind=2), (INVALID, "fit: unknown kind")),
    (fit_samples, dict(n_points=-1), (INVALID, "fit: n_points must be 0..65536")), (fit_samples, dict(n_points=65537), (INVALID, "fit: n_points must be 0..65536")),
    (fit_samples, dict(n_hyp=65537), (INVALID, "fit: n_hyp must be 0..65536")),
    (fit_samples, dict(n=4097, out=False), (INVALID, "fit: n_frames must be 0..4096")), (fit_samples, dict(n=-1), (INVALID, "fit: n_frames must be 0..4096")),
    (fit_samples, dict(counts=(8, 9)), (INVALID, "fit: counts[1] must be 0..n_points")), (fit_samples, dict(counts=(-1, 9)), (INVALID, "fit: counts[0] must be 0..n_points")),
    (fit_samples, dict(out=False), (INVALID, "hg_fit_sample_indices: out is NULL")),
    (fit_samples, dict(n=0, out=False), DONE), (fit_samples, dict(n_hyp=0, out=False), DONE), (fit_samples, dict(counts=(8, 0)), DONE), (fit_samples, dict(), DONE),
    (pack_field, dict(g=None), (INVALID, "hg_pack_field_offsets: bad arguments")), (pack_field, dict(n=-1), (INVALID, "hg_pack_field_offsets: bad arguments")),
    (pack_field, dict(fmt=2), (INVALID, "hg_pack_field_offsets: bad arguments")), (pack_field, dict(offs=False), (INVALID, "hg_pack_field_offsets: bad arguments")),
    (pack_field, dict(total=False), (INVALID, "hg_pack_field_offsets: bad arguments")), (pack_field, dict(), DONE), (pack_field, dict(fmt=IDX, n=0), DONE),
    (pack_plane, dict(g=None), (INVALID, "hg_pack_plane_offsets: bad arguments")), (pack_plane, dict(n=-1), (INVALID, "hg_pack_plane_offsets: bad arguments")),
    (pack_plane, dict(px=0), (INVALID, "hg_pack_plane_offsets: bad arguments")), (pack_plane, dict(offs=False), (INVALID, "hg_pack_plane_offsets: bad arguments")),
    (pack_plane, dict(total=False), (INVALID, "hg_pack_plane_offsets: bad arguments")), (pack_plane, dict(), DONE),
    (pyr_layout, dict(elem=2), (INVALID, "hg_pyramid_layout: bad arguments")), (pyr_layout, dict(channels=0), (INVALID, "hg_pyramid_layout: bad arguments")),
    (pyr_layout, dict(channels=5), (INVALID, "hg_pyramid_layout: bad arguments")), (pyr_layout, dict(levels=0), (INVALID, "hg_pyramid_layout: bad arguments")),
    (pyr_layout, dict(levels=5), (INVALID, "hg_pyramid_layout: bad arguments")), (pyr_layout, dict(W=0), (INVALID, "hg_pyramid_layout: bad arguments")),
    (pyr_layout, dict(offs=False), (INVALID, "hg_pyramid_layout: bad arguments")), (pyr_layout, dict(total=False), (INVALID, "hg_pyramid_layout: bad arguments")),
    (pyr_layout, dict(levels=4), DONE), (pyr_layout, dict(), DONE),
]

# both camera points calls: the same checks under their own names
for _name in ("hg_points_camera_to_source_frames_device", "hg_points_camera_to_canvas_frames_device"):
    _f = cam_points(_name)
    CASES += [
        (_f, dict(surface=7), SURFACE), (_f, dict(scale=-2.0), SCALE), (_f, dict(v0=-INF), U0V0), (_f, dict(n=4097), CAM_FRAMES), (_f, dict(n=-3), CAM_FRAMES),
        (_f, dict(n_pts=(1 << 24) + 1), (INVALID, _name + ": n_pts must be 0..2^24")), (_f, dict(n_pts=-1), (INVALID, _name + ": n_pts must be 0..2^24")),
        (_f, dict(n_sets=0), (INVALID, _name + ": n_sets must be >= 1")),
        (_f, dict(n=0, rec=None), DONE), (_f, dict(n_pts=0, pts=None), DONE),
        (_f, dict(rec=None), (INVALID, _name + ": d_records / d_points / d_out is NULL")), (_f, dict(out=None), (INVALID, _name + ": d_records / d_points / d_out is NULL")),
        (_f, dict(rec=12), (INVALID, _name + ": d_records / d_points / d_out must be aligned to 8 bytes")),
        (_f, dict(pts=132), (INVALID, _name + ": d_records / d_points / d_out must be aligned to 8 bytes")),
        (_f, dict(out=257), (INVALID, _name + ": d_records / d_points / d_out must be aligned to 8 bytes")),
        (_f, dict(), NO_CTX),
        (_f, dict(surface=7, scale=-2.0), SURFACE), (_f, dict(n=4097, n_pts=-1), CAM_FRAMES), (_f, dict(n_sets=0, rec=None), (INVALID, _name + ": n_sets must be >= 1")),
    ]


def test_the_table_covers_every_entry_it_names():
    assert len(CASES) >= 150
    assert len({f for f, _, _ in CASES}) == 12


@pytest.mark.parametrize("k", range(len(CASES)))
def test_first_failing_check_and_its_words(k):
    call, args, (code, message) = CASES[k]
    got = call(**args)
    text = HG.lib().hg_last_error(None).decode()
    assert got == code, (args, got, text)
    if message is not None:
        assert text == message, (args, text)
