"""What the entry points that bind first refuse, and in which words: the table of tests/test_api_checks_cpu.py for the field, remap, mosaic and
points calls, which need a context (and hence a device) before their first check.  Every case returns before any launch: a 2 x 2 canvas, one
3 x 2 frame, device pointers given as small fake integers that nothing dereferences.  HGWARP_LIB runs the same table against another build."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "homography.js_amd"))
import hgwarp as HG                          # noqa: E402

pytestmark = pytest.mark.gpu

INVALID, STATE = 1, 4
SZ = C.c_size_t
IDX, CO = HG.FIELD_INDEX, HG.FIELD_COORDS
F32, U8 = HG.ELEM_F32, HG.ELEM_U8
G1 = (HG.Geom * 1)(HG.Geom(0, 0, 3, 2))
CANVAS = (0, 0, 2, 2)
IDENTITY = (C.c_double * 8)(1, 0, 0, 0, 1, 0, 0, 0)
FMT = (INVALID, "unknown field format (HG_FIELD_INDEX or HG_FIELD_COORDS)")
OFFSET = (INVALID, "field offsets must be multiples of the field's pixel size (4 or 8 bytes)")
OFFSET8 = "field offsets must be multiples of the field's pixel size (8 bytes)"
OUT_OFFSET = (INVALID, "output offsets must be multiples of pixel_bytes (index) or of the element size (bilinear)")
NO_IMAGE = (STATE, "no source image: a field needs its size (hg_set_image)")
POINTS_ALIGN = (INVALID, "d_points / d_out must be aligned to 8 bytes (interleaved x,y float32)")
POINTS_NULL = (INVALID, "d_points / d_out is NULL")


def sizes(*v):
    return (SZ * len(v))(*v)


def L():
    return HG.lib()


# ------------------------------------------------------------------------------------------------ the calls, with a legal argument list as defaults
def field_one(h, kind=HG.HG_AFFINE, m=IDENTITY, fmt=CO, field=256):
    return L().hg_field_inverse_geometric_device(h, kind, m, G1[0], fmt, field)


def field_one_host(h, fmt=CO, out=True):
    return L().hg_field_inverse_geometric(h, HG.HG_AFFINE, IDENTITY, G1[0], fmt, C.cast((C.c_uint8 * 64)(), C.c_void_p) if out else None)


def field_geo(h, fmt=CO, offs=None, field=256):
    return L().hg_field_inverse_geometric_frames_device(h, fmt, offs, field)


def field_pw(h, fmt=CO, offs=None, field=256):
    return L().hg_field_inverse_piecewise_frames_device(h, fmt, offs, field)


def field_pw_host(h, fmt=CO, out=True):
    return L().hg_field_inverse_piecewise(h, fmt, C.cast((C.c_uint8 * 64)(), C.c_void_p) if out else None)


def remap_index(h, field=256, n_px=6, src=512, n_src=4, pb=4, out=1024):
    return L().hg_remap_index_device(h, field, n_px, src, n_src, pb, out)


def remap_f32(h, coords=256, n_px=6, src=512, W=2, H=2, ch=3, out=1024):
    return L().hg_remap_bilinear_f32_device(h, coords, n_px, src, W, H, ch, out)


def remap_u8(h, coords=256, n_px=6, src=512, W=2, H=2, ch=3, out=1024):
    return L().hg_remap_bilinear_u8_device(h, coords, n_px, src, W, H, ch, out)


def index_frames(h, g=G1, n=1, field=256, foffs=None, planes=512, n_src=4, n_planes=1, stride=64, pb=4, out=1024, ooffs=None):
    return L().hg_remap_index_frames_device(h, g, n, field, foffs, planes, n_src, n_planes, stride, pb, out, ooffs)


def flat_frames(name, *tail):
    def call(h, g=G1, n=1, coords=256, foffs=None, planes=512, W=2, H=2, n_planes=1, stride=64, elem=F32, ch=3, out=1024, ooffs=None, tail=tail):
        return getattr(L(), name)(h, g, n, coords, foffs, planes, W, H, n_planes, stride, elem, ch, out, ooffs, *tail)
    return call


def compose(h, g=G1, n=1, outer=256, foffs=None, inner=512, W=2, H=2, n_inner=1, stride=64, out=1024, ooffs=None):
    return L().hg_field_compose_frames_device(h, g, n, outer, foffs, inner, W, H, n_inner, stride, out, ooffs)


def mosaic(name):
    def call(h, g=G1, n=1, coords=256, foffs=None, frames=512, poffs=None, elem=F32, ch=3, W=2, H=2, mode=HG.MOSAIC_MEAN, feather=1.0, canvas=CANVAS,
             out=1024, weight=2048, gains=(1.0,)):
        tail = ((C.c_float * len(gains))(*gains),) if name == "hg_mosaic_frames_gain_device" else ()
        return getattr(L(), name)(h, g, n, coords, foffs, frames, poffs, elem, ch, W, H, mode, feather, HG.Geom(*canvas), out, weight, *tail)
    return call


def robust(h, g=G1, n=1, coords=256, foffs=None, frames=512, poffs=None, ch=3, mode=HG.ROBUST_MEDIAN, trim=0.25, gains=None, canvas=CANVAS, out=1024, weight=2048):
    gp = (C.c_float * len(gains))(*gains) if gains else None
    return L().hg_mosaic_robust_device(h, g, n, coords, foffs, frames, poffs, ch, mode, trim, gp, HG.Geom(*canvas), out, weight)


def stats(h, g=G1, n=1, coords=256, foffs=None, frames=512, poffs=None, ch=3, canvas=CANVAS, out=1024):
    return L().hg_mosaic_overlap_stats_device(h, g, n, coords, foffs, frames, poffs, ch, HG.Geom(*canvas), out)


def multiband(h, g=G1, n=1, coords=256, foffs=None, frames=512, poffs=None, elem=F32, ch=3, W=2, H=2, feather=1.0, bands=2, canvas=CANVAS, out=1024,
              weight=2048, labels=4096, work=8192, work_bytes=0):
    return L().hg_mosaic_multiband_device(h, g, n, coords, foffs, frames, poffs, elem, ch, W, H, feather, bands, HG.Geom(*canvas), out, weight, labels, None,
                                          work, work_bytes)


def points_src(name):
    def call(h, pts=256, n_pts=4, n_sets=1, out=512):
        return getattr(L(), name)(h, pts, n_pts, n_sets, out)
    return call


def points_out_geo(h, pts=256, n_pts=4, n_sets=1, out=512, kind=HG.HG_AFFINE):
    return L().hg_points_to_output_geometric_batch_device(h, kind, IDENTITY, G1, 1, pts, n_pts, n_sets, out)


def points_out_pw(h, pts=256, n_pts=4, n_sets=1, out=512, n=1):
    return L().hg_points_to_output_piecewise_batch_device(h, (C.c_float * 8)(), 1, 1, G1, n, pts, n_pts, n_sets, out)


def fit(h, matches=256, mats=512, counts=1024, best=None, samples=None, min_mats=None):
    return L().hg_fit_matches_frames_device(h, HG.HG_AFFINE, matches, 8, None, 1, 1.0, 4, 7, samples, 0, mats, min_mats, counts, best, None)


def frames_cases(name, call, mip=False):
    """What check_remap_frames and the frame table refuse, under the entry point's name."""
    p = name + ": "
    align = (INVALID, p + "d_coords must be aligned to 8 bytes, d_planes / d_out / plane_stride_bytes to the element size")
    rows = [(call, dict(elem=2), (INVALID, p + "unknown elem (HG_ELEM_F32 or HG_ELEM_U8)")),
            (call, dict(ch=0), (INVALID, p + "channels must be 1..4, W and H >= 1")), (call, dict(ch=5), (INVALID, p + "channels must be 1..4, W and H >= 1")),
            (call, dict(W=0), (INVALID, p + "channels must be 1..4, W and H >= 1")),
            (call, dict(n_planes=0), (INVALID, p + "n_planes must be >= 1")),
            (call, dict(n=-1), (INVALID, p + "n_frames must be 0..65535")), (call, dict(n=65536), (INVALID, p + "n_frames must be 0..65535")),
            (call, dict(n=0, g=None, coords=None), (0, None)),
            (call, dict(g=None), (INVALID, p + "NULL pointer")), (call, dict(planes=None), (INVALID, p + "NULL pointer")),
            (call, dict(coords=260), align), (call, dict(planes=514), align), (call, dict(out=1026), align), (call, dict(stride=66), align),
            (call, dict(elem=U8, planes=513, out=1027, stride=67, coords=260), align),
            (call, dict(foffs=sizes(4)), OFFSET), (call, dict(ooffs=sizes(2)), OUT_OFFSET),
            (call, dict(elem=2, ch=5), (INVALID, p + "unknown elem (HG_ELEM_F32 or HG_ELEM_U8)")), (call, dict(coords=260, foffs=sizes(4)), align)]
    if mip:
        rows += [(call, dict(tail=(4096, 64, 0) + call.__defaults__[-1][3:]), (INVALID, p + "levels must lie in 1..hg_pyramid_levels(W, H)")),
                 (call, dict(tail=(4096, 64, 3) + call.__defaults__[-1][3:]), (INVALID, p + "levels must lie in 1..hg_pyramid_levels(W, H)")),
                 (call, dict(tail=(None, 64, 2) + call.__defaults__[-1][3:]), (INVALID, p + "d_pyr is NULL with levels > 1")),
                 (call, dict(tail=(4098, 64, 2) + call.__defaults__[-1][3:]), (INVALID, p + "d_pyr / pyr_stride_bytes must be aligned to the element size"))]
    return rows


def mosaic_cases(name):
    call, p = mosaic(name), name + ": "
    align = (INVALID, p + "d_coords must be aligned to 8 bytes, d_frames / d_canvas to the element size, d_weight to 4")
    rows = [(call, dict(n=-1), (INVALID, p + "n_frames must be 0..65535")), (call, dict(n=65536), (INVALID, p + "n_frames must be 0..65535")),
            (call, dict(out=None), (INVALID, p + "d_canvas is NULL")),
            (call, dict(elem=2), (INVALID, p + "unknown elem (HG_ELEM_F32 or HG_ELEM_U8)")),
            (call, dict(mode=3), (INVALID, p + "unknown mode (HG_MOSAIC_LAST, HG_MOSAIC_MEAN or HG_MOSAIC_FEATHER)")),
            (call, dict(ch=0), (INVALID, p + "channels must be 1..4, W and H >= 1")), (call, dict(ch=5), (INVALID, p + "channels must be 1..4, W and H >= 1")),
            (call, dict(H=0), (INVALID, p + "channels must be 1..4, W and H >= 1")),
            (call, dict(mode=HG.MOSAIC_FEATHER, feather=0.0), (INVALID, p + "feather must be > 0 (+Inf: uncapped)")),
            (call, dict(coords=None), (INVALID, p + "NULL pointer")), (call, dict(g=None), (INVALID, p + "NULL pointer")),
            (call, dict(coords=260), align), (call, dict(frames=514), align), (call, dict(out=1026), align), (call, dict(weight=2050), align),
            (call, dict(canvas=(1 << 27, 0, 2, 2)), (INVALID, "output window offset beyond 2^26 pixels")),
            (call, dict(foffs=sizes(4)), (INVALID, OFFSET8)), (call, dict(poffs=sizes(2)), (INVALID, p + "frame offsets must be multiples of the element size")),
            (call, dict(n=65536, elem=2), (INVALID, p + "n_frames must be 0..65535")), (call, dict(elem=2, ch=0), (INVALID, p + "unknown elem (HG_ELEM_F32 or HG_ELEM_U8)")),
            (call, dict(canvas=(0, 0, 0, 5)), (0, None))]
    if name == "hg_mosaic_frames_gain_device":
        rows += [(call, dict(gains=(0.0,)), (INVALID, p + "every gain must be finite and > 0")), (call, dict(gains=(float("inf"),)), (INVALID, p + "every gain must be finite and > 0")),
                 (call, dict(gains=(0.0,), foffs=sizes(4)), (INVALID, p + "every gain must be finite and > 0"))]
    return rows


R, S, M = "hg_mosaic_robust_device: ", "hg_mosaic_overlap_stats_device: ", "hg_mosaic_multiband_device: "
BILINEAR = flat_frames("hg_remap_bilinear_frames_device")
BICUBIC = flat_frames("hg_remap_bicubic_frames_device", 0.0, 0.5)
TRILINEAR = flat_frames("hg_remap_trilinear_frames_device", 4096, 64, 1)
ANISO = flat_frames("hg_remap_aniso_frames_device", 4096, 64, 1, 4)

# cases on a fresh context: no image, no mesh, no frames
CASES = [
    (field_one, dict(kind=2), (INVALID, "hg_field_inverse_geometric: bad arguments")), (field_one, dict(m=None), (INVALID, "hg_field_inverse_geometric: bad arguments")),
    (field_one, dict(field=None), (INVALID, "hg_field_inverse_geometric: bad arguments")), (field_one, dict(fmt=2), FMT), (field_one, dict(), NO_IMAGE),
    (field_one_host, dict(out=False), (INVALID, "out is NULL")), (field_one_host, dict(fmt=2), FMT), (field_one_host, dict(), NO_IMAGE),
    (field_geo, dict(field=None), (INVALID, "d_field is NULL")), (field_geo, dict(fmt=-1), FMT), (field_geo, dict(), NO_IMAGE), (field_geo, dict(fmt=IDX), NO_IMAGE),
    (field_pw, dict(field=None), (INVALID, "d_field is NULL")), (field_pw, dict(fmt=2), FMT), (field_pw, dict(), (STATE, "no source image: call hg_set_image first")),
    (field_pw_host, dict(out=False), (INVALID, "out is NULL")), (field_pw_host, dict(fmt=2), FMT), (field_pw_host, dict(), (STATE, "no source image: call hg_set_image first")),
    # the single-plane remaps
    (remap_index, dict(pb=3), (INVALID, "hg_remap_index_device: pixel_bytes must be 1, 2, 4, 8 or 16")), (remap_index, dict(n_px=0, field=None), (0, None)),
    (remap_index, dict(field=None), (INVALID, "hg_remap_index_device: NULL pointer")), (remap_index, dict(src=None), (INVALID, "hg_remap_index_device: NULL pointer")),
    (remap_index, dict(field=258), (INVALID, "hg_remap_index_device: d_src / d_out must be aligned to pixel_bytes, d_field to 4 bytes")),
    (remap_index, dict(src=514), (INVALID, "hg_remap_index_device: d_src / d_out must be aligned to pixel_bytes, d_field to 4 bytes")),
    (remap_index, dict(pb=16, out=1032), (INVALID, "hg_remap_index_device: d_src / d_out must be aligned to pixel_bytes, d_field to 4 bytes")),
    (remap_f32, dict(ch=5), (INVALID, "hg_remap_bilinear_f32_device: channels must be 1..4, W and H >= 1")), (remap_f32, dict(n_px=0, coords=None), (0, None)),
    (remap_f32, dict(out=None), (INVALID, "hg_remap_bilinear_f32_device: NULL pointer")),
    (remap_f32, dict(coords=260), (INVALID, "hg_remap_bilinear_f32_device: d_coords must be aligned to 8 bytes, d_src / d_out to 4")),
    (remap_f32, dict(src=514), (INVALID, "hg_remap_bilinear_f32_device: d_coords must be aligned to 8 bytes, d_src / d_out to 4")),
    (remap_f32, dict(out=1025), (INVALID, "hg_remap_bilinear_f32_device: d_coords must be aligned to 8 bytes, d_src / d_out to 4")),
    (remap_u8, dict(W=0), (INVALID, "hg_remap_bilinear_u8_device: channels must be 1..4, W and H >= 1")), (remap_u8, dict(src=None), (INVALID, "hg_remap_bilinear_u8_device: NULL pointer")),
    (remap_u8, dict(coords=260), (INVALID, "hg_remap_bilinear_u8_device: d_coords must be aligned to 8 bytes")),
    # the index frames remap
    (index_frames, dict(pb=5), (INVALID, "hg_remap_index_frames_device: pixel_bytes must be 1, 2, 4, 8 or 16")),
    (index_frames, dict(n_planes=0), (INVALID, "hg_remap_index_frames_device: n_planes must be >= 1")),
    (index_frames, dict(n=65536), (INVALID, "hg_remap_index_frames_device: n_frames must be 0..65535")), (index_frames, dict(n=0, g=None), (0, None)),
    (index_frames, dict(out=None), (INVALID, "hg_remap_index_frames_device: NULL pointer")),
    (index_frames, dict(field=258), (INVALID, "hg_remap_index_frames_device: d_planes / d_out / plane_stride_bytes must be aligned to pixel_bytes, d_field to 4 bytes")),
    (index_frames, dict(pb=8, planes=516), (INVALID, "hg_remap_index_frames_device: d_planes / d_out / plane_stride_bytes must be aligned to pixel_bytes, d_field to 4 bytes")),
    (index_frames, dict(stride=66), (INVALID, "hg_remap_index_frames_device: d_planes / d_out / plane_stride_bytes must be aligned to pixel_bytes, d_field to 4 bytes")),
    (index_frames, dict(foffs=sizes(2)), OFFSET), (index_frames, dict(ooffs=sizes(2)), OUT_OFFSET), (index_frames, dict(pb=2, ooffs=sizes(2), foffs=sizes(6)), OFFSET),
    # the chained field
    (compose, dict(out=1028), (INVALID, "hg_field_compose_frames_device: d_out must be aligned to 8 bytes")), (compose, dict(ooffs=sizes(4)), OUT_OFFSET),
    (compose, dict(n_inner=0), (INVALID, "hg_field_compose_frames_device: n_planes must be >= 1")),
    # bicubic, anisotropic: the checks in front of the shared ones
    (BICUBIC, dict(tail=(1.5, 0.5)), (INVALID, "hg_remap_bicubic_frames_device: B must lie in [0, 1]")),
    (BICUBIC, dict(tail=(0.0, float("nan"))), (INVALID, "hg_remap_bicubic_frames_device: C must lie in [0, 1]")),
    (ANISO, dict(tail=(4096, 64, 1, 0)), (INVALID, "hg_remap_aniso_frames_device: max_aniso must lie in 1..16")),
    (ANISO, dict(tail=(4096, 64, 1, 17), elem=2), (INVALID, "hg_remap_aniso_frames_device: max_aniso must lie in 1..16")),
    # the robust mosaic, the overlap statistics, the multi-band mosaic
    (robust, dict(n=65536), (INVALID, R + "n_frames must be 0..256")), (robust, dict(n=-1), (INVALID, R + "n_frames must be 0..256")),
    (robust, dict(out=None), (INVALID, R + "d_canvas is NULL")), (robust, dict(ch=5), (INVALID, R + "channels must be 1..4")),
    (robust, dict(frames=None), (INVALID, R + "NULL pointer")),
    (robust, dict(coords=260), (INVALID, R + "d_coords must be aligned to 8 bytes, d_weight to 4")), (robust, dict(weight=2049), (INVALID, R + "d_coords must be aligned to 8 bytes, d_weight to 4")),
    (robust, dict(foffs=sizes(4)), (INVALID, R + OFFSET8)), (robust, dict(canvas=(0, 1 << 27, 2, 2)), (INVALID, R + "output window offset beyond 2^26 pixels")),
    (robust, dict(mode=4), (INVALID, R + "unknown mode (HG_ROBUST_MEDIAN, HG_ROBUST_TRIMMED, HG_ROBUST_MIN or HG_ROBUST_MAX)")),
    (robust, dict(mode=HG.ROBUST_TRIMMED, trim=0.5), (INVALID, R + "trim must lie in [0, 0.5)")),
    (robust, dict(gains=(-1.0,)), (INVALID, R + "every gain must be finite and > 0")), (robust, dict(canvas=(0, 0, 0, 5)), (0, None)),
    (stats, dict(n=257), (INVALID, S + "n_frames must be 0..256")), (stats, dict(ch=0), (INVALID, S + "channels must be 1..4")),
    (stats, dict(out=None), (INVALID, S + "NULL pointer")), (stats, dict(coords=260), (INVALID, S + "d_coords and d_stats must be aligned to 8 bytes")),
    (stats, dict(out=1028), (INVALID, S + "d_coords and d_stats must be aligned to 8 bytes")), (stats, dict(foffs=sizes(12)), (INVALID, OFFSET8)),
    (stats, dict(n=0, g=None, out=None), (0, None)),
    (multiband, dict(n=65536), (INVALID, M + "n_frames must be 0..65535")), (multiband, dict(elem=2), (INVALID, M + "unknown elem (HG_ELEM_F32 or HG_ELEM_U8)")),
    (multiband, dict(ch=5), (INVALID, M + "channels must be 1..4, W and H >= 1")), (multiband, dict(bands=9), (INVALID, M + "n_bands must be 1..8")),
    (multiband, dict(labels=4098), (INVALID, M + "d_coords must be aligned to 8 bytes, d_frames / d_canvas to the element size, d_weight / d_labels to 4")),
    (multiband, dict(coords=260), (INVALID, M + "d_coords must be aligned to 8 bytes, d_frames / d_canvas to the element size, d_weight / d_labels to 4")),
    (multiband, dict(foffs=sizes(4)), (INVALID, OFFSET8)), (multiband, dict(poffs=sizes(2)), (INVALID, M + "frame offsets must be multiples of the element size")),
    (multiband, dict(work=8200), (INVALID, M + "d_work must be aligned to 256 bytes and hold what hg_mosaic_multiband_layout returns")),
    (multiband, dict(), (INVALID, M + "d_work must be aligned to 256 bytes and hold what hg_mosaic_multiband_layout returns")),      # (work_bytes 0)
    (multiband, dict(canvas=(0, 0, 0, 5)), (0, None)),
    # the point lists: the shared checks come first in all four
    (points_out_geo, dict(kind=2), (INVALID, "hg_points_to_output_geometric: bad arguments")), (points_out_geo, dict(), (STATE, "no source image: call hg_set_image first")),
    (points_out_pw, dict(n=0), (INVALID, "hg_points_to_output_piecewise: bad arguments")),
    (fit, dict(matches=264), (INVALID, "hg_fit_matches_frames_device: d_matches must be aligned to 16 bytes ((x, y, u, v) float32)")),
    (fit, dict(mats=516), (INVALID, "hg_fit_matches_frames_device: d_mats / d_min_mats must be aligned to 8 bytes")),
    (fit, dict(min_mats=516), (INVALID, "hg_fit_matches_frames_device: d_mats / d_min_mats must be aligned to 8 bytes")),
    (fit, dict(best=1026), (INVALID, "hg_fit_matches_frames_device: d_counts / d_best / d_samples must be aligned to 4 bytes")),
    (fit, dict(mats=None), (INVALID, "hg_fit_matches_frames_device: d_matches / d_mats / d_counts is NULL")),
]
CASES += frames_cases("hg_remap_bilinear_frames_device", BILINEAR) + frames_cases("hg_remap_bicubic_frames_device", BICUBIC)
CASES += frames_cases("hg_remap_trilinear_frames_device", TRILINEAR, True) + frames_cases("hg_remap_aniso_frames_device", ANISO, True)
CASES += mosaic_cases("hg_mosaic_frames_device") + mosaic_cases("hg_mosaic_frames_gain_device")
for _f in (points_src("hg_points_to_source_geometric_frames_device"), points_src("hg_points_to_source_piecewise_frames_device"), points_out_geo, points_out_pw):
    CASES += [(_f, dict(n_pts=-1), (INVALID, "n_points must be 0..2^24")), (_f, dict(n_pts=(1 << 24) + 1), (INVALID, "n_points must be 0..2^24")),
              (_f, dict(n_sets=0), (INVALID, "n_sets must be >= 1")), (_f, dict(n_pts=0, pts=None, out=None), (0, None)),
              (_f, dict(pts=None), POINTS_NULL), (_f, dict(out=None), POINTS_NULL),
              (_f, dict(pts=260), POINTS_ALIGN), (_f, dict(out=514), POINTS_ALIGN), (_f, dict(pts=257, out=None), POINTS_NULL)]
CASES += [(points_src("hg_points_to_source_geometric_frames_device"), dict(), (STATE, "no source image: the coverage test needs its size (hg_set_image)")),
          (points_src("hg_points_to_source_piecewise_frames_device"), dict(), (STATE, "no source image: call hg_set_image first"))]

# cases on a context with a 2 x 2 image and, where it says so, one geometric 3 x 2 frame
WITH_IMAGE = [(field_geo, dict(), (STATE, "no frames: call hg_geometric_set_frames first")),
              (points_src("hg_points_to_source_geometric_frames_device"), dict(), (STATE, "no frames: call hg_geometric_set_frames first")),
              (field_pw, dict(), (STATE, "no mesh: call hg_piecewise_set_mesh first")),
              (field_one, dict(fmt=2), FMT)]
WITH_FRAME = [(field_geo, dict(offs=sizes(4)), OFFSET), (field_geo, dict(fmt=IDX, offs=sizes(6)), OFFSET), (field_geo, dict(fmt=2, offs=sizes(4)), FMT),
              (field_geo, dict(field=None, offs=sizes(4)), (INVALID, "d_field is NULL"))]


def run(h, rows):
    for call, args, (code, message) in rows:
        got = call(h, **args)
        text = L().hg_last_error(h).decode()
        assert got == code, (call.__name__, args, got, text)
        if message is not None:
            assert text == message, (call.__name__, args, text)


def test_refusals_of_the_entries_that_bind_first():
    assert len(CASES) >= 200
    with HG.Context(0) as c:
        run(c._h, CASES)
        c.set_image(np.zeros((2, 2, 4), np.uint8))
        run(c._h, WITH_IMAGE)
        c.geometric_set_frames(HG.HG_AFFINE, np.array([1, 0, 0, 0, 1, 0, 0, 0], np.float64), [(0, 0, 3, 2)])
        run(c._h, WITH_FRAME)
