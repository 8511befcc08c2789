"""Numpy model of the 8-bit bilinear remap and of the remaps of whole frame sets (include/hgwarp.h, hg_remap_*_frames_device).  Test
infrastructure only; everything rests on tests/hgtest/field.py.

    remap_bilinear_u8    remap_bilinear_f32 over the bytes widened to f32, then minimum(255, floor(v + f32(0.5))) -- blend4's rounding
    pack                 the packed layout both hg_pack_field_offsets and hg_pack_plane_offsets give: 256-byte aligned starts
    frames model         frame f is a flat list of obj_w * obj_h pixels and reads plane f % n_planes"""
import numpy as np

from . import field as FM

F32 = np.float32


def remap_bilinear_u8(coords, src):
    """coords: (n, 2) float32; src: (H, W, C) uint8.  Returns (n, C) uint8."""
    src = np.asarray(src)
    assert src.dtype == np.uint8
    v = FM.remap_bilinear_f32(coords, src.astype(F32))
    r = np.minimum(F32(255), np.floor(v + F32(0.5)))
    assert r.dtype == F32
    return r.astype(np.uint8)


def n_px(g):
    return g[2] * g[3] if g[2] > 0 and g[3] > 0 else 0


def pack(geoms, px_bytes):
    offs, off = [], 0
    for g in geoms:
        offs.append(off)
        off += (n_px(g) * px_bytes + 255) // 256 * 256
    return offs, off


def index_frames(geoms, fields, planes):
    """fields[f]: int32 (n_px,); planes: list of (n_src, pixel_bytes) uint8.  Per frame the (n_px, pixel_bytes) bytes."""
    return [FM.remap_index(fields[f], planes[f % len(planes)]) for f in range(len(geoms))]


def bilinear_frames(geoms, coords, planes):
    """coords[f]: (n_px, 2) float32; planes: list of (H, W, C) float32 or uint8.  Per frame (n_px, C) of the planes' type."""
    fn = remap_bilinear_u8 if planes[0].dtype == np.uint8 else FM.remap_bilinear_f32
    return [fn(coords[f], planes[f % len(planes)]) for f in range(len(geoms))]
