"""The model of the FORWARD source field (hg_field_forward_*): no new restatement of the reference loops -- the oracle's forward warp of an
image whose pixel i (raster order) holds the little-endian uint32 i + 1 names the source pixel every output pixel was copied from.  Read as
uint32, minus 1: the flat source index of the last writer; 0 gives -1: nobody writes, or the last writer reads outside the source array (the
reference then stores undefined -> 0 over the earlier writers).  tests/test_forward_field_cpu.py checks the model before it judges a kernel.
CPU only."""
import numpy as np

from . import fwd_edges as F
from . import oracle as O


def _to_field(rgba):
    h, w = rgba.shape[:2]
    return (np.ascontiguousarray(rgba).view(np.uint32).reshape(h, w).astype(np.int64) - 1).astype(np.int32)


def geometric(kind, m, W, H, geom):
    """(obj_h, obj_w) int32: the field of hg_warp_forward_geometric(kind, m, geom) on a W x H source."""
    return _to_field(O.warp_forward_geometric(kind, np.asarray(m, np.float64)[:6 if kind == 0 else 8], F.rank_image(W, H), *geom))


def geometric_case(case):
    return geometric(case["kind"], case["m"], case["W"], case["H"], case["geom"])


def piecewise_case(case):
    """... of a piecewise case of fwd_edges (its W x H source, its source box and mesh)."""
    return _to_field(F.piecewise_oracle(case, F.rank_image(case["W"], case["H"])))


def gather(field, img):
    """out32[p] = field[p] >= 0 ? img32[field[p]] : 0, as (h, w, 4) uint8: what the field promises to reproduce."""
    flat = np.ascontiguousarray(img, np.uint8).reshape(-1, 4).view(np.uint32).ravel()
    f = field.ravel()
    assert f.max(initial=-1) < flat.size and f.min(initial=0) >= -1
    out = np.where(f >= 0, flat[np.where(f >= 0, f, 0)], np.uint32(0)).astype(np.uint32)
    return out.view(np.uint8).reshape(field.shape[0], field.shape[1], 4)
