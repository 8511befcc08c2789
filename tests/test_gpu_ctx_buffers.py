"""The context's buffers and staging rings on the GPU (csrc/hg_mem.h): a stale pointer or capacity after a buffer regrows, or a staging slot
rewritten too early, shows as a wrong frame -- tiny shapes find it.  One context is driven through growing and shrinking meshes and frame sets,
through more geometric / field / remap uploads than their staging rings have slots, and through a deferred redo out of an old staging slot;
every result is compared with the same call on a fresh context and with the oracle.  tests/test_ctx_mem_cpu.py pins the policy itself."""
import functools

import numpy as np
import pytest

from hgtest import field as FM
from hgtest import golden as G
from hgtest import hip
from hgtest import oracle as O
from hgtest import workloads as WL

pytestmark = pytest.mark.gpu

HG = hip.load()
IDX = HG.FIELD_INDEX
W, H = 48, 32
SMALL, LARGE = (40, 24), (72, 40)            # output windows (the self-span path wants at least 16 columns)


@functools.lru_cache(maxsize=None)
def _image():
    img = G.lcg_image(W, H, 41).copy()
    img.setflags(write=False)
    return img


# ------------------------------------------------------------------------------------------------ grow, shrink, grow
# (cells of the source grid, windows of the frames): 2 triangles x 1 frame, 18 x 5, 2 x 2
STEPS = [(1, [SMALL]), (3, [SMALL, LARGE, LARGE, SMALL, LARGE]), (1, [LARGE, SMALL])]


@functools.lru_cache(maxsize=None)
def _step(k):
    """Mesh and frames of step k: the source grid stretched over each frame's window, every vertex nudged by a fraction of a cell."""
    n, windows = STEPS[k]
    sp, tris = WL.grid_points(W, H, n, n), WL.grid_triangles(n, n)
    frames = []
    for f, (w, h) in enumerate(windows):
        p = sp.reshape(-1, 2).astype(np.float64) * [w / W, h / H]
        i = np.arange(p.shape[0])
        p += np.stack([np.sin(1.0 + i + f + k), np.cos(2.0 + 3 * i + f - k)], 1) * [w / (5.0 * n), h / (5.0 * n)]
        frames.append(p.astype(np.float32).ravel())
    geoms = [(0, 0, w, h) for w, h in windows]
    return sp, tris, WL.src_min(sp), frames, geoms


def _run_step(c, k):
    """Every call of the step on context c (its image is set): the frame set, then the single-frame forms on its last frame."""
    sp, tris, ms, frames, geoms = _step(k)
    offs, total = HG.pack_offsets(geoms)
    c.piecewise_set_mesh(sp, tris, ms[0], ms[1])
    res = {}
    d_out = c.alloc(total)
    try:
        c.piecewise_set_frames(np.concatenate(frames), geoms, offs)
        c.warp_inverse_piecewise_frames_device(d_out)
        for f, g in enumerate(geoms):
            res["frame", f] = c.to_host(d_out, g[2] * g[3] * 4, offs[f]).reshape(g[3], g[2], 4)
    finally:
        c.free(d_out)
    dp, g = frames[-1], geoms[-1]
    c.piecewise_prepare(dp, g)
    res["via_map"] = c.warp_inverse_piecewise_via_map()
    res["tri_map"] = c.get_tri_map()
    res["fwd"], res["inv"] = c.get_matrices(tris.size // 3)
    mm = [int(v) for v in O.minmax_xy(sp)]
    res["forward"] = c.warp_forward_piecewise(dp, mm[2], mm[3], g)
    res["state"] = c.warp_inverse_piecewise_state(res["fwd"], dp, tris, ms[0], ms[1], g)
    return res


@functools.lru_cache(maxsize=None)
def _fresh_steps():
    """Each step on a context of its own that has seen nothing else."""
    out = []
    for k in range(len(STEPS)):
        with HG.Context(0) as c:
            c.set_image(_image())
            out.append(_run_step(c, k))
    return out


@functools.lru_cache(maxsize=None)
def _oracle_step(k):
    sp, tris, ms, frames, geoms = _step(k)
    img = _image()
    want = {("frame", f): O.warp_inverse_piecewise(sp, frames[f], tris, img, ms[0], ms[1], *geoms[f]) for f in range(len(frames))}
    dp, g = frames[-1], geoms[-1]
    want["via_map"], want["tri_map"], want["fwd"], want["inv"] = O.warp_inverse_piecewise(sp, dp, tris, img, ms[0], ms[1], *g, taps=True)
    mm = [int(v) for v in O.minmax_xy(sp)]
    fmap = O.build_tri_map(sp, tris, mm[2] - mm[0], mm[1], (mm[2] - mm[0]) * (mm[3] - mm[1]))
    want["forward"] = O.warp_forward_piecewise(fmap, O.piecewise_matrices(sp, dp, tris), img, mm[0], mm[1], mm[2], mm[3], *g)
    inv = np.stack([O.inverse_affine(m) for m in np.asarray(want["fwd"], np.float32).reshape(-1, 6)])
    want["state"] = O.warp_inverse_piecewise_loop(want["tri_map"], inv, img, ms[0], ms[1], *g)
    return want


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b).reshape(np.shape(a))
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _same_f32(a, b):
    """Bit-equal but for the sign of a zero and the payload of a NaN (the bar of tests/test_gpu_parity.py for the matrices)."""
    a, b = np.ascontiguousarray(a, np.float32).ravel(), np.ascontiguousarray(b, np.float32).ravel()
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)) | ((a == 0) & (b == 0))))


@pytest.mark.parametrize("options", [{}, {"min_row_groups": 0, "self_spans": 1}], ids=["auto", "self_spans"])
def test_grow_shrink_grow_on_one_context(options):
    """Meshes of 2, 18, 2 triangles and frame sets of 1, 5, 2 frames on ONE context: every buffer of the frame set, of the one-frame scratch and
    of the staging slots regrows in step 2 and is larger than its contents in step 3.  Every call's result is byte-equal to the fresh context's
    and to the oracle's."""
    fresh = _fresh_steps()
    with HG.Context(0) as c:
        for key, v in options.items():
            c.set_option(key, v)
        c.set_image(_image())
        for k in range(len(STEPS)):
            got, want = _run_step(c, k), _oracle_step(k)
            assert set(got) == set(fresh[k]) == set(want)
            for key in got:
                assert _same(got[key], fresh[k][key]), (k, key, "differs from a fresh context")
                assert (_same_f32 if key in ("fwd", "inv") else _same)(got[key], want[key]), (k, key, "differs from the oracle")


# ------------------------------------------------------------------------------------------------ the two short rings
GEO = (33, 17)


def _geo_call(k, lap):
    """Frames of call k of a loop over a ring revisited every `lap` calls: 1 or 3 frames, alternating from call to call and from visit to visit
    of a slot (so a slot that held one frame is handed three at its next visit); matrices and windows of their own."""
    n = 3 if (k + k // lap) % 2 else 1
    mats = np.zeros((n, 8))
    for f in range(n):
        mats[f, :6] = [1.0 + 0.01 * k, 0.02 * (f + 1), -0.03, 0.9 - 0.01 * f, 0.5 * k - 3.0, 1.0 + f]      # source = M * output pixel
    geoms = [(f - 1, k % 5 - 2, GEO[0], GEO[1]) for f in range(n)]
    return mats, geoms


@functools.lru_cache(maxsize=None)
def _fresh_geo(n_calls, lap):
    """Frame by frame through the single-frame host calls, on one fresh context: the picture and the index field of every frame."""
    out = []
    with HG.Context(0) as c:
        c.set_image(_image())
        for k in range(n_calls):
            mats, geoms = _geo_call(k, lap)
            out.append([(c.warp_inverse_geometric(0, mats[f], geoms[f]), c.field_inverse_geometric(0, mats[f], geoms[f], IDX)) for f in range(len(geoms))])
    return out


SLOT = 3 * 2304                              # bytes of a call's output: up to three frames of 33 x 17 pixels of 4 bytes, packed


def test_geometric_sets_lap_their_staging_ring():
    """20 geometric frame sets through the ring of 8 staging slots, each warped right behind its upload into a place of its own; the host
    waits for nothing until all of them are queued."""
    want = _fresh_geo(20, 8)
    img = _image()
    with HG.Context(0) as c:
        c.set_image(img)
        d_out = c.alloc(20 * SLOT)
        try:
            calls = []
            for k in range(20):
                mats, geoms = _geo_call(k, 8)
                offs, total = HG.pack_offsets(geoms)
                assert total <= SLOT
                offs = [k * SLOT + o for o in offs]
                c.geometric_set_frames(0, mats, geoms, offs)
                c.warp_inverse_geometric_frames_device(d_out)
                calls.append((mats, geoms, offs))
            c.sync()
            for k, (mats, geoms, offs) in enumerate(calls):
                for f, g in enumerate(geoms):
                    got = c.to_host(d_out, g[2] * g[3] * 4, offs[f]).reshape(g[3], g[2], 4)
                    assert _same(got, want[k][f][0]), (k, f)
                    assert _same(got, O.warp_inverse_geometric(0, mats[f], img, *g)), (k, f, "oracle")
        finally:
            c.free(d_out)


def test_field_and_remap_tables_share_their_staging_ring():
    """10 x (fields of a geometric set, then a frames remap of the source through them): 20 frame tables through the ring of 4 slots, and
    10 frame sets through the ring of 8, all queued before the host waits for anything."""
    want = _fresh_geo(10, 2)
    img = _image()
    src = img.reshape(-1, 4)
    with HG.Context(0) as c:
        c.set_image(img)
        d_src, d_field, d_out = c.alloc(src.nbytes), c.alloc(10 * SLOT), c.alloc(10 * SLOT)
        try:
            c.to_device(d_src, src)
            calls = []
            for k in range(10):
                mats, geoms = _geo_call(k, 2)
                offs, total = HG.pack_field_offsets(geoms, IDX)
                assert total <= SLOT and (offs, total) == HG.pack_plane_offsets(geoms, 4)
                offs = [k * SLOT + o for o in offs]
                c.geometric_set_frames(0, mats, geoms)
                c.field_inverse_geometric_frames_device(IDX, d_field, offs)
                c.remap_index_frames_device(geoms, d_field, d_src, W * H, 1, 0, 4, d_out, offs, offs)
                calls.append((geoms, offs))
            c.sync()
            for k, (geoms, offs) in enumerate(calls):
                for f, g in enumerate(geoms):
                    field = c.to_host(d_field, g[2] * g[3] * 4, offs[f]).view(np.int32)
                    assert _same(field, want[k][f][1]), (k, f, "field")
                    got = c.to_host(d_out, g[2] * g[3] * 4, offs[f])
                    assert _same(got, FM.remap_index(want[k][f][1], src)), (k, f, "remap")
        finally:
            c.free(d_out); c.free(d_field); c.free(d_src)


# ------------------------------------------------------------------------------------------------ a deferred redo out of an old staging slot
def test_deferred_redo_reads_its_own_staging_slot_after_newer_uploads():
    """A set of 3 frames whose frame 1 has a NaN vertex is queued: the fused run only flags that frame.  Three sets of 2 frames are uploaded
    behind it (other slots of the ring, other sizes; the device copy of the set is overwritten) without a sync.  hg_sync then redoes the flagged
    frame from the slot its set was staged in.  (tests/test_gpu_parity.py::test_fresh_point_sets_queue_without_settling_and_redo_from_their_own_set
    covers overflowing sets of one frame count, each of them warped.)"""
    img = _image()
    sp, tris = WL.grid_points(W, H, 4, 3), WL.grid_triangles(4, 3)
    ms = WL.src_min(sp)
    frames = [WL.sin_dst(sp, 2.0 + f, 8 + f) for f in range(3)]
    geoms = [WL.piecewise_geom(frames[0])] * 3                # (one window for all: the NaN frame has none of its own)
    frames[1] = frames[1].copy(); frames[1][4] = np.nan      # an x coordinate: its triangles keep their rows and are irregular
    later = [[WL.sin_dst(sp, 7.0 + s, 5 + f) for f in range(2)] for s in range(3)]
    offs, total = HG.pack_offsets(geoms)
    with HG.Context(0) as c:
        c.set_image(img)
        c.piecewise_set_mesh(sp, tris, ms[0], ms[1])
        c.set_option("min_row_groups", 0); c.set_option("self_spans", 1)      # (k_tri_setup in front: the row lists would simply draw nothing for a NaN triangle)
        d_out = c.alloc(total)
        try:
            c.sync()
            redone = c.redone_frames()
            c.piecewise_set_frames(np.concatenate(frames), geoms, offs)
            c.warp_inverse_piecewise_frames_device(d_out)
            assert c.last_piecewise_self() == 1
            for s in range(3):
                c.piecewise_set_frames(np.concatenate(later[s]), [WL.piecewise_geom(d) for d in later[s]])
            assert c.redone_frames() == redone, "the run was settled before the sync: nothing was deferred"
            c.sync()
            assert c.redone_frames() >= redone + 1
            for f, g in enumerate(geoms):
                want = O.warp_inverse_piecewise(sp, frames[f], tris, img, ms[0], ms[1], *g)
                assert _same(c.to_host(d_out, g[2] * g[3] * 4, offs[f]).reshape(g[3], g[2], 4), want), f
        finally:
            c.free(d_out)
