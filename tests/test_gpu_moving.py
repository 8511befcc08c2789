"""Frame sets whose frames bring their own source points and source minima (hg_piecewise_set_frames_src) on the GPU: every inverse
piecewise kernel, frame index versus image index, the deferred redo from the staged source side, the general-path fallback, the taps and
the JavaScript class.  Expected bytes come from the CPU oracle called once per frame with that frame's source side (tests/hgtest/moving.py);
the premises that make wrong frame indexing visible are asserted in tests/test_moving_cpu.py."""
import hashlib
import json
import os
import tempfile

import numpy as np
import pytest

from hgtest import gpu_frames as GF
from hgtest import hip
from hgtest import moving as M
from hgtest import oracle as O
from hgtest import workloads as WL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HG = hip.load()
NEAR, BIL = HG.SAMPLE_NEAREST, HG.SAMPLE_BILINEAR
ERR_INVALID, ERR_STATE = 1, 4


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(-1))
        first = [(int(r), int(c), got[r, c].tolist(), want[r, c].tolist()) for r, c in bad[:6]]
        raise AssertionError(f"{what}: {len(bad)} of {got.shape[0] * got.shape[1]} pixels differ; (row, col, got, want): {first}")


def _nan_eq(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)) | ((a == 0) & (b == 0))))


class Rig:
    """A context with `n_images` of the set's images on the device (1: a shared source) and an output buffer for the set's packed frames."""

    def __init__(self, ms, opts=(), n_images=None, mode=NEAR):
        self.ms, self.NI = ms, ms.F if n_images is None else n_images
        self.c = HG.Context(0)
        for k, v in dict(opts).items():
            self.c.set_option(k, v)
        self.c.set_sampling(mode)
        self.mode = mode
        self.offs, self.total = HG.pack_offsets(ms.geoms)
        stride = ms.W * ms.H * 4
        self.d_src, self.d_out = self.c.alloc(stride * self.NI), self.c.alloc(self.total)
        for k in range(self.NI):
            self.c.to_device(self.d_src, ms.imgs[k], k * stride)
        if self.NI > 1:
            self.c.set_images_device(self.d_src, ms.W, ms.H, self.NI, stride)
        else:
            self.c.set_image_device(self.d_src, ms.W, ms.H)
        # the mesh-wide source side is NOT that of any frame: a kernel that still reads it gives wrong bytes
        self.c.piecewise_set_mesh(ms.base, ms.tris, *WL.src_min(ms.base))

    def run(self, batch=False, mins="own"):
        ms, c = self.ms, self.c
        mn = ms.min_all if mins == "own" else None
        if batch:
            c.warp_inverse_piecewise_src_batch_device(ms.src_all, mn, ms.dst_all, ms.geoms, self.offs, self.d_out)
        else:
            c.piecewise_set_frames_src(ms.src_all, mn, ms.dst_all, ms.geoms, self.offs)
            c.warp_inverse_piecewise_frames_device(self.d_out)

    def frame(self, f, d_out=None, offs=None):
        g = self.ms.geoms[f]
        return self.c.to_host(self.d_out if d_out is None else d_out, g[2] * g[3] * 4, (self.offs if offs is None else offs)[f]).reshape(g[3], g[2], 4)

    def check(self, what):
        self.c.sync()
        for f in range(self.ms.F):
            w = self.ms.want(f, None if self.NI == self.ms.F else self.NI)
            _same(self.frame(f), w[1] if self.mode == BIL else w[0], (what, f, self.c.last_piecewise_variant()))

    def close(self):
        self.c.free(self.d_out); self.c.free(self.d_src); self.c.close()


# ------------------------------------------------------------------------------------------------ 1. default policy

@pytest.mark.parametrize("mode", [NEAR, BIL], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("s", [4, -12])
def test_default_policy(s, mode):
    ms = M.set_a(s)
    r = Rig(ms, mode=mode)
    try:
        r0 = r.c.redone_frames()
        for batch in (False, True):
            for mins in ("own", None):
                r.run(batch=batch, mins=mins)
                r.check(("default", s, mode, batch, mins))
        assert r.c.redone_frames() == r0
        if mode == BIL:
            assert r.c.last_piecewise_kernel() == 4
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------ 2. every inverse kernel
# Set A: 48 triangles, windows 320 x ~215, at most 26 spans per row, 4 frames (216 four-row groups).  Options as in the forcing table of
# tests/test_gpu_edges.py; the expected (kernel code, variant with the high-dword bounds, variant with the fp64 bounds) follow
# plan_piecewise / launch_pw_rows / launch_pw_patch (variant codes: include/hgwarp.h).  shared: one source image for every frame.
ROWS_SELF = {"self_spans": 1, "patch": 0, "tile": 0, "compact": 0}
ROWS_LIST = {"self_spans": 0, "patch": 0, "tile": 0, "compact": 0}
FORCED = {
    # label: (options, shared source, kernel, variant hi-dword, variant fp64)
    "rows_self_g4": (dict(ROWS_SELF, min_row_groups=1), False, 1, 104011, 101001),
    "rows_self_g1": (dict(ROWS_SELF), False, 2, 104011, 101001),                              # default min_row_groups: a small set, one row per workgroup
    "rows_self_safe0": (dict(ROWS_SELF, min_row_groups=1, safe_spans=0), False, 1, 104011, 101001),
    "rows_self_safe1": (dict(ROWS_SELF, min_row_groups=1, safe_spans=1), False, 1, 104011, 101001),
    "rows_self_hi0": (dict(ROWS_SELF, min_row_groups=1, hi_bounds=0), False, 1, 101001, 101001),
    "rows_self_rot0": (dict(ROWS_SELF, min_row_groups=1, xcc_rotate=0), False, 1, 104011, 101001),
    "rows_self_rot1": (dict(ROWS_SELF, min_row_groups=1, xcc_rotate=1), False, 1, 104011, 101001),
    "rows_self_sub2": (dict(ROWS_SELF, min_row_groups=1, xcc_rotate=0, sub_bands=2), True, 1, 104011, 101001),
    "rows_self_xcc2": (dict(ROWS_SELF, min_row_groups=1, xcc=2), False, 1, 104011, 101001),
    "rows_ph4": (dict(ROWS_LIST, min_row_groups=1, phase=4), False, 1, 104010, 101000),
    "rows_ph4_safe1": (dict(ROWS_LIST, min_row_groups=1, phase=4, safe_spans=1), False, 1, 104010, 101000),
    "rows_ph4_hi0": (dict(ROWS_LIST, min_row_groups=1, phase=4, hi_bounds=0), False, 1, 101000, 101000),
    "rows_ph4_grouped": (dict(ROWS_LIST, min_row_groups=1, phase=4, tri_group=16), False, 1, 104010, 101000),
    "rows_ph2": (dict(ROWS_LIST, min_row_groups=1, phase=2), False, 1, 102010, 101000),
    "rows_ph2_s80": (dict(ROWS_LIST, min_row_groups=1, phase=2), True, 1, 302010, 101000),        # shared source: the 80-SGPR instantiation
    "rows_ph2_s80_sub2": (dict(ROWS_LIST, min_row_groups=1, phase=2, xcc_rotate=0, sub_bands=2), True, 1, 302010, 101000),
    "rows_ph1": (dict(ROWS_LIST, min_row_groups=1, phase=1), False, 1, 101010, 101000),
    "rows_ph1_g1": (dict(ROWS_LIST, phase=1), False, 2, 101010, 101000),
    "rows_compact": (dict(ROWS_LIST, compact=1, phase=2), False, 2, 102110, 101100),
    "rows_compact_grouped": (dict(ROWS_LIST, compact=1, phase=2, tri_group=16), False, 2, 102110, 101100),
    "rows_compact_ph1": (dict(ROWS_LIST, compact=1, phase=1), False, 2, 101110, 101100),
    "patch_self": ({"self_spans": 1, "patch": 1, "tile": 0, "min_row_groups": 1}, False, 3, 408011, 401001),
    "patch_self_safe0": ({"self_spans": 1, "patch": 1, "tile": 0, "min_row_groups": 1, "safe_spans": 0}, False, 3, 408011, 401001),
    "patch_self_hi0": ({"self_spans": 1, "patch": 1, "tile": 0, "min_row_groups": 1, "hi_bounds": 0}, False, 3, 401001, 401001),
    "patch_self_sub2": ({"self_spans": 1, "patch": 1, "tile": 0, "min_row_groups": 1, "xcc_rotate": 0, "sub_bands": 2}, True, 3, 408011, 401001),
    "patch_self_xcc2": ({"self_spans": 1, "patch": 1, "tile": 0, "min_row_groups": 1, "xcc": 2, "xcc_rotate": 1}, False, 3, 408011, 401001),
    "patch_lists": ({"self_spans": 0, "patch": 1, "tile": 0}, False, 3, 408010, 401000),
    "patch_lists_grouped": ({"self_spans": 0, "patch": 1, "tile": 0, "tri_group": 16}, False, 3, 408010, 401000),
    "patch_global": ({"self_spans": 0, "patch": 2, "tile": 0}, False, 3, 801010, 801000),
    "patch_global_hi0": ({"self_spans": 0, "patch": 2, "tile": 0, "hi_bounds": 0}, False, 3, 801000, 801000),
}


# s = -12 once per kernel family and list format (its fp64 instantiations do not depend on the other options)
MIXED_SIGNS = ["rows_self_g4", "rows_self_g1", "rows_ph4", "rows_ph2_s80", "rows_compact", "patch_self", "patch_lists", "patch_global"]


@pytest.mark.parametrize("label,s", [(k, 4) for k in FORCED] + [(k, -12) for k in MIXED_SIGNS])
def test_every_inverse_kernel(label, s):
    """s = 4: the forced instantiation in the bounds form its options ask for; s = -12 (minima of both signs in one set): its fp64 form,
    the variant's high-dword digit 0."""
    opts, shared, kernel, v_hib, v_fp64 = FORCED[label]
    ms = M.set_a(s)
    r = Rig(ms, opts, n_images=1 if shared else None)
    try:
        r.run()
        r.check((label, s))
        v = r.c.last_piecewise_variant()
        assert (r.c.last_piecewise_kernel(), v) == (kernel, v_hib if s == 4 else v_fp64), (label, s, r.c.last_piecewise_kernel(), v)
        if s == -12:
            assert (v // 10) % 10 == 0, v
        assert r.c.redone_frames() == 0
    finally:
        r.close()


WIDE = {
    "tile": ({"self_spans": 1, "patch": 1, "tile": 1, "min_row_groups": 1}, 5, 504011),
    "tile_hi0": ({"self_spans": 1, "patch": 1, "tile": 1, "min_row_groups": 1, "hi_bounds": 0}, 5, 504001),
    "patch_self": ({"self_spans": 1, "patch": 1, "tile": 0, "min_row_groups": 1}, 3, 408011),
    "patch_lists": ({"self_spans": 0, "patch": 1, "tile": 0}, 3, 408010),
    "rows_self_g4": (dict(ROWS_SELF, min_row_groups=1), 1, 104011),
    "rows_ph4": (dict(ROWS_LIST, min_row_groups=1, phase=4), 1, 104010),
    "rows_ph2": (dict(ROWS_LIST, min_row_groups=1, phase=2), 1, 102010),
}


@pytest.mark.parametrize("label", list(WIDE))
def test_wide_short_set(label):
    """2100 x 48, mesh 12 x 2, three frames: two column tiles of k_pw_tile / k_pw_patch, nine 256-pixel windows (the last one ragged) per row."""
    opts, kernel, variant = WIDE[label]
    ms = M.wide_set()
    assert all(g[2] > 2048 for g in ms.geoms)
    r = Rig(ms, opts)
    try:
        r.run()
        r.check(("wide", label))
        assert (r.c.last_piecewise_kernel(), r.c.last_piecewise_variant(), r.c.redone_frames()) == (kernel, variant, 0), \
            (label, r.c.last_piecewise_kernel(), r.c.last_piecewise_variant(), r.c.redone_frames())
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------ 3. frame index versus image index

@pytest.mark.parametrize("opts", [{"xcc_rotate": 1}, {"sub_bands": 2}], ids=["xcc_rotate1", "sub_bands2"])
def test_frame_index_versus_image_index(opts):
    """Five frames over three images: frame f reads image f % 3 but its OWN source side."""
    ms = M.set_a(4, 5)
    r = Rig(ms, opts, n_images=3)
    try:
        r.run()
        r.check(("5 frames over 3 images", opts))
        assert r.c.redone_frames() == 0
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------ 4. deferred redo

def _strip_sets():
    """Sets of three frames on a strip mesh of 1100 thin triangles over a 2400 x 8 source.  In `dense` frames every triangle keeps its rows:
    1100 spans per output row, beyond the 511 of the forced k_pw_rows<512>.  In the other frames only the first 40 triangles do (the rest
    are flattened onto y = 0: no rows).  Every frame has its own jittered, shifted source points; all windows are 2400 x 12."""
    n, W2, H2 = 1100, 2400, 8
    xs = np.linspace(0, W2, n + 1)
    base = np.stack([np.repeat(xs, 2), np.tile([0.0, H2], n + 1)], 1)
    tris = np.array([[2 * i, 2 * i + 2, 2 * i + 1] for i in range(n)], np.uint32).ravel()
    imgs = [WL.lcg_image(W2, H2, 60 + k) for k in range(3)]
    k = np.arange(base.shape[0])

    def frame(j, dense):
        src = np.stack([base[:, 0] + 3 + j + np.sin(0.3 * k + j), base[:, 1] + 1 + (j % 3) + 0.5 * np.cos(0.7 * k + j)], 1).astype(np.float32).ravel()
        d = base.copy()
        d[:, 1] *= 1.5
        if not dense:
            d[2 * 41:, 1] = 0.0
        return src, d.astype(np.float32).ravel()

    sets = []
    for si, dense_at in enumerate((1, None, None)):
        fr = [frame(3 * si + f, f == dense_at) for f in range(3)]
        sets.append(([a for a, _ in fr], [b for _, b in fr]))
    return W2, H2, tris, imgs, sets


def test_deferred_redo_uses_the_staged_source_side():
    W2, H2, tris, imgs, sets = _strip_sets()
    geom = (0, 0, W2, 12)
    for srcs, dsts in sets:
        assert all(WL.piecewise_geom(d) == geom for d in dsts)
    geoms = [geom] * 3
    offs, total = HG.pack_offsets(geoms)
    c = HG.Context(0)
    for k_, v in {"self_spans": 0, "patch": 0, "tile": 0, "compact": 1}.items():
        c.set_option(k_, v)
    stride = W2 * H2 * 4
    d_src = c.alloc(stride * 3)
    outs = [c.alloc(total) for _ in sets]
    try:
        for k_ in range(3):
            c.to_device(d_src, imgs[k_], k_ * stride)
        c.set_images_device(d_src, W2, H2, 3, stride)
        c.piecewise_set_mesh(sets[0][0][0], tris, 0, 0)
        c.sync()
        r0 = c.redone_frames()
        for (srcs, dsts), d_out in zip(sets, outs):
            c.piecewise_set_frames_src(np.concatenate(srcs), None, np.concatenate(dsts), geoms, offs)
            c.warp_inverse_piecewise_frames_device(d_out)
        assert c.last_piecewise_variant() == 111110, c.last_piecewise_variant()       # k_pw_rows<512>, 8-byte entries, high-dword bounds
        assert c.redone_frames() == r0, "the flagged frame is settled at hg_sync, not before"
        c.sync()
        assert c.redone_frames() == r0 + 1, c.redone_frames() - r0
        for si, ((srcs, dsts), d_out) in enumerate(zip(sets, outs)):
            for f in range(3):
                want = O.warp_inverse_piecewise(srcs[f], dsts[f], tris, imgs[f], *WL.src_min(srcs[f]), *geom)
                assert want.any()
                _same(c.to_host(d_out, W2 * 12 * 4, offs[f]).reshape(12, W2, 4), want, ("deferred redo", si, f))
    finally:
        for o in outs:
            c.free(o)
        c.free(d_src); c.close()


# ------------------------------------------------------------------------------------------------ 5. fallback routing

@pytest.mark.parametrize("coord", [0, 1], ids=["minSrcX", "minSrcY"])
def test_a_minimum_beyond_the_fast_range_takes_the_general_kernel(coord):
    ms = M.MovingSet(320, 200, 6, 4, 4, 4)
    sp = ms.srcs[2].copy()
    sp[2 * 9 + coord] = -float((1 << 22) + 3)
    ms.srcs[2] = sp
    ms.mins[2] = WL.src_min(sp)
    assert abs(ms.mins[2][coord]) >= 1 << 22 and all(abs(v) < 1 << 22 for f in (0, 1, 3) for v in ms.mins[f])
    r = Rig(ms)
    try:
        for mins in ("own", None):
            r.run(mins=mins)
            r.check(("fallback", coord, mins))
            assert (r.c.last_piecewise_kernel(), r.c.last_piecewise_variant()) == (4, 600000)
        assert r.c.redone_frames() == 0
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------ 6. taps and single-frame forms

@pytest.mark.parametrize("s", [4, -12])
def test_taps_and_single_frame_forms(s):
    ms = M.set_a(s)
    f = 2
    near, bil, cov, wmap, fwd, inv = ms.want(f)
    c = HG.Context(0)
    try:
        c.set_image(ms.imgs[f])
        c.piecewise_set_mesh(ms.base, ms.tris, *WL.src_min(ms.base))
        for mins in (np.asarray(ms.mins[f], np.int32), None):
            c.piecewise_set_frames_src(ms.srcs[f], mins, ms.dsts[f], [ms.geoms[f]])
            _same(c.warp_inverse_piecewise(), near, ("warp", s))
            _same(c.warp_inverse_piecewise_via_map(), near, ("via map", s))
            assert np.array_equal(c.get_tri_map(fused=False), wmap) and np.array_equal(c.get_tri_map(fused=True), wmap)
            gf, gi = c.get_matrices(ms.tris.size // 3)
            assert _nan_eq(gf, fwd) and _nan_eq(gi, inv)
        c.set_sampling(BIL)
        c.piecewise_set_frames_src(ms.srcs[f], None, ms.dsts[f], [ms.geoms[f]])
        _same(c.warp_inverse_piecewise(), bil, ("bilinear warp", s))
        _same(c.warp_inverse_piecewise_via_map(), bil, ("bilinear via map", s))
        c.set_sampling(NEAR)
        # a plain frame set returns to the mesh-wide source side
        msx, msy = WL.src_min(ms.base)
        plain = O.warp_inverse_piecewise(ms.base, ms.dsts[f], ms.tris, ms.imgs[f], msx, msy, *ms.geoms[f])
        assert not np.array_equal(plain, near)
        c.piecewise_set_frames(ms.dsts[f], [ms.geoms[f]], [0])
        d_out = c.alloc(plain.size)
        try:
            c.warp_inverse_piecewise_frames_device(d_out)
            c.sync()
            _same(c.to_host(d_out, plain.size).reshape(plain.shape), plain, ("plain set after a moving set", s))
        finally:
            c.free(d_out)
        c.piecewise_set_frames_src(ms.srcs[f], None, ms.dsts[f], [ms.geoms[f]])
        c.piecewise_prepare(ms.dsts[f], ms.geoms[f])
        _same(c.warp_inverse_piecewise(), plain, ("prepare after a moving set", s))
        assert c.redone_frames() == 0
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ 7. errors

def test_errors_and_the_transactional_rule():
    ms = M.set_a(4)
    c = HG.Context(0)
    try:
        c.set_image(ms.imgs[0])
        with pytest.raises(HG.HgError) as e:
            c._n_pts = ms.base.size // 2
            c.piecewise_set_frames_src(ms.src_all, None, ms.dst_all, ms.geoms)
        assert e.value.code == ERR_STATE
        c.piecewise_set_mesh(ms.base, ms.tris, *WL.src_min(ms.base))
        d_out = c.alloc(HG.pack_offsets(ms.geoms)[1])
        try:
            for bad in (np.inf, -np.inf, float((1 << 24) + 2), -float((1 << 24) + 2)):
                c.piecewise_set_frames_src(ms.src_all, None, ms.dst_all, ms.geoms)      # a good set first ...
                src = ms.src_all.copy()
                src[-3] = bad
                with pytest.raises(HG.HgError) as e:
                    c.piecewise_set_frames_src(src, None, ms.dst_all, ms.geoms)
                assert e.value.code == ERR_INVALID and "source coordinate is infinite or beyond 2^24" in str(e.value), str(e.value)
                with pytest.raises(HG.HgError) as e:                                    # ... which the refused call has taken away
                    c.warp_inverse_piecewise_frames_device(d_out)
                assert e.value.code == ERR_STATE
            L = HG.lib()
            g = HG._geoms(ms.geoms)
            s_, sp = HG._f32(ms.src_all)
            d_, dp = HG._f32(ms.dst_all)
            assert L.hg_piecewise_set_frames_src(c._h, None, None, dp, g, None, ms.F) == ERR_INVALID
            assert L.hg_piecewise_set_frames_src(c._h, sp, None, None, g, None, ms.F) == ERR_INVALID
            assert L.hg_piecewise_set_frames_src(c._h, sp, None, dp, None, None, ms.F) == ERR_INVALID
            assert L.hg_piecewise_set_frames_src(c._h, sp, None, dp, g, None, 0) == ERR_INVALID
            nan = ms.src_all.copy()
            nan[5] = np.nan                                                                 # NaN stays legal
            c.piecewise_set_frames_src(nan, None, ms.dst_all, ms.geoms)
            c.warp_inverse_piecewise_frames_device(d_out)
            c.sync()
        finally:
            c.free(d_out)
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ 8. the JavaScript class over the real addon

def test_js_class_warp_batch_with_source_points():
    """warpBatch(dst, {sourcePoints, images}) of the class for Set A, bilinear and nearest (every window is taller than the source: warp()
    picks the inverse loop).  The class mirrors the reference's caches: the source minima are refreshed only while its map field is null,
    so every frame is tested against frame 0's minima (:252, :756-758) -- the oracle is called with exactly that."""
    ms = M.set_a(4)
    assert all(g[3] > ms.H for g in ms.geoms)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "set_a.json")
        with open(path, "w") as fh:
            json.dump({"W": ms.W, "H": ms.H, "seed0": 40, "tris": [int(t) for t in ms.tris],
                       "src": [[float(v) for v in a] for a in ms.srcs], "dst": [[float(v) for v in a] for a in ms.dsts]}, fh)
        res = GF.run_node_case("moving_gpu.mjs", path, timeout=600, verdict=False)      # (its record carries `failures`)
    assert res["failures"] == [], res["failures"]
    assert len(res["bilinear"]) == ms.F and len(res["nearest_inverse"]) == ms.F
    for f in range(ms.F):
        near, bil = ms.frame(f, mins=ms.mins[0])[:2]
        for key, want in (("bilinear", bil), ("nearest_inverse", near)):
            got = res[key][f]
            assert (got["w"], got["h"]) == (ms.geoms[f][2], ms.geoms[f][3]), (key, f)
            assert got["min"] == list(ms.mins[0]), (key, f, got["min"])
            assert got["sha"] == M.sha256(want), (key, f)
