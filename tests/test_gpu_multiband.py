"""The multi-band mosaic on the GPU (include/hgwarp.h: hg_mosaic_multiband_device) against the numpy model of tests/hgtest/multiband.py, bit
for bit -- canvas, weight plane and labels, u8 and f32 --, and twice for the same bytes.  tests/test_multiband_cpu.py pins the model itself.
Small shapes throughout; every buffer is filled with 0xA5 before a call and the bytes outside the canvas, the weight plane, the labels and
work_bytes must keep it (hgtest.gpu_multiband.run_multiband checks that on every call)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "homography.js_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hgwarp as HG                          # noqa: E402
from hgtest import gpu_frames as GF          # noqa: E402
from hgtest import gpu_multiband as GM       # noqa: E402
from hgtest import mosaic as MM              # noqa: E402
from hgtest import multiband as MB           # noqa: E402
from hgtest import remap_frames as RF        # noqa: E402
from hgtest.gpu_frames import F32, F32E, FILL, INVALID, U8E      # noqa: E402
import test_gpu_mosaic as TM                 # noqa: E402  (the library's projective and piecewise sets, made once)
import test_multiband_cpu as TC              # noqa: E402  (the property cases, repeated on the device)

pytestmark = pytest.mark.gpu
INF = float("inf")
SW, SH = TM.SW, TM.SH


@pytest.fixture(scope="module")
def ctx():
    c = HG.Context(0)
    yield c
    c.close()


def _dtype(elem):
    return np.uint8 if elem == U8E else F32


def _both(ctx, geoms, fields, frames, elem, ch, feather, bands, canvas, what, gains=None, src=(SW, SH), **kw):
    """Run on the device and compare with the model; returns the device's (canvas bytes, weights, labels)."""
    want = MB.multiband(geoms, fields, frames, src[0], src[1], feather, bands, canvas, gains, like=(_dtype(elem), ch))
    got = GM.run_multiband(ctx, geoms, fields, frames, elem, ch, src[0], src[1], feather, bands, canvas, gains=gains, **kw)
    GM.check(got, want, what)
    return got


def _values(rng, n, elem, ch):
    return rng.integers(1, 160, (n, ch), dtype=np.uint8) if elem == U8E else (rng.standard_normal((n, ch)) * 40 + 3).astype(F32)


# ------------------------------------------------------------------------------------------------ the library's own sets
@pytest.mark.parametrize("channels", (1, 2, 3, 4))
@pytest.mark.parametrize("elem", (F32E, U8E))
@pytest.mark.parametrize("name", ("projective", "piecewise"))
def test_the_librarys_sets_at_1_2_3_and_5_bands(ctx, name, elem, channels):
    geoms, fields, _ = TM._library_sets()[name]
    frames = TM._frames(name, elem, channels)
    canvas = TM.PRO_CANVAS if name == "projective" else TM.PW_CANVAS
    lab = MB.labels(geoms, fields, SW, SH, INF, canvas)[0]
    assert (lab == -1).any() and len(np.unique(lab)) >= 4, np.unique(lab)      # the premises: seams between several owners, and pixels nobody owns
    gains = [0.75 + 0.125 * f for f in range(len(geoms))]
    for bands in (1, 2, 3, 5):
        for feather in (4.0, INF):
            for with_gains in (False, True):
                for with_labels in (False, True):
                    _both(ctx, geoms, fields, frames, elem, channels, feather, bands, canvas, (name, elem, channels, bands, feather, with_gains, with_labels),
                          gains=gains if with_gains else None, labels=with_labels, weight=with_labels or bands != 2)


def test_two_runs_give_the_same_bytes(ctx):
    geoms, fields, _ = TM._library_sets()["projective"]
    for elem, ch in ((U8E, 4), (F32E, 3)):
        frames = TM._frames("projective", elem, ch)
        a = GM.run_multiband(ctx, geoms, fields, frames, elem, ch, SW, SH, INF, 5, TM.PRO_CANVAS)
        b = GM.run_multiband(ctx, geoms, fields, frames, elem, ch, SW, SH, INF, 5, TM.PRO_CANVAS)
        assert all(np.array_equal(GF.u32(x) if x.dtype == F32 else x, GF.u32(y) if y.dtype == F32 else y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ canvas shapes
@pytest.mark.parametrize("canvas,bands", (((-6, 4, 70, 9), 3), ((29, 9, 1, 1), 4), ((-10, -8, 300, 200), 8), ((3, 2, 1, 7), 2), ((400, 400, 5, 3), 3)))
def test_canvas_shapes(ctx, canvas, bands):
    """70 x 9 at 3 bands: no multiple of A; 1 x 1; 300 x 200 at 8 bands: level 7 is a few pixels; a canvas no frame touches."""
    geoms, fields, _ = TM._library_sets()["projective"]
    for elem, ch in ((U8E, 4), (F32E, 2)):
        _both(ctx, geoms, fields, TM._frames("projective", elem, ch), elem, ch, INF, bands, canvas, (canvas, bands, elem, ch))
    if canvas[0] == 400:
        assert not any(g is not None for g in MB.grids(geoms, canvas, bands))


# ------------------------------------------------------------------------------------------------ hand-made sets
HAND_CANVAS = (-4, -3, 40, 21)
# frames hanging over each canvas edge at negative offsets, one wholly outside, an empty one, a 1 x 1 frame, three with identical windows
HAND_GEOMS = [(-12, -9, 20, 14), (30, -8, 16, 12), (-9, 12, 14, 11), (28, 11, 15, 12), (200, 200, 6, 6), (5, 5, 0, 3), (17, 6, 1, 1),
              (8, 2, 16, 9), (8, 2, 16, 9), (8, 2, 16, 9), (2, 1, 30, 15)]


def _hand_set(elem, ch):
    rng = np.random.default_rng(61 + 10 * ch + elem)
    fields, frames = [], []
    for f, g in enumerate(HAND_GEOMS):
        w, h = max(g[2], 0), max(g[3], 0)
        i, j = np.meshgrid(np.arange(w), np.arange(h))
        co = np.stack([(SW - 1.0) * i / max(w - 1, 1) + 0.25 * f, (SH - 1.0) * j / max(h - 1, 1) + 0.125 * f], -1).astype(F32).reshape(-1, 2)
        if f in (6, 7, 8, 9):
            co = np.full((w * h, 2), [SW // 2, SH // 2], F32)           # identical windows AND identical fields: the lowest index owns everything it can
        if f == 10:
            co[:] = np.nan                                              # a field that covers nothing
        if f == 0:
            co[3:6] = [[1e30, 5], [5, -1e30], [-1e30, 1e30]]
        fields.append(co)
        frames.append(_values(rng, w * h, elem, ch))
    return fields, frames


@pytest.mark.parametrize("elem,ch", ((U8E, 4), (U8E, 1), (F32E, 3)))
def test_hand_made_sets(ctx, elem, ch):
    fields, frames = _hand_set(elem, ch)
    for bands in (1, 3, 4):
        got = _both(ctx, HAND_GEOMS, fields, frames, elem, ch, INF, bands, HAND_CANVAS, ("hand-made", elem, ch, bands))
        lab = got[2].reshape(HAND_CANVAS[3], HAND_CANVAS[2])
        assert not np.isin(lab, (4, 5, 8, 9, 10)).any() and (lab == 7).any() and (lab == 6).any() and (lab == -1).any()
    # five frames: the quad table has a partial quad
    _both(ctx, HAND_GEOMS[:5], fields[:5], frames[:5], elem, ch, 2.0, 3, HAND_CANVAS, ("five frames", elem, ch))
    # no frames at all: the canvas is zeroed, labels are -1
    got = _both(ctx, [], [], [], elem, ch, INF, 3, (5, -5, 67, 5), ("no frames", elem, ch))
    assert not got[0].any() and not got[1].view(np.uint8).any() and (got[2] == -1).all()


def test_explicit_offsets_at_odd_but_legal_alignments(ctx):
    for elem, ch in ((U8E, 4), (U8E, 2), (F32E, 1)):
        es = GF.es(elem)
        fields, frames = _hand_set(elem, ch)
        fo = [o + 8 * (2 * f + 1) + 512 * f for f, o in enumerate(RF.pack(HAND_GEOMS, 8)[0])]
        po = [o + 640 * f + es * (2 * f + 1) for f, o in enumerate(RF.pack(HAND_GEOMS, ch * es)[0])]
        assert all(o % 8 == 0 and o % 16 != 0 for o in fo) and all(o % es == 0 and (o // es) % 2 == 1 for o in po)
        _both(ctx, HAND_GEOMS, fields, frames, elem, ch, INF, 3, HAND_CANVAS, ("explicit offsets", elem, ch), foffs=fo, poffs=po, front=256 + 2 * es, cfront=es)


def test_an_empty_canvas_writes_nothing(ctx):
    fields, frames = _hand_set(U8E, 4)
    for canvas in ((0, 0, 0, 9), (0, 0, 9, -1)):
        got = GM.run_multiband(ctx, HAND_GEOMS, fields, frames, U8E, 4, SW, SH, INF, 3, canvas)      # (it checks that every byte kept FILL)
        assert got[0].size == 0


# ------------------------------------------------------------------------------------------------ the properties, on the device
def test_the_property_cases_of_the_cpu_tests_on_the_device(ctx):
    src = (TC.SW, TC.SH)
    run = lambda g, co, fr, b, cv: _both(ctx, g, co, fr, U8E, fr[0].shape[1], INF, b, cv, ("property", b), src=src)
    shaped = lambda g, co, fr, b, cv: (run(g, co, fr, b, cv)[0].reshape(cv[3], cv[2], -1),)
    TC.check_seam_steps(TC.seam_steps(shaped))
    err = TC.ghosting(shaped)
    assert err[TC.GHOST_DISTANCE:].max() <= TC.GHOST_RESIDUAL + 1, err.tolist()
    g, co, cv = TC.split_fields()
    for b in (1, 5):
        assert (run(g, co, [np.full((64 * 16, 3), 77, np.uint8)] * 2, b, cv)[0] == 77).all()
    # n_bands == 1 is HG_MOSAIC_LAST where frames do not overlap
    g = [(0, 0, 6, 4), (6, 0, 5, 4), (0, 4, 11, 2)]
    rng = np.random.default_rng(3)
    fr = [rng.integers(1, 160, (w * h, 3), dtype=np.uint8) for _, _, w, h in g]
    co = [np.full((w * h, 2), 5, F32) for _, _, w, h in g]
    got = run(g, co, fr, 1, (-1, -1, 13, 8))
    assert np.array_equal(got[0], MM.mosaic(g, co, fr, src[0], src[1], MM.LAST, 1.0, (-1, -1, 13, 8))[0].ravel())


# ------------------------------------------------------------------------------------------------ the work area and the refusals
def test_the_work_area_at_exactly_work_bytes_and_one_byte_less(ctx):
    fields, frames = _hand_set(U8E, 4)
    need = HG.mosaic_multiband_layout(HAND_GEOMS, HAND_CANVAS, 4, 4)
    assert need == MB.layout(HAND_GEOMS, HAND_CANVAS, 4, 4)[1]
    _both(ctx, HAND_GEOMS, fields, frames, U8E, 4, INF, 4, HAND_CANVAS, "exact work area", work_bytes=need)
    with pytest.raises(HG.HgError) as e:
        GM.run_multiband(ctx, HAND_GEOMS, fields, frames, U8E, 4, SW, SH, INF, 4, HAND_CANVAS, work_bytes=need - 1)
    assert e.value.code == INVALID


def test_refusals():
    g = [(0, 0, 8, 2), (4, 1, 4, 1)]
    cv = (0, 0, 8, 2)
    need = HG.mosaic_multiband_layout(g, cv, 1, 3)
    with HG.Context(0) as c:
        d = c.alloc(65536)
        d_f, d_p, d_c, d_w, d_l, d_k = d, d + 4096, d + 8192, d + 12288, d + 16384, d + 20480
        co = (np.random.default_rng(2).random((20, 2)) * [7, 3]).astype(F32)
        px = np.arange(1, 21, dtype=np.float32).reshape(20, 1)
        c.to_device(d_f, GF.place([co[:16], co[16:]], [0, 256], 512, 0))
        c.to_device(d_p, GF.place([px[:16], px[16:]], [0, 256], 512, 0))
        want, ww, wl = MB.multiband(g, [co[:16], co[16:]], [px[:16], px[16:]], 8, 4, 2.0, 3, cv)

        def still_works():
            for p in (d_c, d_w, d_l):
                c.to_device(p, np.full(512, FILL, np.uint8))
            c.mosaic_multiband_device(g, d_f, d_p, F32E, 1, 8, 4, 2.0, 3, cv, d_c, d_k, need, d_weight=d_w, d_labels=d_l)
            c.sync()
            raw, wr, lr = c.to_host(d_c, 512), c.to_host(d_w, 512), c.to_host(d_l, 512)
            assert np.array_equal(GF.u32(raw[:64].view(F32)), GF.u32(want.ravel())) and np.array_equal(wr[:64].view(F32), ww.ravel()) and np.array_equal(lr[:64].view(np.int32), wl.ravel())
            assert (raw[64:] == FILL).all() and (wr[64:] == FILL).all() and (lr[64:] == FILL).all()

        def refused(*a, **k):
            assert GF.refusal_code(c.mosaic_multiband_device, *a, **k) == INVALID, (a, k)
            still_works()

        try:
            still_works()
            # (geoms, d_coords, d_frames, elem, channels, w, h, feather, n_bands, canvas, d_canvas, d_work, work_bytes, d_weight, d_labels, field_offsets, frame_offsets, gains)
            refused(g, d_f, d_p, 2, 1, 8, 4, 2.0, 3, cv, d_c, d_k, need)                              # the gain mosaic's list
            for ch in (0, 5):
                refused(g, d_f, d_p, F32E, ch, 8, 4, 2.0, 3, cv, d_c, d_k, 1 << 15)
            refused(g, d_f, d_p, F32E, 1, 0, 4, 2.0, 3, cv, d_c, d_k, need)
            refused(g, d_f, d_p, F32E, 1, 8, 0, 2.0, 3, cv, d_c, d_k, need)
            refused(g, 0, d_p, F32E, 1, 8, 4, 2.0, 3, cv, d_c, d_k, need)
            refused(g, d_f, 0, F32E, 1, 8, 4, 2.0, 3, cv, d_c, d_k, need)
            refused(g, d_f, d_p, F32E, 1, 8, 4, 2.0, 3, cv, 0, d_k, need)
            refused(g, d_f + 4, d_p, F32E, 1, 8, 4, 2.0, 3, cv, d_c, d_k, need)
            refused(g, d_f, d_p + 2, F32E, 1, 8, 4, 2.0, 3, cv, d_c, d_k, need)
            refused(g, d_f, d_p, F32E, 1, 8, 4, 2.0, 3, cv, d_c + 1, d_k, need)
            refused(g, d_f, d_p, F32E, 1, 8, 4, 2.0, 3, cv, d_c, d_k, need, d_w + 2)
            refused(g, d_f, d_p, F32E, 1, 8, 4, 2.0, 3, cv, d_c, d_k, need, d_w, d_l, [0, 260])
            refused(g, d_f, d_p, F32E, 1, 8, 4, 2.0, 3, cv, d_c, d_k, need, d_w, d_l, None, [0, 258])
            refused(g, d_f, d_p, F32E, 1, 8, 4, 2.0, 3, ((1 << 26) + 1, 0, 8, 2), d_c, d_k, 1 << 15)
            for gains in ([1.0, 0.0], [1.0, -1.0], [float("nan"), 1.0], [INF, 1.0]):
                refused(g, d_f, d_p, F32E, 1, 8, 4, 2.0, 3, cv, d_c, d_k, need, gains=gains)
            for bands in (0, 9, -1):                                                                   # n_bands outside 1..8
                refused(g, d_f, d_p, F32E, 1, 8, 4, 2.0, bands, cv, d_c, d_k, 1 << 15)
            for feather in (0.0, -1.0, float("nan"), -INF):                                            # feather NaN or <= 0
                refused(g, d_f, d_p, F32E, 1, 8, 4, feather, 3, cv, d_c, d_k, need)
            refused(g, d_f, d_p, F32E, 1, 8, 4, 2.0, 3, cv, d_c, 0, need)                              # the work area: NULL, misaligned, too small
            refused(g, d_f, d_p, F32E, 1, 8, 4, 2.0, 3, cv, d_c, d_k + 128, need)
            refused(g, d_f, d_p, F32E, 1, 8, 4, 2.0, 3, cv, d_c, d_k, need - 1)
            refused(g, d_f, d_p, F32E, 1, 8, 4, 2.0, 3, cv, d_c, d_k, need, d_w, d_l + 2)              # misaligned labels
            assert GF.refusal_code(c.mosaic_multiband_device, g, d_f, d_p, F32E, 1, 8, 4, 2.0, 0, cv, d_c, d_k, need) == INVALID
            assert b"hg_mosaic_multiband_device" in HG.lib().hg_last_error(c._h)
            c.mosaic_multiband_device(g, d_f, d_p, F32E, 1, 8, 4, 2.0, 3, (0, 0, 0, 2), d_c, 0, 0)     # an empty canvas needs no work area
            still_works()
        finally:
            c.free(d)


def test_js_class_multiband_mosaic_matches_the_ctypes_pipeline():
    """tests/js/multiband_gpu.mjs: h.mosaic(..., { blend: 'multiband' }) of js/Homography.mjs on the real addon for an affine, a projective
    and a piecewise set; it prints its windows and the SHA-256 of every canvas, weight plane and label map, and the same loop through ctypes
    -- stage the set, warp, export the coordinate fields, fit the gains where asked, blend -- must hash alike."""
    import base64
    import hashlib
    res = GF.run_node_case("multiband_gpu.mjs")
    W, H = res["W"], res["H"]
    img = GF.js_pattern_planes(W, H)[0]
    sha = lambda d, n: hashlib.sha256(c.to_host(d, n).tobytes()).hexdigest()
    assert set(res["cases"]) == {"affine", "projective", "piecewise"}
    with HG.Context(0) as c:
        c.set_image(img)
        for name, case in res["cases"].items():
            geoms = [tuple(g) for g in case["geoms"]]
            canvas = tuple(case["canvas"])
            n = canvas[2] * canvas[3]
            assert len(geoms) >= 3 and canvas[2] <= 130 and canvas[3] <= 40, (name, canvas)
            c.set_sampling(case["sampling"])
            if name == "piecewise":
                c.piecewise_set_mesh(np.frombuffer(base64.b64decode(case["src"]), F32), np.frombuffer(base64.b64decode(case["tris"]), np.uint32), *case["minSrc"])
                c.piecewise_set_frames(np.frombuffer(base64.b64decode(case["dst"]), F32), geoms)
            else:
                c.geometric_set_frames_points(0 if name == "affine" else 1, np.frombuffer(base64.b64decode(case["from"]), F32),
                                              np.frombuffer(base64.b64decode(case["to"]), F32), geoms)
            ftotal, ototal = HG.pack_field_offsets(geoms, GF.CO)[1], HG.pack_offsets(geoms)[1]
            F = len(geoms)
            works = {key: HG.mosaic_multiband_layout(geoms, canvas, 4, bands) for key, (bands, _, _) in case["runs"].items()}
            bufs = [c.alloc(t) for t in (ftotal, ototal, n * 4, n * 4, n * 4, max(works.values()), F * F * 16)]
            d_f, d_o, d_c, d_w, d_l, d_k, d_s = bufs
            try:
                if name == "piecewise":
                    c.warp_inverse_piecewise_frames_device(d_o)
                    c.field_inverse_piecewise_frames_device(GF.CO, d_f)
                else:
                    c.warp_inverse_geometric_frames_device(d_o)
                    c.field_inverse_geometric_frames_device(GF.CO, d_f)
                c.sync()
                for key, (bands, feather, fit) in case["runs"].items():
                    gains = None
                    if fit:
                        c.mosaic_overlap_stats_device(geoms, d_f, d_o, 4, canvas, d_s)
                        c.sync()
                        gains = HG.mosaic_solve_gains(c.to_host(d_s, F * F * 16).view(np.uint64), 4)
                        assert base64.b64decode(case["hashes"][key]["gains"]) == gains.tobytes(), (name, key)
                    c.mosaic_multiband_device(geoms, d_f, d_o, U8E, 4, W, H, INF if feather is None else feather, bands, canvas, d_c, d_k, works[key],
                                              d_weight=d_w, d_labels=d_l, gains=gains)
                    c.sync()
                    want = case["hashes"][key]
                    assert c.to_host(d_c, n * 4).any() and sha(d_c, n * 4) == want["data"], (name, key)
                    assert sha(d_w, n * 4) == want["weight"] and sha(d_l, n * 4) == want["labels"], (name, key)
            finally:
                for p_ in bufs:
                    c.free(p_)


def test_state_is_untouched(ctx):
    geoms, fields, _ = TM._library_sets()["projective"]
    before = GF.tap_state(ctx)
    GM.run_multiband(ctx, geoms, fields, TM._frames("projective", U8E, 4), U8E, 4, SW, SH, INF, 3, TM.PRO_CANVAS)
    assert GF.tap_state(ctx) == before
