"""The inverse piecewise kernels on folded and degenerate meshes (tests/hgtest/folds.py): where destination triangles overlap the largest
covering id wins, and a winner that fails the bounds test or has a NaN matrix leaves the pixel 0 whatever lies under it.  Every kernel
resolves that rule in its own way (k_pw_rows: a max over keys through v_readlane or LDS ballot rounds, with a "safe window" shortcut;
k_pw_tile and k_pw_patch: bins; k_pw_fused / k_pw_field: max over ids; the map path: atomicMax), so every run forces its kernel and asserts
which instantiation ran and that no frame was redone through the map.  Every assertion is bit-exact RGBA / map / field against the CPU
oracle or the numpy models; what the meshes contain is asserted in tests/test_folds_cpu.py."""
import numpy as np
import pytest

from hgtest import bilinear as B
from hgtest import edges as E
from hgtest import field as FM
from hgtest import folds as FO
from hgtest import hip
from hgtest import oracle as O
from hgtest.pw_kernels import FRAME_SET_KERNELS, PW_KERNELS, SELF_LABELS

pytestmark = pytest.mark.gpu

HG = hip.load()
NEAR, BIL = HG.SAMPLE_NEAREST, HG.SAMPLE_BILINEAR
IDX, CO = HG.FIELD_INDEX, HG.FIELD_COORDS
W, H = FO.W, FO.H


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(-1))
        first = [(int(r), int(c), got[r, c].tolist(), want[r, c].tolist()) for r, c in bad[:6]]
        raise AssertionError(f"{what}: {len(bad)} of {got.shape[0] * got.shape[1]} pixels differ; (row, col, got, want): {first}")


def _same_bits(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not np.array_equal(g, w):
        diff = g != w
        bad = np.argwhere(diff.any(-1) if diff.ndim == 3 else diff)
        raise AssertionError(f"{what}: {len(bad)} pixels differ; first (row, col, got, want): "
                             f"{[(int(r), int(c), got[r, c].tolist(), want[r, c].tolist()) for r, c in bad[:6]]}")


def _ctx(opts=()):
    c = HG.Context(0)
    for k, v in dict(opts).items():
        c.set_option(k, v)
    return c


def _one_fma(case):
    sp, tris, msx, msy, dp, geom, img = case
    fwd = HG.solve_affine_triangles(sp, dp, tris).reshape(-1, 6)
    return all(HG.affine_one_fma_form(HG.invert_affine(m), geom) for m in fwd)


def _hib(msx, msy, opts):
    return opts.get("hi_bounds", 1) != 0 and msx >= 0 and msy >= 0


def _id(name, twin):
    return f"{name}-two_round" if twin else name


# ------------------------------------------------------------------------------------------------ 1. per instantiation

def _pw_params():
    out = []
    for name, twin in FO.all_cases(deep=False):
        for label in (k for k in PW_KERNELS if k != "rows_dense"):
            if label == "tile_self" and name.startswith("inner_"):
                continue                                            # (k_pw_tile takes windows of 512 columns or more; theirs have 480)
            for hb in ((1, 0) if name != "fold_over_neg" else (1,)):      # (hi_bounds 0 where minSrc >= 0: asserted below)
                out.append(pytest.param(name, twin, label, hb, id=f"{_id(name, twin)}-{label}-hi{hb}"))
    return out


@pytest.mark.parametrize("name,twin,label,hb", _pw_params())
def test_folds_per_instantiation(name, twin, label, hb):
    """One frame of every folded / degenerate mesh through each forced k_pw_rows / k_pw_patch / k_pw_tile instantiation, in both bounds forms;
    the fold_* cases in both coordinate forms.  (The NaN cases always take the two-rounding form: a non-finite entry fails affine_fusable.)"""
    case = FO.case(name, twin)
    sp, tris, msx, msy, dp, geom, img = case
    opts, v_hib, v_fp64 = PW_KERNELS[label]
    opts = dict(opts, hi_bounds=hb)
    assert (min(msx, msy) >= 0) == (name != "fold_over_neg")
    if name in FO.FOLDS:
        assert _one_fma(case) != twin
    want = FO.taps(name, twin)[0]
    c = _ctx(opts)
    try:
        c.set_image(img)
        c.piecewise_set_mesh(sp, tris, msx, msy)
        c.piecewise_prepare(dp, geom)
        got = c.warp_inverse_piecewise()
        variant = c.last_piecewise_variant()
        _same(got, want, (name, twin, label, hb, variant))
        expect = v_hib if _hib(msx, msy, opts) else v_fp64
        assert (variant, c.redone_frames()) == (expect, 0), (name, label, variant, expect, c.redone_frames())
        assert (c.last_piecewise_self() == 1) == (label in SELF_LABELS)
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ 2. deep stacks, by documented capacity
# deepK: K blocks on one another, 4 K spans in every output row, 20 K triangles.  What a workgroup has to hold (hg_kernels.h and the
# kernels' own constants), and what these meshes ask of it (a triangle's rows are [ceil(minY), ceil(maxY)): a row on a cell boundary
# belongs to the lower cell row alone; the last blocks' rightmost triangles spill into the next row, 4 candidate entries more):
#   k_pw_rows           a row's spans: fewer than kRowSpanCapFast = 256 (kRowSpanCapDense = 512 in its 512-slot form).  Rows of more than 64
#                       spans are resolved in LDS ballot rounds of 64: deep20 two, deep40 three, deep70 five.
#   k_pw_rows<SELF>     ... and kCandCap = 256 candidate entries per row group: 4 K + 4.
#   k_pw_tile           kTileRowSpanCap = 96 spans per row and tile, kTileRecs = 128 candidate entries per 8-row tile: 4 K + 4.
#   k_pw_patch<SELF>    kPatchCap = 200 spans per row (199 usable), kPatchRecsSelf = 288 candidate entries per 4-row group: 4 K + 4.
#   k_pw_patch          kPatchCap = 200 spans per row, kPatchRecs = 208 triangles with a span in a 4-row group: 4 K + 1 (asserted below).
# The host sizes the span lists from its own estimate, an upper bound that counts a triangle on the row below its last one too: 8 K here.
# Above 200 (deep40: 320) the lists take 512 slots and k_pw_rows runs in its 512-slot form whatever the options say, which is the list
# form: the row kernels of deep40 are that instantiation (variant digits per include/hgwarp.h: kind 1, 512-slot rows 1, one window per
# phase, 8-byte entries as forced, high-dword bounds 1, self-span form 0).  EXPERIMENTS.md T.1.
# Beyond 256 triangles (deep20 up) k_pw_patch<SELF> and k_pw_tile scan candidate bands instead of the mesh; no digit of the variant says so.
ROWS_LIST = ["rows4", "rows_s80", "rows_compact", "rows1"]
ROWS_SELF = ["rows_self", "rows_self_unsafe", "rows_self_safe"]
INSIDE, OUTSIDE = True, False


def _deep_params():
    out = []

    def add(case, label, limit, inside, variant=None, self_form=None):
        v, s = PW_KERNELS[label][1], label in SELF_LABELS
        out.append(pytest.param(case, label, inside, v if variant is None else variant, s if self_form is None else self_form,
                                id=f"{case}-{label}-{limit}-{'inside' if inside else 'outside'}"))

    for label in ROWS_LIST:
        add("deep12", label, "kRowSpanCapFast", INSIDE)
        add("deep20", label, "kRowSpanCapFast", INSIDE)
        if label in ("rows4", "rows_compact"):                      # (every row label runs the 512-slot list kernel there: one of each entry format)
            add("deep40", label, "kRowSpanCapDense", INSIDE, variant=111110 if label == "rows_compact" else 111010)
    for label in ROWS_SELF:
        add("deep12", label, "kCandCap", INSIDE)                    # 52 entries
        add("deep20", label, "kCandCap", INSIDE)                    # 84 entries
    # (k_pw_tile takes windows of 512 columns or more: the stacks with one cell far to their right, 4 K + 2 spans in rows 0 .. 7)
    add("deep12_wide", "tile_self", "kTileRowSpanCap", INSIDE)      # 50 spans, 54 entries
    add("deep20_wide", "tile_self", "kTileRowSpanCap", INSIDE)      # 82 spans, 86 entries of kTileRecs = 128
    add("deep40_wide", "tile_self", "kTileRowSpanCap", OUTSIDE)     # 162 spans
    add("deep12", "patch_self", "kPatchCap", INSIDE)
    add("deep20", "patch_self", "kPatchCap", INSIDE)                # from candidate bands
    add("deep40", "patch_self", "kPatchCap", INSIDE)                # 160 spans, 164 entries of kPatchRecsSelf = 288
    add("deep70", "patch_self", "kPatchCap", OUTSIDE)               # 280 spans
    add("deep12", "patch_lists", "kPatchRecs", INSIDE)
    add("deep20", "patch_lists", "kPatchRecs", INSIDE)              # 81 triangles
    add("deep40", "patch_lists", "kPatchRecs", INSIDE)              # 161 triangles
    add("deep70", "patch_lists", "kPatchRecs", OUTSIDE)             # 281 triangles, 280 spans
    add("deep70", "rows_dense", "kRowSpanCapDense", INSIDE)         # 280 spans
    return out


def _group_triangles(case, rows):
    """The largest number of triangles with a span in one aligned group of `rows` output rows."""
    sp, tris, msx, msy, dp, geom, img = case
    cov = FO.covers(dp, tris, geom).any(2)
    return max(int(cov[:, r:r + rows].any(1).sum()) for r in range(0, geom[3], rows))


@pytest.mark.parametrize("name,label,inside,variant,self_form", _deep_params())
def test_deep_stacks_by_capacity(name, label, inside, variant, self_form):
    """Inside a kernel's capacity: the bytes, the instantiation and no redone frame.  Outside it: the bytes, and the frame was flagged and
    redone through the map."""
    case = FO.case(name)
    sp, tris, msx, msy, dp, geom, img = case
    K = FO.DEEP[name] if name in FO.DEEP else FO.DEEP_WIDE[name]
    if label == "patch_lists":
        assert _group_triangles(case, 4) == 4 * K + 1 and (4 * K + 1 <= 208) == inside
    want = FO.taps(name)[0]
    c = _ctx(PW_KERNELS[label][0])
    try:
        c.set_image(img)
        c.piecewise_set_mesh(sp, tris, msx, msy)
        c.piecewise_prepare(dp, geom)
        got = c.warp_inverse_piecewise()
        v, redone, self_ran = c.last_piecewise_variant(), c.redone_frames(), c.last_piecewise_self() == 1
        print(name, label, "depth", K, "variant", v, "self", self_ran, "redone", redone, "kernel", c.last_piecewise_kernel())
        _same(got, want, (name, label, v, redone))
        if inside:
            assert (v, redone, self_ran) == (variant, 0, self_form), (name, label, v, redone, self_ran)
        else:
            assert redone == 1, (name, label, v, redone)
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ 3. maps, general kernel, bilinear, fields

@pytest.mark.parametrize("name,twin", FO.all_cases(), ids=[_id(n, t) for n, t in FO.all_cases()])
def test_folds_maps_general_bilinear_and_fields(name, twin):
    """The parity taps (both triangle maps), k_pw_from_map (via-map and reference-state forms) and k_pw_fused (bilinear mode; a mesh padded
    past 32767 triangles) in nearest and bilinear mode, and k_pw_field in both formats against the numpy model, gather == warp."""
    case = FO.case(name, twin)
    sp, tris, msx, msy, dp, geom, img = case
    want, wmap, fwd, inv, sx, sy, valid = FO.taps(name, twin)
    bil, cov = B.warp_piecewise(wmap, inv, img, msx, msy, *geom)
    assert cov.any()
    fields = {IDX: FM.index_field(sx, sy, valid, W, H, msx, msy), CO: FM.coords_field(sx, sy, valid, W, H, msx, msy)}
    assert np.array_equal(FM.remap_index(fields[IDX], img.reshape(-1, 4)).reshape(want.shape), want)
    c = _ctx()
    try:
        c.set_image(img)
        c.piecewise_set_mesh(sp, tris, msx, msy)
        for mode, w in ((NEAR, want), (BIL, bil)):
            c.set_sampling(mode)
            c.piecewise_prepare(dp, geom)
            _same(c.warp_inverse_piecewise(), w, ("warp", mode))
            if mode == BIL: assert c.last_piecewise_variant() == 600000, c.last_piecewise_variant()
            assert np.array_equal(c.get_tri_map(fused=True), wmap) and np.array_equal(c.get_tri_map(), wmap)
            _same(c.warp_inverse_piecewise_via_map(), w, ("via map", mode))
            _same(c.warp_inverse_piecewise_state(fwd, dp, tris, msx, msy, geom), w, ("state form", mode))
        c.set_sampling(NEAR)
        c.piecewise_prepare(dp, geom)
        got = {fmt: c.field_inverse_piecewise(fmt) for fmt in (IDX, CO)}
        for fmt in (IDX, CO):
            _same_bits(got[fmt], fields[fmt], (name, twin, "field", fmt))
        _same(FM.remap_index(got[IDX], img.reshape(-1, 4)).reshape(want.shape), c.warp_inverse_piecewise(), "gather == warp")
        sp2, tris2, dp2 = E.pad_triangles(sp, tris, dp, geom)
        c.piecewise_set_mesh(sp2, tris2, msx, msy)
        c.piecewise_prepare(dp2, geom)
        _same(c.warp_inverse_piecewise(), want, "padded mesh")
        assert c.last_piecewise_variant() == 600000 and c.redone_frames() == 0, (c.last_piecewise_variant(), c.redone_frames())
        assert np.array_equal(c.get_tri_map(fused=True), wmap)
        for fmt in (IDX, CO):
            _same_bits(c.field_inverse_piecewise(fmt), fields[fmt], (name, twin, "field of the padded mesh", fmt))
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ 4. frame sets

def _run_set(c, F, imgs, distinct, stage, geoms, wants, what, variant=None):
    """Stages the set with `stage(offsets)`, warps it into one packed buffer and compares frame by frame."""
    offs, total = HG.pack_offsets(geoms)
    stride = W * H * 4
    d_src, d_out = c.alloc(stride * (F if distinct else 1)), c.alloc(total)
    try:
        for k in range(F if distinct else 1): c.to_device(d_src, imgs[k], k * stride)
        if distinct: c.set_images_device(d_src, W, H, F, stride)
        else: c.set_image_device(d_src, W, H)
        stage(offs)
        c.warp_inverse_piecewise_frames_device(d_out)
        c.sync()
        v = c.last_piecewise_variant()
        for f in range(F):
            g = geoms[f]
            _same(c.to_host(d_out, g[2] * g[3] * 4, offs[f]).reshape(g[3], g[2], 4), wants[f], (what, f, v))
        assert c.redone_frames() == 0, (v, c.redone_frames())
        if variant is not None:
            assert v == variant, (what, v)
    finally:
        c.free(d_out); c.free(d_src)


@pytest.mark.parametrize("distinct", [False, True], ids=["shared", "distinct"])
@pytest.mark.parametrize("label", FRAME_SET_KERNELS)
def test_fold_frame_sets(label, distinct):
    """Eight frames of [A, BLK] whose overlap region moves with the frame (one frame without overlap, one whose BLK has no spans and
    non-finite matrices, every other frame the two-rounding twin), on a shared source in sub-bands and with one source per frame."""
    sp, tris, msx, msy, frames, geoms = FO.moving_fold()
    F = FO.F
    imgs = [O.lcg_image(W, H, 40 + f) for f in range(F)] if distinct else [O.lcg_image(W, H, 11)] * F
    wants = [O.warp_inverse_piecewise(sp, frames[f], tris, imgs[f], msx, msy, *geoms[f]) for f in range(F)]
    assert sum(not np.array_equal(wants[f][:40, :512], wants[0][:40, :512]) for f in range(1, F)) == F - 1
    opts = {} if label == "default" else dict(PW_KERNELS[label][0])
    if not distinct: opts["sub_bands"] = 2
    c = _ctx(opts)
    try:
        c.piecewise_set_mesh(sp, tris, msx, msy)
        _run_set(c, F, imgs, distinct, lambda offs: c.piecewise_set_frames(np.concatenate(frames), list(geoms), offs), list(geoms), wants,
                 (label, distinct), None if label == "default" else PW_KERNELS[label][1])
    finally:
        c.close()


@pytest.mark.parametrize("label", FRAME_SET_KERNELS)
def test_a_source_degenerate_triangle_in_some_frames_of_a_set(label):
    """hg_piecewise_set_frames_src: the last triangle's source is coincident in frames 1 and 5 only, so NaN matrices exist in some frames
    of the set; frames 3 and 7 are two-rounding twins with finite matrices and frames 0, 2, 4, 6 take the one-fma form (asserted on the
    host), so the two-rounding flag differs from frame to frame."""
    tris, srcs, dsts, geoms, mins = FO.moving_nan()
    F = FO.F
    img = O.lcg_image(W, H, 11)
    wants, holes = [], []
    for f in range(F):
        out, wmap, fwd, inv = O.warp_inverse_piecewise(srcs[f], dsts[f], tris, img, *mins[f], *geoms[f], taps=True)
        assert np.isnan(inv[-1]).all() == (f in FO.NAN_FRAMES)
        assert _one_fma((srcs[f], tris, 0, 0, dsts[f], geoms[f], img)) == (f not in FO.NAN_FRAMES + FO.TWIN_FRAMES), f
        wants.append(out)
        holes.append(int((~out[wmap.reshape(out.shape[:2]) == tris.size // 3 - 1].any(-1)).sum()))
    assert all((holes[f] >= 3000) == (f in FO.NAN_FRAMES) for f in range(F)), holes
    opts = {} if label == "default" else dict(PW_KERNELS[label][0])
    c = _ctx(opts)
    try:
        c.piecewise_set_mesh(srcs[0], tris, *mins[0])
        _run_set(c, F, [img] * F, False, lambda offs: c.piecewise_set_frames_src(np.concatenate(srcs), None, np.concatenate(dsts), list(geoms), offs),
                 list(geoms), wants, ("own source", label), None if label == "default" else PW_KERNELS[label][1])
    finally:
        c.close()
