"""The inverse warp kernels at the edges of their proofs (tests/hgtest/edges.py): exact Math.round ties, the bounds limits, signed and
past-the-end flat indices, and the admission limits that pick a fast kernel over the general one.  Every run forces its kernel through
options and asserts which instantiation ran (hg_last_piecewise_variant / hg_last_geometric_kernel) and that no frame was redone through
the map; the bar is bit-exact RGBA against the oracle (nearest) or the numpy model (bilinear)."""
import numpy as np
import pytest

from hgtest import bilinear as B
from hgtest import edges as E
from hgtest import hip
from hgtest import oracle as O
from hgtest import workloads as WL
from hgtest.pw_kernels import FRAME_SET_KERNELS, PW_KERNELS, SELF_LABELS

pytestmark = pytest.mark.gpu

HG = hip.load()
NEAR, BIL = HG.SAMPLE_NEAREST, HG.SAMPLE_BILINEAR


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(-1))
        first = [(int(r), int(c), got[r, c].tolist(), want[r, c].tolist()) for r, c in bad[:6]]
        raise AssertionError(f"{what}: {len(bad)} of {got.shape[0] * got.shape[1]} pixels differ; (row, col, got, want): {first}")


def _ctx(opts=()):
    c = HG.Context(0)
    for k, v in dict(opts).items():
        c.set_option(k, v)
    return c


def _one_fma(case):
    sp, tris, msx, msy, dp, geom, img = case
    fwd = HG.solve_affine_triangles(sp, dp, tris).reshape(-1, 6)
    return all(HG.affine_one_fma_form(HG.invert_affine(m), geom) for m in fwd)


def _hib(msx, msy, W, H, opts):
    return opts.get("hi_bounds", 1) != 0 and msx >= 0 and msy >= 0 and W + msx < (1 << 20) and H + msy < (1 << 20)


def _pw_params():
    out = []
    for name in E.PIECEWISE:
        for label in (["rows_dense"] if name == "dense" else [k for k in PW_KERNELS if k != "rows_dense"]):
            for hb in ((1, 0) if name in ("pos", "exact", "dense") else (1,)):
                for twin in (False, True):
                    out.append(pytest.param(name, label, hb, twin, id=f"{name}-{label}-hi{hb}-{'two_round' if twin else 'one_fma'}"))
    return out


@pytest.mark.parametrize("name,label,hb,twin", _pw_params())
def test_piecewise_edges_per_instantiation(name, label, hb, twin):
    """One frame of each edge mesh through each forced k_pw_rows / k_pw_patch / k_pw_tile instantiation, in both bounds forms and both
    coordinate forms (a twin with one vertex moved by two f32 ulps takes the two-rounding form)."""
    case = E.piecewise(name, twin)
    sp, tris, msx, msy, dp, geom, img = case
    opts, v_hib, v_fp64 = PW_KERNELS[label]
    opts = dict(opts, hi_bounds=hb)
    assert _one_fma(case) != twin
    want = O.warp_inverse_piecewise(sp, dp, tris, img, msx, msy, *geom)
    c = _ctx(opts)
    try:
        c.set_image(img)
        c.piecewise_set_mesh(sp, tris, msx, msy)
        c.piecewise_prepare(dp, geom)
        got = c.warp_inverse_piecewise()
        variant = c.last_piecewise_variant()
        _same(got, want, (name, label, hb, twin, variant))
        expect = v_hib if _hib(msx, msy, img.shape[1], img.shape[0], opts) else v_fp64
        assert (variant, c.redone_frames()) == (expect, 0), (name, label, variant, expect, c.redone_frames())
        assert (c.last_piecewise_self() == 1) == (label in SELF_LABELS)
    finally:
        c.close()


@pytest.mark.parametrize("twin", [False, True], ids=["one_fma", "two_round"])
@pytest.mark.parametrize("name", list(E.PIECEWISE))
def test_piecewise_edges_maps_general_and_bilinear(name, twin):
    """The same meshes through the parity taps (triangle maps), k_pw_fused (a mesh padded past 32767 triangles), k_pw_from_map (via-map
    and reference-state forms), in nearest and bilinear mode."""
    case = E.piecewise(name, twin)
    sp, tris, msx, msy, dp, geom, img = case
    want, wmap, fwd, inv = O.warp_inverse_piecewise(sp, dp, tris, img, msx, msy, *geom, taps=True)
    bil, cov = B.warp_piecewise(wmap, inv, img, msx, msy, *geom)
    assert cov.any()
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
        sp2, tris2, dp2 = E.pad_triangles(sp, tris, dp, geom)
        c.piecewise_set_mesh(sp2, tris2, msx, msy)
        c.piecewise_prepare(dp2, geom)
        _same(c.warp_inverse_piecewise(), want, "padded mesh")
        assert c.last_piecewise_variant() == 600000 and c.redone_frames() == 0, (c.last_piecewise_variant(), c.redone_frames())
        assert np.array_equal(c.get_tri_map(fused=True), wmap)
    finally:
        c.close()


@pytest.mark.parametrize("distinct", [False, True], ids=["shared", "distinct"])
@pytest.mark.parametrize("label", FRAME_SET_KERNELS)
@pytest.mark.parametrize("name", ["pos", "neg"])
def test_piecewise_edge_frame_sets(name, label, distinct):
    """Eight frames (every other one the two-rounding twin, each translated by a different number of pixels) on a shared source, in
    sub-bands, and with one source per frame."""
    F = 8
    base, twin = E.piecewise(name), E.piecewise(name, True)
    sp, tris, msx, msy = base[:4]
    H, W = base[6].shape[:2]
    frames = [((twin if f % 2 else base)[4].reshape(-1, 2) + np.float32([f, f // 2])).astype(np.float32).ravel() for f in range(F)]
    geoms = [WL.piecewise_geom(d) for d in frames]
    imgs = [O.lcg_image(W, H, 40 + f) for f in range(F)] if distinct else [base[6]] * F
    opts = {} if label == "default" else dict(PW_KERNELS[label][0])
    if not distinct: opts["sub_bands"] = 2
    offs, total = HG.pack_offsets(geoms)
    stride = W * H * 4
    c = _ctx(opts)
    d_src, d_out = c.alloc(stride * (F if distinct else 1)), c.alloc(total)
    try:
        for k in range(F if distinct else 1): c.to_device(d_src, imgs[k], k * stride)
        if distinct: c.set_images_device(d_src, W, H, F, stride)
        else: c.set_image_device(d_src, W, H)
        c.piecewise_set_mesh(sp, tris, msx, msy)
        c.piecewise_set_frames(np.concatenate(frames), geoms, offs)
        c.warp_inverse_piecewise_frames_device(d_out)
        c.sync()
        v = c.last_piecewise_variant()
        for f in range(F):
            g = geoms[f]
            want = O.warp_inverse_piecewise(sp, frames[f], tris, imgs[f], msx, msy, *g)
            _same(c.to_host(d_out, g[2] * g[3] * 4, offs[f]).reshape(g[3], g[2], 4), want, (name, label, distinct, f, v))
        assert c.redone_frames() == 0, (v, c.redone_frames())
        if label != "default":
            _, v_hib, v_fp64 = PW_KERNELS[label]
            assert v == (v_hib if _hib(msx, msy, W, H, opts) else v_fp64), (label, v)
    finally:
        c.free(d_out); c.free(d_src); c.close()


# ------------------------------------------------------------------------------------------------ geometric

@pytest.mark.parametrize("nw", [8, 4, 2, 1])
@pytest.mark.parametrize("name", list(E.GEOMETRIC))
def test_geometric_edges(name, nw):
    """k_geo_fast<KIND, NW, 0> for every NW, and k_geo_fast<KIND, 8, 1> in bilinear mode, on the edge matrices."""
    kind, m, img, geom = E.GEOMETRIC[name]()
    K = E.GEOMETRIC_KIND[name]
    c = _ctx({"geo_windows": nw})
    try:
        c.set_image(img)
        _same(c.warp_inverse_geometric(kind, m, geom), O.warp_inverse_geometric(kind, m, img, *geom), (name, nw))
        assert c.last_geometric_kernel() == 100 * K + 10 * nw, c.last_geometric_kernel()
        if nw == 8:
            c.set_sampling(BIL)
            _same(c.warp_inverse_geometric(kind, m, geom), B.warp_geometric(kind, m, img, *geom)[0], (name, "bilinear"))
            assert c.last_geometric_kernel() == 100 * K + 81, c.last_geometric_kernel()
    finally:
        c.close()


def test_geometric_edges_device_solves():
    """KIND 4: projective frames solved on the device from point sets (source = half the destination less a shift: exact ties), against
    the oracle run on the matrices the device solved; those equal the host solve."""
    W, H, F = 256, 24, 8
    img = O.lcg_image(W, H, 31)
    src = np.float32([0, 0, 0, H, W, 0, W, H])
    froms, tos, geoms = [], [], []
    for f in range(F):
        froms.append((2 * src.reshape(-1, 2) + np.float32([f - 3, 1 - f])).astype(np.float32).ravel())
        tos.append(src)
        geoms.append((f - 6, -2 - f, 2 * W + 8, 2 * H + 8))
    offs, total = HG.pack_offsets(geoms)
    c = _ctx()
    d_out = c.alloc(total)
    try:
        c.set_image(img)
        c.geometric_set_frames_points(1, np.concatenate(froms), np.concatenate(tos), geoms, offs)
        c.warp_inverse_geometric_frames_device(d_out)
        c.sync()
        assert c.last_geometric_kernel() == 480, c.last_geometric_kernel()
        mats = c.get_geometric_matrices(F)
        for f in range(F):
            assert np.array_equal(mats[f], HG.solve_projective(froms[f], tos[f])), f
            g = geoms[f]
            sx, sy = B.geometric_coords(1, mats[f], *g)
            assert E.classify(sx, sy, np.ones(sx.shape, bool), W, H)["E1 tie x>=0"] >= 32, f
            _same(c.to_host(d_out, g[2] * g[3] * 4, offs[f]).reshape(g[3], g[2], 4), O.warp_inverse_geometric(1, mats[f], img, *g), f)
    finally:
        c.free(d_out); c.close()


# ------------------------------------------------------------------------------------------------ admission limits

LW, LH = 32768, 16381                       # (LH + 2) * LW * 4 = 2^31 - 131072: the largest source both fast paths admit


@pytest.fixture(scope="module")
def largest():
    """One device buffer of LW x (LH + 1) pixels (the only near-2 GiB source of this module), bound as LH and as LH + 1 rows."""
    img = O.lcg_image(LW, LH + 1, 9)
    c = HG.Context(0)
    d = c.alloc(img.nbytes)
    c.to_device(d, img)
    yield c, d, img
    c.free(d)
    c.close()


@pytest.mark.parametrize("H", [LH, LH + 1])
def test_largest_source_geometric(largest, H):
    """The last rows and the last pixel: s_x = W - 0.5 on the last row is index W * H, real memory past the binding that the
    descriptor's range check must read as 0; and the origin, with negative coordinates."""
    c, d, img = largest
    assert ((H + 2) * LW * 4 < (1 << 31)) == (H == LH)
    c.set_image_device(d, LW, H)
    view = img[:H]
    for m, g in (([0.5, 0, 0, 0.5, LW - 20, H - 4], (0, 0, 44, 12)), ([0.5, 0, 0, 0.5, -1.5, -1.5], (0, 0, 12, 12))):
        m = np.float64(m)
        _same(c.warp_inverse_geometric(0, m, g), O.warp_inverse_geometric(0, m, view, *g), (H, g))
        assert c.last_geometric_kernel() == (80 if H == LH else 1000), c.last_geometric_kernel()
    sx, sy = B.geometric_coords(0, np.float64([0.5, 0, 0, 0.5, LW - 20, H - 4]), 0, 0, 44, 12)
    assert E.classify(sx, sy, np.ones(sx.shape, bool), LW, H)["E3 high in, past the end"] >= 1


@pytest.mark.parametrize("msx", [0, -1])
@pytest.mark.parametrize("H", [LH, LH + 1])
def test_largest_source_piecewise(largest, H, msx):
    """A tie grid on the last rows and columns next to a small block at the origin (minSrcX 0 or -1, minSrcY 0: pw_fast_ok counts
    |minSrc|): k_pw_rows at LH rows, k_pw_fused at LH + 1."""
    c, d, img = largest
    view = img[:H]
    blocks = [(LW - 20.5, H - 4.5, 6, 2, 4, 4, (2, 2)), (msx - 0.5 if msx else 0.0, 0.0, 1, 1, 4, 4, (56, 2))]
    sp, tris, cmx, cmy, dp, geom, _ = E.piecewise_case(LW, H, blocks, image=view)
    assert (cmx, cmy) == (msx, 0)
    want, wmap, fwd, inv = O.warp_inverse_piecewise(sp, dp, tris, view, cmx, cmy, *geom, taps=True)
    sx, sy, valid = B.piecewise_coords(wmap, inv, *geom)
    cl = E.classify(sx, sy, valid, LW, H, cmx, cmy)
    e3 = cl["E3 high in, next row"] + cl["E3 high in, same row"]
    assert e3 >= 4 and (cl["E3 high in, past the end"] >= 1 if msx == 0 else cl["E1 tie x<0"] >= 1), cl
    for label in ("rows_self", "rows1"):
        c = _ctx(PW_KERNELS[label][0])                # (its own context, bound to the module's buffer)
        try:
            c.set_image_device(d, LW, H)
            c.piecewise_set_mesh(sp, tris, cmx, cmy)
            c.piecewise_prepare(dp, geom)
            _same(c.warp_inverse_piecewise(), want, (H, msx, label))
            if H == LH:
                expect = PW_KERNELS[label][1] if msx == 0 else PW_KERNELS[label][2]
                assert c.last_piecewise_kernel() != 4 and c.last_piecewise_variant() == expect, (label, c.last_piecewise_variant())
            else:
                assert c.last_piecewise_kernel() == 4 and c.last_piecewise_variant() == 600000, (label, c.last_piecewise_variant())
            c.sync()
            assert c.redone_frames() == 0
            _same(c.warp_inverse_piecewise_via_map(), want, (H, msx, "via map"))
        finally:
            c.close()


@pytest.mark.parametrize("W,msx", [((1 << 20) - 1, 0), (1 << 20, 0), ((1 << 20) - 1, -1), (1 << 20, -1)])
def test_hi_dword_bounds_limit(W, msx):
    """W + minSrcX just below 2^20 takes the high-dword bounds; 2^20, or minSrcX < 0, the fp64 compares.  E3 pixels of rows 0 and 1 read
    the next row (minSrcX = 0) or the last pixel of their own row (minSrcX = -1).  Geometric: W = 2^20 - 1 runs k_geo_fast, 2^20 k_geo."""
    H = 3
    img = O.lcg_image(W, H, 17)
    blocks = [(W + msx - 8.5, -0.5, 3, 1, 3, 4, (2, 2)), (msx - 0.5 if msx else 0.0, 0.0, 1, 1, 2, 2, (30, 2))]
    sp, tris, cmx, cmy, dp, geom, _ = E.piecewise_case(W, H, blocks, image=img)
    assert (cmx, cmy) == (msx, 0)
    want, wmap, fwd, inv = O.warp_inverse_piecewise(sp, dp, tris, img, cmx, cmy, *geom, taps=True)
    sx, sy, valid = B.piecewise_coords(wmap, inv, *geom)
    cl = E.classify(sx, sy, valid, W, H, cmx, cmy)
    assert cl["E3 high in, next row" if msx >= 0 else "E3 high in, same row"] >= 3, cl
    hib = msx == 0 and W + msx < (1 << 20)
    for label in ("rows_self", "rows1", "patch_self"):
        c = _ctx(PW_KERNELS[label][0])
        try:
            c.set_image(img)
            c.piecewise_set_mesh(sp, tris, cmx, cmy)
            c.piecewise_prepare(dp, geom)
            _same(c.warp_inverse_piecewise(), want, (W, msx, label))
            v = c.last_piecewise_variant()
            assert (v // 10 % 10 == 1) == hib and c.redone_frames() == 0, (W, msx, label, v)
        finally:
            c.close()
    c = _ctx()
    try:
        c.set_image(img)
        m, g = np.float64([0.5, 0, 0, 0.5, W - 10, -1.5]), (0, 0, 24, 8)
        _same(c.warp_inverse_geometric(0, m, g), O.warp_inverse_geometric(0, m, img, *g), ("geometric", W))
        assert c.last_geometric_kernel() == (80 if W < (1 << 20) else 1000), c.last_geometric_kernel()
    finally:
        c.close()


M22 = (1 << 22) - 1


def _tall_case(img, x0, y0, y1):
    """Two tie blocks of a W = 2 source: rows from y0 (minSrcY) and rows from y1."""
    return E.piecewise_case(img.shape[1], img.shape[0], [(x0, y0, 1, 2, 4, 2, (2, 2)), (x0, y1, 1, 2, 4, 2, (14, 2))], image=img)


@pytest.fixture(scope="module")
def tall():
    return O.lcg_image(2, M22, 5)


@pytest.mark.parametrize("which", ["mul24+", "mul24-", "opposite"])
def test_mul24_operand_range(tall, which):
    """W = 2, H = 2^22 - 1 at the extremes of pw_fast_ok: round(sy) reaches 2^23 - 2 ("mul24+") and -(2^22 - 1) ("mul24-"), both inside
    __mul24's signed 24-bit operand range, so no correct kernel wraps there; with W = 2 every index of those rows lies past the end or
    below 0, and what these two cases pin is the zero fill of such indices and the fast kernel's admission.  Large opposite-sign minima
    (minSrcX ~ 2^22, minSrcY = -2^21) bring flat indices back inside the source: there a wrong row product reads wrong nonzero bytes."""
    img = tall
    if which == "mul24+":
        case = _tall_case(img, -0.5, M22 - 0.5, M22 + M22 - 3.5)
    elif which == "mul24-":
        case = _tall_case(img, -0.5, -M22 - 0.5, -3.5)
    else:
        case = _tall_case(img, (1 << 22) - 2.5, -(1 << 21) - 0.5, -(1 << 21) + 7.5)
    sp, tris, msx, msy, dp, geom, _ = case
    want, wmap, _, inv = O.warp_inverse_piecewise(sp, dp, tris, img, msx, msy, *geom, taps=True)
    sx, sy, valid = B.piecewise_coords(wmap, inv, *geom)
    inb = valid & (sx >= msx) & (sx < 2 + msx) & (sy >= msy) & (sy < M22 + msy)
    ry, rx = E.js_round(sy[inb]).astype(np.int64), E.js_round(sx[inb]).astype(np.int64)
    idx = ry * 2 + rx
    if which == "mul24+":
        assert int(ry.max()) == (1 << 23) - 2 and (idx >= 2 * M22).all() and not want.any()
    elif which == "mul24-":
        assert int(ry.min()) == -M22 and (idx < 0).sum() >= 16 and want.any()      # (the rows near 0 read row 0)
    else:
        assert ((idx >= 0) & (idx < 2 * M22)).sum() >= 16 and want.any()
    for label in ("rows_self", "rows1"):
        c = _ctx(PW_KERNELS[label][0])
        try:
            c.set_image(img)
            c.piecewise_set_mesh(sp, tris, msx, msy)
            c.piecewise_prepare(dp, geom)
            _same(c.warp_inverse_piecewise(), want, (which, label))
            assert c.last_piecewise_kernel() != 4 and c.redone_frames() == 0, (which, label, c.last_piecewise_variant())
        finally:
            c.close()


# step -> (source W, H, tie blocks, k_pw_fused expected): each pw_fast_ok limit one step past it, and W and |minSrcX| just inside
_LIMITS = {
    "H = 2^22": (2, M22 + 1, [(-0.5, 0.0, 1, 2, 4, 2, (2, 2)), (-0.5, M22 - 2.5, 1, 2, 4, 2, (14, 2))], True),
    "minSrcY = -2^22": (2, 64, [((1 << 22) - 2.5, -(1 << 22) - 0.5, 1, 2, 4, 2, (2, 2)), ((1 << 22) - 2.5, -(1 << 22) + 8.5, 1, 2, 4, 2, (14, 2))], True),
    "minSrcX = 2^22": (2, 64, [((1 << 22) - 0.5, -0.5, 1, 2, 4, 2, (2, 2))], True),
    "minSrcX = 2^22 - 1": (2, 64, [((1 << 22) - 1.5, -0.5, 1, 2, 4, 2, (2, 2))], False),
    "W = 2^21": (1 << 21, 2, [((1 << 21) - 8.5, -0.5, 3, 1, 3, 3, (2, 2)), (0.0, 0.0, 1, 1, 2, 2, (30, 2))], True),
    "W = 2^21 - 1": ((1 << 21) - 1, 2, [((1 << 21) - 9.5, -0.5, 3, 1, 3, 3, (2, 2)), (0.0, 0.0, 1, 1, 2, 2, (30, 2))], False),
}


@pytest.mark.parametrize("step", list(_LIMITS))
def test_pw_fast_ok_limits(step):
    """One step past H < 2^22, |minSrcY| < 2^22, |minSrcX| < 2^22 and W < 2^21: k_pw_fused; |minSrcX| and W just inside: a fast kernel."""
    W, H, blocks, fused = _LIMITS[step]
    img = O.lcg_image(W, H, 6)
    sp, tris, msx, msy, dp, geom, _ = E.piecewise_case(W, H, blocks, image=img)
    want = O.warp_inverse_piecewise(sp, dp, tris, img, msx, msy, *geom)
    c = _ctx(PW_KERNELS["rows_self"][0])
    try:
        c.set_image(img)
        c.piecewise_set_mesh(sp, tris, msx, msy)
        c.piecewise_prepare(dp, geom)
        _same(c.warp_inverse_piecewise(), want, step)
        v = c.last_piecewise_variant()
        assert (v == 600000) == fused and (c.last_piecewise_kernel() == 4) == fused and c.redone_frames() == 0, (step, msx, msy, v)
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ the generic k_geo

GW = 1 << 20                                # a source 2^20 wide: k_geo<kind, S>


@pytest.fixture(scope="module")
def wide():
    return O.lcg_image(GW, 32, 27)


@pytest.mark.parametrize("name", list(E.GEOMETRIC))
def test_generic_geometric_edges(wide, name):
    """The edge matrices through k_geo<kind, S> in both sampling modes, on a source 2^20 wide: the builder's window at the origin
    (ties, Q1, the low limits) and the same window moved to the right edge (the high limit, s_x = W - 0.5 reading the next row)."""
    kind, m, small, geom = E.GEOMETRIC[name]()
    img = wide[:small.shape[0]]
    shift = int((GW - small.shape[1]) / m[0])                  # (m[0] is 1 or 0.5, the denominators are 1)
    wins = [geom, (geom[0] + shift, geom[1], geom[2], geom[3])]
    c = _ctx()
    try:
        c.set_image(img)
        for g in wins:
            sx, sy = B.geometric_coords(kind, m, *g)
            for mode in (NEAR, BIL):
                c.set_sampling(mode)
                want = O.warp_inverse_geometric(kind, m, img, *g) if mode == NEAR else B.warp_geometric(kind, m, img, *g)[0]
                _same(c.warp_inverse_geometric(kind, m, g), want, (name, g, mode))
                assert c.last_geometric_kernel() == 1000 + 10 * kind + mode, c.last_geometric_kernel()
        cl = E.classify(sx, sy, np.ones(sx.shape, bool), GW, img.shape[0])
        if name != "affine_below":                              # (its offsets vanish next to 2^20: s lands on integers there)
            assert cl["E3 high in, next row"] >= 16 and cl["E3 high in, past the end"] >= 1, cl
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ forward tile kernels

def _fwd_pw_oracle(sp, dp, tris, img, geom):
    ms = O.minmax_xy(sp)
    mw, mh = int(ms[2] - ms[0]), int(ms[3] - ms[1])
    fwd = O.piecewise_matrices(sp, dp, tris)
    fmap = O.build_tri_map(sp, tris, mw, int(ms[1]), mw * mh)
    return O.warp_forward_piecewise(fmap, fwd, img, int(ms[0]), int(ms[1]), int(ms[2]), int(ms[3]), *geom)


# the forward loops round destination coordinates: half-pixel translations (every coordinate a tie, also below 0), a 1.5 scale
# (ties on every even source pixel), Q1 in a projective offset
FORWARD = {
    "affine_half_shift": (0, [1, 0, 0, 1, 0.5, -0.5]),
    "affine_neg_shift": (0, [1, 0, 0, 1, -20.5, -10.5]),
    "affine_scale": (0, [1.5, 0, 0, 1.5, 0.5, 2.5]),
    "proj_q1": (1, [1, 0, E.Q1, 0, 1, -E.Q1, 0, 0]),
}


@pytest.mark.parametrize("name", list(FORWARD))
def test_forward_tiles_at_ties(name):
    """k_fwd_tiles (fwd_tiles 1) against scatter + gather (fwd_tiles 0) and the oracle, on its window and on the window moved so that
    destination x lands just outside it (the flat index aliases into the neighbouring row)."""
    kind, m = FORWARD[name]
    m = np.float64(m)
    W, H = 300, 80
    img = O.lcg_image(W, H, 51)
    x = np.arange(W, dtype=np.float64)
    dx = (m[0] * x + m[2]) if kind == 1 else (m[0] * x + m[4])
    assert ((dx - np.floor(dx)) == 0.5).sum() >= 100
    lim = [int(v) for v in O.transform_limits(kind, m, W, H)]
    c = _ctx()
    try:
        c.set_image(img)
        for geom in (tuple(lim), (lim[0] + 9, lim[1] - 3, lim[2] - 20, lim[3] + 5)):
            assert HG.forward_tiles_admissible(kind, m, W, H, geom) >= 1, geom
            want = O.warp_forward_geometric(kind, m, img, *geom)
            assert want.any()
            for opt, code in ((0, 1), (1, 2)):
                c.set_option("fwd_tiles", opt)
                _same(c.warp_forward_geometric(kind, m, geom), want, (name, geom, opt))
                assert c.last_forward_kernel() == code, (name, geom, c.last_forward_kernel())
    finally:
        c.close()


@pytest.mark.parametrize("t", [(2.5, 2.5), (-30.5, -12.5)], ids=["pos", "neg"])
def test_forward_piecewise_tiles_at_ties(t):
    """k_fwd_pw_bins + k_fwd_pw_tiles against scatter + gather and the oracle: a half-scale-inverse tie mesh (destination 2 src + t with
    a half-integer t) puts every destination coordinate on a tie."""
    W, H = 256, 64
    img = O.lcg_image(W, H, 52)
    sp, tris, dp = E.tie_mesh([(0.0, 0.0, 8, 4, 32, 16, t)])
    md = O.minmax_xy(dp)
    geom = (int(md[0]), int(md[1]), int(md[2] - md[0]), int(md[3] - md[1]))
    ms = O.minmax_xy(sp)
    want = _fwd_pw_oracle(sp, dp, tris, img, geom)
    assert want.any()
    c = _ctx()
    try:
        c.set_image(img)
        c.piecewise_set_mesh(sp, tris, int(ms[0]), int(ms[1]))
        for opt, code in ((0, 1), (1, 2)):
            c.set_option("fwd_tiles", opt)
            _same(c.warp_forward_piecewise(dp, int(ms[2]), int(ms[3]), geom), want, (t, opt))
            assert c.last_forward_kernel() == code and c.redone_frames() == 0, (t, c.last_forward_kernel(), c.redone_frames())
    finally:
        c.close()
