"""CPU-side checks of the bundle adjustment (include/hgwarp.h, "adjusting a frame set over all pairs"): the header declares and the library
exports the entries and enums; every refusal that needs no device is made in the header's order; hg_bundle_chain_from_pairs and
hg_bundle_invert_matrix equal numpy; the numpy model of tests/hgtest/bundle.py agrees with scipy.optimize.least_squares on the same
residual, closes a ring of frames better than the chain does and resists outliers with huber; on every case the GPU test compares exactly no
decision of the model lies near a tie; and the kernel text itself runs on the host under sanitizers.  tests/test_gpu_bundle.py compares the
device with the model."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "homography.js_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hgwarp as HG                          # noqa: E402
from hgtest import bundle as BM              # noqa: E402

NEW = ["hg_bundle_layout", "hg_bundle_adjust_frames_device", "hg_bundle_chain_from_pairs", "hg_bundle_invert_matrix"]
INVALID = 1
KINDS = (BM.AFFINE, BM.PROJECTIVE)
U = 2.0 ** -53
CLANGXX = next((p for p in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("clang++")) if p and os.path.exists(p)), None)
CSRC = os.path.join(ROOT, "homography.js_amd", "csrc")


def test_header_declares_and_library_exports_the_bundle_entry_points():
    text = open(os.path.join(ROOT, "include", "hgwarp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hg_[a-z0-9_]+)\s*\(", code))
    L = HG.lib()
    for name in NEW:
        assert name in declared and hasattr(L, name) and name in HG.EXPORTS, name
    assert "adjusting a frame set over all pairs" in text
    enums = dict(re.findall(r"\b(HG_BUNDLE_[A-Z_]+) = (\d+)", code))
    assert enums == {"HG_BUNDLE_MAX_FRAMES": "256", "HG_BUNDLE_MAX_PAIRS": "8192", "HG_BUNDLE_CONVERGED": "0", "HG_BUNDLE_MAX_ITER": "1", "HG_BUNDLE_STALLED": "2",
                     "HG_BUNDLE_SINGULAR": "3", "HG_BUNDLE_FRAME_ADJUSTED": "0", "HG_BUNDLE_FRAME_FIXED": "1", "HG_BUNDLE_FRAME_UNANCHORED": "2",
                     "HG_BUNDLE_FRAME_BAD_INPUT": "3", "HG_BUNDLE_SUMS": "154"}
    assert (HG.BUNDLE_CONVERGED, HG.BUNDLE_MAX_ITER, HG.BUNDLE_STALLED, HG.BUNDLE_SINGULAR, HG.BUNDLE_SUMS) == (0, 1, 2, 3, 154) == \
        (BM.CONVERGED, BM.MAX_ITER, BM.STALLED, BM.SINGULAR, BM.SUMS)
    assert (HG.BUNDLE_FRAME_ADJUSTED, HG.BUNDLE_FRAME_FIXED, HG.BUNDLE_FRAME_UNANCHORED, HG.BUNDLE_FRAME_BAD_INPUT) == (BM.ADJUSTED, BM.FIXED, BM.UNANCHORED, BM.BAD_INPUT)
    assert HG.BUNDLE_INFO.itemsize == 48 and HG.BUNDLE_PAIR_INFO.itemsize == 24 and HG.bundle_info_bytes(3, 2) == 48 + 16 + 48
    assert BM.chunk() % 128 == 0 and BM.lds_cap() >= 2 * BM.panel() and (BM.lds_cap() + 1) * BM.lds_cap() * 8 <= 160 * 1024     # the constants the GPU test sizes its cases by
    assert BM.SUMS == 17 * 9 + 1


def test_refusals_without_a_device_in_the_headers_order():
    """Every shape check is made before the context is looked at (ctx is NULL throughout) and names itself in hg_last_error; a call that
    passes them all is refused for the NULL context.  Each bad argument is paired with a LATER one that is bad too: the earlier one must be
    the one reported."""
    L = HG.lib()
    good = dict(kind=1, W=96, H=64, F=3, fixed=[1, 0, 0], pairs=[0, 1, 1, 2], NP=2, n=8, counts=[8, 8], n_iter=5, eps=0.01, lam=1e-3, huber=0.0, scratch=1 << 30)
    fake = C.c_void_p(1 << 20)                                    # (never dereferenced: the context is refused first)

    def call(**k):
        a = dict(good, **k)
        fx = (C.c_uint8 * max(len(a["fixed"]), 1))(*a["fixed"]) if a["fixed"] is not None else None
        pr = (C.c_int32 * max(len(a["pairs"]), 1))(*a["pairs"]) if a["pairs"] is not None else None
        cn = (C.c_int32 * max(len(a["counts"]), 1))(*a["counts"]) if a["counts"] is not None else None
        code = L.hg_bundle_adjust_frames_device(None, a["kind"], a["W"], a["H"], a["F"], fx, pr, a["NP"], fake, a["n"], cn, None, a["n_iter"], a["eps"], a["lam"],
                                                a["huber"], fake, fake, fake, None, fake, a["scratch"])
        return code, L.hg_last_error(None).decode()

    nan, inf = float("nan"), float("inf")
    order = [(dict(kind=2), "unknown kind"), (dict(kind=-1), "unknown kind"),
             (dict(W=0), "W and H"), (dict(H=32769), "W and H"),
             (dict(F=-1), "n_frames must"), (dict(F=257), "n_frames must"),
             (dict(NP=-1), "n_pairs must"), (dict(NP=8193), "n_pairs must"),
             (dict(n=-1), "n_points must"), (dict(n=65537), "n_points must"),
             (dict(pairs=[0, 3, 1, 2]), "pairs[0]"), (dict(pairs=[0, 1, 2, 2]), "pairs[1]"), (dict(pairs=[-1, 1, 1, 2]), "pairs[0]"), (dict(pairs=None), "pairs is NULL"),
             (dict(counts=[8, 9]), "counts[1]"), (dict(counts=[-1, 8]), "counts[0]"),
             (dict(n_iter=-1), "n_iter must"), (dict(n_iter=65), "n_iter must"),
             (dict(eps=-1.0), "eps must"), (dict(eps=nan), "eps must"), (dict(eps=inf), "eps must"),
             (dict(lam=0.0), "lambda0 must"), (dict(lam=-1.0), "lambda0 must"), (dict(lam=nan), "lambda0 must"), (dict(lam=inf), "lambda0 must"),
             (dict(huber=-1.0), "huber must"), (dict(huber=nan), "huber must"), (dict(huber=inf), "huber must"),
             (dict(fixed=None), "fixed is NULL"), (dict(fixed=[0, 0, 0]), "at least one frame"),
             (dict(scratch=HG.bundle_layout(1, 3, 2, 8) - 1), "scratch_bytes")]
    for k, (bad, word) in enumerate(order):
        code, msg = call(**bad)
        assert code == INVALID and word in msg, (bad, msg)
        for later, word2 in order[k + 1:]:
            if word2 == word or set(later) & set(bad) or ("F" in bad and ("pairs" in later or "fixed" in later)) or ("n" in bad and "counts" in later):
                continue
            code, msg = call(**dict(later, **bad))
            assert code == INVALID and word in msg, (bad, later, msg)
    for ok in (dict(), dict(eps=0.0), dict(n_iter=0), dict(n_iter=64), dict(huber=3.0), dict(kind=0), dict(F=0, pairs=[], NP=0, fixed=[], counts=[]),
               dict(counts=None), dict(scratch=HG.bundle_layout(1, 3, 2, 8)), dict(pairs=[0, 1, 1, 0]), dict(pairs=[0, 1, 0, 1])):
        code, msg = call(**ok)
        assert code == INVALID and "ctx is NULL" in msg, (ok, msg)   # the limits themselves are legal: only the context is missing
    # 2048 unknowns: 256 projective frames with one fixed are 2040
    code = L.hg_bundle_adjust_frames_device(None, 1, 96, 64, 256, (C.c_uint8 * 256)(1), (C.c_int32 * 510)(*[v for f in range(255) for v in (f, f + 1)]), 255, fake, 8,
                                            None, None, 2, 0.01, 1e-3, 0.0, fake, fake, fake, None, fake, 1 << 40)
    assert code == INVALID and "ctx is NULL" in L.hg_last_error(None).decode()
    # the layout and the host helpers
    total = C.c_size_t(7)
    assert L.hg_bundle_layout(1, 0, 0, 0, C.byref(total)) == 0 and total.value == 0
    assert L.hg_bundle_layout(1, 3, 2, 8, C.byref(total)) == 0 and total.value > 0 and total.value % 256 == 0
    for args in ((2, 3, 2, 8), (1, 257, 2, 8), (1, 3, 8193, 8), (1, 3, 2, 65537), (1, -1, 2, 8)):
        assert L.hg_bundle_layout(*args, C.byref(total)) == INVALID, args
    assert L.hg_bundle_layout(1, 3, 2, 8, None) == INVALID
    assert HG.bundle_layout(1, 256, 1000, 256) > HG.bundle_layout(1, 16, 30, 2048) > 0
    m = (C.c_double * 8)(1, 0, 0, 0, 1, 0, 0, 0)
    out = (C.c_double * 8)()
    assert L.hg_bundle_invert_matrix(1, m, out) == 0 and L.hg_bundle_invert_matrix(0, m, m) == 0
    for args in ((2, m, out), (-1, m, out), (1, None, out), (1, m, None)):
        assert L.hg_bundle_invert_matrix(*args) == INVALID, args
    pr = (C.c_int32 * 2)(0, 1)
    for args in ((2, 2, pr, 1, m, 0, out), (1, 257, pr, 1, m, 0, out), (1, 2, pr, 1, m, 2, out), (1, 2, pr, 1, m, -1, out), (1, 2, pr, 1, None, 0, out),
                 (1, 2, pr, 1, m, 0, None), (1, 1, pr, 1, m, 0, out), (1, 2, None, 1, m, 0, out)):
        assert L.hg_bundle_chain_from_pairs(*args) == INVALID, args
    with pytest.raises(HG.HgError) as e:
        HG.bundle_invert_matrix(3, np.zeros(8))
    assert e.value.code == INVALID


# ------------------------------------------------------------------------------------------------ the host helpers
def cond3(kind, m):
    return float(np.linalg.cond(BM.to3x3(kind, m)))


@pytest.mark.parametrize("kind", KINDS)
def test_invert_matrix_equals_numpy(kind):
    """The adjugate inverse against numpy's in longdouble: entry by entry within 16 u cond(M) of the largest entry, M invert(M) = identity
    within the same, affine stays affine, and the call may work in place."""
    rng = np.random.default_rng(2)
    for m in BM.true_mats(kind, 8, 96, 64, rng):
        got = HG.bundle_invert_matrix(kind, m)
        want = BM.from3x3(kind, np.linalg.inv(BM.to3x3(kind, m)).astype(BM.LD))
        bound = 16 * U * cond3(kind, m)
        assert np.abs(got - want.astype(np.float64)).max() <= bound * np.abs(want.astype(np.float64)).max(), (m, got, want)
        prod = BM.to3x3(kind, m, BM.LD) @ BM.to3x3(kind, got, BM.LD)
        assert np.abs(prod / prod[2, 2] - np.eye(3)).max() <= bound * max(1.0, float(np.abs(BM.to3x3(kind, m)).max()))
        if kind == BM.AFFINE:
            assert got[6] == 0 and got[7] == 0
        buf = np.array(m, np.float64)
        p = buf.ctypes.data_as(C.POINTER(C.c_double))
        assert HG.lib().hg_bundle_invert_matrix(kind, p, p) == 0 and np.array_equal(buf, got)


@pytest.mark.parametrize("kind", KINDS)
def test_chain_from_pairs_equals_numpy(kind):
    """Breadth-first from the anchor with a repeated pair (the first in index order wins), a reversed pair, a pair of NaNs that is skipped
    and a frame nobody reaches, against the longdouble chain: within 64 u times the product of the condition numbers along the walk."""
    rng = np.random.default_rng(3)
    truth = BM.true_mats(kind, 6, 96, 64, rng)

    def pm(a, b, wobble=0.0):                                    # maps frame a to frame b
        q = np.linalg.inv(BM.to3x3(kind, truth[b])) @ BM.to3x3(kind, truth[a])
        q[0, 2] += wobble
        return BM.from3x3(kind, q)
    pairs = [(0, 1), (0, 1), (2, 1), (1, 3), (3, 4), (0, 3), (2, 4)]
    mats = np.stack([pm(0, 1), pm(0, 1, 5.0), pm(2, 1), np.full(8, np.nan), pm(3, 4), pm(0, 3, 1.0), pm(2, 4, 9.0)])
    got = HG.bundle_chain_from_pairs(kind, 6, pairs, mats, anchor=0)
    want = BM.chain(kind, 6, pairs, mats, 0)
    kappa = np.prod([cond3(kind, m) for m in mats if np.isfinite(m).all()])
    assert np.isnan(got[5]).all() and np.isnan(want[5]).all()
    for f in range(5):
        assert np.abs(got[f] - want[f]).max() <= 64 * U * kappa * max(1.0, np.abs(want[f]).max()), (f, got[f], want[f])
    assert BM.corner_displacement(kind, got[1], truth[1], 96, 64) < 1e-9          # the first (0, 1), not the wobbled one
    assert BM.corner_displacement(kind, got[2], truth[2], 96, 64) < 1e-9          # through the reversed pair (2, 1) in level 2, not (2, 4)
    assert 0.9 < BM.corner_displacement(kind, got[3], truth[3], 96, 64) < 1.1     # (1, 3) is NaN: (0, 3) with its wobble of a pixel, level 1
    assert BM.corner_displacement(kind, got[4], truth[4], 96, 64) > 0.5           # 4 hangs on 3
    other = HG.bundle_chain_from_pairs(kind, 6, pairs, mats, anchor=4)
    ident = np.array([1, 0, 0, 0, 1, 0, 0, 0.0]) if kind == BM.PROJECTIVE else np.array([1, 0, 0, 1, 0, 0, 0, 0.0])
    assert np.array_equal(other[4], ident) and np.isnan(other[5]).all() and np.isfinite(other[:5]).all()
    assert HG.bundle_chain_from_pairs(kind, 0, np.zeros((0, 2), np.int32), np.zeros((0, 8))).shape == (0, 8)


# ------------------------------------------------------------------------------------------------ the model against scipy
def scipy_adjust(c):
    """scipy.optimize.least_squares over the parameters of the free frames, on the model's own residual (pixels, huber off)."""
    from scipy.optimize import least_squares
    cls, fidx = BM.classify(c)
    P = BM.p_of(c.kind)
    X0 = np.stack([BM.normalise(c.kind, c.mats[f], c.W, c.H) for f in range(c.F)])
    s = 2.0 / max(c.W, c.H)

    def unpack(x):
        X = X0.copy()
        for f in range(c.F):
            if cls[f] == 0:
                for j in range(P):
                    X[f, BM.SLOT[c.kind][j]] = x[fidx[f] * P + j]
        return X

    def fun(x):
        X = unpack(x)
        out = []
        for p, (a, b) in enumerate(c.pairs):
            n = int(c.counts[p])
            ok, V, w, rho = BM.slots(c.kind, X[a], X[b], c.matches[p, :n], np.ones(n, bool), c.W, c.H, 0.0, np.float64)
            out += [V[:, 0, 2 * P] / s, V[:, 1, 2 * P] / s]
        return np.concatenate(out)
    x0 = np.concatenate([[X0[f, BM.SLOT[c.kind][j]] for j in range(P)] for f in range(c.F) if cls[f] == 0])
    r = least_squares(fun, x0, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=20000)
    X = unpack(r.x)
    mats = np.stack([BM.denormalise(c.kind, X[f], c.W, c.H) if cls[f] == 0 else c.mats[f] for f in range(c.F)])
    return mats, float(np.sum(r.fun ** 2)), len(r.fun) // 2


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("F", (4, 5, 6))
def test_model_and_scipy_find_the_planted_frames(kind, F):
    """Noise-free planted frames started a few pixels off, the coordinates rounded to float32 as the call receives them.  A coordinate c
    is off by at most |c| 2^-24 after the rounding, a slot has four of them and a frame -> canvas matrix here stretches by less than 1.1, so
    at the planted matrices no residual exceeds 4.4 cmax 2^-24 px: both solvers must end at an rms below that, and at the same matrices
    within it."""
    c = BM.planted_case(kind, F=F, seed=20 + F, px=1.5, n_iter=40, eps=1e-9)
    start = BM.truth_error(c, c.mats)
    assert 2.0 <= start <= 8.0, start
    bound = 4.4 * float(np.abs(c.matches).max()) * 2.0 ** -24
    m = BM.adjust(c)
    mats, cost, n = scipy_adjust(c)
    rms_model, rms_scipy = float(m.info["rms_last"]), np.sqrt(cost / n)
    print(f"kind {kind}, {F} frames: start {start:.3g} px, bound {bound:.3g} px, rms model {rms_model:.3g}, scipy {rms_scipy:.3g}")
    assert rms_model < bound and rms_scipy < bound and m.info["n_valid_last"] == n
    for f in range(F):
        assert BM.corner_displacement(kind, m.mats[f], mats[f], c.W, c.H) < bound, f
        assert BM.corner_displacement(kind, m.mats[f], c.truth[f], c.W, c.H) < 64 * bound, f


@pytest.mark.parametrize("kind", KINDS)
def test_model_reaches_scipys_cost_on_noisy_matches(kind):
    """sigma = 0.5 px: the model's final cost is not above scipy's by more than 16 x the model's own base (float64 against longdouble)."""
    c = BM.planted_case(kind, F=5, seed=31, px=1.5, sigma=0.5, n_iter=60, eps=1e-10)
    m, l = BM.adjust(c), BM.adjust(c, BM.LD)
    mats, cost, n = scipy_adjust(c)
    base = max(float(BM.rel(m.info["cost_last"], l.info["cost_last"])), BM.HALF_ULP)
    print(f"kind {kind}: cost model {float(m.info['cost_last']):.17g}, scipy {cost:.17g}, base {base:.3g}")
    assert m.info["n_valid_last"] == n and float(m.info["cost_last"]) <= cost * (1 + 16 * base)
    assert 0.3 < float(m.info["rms_last"]) / np.sqrt(2) < 0.7


# ------------------------------------------------------------------------------------------------ the demonstrations
def test_the_ring_closes_on_the_model():
    """BM.ring_case(seed 5): 8 frames of 96 x 64 around a 3 x 3 block, 32 matches per neighbouring pair with sigma = 0.5 px, pairwise
    least-squares matrices (the model of the fit's n_hyp = 0 refit), chained without the closing pair (7, 0).  Over all 8 pairs the chain's
    rms is 0.823 px, the adjusted frames' 0.660 px (the README's numbers); the closing pair alone misses by more than the rest."""
    c = BM.ring_case(5)
    m = BM.adjust(c)
    before, after = BM.rms_over_pairs(c, c.mats), BM.rms_over_pairs(c, m.mats)
    print(f"ring: {before:.4g} px chained, {after:.4g} px adjusted; closing pair {float(m.pairs['rms_first'][7]):.4g} -> {float(m.pairs['rms_last'][7]):.4g} px")
    assert m.info["status"] == BM.CONVERGED and after < before
    assert abs(before - 0.823) < 5e-3 and abs(after - 0.660) < 5e-3
    assert m.pairs["rms_first"][7] == max(m.pairs["rms_first"]) and m.pairs["rms_last"][7] < m.pairs["rms_first"][7]
    got = HG.bundle_chain_from_pairs(c.kind, 8, c.pairs[:7], c.pair_mats[:7], 0)
    for f in range(8):
        assert BM.corner_displacement(c.kind, got[f], c.mats[f], c.W, c.H) < 1e-9      # the library's chain is the case's start


@pytest.mark.parametrize("kind", KINDS)
def test_huber_resists_outliers_on_the_model(kind):
    """10 % of the slots moved by 30 px, no mask: with huber = 1 the model ends closer to the planted matrices than with huber = 0."""
    res = {}
    for huber in (0.0, 1.0):
        c = BM.huber_case(huber, kind)
        res[huber] = BM.truth_error(c, BM.adjust(c).mats)
    print(f"kind {kind}: corner error {res[0.0]:.3g} px without, {res[1.0]:.3g} px with huber")
    assert res[1.0] < res[0.0]


def test_gpu_cases_have_no_decision_near_a_tie():
    """The conditions under which tests/test_gpu_bundle.py compares status, rounds, accepted and n_valid exactly (BM.decisions_clear): the
    float64 and the longdouble model take the same decisions, and no accepted / rejected cost, no displacement against eps and no lambda
    against 1e12 lies within 16 x the cost's base of its tie.  Every listed case meets them."""
    for name, c in list(BM.gpu_cases()) + [(("big",), BM.big_case())]:
        m, l = BM.adjust(c), BM.adjust(c, BM.LD)
        assert BM.decisions_clear(m, l), (name, m.margin, m.info, l.info)


def test_model_statuses():
    """MAX_ITER on an evaluation, STALLED when nothing can improve, SINGULAR is out of reach of a positive lambda0 on finite sums."""
    c = BM.planted_case(BM.PROJECTIVE, F=3, extra=(), n_iter=0)
    assert BM.adjust(c).info["status"] == BM.MAX_ITER and BM.adjust(c).info["rounds"] == 0
    c = BM.planted_case(BM.AFFINE, F=3, extra=(), sigma=0.3, n_iter=64, eps=0.0)
    m = BM.adjust(c)
    assert m.info["status"] == BM.STALLED and m.info["lambda_last"] > 1e12 and m.info["accepted"] >= 1


# ------------------------------------------------------------------------------------------------ the kernel text on the host
@pytest.mark.skipif(CLANGXX is None, reason="clang++ (ROCm's) not available")
def test_kernel_source_text_on_the_host_under_sanitizers(tmp_path):
    """tests/cpp/bundle_check.cpp: hg_k_bundle.hip itself, compiled for the CPU behind the thread-index shim -- a workgroup as real host
    threads -- and run under ASan + UBSan on exact-size heap buffers: the pass, the reduction, the assembly, both solve paths (the blocked
    one forced at a small N by a flag of the case) and the decision, against the model by the GPU test's rule; the two paths give the same
    bytes.  A stand-alone program; nothing is loaded into Python."""
    exe = str(tmp_path / "bundle_check")
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wno-everything", "-pthread", "-I", os.path.join(cpp, "hip_stub"), "-I", CSRC, os.path.join(cpp, "bundle_check.cpp"), "-o", exe],
                   check=True, cwd=str(tmp_path), timeout=600)
    n_case = [0]

    def run(c, large=False, want_sums=True):
        fin, fout = tmp_path / f"case{n_case[0]}.in", tmp_path / f"case{n_case[0]}.out"
        n_case[0] += 1
        fin.write_bytes(BM.pack(c, large, want_sums))
        p = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and "host check ran" in p.stdout, (n_case[0], (p.stdout + p.stderr)[-3000:])
        assert "runtime error" not in p.stdout + p.stderr and "AddressSanitizer" not in p.stderr, (n_case[0], (p.stdout + p.stderr)[-3000:])
        return BM.unpack_host(fout.read_bytes(), c, want_sums)

    worst = 0.0
    for kind in KINDS:
        cases = [BM.count_case(kind, n) for n in (0, 1, 257, BM.chunk() + 1)]
        cases += [BM.planted_case(kind, sigma=0.3, huber=1.0, n=70), BM.free_case(kind, 5)]
        # the blocked path at one panel exactly (N = 32), below one (30), and at two panels plus a remainder (N = 80, 66)
        cases = [BM.free_case(kind, n_free) for n_free in ((4, 10) if kind == BM.PROJECTIVE else (5, 11))] + cases
        for c in cases:
            g = run(c)
            m64, mld = BM.adjust(c), BM.adjust(c, BM.LD)
            worst = max(worst, BM.compare(c, g, m64, mld))
            assert BM.decisions_clear(m64, mld)
            BM.compare_exact(g, m64)
            big = run(c, large=True)
            assert big.raw == g.raw, "the blocked solve and the one-workgroup solve give the same bytes"
        bare = run(cases[-2], want_sums=False)
        assert bare.mats.tobytes() == run(cases[-2]).mats.tobytes()
    print(f"host check: largest kernel / base ratio {worst:.3g}")


# ------------------------------------------------------------------------------------------------ the drop-in class
@pytest.mark.skipif(shutil.which("node") is None, reason="node is missing")
def test_js_class_bundle_adjust_over_the_recording_mock_addon():
    """tests/js/bundle_class.mjs: h.bundleAdjust, h.chainMatrices and h.invertMatrix over a recording mock addon: the option defaults, how
    lists, masks, pairs and fixed frames are marshalled, the bare strings they throw, the shape of the results."""
    import json
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "bundle_class.mjs")], capture_output=True, text=True, timeout=300,
                       cwd=ROOT, env=dict(os.environ, HGWARP_ADDON=os.path.join(ROOT, "tests", "js", "mock_bundle_addon.cjs")))
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads(line[-1])
    assert res["ok"] and res["fails"] == [] and p.returncode == 0, (res["fails"], p.stderr[-2000:])
    assert res["checks"] >= 50
