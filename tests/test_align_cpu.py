"""CPU-side checks of the alignment feature (include/hgwarp.h, "refining transforms on the pixels"): the header declares and the library
exports the entries and enums, every refusal that needs no device is made in the header's order, hg_align_scale_matrix equals the model,
the numpy model of tests/hgtest/align.py is pinned by hand-worked facts and meets, on every case the GPU test runs, the conditions under
which n_valid, status and updates may be compared exactly; the chain detect -> match -> fit -> refine runs on the models alone; and the
kernel text itself runs on the host under sanitizers.  tests/test_gpu_align.py compares the device with the model."""
import ctypes as C
import json
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
from hgtest import align as AM               # noqa: E402
from hgtest import detect as DM              # noqa: E402

NEW = ["hg_align_scale_matrix", "hg_align_refine_frames_device"]
INVALID = 1
KINDS = (AM.AFFINE, AM.PROJECTIVE)
MODES = [(k, p) for k in KINDS for p in (0, 1)]
F64P = C.POINTER(C.c_double)
CLANGXX = next((p for p in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("clang++")) if p and os.path.exists(p)), None)
CSRC = os.path.join(ROOT, "homography.js_amd", "csrc")


def test_header_declares_and_library_exports_the_align_entry_points():
    text = open(os.path.join(ROOT, "include", "hgwarp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hg_[a-z0-9_]+)\s*\(", code))
    L = HG.lib()
    for name in NEW:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in HG.EXPORTS, name
    assert "refining transforms on the pixels" in text and "hg_align_refine_frames_device */" in text.split("enum {")[0]      # the section; the note beside HG_VERSION
    enums = dict(re.findall(r"\b(HG_ALIGN_[A-Z_]+) = (\d+)", code))
    assert enums == {"HG_ALIGN_CONVERGED": "0", "HG_ALIGN_MAX_ITER": "1", "HG_ALIGN_TOO_FEW": "2", "HG_ALIGN_SINGULAR": "3", "HG_ALIGN_WORSE": "4",
                     "HG_ALIGN_BAD_INPUT": "5", "HG_ALIGN_SUMS": "66"}
    assert (HG.ALIGN_CONVERGED, HG.ALIGN_MAX_ITER, HG.ALIGN_TOO_FEW, HG.ALIGN_SINGULAR, HG.ALIGN_WORSE, HG.ALIGN_BAD_INPUT, HG.ALIGN_SUMS) == (0, 1, 2, 3, 4, 5, 66)
    assert HG.ALIGN_INFO.itemsize == 48 and AM.INFO == HG.ALIGN_INFO
    assert callable(HG.align_scale_matrix) and callable(HG.Context.align_refine_frames_device) and callable(HG.align_refine_coarse_to_fine)
    assert AM.chunk() >= 256 and AM.chunk() % 256 == 0             # the constant the GPU test sizes its cases by


def test_refusals_without_a_device_in_the_headers_order():
    """Every shape check is made before the context is looked at (ctx is NULL throughout) and names itself in hg_last_error; a call that
    passes them all is refused for the NULL context.  Each bad argument is paired with a LATER one that is bad too: the earlier one must be
    the one reported."""
    L = HG.lib()
    good = dict(kind=1, Wf=64, Hf=48, n_frames=3, fs=64 * 48, Wt=97, Ht=71, n_to=1, ts=97 * 71, ch=1, rx=0, ry=0, rw=64, rh=48, step=2, photo=1, n_iter=8, eps=0.01,
                min_valid=10)

    def call(**k):
        a = dict(good, **k)
        code = L.hg_align_refine_frames_device(None, a["kind"], None, a["Wf"], a["Hf"], a["n_frames"], a["fs"], None, a["Wt"], a["Ht"], a["n_to"], a["ts"], a["ch"],
                                               a["rx"], a["ry"], a["rw"], a["rh"], a["step"], a["photo"], a["n_iter"], a["eps"], a["min_valid"], None, None, None, None)
        return code, L.hg_last_error(None).decode()

    order = [(dict(kind=2), "unknown kind"), (dict(kind=-1), "unknown kind"),
             (dict(Wf=0), "W and H"), (dict(Hf=32769), "W and H"), (dict(Wt=32768, Ht=32769), "W and H"),
             (dict(ch=3), "channels must"), (dict(ch=0), "channels must"),
             (dict(rw=0), "rectangle must"), (dict(rh=-1), "rectangle must"), (dict(rx=-1), "rectangle must"), (dict(rx=1), "rectangle must"), (dict(ry=1, rh=48), "rectangle must"),
             (dict(step=0), "step must"), (dict(step=65), "step must"),
             (dict(photo=2), "photometric must"), (dict(photo=-1), "photometric must"),
             (dict(n_iter=-1), "n_iter must"), (dict(n_iter=65), "n_iter must"),
             (dict(eps=-1.0), "eps must"), (dict(eps=float("nan")), "eps must"), (dict(eps=float("inf")), "eps must"),
             (dict(min_valid=9), "min_valid must"), (dict(kind=0, photo=0, min_valid=5), "min_valid must"), (dict(photo=0, min_valid=7), "min_valid must"),
             (dict(n_frames=-1), "n_frames must"), (dict(n_frames=4097), "n_frames must"),
             (dict(n_to=0), "n_to_sets must"), (dict(n_to=4), "n_to_sets must"), (dict(n_frames=0, n_to=2), "n_to_sets must"),
             (dict(fs=64 * 48 - 1), "stride must"), (dict(ts=97 * 71 - 1), "stride must"), (dict(ch=4), "stride must")]
    for k, (bad, word) in enumerate(order):
        code, msg = call(**bad)
        assert code == INVALID and word in msg, (bad, msg)
        for later, word2 in order[k + 1:]:
            if word2 == word or set(later) & set(bad):
                continue
            code, msg = call(**dict(later, **bad))
            assert code == INVALID and word in msg, (bad, later, msg)
    for ok in (dict(), dict(eps=0.0), dict(n_iter=0), dict(n_iter=64), dict(step=64), dict(kind=0, photo=0, min_valid=6), dict(n_frames=0), dict(n_frames=4096, n_to=4096),
               dict(rx=63, ry=47, rw=1, rh=1)):
        code, msg = call(**ok)
        assert code == INVALID and "ctx is NULL" in msg, (ok, msg)   # the limits themselves are legal: only the context is missing
    # hg_align_scale_matrix: host only
    m = (C.c_double * 8)(1, 0, 0, 0, 1, 0, 0, 0)
    out = (C.c_double * 8)()
    assert L.hg_align_scale_matrix(1, m, 0, 30, out) == 0 and L.hg_align_scale_matrix(0, m, 30, 0, out) == 0 and L.hg_align_scale_matrix(1, m, 3, 3, m) == 0
    for args in ((2, m, 0, 1, out), (-1, m, 0, 1, out), (1, m, -1, 0, out), (1, m, 0, 31, out), (1, m, 31, 0, out), (1, None, 0, 1, out), (1, m, 0, 1, None)):
        assert L.hg_align_scale_matrix(*args) == INVALID, args
    with pytest.raises(HG.HgError) as e:
        HG.align_scale_matrix(3, np.zeros(8), 0, 1)
    assert e.value.code == INVALID


@pytest.mark.parametrize("kind", KINDS)
def test_scale_matrix_equals_the_model_and_commutes_with_the_levels(kind):
    rng = np.random.default_rng(5)
    for _ in range(20):
        m = AM.TRUE[kind] * (1 + rng.uniform(-0.05, 0.05, 8))
        if kind == AM.AFFINE:
            m[6:] = 0
        for li, lo in ((0, 1), (0, 3), (3, 0), (2, 5), (4, 4), (0, 30), (30, 0)):
            got = HG.align_scale_matrix(kind, m, li, lo)
            want = AM.scale_matrix(kind, m, li, lo)
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (li, lo, got, want)
            if kind == AM.AFFINE:
                assert (got[6:] == 0).all()
        # a level-0 point and its level-k image commute with the converted matrix
        for k in (1, 2, 5):
            mk = AM.scale_matrix(kind, m, 0, k, AM.LD)
            x, y = rng.uniform(0, 60, 16), rng.uniform(0, 44, 16)
            u0, v0 = AM.apply_px(kind, m, x, y)
            to_k = lambda p: (np.asarray(p, AM.LD) + AM.LD(0.5)) / AM.LD(2) ** k - AM.LD(0.5)
            uk, vk = AM.apply_px(kind, mk.astype(AM.LD), to_k(x), to_k(y))
            assert float(np.abs(uk - to_k(u0)).max()) < 1e-12 and float(np.abs(vk - to_k(v0)).max()) < 1e-12
            back = AM.scale_matrix(kind, AM.scale_matrix(kind, m, 0, k), k, 0)
            assert AM.corner_displacement(kind, back, m, (0, 0, 64, 48)) < 1e-12


# ------------------------------------------------------------------------------------------------ the model, by hand
@pytest.mark.parametrize("kind,photometric", MODES)
def test_model_on_hand_worked_facts(kind, photometric):
    ident = np.array([1, 0, 0, 0, 1, 0, 0, 0], np.float64) if kind == AM.PROJECTIVE else np.array([1, 0, 0, 1, 0, 0, 0, 0], np.float64)
    scene = AM.to_scene(3, 64, 48)
    rect = (4, 4, 56, 40)
    # a constant TO plane: zero gradients, a zero geometric block, SINGULAR; the input's bits come back
    r = AM.refine(AM.case(kind, photometric, [scene], [DM.constant(64, 48)], [ident], rect, 1, 4))[0]
    assert r.status == AM.SINGULAR and r.updates == 0 and r.n_valid_first == 56 * 40 and np.array_equal(r.mat, ident)
    P = AM.p_of(kind, photometric)
    geo = 8 if kind == AM.PROJECTIVE else 6
    tri = np.zeros((P, P))
    tri[np.triu_indices(P)] = r.sums[:P * (P + 1) // 2]
    assert (tri[:geo] == 0).all() and (r.sums[P * (P + 1) // 2:P * (P + 1) // 2 + geo] == 0).all()
    # an identity start on identical planes: zero residual, delta = 0, CONVERGED after one update, rms exactly 0
    r = AM.refine(AM.case(kind, photometric, [scene], [scene], [ident], rect, 1, 4))[0]
    assert r.status == AM.CONVERGED and r.updates == 1 and r.disps == [0.0] and r.rms_first == 0 and r.rms_last == 0
    assert AM.corner_displacement(kind, r.mat, ident, rect) < 1e-12 and (r.gain, r.bias) == (1.0, 0.0)
    # FROM = TO shifted by whole pixels (3 right, 2 down), started one pixel off: ends at the shift
    frm = np.zeros_like(scene)
    frm[:46, :61] = scene[2:, 3:]
    shift = AM.from3x3(kind, np.array([[1, 0, 3.0], [0, 1, 2.0], [0, 0, 1]]))
    start = AM.from3x3(kind, np.array([[1, 0, 3.7], [0, 1, 1.3], [0, 0, 1]]))
    eps = 1e-6
    c = AM.case(kind, photometric, [frm], [scene], [start], (4, 4, 52, 36), 1, 16, eps)
    r, rl = AM.refine(c)[0], AM.refine(c, AM.LD)[0]
    assert r.status == AM.CONVERGED and rl.status == AM.CONVERGED and r.updates == rl.updates
    err = AM.corner_displacement(kind, r.mat, shift, c.rect)
    print(f"whole-pixel shift, kind {kind}, photometric {photometric}: {r.updates} updates, {err:.3g} px from the shift, displacements {r.disps}")
    # the picture is exact at the shift (every residual is 0 there), so the shift is the iteration's fixed point; near it every update
    # shrinks the displacement by a factor rho < 1 / 2 (asserted; measured 1 / 6 to 1 / 9), and what remains after a displacement d < eps
    # is below d rho / (1 - rho) < eps
    tail = r.disps[-4:]
    assert all(b < a / 2 for a, b in zip(tail, tail[1:])), r.disps
    assert err < eps, (err, r.disps)
    assert r.rms_last < 1e-3 * r.rms_first


@pytest.mark.parametrize("kind,photometric", MODES)
def test_a_brightened_frame_needs_the_photometric_terms(kind, photometric):
    """A frame brightened by x 1.2 + 10 (clipped) ends nearer the truth with the gain and bias terms than without."""
    to = AM.to_scene(11)
    true = AM.TRUE[kind]
    frm = AM.resample(to, kind, true, 64, 48, 1.2, 10.0)
    rect = (2, 2, 60, 44)
    start = AM.perturbed(kind, true, rect, 0.9, 3)
    err = {}
    for ph in (0, 1):
        r = AM.refine(AM.case(kind, ph, [frm], [to], [start], rect, 1, 8, 1e-6))[0]
        err[ph] = AM.corner_displacement(kind, r.mat, true, rect)
    print(f"brightened frame, kind {kind}: {err[0]:.3f} px without, {err[1]:.3f} px with the photometric terms (start 0.9 px)")
    assert err[1] < err[0] and err[1] < 0.9


# ------------------------------------------------------------------------------------------------ the GPU test's cases meet the model's conditions
def gpu_cases():
    """Every case tests/test_gpu_align.py sends to the device, by name."""
    ch = AM.chunk()
    for kind, ph in MODES:
        for n in (1, 63, 64, 65, 255, 256, 257, ch - 1, ch, ch + 1, 2 * ch + 1):
            yield ("count", kind, ph, n), AM.count_case(kind, ph, n)
        for step in (1, 2, 3, 64):
            yield ("step", kind, ph, step), AM.step_case(kind, ph, step)
        yield ("offset", kind, ph), AM.offset_rect_case(kind, ph)
        for row in (True, False):
            yield ("line", kind, ph, row), AM.line_case(kind, ph, row)
            yield ("line, too few", kind, ph, row), AM.line_case(kind, ph, row, 100)
        for args in ((1, 1, 0), (4, 1, 0), (4, 2, 0), (1, 3, 64), (4, 3, 64), (1, 1, 32, True), (4, 1, 0, True)):
            yield ("planes", kind, ph) + args, AM.planes_case(kind, ph, *args)
        yield ("statuses", kind, ph), AM.status_case(kind, ph)
        for px in (1.0, 2.0):
            yield ("planted", kind, ph, px), AM.planted_case(kind, ph, px)


def test_the_model_meets_the_conditions_of_an_exact_comparison_on_every_gpu_case():
    """No sample within 1e-6 of a validity bound, no displacement within a factor 4 of eps, no final rms within 1e-9 (relative) of the
    first -- and the float64 and the longdouble-sums models agree on status, updates and counts: only then may a device that sums in
    another order be compared exactly."""
    n = 0
    for name, c in gpu_cases():
        a, b = AM.refine(c), AM.refine(c, AM.LD)
        AM.conditions(c, a, name)
        AM.conditions(c, b, name)
        for f, (x, y) in enumerate(zip(a, b)):
            assert (x.status, x.updates, x.n_valid_first, x.n_valid_last) == (y.status, y.updates, y.n_valid_first, y.n_valid_last), (name, f)
        n += 1
    assert n == 4 * 30
    c, _ = AM.walk_case()
    for T in (AM.F64, AM.LD):
        for ck in AM.walk(c, 3, T)[2]:
            AM.conditions(ck, AM.refine(ck, T), ("walk", ck.rect))


def test_the_statuses_and_the_lines_come_out_as_planned():
    for kind, ph in MODES:
        res = AM.refine(AM.status_case(kind, ph))
        assert [r.status for r in res] == [AM.CONVERGED, AM.MAX_ITER, AM.TOO_FEW, AM.BAD_INPUT, AM.SINGULAR]
        assert res[0].updates == 1 and res[1].updates == 2 and res[2].n_valid_first == 0 and np.isnan(res[2].rms_first) and np.isnan(res[3].mat).all()
        for row in (True, False):
            assert all(r.status == AM.SINGULAR for r in AM.refine(AM.line_case(kind, ph, row)))
            assert all(r.status == AM.TOO_FEW for r in AM.refine(AM.line_case(kind, ph, row, 100)))
        small = AM.refine(AM.planes_case(kind, ph, 1, 1, 32, True))
        assert all(0 < r.n_valid_first < 93 * 67 for r in small)     # a TO plane smaller than the FROM plane: part of every frame is invalid


# ------------------------------------------------------------------------------------------------ the chain on the models alone
def test_the_chain_on_the_models_alone():
    """DM.chain_case(CHAIN_SEED): detect, match and fit (no refit) by their numpy models, then 8 updates at step 2 with the photometric
    terms.  The corner error of every frame comes out no larger than before and below AM.CHAIN_BOUND = 0.0035 px = 2 x the largest the model
    reaches.  Measured (before -> after, px): shift 5.8e-14 -> 2.1e-14, 20 degrees 0.578 -> 0.00172, 30 degrees with perspective 0.842 ->
    0.00094; in 1, 3 and 3 updates (eps 0.01)."""
    c = AM.chain_case()
    before = AM.chain_errors(c.mats)
    res = AM.refine(c, key="chain")
    after = AM.chain_errors(np.stack([r.mat for r in res]))
    print("chain: corner errors before", before, "after", after, "updates", [r.updates for r in res])
    assert [round(b, 2) for b in before] == [0.0, 0.58, 0.84]
    assert all(r.status in (AM.CONVERGED, AM.MAX_ITER) for r in res)
    for f in range(3):
        assert after[f] <= before[f] and after[f] < AM.CHAIN_BOUND, (f, before[f], after[f])
    assert max(after) > AM.CHAIN_BOUND / 2.5                         # the bound is 2 x what is reached, not a loose one


# ------------------------------------------------------------------------------------------------ the kernel text on the host
@pytest.mark.skipif(CLANGXX is None, reason="clang++ (ROCm's) not available")
def test_kernel_source_text_on_the_host_under_sanitizers(tmp_path):
    """tests/cpp/align_check.cpp: hg_k_align.hip itself, compiled for the CPU behind the thread-index shim -- a workgroup of either kernel as
    256 host threads -- and run under ASan + UBSan on exact-size heap buffers: no byte outside a buffer is touched (the canary of every
    output is the allocation's end), and what the kernels compute is the model's by the GPU test's rule.  d_sums passed as NULL changes no
    other output.  The cases are the GPU test's small ones.  A stand-alone program; nothing is loaded into Python."""
    exe = str(tmp_path / "align_check")
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wno-everything", "-pthread", "-I", os.path.join(cpp, "hip_stub"), "-I", CSRC, os.path.join(cpp, "align_check.cpp"), "-o", exe],
                   check=True, cwd=str(tmp_path), timeout=600)
    n_case = [0]

    def run(c, want_sums=True):
        fin, fout = tmp_path / f"case{n_case[0]}.in", tmp_path / f"case{n_case[0]}.out"
        n_case[0] += 1
        fin.write_bytes(AM.pack(c, want_sums))
        p = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and "host check ran" in p.stdout, (n_case[0], (p.stdout + p.stderr)[-3000:])
        assert "runtime error" not in p.stdout + p.stderr and "AddressSanitizer" not in p.stderr, (n_case[0], (p.stdout + p.stderr)[-3000:])
        raw, F = fout.read_bytes(), len(c.frm)
        assert len(raw) == F * (112 + (528 if want_sums else 0))
        return AM.unpack(raw[:F * 64], raw[F * 64:F * 112], raw[F * 112:] if want_sums else None, F)

    ch = AM.chunk()
    worst = 0.0
    for kind, ph in MODES:
        for n in (1, 64, 257, ch + 1):
            c = AM.count_case(kind, ph, n)
            worst = max(worst, AM.check(c, run(c), ("count", kind, ph, n)))
        for name, c in (("step 3", AM.step_case(kind, ph, 3)), ("step 64", AM.step_case(kind, ph, 64)), ("line", AM.line_case(kind, ph, True)),
                        ("rgba, two TO sets", AM.planes_case(kind, ph, 4, 2, 0)), ("strides, small TO", AM.planes_case(kind, ph, 1, 1, 32, True)),
                        ("statuses", AM.status_case(kind, ph)), ("planted", AM.planted_case(kind, ph, 1.0))):
            g = run(c)
            worst = max(worst, AM.check(c, g, (name, kind, ph)))
            if name == "statuses":
                bare = run(c, want_sums=False)
                assert bare.mats.tobytes() == g.mats.tobytes() and bare.info.tobytes() == g.info.tobytes()
                one = run(AM.alone(c, 0))
                assert one.mats[0].tobytes() == g.mats[0].tobytes() and one.info[0].tobytes() == g.info[0].tobytes() and one.sums[0].tobytes() == g.sums[0].tobytes()
    print(f"host check: largest kernel / base ratio {worst:.3g}")


# ------------------------------------------------------------------------------------------------ the drop-in class
@pytest.mark.skipif(shutil.which("node") is None, reason="node is missing")
def test_js_class_refine_alignment_over_the_recording_mock_addon():
    """tests/js/align_class.mjs: h.refineAlignment(fromImages, toImages, matrices, options) over a recording mock addon: the option
    defaults, the bare strings it throws, the shape of the result, and the level walk -- the sequence of calls, their level sizes and
    rectangles, and the matrices converted between the levels."""
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "align_class.mjs")], capture_output=True, text=True, timeout=300,
                       cwd=ROOT, env=dict(os.environ, HGWARP_ADDON=os.path.join(ROOT, "tests", "js", "mock_align_addon.cjs")))
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads(line[-1])
    assert res["ok"] and res["fails"] == [] and p.returncode == 0, (res["fails"], p.stderr[-2000:])
    assert res["checks"] >= 30
