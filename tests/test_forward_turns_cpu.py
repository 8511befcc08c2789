"""The builders and the bins model of tests/hgtest/fwd_turns.py, checked without a GPU: the model of k_fwd_pw_bins reproduces what every
existing piecewise case of fwd_edges claims about that kernel (which tests/test_gpu_forward_edges.py holds the kernel itself to); every
named case has the matrices it is named for, stays on the tile path by the model, and the classifier's last-writer resolution equals the
oracle's bytes on an image that names every source pixel; the fuzz reaches every class often enough that the GPU test cannot pass empty."""
import numpy as np
import pytest

from hgtest import fwd_edges as F
from hgtest import fwd_turns as T

PW = F.piecewise_cases()
NAMED = T.named_cases()
FUZZ_SEED, FUZZ_DRAWS = 2026, 240          # (tests/test_gpu_forward_turns.py runs the same draws)


def _agree(case, maps, counts_win_sidx=None):
    _, win, sidx = F.classify_piecewise(case, maps) if counts_win_sidx is None else counts_win_sidx
    img = F.rank_image(case["W"], case["H"])
    assert np.array_equal(F.piecewise_oracle(case, img), F.expected_piecewise(case, img, win, sidx)), case["name"]


# ------------------------------------------------------------------------------------------------ the model against the existing cases

@pytest.mark.parametrize("name", [n for n in PW if n != "box_65536"])      # (the launcher refuses that box before the bins kernel runs)
def test_bins_model_reproduces_the_existing_claims(name):
    c = PW[name]
    flag, most, shifts = T.bins_model(c)
    print(name, flag, most, sorted(shifts))
    over = c.get("entries", 0) > F.PW_CAP0
    assert (flag is None) == (c["flagged"] == 0 and not over), (name, flag)
    if name in ("shifts_7", "entry_2e6", "nan_vertex"):
        assert flag == "fallback"
    elif flag is not None:
        assert flag == "overflow"
    if "entries" in c:
        assert most == c["entries"]
    if name == "shifts_5":
        assert shifts == {-2, -1, 0, 1, 2}


def test_bins_model_known_answers():
    """One triangle pair that maps 1:1 into a window with 3 free columns and rows around it: both triangles under every tile their cell
    boxes touch, k = 0 only.  The same window with its left edge at 0: the upper-left triangle's cells start at x = 0, its padded bound
    at floor(0.5) - 2 = -2, which is columns 133 and 134 of k = -1, in the third tile beside the two k = 0 entries; the lower-right
    triangle's leftmost cell is x = 2 (the diagonal from (128, 0) to (0, 64) in map row 63), its bound floor(2.5) - 2 = 0: k = 0 only."""
    s, tris = F._grid(0, 0, 128, 64, 1, 1)
    c = F._p("pair", s, tris, s + [0.5, 0.5], 128, 64, (-3, -3, 135, 71))
    assert T.bins_model(c) == (None, 2, {0})
    c = F._p("pair_left", s, tris, s + [0.5, 0.5], 128, 64, (0, -3, 135, 71))
    assert T.bins_model(c) == (None, 3, {-1, 0})
    c = F._p("pair_empty", s, tris, s + [0.5, 0.5], 128, 64, (0, 0, 0, 64))
    assert T.bins_model(c) == (None, 0, set())


# ------------------------------------------------------------------------------------------------ the named cases

@pytest.mark.parametrize("name", list(NAMED))
def test_named_cases_are_what_they_are_named_for(name):
    c = NAMED[name]
    maps = F.piecewise_maps(c)
    counts, win, sidx = F.classify_piecewise(c, maps)
    print(name, c["geom"], {k: v for k, v in counts.items() if k not in ("alias_left", "alias_right")})
    _agree(c, maps, (counts, win, sidx))
    flag, most, shifts = T.bins_model(c, maps)
    assert flag is None and most <= F.PW_CAP0, (name, flag, most)
    assert shifts >= {-1, 0} and (1 in shifts or name == "shear_x_2"), (name, shifts)   # (that window is wider than its padded bound on the right)
    fwd = maps[1].astype(np.float64)
    det = T.dets(fwd)
    assert np.isfinite(fwd).all()
    if name in T.RIGID or name == "turn_45_narrow":
        assert (det < 0).all() if name in T.MIRRORED else (det > 0).all(), (name, det)
        if name == "turn_180":
            assert (fwd[:, 0] < 0).all() and (fwd[:, 3] < 0).all()
            assert counts["overwritten"] == 0 and c["geom"][2] * c["geom"][3] - counts["written"] >= 256     # ties fold a row and a column onto their neighbours' places
        if name in T.OBLIQUE or name in ("turn_45_narrow", "turn_135_mirror_x"):
            assert np.minimum(np.abs(fwd[:, 0]), np.abs(fwd[:, 1])).min() > 0.4
            assert c["geom"][2] * c["geom"][3] - counts["written"] >= 30000                                  # holes
        if name in T.AXIS_ALIGNED or name.startswith("shear"):
            assert counts["tie_x"] >= 40000 and counts["tie_y"] >= 40000, (counts["tie_x"], counts["tie_y"])
        if name == "turn_45_narrow":
            assert counts["shift"][-1] > 0 and counts["shift"][1] > 0, counts["shift"]
        if name.startswith("shear"):
            assert max(np.abs(fwd[:, 1]).max(), np.abs(fwd[:, 2]).max()) == 2.0
    if "slope" in c:
        k, v = c["slope"]
        other = fwd[:, 1 - k]
        nz = fwd[:, k][fwd[:, k] != 0]
        lo, hi = (0.0, T.SLOPE_SWITCH) if v <= 0.5 else (T.SLOPE_SWITCH, 4e-9)
        assert 0 < nz.size < fwd.shape[0] and ((np.abs(nz) > lo) & (np.abs(nz) < hi)).all(), (name, nz)
        assert (nz > 0).any() and (nz < 0).any(), (name, nz)
        assert (np.abs(other) == 1.0).all()
        if name.endswith("mirror_y"):
            assert (det < 0).all() and (fwd[:, 1] == -1.0).all()
        else:
            assert (det > 0).all()
        assert counts["tie_y" if k == 0 else "tie_x"] >= 40000
    if "guard_e" in c:
        e = c["guard_e"]
        want = 2.0 ** -e / 64
        assert want / 2 < abs(det[0]) < want * 2 and (det[0] < 0) == name.endswith("mirror_y"), (name, det[0])
        assert (det < 0).all() or (det > 0).all()
        assert counts["writers_max"] >= 64, counts["writers_max"]


def test_guard_cases_cross_the_guard_of_step_0():
    """Step (0)'s evaluation-error guard, restated for the flat triangle under every tile of the window (k = 0): the pre-image is trusted
    under every tile at the largest determinants and under none at the smallest, on both signs, and no case has |det| <= 1e-300 (a zero
    determinant is fwd_edges' collapsed_collinear)."""
    trusted = {}
    for name, c in NAMED.items():
        if "guard_e" not in c: continue
        m = F.piecewise_maps(c)[1][0].astype(np.float64)
        det = m[0] * m[3] - m[2] * m[1]
        assert abs(det) > 1e-300
        xo, yo, ow, oh = c["geom"]
        eps = 1.0 / 64
        oks = []
        for ty0 in range(0, oh, F.TILE):
            for tx0 in range(0, ow, F.TILE):
                ok = True
                for fx in (tx0 + xo - 0.5 - eps, min(tx0 + F.TILE, ow) - 1 + xo + 0.5 + eps):
                    for fy in (ty0 + yo - 0.5 - eps, min(ty0 + F.TILE, oh) - 1 + yo + 0.5 + eps):
                        a, b = m[0] * (fy - m[5]), m[1] * (fx - m[4])
                        sy = (a - b) / det
                        if not 8.0e-16 * (abs(a) + abs(b) + abs(det) * abs(sy)) < 0.5 * abs(det): ok = False
                oks.append(ok)
        trusted[name] = "all" if all(oks) else "none" if not any(oks) else "some"
    print(trusted)
    assert trusted["guard_2^-10"] == trusted["guard_2^-20"] == trusted["guard_2^-30"] == "all"
    assert trusted["guard_2^-44"] == trusted["guard_2^-50"] == trusted["guard_2^-60"] == "none"
    assert trusted["guard_2^-44_mirror_y"] == trusted["guard_2^-60_mirror_y"] == "none"
    assert trusted["guard_2^-36"] != "none" and trusted["guard_2^-36_mirror_y"] != "none"


def test_batch_frames():
    """T4: every frame agrees with the oracle, stays on the tile path by the model, and the frames differ in what they file."""
    b = T.turns_batch()
    cases = T.batch_cases(b)
    assert len(cases) == 6 and len(b["seeds"]) == 3
    filed = []
    for c in cases:
        maps = F.piecewise_maps(c)
        _agree(c, maps)
        flag, most, shifts = T.bins_model(c, maps)
        assert flag is None and most <= F.PW_CAP0, (c["name"], flag, most)
        filed.append((most, tuple(sorted(shifts))))
    det = [T.dets(F.piecewise_maps(c)[1]) for c in cases]
    assert (det[0] > 0).all() and (det[1] > 0).all() and (det[2] < 0).all() and (det[3] > 0).all()
    m0 = F.piecewise_maps(cases[4])[1][:, 0].astype(np.float64)
    assert (m0 > 0).any() and (m0 < 0).any() and np.abs(m0).max() < T.SLOPE_SWITCH
    assert 0 < abs(det[5][0]) < 1e-11
    assert len(set(filed)) >= 3, filed
    assert len({c["geom"] for c in cases}) == 6


# ------------------------------------------------------------------------------------------------ the fuzz

def test_fuzz_reaches_every_class():
    cases, dropped = T.fuzz(FUZZ_SEED, FUZZ_DRAWS)
    census = []
    for i, c in enumerate(cases):
        maps = F.piecewise_maps(c)
        cen, resolved = T.fuzz_census(c, maps)
        census.append(cen)
        if i % 10 == 0:                                                # (the whole set is compared on the GPU; a sample of it here)
            _agree(c, maps, resolved)
    n = lambda key: sum(bool(c[key]) for c in census)
    unflagged = sum(c["flag"] is None for c in census)
    print(len(cases), "usable,", dropped, "dropped,", unflagged, "unflagged,", {k: n(k) for k in ("mirrored", "oblique", "aliasing", "near_singular")},
          {f: sum(c["flag"] == f for c in census) for f in ("fallback", "overflow")}, "most entries", max(c["entries"] for c in census))
    assert len(cases) >= 220 and unflagged >= 200
    assert n("mirrored") >= 50 and n("oblique") >= 30 and n("aliasing") >= 60 and n("near_singular") >= 10
    assert len(cases) - unflagged >= 1
    assert all(c["geom"][2] * c["geom"][3] <= T.FUZZ_PIXELS_MAX for c in cases)
