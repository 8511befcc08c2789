"""What tests/test_gpu_span_runs_wide.py relies on, proved on the oracle alone: the runs of a row are the changes of the winner along it
(hgtest.span_rows), and a 4-row group can be held in run form iff none of its rows has more than 64 of them.  No GPU."""
import numpy as np
import pytest

from hgtest import span_rows as S


@pytest.mark.parametrize("long_form", [False, True], ids=["one_fma", "long_form"])
@pytest.mark.parametrize("width", S.WIDTHS)
def test_wide_placements(width, long_form):
    """Every width shows its features in windows 4 and up -- a trip behind the first, whether a trip takes one window or four -- and every row
    of every frame fits a row block: all groups are cacheable."""
    S.check_wide_placement(width, long_form)
    P = S.wide_parts()
    windows = (width + 255) // 256
    assert {1152: 5, 1153: 5, 1300: 6, 2052: 9, 40: 1}[width] == windows
    for name, (dp, geom) in S.wide_frames(width, long_form).items():
        assert geom == (0, 0, width, S.wide_height(width)) and geom[3] % S.GROUP != 0 and geom[2] * geom[3] > S.COL_W + 2
        assert S.row_cover(dp, P.tris, geom).max() <= 56, name          # the planner keeps 4-row groups up to 56 triangles a row
        assert S.cacheable_groups(S.wide_want(width, long_form)[name][1]).all(), name


def test_wide_widths_pin_what_they_are_meant_to():
    assert 1152 == 1024 + 128 and 1152 % 4 == 0                          # the last window's second pair of pieces is dead
    assert 1153 % 4 != 0 and 1153 - 1024 - 128 == 1                      # one live pixel in the third piece; no 16-byte zero stores
    assert 1300 - 1280 == 20 and 1300 % 4 == 0                           # a ragged window of 20 pixels ends the second trip
    assert (2052 + 255) // 256 == 9 and 2052 - 2048 == 4 and 2052 % 4 == 0      # three trips of four windows
    assert 40 < 64
    for width in (1152, 1300, 2052):                                     # an empty window of a later trip, where the zero stores are 16 bytes wide
        m = S.wide_want(width, False)["islands"][1]
        assert (m[:, 1024:1280] < 0).all()


@pytest.mark.parametrize("long_form", [False, True], ids=["one_fma", "long_form"])
def test_mixed_set_shape(long_form):
    dps, geoms, offs, total, want = S.mixed_set(long_form)
    assert [g[2:] for g in geoms] == [(2052, 10), (1300, 3), (40, 22), (0, 22)]
    assert geoms[0][:2] == (5, 3)                                        # a window origin of its own
    assert geoms[1][2] % 4 == 0 and offs[1] % 16 == 4 and (geoms[1][2] * 4) % 16 == 0      # every row of the frame starts off a 16-byte boundary
    assert all(o % 4 == 0 for o in offs)
    ends = [o + g[2] * g[3] * 4 for o, g in zip(offs, geoms)]
    assert all(ends[k] <= offs[k + 1] for k in range(3)) and ends[-1] <= total
    assert sum(S.group_count(g[3]) for g in geoms if g[2] > 0) == 3 + 1 + 6
    for w, g in zip(want[:3], geoms):
        assert w.shape == (g[3], g[2], 4) and w.any()
    # (a window origin in x moves the reference's flat fill indices: the frame is not the picture of the same placement at (0, 0))
    assert S.cacheable_groups(S.wide_want(2052, long_form, (5, 3), 10)["shift+0"][1]).all()


@pytest.mark.parametrize("long_form", [False, True], ids=["one_fma", "long_form"])
def test_capacity_rows(long_form):
    """63 spans and 64 runs with run 63 a gap, the same with run 63 a record, 63 spans and 65 runs, 64 spans."""
    S.check_capacities(long_form)
    want = S.cap_want(long_form)
    ok = {k: S.cacheable_groups(v[1]) for k, v in want.items()}
    assert ok["low"].all() and ok["gap63"].all() and ok["rec64"].all() and not ok["runs65"].any() and not ok["spans64"].any()
    P = S.cap_parts()
    for name, dp in S.cap_frames(long_form).items():
        # no span crosses the row end (it would spill a second span of its triangle into the next row): the last column is a gap or the tail cell's
        assert (want[name][1][:, -1] < 2).all(), name
        assert S.row_cover(dp, P.tris, S.CAP_WIN).max() == want[name][2], name
    assert S.row_cover(S.cap_frames(long_form)["low"], P.tris, S.CAP_WIN).max() in range(31, 57)      # 4-row groups, and a buffer sized for 64 runs a row


def test_random_sets_meet_the_quarter_cap():
    total, bad = S.check_random_sets()
    print("groups", total, "not cacheable", bad)
    assert total >= 3 * len(S.SEEDS) and 4 * bad <= total
    assert len(S.SEEDS) == 12 and len(set(S.SEEDS)) == 12
    for seed in S.SEEDS:                                                 # the same set from the same seed
        a, b = S.random_set(seed), S.random_set(seed)
        assert np.array_equal(a["tris"], b["tris"]) and all(np.array_equal(x[0], y[0]) and x[1] == y[1] for x, y in zip(a["frames"], b["frames"]))
        assert 2 <= len(a["frames"]) <= 3 and all(o % 4 == 0 for o in a["offs"])
