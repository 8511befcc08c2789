"""The run form of a cached row (hg_span_runs.h) on the host: builds tests/cpp/span_runs_check.cpp -- a stand-alone program, host code only, under
AddressSanitizer and UndefinedBehaviorSanitizer -- and runs it.  The program drives the build kernel's own resolve functions lane by lane and the
window lookup against a brute-force largest-id scan."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from hgtest import span_rows as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
OVER_LIMIT_BLOCKS = 40                                # tests/test_gpu_span_runs.py: the over-limit frame's rows hold one wide span under this many blocks


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("span_runs")
    path = str(d / "span_runs_check")
    subprocess.run([HIPCC, "--cuda-host-only", "-x", "hip", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "homography.js_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "span_runs_check.cpp"), "-o", path], check=True, cwd=str(d), timeout=600)
    return path


def _run(args):
    p = subprocess.run(args, capture_output=True, text=True, timeout=600)
    out = p.stdout + p.stderr
    print(out)
    assert p.returncode == 0, out[-3000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-3000:]
    return p.stdout


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_span_runs_resolve_and_lookup(exe):
    m = re.search(r"span_runs_check: checks (\d+) failures (\d+)", _run([exe]))
    assert m
    checks, bad = (int(v) for v in m.groups())
    assert bad == 0
    assert checks >= 1000000, "the program must have walked its tables and its random rows, pixel by pixel"


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_over_limit_row_of_the_gpu_case(exe):
    """The row the GPU test builds from overlapping blocks: fewer than 64 spans, more runs than a row may hold."""
    m = re.search(r"span_runs_check: spans (\d+) runs (\d+) limit (\d+) failures (\d+)", _run([exe, "--over-limit", str(OVER_LIMIT_BLOCKS)]))
    assert m
    spans, runs, limit, bad = (int(v) for v in m.groups())
    assert bad == 0 and spans == OVER_LIMIT_BLOCKS + 1 and spans < 64 and runs == 2 * OVER_LIMIT_BLOCKS + 1 and runs > limit == 64


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
@pytest.mark.parametrize("name,runs", [("gap63", 64), ("rec64", 64), ("runs65", 65)])
def test_capacity_rows_of_the_gpu_cases(exe, name, runs):
    """The rows tests/test_gpu_span_runs_wide.py builds from 63 triangles, by position: the pieces of the oracle's winner map that bear a
    triangle, as 63 abutting or separated spans.  At 64 runs the resolve fills every slot and the lookup finds run 63; at 65 nothing is written."""
    wmap = S.cap_want(False)[name][1]
    row = wmap[int(np.argmax(S.run_counts(wmap)))]
    starts = S.run_starts(row)
    ends = np.r_[starts[1:], row.size]
    spans = [(int(a), int(b), int(row[a])) for a, b in zip(starts, ends) if row[a] >= 0]
    assert len(spans) == S.SPAN_LIMIT and len(starts) == runs
    m = re.search(r"span_runs_check: spans (\d+) runs (\d+) limit (\d+) failures (\d+)", _run([exe, "--row", str(row.size)] + [str(v) for sp in spans for v in sp]))
    assert m
    assert tuple(int(v) for v in m.groups()) == (S.SPAN_LIMIT, runs, S.RUN_LIMIT, 0)
