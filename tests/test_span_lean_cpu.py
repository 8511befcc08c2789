"""The lean span form of the self-span prologues (span_cells_lean, hg_math.h) against span_cells, on the host: builds
tests/cpp/span_lean_check.cpp -- a stand-alone program, host code only, under UndefinedBehaviorSanitizer -- and runs it."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_lean_span_form_equals_span_cells(tmp_path):
    exe = str(tmp_path / "span_lean_check")
    subprocess.run([HIPCC, "--cuda-host-only", "-x", "hip", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                    "-Xarch_host", "-fsanitize=undefined", "-I", os.path.join(ROOT, "homography.js_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "span_lean_check.cpp"), "-o", exe], check=True, cwd=str(tmp_path), timeout=600)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "runtime error" not in p.stdout + p.stderr, (p.stdout + p.stderr)[-3000:]
    m = re.search(r"rows (\d+) nonempty (\d+) .* mismatches (\d+)", p.stdout)
    assert m, p.stdout
    rows, nonempty, bad = (int(v) for v in m.groups())
    assert bad == 0
    assert rows >= 4_000_000 and nonempty * 10 >= rows, "the comparison must not pass vacuously"
