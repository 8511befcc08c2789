"""The division-free block decode of the span cache's use kernel (hg_span_start.h) on the host: builds tests/cpp/span_start_check.cpp -- a
stand-alone program, host code only, under AddressSanitizer and UndefinedBehaviorSanitizer -- and runs it.  The program walks every block id of
its grids (fixed bands, rotating bands, sub-bands 2, 3 and 8; 1, 3, 64 and 513 frames; group counts that do and do not divide) and compares the
decode with frame_group's divisions."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_span_start_decode_equals_frame_group(tmp_path):
    exe = str(tmp_path / "span_start_check")
    subprocess.run([HIPCC, "--cuda-host-only", "-x", "hip", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "homography.js_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "span_start_check.cpp"), "-o", exe], check=True, cwd=str(tmp_path), timeout=600)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    out = p.stdout + p.stderr
    print(out)
    assert p.returncode == 0, out[-3000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-3000:]
    m = re.search(r"span_start_check: checks (\d+) failures (\d+)", p.stdout)
    assert m, p.stdout
    checks, bad = (int(v) for v in m.groups())
    assert bad == 0
    assert checks >= 10000000, "the program must have walked its grids block by block"
