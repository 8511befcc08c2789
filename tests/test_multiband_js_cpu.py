"""The drop-in class's mosaic(..., { blend: 'multiband' }) over a recording mock addon: what goes down to the native entries, what comes back,
and what is refused, without a GPU."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("node") is None, reason="node is missing")
def test_js_class_multiband_mosaic_over_the_recording_mock_addon():
    """tests/js/multiband_class.mjs: h.mosaic with blend 'multiband' reaches 'mosaicMultibandInverse' + family with the plain mosaic's
    windows, points and canvas, the band count (default 5), the feather, the weight and label flags and the exposure; labels and gains come
    back per destiny point set; bad `bands`, `labels` without 'multiband' and an unknown blend throw strings; the other blends keep their
    entries and arguments."""
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "multiband_class.mjs")], capture_output=True, text=True, timeout=300,
                       cwd=ROOT, env=dict(os.environ, HGWARP_ADDON=os.path.join(ROOT, "tests", "js", "mock_multiband_addon.cjs")))
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads(line[-1])
    assert res["failures"] == [] and p.returncode == 0, (res["failures"], p.stderr[-2000:])
    assert res["checks"] >= 90
