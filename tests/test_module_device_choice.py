"""CPU: every C filter module takes its device through the shared choice (module/mi355x_gpu_state.h: mi355x_gpu_open ->
mi355x_next_state_device).  A malformed --param mi355x-device list is refused at init, with the shared message, before any HIP call -- so this
needs no GPU: the four filter harnesses, one name each."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref")
# (harness, the arguments of `run` up to the frames): init comes first in every harness, the frame file is never opened
CASES = {
    "scale": ("ug_vopp_harness", ["scale_mi355x:8:8", "UYVY", "prog", "0", "8", "8", "none.raw", "none.out"]),
    "deinterlace": ("ug_deint_harness", ["deinterlace_mi355x", "-", "UYVY", "merged", "0", "none", "1", "8", "8", "none.raw"]),
    "flip": ("ug_cfilter_harness", ["flip_mi355x", "-", "UYVY", "cf", "none", "1", "8", "8", "none.raw"]),
    "crop": ("ug_compose_harness", ["crop_mi355x", "width=2", "UYVY", "pp", "1", "none", "8", "8", "none.raw"]),
}


@pytest.mark.parametrize("case", list(CASES))
def test_a_malformed_device_list_is_refused_at_init(tmp_path, case):
    harness, args = CASES[case]
    exe = os.path.join(REF, harness)
    if not os.path.exists(exe):
        pytest.skip(f"oracle/_ref/{harness} not built (no reference tree)")
    r = subprocess.run([exe, "run", *args], capture_output=True, text=True, timeout=60, cwd=tmp_path, env=dict(os.environ, UG_PARAM="mi355x-device=x"))
    out = r.stdout + r.stderr
    assert r.returncode == 2, out[-2000:]
    assert "mi355x-device=x: expected <n>[:<n>...]" in out, out[-2000:]
