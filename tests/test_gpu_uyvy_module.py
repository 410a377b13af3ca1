"""GPU: `-c uyvy` / `-c uyvy_mi355x` and the reference's DXT module names through UltraGrid's own compress framework (oracle/_ref/ug_harness:
the reference's video_compress.cpp + lib_common.cpp registry with this repository's module objects, built as a build without the reference's
GL / CUDA modules).  Bytes against tests/uyvy_glsl_restatement.py (itself pinned to the executed shader)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import uyvy_glsl_restatement as rs  # noqa: E402

ROOT = os.path.dirname(HERE)
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ug_harness")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(HARNESS), reason="oracle/_ref/ug_harness not built (needs the reference tree)")]


def _run(args):
    return subprocess.run([HARNESS] + [str(a) for a in args], capture_output=True, text=True, timeout=60)


def test_list_shows_uyvy_mi355x():
    r = _run(["list"])
    assert r.returncode == 0 and "uyvy_mi355x" in r.stdout.split()


@pytest.mark.parametrize("cfg", ["uyvy", "uyvy_mi355x", "uyvy_mi355x:dev=0:workers=2:batch=2"])
@pytest.mark.parametrize("codec", ["RGB", "RGBA"])
@pytest.mark.parametrize("mode", ["host", "dev"])
@pytest.mark.parametrize("wh", [(192, 64), (66, 9)])
def test_uyvy_through_reference_framework(tmp_path, cfg, codec, mode, wh):
    w, h = wh
    bpp = 3 if codec == "RGB" else 4
    frames = 3
    src = np.random.default_rng(w * bpp + len(cfg)).integers(0, 256, frames * w * h * bpp, dtype=np.uint8)
    raw, out = tmp_path / "in.raw", tmp_path / "out.bin"
    src.tofile(raw)
    r = _run([cfg, codec, w, h, raw, out, 1, mode, frames])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "codec=UYVY" in r.stdout
    got = out.read_bytes()
    n = w * h * bpp
    want = b"".join(rs.rgb_to_uyvy_gl(src[f * n:(f + 1) * n], w, h, bpp).tobytes() for f in range(frames))
    assert got == want


def test_uyvy_input_is_refused_with_the_reference_message(tmp_path):
    w, h = 64, 8
    raw, out = tmp_path / "in.raw", tmp_path / "out.bin"
    np.zeros(w * h * 2, np.uint8).tofile(raw)
    r = _run(["uyvy", "UYVY", w, h, raw, out])
    assert r.returncode == 3, r.stdout + r.stderr
    assert "[UYVY compress] We can transform only RGB or RGBA to UYVY." in r.stderr


@pytest.mark.parametrize("alias,fmt,codec", [("RTDXT", "DXT5", "UYVY"), ("cuda_dxt", "DXT1", "RGB"), ("rtdxt", "DXT1_YUV", "UYVY")])
def test_reference_dxt_names_give_the_dxt_bytes(tmp_path, alias, fmt, codec):
    w, h = 128, 32
    bpp = 2 if codec == "UYVY" else 3
    raw = tmp_path / "in.raw"
    np.random.default_rng(3).integers(0, 256, w * h * bpp, dtype=np.uint8).tofile(raw)
    outs = []
    for cfg in (f"dxt:{fmt}", f"{alias}:{fmt}"):
        out = tmp_path / (cfg.replace(":", "_") + ".bin")
        r = _run([cfg, codec, w, h, raw, out])
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(out.read_bytes())
    assert outs[0] == outs[1] and len(outs[0]) > 0
