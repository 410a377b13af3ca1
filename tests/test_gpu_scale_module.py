"""GPU: `-p scale` / `-p scale_mi355x` through UltraGrid's own postprocess framework (oracle/_ref/ug_vopp_harness: the reference's
src/vo_postprocess.c + lib_common registry with module/vo_pp_scale_mi355x.c, built as a build without the GL `scale` module).  Bytes against
tests/scale_gl_restatement.py (itself pinned to the module executed on llvmpipe)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import scale_gl_restatement as rs  # noqa: E402

HARNESS = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "ug_vopp_harness")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(HARNESS), reason="oracle/_ref/ug_vopp_harness not built (needs the reference tree)")]


def _run(tmp_path, cfg, codec, inter, extra, frames, env=None):
    """frames: [(w, h)]; returns (CompletedProcess, [(src, out bytes)])"""
    args, io = [HARNESS, "run", cfg, codec, inter, str(extra)], []
    for i, (w, h) in enumerate(frames):
        src = np.random.default_rng(w * 31 + h + i).integers(0, 256, rs.linesize(codec, w) * h, dtype=np.uint8)
        a, b = tmp_path / f"in{i}.raw", tmp_path / f"out{i}.raw"
        src.tofile(a)
        args += [str(w), str(h), str(a), str(b)]
        io.append((src, b))
    r = subprocess.run(args, capture_output=True, text=True, timeout=60, env=dict(os.environ, **(env or {})))
    return r, [(src, b.read_bytes() if b.exists() else b"") for src, b in io]


@pytest.mark.parametrize("name", ["scale", "scale_mi355x"])
@pytest.mark.parametrize("codec", [rs.RGBA, rs.UYVY])
@pytest.mark.parametrize("inter", ["prog", "merged"])
@pytest.mark.parametrize("extra", [0, 20])
def test_through_the_framework(tmp_path, name, codec, inter, extra):
    """req_pitch equal to the line size and different from it, both names, both codecs, merged interlace"""
    ow, oh = 150, 84
    w, h = 256, 144
    r, io = _run(tmp_path, f"{name}:{ow}:{oh}", codec, inter, extra, [(w, h)], env={"UG_PARAM": "mi355x-device=0"})
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"frame {ow} {oh} {codec} {3 if inter == 'merged' else 0} 1 0 ret=1" in r.stdout
    assert "null=0" in r.stdout  # postprocess(NULL): false
    ls = rs.linesize(codec, ow)
    got = np.frombuffer(io[0][1], np.uint8).reshape(oh, ls + extra)
    assert np.array_equal(got[:, :ls].reshape(-1), rs.scale(io[0][0], codec, w, h, ow, oh, inter == "merged"))
    assert np.all(got[:, ls:] == 0xA5)


def test_reconfigure_to_a_new_input_size(tmp_path):
    frames = [(320, 180), (320, 180), (1280, 720), (67, 33)]
    r, io = _run(tmp_path, "scale:640:360", rs.RGBA, "prog", 16, frames)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("ret=1") == len(frames)
    for (w, h), (src, out) in zip(frames, io):
        got = np.frombuffer(out, np.uint8).reshape(360, 640 * 4 + 16)[:, : 640 * 4].reshape(-1)
        assert np.array_equal(got, rs.scale(src, rs.RGBA, w, h, 640, 360)), (w, h)


def test_odd_uyvy_width_takes_whole_pairs(tmp_path):
    r, io = _run(tmp_path, "scale:41:10", rs.UYVY, "prog", 0, [(33, 9)])
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(np.frombuffer(io[0][1], np.uint8), rs.scale(io[0][0], rs.UYVY, 33, 9, 41, 10))


def test_more_than_one_tile_is_refused(tmp_path):
    """the reference writes out->tiles[1..] of a one-tile frame for such a description (tests/test_scale_gl.py::test_slip_tile_count)"""
    r, _ = _run(tmp_path, "scale:64:32", rs.RGBA, "prog", 0, [(128, 64)], env={"UG_VOPP_TILES": "2"})
    assert r.returncode == 3, r.stdout + r.stderr


def test_odd_output_height_with_merged_interlace_is_refused(tmp_path):
    r, _ = _run(tmp_path, "scale:64:33", rs.RGBA, "merged", 0, [(128, 64)])
    assert r.returncode == 3, r.stdout + r.stderr


@pytest.mark.parametrize("cfg", ["scale:0:10", "scale:10", "scale_mi355x:-4:4", "scale_mi355x:help"])
def test_bad_options_are_refused(tmp_path, cfg):
    r, _ = _run(tmp_path, cfg, rs.RGBA, "prog", 0, [(16, 16)])
    assert r.returncode == 2, r.stdout + r.stderr
