"""GPU: RGB / RGBA -> UG_PF_UYVY_GL (`-c uyvy`'s conversion) against the executed shader (tests/golden/uyvy_glsl_ref.npz) and the numpy
restatement (tests/uyvy_glsl_restatement.py), packed and padded pitches, single frames and batches, and the two recorded deviations."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import uyvy_glsl_restatement as rs  # noqa: E402
from ultragrid_amd import codec, lib as L  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(HERE, "golden", "uyvy_glsl_ref.npz"))


def cases():
    for k in sorted(GOLD.files):
        if k.startswith("in_"):
            key = k[3:]
            w, h = map(int, key.split("_")[0].split("x"))
            yield key, w, h


def convert(fmt, src, w, h, src_pitch=0, dst_pitch=0):
    """one launch through ug_hip_pixfmt_convert at the given pitches; returns the packed UYVY lines"""
    bpp = 3 if fmt == L.PF_RGB else 4
    sp = src_pitch or w * bpp
    line = (w + 1) // 2 * 4
    dp = dst_pitch or line
    buf = np.zeros((h, sp), np.uint8)
    buf[:, : w * bpp] = src.reshape(h, w * bpp)
    dsrc = torch.from_numpy(buf.reshape(-1)).cuda()
    ddst = torch.full((dp * h,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = L.load().ug_hip_pixfmt_convert(fmt, L.PF_UYVY_GL, dsrc.data_ptr(), ddst.data_ptr(), w, h, src_pitch, dst_pitch, 0, 8, 16, None)
    assert rc == L.SUCCESS, L.last_error() if hasattr(L, "last_error") else rc
    out = ddst.cpu().numpy().reshape(h, dp)
    assert np.all(out[:, line:] == 0xA5)  # nothing written past the line
    return out[:, :line].reshape(-1)


def _pic(key, w, h, fmt):
    rgba = GOLD["in_" + key].reshape(h, w, 4)
    return (rgba[..., :3] if fmt == L.PF_RGB else rgba).reshape(-1)


@pytest.mark.parametrize("fmt", [L.PF_RGB, L.PF_RGBA], ids=["RGB", "RGBA"])
@pytest.mark.parametrize("pitches", [(0, 0), (1, 1), (37, 3), (64, 8)], ids=["packed", "pad1", "pad37_3", "pad64_8"])
def test_equals_the_executed_shader(fmt, pitches):
    bpp = 3 if fmt == L.PF_RGB else 4
    for key, w, h in cases():
        src = _pic(key, w, h, fmt)
        sp = w * bpp + pitches[0] if any(pitches) else 0
        dp = (w + 1) // 2 * 4 + pitches[1] if any(pitches) else 0
        got = convert(fmt, src, w, h, sp, dp)
        want = rs.rgb_to_uyvy_gl(src, w, h, bpp)
        assert np.array_equal(got, want), (key, pitches)
        if w % 2 == 0:
            gl = GOLD["gl_" + key]
            diff = np.nonzero(got != gl)[0]
            assert diff.size == 0 or key.endswith("_ties"), key  # (the ties picture: tests/test_uyvy_glsl.py pins its bytes)
            if key.endswith("_ties"):
                assert diff.size == 38 and np.all(diff % 4 % 2 == 0)


@pytest.mark.parametrize("fmt", [L.PF_RGB, L.PF_RGBA], ids=["RGB", "RGBA"])
def test_codec_helper(fmt):
    key, w, h = "64x32_rand", 64, 32
    src = _pic(key, w, h, fmt)
    got = codec.pixfmt_convert(fmt, L.PF_UYVY_GL, torch.from_numpy(src).cuda(), w, h).cpu().numpy()
    assert np.array_equal(got, GOLD["gl_" + key])


@pytest.mark.parametrize("fmt", [L.PF_RGB, L.PF_RGBA], ids=["RGB", "RGBA"])
@pytest.mark.parametrize("wh", [(1920, 1080), (3840, 2160)], ids=["1080p", "4K"])
def test_large_random_frames(fmt, wh):
    w, h = wh
    bpp = 3 if fmt == L.PF_RGB else 4
    src = np.random.default_rng(w + bpp).integers(0, 256, w * h * bpp, dtype=np.uint8)
    got = codec.pixfmt_convert(fmt, L.PF_UYVY_GL, torch.from_numpy(src).cuda(), w, h).cpu().numpy()
    assert np.array_equal(got, rs.rgb_to_uyvy_gl(src, w, h, bpp))


@pytest.mark.parametrize("fmt", [L.PF_RGB, L.PF_RGBA], ids=["RGB", "RGBA"])
@pytest.mark.parametrize("layout", ["one_launch", "odd_strides"])
def test_batch(fmt, layout):
    w, h, n = 66, 9, 5
    bpp = 3 if fmt == L.PF_RGB else 4
    line = (w + 1) // 2 * 4
    sfs, dfs = (w * bpp * h, line * h) if layout == "one_launch" else (w * bpp * h + 13, line * h + 7)
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, sfs * n, dtype=np.uint8)
    dsrc = torch.from_numpy(src).cuda()
    ddst = torch.full((dfs * n,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = L.load().ug_hip_pixfmt_convert_batch(fmt, L.PF_UYVY_GL, dsrc.data_ptr(), ddst.data_ptr(), w, h, 0, 0, 0, 8, 16, n, sfs, dfs, None)
    assert rc == L.SUCCESS
    out = ddst.cpu().numpy()
    for f in range(n):
        want = rs.rgb_to_uyvy_gl(src[f * sfs: f * sfs + w * bpp * h], w, h, bpp)
        assert np.array_equal(out[f * dfs: f * dfs + line * h], want), f
        assert np.all(out[f * dfs + line * h: (f + 1) * dfs] == 0xA5)


def test_rgb_alignment_deviation():
    """packed RGB, 3 w % 4 != 0: the stand-in's rule (packed lines) holds, and it differs from what GL produced at its 4-byte alignment"""
    seen = 0
    for key, w, h in cases():
        if "glrgb_" + key not in GOLD.files or w % 2 or h < 2:
            continue
        src = _pic(key, w, h, L.PF_RGB)
        got = convert(L.PF_RGB, src, w, h)
        assert np.array_equal(got, rs.rgb_to_uyvy_gl(src, w, h, 3)) and np.array_equal(got, GOLD["gl_" + key])
        assert not np.array_equal(got, GOLD["glrgb_" + key])
        seen += 1
    assert seen


def test_odd_width_deviation():
    """odd widths: vc_get_linesize lines whose last pair repeats the last pixel, unlike GL's w/2-wide read-back"""
    for key, w, h in cases():
        if w % 2 == 0:
            continue
        for fmt in (L.PF_RGB, L.PF_RGBA):
            src = _pic(key, w, h, fmt)
            got = convert(fmt, src, w, h)
            assert got.size == (w + 1) // 2 * 4 * h
            assert np.array_equal(got, rs.rgb_to_uyvy_gl(src, w, h, 3 if fmt == L.PF_RGB else 4))
            a = src.reshape(h, w, -1)[:, :, :3]
            last = rs.rgb_to_uyvy_gl(np.concatenate([a[:, -1:], a[:, -1:]], axis=1).reshape(-1), 2, h, 3).reshape(h, 4)
            assert np.array_equal(got.reshape(h, -1)[:, -4:], last)
            gl = GOLD["gl_" + key][: (w // 2) * 4 * h]
            assert not np.array_equal(got.reshape(h, -1)[:, : (w // 2) * 4].reshape(-1), gl)


@pytest.mark.parametrize("fmt,w,sp,dp", [(L.PF_RGBA, 66, 272, 136), (L.PF_RGB, 66, 200, 136), (L.PF_RGBA, 1366, 5472, 2736)])
def test_aligned_pitches_with_a_partial_last_quad(fmt, w, sp, dp):
    """width % 4 != 0 at pitches aligned for the wide accesses: the wide path with its pair-at-a-time tail quad"""
    h = 7
    bpp = 3 if fmt == L.PF_RGB else 4
    src = np.random.default_rng(w + sp).integers(0, 256, w * h * bpp, dtype=np.uint8)
    got = convert(fmt, src, w, h, sp, dp)
    assert np.array_equal(got, rs.rgb_to_uyvy_gl(src, w, h, bpp))
