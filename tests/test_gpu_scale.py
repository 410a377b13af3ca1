"""GPU: ug_hip_scale (`-p scale`'s resampler) against the module executed on llvmpipe (tests/golden/scale_gl_ref.npz) and the numpy
restatement (tests/scale_gl_restatement.py) over a size grid: widths that are no multiple of 4, pitched output, batches, merged interlace."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import scale_gl_restatement as rs  # noqa: E402
from ultragrid_amd import codec, lib as L  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(HERE, "golden", "scale_gl_ref.npz"))
PF = {rs.RGBA: L.PF_RGBA, rs.UYVY: L.PF_UYVY}


def run(fmt, src, w, h, ow, oh, merged=False, src_pitch=0, dst_pitch=0, frames=1, sstride=0, dstride=0):
    """one ug_hip_scale call; src: numpy bytes (frames back to back at sstride); returns the dst buffer (filled with 0xA5 first)"""
    dp = dst_pitch or rs.linesize(fmt, ow)
    dstride = dstride or dp * oh
    dsrc = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    ddst = torch.full(((frames - 1) * dstride + dp * oh,), 0xA5, dtype=torch.uint8, device="cuda")
    d = L.ScaleDesc(dsrc.data_ptr(), ddst.data_ptr(), PF[fmt], int(merged), w, h, ow, oh, src_pitch, dst_pitch, frames, sstride, dstride)
    rc = L.load().ug_hip_scale(C.byref(d), None)
    assert rc == L.SUCCESS, (rc, L.last_error())
    torch.cuda.synchronize()
    return ddst.cpu().numpy()


TIE_CASE, TIE_BYTES, TIE_MAX = "RGBA_300x20p_107x7_p0_t1", 7, 1  # as tests/test_scale_gl.py pins them (fp32 coordinates vs exact positions)


def test_equals_the_executed_module():
    """every fixture case outside the reference's slips, at the case's req_pitch: bit for bit (TIE_CASE: its pinned bytes), padding untouched"""
    n = 0
    for k in sorted(GOLD.files):
        if not k.startswith("meta_"):
            continue
        key, m = k[5:], [int(v) for v in GOLD[k]]
        fmt = rs.UYVY if m[0] else rs.RGBA
        w, h, merged, ow, oh, pitch, tiles = m[1], m[2], bool(m[3]), m[4], m[5], m[6], m[7]
        if (fmt == rs.UYVY and (w % 2 or ow % 2)) or (merged and oh % 2) or tiles > 1:
            continue
        got = run(fmt, GOLD["in_" + key], w, h, ow, oh, merged, dst_pitch=pitch)
        diff = got.astype(int) - GOLD["gl_" + key]
        if key == TIE_CASE:
            assert np.count_nonzero(diff) == TIE_BYTES and np.abs(diff).max() == TIE_MAX
        else:
            assert np.count_nonzero(diff) == 0, (key, np.count_nonzero(diff))
        ls = rs.linesize(fmt, ow)
        assert np.array_equal(got.reshape(oh, pitch)[:, :ls].reshape(-1), rs.scale(GOLD["in_" + key], fmt, w, h, ow, oh, merged)), key
        n += 1
    assert n >= 16


GRID = [(64, 32, 32, 16), (67, 31, 45, 17), (1, 1, 7, 3), (5, 3, 1, 1), (5, 3, 2, 1), (1366, 9, 1921, 5), (3840, 6, 1918, 4), (129, 65, 130, 66),
        (300, 200, 1003, 701), (37, 91, 613, 11)]


@pytest.mark.parametrize("fmt", [rs.RGBA, rs.UYVY])
@pytest.mark.parametrize("geom", GRID, ids=[f"{a}x{b}to{c}x{d}" for a, b, c, d in GRID])
@pytest.mark.parametrize("pitch", [(0, 0), (12, 20), (4, 16)], ids=["packed", "pad12_20", "pad4_16"])
def test_equals_the_restatement(fmt, geom, pitch):
    w, h, ow, oh = geom
    sls, dls = rs.linesize(fmt, w), rs.linesize(fmt, ow)
    sp, dp = (sls + pitch[0], dls + pitch[1]) if any(pitch) else (0, 0)
    rng = np.random.default_rng(w * 7 + ow)
    src = rng.integers(0, 256, (sp or sls) * h, dtype=np.uint8)
    got = run(fmt, src, w, h, ow, oh, src_pitch=sp, dst_pitch=dp).reshape(oh, dp or dls)
    want = rs.scale(src, fmt, w, h, ow, oh, src_pitch=sp).reshape(oh, dls)
    assert np.array_equal(got[:, :dls], want), np.count_nonzero(got[:, :dls] != want)
    assert np.all(got[:, dls:] == 0xA5)


@pytest.mark.parametrize("fmt", [rs.RGBA, rs.UYVY])
@pytest.mark.parametrize("geom", [(64, 32, 48, 20), (67, 33, 130, 62), (1920, 10, 1280, 6), (33, 2, 7, 2)])
def test_merged_interlace(fmt, geom):
    w, h, ow, oh = geom
    src = np.random.default_rng(w + h).integers(0, 256, rs.linesize(fmt, w) * h, dtype=np.uint8)
    got = run(fmt, src, w, h, ow, oh, merged=True)
    assert np.array_equal(got, rs.scale(src, fmt, w, h, ow, oh, merged=True))


@pytest.mark.parametrize("fmt", [rs.RGBA, rs.UYVY])
@pytest.mark.parametrize("layout", ["packed", "strided", "aligned16"])
def test_batch(fmt, layout):
    """aligned16: every output line and frame 16-B aligned (dst pitch and frame stride multiples of 16): the dwordx4 store path"""
    w, h, ow, oh, n = 131, 37, (128 if layout == "aligned16" else 77), 51, 6
    sls, dls = rs.linesize(fmt, w), rs.linesize(fmt, ow)
    sstride, dstride = {"packed": (sls * h, dls * oh), "strided": (sls * h + 52, dls * oh + 36), "aligned16": (sls * h + 12, dls * oh + 48)}[layout]
    if layout == "aligned16":
        assert dls % 16 == 0 and dstride % 16 == 0
    src = np.random.default_rng(11).integers(0, 256, sstride * n, dtype=np.uint8)
    got = run(fmt, src, w, h, ow, oh, frames=n, sstride=sstride, dstride=dstride)
    for f in range(n):
        want = rs.scale(src[f * sstride: f * sstride + sls * h], fmt, w, h, ow, oh)
        assert np.array_equal(got[f * dstride: f * dstride + dls * oh], want), f
        assert np.all(got[f * dstride + dls * oh: (f + 1) * dstride] == 0xA5)


@pytest.mark.parametrize("geom", [(3840, 2160, 1920, 1080), (1920, 1080, 3840, 2160)], ids=["4Kto1080p", "1080pto4K"])
def test_large_frames_via_the_codec_helper(geom):
    w, h, ow, oh = geom
    src = np.random.default_rng(3).integers(0, 256, 4 * w * h, dtype=np.uint8)
    got = codec.scale(L.PF_RGBA, torch.from_numpy(src).cuda(), w, h, ow, oh).cpu().numpy()
    assert np.array_equal(got, rs.scale(src, rs.RGBA, w, h, ow, oh))


def test_odd_uyvy_width_rule():
    """the stand-in's rule for odd UYVY widths ((w + 1) // 2 texels per line), not the reference's sheared rows"""
    w, h, ow, oh = 33, 9, 41, 10
    src = np.random.default_rng(1).integers(0, 256, rs.linesize(rs.UYVY, w) * h, dtype=np.uint8)
    got = run(rs.UYVY, src, w, h, ow, oh)
    assert np.array_equal(got, rs.scale(src, rs.UYVY, w, h, ow, oh))
    assert not np.array_equal(got[: (ow // 2) * 4 * oh], rs.reference_gl(src, rs.UYVY, w, h, ow, oh, False, rs.linesize(rs.UYVY, ow))[0][: (ow // 2) * 4 * oh])
