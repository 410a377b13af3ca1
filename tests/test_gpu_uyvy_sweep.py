"""GPU: RGB / RGBA -> UG_PF_UYVY_GL (csrc/uyvy_gl.hip, csrc/rgba_to_yuv422_device.h) against the numpy restatement of the shader
(tests/uyvy_glsl_restatement.py), byte for byte, where the fixture and the random frames of tests/test_gpu_uyvy.py do not reach:
  - all 2^24 colours as the first and as the second pixel of a pair (the fixed-point form and its guard against the shader's fp32 form),
    through the wide RGB kernel, the pair-at-a-time kernel and, for four slices, the wide RGBA kernel;
  - more than 65535 lines in one launch (the line loop's second trip): single pictures 65536 lines tall and a packed batch;
  - the instantiations with two and four quads per lane at widths that leave a ragged workgroup and a partial last quad.
Every destination lies between canaries and is compared whole (tests/pitch_layout.py); source padding is random."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pitch_layout as pl  # noqa: E402
import uyvy_glsl_restatement as rs  # noqa: E402
from ultragrid_amd import lib as L  # noqa: E402

pytestmark = pytest.mark.gpu
FMT = {3: L.PF_RGB, 4: L.PF_RGBA}


def up(n, a):
    return (n + a - 1) // a * a


def place(rgb, w, h, bpp, sp, so, seed):
    """(h, w, 3) colours as lines of bpp bytes per pixel, `sp` apart, `so` bytes into a 256-byte aligned buffer; alpha, padding, the bytes in
    front and SLACK bytes behind are random"""
    buf = pl.aligned_bytes(so + sp * h + pl.SLACK, rng=np.random.default_rng(seed))
    lines = np.lib.stride_tricks.as_strided(buf[so:], (h, w, bpp), (sp, bpp, 1))
    lines[:, :, :3] = rgb
    return buf


def convert(bpp, src, so, w, h, sp, dp, do=0, frames=1, sstride=0, dstride=0):
    """one ug_hip_pixfmt_convert[_batch] call with explicit pitches -> (the whole destination buffer, front)"""
    front = pl.GUARD + do
    dst = pl.aligned_bytes(front + (frames - 1) * dstride + dp * h + pl.GUARD, fill=pl.FILL)
    dsrc, ddst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    assert dsrc.data_ptr() % 256 == 0 and ddst.data_ptr() % 256 == 0
    lib = L.load()
    if frames == 1:
        rc = lib.ug_hip_pixfmt_convert(FMT[bpp], L.PF_UYVY_GL, dsrc.data_ptr() + so, ddst.data_ptr() + front, w, h, sp, dp, 0, 8, 16, None)
    else:
        rc = lib.ug_hip_pixfmt_convert_batch(FMT[bpp], L.PF_UYVY_GL, dsrc.data_ptr() + so, ddst.data_ptr() + front, w, h, sp, dp, 0, 8, 16,
                                             frames, sstride, dstride, None)
    assert rc == L.SUCCESS, (rc, L.last_error())
    torch.cuda.synchronize()
    return ddst.cpu().numpy(), front


def expect(wants, w, h, dp, do, dstride):
    """the buffer convert() must leave: each frame's restated lines in place, FILL everywhere else"""
    line = (w + 1) // 2 * 4
    front = pl.GUARD + do
    buf = pl.aligned_bytes(front + (len(wants) - 1) * dstride + dp * h + pl.GUARD, fill=pl.FILL)
    for f, want in enumerate(wants):
        at = front + f * dstride
        np.lib.stride_tricks.as_strided(buf[at:], (h, line), (dp, 1))[:] = want.reshape(h, line)
    return buf


def check(bpp, rgb, want, w, h, sp, dp, so=0, do=0, seed=0):
    """one picture: (h, w, 3) colours, `want` its restated UYVY bytes"""
    got, front = convert(bpp, place(rgb, w, h, bpp, sp, so, seed), so, w, h, sp, dp, do)
    found = pl.compare(got, expect([want], w, h, dp, do, 0), h, dp, (w + 1) // 2 * 4, front)
    assert not found, (bpp, w, h, sp, dp, so, do, found)


def differing_pairs(bpp, rgb, want, w, h, sp, dp, so):
    """-> the (first colour, second colour, got, want) of up to 8 pairs whose word differs from the restatement"""
    got, front = convert(bpp, place(rgb, w, h, bpp, sp, so, 1), so, w, h, sp, dp)
    line = (w + 1) // 2 * 4
    assert np.all(got[:front] == pl.FILL) and np.all(got[front + dp * h:] == pl.FILL)
    g = got[front: front + dp * h].reshape(h, dp)
    assert np.all(g[:, line:] == pl.FILL)
    bad = np.flatnonzero((g[:, :line].reshape(-1, 4) != want.reshape(-1, 4)).any(axis=1))
    px = rgb.reshape(-1, 2, 3)
    return bad.size, [(px[k, 0].tolist(), px[k, 1].tolist(), g[:, :line].reshape(-1, 4)[k].tolist(), want.reshape(-1, 4)[k].tolist()) for k in bad[:8]]


# ------------------------------------------------ the complete colour sweep ------------------------------------------------
SLICE_W, SLICE_H = 2048, 1024      # 2^20 pairs
MULT = 0x9E3779B1                  # odd: c -> c * MULT mod 2^24 is a bijection
RGBA_SLICES = (0, 5, 10, 15)


def slice_colours(s):
    """pairs (c, c * MULT mod 2^24) for the 2^20 colours c of slice s, c = R | G << 8 | B << 16 -> (SLICE_H, SLICE_W, 3)"""
    c = np.arange(s << 20, (s + 1) << 20, dtype=np.uint64)
    both = np.stack([c, (c * MULT) & 0xFFFFFF], axis=1).reshape(-1)
    return np.stack([both & 255, (both >> 8) & 255, both >> 16], axis=1).astype(np.uint8).reshape(SLICE_H, SLICE_W, 3)


def test_the_second_pixel_runs_through_every_colour_too():
    assert MULT % 2 == 1  # a unit modulo 2^24
    seen = np.zeros(1 << 24, bool)
    seen[(np.arange(1 << 24, dtype=np.uint64) * MULT) & 0xFFFFFF] = True
    assert seen.all()
    rgb = slice_colours(3)
    assert rgb[0, 0].tolist() == [0, 0, 0x30] and rgb[0, 2].tolist() == [1, 0, 0x30]
    c1 = (3 << 20) + 1
    assert rgb[0, 3].tolist() == [(c1 * MULT) & 255, (c1 * MULT >> 8) & 255, (c1 * MULT >> 16) & 255]


@pytest.mark.parametrize("s", range(16))
def test_every_colour_pair_slice(s):
    """slice s of the 2^24 pairs: the wide RGB kernel (aligned base and pitch), the pair-at-a-time kernel (source base + 1) and, for four
    slices, the wide RGBA kernel give the shader's bytes.  A pair that differs means the guard budget of rgba_to_yuv422_device.h is wrong."""
    w, h = SLICE_W, SLICE_H
    rgb = slice_colours(s)
    want = rs.rgb_to_uyvy_gl(rgb.reshape(-1), w, h, 3)
    tiers = [("RGB wide", 3, 3 * w, 0), ("RGB pair at a time", 3, 3 * w, 1)] + ([("RGBA wide", 4, 4 * w, 0)] if s in RGBA_SLICES else [])
    for name, bpp, sp, so in tiers:
        n, pairs = differing_pairs(bpp, rgb, want, w, h, sp, 2 * w, so)
        assert n == 0, (name, s, n, pairs)


# ------------------------------------------------ the line loop's second trip ------------------------------------------------
def random_rgb(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("bpp", [3, 4], ids=["RGB", "RGBA"])
@pytest.mark.parametrize("w", [2, 6])
@pytest.mark.parametrize("pitches", ["packed", "aligned"])
def test_65536_lines_in_one_call(bpp, w, pitches):
    """line 65535 is the second trip of a workgroup through the line loop; packed these widths take the pair-at-a-time kernel, at aligned
    pitches the wide one"""
    h = 65536
    line = (w + 1) // 2 * 4
    sp, dp = (w * bpp, line) if pitches == "packed" else (up(w * bpp, 16 if bpp == 4 else 4) + (16 if bpp == 4 else 4), up(line, 8) + 8)
    rgb = random_rgb(w, h, w + bpp)
    check(bpp, rgb, rs.rgb_to_uyvy_gl(rgb.reshape(-1), w, h, 3), w, h, sp, dp, seed=w)


@pytest.mark.parametrize("bpp", [3, 4], ids=["RGB", "RGBA"])
@pytest.mark.parametrize("gap", [(0, 0), (16, 8)], ids=["one_launch", "frame_by_frame"])
def test_batch_of_69632_lines(bpp, gap):
    """4 x 4096 x 17 frames: one picture apart -- a single launch of 69632 lines -- and further apart: frame by frame"""
    w, h, n = 4, 4096, 17
    sp, dp = w * bpp, 8
    sstride, dstride = sp * h + gap[0], dp * h + gap[1]
    rgb = random_rgb(w, h * n, 17 + bpp).reshape(n, h, w, 3)
    src = pl.aligned_bytes(n * sstride + pl.SLACK, rng=np.random.default_rng(3))
    for f in range(n):
        np.lib.stride_tricks.as_strided(src[f * sstride:], (h, w, bpp), (sp, bpp, 1))[:, :, :3] = rgb[f]
    wants = [rs.rgb_to_uyvy_gl(rgb[f].reshape(-1), w, h, 3) for f in range(n)]
    got, front = convert(bpp, src, 0, w, h, sp, dp, 0, n, sstride, dstride)
    found = pl.compare_frames(got, expect(wants, w, h, dp, 0, dstride), n, dstride, h, dp, 8, front)
    assert not found, found


# ------------------------------------------------ two and four quads per lane ------------------------------------------------
@pytest.mark.parametrize("bpp", [3, 4], ids=["RGB", "RGBA"])
@pytest.mark.parametrize("w", [1537, 1538, 1541, 3073, 3074, 3077, 4097])
@pytest.mark.parametrize("so", [0, 1], ids=["aligned", "src_base_1"])
def test_wide_instantiations_with_ragged_ends(bpp, w, so):
    """lines of at least 384 / 768 quads (two / four quads per lane) whose last workgroup is ragged and whose last quad is partial, at pitches
    aligned for the wide kernel, and the same lines one byte off on the source (pair at a time)"""
    h = 3
    assert (w + 3) // 4 >= (768 if w > 3000 else 384) and w % 4
    sp = up(w * bpp, 16) + 16 if bpp == 4 else up(w * bpp, 4) + 4
    dp = up((w + 1) // 2 * 4, 8) + 8
    rgb = random_rgb(w, h, w)
    check(bpp, rgb, rs.rgb_to_uyvy_gl(rgb.reshape(-1), w, h, 3), w, h, sp, dp, so=so, seed=w + so)
