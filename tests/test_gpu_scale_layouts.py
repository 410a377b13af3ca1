"""GPU: ug_hip_scale on the layouts, weights and sizes that move its addressing (csrc/scale.hip), against the numpy restatement
(tests/scale_gl_restatement.py), byte for byte:
  - INTERLACED_MERGED pictures with a source pitch (the second half of a texel row starts one PITCH, not one line size, after the first), a
    destination pitch, batches, and both store paths (dwordx4 / word by word);
  - the same layout combinations without merging that no other test makes: source pitch in a batch, an aligned pitch on a base that is not
    16-byte aligned, a batch whose destination stride is no multiple of 16;
  - every one of the 256 weights of a lerp, on both axes, between the extreme byte values;
  - positions at the largest sizes the header accepts (65536 texels; merged: a texture 131072 texels wide), on pictures one or two lines thin.
Every destination lies between canaries and is compared whole (tests/pitch_layout.py); source padding, gaps and slack are random bytes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pitch_layout as pl  # noqa: E402
import scale_gl_restatement as rs  # noqa: E402
from ultragrid_amd import lib as L  # noqa: E402

pytestmark = pytest.mark.gpu
PF = {rs.RGBA: L.PF_RGBA, rs.UYVY: L.PF_UYVY}
FMTS = [rs.RGBA, rs.UYVY]


def r16(n):
    return (n + 15) // 16 * 16


def call(fmt, src, w, h, ow, oh, merged=False, sp=0, dp=0, do=0, frames=1, sstride=0, dstride=0):
    """one ug_hip_scale call.  src: host bytes at a 256-byte aligned address; the destination starts GUARD + do bytes into a 256-byte aligned
    buffer of FILL that ends GUARD bytes behind the last line.  -> (the whole destination buffer, front)"""
    pitch = dp or rs.linesize(fmt, ow)
    front = pl.GUARD + do
    dst = pl.aligned_bytes(front + (frames - 1) * dstride + pitch * oh + pl.GUARD, fill=pl.FILL)
    dsrc, ddst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    assert dsrc.data_ptr() % 256 == 0 and ddst.data_ptr() % 256 == 0
    d = L.ScaleDesc(dsrc.data_ptr(), ddst.data_ptr() + front, PF[fmt], int(merged), w, h, ow, oh, sp, dp, frames, sstride, dstride)
    rc = L.load().ug_hip_scale(C.byref(d), None)
    assert rc == L.SUCCESS, (rc, L.last_error())
    torch.cuda.synchronize()
    return ddst.cpu().numpy(), front


def expect(wants, fmt, ow, oh, dp, do, dstride):
    """the destination buffer call() must leave: the restated lines of every frame in place, FILL everywhere else"""
    dls = rs.linesize(fmt, ow)
    pitch = dp or dls
    front = pl.GUARD + do
    buf = pl.aligned_bytes(front + (len(wants) - 1) * dstride + pitch * oh + pl.GUARD, fill=pl.FILL)
    for f, want in enumerate(wants):
        rows = want.reshape(oh, dls)
        for y in range(oh):
            at = front + f * dstride + y * pitch
            buf[at: at + dls] = rows[y]
    return buf


def lines_of(got, front, fmt, ow, oh, dp, frames=1, dstride=0):
    dls = rs.linesize(fmt, ow)
    pitch = dp or dls
    return np.stack([got[front + f * dstride + y * pitch: front + f * dstride + y * pitch + dls] for f in range(frames) for y in range(oh)])


def check(fmt, src, w, h, ow, oh, merged, sp=0, dp=0, do=0, frames=1, sstride=0, dstride=0):
    """the call against the restatement of every frame, the whole buffer; -> (restated frames, the lines the kernel wrote)"""
    sls, dls = rs.linesize(fmt, w), rs.linesize(fmt, ow)
    wants = [rs.scale(src[f * sstride: f * sstride + (sp or sls) * h], fmt, w, h, ow, oh, merged=merged, src_pitch=sp) for f in range(frames)]
    got, front = call(fmt, src, w, h, ow, oh, merged, sp, dp, do, frames, sstride, dstride)
    want = expect(wants, fmt, ow, oh, dp, do, dstride)
    found = pl.compare_frames(got, want, frames, dstride, oh, dp or dls, dls, front)
    assert not found, found
    assert np.array_equal(got, want)
    return wants, lines_of(got, front, fmt, ow, oh, dp, frames, dstride)


def both_store_paths(fmt, src, w, h, ow, oh, merged, sp, frames, sstride):
    """the same pictures through the dwordx4 stores (16-byte aligned base, pitch and stride) and word by word (the same pitch on a base + 4)
    -> the lines of either run"""
    dp = r16(rs.linesize(fmt, ow)) + 16
    dstride = r16(dp * oh) + 32 if frames > 1 else 0
    out = []
    for do in (0, 4):
        got, front = call(fmt, src, w, h, ow, oh, merged, sp, dp, do, frames, sstride, dstride)
        out.append(lines_of(got, front, fmt, ow, oh, dp, frames, dstride))
    return out


def make_src(size, seed):
    return pl.aligned_bytes(size + pl.SLACK, rng=np.random.default_rng(seed))


# ------------------------------------------------ 1. merged pictures in every layout ------------------------------------------------
# (33, 3): the odd last line is dropped; the two that enlarge have output texels BETWEEN the last texel of the even line and the first of the
# odd line (the texture filters across that seam, as the reference's does)
MERGED_GEOMS = [(67, 34, 45, 18), (64, 32, 48, 20), (33, 3, 7, 2), (131, 10, 128, 6), (45, 18, 67, 34), (7, 4, 33, 6)]


def crosses_the_seam(fmt, w, ow):
    tpl = rs.texels_per_line(fmt, w)
    i0, i1, wgt = rs.axis(2 * tpl, 2 * rs.texels_per_line(fmt, ow))
    return bool(np.any((i0 == tpl - 1) & (i1 == tpl) & (wgt > 0)))
MERGED_LAYOUTS = ["packed", "src_pad12", "src_pad16_32", "dst_pad20", "dst_pad16_wide", "dst_pad16_base4", "batch_gaps", "batch_16"]


def merged_layout(name, sls, dls, h, oh):
    """-> dict(sp, dp, do, frames, sstride, dstride)"""
    a = dict(sp=0, dp=0, do=0, frames=1, sstride=0, dstride=0)
    if name == "src_pad12":
        a.update(sp=sls + 12)
    elif name == "src_pad16_32":
        a.update(sp=r16(sls) + 32)
    elif name == "dst_pad20":
        a.update(dp=dls + 20)
    elif name == "dst_pad16_wide":
        a.update(dp=r16(dls) + 16)
    elif name == "dst_pad16_base4":
        a.update(dp=r16(dls) + 16, do=4)
    elif name == "batch_gaps":
        a.update(frames=3, sstride=sls * h + 52, dstride=dls * oh + 36)
    elif name == "batch_16":
        a.update(frames=3, sstride=r16(sls * h) + 16, dstride=r16(dls * oh) + 32)
    else:
        assert name == "packed"
    return a


def misread_as_packed(src, fmt, w, h, ow, oh, sp):
    """the restated output if the second half of a texel row were taken one LINE SIZE behind the first -- the even line's padding, then the
    odd line's start -- instead of one pitch behind it"""
    tpl = rs.texels_per_line(fmt, w)
    rows = np.stack([src[2 * j * sp: 2 * j * sp + 8 * tpl] for j in range(h // 2)]).reshape(h // 2, 2 * tpl, 4)
    return rs.resample(rows, 2 * rs.texels_per_line(fmt, ow), oh // 2).reshape(-1)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("geom", MERGED_GEOMS, ids=lambda g: "{}x{}to{}x{}".format(*g))
@pytest.mark.parametrize("layout", MERGED_LAYOUTS)
def test_merged_in_every_layout(fmt, geom, layout):
    w, h, ow, oh = geom
    sls, dls = rs.linesize(fmt, w), rs.linesize(fmt, ow)
    a = merged_layout(layout, sls, dls, h, oh)
    assert crosses_the_seam(fmt, w, ow) == (ow > w)
    src = make_src((a["frames"] - 1) * a["sstride"] + (a["sp"] or sls) * h, seed=w * 31 + h + len(layout))
    wants, got = check(fmt, src, w, h, ow, oh, True, **a)
    wide, narrow = both_store_paths(fmt, src, w, h, ow, oh, True, a["sp"], a["frames"], a["sstride"])
    assert np.array_equal(wide, narrow) and np.array_equal(wide, got)
    if a["sp"]:  # the case tells a pitch from a line size: reading on past the even line's end gives other bytes
        assert not np.array_equal(misread_as_packed(src, fmt, w, h, ow, oh, a["sp"]), wants[0])
    else:        # (packed lines: the two readings are one and the same)
        assert np.array_equal(misread_as_packed(src, fmt, w, h, ow, oh, sls), wants[0])


# ------------------------------------------------ 2. the same layout gaps, not merged ------------------------------------------------
PLAIN_GEOMS = [(67, 31, 45, 17), (64, 32, 48, 20)]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("geom", PLAIN_GEOMS, ids=lambda g: "{}x{}to{}x{}".format(*g))
@pytest.mark.parametrize("layout", ["src_pitch_in_a_batch", "aligned_pitch_base4", "batch_stride_4_not_16"])
def test_layout_combinations_not_merged(fmt, geom, layout):
    w, h, ow, oh = geom
    sls, dls = rs.linesize(fmt, w), rs.linesize(fmt, ow)
    if layout == "src_pitch_in_a_batch":
        sp = sls + 12
        a = dict(sp=sp, dp=0, do=0, frames=3, sstride=sp * h + 52, dstride=dls * oh + 36)
    elif layout == "aligned_pitch_base4":
        a = dict(sp=0, dp=r16(dls) + 16, do=4, frames=1, sstride=0, dstride=0)
    else:  # base, pitch and source all aligned; only the destination's frame stride is not: the whole batch stores word by word
        dp = r16(dls) + 16
        a = dict(sp=0, dp=dp, do=0, frames=2, sstride=r16(sls * h), dstride=dp * oh + 4)
        assert a["dstride"] % 4 == 0 and a["dstride"] % 16 != 0 and dp % 16 == 0
    src = make_src((a["frames"] - 1) * a["sstride"] + (a["sp"] or sls) * h, seed=w + 3 * oh + len(layout))
    _, got = check(fmt, src, w, h, ow, oh, False, **a)
    wide, narrow = both_store_paths(fmt, src, w, h, ow, oh, False, a["sp"], a["frames"], a["sstride"])
    assert np.array_equal(wide, narrow) and np.array_equal(wide, got)


# ------------------------------------------------ 3. every weight pair ------------------------------------------------
EXTREMES = np.array([0, 1, 127, 128, 254, 255], np.uint8)
WEIGHT_SOURCES = {
    # texels t00 t01 / t10 t11: every channel has a low value on one side and a high one on the other of the horizontal and the vertical lerp
    "lo_hi": [0, 255, 1, 254, 255, 0, 254, 1, 254, 1, 255, 0, 1, 254, 0, 255],
    "mid": [127, 128, 0, 255, 128, 127, 255, 0, 1, 254, 128, 127, 254, 1, 127, 128],
    "drawn": EXTREMES[np.random.default_rng(6).integers(0, 6, 16)].tolist(),
}


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", sorted(WEIGHT_SOURCES))
def test_every_weight_pair(fmt, name):
    """2 x 2 texels -> 512 x 512 texels: all 256 x 256 pairs of weights between the two columns and the two rows, 1 MB compared whole"""
    w, ow = (2, 512) if fmt == rs.RGBA else (4, 1024)
    src = make_src(16, seed=1)
    src[:16] = WEIGHT_SOURCES[name]
    assert set(src[:16].tolist()) <= set(EXTREMES.tolist())
    check(fmt, src, w, 2, ow, 512, False)


# ------------------------------------------------ 4. positions at the size limit ------------------------------------------------
LIMIT = 65536
AXIS_PAIRS = [(LIMIT, 1), (1, LIMIT), (LIMIT, LIMIT - 1), (LIMIT - 1, LIMIT), (LIMIT, 3), (3, LIMIT)]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("n", AXIS_PAIRS, ids=lambda n: f"{n[0]}to{n[1]}")
def test_widths_at_the_limit(fmt, n):
    w, ow = n
    src = make_src(rs.linesize(fmt, w), seed=w % 977 + ow % 13)
    check(fmt, src, w, 1, ow, 1, False)


@pytest.mark.parametrize("n", AXIS_PAIRS, ids=lambda n: f"{n[0]}to{n[1]}")
def test_heights_at_the_limit(n):
    h, oh = n
    src = make_src(4 * h, seed=h % 977 + oh % 13 + 1)
    check(rs.RGBA, src, 1, h, 1, oh, False)


@pytest.mark.parametrize("n", [(LIMIT, 2), (2, LIMIT)], ids=lambda n: f"{n[0]}to{n[1]}")
def test_merged_widths_at_the_limit(n):
    """two lines of 65536 texels side by side: a texture 131072 texels wide, the largest numerators position() sees"""
    w, ow = n
    src = make_src(4 * w * 2, seed=w % 977 + 5)
    _, got = check(rs.RGBA, src, w, 2, ow, 2, True)
    wide, narrow = both_store_paths(rs.RGBA, src, w, 2, ow, 2, True, 0, 1, 0)
    assert np.array_equal(wide, narrow) and np.array_equal(wide, got)
