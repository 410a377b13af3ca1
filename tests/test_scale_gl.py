"""CPU: the pin of `-p scale` (src/vo_postprocess/scale.c) and of ug_hip_scale's place in the C ABI.

The chain: scale.c compiled unmodified and executed on llvmpipe (tools/scale_gl_run.c) -> tests/golden/scale_gl_ref.npz ->
tests/scale_gl_restatement.py, byte for byte -> the GPU kernel (tests/test_gpu_scale.py)."""
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import scale_gl_restatement as rs  # noqa: E402
from ultragrid_amd import lib  # noqa: E402

REF = "/root/reference"
GOLD_PATH = os.path.join(HERE, "golden", "scale_gl_ref.npz")
GOLD = np.load(GOLD_PATH)
_P = 0x7F0000001000  # non-NULL, never dereferenced


def cases():
    """key, codec, w, h, merged, ow, oh, req_pitch, tiles, meta"""
    for k in sorted(GOLD.files):
        if k.startswith("meta_"):
            m = [int(v) for v in GOLD[k]]
            yield (k[5:], rs.UYVY if m[0] else rs.RGBA, m[1], m[2], bool(m[3]), m[4], m[5], m[6], m[7], m)


def is_slip(codec, w, h, merged, ow, oh, tiles):
    return (codec == rs.UYVY and (w % 2 or ow % 2)) or (merged and oh % 2) or tiles > 1


def test_fixture_is_small_and_covers_the_cases():
    assert os.path.getsize(GOLD_PATH) < 512 * 1024
    seen = set()
    for _, codec, w, h, merged, ow, oh, pitch, tiles, _m in cases():
        seen.add(codec)
        if ow < w and oh < h:
            seen.add("down")
        if ow > w and oh > h:
            seen.add("up")
        if w % ow and ow % w:
            seen.add("non-integer")
        if (ow, oh) in ((1, 1), (2, 1)):
            seen.add(f"{ow}x{oh}")
        if merged:
            seen.add("merged")
        if pitch != rs.linesize(codec, ow):
            seen.add("pitch")
        if w * 4 > 2 * ow * 4 and codec == rs.RGBA:
            seen.add("down by more than 2")
    assert seen >= {"RGBA", "UYVY", "down", "up", "non-integer", "1x1", "2x1", "merged", "pitch", "down by more than 2"}, seen


# Where llvmpipe's fp32 texture coordinates and the exact rational position fall on opposite sides of a rounding tie: the only such case of the
# fixture, its differing bytes and their largest difference.  Every other case is equal bit for bit.
TIE_CASE, TIE_BYTES, TIE_MAX = "RGBA_300x20p_107x7_p0_t1", 7, 1


def test_restatement_equals_the_executed_module():
    """every case outside the slips: the written lines equal the restatement bit for bit -- except the pinned bytes of TIE_CASE -- and the
    pitch padding is untouched"""
    n = 0
    for key, codec, w, h, merged, ow, oh, pitch, tiles, _m in cases():
        if is_slip(codec, w, h, merged, ow, oh, tiles):
            continue
        ls = rs.linesize(codec, ow)
        got = GOLD["gl_" + key].reshape(oh, pitch)
        want = rs.scale(GOLD["in_" + key], codec, w, h, ow, oh, merged).reshape(oh, ls)
        diff = got[:, :ls].astype(int) - want
        if key == TIE_CASE:
            assert np.count_nonzero(diff) == TIE_BYTES and np.abs(diff).max() == TIE_MAX, (np.count_nonzero(diff), np.abs(diff).max())
        else:
            assert np.count_nonzero(diff) == 0, (key, np.count_nonzero(diff))
        assert np.all(got[:, ls:] == 0xA5), key
        n += 1
    assert n >= 16


def test_frame_flow_of_the_module():
    """postprocess returns true, postprocess(NULL) false; get_out_desc: the scaled size, tile_count 1, the input's interlacing,
    DISPLAY_PROPERTY_VIDEO_MERGED (scale.c:231-235, :331-344)"""
    for key, codec, w, h, merged, ow, oh, pitch, tiles, m in cases():
        ret, null_ret, dw, dh, inter, tile_count, mode = m[8:15]
        assert (ret, null_ret) == (1, 0), key
        assert (dw, dh, tile_count, mode) == (ow, oh, 1, 0), key
        assert inter == (3 if merged else 0), key  # INTERLACED_MERGED = 3, PROGRESSIVE = 0 (types.h)


def test_restatement_of_the_reference_reproduces_every_case():
    """the reference's texel view including its slips (tests/scale_gl_restatement.py reference_gl): every determinate byte of every case (the
    pinned bytes of TIE_CASE aside) -- what the slip tests below compare the stand-in against is what the module computes"""
    for key, codec, w, h, merged, ow, oh, pitch, tiles, _m in cases():
        src = GOLD["in_" + key][: rs.linesize(codec, w) * h]
        want, known = rs.reference_gl(src, codec, w, h, ow, oh, merged, pitch)
        diff = np.count_nonzero((want != GOLD["gl_" + key]) & known)
        assert diff == (TIE_BYTES if key == TIE_CASE else 0), (key, diff)


def _case(pred):
    return [c for c in cases() if pred(*c[1:9])]


def test_slip_odd_uyvy_width():
    """odd UYVY widths: the reference's textures are w // 2 texels wide over lines of (w + 1) // 2 pairs -- rows shear on upload (odd input
    width) and on read-back (odd output width).  The stand-in takes (w + 1) // 2 texels per line in and out, and differs"""
    odd = _case(lambda codec, w, h, merged, ow, oh, p, t: codec == rs.UYVY and (w % 2 or ow % 2))
    assert len(odd) >= 3
    for key, codec, w, h, merged, ow, oh, pitch, tiles, _m in odd:
        ls = rs.linesize(codec, ow)
        gl = GOLD["gl_" + key].reshape(oh, pitch)[:, :ls]
        mine = rs.scale(GOLD["in_" + key], codec, w, h, ow, oh, merged).reshape(oh, ls)
        assert not np.array_equal(gl, mine), key


def test_slip_odd_height_merged():
    """INTERLACED_MERGED: an odd input height drops the last line (the reference and the stand-in alike: a texel row needs two lines);
    an odd output height leaves the reference's last line unwritten -- the stand-in refuses it"""
    (key, codec, w, h, merged, ow, oh, pitch, tiles, _m), = _case(lambda codec, w, h, merged, ow, oh, p, t: merged and h % 2)
    src = GOLD["in_" + key]
    got = GOLD["gl_" + key].reshape(oh, pitch)[:, : rs.linesize(codec, ow)].reshape(-1)
    assert np.array_equal(got, rs.scale(src, codec, w, h, ow, oh, True))
    changed = src.copy()
    changed[-rs.linesize(codec, w):] ^= 0xFF  # the last line plays no part
    assert np.array_equal(rs.scale(changed, codec, w, h, ow, oh, True), rs.scale(src, codec, w, h, ow, oh, True))
    (key, codec, w, h, merged, ow, oh, pitch, tiles, _m), = _case(lambda codec, w, h, merged, ow, oh, p, t: merged and oh % 2)
    out = GOLD["gl_" + key].reshape(oh, pitch)
    assert np.all(out[-1] == 0xA5) and np.any(out[:-1] != 0xA5)
    with pytest.raises(ValueError):
        rs.scale(GOLD["in_" + key], codec, w, h, ow, oh, True)


def test_slip_tile_count():
    """tile_count > 1: the loop writes out->tiles[i] for every input tile although the output frame has one (scale.c:252-306, :341) -- the
    runner's spare slot 1 was written.  (What the stand-in does instead -- its module refuses the description at reconfigure -- is
    tests/test_gpu_scale_module.py::test_more_than_one_tile_is_refused.)"""
    multi = _case(lambda codec, w, h, merged, ow, oh, p, t: t > 1)
    assert multi
    for key, codec, w, h, merged, ow, oh, pitch, tiles, m in multi:
        assert m[15] > 0.9 * rs.linesize(codec, ow) * oh, (key, m[15])
        assert m[13] == 1  # get_out_desc still says one tile


def test_axis_rule():
    """the rule as stated: 2:1 samples between texels 2x and 2x + 1 at weight 128; 1:2 at 64 / 192; edges clamp"""
    i0, i1, w = rs.axis(8, 4)
    assert list(i0) == [0, 2, 4, 6] and list(i1) == [1, 3, 5, 7] and set(w) == {128}
    i0, i1, w = rs.axis(4, 8)
    assert list(i0) == [0, 0, 0, 1, 1, 2, 2, 3] and list(i1) == [0, 1, 1, 2, 2, 3, 3, 3] and list(w) == [192, 64, 192, 64, 192, 64, 192, 64]
    assert rs.lerp(np.int64(0), np.int64(255), 128) == 128 and rs.lerp(np.int64(255), np.int64(0), 128) == 128
    assert rs.lerp(np.int64(1), np.int64(2), 128) == 2


@pytest.mark.parametrize("codec", [rs.RGBA, rs.UYVY])
@pytest.mark.parametrize("merged", [False, True])
@pytest.mark.parametrize("geom", [(67, 34, 45, 18), (64, 32, 48, 20), (33, 3, 7, 2), (131, 10, 128, 6)])
@pytest.mark.parametrize("pad", [12, 48])
def test_restatement_takes_a_source_pitch(codec, merged, geom, pad):
    """lines `src_pitch` apart among random padding give exactly what the same lines give packed (the reference of the pitched and merged
    cases of tests/test_gpu_scale_layouts.py), and the padding plays no part"""
    w, h, ow, oh = geom
    ls = rs.linesize(codec, w)
    rng = np.random.default_rng(w + h + pad)
    packed = rng.integers(0, 256, ls * h, dtype=np.uint8)
    pitched = rng.integers(0, 256, (ls + pad) * h, dtype=np.uint8)
    pitched.reshape(h, ls + pad)[:, :ls] = packed.reshape(h, ls)
    want = rs.scale(packed, codec, w, h, ow, oh, merged)
    assert np.array_equal(rs.scale(pitched, codec, w, h, ow, oh, merged, src_pitch=ls + pad), want)
    pitched.reshape(h, ls + pad)[:, ls:] ^= 0xFF
    assert np.array_equal(rs.scale(pitched, codec, w, h, ow, oh, merged, src_pitch=ls + pad), want)
    assert not np.array_equal(rs.scale(pitched, codec, w, h, ow, oh, merged), want)  # (read as packed lines it is another picture)


def test_two_texels_to_512_yield_every_weight():
    """the shape of tests/test_gpu_scale_layouts.py::test_every_weight_pair: between texels 0 and 1, all 256 weights"""
    i0, i1, wgt = rs.axis(2, 512)
    assert set(wgt[(i0 == 0) & (i1 == 1)].tolist()) == set(range(256))


def test_positions_fit_int64_at_the_size_limit():
    """(2 x + 1) * n_in * 256 + n_out < 2^44 for a merged texture of 2 * 65536 texels; the first and last positions of the widest axes"""
    assert (2 * (2 * 65536 - 1) + 1) * (2 * 65536) * 256 + 2 * 65536 < 2 ** 44
    # the kernel's quotient (csrc/scale.hip: position): floor of the IEEE fp64 division of numerator by denominator.  Both are exact in
    # fp64 and the nearest fraction below an integer n lies 1 / den under it, further than half an ulp of n while n * den < 2^53: the
    # truncated quotient IS the floor on every axis the header accepts, the widest ones checked here
    for n_in, n_out in ((131072, 4), (4, 131072), (131072, 131071), (131071, 131072), (65536, 65535), (65535, 65536), (65536, 1), (3, 65536)):
        x = np.arange(n_out, dtype=np.int64)
        num, den = (2 * x + 1) * n_in * 256 + n_out, 2 * n_out
        assert np.array_equal((num.astype(np.float64) / np.float64(den)).astype(np.int64), num // den), (n_in, n_out)
    i0, i1, w = rs.axis(131072, 4)
    assert list(i0) == [16383, 49151, 81919, 114687] and list(i1) == [16384, 49152, 81920, 114688] and set(w) == {128}
    i0, i1, w = rs.axis(4, 131072)
    assert i0[0] == 0 and i1[0] == 0 and i0[-1] == 3 and i1[-1] == 3 and i0[65536] == 1 and i1[65536] == 2 and w[65536] == 128


@pytest.mark.skipif(not os.path.exists(os.path.join(REF, "src", "vo_postprocess", "scale.c")) or shutil.which("gcc") is None
                    or not os.path.exists("/usr/lib/x86_64-linux-gnu/dri/swrast_dri.so"), reason="needs the reference tree and Mesa llvmpipe")
def test_fixture_regenerates_from_the_reference():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "g.npz")
        subprocess.check_call([sys.executable, os.path.join(HERE, "golden", "make_scale_gl_golden.py"), out])
        new = np.load(out)
        assert sorted(new.files) == sorted(GOLD.files)
        for k in GOLD.files:
            if k.startswith("gl_"):  # bytes the module copies from its uninitialised temporary buffer are not compared
                key, (codec, w, h, merged, ow, oh, pitch) = k[3:], _geometry(k[3:])
                _, known = rs.reference_gl(GOLD["in_" + key][: rs.linesize(codec, w) * h], codec, w, h, ow, oh, merged, pitch)
                assert np.array_equal(new[k][known], GOLD[k][known]), k
            else:
                assert np.array_equal(new[k], GOLD[k]), k


def _geometry(key):
    m = [int(v) for v in GOLD["meta_" + key]]
    return rs.UYVY if m[0] else rs.RGBA, m[1], m[2], bool(m[3]), m[4], m[5], m[6]


# ---- the C ABI ----
def _desc(**kw):
    d = dict(src=_P, dst=_P, format=lib.PF_RGBA, interlaced_merged=0, src_width=96, src_height=32, dst_width=64, dst_height=20, src_pitch=0,
             dst_pitch=0, frames=1, src_frame_stride=0, dst_frame_stride=0)
    d.update(kw)
    return lib.ScaleDesc(**d)


ABSURD = [dict(src_width=w, src_height=h) for w, h in ((0, 16), (-16, 16), (16, 0), (65537, 16), (16, 65537), (2 ** 30, 2 ** 30), (65536, 65536))] + \
         [dict(dst_width=w, dst_height=h) for w, h in ((0, 16), (16, -2), (65537, 4), (65536, 65536), (49152, 65536))] + [
    dict(src=None), dict(dst=None), dict(src_pitch=96 * 4 - 4), dict(src_pitch=96 * 4 + 2), dict(dst_pitch=64 * 4 + 1), dict(dst_pitch=2 ** 31),
    dict(src_pitch=2 ** 40), dict(frames=0), dict(frames=-1), dict(frames=65536), dict(frames=2, src_frame_stride=96 * 4 * 32 - 4, dst_frame_stride=1 << 20),
    dict(frames=2, src_frame_stride=1 << 20, dst_frame_stride=64 * 4 * 20 - 4), dict(frames=2, src_frame_stride=(1 << 20) + 2, dst_frame_stride=1 << 20),
    dict(frames=3, src_frame_stride=2 ** 63, dst_frame_stride=1 << 20), dict(src=_P + 2), dict(dst=_P + 1),
    dict(interlaced_merged=1, dst_height=21), dict(interlaced_merged=1, src_height=1),
]


def test_absurd_descriptors_are_refused():
    l = lib.load()
    for kw in ABSURD:
        d = _desc(**kw)
        assert l.ug_hip_scale(C.byref(d), None) == lib.EINVAL, kw
    assert l.ug_hip_scale(None, None) == lib.EINVAL
    for fmt in (lib.PF_RGB, lib.PF_V210, lib.PF_UYVY_GL, lib.PF_NONE, 99):
        assert l.ug_hip_scale(C.byref(_desc(format=fmt)), None) == lib.EUNSUPP, fmt


def test_sane_descriptors_pass_validation_without_a_gpu():
    """the control of the test above: sane descriptors get past validation -- UG_HIP_ERUNTIME where no GPU is present.  Not run where one is
    (the pointers are fake)"""
    l = lib.load()
    n = C.c_int(0)
    if l.ug_hip_device_count(C.byref(n)) == lib.SUCCESS and n.value > 0:
        pytest.skip("a GPU is present: fake device pointers must not be launched on")
    for kw in (dict(), dict(format=lib.PF_UYVY, src_width=33, dst_width=41), dict(interlaced_merged=1, src_height=33),
               dict(src_pitch=1024, dst_pitch=512, frames=8, src_frame_stride=1024 * 32, dst_frame_stride=512 * 20),
               dict(src_width=65536, src_height=8, dst_width=1, dst_height=1)):
        assert l.ug_hip_scale(C.byref(_desc(**kw)), None) == lib.ERUNTIME, kw


def test_descriptor_binding_matches_the_header():
    import re
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "ug_mi355x.h")).read()
    body = re.search(r"struct ug_scale_desc \{(.*?)\};", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\*?(\w+)\s*[,;]", body)
    assert names == [f[0] for f in lib.ScaleDesc._fields_]
    assert "ug_hip_scale" in lib.SYMBOLS and lib.load().ug_hip_abi_version() == 5
