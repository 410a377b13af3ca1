"""CPU: the pin of `-c uyvy`'s conversion (src/video_compress/uyvy.cpp) and of UG_PF_UYVY_GL's place in the C ABI.

The chain: uyvy.cpp's shader string == dxt_compress/rgba_to_yuv422.glsl (modulo the macro name and prologue) -> glsl_ref rgba2uyvy executes
that file on llvmpipe -> tests/golden/uyvy_glsl_ref.npz -> tests/uyvy_glsl_restatement.py, byte for byte -> the GPU kernel
(tests/test_gpu_uyvy.py)."""
import ctypes as C
import os
import re
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import uyvy_glsl_restatement as rs  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
from ultragrid_amd import lib  # noqa: E402

REF = "/root/reference"
GOLD_PATH = os.path.join(HERE, "golden", "uyvy_glsl_ref.npz")
GOLD = np.load(GOLD_PATH)
_P = C.c_void_p(0x1000)


def cases():
    for k in sorted(GOLD.files):
        if k.startswith("in_"):
            key = k[3:]
            w, h = map(int, key.split("_")[0].split("x"))
            yield key, w, h


def fp32_ties(rgba, w, h):
    """mask over the UYVY bytes: U / V samples whose fp32 value times 255 lies within 2^-12 of a .5 (the engineered "ties" picture)"""
    a = rgba.reshape(h, w, 4)[..., :3]
    y1, u1, v1 = rs._yuv(a[:, 0::2])
    y2, u2, v2 = rs._yuv(a[:, 1::2])
    m = np.zeros((h, w // 2, 4), bool)
    for c, x in ((0, u1 * np.float32(0.5) + u2 * np.float32(0.5)), (2, v1 * np.float32(0.5) + v2 * np.float32(0.5))):
        t = x * np.float32(255)
        m[..., c] = np.abs(t.astype(np.float64) - np.floor(t) - 0.5) < 2.0 ** -12
    return m.reshape(-1)


def test_fixture_is_small_and_covers_the_cases():
    assert os.path.getsize(GOLD_PATH) < 256 * 1024
    keys = {k for k, _, _ in cases()}
    for need in ("2x1_rand", "4x4_rand", "6x3_rand", "64x32_rand", "1920x8_rand", "7x5_rand", "33x9_rand", "64x4_zero", "64x4_full"):
        assert need in keys
    assert any(k.endswith("_ties") for k in keys)


def test_restatement_equals_the_executed_shader():
    """every byte of every even-width case, except U / V samples of the "ties" picture within a hair of a .5, where llvmpipe's U and V
    land one code value away from the shader's statements evaluated in fp32 as written; those bytes and their count are pinned"""
    ties_off = 0
    for key, w, h in cases():
        if w % 2:
            continue
        got, gl = rs.rgb_to_uyvy_gl(GOLD["in_" + key], w, h, 4), GOLD["gl_" + key]
        diff = np.nonzero(got != gl)[0]
        if key.endswith("_ties"):
            assert np.all(fp32_ties(GOLD["in_" + key], w, h)[diff]), key
            assert np.all(np.abs(got[diff].astype(int) - gl[diff]) == 1)
            ties_off += diff.size
        else:
            assert diff.size == 0, (key, diff[:8])
    assert ties_off == 38


def test_rgb_and_padded_pitch_restatement():
    for key, w, h in cases():
        rgba = GOLD["in_" + key].reshape(h, w, 4)
        want = rs.rgb_to_uyvy_gl(rgba.reshape(-1), w, h, 4)
        assert np.array_equal(rs.rgb_to_uyvy_gl(rgba[..., :3].reshape(-1), w, h, 3), want)
        padded = np.zeros((h, 4 * w + 20), np.uint8)
        padded[:, : 4 * w] = rgba.reshape(h, -1)
        assert np.array_equal(rs.rgb_to_uyvy_gl(padded.reshape(-1), w, h, 4, pitch=4 * w + 20), want)


def test_odd_width_deviation():
    """the reference's w/2-wide framebuffer for odd w: GL's bytes are (w // 2) * 4 per line; the stand-in writes (w + 1) // 2 * 4 per line
    (vc_get_linesize) and its pairs are not GL's"""
    for key, w, h in cases():
        if w % 2 == 0:
            continue
        got = rs.rgb_to_uyvy_gl(GOLD["in_" + key], w, h, 4)
        gl = GOLD["gl_" + key]
        assert got.size == (w + 1) // 2 * 4 * h and gl.size == 2 * w * h
        assert not np.array_equal(got[: (w // 2) * 4 * h], gl[: (w // 2) * 4 * h])


def test_rgb_alignment_deviation():
    """packed RGB lines with 3 w % 4 != 0: the reference's GL reads them at a 4-byte row alignment (a skewed picture); the stand-in does not"""
    seen = 0
    for key, w, h in cases():
        if "glrgb_" + key not in GOLD.files or w % 2:
            continue
        rgb = GOLD["in_" + key].reshape(h, w, 4)[..., :3].reshape(-1)
        got, skew = rs.rgb_to_uyvy_gl(rgb, w, h, 3), GOLD["glrgb_" + key]
        line = (w + 1) // 2 * 4
        assert np.array_equal(got[:line], skew[:line])                    # line 0 is the same
        if h > 1:
            assert not np.array_equal(got, skew)
            seen += 1
    assert seen


@pytest.mark.skipif(not po.have_glsl_ref(), reason="oracle/_ref/glsl_ref or the reference tree not available")
def test_fixture_regenerates_from_the_reference():
    import subprocess
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "g.npz")
        subprocess.check_call([sys.executable, os.path.join(HERE, "golden", "make_uyvy_glsl_golden.py"), out])
        new = np.load(out)
        assert sorted(new.files) == sorted(GOLD.files)
        for k in GOLD.files:
            assert np.array_equal(new[k], GOLD[k]), k


def _shader_body(text):
    """the GLSL from `uniform sampler2D image;` to the end of main(), blank lines and trailing blanks dropped"""
    start = text.index("uniform sampler2D image;")
    lines = [ln.rstrip() for ln in text[start:].splitlines()]
    return [ln for ln in lines if ln.strip()]


@pytest.mark.skipif(not os.path.exists(os.path.join(REF, "src", "video_compress", "uyvy.cpp")), reason="reference tree not available")
def test_uyvy_cpp_shader_is_rgba_to_yuv422_glsl():
    src = open(os.path.join(REF, "src", "video_compress", "uyvy.cpp")).read()
    m = re.search(r"fp_display_rgba_to_yuv422_legacy\[\]\s*=\s*((?:\s*\"(?:[^\"\\]|\\.)*\")+)", src)
    assert m, "shader string not found"
    parts = re.findall(r"\"((?:[^\"\\]|\\.)*)\"", m.group(1))
    shader = "".join(parts).encode().decode("unicode_escape")
    glsl = open(os.path.join(REF, "dxt_compress", "rgba_to_yuv422.glsl")).read()
    # the file's prologue (#if legacy ... #endif) picks the legacy names; the string uses them directly (or under LEGACY)
    assert _shader_body(shader.replace("LEGACY", "legacy")) == _shader_body(glsl)


def test_abi_uyvy_gl_is_an_output_of_rgb_and_rgba_only():
    l = lib.load()
    assert lib.PF_UYVY_GL == 17 and lib.PF_UYVY_GL not in lib.PF_NAMES.values()
    others = [v for v in range(0, 18) if v not in (lib.PF_RGB, lib.PF_RGBA)]
    for fin in others:
        assert l.ug_hip_pixfmt_supported(fin, lib.PF_UYVY_GL) == 0, fin
        assert l.ug_hip_pixfmt_convert(fin, lib.PF_UYVY_GL, _P, _P, 64, 4, 0, 0, 0, 8, 16, None) == lib.EUNSUPP, fin
        assert l.ug_hip_pixfmt_convert_batch(fin, lib.PF_UYVY_GL, _P, _P, 64, 4, 0, 0, 0, 8, 16, 2, 1 << 20, 1 << 20, None) == lib.EUNSUPP, fin
    for fout in range(0, 18):
        assert l.ug_hip_pixfmt_supported(lib.PF_UYVY_GL, fout) == 0, fout
        assert l.ug_hip_pixfmt_convert(lib.PF_UYVY_GL, fout, _P, _P, 64, 4, 256, 256, 0, 8, 16, None) in (lib.EUNSUPP, lib.EINVAL), fout
    for fin in (lib.PF_RGB, lib.PF_RGBA):
        assert l.ug_hip_pixfmt_supported(fin, lib.PF_UYVY_GL) == 1
    assert l.ug_hip_linesize(lib.PF_UYVY_GL, 7) == 16 and l.ug_hip_linesize(lib.PF_UYVY_GL, 3840) == 7680


def test_abi_uyvy_gl_is_never_a_best_decoder():
    l = lib.load()
    out = C.c_int(-1)
    for fin in (lib.PF_RGB, lib.PF_RGBA):
        cand = (C.c_int * 2)(lib.PF_UYVY_GL, 0)
        assert l.ug_hip_pixfmt_best(fin, cand, C.byref(out)) == lib.EUNSUPP
        cand = (C.c_int * 3)(lib.PF_UYVY_GL, lib.PF_UYVY, 0)
        assert l.ug_hip_pixfmt_best(fin, cand, C.byref(out)) == lib.SUCCESS and out.value == lib.PF_UYVY
