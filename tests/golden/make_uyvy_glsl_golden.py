#!/usr/bin/env python3
"""Generate tests/golden/uyvy_glsl_ref.npz: the conversion of `-c uyvy` (src/video_compress/uyvy.cpp) as the reference's own shader
computes it.  uyvy.cpp's fragment shader has the text of dxt_compress/rgba_to_yuv422.glsl (tests/test_uyvy_glsl.py checks that), and
oracle/_ref/glsl_ref's `rgba2uyvy` mode executes that file on Mesa llvmpipe over a w/2 x h viewport with GL_NEAREST / CLAMP_TO_EDGE
texturing and imageWidth = w, as uyvy.cpp does.

Run where the reference tree and glsl_ref exist:
    make -C oracle ref && python tests/golden/make_uyvy_glsl_golden.py [out.npz]

Arrays, per case `<w>x<h>_<kind>`:
  in_<case>       RGBA input, h * w * 4 bytes (the RGB cases take bytes R, G, B of each pixel)
  gl_<case>       glsl_ref's output for it: 2 * w * h bytes, lines of (w // 2) * 4 bytes (the read-back of a w/2 wide framebuffer)
  glrgb_<case>    (where 3 w % 4 != 0) glsl_ref's output on the texture GL builds from the same picture handed over as packed RGB lines at
                  GL's default unpack alignment of 4 (uyvy.cpp never sets GL_UNPACK_ALIGNMENT): every line after the first skewed
"""
import os
import subprocess
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import pyoracle as po  # noqa: E402
import uyvy_glsl_restatement as rs  # noqa: E402

REFDIR = "/root/reference"
RANDOM_SIZES = [(2, 1), (4, 4), (6, 3), (64, 32), (1920, 8), (7, 5), (33, 9)]


def run_glsl(rgba: np.ndarray, w: int, h: int) -> np.ndarray:
    with tempfile.TemporaryDirectory() as d:
        a, b = os.path.join(d, "in.rgba"), os.path.join(d, "out.uyvy")
        np.ascontiguousarray(rgba, np.uint8).tofile(a)
        subprocess.check_call([po.GLSL_REF, REFDIR, "rgba2uyvy", "rgba", str(w), str(h), a, b])
        return np.fromfile(b, np.uint8)


def tie_pixels() -> np.ndarray:
    """RGB colours for which Y', Cb or Cr times 255 is an exact .5 in the shader's fp32 arithmetic (a pair of two equal pixels keeps the
    chroma value: mix(a, a, 0.5) == a exactly), the cases the float -> unorm8 tie rule decides"""
    c = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([c & 255, (c >> 8) & 255, c >> 16], axis=-1).astype(np.uint8)
    found = []
    for val in rs._yuv(rgb):
        x = val * np.float32(255)
        idx = np.nonzero(x - np.floor(x) == np.float32(0.5))[0]
        found.append(idx[np.random.default_rng(len(found)).permutation(idx.size)[:256]])
    return rgb[np.concatenate(found)]


def cases():
    for w, h in RANDOM_SIZES:
        rng = np.random.default_rng(zlib.crc32(f"uyvy{w}x{h}".encode()))
        yield w, h, "rand", rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    ties = tie_pixels()
    w = 64
    h = (2 * len(ties) + w - 1) // w
    pix = np.repeat(ties, 2, axis=0)  # each tie colour as both pixels of a pair
    pix = np.concatenate([pix, np.zeros((w * h - len(pix), 3), np.uint8)])
    alpha = np.random.default_rng(7).integers(0, 256, (w * h, 1), dtype=np.uint8)
    yield w, h, "ties", np.concatenate([pix, alpha], axis=-1).reshape(h, w, 4)
    for v, name in ((0, "zero"), (255, "full")):
        yield 64, 4, name, np.full((4, 64, 4), v, np.uint8)


def main():
    if not po.have_glsl_ref():
        sys.exit("needs oracle/_ref/glsl_ref and the reference tree")
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "uyvy_glsl_ref.npz")
    arrays = {}
    for w, h, kind, rgba in cases():
        key = f"{w}x{h}_{kind}"
        arrays["in_" + key] = rgba.reshape(-1)
        arrays["gl_" + key] = run_glsl(rgba, w, h)
        if (3 * w) % 4:
            rgb = rgba[..., :3].reshape(-1)
            arrays["glrgb_" + key] = run_glsl(rs.gl_skewed_rgba(rgb, w, h), w, h)
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
