"""CPU: the R, G, B 4:2:0 / 4:2:2 layout of the encoder (create_ex with UG_JPEG_INPUT_RGB) on the host side -- the flag in the header and in the
Python binding, and the streams the GPU tests hold the encoder to (tests/jpeg_layout_bitstream.py: write_layout_jpeg over layout_coefs,
rgb="both") read back by libjpeg (Pillow) in both scan layouts."""
import io
import os
import re

import numpy as np
import pytest
from PIL import Image

from jpeg_layout_bitstream import layout_coefs, picture, write_layout_jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTORS = {420: ((2, 2), (1, 1), (1, 1)), 422: ((2, 1), (1, 1), (1, 1))}


def test_input_rgb_flag():
    from ultragrid_amd import lib as L
    assert L.JPEG_INPUT_RGB == 4
    with open(os.path.join(ROOT, "include", "ug_mi355x.h")) as f:
        header = f.read()
    assert re.search(r"^#define UG_JPEG_INPUT_RGB\s+4\s*$", header, re.M)
    assert not L.JPEG_INPUT_RGB & (L.JPEG_NONINTERLEAVED | L.JPEG_INPUT_UYVY)


def _segments(data):
    """the marker segments in front of the first SOS: [(marker, payload)]"""
    out, i = [], 2
    while data[i + 1] != 0xDA:
        n = int.from_bytes(data[i + 2:i + 4], "big")
        out.append((data[i + 1], data[i + 4:i + 2 + n]))
        i += 2 + n
    return out


@pytest.mark.parametrize("dims", [(17, 9), (9, 17), (40, 24)], ids=lambda d: f"{d[0]}x{d[1]}")
@pytest.mark.parametrize("ri", [0, 1, 4, 8])
@pytest.mark.parametrize("nonint", [False, True], ids=["interleaved", "nonint"])
@pytest.mark.parametrize("sub", [420, 422])
def test_expected_streams_read_back(po, sub, nonint, ri, dims):
    """the stream the encoder must write: Adobe transform 0, no JFIF, one DQT and two DHT (table 0), SOF0 'R' 2x2 / 2x1, 'G' / 'B' 1x1 -- and
    libjpeg decodes it to the picture, within what the quantiser and the subsampling of G and B leave"""
    w, h = dims
    x = picture(w, h, seed=ri)
    ql, qc = po.jpeg_qtable(75, 0), po.jpeg_qtable(75, 1)
    data = write_layout_jpeg(w, h, FACTORS[sub], ql, qc, layout_coefs(po, x, FACTORS[sub], ql, qc, rgb=True), restart=ri, nonint=nonint, rgb="both")
    seg = _segments(data)
    kinds = [m for m, _ in seg]
    assert kinds.count(0xDB) == 1 and kinds.count(0xC4) == 2 and 0xEE in kinds and 0xE0 not in kinds
    sof = dict(seg)[0xC0]
    hs, vs = FACTORS[sub][0]
    assert sof[5] == 3 and sof[6:] == bytes([ord("R"), hs << 4 | vs, 0, ord("G"), 0x11, 0, ord("B"), 0x11, 0])
    info, _, _ = po.jpeg_decode_planes(data)
    assert info["scans"] == (3 if nonint else 1) and info["restart"] == ri
    img = Image.open(io.BytesIO(data))
    assert img.mode == "RGB" and img.size == (w, h)
    err = np.asarray(img).astype(float) - x.astype(float)
    assert 10 * np.log10(255.0 ** 2 / np.mean(err ** 2)) > 28
