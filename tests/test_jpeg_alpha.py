"""CPU: four-component (R, G, B, alpha) JPEG streams on the host side -- the reference writer read back by libjpeg (Pillow), and the decoder's
header parse (ug_hip_jpeg_read_info) on such streams: what it reports and what it refuses."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

from jpeg_alpha_bitstream import coefs4444, rgba_picture, write_jpeg4444


def _info(data):
    from ultragrid_amd import lib as L
    w, h, s, r, ri = (C.c_int() for _ in range(5))
    rc = L.load().ug_hip_jpeg_read_info(data, len(data), C.byref(w), C.byref(h), C.byref(s), C.byref(r), C.byref(ri))
    return rc, (w.value, h.value, s.value, r.value, ri.value)


def _pillow_cmyk(x, **kw):
    b = io.BytesIO()
    Image.fromarray(x, "CMYK").save(b, "JPEG", quality=90, **kw)
    return b.getvalue()


@pytest.mark.parametrize("nonint", [False, True])
@pytest.mark.parametrize("ri", [0, 3])
def test_writer_reads_back_with_libjpeg(po, nonint, ri):
    """the reference writer's streams are what libjpeg takes for an Adobe four-component picture (inverted CMYK to Pillow): 255 - Pillow's
    planes come within the quantiser's reach of the picture"""
    w, h = 45, 30
    x = rgba_picture(w, h)
    ql, qc = po.jpeg_qtable(90, 0), po.jpeg_qtable(90, 1)
    data = write_jpeg4444(w, h, ql, qc, coefs4444(po, x, ql), restart=ri, nonint=nonint)
    img = Image.open(io.BytesIO(data))
    assert img.mode == "CMYK" and img.size == (w, h)
    back = 255 - np.asarray(img).astype(int)
    assert np.abs(back - x).mean() < 4


def test_read_info_reports_4444():
    x = rgba_picture(64, 40)
    for kw in ({}, {"restart_marker_blocks": 2}, {"optimize": True}):
        rc, (w, h, sub, rgb, _) = _info(_pillow_cmyk(x, **kw))
        assert rc == 0 and (w, h, sub, rgb) == (64, 40, 4444, 1)


def test_read_info_of_the_writer(po):
    ql = po.jpeg_qtable(75, 0)
    x = rgba_picture(24, 16)
    for nonint in (False, True):
        rc, info = _info(write_jpeg4444(24, 16, ql, po.jpeg_qtable(75, 1), coefs4444(po, x, ql), restart=5, nonint=nonint))
        assert rc == 0 and info == (24, 16, 4444, 1, 5)


def test_four_components_refused_where_not_rgba():
    """subsampled four-component streams and Y'CbCr-K (Adobe transform 1 / 2) are not R, G, B, A: refused, not misread"""
    from ultragrid_amd import lib as L
    x = rgba_picture(32, 32)
    d = bytearray(_pillow_cmyk(x))
    sof = d.index(b"\xff\xc0")
    assert d[sof + 9] == 4
    sub = bytearray(d)
    sub[sof + 11] = 0x22  # component 0 sampled 2x2
    assert _info(bytes(sub))[0] == L.EUNSUPP
    adobe = d.index(b"Adobe")
    for t in (1, 2):
        ycck = bytearray(d)
        ycck[adobe + 11] = t
        assert _info(bytes(ycck))[0] == L.EUNSUPP
    ycck = bytearray(d)
    ycck[adobe + 11] = 0
    assert _info(bytes(ycck))[0] == 0
