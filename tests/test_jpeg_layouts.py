"""CPU: JPEG sampling layouts beyond 4:4:4 / 4:2:2 / 4:2:0 on the host side -- the layout writer read back by libjpeg (Pillow) and by the decode
oracle, and the decoder's header parse (ug_hip_jpeg_read_info): the code it reports for every layout, and what it refuses."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

from jpeg_layout_bitstream import LAYOUTS, geometry, layout_coefs, layout_stream, picture, write_layout_jpeg

RGB_MARKS = [None, "adobe", "ids"]


def _info(data):
    from ultragrid_amd import lib as L
    w, h, s, r, ri = (C.c_int() for _ in range(5))
    rc = L.load().ug_hip_jpeg_read_info(data, len(data), C.byref(w), C.byref(h), C.byref(s), C.byref(r), C.byref(ri))
    return rc, (w.value, h.value, s.value, r.value, ri.value)


def _with_factors(po, factors, w=40, h=24, nonint=False, rgb=None):
    ql, qc = po.jpeg_qtable(75, 0), po.jpeg_qtable(75, 1)
    return write_layout_jpeg(w, h, factors, ql, qc, layout_coefs(po, picture(w, h), factors, ql, qc, rgb), restart=3, nonint=nonint, rgb=rgb)


@pytest.mark.parametrize("rgb", RGB_MARKS, ids=str)
@pytest.mark.parametrize("nonint", [False, True], ids=["interleaved", "nonint"])
@pytest.mark.parametrize("code", list(LAYOUTS))
def test_writer_reads_back_with_libjpeg(po, code, nonint, rgb):
    """the writer's streams are JPEG as libjpeg reads it: the full-resolution component is the decode oracle's plane bit for bit, the picture
    comes back within the quantiser's and the subsampling's reach"""
    w, h = 75, 38
    data = layout_stream(po, w, h, code, restart=4, nonint=nonint, rgb=rgb)
    img = Image.open(io.BytesIO(data))
    assert img.size == (w, h)
    if rgb is None:
        img.draft("YCbCr", img.size)  # the samples as coded: no colour conversion
    assert img.mode == ("RGB" if rgb else "YCbCr")
    got = np.asarray(img).astype(int)
    info, crop, _ = po.jpeg_decode_planes(data)
    assert info["scans"] == (3 if nonint else 1)
    assert np.array_equal(got[..., 0], crop[0])
    assert np.abs(got - picture(w, h).astype(int)).mean() < 4


@pytest.mark.parametrize("rgb", RGB_MARKS, ids=str)
@pytest.mark.parametrize("nonint", [False, True], ids=["interleaved", "nonint"])
@pytest.mark.parametrize("code", list(LAYOUTS))
def test_read_info_reports_the_layout(po, code, nonint, rgb):
    rc, info = _info(layout_stream(po, 33, 17, code, restart=5, nonint=nonint, rgb=rgb))
    assert rc == 0 and info == (33, 17, code, int(rgb is not None), 5)


@pytest.mark.parametrize("factors,code", [
    (((2, 2), (1, 2), (1, 2)), 422),   # 4:2:2 chroma from other factors
    (((2, 1), (2, 1), (2, 1)), 444),
    (((1, 4), (1, 2), (1, 2)), 440),
    (((1, 2), (1, 2), (1, 2)), 444),
    (((4, 1), (2, 1), (2, 1)), 422),
    (((2, 2), (2, 1), (2, 1)), 440),
], ids=str)
def test_read_info_codes_the_chroma_ratio(po, factors, code):
    """the code follows the chroma's ratio to the full resolution, not the luma's factors"""
    for nonint in (False, True):
        rc, info = _info(_with_factors(po, factors, nonint=nonint))
        assert rc == 0 and info[2] == code
        assert po.jpeg_decode_planes(_with_factors(po, factors, nonint=nonint))[0]["h"] == [f[0] for f in factors]


@pytest.mark.parametrize("factors", [
    ((3, 1), (1, 1), (1, 1)),          # fractional ratios (libjpeg refuses them)
    ((4, 1), (3, 1), (3, 1)),
    ((2, 3), (1, 2), (1, 2)),
    ((4, 2), (2, 1), (2, 1)),          # 12 blocks in an interleaved MCU (T.81 B.2.3: at most 10)
    ((2, 2), (2, 2), (2, 2)),
    ((1, 1), (2, 1), (2, 1)),          # chroma finer than the luma
    ((2, 2), (1, 1), (2, 1)),          # Cb and Cr at different ratios
    ((1, 4), (1, 1), (1, 1)),          # a vertical chroma ratio of 4: no code for it
    ((8, 1), (1, 1), (1, 1)),
], ids=str)
def test_other_layouts_are_refused(po, factors):
    from ultragrid_amd import lib as L
    ql, qc = po.jpeg_qtable(75, 0), po.jpeg_qtable(75, 1)
    _, _, _, _, grids, _ = geometry(40, 24, factors)
    coefs = [np.zeros((gw * gh, 64), np.int16) for gw, gh in grids]
    data = write_layout_jpeg(40, 24, factors, ql, qc, coefs, restart=2)
    assert _info(data)[0] == L.EUNSUPP


def test_block_limit_is_for_interleaved_scans(po):
    """one scan per component is not interleaved: the 10-block limit is not its business (T.81 B.2.3; libjpeg likewise)"""
    factors = ((4, 2), (2, 1), (2, 1))
    rc, info = _info(_with_factors(po, factors, nonint=True))
    assert rc == 0 and info[2] == 420
    assert _info(_with_factors(po, factors, nonint=False))[0] != 0


def test_old_layouts_keep_their_codes(po):
    """the codes of the layouts the decoder took before: Pillow's 4:4:4 / 4:2:2 / 4:2:0 and greyscale"""
    x = picture(48, 32)
    for sub, code in ((0, 444), (1, 422), (2, 420)):
        b = io.BytesIO()
        Image.fromarray(x).save(b, "JPEG", quality=85, subsampling=sub)
        rc, info = _info(b.getvalue())
        assert rc == 0 and info[2:4] == (code, 0)
    b = io.BytesIO()
    Image.fromarray(x[..., 0]).save(b, "JPEG", quality=85)
    assert _info(b.getvalue())[1][2] == 400
