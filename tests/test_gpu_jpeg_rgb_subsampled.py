"""GPU: the R, G, B 4:2:0 / 4:2:2 encoder (create_ex with UG_JPEG_INPUT_RGB, RGB input) -- byte for byte against the layout writer over the test
helper's planes (tests/jpeg_layout_bitstream.py: write_layout_jpeg + layout_coefs, rgb="both") in both scan layouts and on every unfused coder path,
batches, a pitched source, the capacity check, max_size, the round trip through the product decoder, the refusals, and `-c jpeg:RGB:subsampling=42x`
through the reference framework.  The samples (the box downsampling) are unpinned towards libgpujpeg, like the FDCT."""
import ctypes as C
import io
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

from jpeg_layout_bitstream import geometry, layout_coefs, picture, write_layout_jpeg
from jpeg_layout_restatement import expected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ug_harness")
DEC_HARNESS = os.path.join(ROOT, "oracle", "_ref", "ug_dec_harness")
needs_harness = pytest.mark.skipif(not (os.path.exists(HARNESS) and os.path.exists(DEC_HARNESS)), reason="oracle/_ref/ug_harness not built")

FACTORS = {420: ((2, 2), (1, 1), (1, 1)), 422: ((2, 1), (1, 1), (1, 1))}


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _want(po, x, sub, q, ri, nonint):
    h, w, _ = x.shape
    ql, qc = po.jpeg_qtable(q, 0), po.jpeg_qtable(q, 1)
    return write_layout_jpeg(w, h, FACTORS[sub], ql, qc, layout_coefs(po, x, FACTORS[sub], ql, qc, rgb=True), restart=ri, nonint=nonint, rgb="both")


def _encoder(hip, w, h, q, ri, sub, nonint, cs=0):
    from ultragrid_amd import lib as L
    return hip.JpegEncoder(w, h, q, ri, subsampling=sub, internal_cs=cs, flags=L.JPEG_INPUT_RGB | (L.JPEG_NONINTERLEAVED if nonint else 0))


def _encode(hip, x, q, ri, sub, nonint, cs=0):
    import torch
    from ultragrid_amd import lib as L
    h, w, _ = x.shape
    enc = _encoder(hip, w, h, q, ri, sub, nonint, cs)
    data = enc.encode(torch.from_numpy(np.ascontiguousarray(x).ravel()).cuda(), L.PF_RGB)
    enc.close()
    return data


# (sub, nonint, restart, q, (w, h)): every value at least once; 1366x768 and 1920x1080 in a few combinations (the writer is Python)
CASES = [
    (420, False, 4, 75, (16, 16)), (422, True, 1, 95, (16, 16)),
    (420, True, 1, 95, (17, 9)), (422, False, 0, 95, (17, 9)),
    (422, True, 8, 75, (9, 17)), (420, True, 0, 75, (9, 17)),
    (420, True, 0, 75, (96, 64)), (422, True, 4, 95, (96, 64)), (420, False, 300, 75, (96, 64)),
    (420, True, 300, 75, (722, 486)), (422, False, 2000, 75, (722, 486)), (420, False, 8, 95, (722, 486)), (422, True, 0, 75, (722, 486)),
    (422, True, 2000, 95, (1366, 768)), (420, True, 4, 75, (1366, 768)),
    (420, True, 8, 75, (1920, 1080)), (422, False, 1, 75, (1920, 1080)), (420, True, 2000, 75, (1920, 1080)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("sub,nonint,ri,q,dims", CASES, ids=[f"{s}-{'nonint' if n else 'int'}-ri{r}-q{q}-{d[0]}x{d[1]}" for s, n, r, q, d in CASES])
def test_gpu_bytes_equal_the_writer(hip, po, sub, nonint, ri, q, dims):
    w, h = dims
    x = picture(w, h, seed=sub + ri)
    data = _encode(hip, x, q, ri, sub, nonint, cs=ri % 2)  # UG_JPEG_CS_RGB = UG_JPEG_CS_ASIS for RGB input
    assert data == _want(po, x, sub, q, ri, nonint)


@pytest.mark.gpu
@pytest.mark.parametrize("nonint", [False, True], ids=["interleaved", "nonint"])
@pytest.mark.parametrize("sub", [420, 422])
def test_gpu_4k_header_and_coefficients(hip, po, sub, nonint):
    """4K: the header bytes up to the first SOS, and the coefficients the oracle's entropy decoder reads back == layout_coefs"""
    w, h, q, ri = 3840, 2160, 85, 4
    x = picture(w, h, seed=3)
    data = _encode(hip, x, q, ri, sub, nonint)
    ql, qc = po.jpeg_qtable(q, 0), po.jpeg_qtable(q, 1)
    grids = geometry(w, h, FACTORS[sub])[4]
    zeros = write_layout_jpeg(w, h, FACTORS[sub], ql, qc, [np.zeros((gw * gh, 64), np.int16) for gw, gh in grids], restart=ri, nonint=nonint, rgb="both")
    head = zeros[: zeros.index(b"\xff\xda") + (10 if nonint else 14)]
    assert data[: len(head)] == head
    info, got = po.jpeg_decode_coeffs(data)
    assert info["scans"] == (3 if nonint else 1) and info["h"] == [FACTORS[sub][0][0], 1, 1] and info["v"] == [FACTORS[sub][0][1], 1, 1]
    want = layout_coefs(po, x, FACTORS[sub], ql, qc, rgb=True)
    for c in range(3):
        assert np.array_equal(got[c], want[c]), f"component {c}"  # (4K: W and H are multiples of 16, the R scan covers its whole grid)


@pytest.mark.gpu
@pytest.mark.parametrize("env", ["UG_JPEG_WAVE_KERNEL", "UG_JPEG_LOOKBACK"])
@pytest.mark.parametrize("nonint", [False, True], ids=["interleaved", "nonint"])
@pytest.mark.parametrize("sub", [420, 422])
def test_gpu_coder_paths(hip, po, sub, nonint, env, monkeypatch):
    """UG_JPEG_WAVE_KERNEL=1 (the wave-per-segment coder + compaction) and UG_JPEG_LOOKBACK=0 (the two-launch placement for one-frame calls): read
    when an encoder is made"""
    monkeypatch.setenv(env, "1" if env == "UG_JPEG_WAVE_KERNEL" else "0")
    w, h, q = 150, 70, 80
    x = picture(w, h, seed=5)
    for ri in (4, 300, 0):
        assert _encode(hip, x, q, ri, sub, nonint) == _want(po, x, sub, q, ri, nonint), ri


_NORI_OFF = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np, torch
from oracle import pyoracle as po
from ultragrid_amd import codec as hip, lib as L
from jpeg_layout_bitstream import layout_coefs, picture, write_layout_jpeg
F = {420: ((2, 2), (1, 1), (1, 1)), 422: ((2, 1), (1, 1), (1, 1))}
bad = []
for sub in (420, 422):
    for nonint in (False, True):
        for ri, (w, h) in ((0, (150, 70)), (2000, (722, 486)), (300, (1366, 768))):
            x = picture(w, h, seed=ri)
            ql, qc = po.jpeg_qtable(80, 0), po.jpeg_qtable(80, 1)
            e = hip.JpegEncoder(w, h, 80, ri, subsampling=sub, flags=L.JPEG_INPUT_RGB | (L.JPEG_NONINTERLEAVED if nonint else 0))
            d = e.encode(torch.from_numpy(x.ravel()).cuda(), L.PF_RGB)
            e.close()
            if d != write_layout_jpeg(w, h, F[sub], ql, qc, layout_coefs(po, x, F[sub], ql, qc, rgb=True), restart=ri, nonint=nonint, rgb="both"):
                bad.append((sub, nonint, ri))
print("BAD", bad)
sys.exit(1 if bad else 0)
"""


@pytest.mark.gpu
def test_gpu_coder_without_the_parallel_forms(hip, po):
    """UG_JPEG_NORI=0 (read once per process: a process of its own): restart 0 and long intervals on the wave-per-segment coder"""
    code = _NORI_OFF % {"root": ROOT, "tests": os.path.dirname(os.path.abspath(__file__))}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env={**os.environ, "UG_JPEG_NORI": "0"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("nonint", [False, True], ids=["interleaved", "nonint"])
@pytest.mark.parametrize("sub", [420, 422])
def test_gpu_encode_batch(hip, po, sub, nonint):
    """batches of 2, 5 and 16 frames == the single-frame calls, restart 0 included"""
    import torch
    from ultragrid_amd import lib as L
    w, h, q = 200, 90, 80
    frames = [picture(w, h, seed=s) for s in range(16)]
    for ri in (4, 0):
        enc = _encoder(hip, w, h, q, ri, sub, nonint)
        one = [enc.encode(torch.from_numpy(f.ravel()).cuda(), L.PF_RGB) for f in frames]
        assert len(set(one)) == 16
        for n in (2, 5, 16):
            got = enc.encode_batch(torch.stack([torch.from_numpy(f.ravel()) for f in frames[:n]]).cuda(), L.PF_RGB)
            assert got == one[:n], (ri, n)
        enc.close()
        assert one[0] == _want(po, frames[0], sub, q, ri, nonint)


@pytest.mark.gpu
@pytest.mark.parametrize("nonint", [False, True], ids=["interleaved", "nonint"])
@pytest.mark.parametrize("sub", [420, 422])
def test_gpu_pitched_source(hip, po, sub, nonint):
    """src_pitch > 3 w (and not a multiple of 4): the same stream as the packed frame"""
    import torch
    from ultragrid_amd import lib as L
    w, h, q, ri = 131, 45, 85, 2
    x = picture(w, h, seed=9)
    for pitch in (3 * w + 13, 3 * w + 64):
        buf = np.full((h, pitch), 0xEE, np.uint8)
        buf[:, : 3 * w] = x.reshape(h, 3 * w)
        dev = torch.from_numpy(buf.ravel()).cuda()
        enc = _encoder(hip, w, h, q, ri, sub, nonint)
        out = torch.empty(enc.max_size, dtype=torch.uint8, device="cuda")
        n = C.c_size_t(0)
        assert L.load().ug_hip_jpeg_encoder_encode(enc._h, L.PF_RGB, dev.data_ptr(), pitch, out.data_ptr(), enc.max_size, C.byref(n), _stream()) == 0
        enc.close()
        assert bytes(out[: n.value].cpu().numpy()) == _want(po, x, sub, q, ri, nonint), pitch


@pytest.mark.gpu
@pytest.mark.parametrize("nonint", [False, True], ids=["interleaved", "nonint"])
@pytest.mark.parametrize("sub", [420, 422])
def test_gpu_capacity_and_max_size(hip, po, sub, nonint):
    """an undersized out_capacity: EINVAL, out_len = the size it needs, nothing written past the capacity; noise at q=100 fits max_size"""
    import torch
    from ultragrid_amd import lib as L
    l = L.load()
    w, h = 250, 130
    x = picture(w, h, seed=11)
    enc = _encoder(hip, w, h, 85, 4, sub, nonint)
    src = torch.from_numpy(x.ravel()).cuda()
    need = len(enc.encode(src, L.PF_RGB))
    short = need // 3
    buf = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    m = C.c_size_t(0)
    assert l.ug_hip_jpeg_encoder_encode(enc._h, L.PF_RGB, src.data_ptr(), 0, buf.data_ptr(), short, C.byref(m), _stream()) == L.EINVAL
    torch.cuda.synchronize()
    enc.close()
    assert m.value == need and bool((buf[short:] == 0xA5).all())
    for ri in (1, 0, 300):
        noise = np.random.default_rng(ri).integers(0, 256, (h, w, 3), dtype=np.uint8)
        enc = _encoder(hip, w, h, 100, ri, sub, nonint)
        data = enc.encode(torch.from_numpy(noise.ravel()).cuda(), L.PF_RGB)
        assert len(data) <= enc.max_size
        enc.close()
        assert data == _want(po, noise, sub, 100, ri, nonint)


@pytest.mark.gpu
@pytest.mark.parametrize("nonint", [False, True], ids=["interleaved", "nonint"])
@pytest.mark.parametrize("sub", [420, 422])
@pytest.mark.parametrize("dims", [(17, 9), (150, 70), (722, 486)], ids=lambda d: f"{d[0]}x{d[1]}")
def test_gpu_round_trip(hip, po, sub, nonint, dims):
    """the product decoder reads the encoder's streams: RGB / RGBA / UYVY == the replication rule over the stream's planes, read_info says R, G, B at
    the encoder's sampling, Pillow reads them"""
    from ultragrid_amd import lib as L
    w, h = dims
    x = picture(w, h, seed=13)
    data = _encode(hip, x, 80, 3, sub, nonint)
    info = hip.jpeg_read_info(data)
    assert info == dict(width=w, height=h, subsampling=sub, is_rgb=True, restart=3)
    _, crop, _ = po.jpeg_decode_planes(data)
    rr = (2, 2 if sub == 420 else 1)  # G and B: a sample per 2 x 2 / 2 x 1 pixels
    dec = hip.JpegDecoder()
    for out in ("RGB", "RGBA", "UYVY"):
        got = dec.decode(data, getattr(L, "PF_" + out)).cpu().numpy()
        assert np.array_equal(got, expected(po, crop, [(1, 1), rr, rr], w, h, True, out).ravel()), out
    dec.close()
    img = Image.open(io.BytesIO(data))
    assert img.mode == "RGB" and img.size == (w, h)
    err = np.asarray(img).astype(float) - x.astype(float)
    assert 10 * np.log10(255.0 ** 2 / np.mean(err ** 2)) > 28


@pytest.mark.gpu
def test_gpu_refusals(hip, po):
    """the acceptance matrix of UG_JPEG_INPUT_RGB, and every refusal pinned before it, with its return code"""
    import torch
    from ultragrid_amd import lib as L
    l = L.load()
    enc = C.c_void_p()
    RGBF, NI = L.JPEG_INPUT_RGB, L.JPEG_NONINTERLEAVED
    for flags in (RGBF, RGBF | NI):
        for sub in (444, 4444):
            assert l.ug_hip_jpeg_encoder_create_ex(64, 64, 75, 4, sub, 0, flags, C.byref(enc)) == L.EINVAL
        for sub in (420, 422):
            assert l.ug_hip_jpeg_encoder_create_ex(64, 64, 75, 4, sub, 0, flags | L.JPEG_INPUT_UYVY, C.byref(enc)) == L.EINVAL
            for cs in (L.JPEG_CS_YCBCR_BT601, L.JPEG_CS_YCBCR_BT601_256LVLS, L.JPEG_CS_YCBCR_BT709):
                assert l.ug_hip_jpeg_encoder_create_ex(64, 64, 75, 4, sub, cs, flags, C.byref(enc)) == L.EUNSUPP
            for cs in (L.JPEG_CS_ASIS, L.JPEG_CS_RGB):
                for w, h in ((1, 1), (64, 64), (65535, 1)):
                    assert l.ug_hip_jpeg_encoder_create_ex(w, h, 75, 4, sub, cs, flags, C.byref(enc)) == 0
                    l.ug_hip_jpeg_encoder_destroy(enc)
    # pinned before this flag existed: unchanged
    assert l.ug_hip_jpeg_encoder_create_ex(64, 64, 75, 4, 444, 0, 4, C.byref(enc)) == L.EINVAL
    assert l.ug_hip_jpeg_encoder_create_ex(64, 64, 75, 4, 420, L.JPEG_CS_RGB, 0, C.byref(enc)) == L.EUNSUPP
    assert l.ug_hip_jpeg_encoder_create_ex(64, 64, 75, 4, 422, 0, NI, C.byref(enc)) == L.EUNSUPP
    assert l.ug_hip_jpeg_encoder_create_ex(64, 64, 75, 4, 422, 0, L.JPEG_INPUT_UYVY, C.byref(enc)) == L.EUNSUPP
    assert l.ug_hip_jpeg_encoder_create_ex(64, 64, 75, 4, 4444, 0, L.JPEG_INPUT_UYVY, C.byref(enc)) == L.EUNSUPP
    assert l.ug_hip_jpeg_encoder_create_ex(64, 64, 75, 4, 444, 7, 0, C.byref(enc)) == L.EINVAL
    assert l.ug_hip_jpeg_encoder_create_ex(64, 64, 75, 4, 444, 0, 8, C.byref(enc)) == L.EINVAL
    # such an encoder takes RGB only; a 4:2:x encoder without the flag still refuses RGB
    w, h = 64, 32
    src = torch.zeros(4 * w * h * 2, dtype=torch.uint8, device="cuda")
    out = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    n = C.c_size_t(0)
    for sub in (420, 422):
        assert l.ug_hip_jpeg_encoder_create_ex(w, h, 75, 4, sub, 0, RGBF, C.byref(enc)) == 0
        for fmt in (L.PF_UYVY, L.PF_I420, L.PF_RGBA):
            assert l.ug_hip_jpeg_encoder_encode(enc, fmt, src.data_ptr(), 0, out.data_ptr(), out.numel(), C.byref(n), _stream()) == L.EUNSUPP, fmt
        assert l.ug_hip_jpeg_encoder_encode(enc, L.PF_RGB, src.data_ptr(), 0, out.data_ptr(), out.numel(), C.byref(n), _stream()) == 0
        l.ug_hip_jpeg_encoder_destroy(enc)
        assert l.ug_hip_jpeg_encoder_create_ex(w, h, 75, 4, sub, 0, 0, C.byref(enc)) == 0
        assert l.ug_hip_jpeg_encoder_encode(enc, L.PF_RGB, src.data_ptr(), 0, out.data_ptr(), out.numel(), C.byref(n), _stream()) == L.EUNSUPP
        l.ug_hip_jpeg_encoder_destroy(enc)


def _module_input(po, rgb, codec, w, h):
    """(the frame in `codec`, the RGB the module feeds the encoder)"""
    from test_module_harness import _ref_best_and_decode, _to_codec
    if codec == "RGB":
        return rgb.ravel(), rgb
    if codec == "RGBA":
        rgba = po.convert_frame("RGB", "RGBA", rgb, w, h)
        return rgba, po.convert_frame("RGBA", "RGB", rgba, w, h).reshape(h, w, 3)
    src = _to_codec(po, rgb, codec, w, h)
    target, conv = _ref_best_and_decode(po, codec, ["UYVY", "RGB", "RGBA"], src, w, h)
    assert target in ("RGB", "RGBA"), target
    return src, (conv if target == "RGB" else po.convert_frame("RGBA", "RGB", conv, w, h)).reshape(h, w, 3)


@needs_harness
@pytest.mark.gpu
@pytest.mark.parametrize("codec", ["RGB", "RGBA", "BGR", "R10k"])
def test_gpu_through_the_reference_framework(tmp_path, hip, po, codec):
    """`-c jpeg:q=85:restart=4:RGB:subsampling=420|422[:interleaved]` (and `gpujpeg:`) on RGB-family input: the writer's stream over the RGB the
    module feeds the encoder; jpeg_mi355x and jpeg_to_dxt_mi355x decode it"""
    if codec != "RGB" and codec != "RGBA" and not po.have_ref():
        pytest.skip("oracle/_ref/libugref.so not built")
    w, h = 200, 72
    rgb = picture(w, h, seed=17)
    src, fed = _module_input(po, rgb, codec, w, h)
    raw = tmp_path / "in.raw"
    np.ascontiguousarray(src).tofile(raw)
    for sub in (420, 422):
        for inter in ("", ":interleaved"):
            want = _want(po, fed, sub, 85, 4, not inter)
            for name in ("jpeg", "gpujpeg"):
                cfg = f"{name}:q=85:restart=4:RGB:subsampling={sub}{inter}"
                out = tmp_path / "o.jpg"
                r = subprocess.run([HARNESS, cfg, codec, str(w), str(h), str(raw), str(out)], capture_output=True, text=True, timeout=60)
                assert r.returncode == 0, cfg + r.stdout + r.stderr
                assert out.read_bytes() == want, cfg
            jpg = tmp_path / "w.jpg"
            jpg.write_bytes(want)
            d = tmp_path / "d.raw"
            r = subprocess.run([DEC_HARNESS, "JPEG", "RGB", str(w), str(h), str(jpg), str(d)], capture_output=True, text=True, timeout=60)
            assert r.returncode == 0, r.stdout + r.stderr
            _, crop, _ = po.jpeg_decode_planes(want)
            rr = (2, 2 if sub == 420 else 1)
            got = np.fromfile(d, np.uint8)[: 3 * w * h]
            assert np.array_equal(got, expected(po, crop, [(1, 1), rr, rr], w, h, True, "RGB").ravel())
            x = tmp_path / "d.dxt"
            r = subprocess.run([DEC_HARNESS, "JPEG", "DXT5", str(w), str(h), str(jpg), str(x)], capture_output=True, text=True, timeout=60)
            assert r.returncode == 0 and x.stat().st_size > 0, r.stdout + r.stderr
