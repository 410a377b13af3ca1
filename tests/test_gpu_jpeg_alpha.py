"""GPU: four-component (R, G, B, alpha) JPEG -- the 4:4:4:4 encoder (subsampling=4444, RGBA input) byte for byte against the reference writer,
the decoder on its own streams and on libjpeg's (Pillow's CMYK) against Pillow, the outputs, the refusals, the receiving modules, and the
capacity check of a later scan of a non-interleaved stream."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

from jpeg_alpha_bitstream import coefs4444, rgba_picture, write_jpeg4444

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEC_HARNESS = os.path.join(ROOT, "oracle", "_ref", "ug_dec_harness")


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _planes_equal_pillow(hip, data, w, h):
    """the product decoder's four planes == 255 - Pillow's (inverted) CMYK, bit for bit; returns them (h, w, 4)"""
    dec = hip.JpegDecoder()
    planes = [p.cpu().numpy() for p in dec.planes(data)]
    dec.close()
    assert len(planes) == 4 and all(p.shape == (h, w) for p in planes)
    got = np.stack(planes, -1)
    img = Image.open(io.BytesIO(data))
    assert img.mode == "CMYK"
    assert np.array_equal(got, 255 - np.asarray(img))
    return got


CASES = [((64, 32), 85, 4), ((64, 32), 100, 1), ((150, 70), 50, 1), ((150, 70), 85, 300), ((150, 70), 100, 0),
         ((1366, 768), 85, 0), ((1366, 768), 50, 2000), ((1366, 768), 85, 4), ((3840, 2160), 85, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("nonint", [False, True], ids=["interleaved", "nonint"])
@pytest.mark.parametrize("dims,q,ri", CASES, ids=[f"{d[0]}x{d[1]}-q{q}-ri{ri}" for d, q, ri in CASES])
def test_gpu_encoder_bytes_equal_the_writer(hip, po, dims, q, ri, nonint):
    import torch
    from ultragrid_amd import lib as L
    w, h = dims
    x = rgba_picture(w, h)
    ql, qc = po.jpeg_qtable(q, 0), po.jpeg_qtable(q, 1)
    enc = hip.JpegEncoder(w, h, q, ri, subsampling=4444, flags=L.JPEG_NONINTERLEAVED if nonint else 0)
    data = enc.encode(torch.from_numpy(x.ravel()).cuda(), L.PF_RGBA)
    enc.close()
    assert data == write_jpeg4444(w, h, ql, qc, coefs4444(po, x, ql), restart=ri, nonint=nonint)
    if w * h <= 1366 * 768:
        _planes_equal_pillow(hip, data, w, h)


@pytest.mark.gpu
@pytest.mark.parametrize("nonint", [False, True], ids=["interleaved", "nonint"])
@pytest.mark.parametrize("ri", [4, 300, 0])
def test_gpu_wave_kernel_path(hip, po, ri, nonint, monkeypatch):
    """UG_JPEG_WAVE_KERNEL=1: the wave-per-segment coder and its compaction (the path of long restart intervals) on a small picture"""
    import torch
    from ultragrid_amd import lib as L
    monkeypatch.setenv("UG_JPEG_WAVE_KERNEL", "1")
    w, h, q = 150, 70, 85
    x = rgba_picture(w, h, 1)
    ql, qc = po.jpeg_qtable(q, 0), po.jpeg_qtable(q, 1)
    enc = hip.JpegEncoder(w, h, q, ri, subsampling=4444, internal_cs=L.JPEG_CS_RGB, flags=L.JPEG_NONINTERLEAVED if nonint else 0)
    data = enc.encode(torch.from_numpy(x.ravel()).cuda(), L.PF_RGBA)
    enc.close()
    assert data == write_jpeg4444(w, h, ql, qc, coefs4444(po, x, ql), restart=ri, nonint=nonint)


@pytest.mark.gpu
@pytest.mark.parametrize("nonint", [False, True], ids=["interleaved", "nonint"])
@pytest.mark.parametrize("ri", [4, 0])
def test_gpu_encode_batch(hip, po, ri, nonint):
    """three distinct frames in one call: each stream == the single-frame encode == the writer's"""
    import torch
    from ultragrid_amd import lib as L
    w, h, q = 640, 360, 80
    frames = [rgba_picture(w, h, s) for s in (1, 2, 3)]
    ql, qc = po.jpeg_qtable(q, 0), po.jpeg_qtable(q, 1)
    enc = hip.JpegEncoder(w, h, q, ri, subsampling=4444, flags=L.JPEG_NONINTERLEAVED if nonint else 0)
    got = enc.encode_batch(torch.stack([torch.from_numpy(f.ravel()) for f in frames]).cuda(), L.PF_RGBA)
    one = [enc.encode(torch.from_numpy(f.ravel()).cuda(), L.PF_RGBA) for f in frames]
    enc.close()
    assert len(got) == 3 and got == one and len(set(got)) == 3
    for f, data in zip(frames, got):
        assert data == write_jpeg4444(w, h, ql, qc, coefs4444(po, f, ql), restart=ri, nonint=nonint)


def _pillow_cmyk(x, **kw):
    b = io.BytesIO()
    Image.fromarray(x, "CMYK").save(b, "JPEG", quality=90, **kw)
    return b.getvalue()


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [{}, {"restart_marker_blocks": 3}, {"optimize": True}], ids=["plain", "restart", "optimize"])
@pytest.mark.parametrize("dims", [(150, 70), (1366, 768)], ids=str)
def test_gpu_third_party_four_component_streams(hip, po, kw, dims):
    """libjpeg's four-component streams (Pillow CMYK, no restart intervals by default): the planes, and every output of the decoder"""
    import torch
    from ultragrid_amd import lib as L
    w, h = dims
    data = _pillow_cmyk(rgba_picture(w, h, 5), **kw)
    planes = _planes_equal_pillow(hip, data, w, h)
    dec = hip.JpegDecoder()
    rgba = dec.decode(data, L.PF_RGBA).cpu().numpy().reshape(h, w, 4)
    assert np.array_equal(rgba, planes)
    bgr = dec.decode(data, L.PF_RGBA, shifts=(16, 8, 0)).cpu().numpy().reshape(h, w, 4)
    assert np.array_equal(bgr[..., :3], planes[..., 2::-1]) and (bgr[..., 3] == 255).all()
    rgb_planes = np.ascontiguousarray(planes[..., :3])
    for out in ("RGB", "UYVY"):
        got = dec.decode(data, getattr(L, "PF_" + out)).cpu().numpy()
        assert np.array_equal(got, po.convert_frame("RGB", out, rgb_planes.ravel(), w, h).ravel()), out
    # guard bytes behind dst stay untouched (packed RGBA)
    n = 4 * w * h
    buf = torch.full((n + 4096,), 0x5A, dtype=torch.uint8, device="cuda")
    assert L.load().ug_hip_jpeg_decoder_decode_sized(dec._h, data, len(data), w, h, L.PF_RGBA, buf.data_ptr(), 0, 0, 8, 16, _stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(buf[:n].cpu().numpy().reshape(h, w, 4), planes) and bool((buf[n:] == 0x5A).all())
    assert dec.decode(data, L.PF_RGB).numel() == 3 * w * h
    with pytest.raises(L.UgHipError):
        dec.decode(data, L.PF_I420)
    dec.close()


@pytest.mark.gpu
def test_gpu_refusals_and_damage(hip, po):
    import torch
    from ultragrid_amd import lib as L
    l = L.load()
    h_enc = C.c_void_p()
    for cs in (L.JPEG_CS_YCBCR_BT601, L.JPEG_CS_YCBCR_BT601_256LVLS, L.JPEG_CS_YCBCR_BT709):
        assert l.ug_hip_jpeg_encoder_create_ex(64, 32, 80, 4, 4444, cs, 0, C.byref(h_enc)) == L.EUNSUPP
    assert l.ug_hip_jpeg_encoder_create_ex(64, 32, 80, 4, 4444, 0, L.JPEG_INPUT_UYVY, C.byref(h_enc)) == L.EUNSUPP
    w, h = 64, 32
    x = rgba_picture(w, h)
    enc = hip.JpegEncoder(w, h, 80, 4, subsampling=4444)
    with pytest.raises(L.UgHipError):
        enc.encode(torch.from_numpy(np.ascontiguousarray(x[..., :3]).ravel()).cuda(), L.PF_RGB)
    data = enc.encode(torch.from_numpy(x.ravel()).cuda(), L.PF_RGBA)
    enc.close()
    # an R,G,B 4:4:4 encoder does not take RGBA
    enc3 = hip.JpegEncoder(w, h, 80, 4, subsampling=444)
    with pytest.raises(L.UgHipError):
        enc3.encode(torch.from_numpy(x.ravel()).cuda(), L.PF_RGBA)
    enc3.close()
    # damaged streams: a defined code, nothing written behind dst
    sos = data.index(b"\xff\xda")
    rst = data.index(b"\xff\xd0", sos)
    dec = hip.JpegDecoder()
    for bad in (data[: len(data) - 40], data[:rst] + data[rst + 2:]):
        n = 4 * w * h
        buf = torch.full((n + 4096,), 0x5A, dtype=torch.uint8, device="cuda")
        rc = l.ug_hip_jpeg_decoder_decode_sized(dec._h, bad, len(bad), w, h, L.PF_RGBA, buf.data_ptr(), 0, 0, 8, 16, _stream())
        torch.cuda.synchronize()
        assert rc in (0, L.EUNSUPP, L.EINVAL) and bool((buf[n:] == 0x5A).all())
    dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ncomp", [3, 4])
def test_gpu_later_scan_header_respects_capacity(hip, po, ncomp):
    """a stream of one scan per component that does not fit the buffer -- the later scans' headers must not be written past the
    capacity either: EINVAL, out_len = the size it needs, every byte behind the capacity untouched"""
    import torch
    from ultragrid_amd import lib as L
    l = L.load()
    w, h, q, ri = 640, 360, 85, 4
    x = rgba_picture(w, h, 7)
    src = torch.from_numpy((x if ncomp == 4 else np.ascontiguousarray(x[..., :3])).ravel()).cuda()
    fmt = L.PF_RGBA if ncomp == 4 else L.PF_RGB
    enc = C.c_void_p()
    assert l.ug_hip_jpeg_encoder_create_ex(w, h, q, ri, 4444 if ncomp == 4 else 444, 0, L.JPEG_NONINTERLEAVED, C.byref(enc)) == 0
    cap = l.ug_hip_jpeg_encoder_max_size(enc)
    full = torch.empty(cap, dtype=torch.uint8, device="cuda")
    n = C.c_size_t(0)
    assert l.ug_hip_jpeg_encoder_encode(enc, fmt, src.data_ptr(), 0, full.data_ptr(), cap, C.byref(n), _stream()) == 0
    need = n.value
    short = need // 5
    buf = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    m = C.c_size_t(0)
    assert l.ug_hip_jpeg_encoder_encode(enc, fmt, src.data_ptr(), 0, buf.data_ptr(), short, C.byref(m), _stream()) == L.EINVAL
    torch.cuda.synchronize()
    l.ug_hip_jpeg_encoder_destroy(enc)
    assert m.value == need and bool((buf[short:] == 0xA5).all())


needs_dec_harness = pytest.mark.skipif(not os.path.exists(DEC_HARNESS), reason="oracle/_ref/ug_dec_harness not built")


@needs_dec_harness
@pytest.mark.gpu
def test_gpu_receiving_modules(tmp_path, hip, po):
    """jpeg_mi355x: the probe says 4444 / RGB, RGBA output keeps the alpha at any display pitch; the JPEG -> DXT5 transcoder reads the R, G, B
    components of a 4444 stream exactly as it reads the R,G,B stream of the same coefficient planes"""
    import torch
    from jpeg_bitstream import write_jpeg
    from ultragrid_amd import lib as L
    w, h, q = 256, 128, 85
    x = rgba_picture(w, h, 9)
    enc = hip.JpegEncoder(w, h, q, 4, subsampling=4444)
    data = enc.encode(torch.from_numpy(x.ravel()).cuda(), L.PF_RGBA)
    enc.close()
    planes = _planes_equal_pillow(hip, data, w, h)
    src, dst = tmp_path / "a.jpg", tmp_path / "out.raw"
    src.write_bytes(data)
    for pitch in (4 * w, 4 * w + 64):
        r = subprocess.run([DEC_HARNESS, "JPEG", "RGBA", str(w), str(h), str(src), str(dst), str(pitch)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "PROBE" in r.stdout and "subsampling=4444 rgb=1" in r.stdout, r.stdout
        got = np.fromfile(dst, np.uint8).reshape(h, pitch)[:, : 4 * w].reshape(h, w, 4)
        assert np.array_equal(got, planes)
    ql, qc = po.jpeg_qtable(q, 0), po.jpeg_qtable(q, 1)
    c = coefs4444(po, x, ql)
    rgb_src = tmp_path / "rgb.jpg"
    rgb_src.write_bytes(write_jpeg(w, h, ql, qc, c[0], c[1], c[2], restart=4, sub=444))
    outs = []
    for f in (src, rgb_src):
        o = tmp_path / (f.stem + ".dxt")
        r = subprocess.run([DEC_HARNESS, "JPEG", "DXT5", str(w), str(h), str(f), str(o)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(o.read_bytes())
    assert outs[0] == outs[1] and len(outs[0]) > 0
