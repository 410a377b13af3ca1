"""GPU: the JPEG decoder's own dst_pitch and dst_dev (ug_hip_jpeg_decoder_decode_sized) at the pitches and base addresses that move its output
kernels between their tiers (csrc/jpeg_decode.hip: planar_rgb_pack_kernel, yuv444p_to_uyvy_kernel, layout_pack_kernel; csrc/planar.hip:
planar_to_uyvy_kernel; the pixel-format converter behind them).  The streams are inputs made without the GPU; the expectation is the decode
oracle's planes through the compositions tests/test_gpu_jpeg_decode.py uses, laid out at the destination's pitch with canaries in front of the
picture, behind it and in every line's padding (tests/pitch_layout.py).  Then the rule of include/ug_mi355x.h: what it refuses is UG_HIP_EINVAL
with nothing written, and the decoder object decodes the next picture as before."""
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pitch_layout as pl  # noqa: E402
from jpeg_alpha_bitstream import coefs4444, rgba_picture, write_jpeg4444  # noqa: E402
from jpeg_bitstream import write_jpeg  # noqa: E402
from jpeg_layout_bitstream import layout_stream  # noqa: E402
from jpeg_layout_restatement import expected, ycc_to_uyvy  # noqa: E402
from test_oracle_jpeg_decode import picture, pil_jpeg  # noqa: E402

pytestmark = pytest.mark.gpu

# 520 x 10: width % 8 == 0 and 65 eight-pixel units, one more than a workgroup row of planar_to_uyvy_kernel<_, true>; 50 x 9: the general tier;
# 17 x 9: odd width -- the last pair's second pixel, a UYVY line longer than 2 w
SIZES = [(520, 10), (50, 9), (17, 9)]
KINDS = ["ycc444", "ycc422", "ycc420", "grey", "rgb444", "rgba"]   # restart intervals: ycc422 (3 blocks), rgb444 (4 MCUs); the others have none
OUTS = [("UYVY", (0, 8, 16)), ("RGB", (0, 8, 16)), ("RGBA", (0, 8, 16)), ("RGBA", (16, 8, 0))]


def r16(x):
    return (x + 15) // 16 * 16


_STREAMS = {}


def stream_of(po, kind, w, h):
    """-> (stream, the oracle's planes cropped to the components' sizes); made once per (kind, size)"""
    if (kind, w, h) not in _STREAMS:
        if kind.startswith("ycc"):
            kw = {"ycc444": dict(quality=90, subsampling=0), "ycc422": dict(quality=85, subsampling=1, restart_marker_blocks=3), "ycc420": dict(quality=80, subsampling=2)}[kind]
            data = pil_jpeg(picture(w, h, seed=w), **kw)
        elif kind == "grey":
            b = io.BytesIO()
            Image.fromarray(picture(w, h, seed=w + 1)[..., 1].copy(), "L").save(b, "JPEG", quality=88)
            data = b.getvalue()
        elif kind == "rgb444":
            rgb = picture(w, h, seed=w + 2)
            ql = po.jpeg_qtable(85, 0)
            coefs = [po.jpeg_fdct_quant_plane(np.ascontiguousarray(rgb[..., c]), po.jpeg_divisors(ql), (w + 7) // 8, (h + 7) // 8) for c in range(3)]
            data = write_jpeg(w, h, ql, po.jpeg_qtable(85, 1), *coefs, restart=4, sub=444)
        else:
            ql, qc = po.jpeg_qtable(85, 0), po.jpeg_qtable(85, 1)
            data = write_jpeg4444(w, h, ql, qc, coefs4444(po, rgba_picture(w, h, 3), ql), restart=0)
        if kind == "rgba":   # four components: libjpeg's planes, which Pillow hands back inverted as CMYK (tests/test_gpu_jpeg_alpha.py)
            img = Image.open(io.BytesIO(data))
            assert img.mode == "CMYK"
            crop = [np.ascontiguousarray(255 - np.asarray(img)[..., c]) for c in range(4)]
        else:
            _, crop, _ = po.jpeg_decode_planes(data)
        assert len(crop) == {"grey": 1, "rgba": 4}.get(kind, 3) and crop[0].shape == (h, w)
        _STREAMS[(kind, w, h)] = (data, crop)
    return _STREAMS[(kind, w, h)]


def _packed_uyvy(po, kind, crop, w, h):
    """-> ((h, line) bytes, bytes of a line the decoder writes): 4:2:2 hands its samples back, w // 2 pairs, nothing for an odd tail (yuv422p_to_uyvy);
    4:2:0 repeats the chroma lines, an odd tail is Cb Y Cr 0 (yuv420p_to_uyvy); 4:4:4 and greyscale (chroma 128) average the pair's chroma, the
    last pair of an odd width takes its first pixel twice"""
    line = 4 * ((w + 1) // 2)
    if kind in ("ycc422", "ycc420"):
        return po.planar_to_uyvy(*crop, w, h, chroma=int(kind[3:])).reshape(h, line), (4 * (w // 2) if kind == "ycc422" else line)
    planes = list(crop) if kind == "ycc444" else [crop[0], np.full((h, w), 128, np.uint8), np.full((h, w), 128, np.uint8)]
    return ycc_to_uyvy([p.astype(np.int64) for p in planes], w), line


def _with_slack(lines):
    buf = pl.aligned_bytes(lines.size + pl.SLACK)
    buf[: lines.size] = lines.ravel()
    return buf


def want_buffer(po, kind, crop, w, h, out, sh, dp, do):
    """-> (the whole destination as it has to be afterwards, front, bytes of a line to compare): FILL wherever the decoder writes nothing"""
    line = {"UYVY": 4 * ((w + 1) // 2), "RGB": 3 * w, "RGBA": 4 * w}[out]
    want, front = pl.make_dst(h, dp, do)

    def put(lines, n):
        for y in range(h):
            want[front + y * dp: front + y * dp + n] = lines[y, :n]
        return want, front, line

    if kind in ("rgb444", "rgba"):
        r, g, b = (c.astype(np.uint32) for c in crop[:3])
        if out == "RGB":
            return put(np.stack([r, g, b], -1).astype(np.uint8).reshape(h, 3 * w), line)
        if out == "RGBA":   # the A sample where the shifts leave it the top byte, else 0xFF in the byte they leave
            rs, gs, bs = sh
            rest = crop[3].astype(np.uint32) << 24 if kind == "rgba" and sh == (0, 8, 16) else np.uint32(0xFFFFFFFF ^ (0xFF << rs) ^ (0xFF << gs) ^ (0xFF << bs))
            return put((rest | r << rs | g << gs | b << bs).astype("<u4").view(np.uint8).reshape(h, 4 * w), line)
        src = _with_slack(np.stack([r, g, b], -1).astype(np.uint8))   # UYVY: through packed RGB and vc_copylineRGBtoUYVY
        want, front = pl.ref_convert_pitched(po, "RGB", "UYVY", src, 0, w, h, 3 * w, dp, sh, dst_off=do)
        return want, front, pl.Sizes(po, "RGB", "UYVY", w).written_len
    uyvy, n = _packed_uyvy(po, kind, crop, w, h)
    if out == "UYVY":
        return put(uyvy, n)
    # RGB / RGBA: that UYVY through vc_copylineUYVYtoRGB[A], a whole pair per step (the last pixel of an odd width stays as it was)
    want, front = pl.ref_convert_pitched(po, "UYVY", out, _with_slack(uyvy), 0, w, h, uyvy.shape[1], dp, sh, dst_off=do)
    return want, front, pl.Sizes(po, "UYVY", out, w).written_len


def dst_layouts(out, line):
    """-> [(name, pitch argument, pitch, base offset)]"""
    p16 = r16(line) + 32
    wp = line + 4 + (4 if (line + 4) % 16 == 0 else 0)
    lay = [("packed", 0, line, 0), ("padded16", p16, p16, 0), ("word_pitch", wp, wp, 0), ("dst_off", p16, p16, 4)]
    if out == "RGB":
        lay.append(("odd_pitch", line + 13, line + 13, 1))
    return lay


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def decode_at(hip, dec, data, w, h, out, dst, front, pitch_arg, sh):
    """one ug_hip_jpeg_decoder_decode_sized call on a device copy of the destination -> (rc, the whole buffer afterwards)"""
    import torch
    L = hip.L
    dev = torch.from_numpy(dst).cuda()
    assert dev.data_ptr() % 256 == 0
    rc = L.load().ug_hip_jpeg_decoder_decode_sized(dec._h, data, len(data), w, h, getattr(L, "PF_" + out), dev.data_ptr() + front, pitch_arg, *sh, _stream())
    torch.cuda.synchronize()
    return rc, dev.cpu().numpy()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", KINDS)
def test_outputs_at_every_destination_layout(hip, po, kind, size):
    """every output of a stream at every destination layout, on ONE decoder object: the lines == the expectation, every other byte still FILL"""
    w, h = size
    data, crop = stream_of(po, kind, w, h)
    dec = hip.JpegDecoder()
    problems = []
    for out, sh in OUTS:
        line = {"UYVY": 4 * ((w + 1) // 2), "RGB": 3 * w, "RGBA": 4 * w}[out]
        assert line == hip.linesize(getattr(hip.L, "PF_" + out), w)
        for lname, parg, dp, do in dst_layouts(out, line):
            want, front, n = want_buffer(po, kind, crop, w, h, out, sh, dp, do)
            dst, _ = pl.make_dst(h, dp, do)
            rc, got = decode_at(hip, dec, data, w, h, out, dst, front, parg, sh)
            found = [("rc", rc, hip.L.last_error())] if rc != 0 else pl.compare(got, want, h, dp, n, front)
            if found:
                problems.append((out, sh, lname, (dp, do), found))
    dec.close()
    assert not problems, (kind, size, problems)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ["ycc420", "grey"])
def test_i420_output(hip, po, kind, size):
    """UG_PF_I420 (4:2:0 and greyscale streams) is tightly packed: dst_pitch 0 and the width give the planes back to back, nothing around them"""
    w, h = size
    data, crop = stream_of(po, kind, w, h)
    cn = ((w + 1) // 2) * ((h + 1) // 2)
    planes = np.concatenate([p.ravel() for p in crop]) if kind == "ycc420" else np.concatenate([crop[0].ravel(), np.full(2 * cn, 128, np.uint8)])
    assert planes.size == w * h + 2 * cn
    dec = hip.JpegDecoder()
    for pitch in (0, w):
        dst = pl.aligned_bytes(pl.GUARD + planes.size + pl.GUARD, fill=pl.FILL)
        want = dst.copy()
        want[pl.GUARD: pl.GUARD + planes.size] = planes
        rc, got = decode_at(hip, dec, data, w, h, "I420", dst, pl.GUARD, pitch, (0, 8, 16))
        assert rc == 0, (pitch, hip.L.last_error())
        assert pl.compare_frames(got, want, 1, 0, 1, planes.size, planes.size, pl.GUARD) == [], (kind, size, pitch)
    dec.close()


@pytest.mark.parametrize("code,rgb", [(440, None), (411, "ids")], ids=["440-ycc", "411-rgb"])
def test_other_sampling_layouts_at_an_odd_base(hip, po, code, rgb):
    """layout_pack_kernel (4:4:0 Y'CbCr, 4:1:1 R,G,B) takes any base: a padded pitch with the picture one byte off a 256-byte aligned address, after
    a packed decode on the same decoder object"""
    problems = []
    dec = hip.JpegDecoder()
    for (w, h) in SIZES[1:]:
        data = layout_stream(po, w, h, code, restart=3, rgb=rgb, seed=1)
        info, crop, _ = po.jpeg_decode_planes(data)
        hmax, vmax = max(info["h"]), max(info["v"])
        ratios = [(hmax // hs, vmax // vs) for hs, vs in zip(info["h"], info["v"])]
        for out, sh in OUTS:
            line = hip.linesize(getattr(hip.L, "PF_" + out), w)
            lines = expected(po, crop, ratios, w, h, rgb is not None, out, sh)
            n = line - (line // w if rgb is None and out != "UYVY" and w % 2 else 0)   # Y'CbCr -> RGB[A]: a whole pair per step, as everywhere
            for parg, dp, do in ((0, line, 0), (r16(line) + 32, r16(line) + 32, 1)):
                want, front = pl.make_dst(h, dp, do)
                for y in range(h):
                    want[front + y * dp: front + y * dp + n] = lines[y, :n]
                dst, _ = pl.make_dst(h, dp, do)
                rc, got = decode_at(hip, dec, data, w, h, out, dst, front, parg, sh)
                found = [("rc", rc, hip.L.last_error())] if rc != 0 else pl.compare(got, want, h, dp, line, front)
                if found:
                    problems.append(((w, h), out, sh, (dp, do), found))
    dec.close()
    assert not problems, (code, problems)


# ---------------------------------------------------------------------- the rule ----------------------------------------------------------------------
def _refused(hip, dec, data, w, h, out, pitch, off, lines=None):
    """a call the rule refuses, its pointer in the middle of an allocation with |pitch| * height + 4096 owned bytes on both sides
    -> findings (empty: UG_HIP_EINVAL and every byte still FILL)"""
    import torch
    L = hip.L
    margin = r16(abs(pitch) * h + 4096)
    buf = torch.full((2 * margin + abs(pitch) * h + 4096,), pl.FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    rc = L.load().ug_hip_jpeg_decoder_decode_sized(dec._h, data, len(data), w, h, getattr(L, "PF_" + out), buf.data_ptr() + margin + off, pitch, 0, 8, 16, _stream())
    torch.cuda.synchronize()
    found = []
    if rc != L.EINVAL:
        found.append(("not refused", rc))
    if not bool((buf == pl.FILL).all()):
        found.append("the destination was written")
    return found


@pytest.mark.parametrize("kind", KINDS)
def test_refused_pitches_and_addresses(hip, po, kind):
    """dst_pitch below the line, a negative one, and -- UYVY and RGBA, on every classic stream alike -- a pitch or a base that is no multiple of 4;
    I420 at a pitch that is not the width: UG_HIP_EINVAL, the destination still all FILL, and the same decoder object then decodes the picture
    packed, correctly"""
    w, h = 50, 9
    data, crop = stream_of(po, kind, w, h)
    dec = hip.JpegDecoder()
    problems = []
    for out in ("UYVY", "RGBA", "RGB"):
        line = hip.linesize(getattr(hip.L, "PF_" + out), w)
        p16 = r16(line) + 32
        cases = [("below the line", line - 4, 0), ("pitch 4", 4, 0), ("negative", -r16(line), 0)]
        if out != "RGB":
            cases += [("pitch % 4 == 2", p16 + 2, 0), ("pitch % 4 == 1", p16 + 1, 0), ("base + 2", p16, 2), ("base + 1", p16, 1), ("base + 2, packed", 0, 2)]
        for what, pitch, off in cases:
            found = _refused(hip, dec, data, w, h, out, pitch, off)
            if found:
                problems.append((out, what, found))
        want, front, n = want_buffer(po, kind, crop, w, h, out, (0, 8, 16), line, 0)
        dst, _ = pl.make_dst(h, line, 0)
        rc, got = decode_at(hip, dec, data, w, h, out, dst, front, 0, (0, 8, 16))
        found = [("rc", rc, hip.L.last_error())] if rc != 0 else pl.compare(got, want, h, line, n, front)
        if found:
            problems.append((out, "the packed decode after the refusals", found))
    if kind in ("ycc420", "grey"):
        found = _refused(hip, dec, data, w, h, "I420", w + 16, 0)
        if found:
            problems.append(("I420", "pitch = width + 16", found))
        dst = pl.aligned_bytes(pl.GUARD + w * h + 2 * 25 * 5 + pl.GUARD, fill=pl.FILL)
        rc, got = decode_at(hip, dec, data, w, h, "I420", dst, pl.GUARD, 0, (0, 8, 16))
        if rc != 0 or not np.array_equal(got[pl.GUARD: pl.GUARD + w * h].reshape(h, w), crop[0]):
            problems.append(("I420", "the packed decode after the refusal", rc))
    dec.close()
    assert not problems, (kind, problems)
