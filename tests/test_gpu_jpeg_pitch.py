"""GPU: the JPEG encoder and its front ends at the pitches, base addresses and frame strides that move them between their 16-byte, 4-byte and
byte tiers (csrc/jpeg_entropy.hip: the fused coder; csrc/jpeg_fdct.hip: the fast, general and plane kernels, the colour stage).  The source is
placed among random bytes (tests/pitch_layout.py: place_frames) -- line padding, the gaps between the frames of a batch, what lies in front of
the first line and behind the last --, the expectation is always the oracle on the PACKED frame through the test writers: the stream bytes and
out_len are equal, 0 bytes differing, whatever the layout.  Then the pitch and alignment rule of include/ug_mi355x.h: what it refuses is
refused with UG_HIP_EINVAL on every path alike, with nothing written."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pitch_layout as pl  # noqa: E402
from jpeg_alpha_bitstream import coefs4444, write_jpeg4444  # noqa: E402
from jpeg_bitstream import write_jpeg, write_jpeg_noninterleaved  # noqa: E402
from jpeg_layout_bitstream import layout_coefs, write_layout_jpeg  # noqa: E402

pytestmark = pytest.mark.gpu

Q = 90
# 528 x 40: width % 16 == 0, 33 MCUs = one more than the strip of 32 (RGB: 64) of a fast / fused workgroup, the last MCU row replicates;
# 522 x 9: even, width % 16 != 0, odd height: the general kernels, column and row replication next to random padding;
# 48 x 16: 3 MCUs, the smallest picture the fused coder takes
SIZES = [(528, 40), (522, 9), (48, 16)]
FRAMES = 3
CS_RGB, Y601, Y601FULL, Y709 = 1, 2, 3, 4
RGB42X = ((2, 2), (1, 1), (1, 1))

# name -> (input, restart interval, subsampling, internal_cs, flags, expectation).  Restart interval 4 divides a workgroup's 32 (64) MCUs: the fused
# coder where the alignment allows; 7 does not: front end + coder
PATHS = {
    "uyvy420-ri4": ("UYVY", 4, 420, 0, (), "uyvy42x"),
    "uyvy420-ri7": ("UYVY", 7, 420, 0, (), "uyvy42x"),
    "uyvy422-ri4": ("UYVY", 4, 422, 0, (), "uyvy42x"),
    "uyvy422-ri7": ("UYVY", 7, 422, 0, (), "uyvy42x"),
    "rgb444-ri4": ("RGB", 4, 444, 0, (), "rgb444"),
    "rgb444-ri7": ("RGB", 7, 444, 0, (), "rgb444"),
    "rgb444-nonint": ("RGB", 4, 444, 0, ("JPEG_NONINTERLEAVED",), "rgb444"),
    "rgb444-bt601full": ("RGB", 4, 444, Y601FULL, (), "rgb444ycc"),       # colour stage + the strided plane FDCT
    "rgba4444": ("RGBA", 4, 4444, 0, (), "rgba"),
    "uyvy444": ("UYVY", 4, 444, 0, ("JPEG_INPUT_UYVY",), "uyvy444"),
    "uyvy422-bt601": ("UYVY", 4, 422, Y601, (), "uyvy42x"),
    "rgb420-inrgb": ("RGB", 4, 420, 0, ("JPEG_INPUT_RGB",), "rgb42x"),
}
# (R, G, B at 4:2:0 has a pitch test of its own, tests/test_gpu_jpeg_rgb_subsampled.py: here the base offset and the batch strides it lacks)
CASES = [(name, size) for name in PATHS if name != "rgb420-inrgb" for size in SIZES] + [("rgb420-inrgb", SIZES[0])]


def r16(x):
    return (x + 15) // 16 * 16


def line_of(hip, fmt, w):
    return hip.linesize(hip.L.PF_UYVY, w) if fmt == "UYVY" else (4 if fmt == "RGBA" else 3) * w


def layouts(fmt, line, only=None):
    """-> [(name, pitch argument, pitch, base offset)]"""
    e = 1 if fmt == "RGB" else 4
    p16 = r16(line) + 16
    wp = line + 4 + (4 if (line + 4) % 16 == 0 else 0)
    out = [("packed", 0, line, 0), ("padded16", p16, p16, 0), ("word_pitch", wp, wp, 0)]
    if fmt == "RGB":
        out.append(("odd_pitch", line + 13, line + 13, 0))
    out.append(("src_off", p16, p16, e))
    return [x for x in out if only is None or x[0] in only]


def _frames(fmt, line, w, h):
    rng = np.random.default_rng([w, h, len(fmt)])
    return [rng.integers(0, 256, line * h, dtype=np.uint8) for _ in range(FRAMES)]


def _coefs444(po, planes, ql, qc, w, h):
    bw, bh = (w + 7) // 8, (h + 7) // 8
    return [po.jpeg_fdct_quant_plane(np.ascontiguousarray(planes[..., c]), po.jpeg_divisors(ql if c == 0 or qc is None else qc), bw, bh) for c in range(3)]


def _coefs42x(po, uyvy, w, h, sub, ql, qc):
    y, u, v = po.uyvy_to_i420(uyvy, w, h) if sub == 420 else po.uyvy_to_i422(uyvy, w, h)
    mw, mh, vs = (w + 15) // 16, ((h + 15) // 16 if sub == 420 else (h + 7) // 8), (2 if sub == 420 else 1)
    dl, dc = po.jpeg_divisors(ql), po.jpeg_divisors(qc)
    return po.jpeg_fdct_quant_plane(y, dl, 2 * mw, vs * mh), po.jpeg_fdct_quant_plane(u, dc, mw, mh), po.jpeg_fdct_quant_plane(v, dc, mw, mh)


_WANT = {}


def want_stream(po, name, frame, w, h, key):
    """the oracle on the packed frame, through the test writers; computed once per (path, size, frame)"""
    if (name, w, h, key) in _WANT:
        return _WANT[(name, w, h, key)]
    fmt, ri, sub, cs, flags, kind = PATHS[name]
    ql, qc = po.jpeg_qtable(Q, 0), po.jpeg_qtable(Q, 1)
    if kind == "uyvy42x":
        uyvy = po.jpeg_colour_convert("UYVY", Y709, cs, frame, w, h) if cs else frame
        data = write_jpeg(w, h, ql, qc, *_coefs42x(po, uyvy, w, h, sub, ql, qc), restart=ri, sub=sub)
    elif kind == "rgb444":
        coefs = _coefs444(po, frame.reshape(h, w, 3), ql, None, w, h)
        data = write_jpeg_noninterleaved(w, h, ql, coefs, restart=ri) if flags else write_jpeg(w, h, ql, qc, *coefs, restart=ri, sub=444)
    elif kind == "rgb444ycc":
        ycc = po.jpeg_colour_convert("RGB", CS_RGB, cs, frame, w, h).reshape(h, w, 3)
        data = write_jpeg(w, h, ql, qc, *_coefs444(po, ycc, ql, qc, w, h), restart=ri, sub=444, ycc=True)
    elif kind == "rgba":
        data = write_jpeg4444(w, h, ql, qc, coefs4444(po, frame.reshape(h, w, 4), ql), restart=ri)
    elif kind == "uyvy444":
        pic = po.jpeg_colour_convert("UYVY444", Y709, Y709, frame, w, h).reshape(h, w, 3)
        data = write_jpeg(w, h, ql, qc, *_coefs444(po, pic, ql, qc, w, h), restart=ri, sub=444, ycc=True)
    else:
        x = frame.reshape(h, w, 3)
        data = write_layout_jpeg(w, h, RGB42X, ql, qc, layout_coefs(po, x, RGB42X, ql, qc, rgb=True), restart=ri, nonint=False, rgb="both")
    _WANT[(name, w, h, key)] = data
    return data


def _upload(buf):
    import torch
    dev = torch.from_numpy(buf).cuda()
    assert dev.data_ptr() % 256 == 0
    return dev


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _make_encoder(hip, name, w, h):
    fmt, ri, sub, cs, flags, _ = PATHS[name]
    return hip.JpegEncoder(w, h, Q, ri, subsampling=sub, internal_cs=cs, flags=sum(getattr(hip.L, f) for f in flags))


def encode_at(hip, enc, fmt, src_ptr, pitch_arg, n, stride):
    """one encode (n == 1) / encode_batch call into a destination of FILL between guards, slices r16(capacity) + 48 apart
    -> (rc, [out_len], [the bytes of each slice up to its capacity], findings about every byte the encoder does not own)"""
    import torch
    L = hip.L
    cap = enc.max_size
    ostride = r16(cap) + 48
    out = torch.full((pl.GUARD + n * ostride + pl.GUARD,), pl.FILL, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 256 == 0
    lens = (C.c_size_t * n)()
    pf = L.PF_NAMES[fmt]
    if n == 1:
        rc = L.load().ug_hip_jpeg_encoder_encode(enc._h, pf, src_ptr, pitch_arg, out.data_ptr() + pl.GUARD, cap, lens, _stream())
    else:
        rc = L.load().ug_hip_jpeg_encoder_encode_batch(enc._h, pf, n, src_ptr, pitch_arg, stride, out.data_ptr() + pl.GUARD, ostride, cap, lens, _stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    found = []
    if (got[: pl.GUARD] != pl.FILL).any() or (got[pl.GUARD + n * ostride:] != pl.FILL).any():
        found.append("a guard was written")
    slices = []
    for f in range(n):
        s = got[pl.GUARD + f * ostride: pl.GUARD + (f + 1) * ostride]
        if (s[cap:] != pl.FILL).any():
            found.append(f"frame {f}: bytes at or beyond out_capacity written")
        slices.append(s[:cap])
    return rc, [int(x) for x in lens], slices, found


def _differing(slice_, length, want):
    """bytes in which the stream differs from the expected one (a length that differs counts every byte of the difference)"""
    n = min(length, len(want), slice_.size)
    return int(np.count_nonzero(slice_[:n] != np.frombuffer(want, np.uint8)[:n])) + abs(length - len(want))


@pytest.mark.parametrize("name,size", CASES, ids=[f"{n}-{s[0]}x{s[1]}" for n, s in CASES])
def test_streams_at_every_source_layout(hip, po, name, size):
    """every source layout, one frame per call and three (frames 16 bytes aligned: + 80; frames 1 and 2 off the 16-byte tier: + 12): each stream
    == the oracle's for the packed frame, out_len == its length, nothing written at or beyond out_capacity of a slice or in the guards"""
    w, h = size
    fmt = PATHS[name][0]
    line = line_of(hip, fmt, w)
    frames = _frames(fmt, line, w, h)
    want = [want_stream(po, name, f, w, h, k) for k, f in enumerate(frames)]
    assert len(set(want)) == FRAMES
    enc = _make_encoder(hip, name, w, h)
    problems = []
    for lname, parg, pitch, off in layouts(fmt, line, only=("src_off",) if name == "rgb420-inrgb" else None):
        for extra in (80, 12):
            stride = pitch * h + extra
            dev = _upload(pl.place_frames(frames, line, h, pitch, off, stride, np.random.default_rng(pitch + extra)))
            for n in ((1, FRAMES) if extra == 80 else (FRAMES,)):
                rc, lens, slices, found = encode_at(hip, enc, fmt, dev.data_ptr() + off, parg, n, stride)
                tag = (lname, pitch, off, f"{n} frame(s)", f"stride + {extra}")
                if rc != 0:
                    problems.append((tag, "rc", rc, hip.L.last_error()))
                    continue
                bad = [(f, lens[f], len(want[f]), _differing(slices[f], lens[f], want[f])) for f in range(n)]
                bad = [b for b in bad if b[3] or b[1] != b[2]]
                if bad or found:
                    problems.append((tag, "(frame, out_len, expected length, bytes differing)", bad, found))
    enc.close()
    assert not problems, (name, size, problems)


# ------------------------------------------------------------- the front-end entry points -------------------------------------------------------------
def _i16_dst(n_bytes, frames, stride):
    """int16 coefficient planes as bytes of FILL between guards: `frames` planes of n_bytes, `stride` bytes apart"""
    return pl.aligned_bytes(pl.GUARD + (frames - 1) * stride + n_bytes + pl.GUARD, fill=pl.FILL)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("sub", [420, 422])
def test_uyvy_coefficient_front_ends(hip, po, sub, size):
    """ug_hip_uyvy_to_jpeg420_coeffs / _422_ at every source layout, and _42x_coeffs_batch with frame strides for the source, the luma and the chroma
    planes that leave gaps: coefficients == the oracle's, the gaps and guards keep FILL"""
    import torch
    L = hip.L
    w, h = size
    line = line_of(hip, "UYVY", w)
    frames = _frames("UYVY", line, w, h)
    ql, qc = po.jpeg_qtable(Q, 0), po.jpeg_qtable(Q, 1)
    want = [_coefs42x(po, f, w, h, sub, ql, qc) for f in frames]
    div = hip.jpeg_divisors_device(Q, "cuda")
    ny, nc = want[0][0].size * 2, want[0][1].size * 2   # bytes of a luma / chroma plane
    ys, cs = ny + 32, nc + 48                           # frame strides of the planes: multiples of 16, with gaps
    single = {420: L.load().ug_hip_uyvy_to_jpeg420_coeffs, 422: L.load().ug_hip_uyvy_to_jpeg422_coeffs}[sub]
    problems = []
    for lname, parg, pitch, off in layouts("UYVY", line):
        for extra in (80, 12):
            stride = pitch * h + extra
            dev = _upload(pl.place_frames(frames, line, h, pitch, off, stride, np.random.default_rng(pitch + extra)))
            for n in ((1, FRAMES) if extra == 80 else (FRAMES,)):
                outs = [_upload(_i16_dst(nb, n, st)) for nb, st in ((ny, ys), (nc, cs), (nc, cs))]
                ptrs = [o.data_ptr() + pl.GUARD for o in outs]
                if n == 1:
                    rc = single(dev.data_ptr() + off, parg, w, h, div.data_ptr(), *ptrs, _stream())
                else:
                    rc = L.load().ug_hip_uyvy_to_jpeg42x_coeffs_batch(sub, dev.data_ptr() + off, parg, w, h, div.data_ptr(), *ptrs, n, stride, ys, cs, _stream())
                torch.cuda.synchronize()
                tag = (lname, pitch, off, n, extra)
                if rc != 0:
                    problems.append((tag, "rc", rc, L.last_error()))
                    continue
                for c, (o, nb, st) in enumerate(zip(outs, (ny, nc, nc), (ys, cs, cs))):
                    exp = _i16_dst(nb, n, st)
                    for f in range(n):
                        exp[pl.GUARD + f * st: pl.GUARD + f * st + nb] = want[f][c].view(np.uint8).ravel()
                    found = pl.compare_frames(o.cpu().numpy(), exp, n, st, 1, nb, nb, pl.GUARD)
                    if found:
                        problems.append((tag, "Y Cb Cr".split()[c], found))
    assert not problems, (sub, size, problems)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_plane_fdct_at_pitches_and_base_offsets(hip, po, size):
    """ug_hip_jpeg_fdct_quant_plane: pitch == width, roundup8(width) + 8 (the 8-byte tier with padding behind the line) and width + 3 (bytes), the
    plane at an aligned address and one byte further on"""
    import torch
    L = hip.L
    w, h = size
    plane = np.random.default_rng([w, h]).integers(0, 256, w * h, dtype=np.uint8)
    div = po.jpeg_divisors(po.jpeg_qtable(Q, 0))
    want = po.jpeg_fdct_quant_plane(plane.reshape(h, w), div)
    ddiv = torch.from_numpy(div).cuda()
    bw, bh = (w + 7) // 8, (h + 7) // 8
    problems = []
    for pitch in (w, (w + 7) // 8 * 8 + 8, w + 3):
        for off in (0, 1):
            dev = _upload(pl.place_frames([plane], w, h, pitch, off, 0, np.random.default_rng(pitch + off)))
            out = _upload(_i16_dst(want.size * 2, 1, 0))
            rc = L.load().ug_hip_jpeg_fdct_quant_plane(dev.data_ptr() + off, pitch, w, h, bw, bh, ddiv.data_ptr(), out.data_ptr() + pl.GUARD, None, _stream())
            torch.cuda.synchronize()
            if rc != 0:
                problems.append((pitch, off, "rc", rc, L.last_error()))
                continue
            exp = _i16_dst(want.size * 2, 1, 0)
            exp[pl.GUARD: pl.GUARD + want.size * 2] = want.view(np.uint8).ravel()
            found = pl.compare_frames(out.cpu().numpy(), exp, 1, 0, 1, want.size * 2, want.size * 2, pl.GUARD)
            if found:
                problems.append((pitch, off, found))
    assert not problems, (size, problems)


def dst_layouts(fmt, line):
    """-> [(name, pitch argument, pitch, base offset)] of a destination: never the pitch the source has in the same position of layouts()"""
    e = 1 if fmt == "RGB" else 4
    p16 = r16(line) + 32
    wp = line + 4 + (4 if (line + 4) % 16 == 0 else 0)
    out = [("padded16", p16, p16, 0), ("word_pitch", wp, wp, 0), ("packed", 0, line, 0)]
    if fmt == "RGB":
        out.append(("dst_off", p16, p16, e))
        out.append(("odd_pitch", line + 13, line + 13, 1))
    else:
        out.append(("dst_off", p16, p16, e))
    return out


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", ["RGB", "UYVY"])
def test_colour_stage_at_different_pitches(hip, po, fmt, size):
    """ug_hip_jpeg_colour_convert with a source and a destination pitch that differ: the lines == the oracle's on the packed frame, the padding of
    every destination line and the canaries around the destination keep FILL"""
    import torch
    L = hip.L
    w, h = size
    line = line_of(hip, fmt, w)
    frame = _frames(fmt, line, w, h)[0]
    cs_in, cs_out = (CS_RGB, Y601FULL) if fmt == "RGB" else (Y709, Y601)
    packed = po.jpeg_colour_convert(fmt, cs_in, cs_out, frame, w, h).reshape(h, line)
    problems = []
    for (sname, sarg, sp, so), (dname, darg, dp, do) in zip(layouts(fmt, line), dst_layouts(fmt, line)):
        assert sp != dp
        dev = _upload(pl.place_frames([frame], line, h, sp, so, 0, np.random.default_rng(sp + so)))
        dst, front = pl.make_dst(h, dp, do)
        want = dst.copy()
        for y in range(h):
            want[front + y * dp: front + y * dp + line] = packed[y]
        ddst = _upload(dst)
        rc = L.load().ug_hip_jpeg_colour_convert(L.PF_NAMES[fmt], cs_in, cs_out, dev.data_ptr() + so, sarg, ddst.data_ptr() + front, darg, w, h, _stream())
        torch.cuda.synchronize()
        found = [("rc", rc, L.last_error())] if rc != 0 else pl.compare(ddst.cpu().numpy(), want, h, dp, line, front)
        if found:
            problems.append((sname, dname, (sp, dp, so, do), found))
    assert not problems, (fmt, size, problems)


# ---------------------------------------------------------------------- the rule ----------------------------------------------------------------------
def _owned(n_bytes, margin, rng=None):
    """a device buffer with `margin` owned bytes on both sides of the n_bytes a call is given: -> (tensor, offset of the middle, 16-byte aligned)"""
    import torch
    margin = r16(margin)
    if rng is None:
        t = torch.full((2 * margin + n_bytes,), pl.FILL, dtype=torch.uint8, device="cuda")
    else:
        t = torch.from_numpy(np.frombuffer(rng.bytes(2 * margin + n_bytes), np.uint8).copy()).cuda()
    assert t.data_ptr() % 256 == 0
    return t, margin


REFUSED = {"UYVY": ("uyvy422", 422, ()), "UYVY444": ("uyvy444", 444, ("JPEG_INPUT_UYVY",)), "RGB": ("rgb444", 444, ()), "RGBA": ("rgba4444", 4444, ())}


@pytest.mark.parametrize("kind", list(REFUSED))
def test_refused_pitches_and_addresses(hip, po, kind):
    """src_pitch below the line, a negative one, and -- UYVY and RGBA -- a pitch, a base or a batch stride that is no multiple of 4: UG_HIP_EINVAL
    with restart interval 4 (the fused coder's) and 7 alike, and the output is still all FILL.  Every pointer lies in the middle of one
    allocation with |pitch| * height + 4096 owned bytes on both sides: a call wrongly accepted reads and writes only memory of the test's."""
    import torch
    L = hip.L
    _, sub, flags = REFUSED[kind]
    fmt = "UYVY" if kind.startswith("UYVY") else kind
    w, h = 48, 16
    line = line_of(hip, fmt, w)
    p16 = r16(line) + 16
    cases = [("below the line", line - (4 if fmt != "RGB" else 1), 0, 1, 0), ("pitch 1 or 4", 1 if fmt == "RGB" else 4, 0, 1, 0),
             ("negative", -r16(line), 0, 1, 0), ("negative, batch", -r16(line), 0, 2, r16(line) * h)]
    if fmt != "RGB":
        cases += [("pitch % 4 == 2", p16 + 2, 0, 1, 0), ("pitch % 4 == 1", p16 + 1, 0, 1, 0), ("base + 2", p16, 2, 1, 0), ("base + 1", p16, 1, 1, 0),
                  ("stride % 4 == 2", p16, 0, 2, p16 * h + 2)]
    problems = []
    for ri in (4, 7):
        enc = hip.JpegEncoder(w, h, Q, ri, subsampling=sub, flags=sum(getattr(L, f) for f in flags))
        cap = enc.max_size
        for what, pitch, off, n, stride in cases:
            margin = abs(pitch) * h + 4096 + (stride if n > 1 else 0)
            src, mid = _owned(p16 * h * n, margin, np.random.default_rng(7))
            out, omid = _owned(r16(cap) * n, 4096)
            lens = (C.c_size_t * n)()
            if n == 1:
                rc = L.load().ug_hip_jpeg_encoder_encode(enc._h, L.PF_NAMES[fmt], src.data_ptr() + mid + off, pitch, out.data_ptr() + omid, cap, lens, _stream())
            else:
                rc = L.load().ug_hip_jpeg_encoder_encode_batch(enc._h, L.PF_NAMES[fmt], n, src.data_ptr() + mid + off, pitch, stride, out.data_ptr() + omid, r16(cap), cap,
                                                               lens, _stream())
            torch.cuda.synchronize()
            if rc != L.EINVAL:
                problems.append((ri, what, "not refused", rc))
            if not bool((out == pl.FILL).all()):
                problems.append((ri, what, "the output was written"))
        enc.close()
    assert not problems, (kind, problems)


def test_refused_i420_pitch(hip):
    """planar I420 is tightly packed: src_pitch 0 or the width, anything else UG_HIP_EINVAL with nothing written -- fused (restart interval 4) or not"""
    import torch
    L = hip.L
    w, h = 48, 16
    for ri in (4, 7):
        enc = hip.JpegEncoder(w, h, Q, ri, subsampling=420)
        src, mid = _owned((w + 16) * h * 2, (w + 16) * h + 4096, np.random.default_rng(1))
        for pitch, rc_want in ((w + 16, L.EINVAL), (w, 0), (0, 0)):
            out, omid = _owned(r16(enc.max_size), 4096)
            n = C.c_size_t(0)
            rc = L.load().ug_hip_jpeg_encoder_encode(enc._h, L.PF_I420, src.data_ptr() + mid, pitch, out.data_ptr() + omid, enc.max_size, C.byref(n), _stream())
            torch.cuda.synchronize()
            assert rc == rc_want, (ri, pitch, rc)
            assert rc == 0 or bool((out == pl.FILL).all()), (ri, pitch)
        enc.close()
