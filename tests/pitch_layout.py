"""Pitched and offset buffers for the tests of the pitch / alignment arguments of the C ABI (ug_hip_pixfmt_convert[_batch],
ug_hip_dxt_decode): the layouts, the reference conversion run line by line on the very same pitched bytes, and the byte-for-byte
comparison with canaries in front of the buffer, behind it and in the padding of every line; and, for the JPEG encoder and decoder
(tests/test_gpu_jpeg_pitch.py, tests/test_gpu_jpeg_decode_pitch.py), the source side: packed frames placed at a pitch, an offset and a frame
stride among random bytes (place_frames).  Plain numpy + ctypes, no GPU: the helper's own checks are tests/test_pitch_layout.py."""
import ctypes as C
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FILL = 0xA5    # every destination byte beforehand, on both sides: what a converter leaves alone must still hold it
GUARD = 256    # canary bytes in front of and behind a destination
SLACK = 256    # source bytes behind the last line: converters read past a line's last pixel (MAX_PADDING is 64), both sides see the same
SHIFTS = [(0, 8, 16), (16, 8, 0)]
DEC = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int)

# the 17 pairs of csrc/pixfmt.hip (the others: csrc/pixfmt_ext.hip) -- the ones oracle/pixfmt_oracle.c restates
CORE_PAIRS = [("BGR", "RGB"), ("BGR", "UYVY"), ("RG48", "UYVY"), ("RGB", "RGB"), ("RGB", "RGBA"), ("RGB", "UYVY"), ("RGBA", "RGB"),
              ("RGBA", "RGBA"), ("RGBA", "UYVY"), ("UYVY", "RGB"), ("UYVY", "RGBA"), ("UYVY", "YUYV"), ("UYVY", "v210"),
              ("YUYV", "UYVY"), ("v210", "RG48"), ("v210", "RGB"), ("v210", "UYVY")]
COPIES = [("UYVY", "UYVY"), ("v210", "v210"), ("YUYV", "YUYV")]


def decoder_pairs():
    """decoders[] of the reference (tests/golden/reference_tables.json): 61 pairs"""
    with open(os.path.join(HERE, "golden", "reference_tables.json")) as f:
        return [tuple(p) for p in json.load(f)["pixfmt_decoders"]]


def all_pairs():
    """decoders[] plus the identity copies get_decoder_from_to() answers with vc_memcpy (RGB -> RGB and RGBA -> RGBA are in decoders[])"""
    pairs = decoder_pairs()
    return pairs + [p for p in COPIES if p not in pairs]


# widths a pair's reference function cannot take: vc_copylineDVS10 moves 64-bit words of a line whose length it derives from dst_len / 1.5
# (tests/test_gpu_pixfmt_ext.py::test_dvs10_to_uyvy keeps to widths whose lines hold whole ones)
def width_ok(i, o, w):
    return not ((i, o) == ("DVS10", "UYVY") and w % 48)


def natural_align(fmt, dst):
    """the alignment a format's own samples have: 32-bit words, 16-bit samples, or bytes"""
    if fmt in ("v210", "DVS10", "RGBA", "VUYA", "UYVY", "YUYV") or (fmt == "R10k" and dst):
        return 4
    return 2 if fmt in ("RG48", "Y216", "Y416") else 1


def ext_rule(i, o):
    """(source, destination) alignment of base and pitch that csrc/pixfmt_ext.hip: pixfmt_ext_convert asks of a pair: the 16- and 32-bit
    formats it addresses as such (the reference asserts the same); everything else is read and written bytewise"""
    s = 4 if i in ("v210", "DVS10") else 2 if i in ("RG48", "Y216", "Y416") else 1
    if o in ("RG48", "Y216", "Y416"):
        d = 2
    elif o in ("RGB", "R12L") or (o == "R10k" and i in ("R12L", "Y416")):
        d = 1
    else:
        d = 4
    return s, d


class Sizes:
    """line sizes of a pair at a width: from the compiled reference where it is there, else from the restatement (core formats only)"""

    def __init__(self, po, i, o, w):
        if po.have_ref():
            r = po.ref()
            r.get_codec_from_name.argtypes = [C.c_char_p]
            ci, co = r.get_codec_from_name(i.encode()), r.get_codec_from_name(o.encode())
            self.src_line, self.src_size = r.vc_get_linesize(w, ci), r.vc_get_size(w, ci)
            self.dst_line, self.dst_size = r.vc_get_linesize(w, co), r.vc_get_size(w, co)
        else:
            l = po.lib()
            self.src_line, self.src_size = l.oracle_linesize(w, po.OPF[i]), l.oracle_size(w, po.OPF[i])
            self.dst_line, self.dst_size = l.oracle_linesize(w, po.OPF[o]), l.oracle_size(w, po.OPF[o])
        self.written_len = self.dst_size


def ref_lib(po, i, o):
    """the compiled reference a pair is held to: its portable build for the pairs of csrc/pixfmt.hip, as tests/test_gpu_pixfmt.py does (the
    SSSE3 branch of vc_copylineRGBAtoRGB never advances `src` in its tail loop, pixfmt_conv.c:889-895; oracle/Makefile), the default
    build for the others, as tests/test_gpu_pixfmt_ext.py does"""
    r = po.ref(scalar=(i, o) in CORE_PAIRS)
    r.get_codec_from_name.argtypes = [C.c_char_p]
    return r


def restated(i, o):
    """pairs oracle/pixfmt_oracle.c restates: what is checked where oracle/_ref is absent"""
    return (i, o) in CORE_PAIRS or (i, o) in COPIES


def line_converter(po, i, o, use_ref=None):
    """-> f(dst address, src address, dst_len, rshift, gshift, bshift): the pair's decoder_t of the compiled reference (ref_lib) or, where
    oracle/_ref is absent (use_ref False: on demand), its restatement oracle_convert_line -- the same call shape, the same pitched bytes,
    so bytes a converter leaves alone inside dst_len stay FILL with either"""
    if po.have_ref() if use_ref is None else use_ref:
        r = ref_lib(po, i, o)
        fn = r.get_decoder_from_to(r.get_codec_from_name(i.encode()), r.get_codec_from_name(o.encode()))
        assert fn, (i, o)
        return DEC(fn)
    if not restated(i, o):
        raise LookupError(f"no restatement of {i}->{o}")
    line, fi, fo = po.lib().oracle_convert_line, po.OPF[i], po.OPF[o]

    def f(dst, src, dst_len, rs, gs, bs):
        assert line(fi, fo, dst, src, dst_len, rs, gs, bs) == 0, (i, o)
    return f


LAYOUTS = ["padded16", "odd_pitch", "src_off", "dst_off"]


def layout(name, i, o, sz):
    """-> (src_pitch, dst_pitch, src_off, dst_off); offsets are those of the bases from a 256-byte aligned address"""
    sp, dp = max(sz.src_line, sz.src_size), max(sz.dst_line, sz.dst_size)
    if name == "packed":
        return sp, dp, 0, 0
    if name == "odd_pitch":  # lines start at every residue the format allows: no 128-bit tier
        sp, dp = sp + natural_align(i, False), dp + natural_align(o, True)
        if sp % 16 == 0:
            sp += natural_align(i, False)
        if dp % 16 == 0:
            dp += natural_align(o, True)
        return sp, dp, 0, 0
    sp, dp = (sp + 15) // 16 * 16 + 16, (dp + 15) // 16 * 16 + 32
    return sp, dp, natural_align(i, False) if name == "src_off" else 0, natural_align(o, True) if name == "dst_off" else 0


def aligned_bytes(n, fill=None, rng=None):
    """n bytes at a 256-byte aligned address"""
    buf = np.empty(n + 256, np.uint8)
    off = (-buf.ctypes.data) % 256
    v = buf[off: off + n]
    if rng is not None:
        v[:] = np.frombuffer(rng.bytes(n), np.uint8)
    else:
        v[:] = 0 if fill is None else fill
    return v


def make_src(h, src_pitch, src_off, rng):
    """random bytes everywhere: the lines, their padding and what follows the picture"""
    return aligned_bytes(src_off + src_pitch * h + SLACK, rng=rng)


def frame_mask(frames, line, h, pitch, off, stride, size):
    """the bytes of a buffer of `size` bytes that belong to the lines of `frames` pictures (place_frames): a bool array"""
    inside = np.zeros(size, bool)
    at = off + (np.arange(frames)[:, None, None] * stride + np.arange(h)[None, :, None] * pitch + np.arange(line)[None, None, :])
    inside[at.ravel()] = True
    return inside


def place_frames(frames_packed, line, h, pitch, off, stride, rng):
    """Source side: the packed frames (each h lines of `line` bytes) laid out `stride` bytes apart at `pitch` bytes per line, the first one `off`
    bytes into a 256-byte aligned buffer.  Every other byte is random (rng.bytes): the `off` bytes in front, the padding of every line, the gaps
    between the frames and SLACK bytes behind the last line -- a kernel that reads padding as pixels, or replicates an edge from the padding
    instead of the last pixel, computes something else."""
    n = len(frames_packed)
    assert pitch >= line and (n == 1 or stride >= pitch * h)
    buf = aligned_bytes(off + (n - 1) * stride + pitch * h + SLACK, rng=rng)
    for f, frame in enumerate(frames_packed):
        rows = np.asarray(frame, np.uint8).reshape(-1)[: line * h].reshape(h, line)
        for y in range(h):
            at = off + f * stride + y * pitch
            buf[at: at + line] = rows[y]
    return buf


def extract_frames(buf, frames, line, h, pitch, off, stride):
    """the packed frames back out of a buffer place_frames made"""
    return [np.stack([buf[off + f * stride + y * pitch: off + f * stride + y * pitch + line] for y in range(h)]).ravel() for f in range(frames)]


def make_dst(h, dst_pitch, dst_off):
    """-> (buffer of FILL, front): the picture starts `front` bytes in; the bytes before it and GUARD bytes behind it are canaries"""
    front = GUARD + dst_off
    return aligned_bytes(front + dst_pitch * h + GUARD, fill=FILL), front


def ref_convert_pitched(po, i, o, src, src_off, w, h, src_pitch, dst_pitch, sh, dst_off=0, scratch=False, use_ref=None):
    """The reference at these pitches: the pair's line converter (line_converter: get_decoder_from_to() of the compiled reference; without
    oracle/_ref the restatement, core pairs and copies only) once per line at dst + y * dst_pitch, src + y * src_pitch with
    dst_len = vc_get_size(width, out), on the pitched bytes themselves (what follows a line is what the converter reads past its last
    pixel) and into a destination of FILL.
    scratch: every line (with the SLACK bytes that follow it) is converted at an aligned address of its own and copied into place -- for
    pitches the host's converters cannot be pointed at (a line of 32-bit words at an odd address).
    -> (want buffer, front), laid out as make_dst() lays out the destination."""
    sz = Sizes(po, i, o, w)
    want, front = make_dst(h, dst_pitch, dst_off)
    dec = line_converter(po, i, o, use_ref)
    if scratch:
        room = sz.written_len + SLACK
        for y in range(h):
            s = aligned_bytes(sz.src_line + SLACK)
            part = src[src_off + y * src_pitch: src_off + y * src_pitch + s.size]
            s[: part.size] = part
            d = aligned_bytes(room, fill=FILL)
            dec(d.ctypes.data, s.ctypes.data, sz.written_len, *sh)
            want[front + y * dst_pitch: front + y * dst_pitch + sz.written_len] = d[: sz.written_len]
        return want, front
    sp0, dp0 = src.ctypes.data + src_off, want.ctypes.data + front
    for y in range(h):
        dec(dp0 + y * dst_pitch, sp0 + y * src_pitch, sz.written_len, *sh)
    return want, front


def compare(got, want, h, dst_pitch, written_len, front=GUARD):
    """got, want: whole destination buffers, canaries included, the picture `front` bytes in.  Findings (empty = equal):
    bytes [0, written_len) of every line differ; a byte of [written_len, dst_pitch) of a line is no longer FILL; a canary in front of or
    behind the buffer is no longer FILL.  (`want` is only read inside the lines: what a reference spills behind dst_len is its own.)"""
    got, want = np.asarray(got), np.asarray(want)
    out = []
    if got.size != want.size or got.size < front + h * dst_pitch:
        return [f"buffer sizes: got {got.size}, want {want.size}, picture needs {front + h * dst_pitch}"]
    end = front + h * dst_pitch
    g, wv = got[front:end].reshape(h, dst_pitch), want[front:end].reshape(h, dst_pitch)
    bad = g[:, :written_len] != wv[:, :written_len]
    if bad.any():
        ys, xs = np.nonzero(bad)
        out.append(f"{int(bad.sum())} bytes differ inside the lines; first at line {int(ys[0])} byte {int(xs[0])}; "
                   f"bytes of a line: {sorted(set(xs.tolist()))[:16]}; lines: {sorted(set(ys.tolist()))[:8]}")
    pad = g[:, written_len:] != FILL
    if pad.any():
        ys, xs = np.nonzero(pad)
        out.append(f"{int(pad.sum())} padding bytes written; first at line {int(ys[0])} byte {written_len + int(xs[0])}")
    for name, part, base in (("in front of", got[:front], 0), ("behind", got[end:], end)):
        hit = np.flatnonzero(part != FILL)
        if hit.size:
            out.append(f"{hit.size} canary bytes {name} the buffer written; first at {base + int(hit[0]) - front} from the picture's start")
    return out


def compare_frames(got, want, frames, stride, h, dst_pitch, written_len, front=GUARD):
    """compare() for `frames` pictures `stride` bytes apart: the bytes of the lines equal `want`, every other byte of the buffer -- line
    padding, the gaps between the frames, the canaries at both ends -- is still FILL"""
    got, want = np.asarray(got), np.asarray(want)
    if got.size != want.size or got.size < front + (frames - 1) * stride + h * dst_pitch:
        return [f"buffer sizes: got {got.size}, want {want.size}"]
    inside = np.zeros(got.size, bool)
    at = front + (np.arange(frames)[:, None, None] * stride + np.arange(h)[None, :, None] * dst_pitch + np.arange(written_len)[None, None, :])
    inside[at.ravel()] = True
    out = []
    bad = np.flatnonzero(inside & (got != want))
    if bad.size:
        out.append(f"{bad.size} bytes differ inside the lines; first at {int(bad[0]) - front} from the first picture's start")
    hit = np.flatnonzero(~inside & (got != FILL))
    if hit.size:
        out.append(f"{hit.size} bytes outside the lines written; first at {int(hit[0]) - front} from the first picture's start")
    return out
