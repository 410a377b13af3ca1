"""Frame layouts for the tests of the lavc converters' line sizes and plane addresses (ug_hip_uv_to_av / ug_hip_av_to_uv, csrc/lavc_conv.hip
and the rows it forwards): the layouts FFmpeg hands out beyond its default allocator's -- tight lines, lines a sample or two longer, planes
a sample past an aligned address -- made by the layout switch of the FFmpeg stand-in (oracle/lavc_stub: ug_stub_set_frame_layout), the
compiled reference run on exactly those bytes, a device mirror of whole allocations (guards, padding, spare line) at congruent addresses,
and the byte-for-byte comparison with canaries.  Modelled on tests/pitch_layout.py.  Plain numpy + ctypes, no GPU: the helper's own checks
are tests/test_lavc_layout.py; `python lavc_layout.py to|from` runs the reference over every case in a process of its own."""
import ctypes as C
import json
import sys

import numpy as np

import test_lavc_conv as T
from pitch_layout import FILL, GUARD, aligned_bytes

MODES = {"default": 0, "tight": 1, "odd": 2, "offset": 3, "last_plane_off": 4}  # ug_lavc_stub.h
LAYOUTS = ["tight", "odd", "offset"]
# the smallest sizes that reach each hazard: a fast-eligible width of many workgroups, a fast-eligible width with an odd height, a width
# ragged for 6-, 8- and 16-pixel groups, an odd pair count with one partial v210 group
SIZES = [(1920, 2), (96, 5), (50, 7), (18, 3)]
DST_UNIT = 4  # destinations of av_to_uv: the reference asserts 4-byte alignment even for RGB (from_lavc_vid_conv.c:1283)

# rows with an 8-pixels-per-lane kernel (csrc/lavc_conv.hip: the `fast` column of kToAv / kFromAv; yuvj* take the rows of yuv*)
FAST_TO = [("UYVY", "yuv444p"), ("UYVY", "yuvj444p"), ("v210", "yuv420p10le"), ("v210", "yuv422p10le"), ("RGB", "gbrp"), ("RGBA", "gbrp")]
FAST_FROM = [("yuv420p10le", "v210"), ("p210le", "v210"), ("p010le", "v210"), ("yuv420p", "v210"), ("yuv420p", "RGB"), ("yuv420p", "RGBA"),
             ("yuv422p", "v210"), ("yuv422p", "RGB"), ("yuv422p", "RGBA"), ("yuvj420p", "RGB"), ("yuvj422p", "RGBA"),
             ("nv12", "UYVY"), ("nv12", "RGB"), ("nv12", "RGBA")]
# rows whose kernels read their destination (k_r10k_to_yuv42Xp10le<2>: odd pairs average with what the chroma planes hold); the 4:2:2 twin
# shares the kernel and must not
READS_DST = [("R10k", "yuv420p10le"), ("R10k", "yuv422p10le")]


def frame_unit(av):
    """frame_align() of csrc/lavc_conv.hip: bytes per sample of a frame format's planes as the kernels address them"""
    if any(s in av for s in ("xv30", "vuy", "x2rgb")):
        return 4
    if any(s in av for s in ("10le", "12le", "16le", "48le", "y21", "ayuv64")):
        return 2
    return 1


def ref(lib=None):
    """the compiled reference (or another build of it with the stand-in inside, e.g. the hook build) with the layout functions typed"""
    r = lib if lib is not None else T.ref()
    r.ug_stub_set_frame_layout.restype = None
    r.ug_stub_set_frame_layout.argtypes = [C.c_int, C.c_int, C.c_int]
    r.ug_stub_plane_line_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    r.ug_stub_plane_span.argtypes = [C.POINTER(T.StubAVFrame), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    r.ug_stub_format_count.restype = C.c_int
    r.ug_stub_format_name.restype = C.c_char_p
    r.ug_stub_format_name.argtypes = [C.c_int]
    return r


class laid_out:
    """with laid_out(r, "tight", unit): frames allocated inside have that layout; the default comes back afterwards"""

    def __init__(self, r, layout, unit, fill=FILL):
        self.r, self.args = r, (MODES[layout], unit, fill)

    def __enter__(self):
        self.r.ug_stub_set_frame_layout(*self.args)

    def __exit__(self, *exc):
        self.r.ug_stub_set_frame_layout(0, 1, 0)


class Plane:
    """one plane of a stub frame: `whole` = its allocation (front guard, lines, padding, spare line, back guard), the lines `off` bytes in"""

    def __init__(self, whole, off, ls, rows, addr):
        self.whole, self.off, self.ls, self.rows, self.addr = whole, off, ls, rows, addr  # addr: host address of the first line

    def lines(self, spare=False):
        n = self.rows + (1 if spare else 0)
        return self.whole[self.off: self.off + n * self.ls].reshape(n, self.ls)

    def copy(self):
        return Plane(self.whole.copy(), self.off, self.ls, self.rows, self.addr)


def frame_planes(r, fr, h):
    """live views of the planes of a stub frame (valid until the frame is freed)"""
    out = []
    for i in range(4):
        if not fr.data[i]:
            break
        base, size = C.c_void_p(), C.c_size_t()
        assert r.ug_stub_plane_span(C.byref(fr), i, C.byref(base), C.byref(size)) == 0
        whole = np.ctypeslib.as_array(C.cast(base, C.POINTER(C.c_uint8)), shape=(size.value,))
        out.append(Plane(whole, fr.data[i] - base.value, fr.linesize[i], r.ug_stub_plane_rows(fr.format, i, h), fr.data[i]))
    return out


def to_av_height(uv, av, h):
    """the reference's v210_to_yuv420p10le reads and writes one line past an odd-height picture (to_lavc_vid_conv.c:204-208): even heights, as
    tests/test_lavc_conv.py::test_gpu_uv_to_av_random_sizes has it"""
    return h + h % 2 if (uv, av) == ("v210", "yuv420p10le") else h


def to_av_masked(uv, av, layout):
    """y216_to_p010le finds the odd luma line by running on from the even one (to_planar.c:191-199): with a line size beyond 2 * width bytes
    it writes that line into the even line's padding.  Those cases are held to oracle/planar_oracle.py, as test_gpu_uv_to_av does."""
    return (uv, av) == ("Y216", "p010le") and layout != "tight"


def from_av_masked(uv, w):
    """the reference packs uninitialised stack behind a ragged R12L line end (from_planar.c:74-82, from_lavc_vid_conv.c:391-433 write whole
    groups of 8): only the bits of real pixels are compared"""
    return uv == "R12L" and w % 8 != 0


def make_uv_source(r, uv, w, h, seed):
    """random bytes for a packed source of vc_get_linesize() lines, one spare line and 64 bytes behind it (converters read whole groups)"""
    ls = r.vc_get_linesize(w, r.get_codec_from_name(uv.encode()))
    return aligned_bytes(ls * (h + 1) + 64, rng=np.random.default_rng(seed))


def ref_uv_to_av_laid_out(r, uv, av, srcs, w, h, layout, fill=FILL):
    """to_lavc_vid_conv() of the compiled reference into a frame of `layout`, once per source in `srcs`, one after the other into the same
    frame as the reference reuses it.  -> [planes before the first call (all `fill`), planes after call 1, after call 2, ...], each a list
    of Plane copies (whole allocations)"""
    with laid_out(r, layout, frame_unit(av), fill):
        st = r.to_lavc_vid_conv_init(r.get_codec_from_name(uv.encode()), w, h, r.ug_stub_pixfmt_by_name(av.encode()), 1)
    assert st, (uv, av, "the reference has no such conversion")
    states = []
    for src in srcs:
        frp = r.to_lavc_vid_conv(st, src.ctypes.data)
        assert frp and frp.contents.stub_buf[0], (uv, av, "the reference returned no frame of its own")
        planes = [p.copy() for p in frame_planes(r, frp.contents, h)]
        if not states:
            first = [p.copy() for p in planes]
            for p in first:
                p.whole[:] = fill
            states.append(first)
        states.append(planes)
    stp = C.c_void_p(st)
    r.to_lavc_vid_conv_destroy(C.byref(stp))
    return states


def make_frame_laid_out(r, av, w, h, layout, seed, colorspace, color_range, fill=FILL):
    """a stub frame of `layout` whose lines, padding and spare line hold random samples of the format's depth; the guards hold `fill`"""
    with laid_out(r, layout, frame_unit(av), fill):
        frp = r.ug_stub_frame_new(r.ug_stub_pixfmt_by_name(av.encode()), w, h)
    assert frp, av
    fr = frp.contents
    fr.colorspace, fr.color_range = colorspace, color_range
    rng = np.random.default_rng(seed)
    d = T.depth_of(av)
    for p in frame_planes(r, fr, h):
        v = p.lines(spare=True)
        if d == 8 or av in ("xv30le", "y210le", "y212le", "ayuv64le", "rgb48le"):
            v[:] = rng.integers(0, 256, v.shape)
        else:
            s = rng.integers(0, 1 << d, (v.shape[0], v.shape[1] // 2)).astype("<u2")
            if av in ("p010le", "p210le"):
                s = s << 6
            v[:] = s.view(np.uint8)
    return frp


def dst_layout(layout, line):
    """the destination a source layout is paired with -> (pitch, offset of the base from a 256-byte aligned address)"""
    if layout in ("tight", "default"):
        return line, 0
    if layout == "odd":
        pitch = line + DST_UNIT
        return (pitch + DST_UNIT if pitch % 16 == 0 else pitch), 0
    return (line + 63) // 64 * 64 + 64, DST_UNIT


def make_dst(h, pitch, off, fill=FILL):
    """-> (buffer of `fill` at a 256-byte aligned address, front): h lines and a spare one `front` bytes in, GUARD canary bytes at each end"""
    front = GUARD + off
    return aligned_bytes(front + pitch * (h + 1) + GUARD, fill=fill), front


def ref_av_to_uv_laid_out(r, frp, av, uv, h, pitch, off, shifts, fill=FILL):
    """av_to_uv_convert() of the compiled reference from the frame as it lies into a destination of `fill` -> (whole buffer, front)"""
    conv = r.get_av_to_uv_conversion(r.ug_stub_pixfmt_by_name(av.encode()), r.get_codec_from_name(uv.encode()))
    assert conv, (av, uv, "the reference has no such conversion")
    want, front = make_dst(h, pitch, off, fill)
    r.av_to_uv_convert(conv, want.ctypes.data + front, frp, pitch, (C.c_int * 3)(*shifts))
    cp = C.c_void_p(conv)
    r.av_to_uv_conversion_destroy(C.byref(cp))
    return want, front


# ---- the device side -------------------------------------------------------------------------------------------------------------------
def mirror_bytes(torch, host, addr=None, device="cuda"):
    """a device (or, for the helper's own test, CPU) byte tensor holding `host`, at an address congruent to `addr` (default: host's own)
    modulo 256"""
    addr = host.ctypes.data if addr is None else addr
    buf = torch.empty(host.size + 256, dtype=torch.uint8, device=device)
    skip = (addr - buf.data_ptr()) % 256
    view = buf[skip: skip + host.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(host)))
    return view


def mirror_planes(torch, planes, device="cuda"):
    """whole allocations of `planes` copied to the device -> (whole tensors, plane views for codec.uv_to_av / av_to_uv): a view's data_ptr()
    is congruent to the host plane's address modulo 256 and its stride(0) is the line size"""
    wholes, views = [], []
    for p in planes:
        t = mirror_bytes(torch, p.whole, p.addr - p.off, device)
        wholes.append(t)
        views.append(t[p.off: p.off + p.rows * p.ls].view(p.rows, p.ls))
    return wholes, views


def _where(bad):
    ys, xs = np.nonzero(bad)
    return f"first at line {int(ys[0])} byte {int(xs[0])}; bytes of a line: {sorted(set(xs.tolist()))[:12]}; lines: {sorted(set(ys.tolist()))[:8]}"


def compare_planes(got_wholes, want, fill=FILL, line_bytes=None, spare_was=None):
    """got_wholes: whole allocations as the product left them (numpy), want: the reference's Planes.  Findings (empty = equal): a byte of
    [0, linesize) of a line differs (line_bytes[k]: only the first so many bytes are held to `want`, the rest of the line to `fill`); a guard
    byte in front of the first line or behind the spare line is no longer `fill`.  What the reference spills into the spare line is its
    own and not compared; the product's planes end with their last line, so its spare line must still hold what it held (spare_was[k],
    default `fill`)."""
    out = []
    for k, (g, p) in enumerate(zip(got_wholes, want)):
        g = np.asarray(g)
        if g.size != p.whole.size:
            out.append(f"plane {k}: sizes {g.size} / {p.whole.size}")
            continue
        gl, wl = g[p.off: p.off + p.rows * p.ls].reshape(p.rows, p.ls), p.lines()
        n = p.ls if line_bytes is None else line_bytes[k]
        bad = gl[:, :n] != wl[:, :n]
        if bad.any():
            out.append(f"plane {k}: {int(bad.sum())} bytes differ inside the lines; {_where(bad)}")
        pad = gl[:, n:] != fill
        if pad.any():
            out.append(f"plane {k}: {int(pad.sum())} padding bytes written; {_where(pad)}")
        end = p.off + (p.rows + 1) * p.ls
        spare = g[end - p.ls: end] != (fill if spare_was is None else spare_was[k])
        if spare.any():
            out.append(f"plane {k}: {int(spare.sum())} bytes behind the last line written; first at byte {int(np.flatnonzero(spare)[0])}")
        for name, part in (("in front of", g[: p.off]), ("behind", g[end:])):
            hit = np.flatnonzero(part != fill)
            if hit.size:
                out.append(f"plane {k}: {hit.size} guard bytes {name} the plane written; first at {int(hit[0])}")
    return out


def compare_dst(got, want, h, pitch, front, fill=FILL, r12l_width=0):
    """whole destination buffers of av_to_uv: bytes [0, pitch) of each of the h lines equal the reference's, both guards still `fill`; the
    spare line behind the picture is the reference's own where it spills, and still `fill` in `got` (the caller's buffer ends there).
    r12l_width: a ragged R12L line (from_av_masked) -- only the bits of its real pixels are compared"""
    got, want = np.asarray(got), np.asarray(want)
    if got.size != want.size:
        return [f"buffer sizes: got {got.size}, want {want.size}"]
    out = []
    g, wv = got[front: front + h * pitch].reshape(h, pitch), want[front: front + h * pitch].reshape(h, pitch)
    if r12l_width:
        full, rem = 36 * r12l_width // 8, 36 * r12l_width % 8
        bad = g[:, :full] != wv[:, :full]
        if rem and ((g[:, full] ^ wv[:, full]) & ((1 << rem) - 1)).any():
            out.append("the last real pixel's bits differ")
    else:
        bad = g != wv
    if bad.any():
        out.append(f"{int(bad.sum())} bytes differ inside the lines; {_where(bad)}")
    end = front + (h + 1) * pitch
    for name, part in (("in front of", got[:front]), ("behind", got[end:]), ("in the spare line behind", got[end - pitch: end])):
        hit = np.flatnonzero(part != fill)
        if hit.size:
            out.append(f"{hit.size} guard bytes {name} the buffer written; first at {int(hit[0])}")
    return out


def from_av_params(i):
    """colour space / range and shifts alternate from case to case"""
    return ((1, 1), (6, 2))[i % 2], ((0, 8, 16), (16, 8, 0))[i % 2]


# ---- every case once through the reference alone ---------------------------------------------------------------------------------------
def run_reference(direction):
    """the compiled reference over every row x size x layout of one direction -> {"cases", "masked", "skipped"}"""
    r = ref()
    cases = masked = 0
    if direction == "to":
        for uv, av in T.TO_AV:
            for w, h in SIZES:
                h = to_av_height(uv, av, h)
                src = make_uv_source(r, uv, w, h, w + h)
                for layout in LAYOUTS:
                    before, after = ref_uv_to_av_laid_out(r, uv, av, [src], w, h, layout)
                    assert not compare_planes([p.whole for p in before], before), "a fresh frame is not all fill"
                    assert len(after) == len(before)
                    cases += 1
                    masked += to_av_masked(uv, av, layout)
    else:
        for av, uv in T.FROM_AV:
            for k, (w, h) in enumerate(SIZES):
                line = r.vc_get_linesize(w, r.get_codec_from_name(uv.encode()))
                for j, layout in enumerate(LAYOUTS):
                    (cs, rng_), shifts = from_av_params(k + j)
                    frp = make_frame_laid_out(r, av, w, h, layout, k, cs, 2 if av.startswith("yuvj") else rng_)
                    pitch, off = dst_layout(layout, line)
                    want, front = ref_av_to_uv_laid_out(r, frp, av, uv, h, pitch, off, shifts)
                    assert want.size == front + pitch * (h + 1) + GUARD
                    r.av_frame_free(C.byref(frp))
                    cases += 1
                    masked += from_av_masked(uv, w)
    return {"cases": cases, "masked": masked, "skipped": 0}


if __name__ == "__main__":
    print("\nRESULT " + json.dumps(run_reference(sys.argv[1])), flush=True)  # (the reference's own messages share the stream)
