"""Plane and buffer layouts for the tests of the pitch and base arguments of the planar shuffles: ug_hip_from_planar / ug_hip_to_planar
(csrc/planar_api.hip) and the seven entry points they forward to or that stand beside them (csrc/planar.hip, csrc/pixfmt.hip).  A layout
describes every operand of a call -- each plane and the packed side -- as an allocation of its own: canaries, the lines at a pitch, one
spare line, canaries.  Destinations hold FILL everywhere, sources random bytes everywhere (padding read as pixels changes the result).
The expected bytes are computed on the host on the very same laid-out bytes: by the compiled reference (oracle/_ref) called with the
layout's pointers and line sizes, and always by the restatement (oracle/planar_oracle.py, oracle/pyoracle.py) on the views inside the
lines; where oracle/_ref is absent the restatement stands alone.  Modelled on tests/pitch_layout.py and tests/lavc_layout.py.  Plain
numpy + ctypes, no GPU: the helper's own checks are tests/test_planar_layout.py.

What each conversion is held to (expectations() encodes exactly this and masks nothing else):
  from_planar  every variant: the compiled reference byte for byte (its portable build for yuv420p_to_uyvy below 16 pixels, whose SSE loop
               counts `x < width - 15` unsigned), padding, spare line and canaries untouched.
               R12L output at width % 8 != 0: the reference packs uninitialised stack behind the last pixel (from_planar.c:74-82), so
               only the bits of real pixels are held to it; the whole group is held to the restatement's zero tail, which the header
               promises.
  to_planar    uyvy_to_nv12, uyvy_to_i420: the reference at even sizes, the restatement alone at odd ones (the reference strides the UYVY
               source by 2 * width, to_planar.c:213).  Of the GPU sizes only 96x6 is even both ways: at the others the device is held to
               the restatement, which tests/test_planar_layout.py pins to the reference on the CPU.  rgba_to_bgra, vuya_to_i444: the
               reference.
               r12l_to_*: the samples inside the picture are held to the reference, everything past `width` must still be FILL (the
               reference writes its whole last group there; the header states the difference).
               y216_to_p010le: the reference when every line is tight; the restatement when a line is longer, because the reference
               finds the odd luma line by running on from the even one (to_planar.c:191-199).
               v210_to_p010le: width % 6 == 0 the reference; otherwise pyoracle.v210_to_p010le(use_ref=True, y_pad, uv_pad) on whole
               lines -- the reference writes whole groups past `width` and the product reproduces it, so the padding is part of the
               result there (pads are whole samples).
The reference has no source pitch (it assumes vc_get_linesize; uyvy_to_nv12 2 * width) and nothing in it puts an operand one sample
past an aligned address while the others stay: for the `one_off` layout and for the source pitches of the direct entry points
(`custom`) the reference runs on the same lines gathered tight and its lines are carried over."""
import ctypes as C

import numpy as np

from oracle import planar_oracle as PO
from oracle import pyoracle as O
from pitch_layout import FILL, GUARD, SLACK, aligned_bytes

LAYOUTS = ["tight", "odd", "offset"]
FROM_SIZES = [(1, 1), (2, 3), (6, 2), (7, 5), (9, 4), (16, 2), (17, 3), (50, 7), (96, 5), (515, 2), (560, 3)]
TO_SIZES = [(2, 2), (6, 6), (7, 5), (9, 4), (16, 2), (17, 3), (18, 6), (50, 7), (96, 5), (515, 2), (560, 3)]
# the smallest sizes that reach each hazard: 70 groups of 8 = a full wave on the wave-wide store path, then a wave of 6 whole groups; a full
# wave, then one ragged group (lane-by-lane stores beside the wave path); fast-eligible with an odd height (one 4:2:0 line standing alone);
# line pairs across the 4-row workgroup; ragged for 6-, 8- and 16-pixel groups; three whole v210 groups, an odd pair count; one pixel
GPU_SIZES = [(560, 3), (515, 2), (96, 5), (16, 9), (50, 7), (18, 3), (1, 1)]
V210_SIZES = [(390, 2), (780, 2)]  # v210_to_p010le_kernel's 128- and 256-lane blocks, each with a partly filled last wave
ONE_OFF_SIZES = [(560, 3), (96, 5)]
TO_NAMES = PO.TO_NAMES + ["uyvy_to_i422"]  # (no decode_buffer_func_t of the reference's: ug_hip_uyvy_to_i422 only)


def from_variants():
    """(name, in_depth): the XX conversions at every depth the reference routes to them (as tests/test_planar_api.py)"""
    depths = {"rgbpXX_to_rgb": (8, 10, 12, 16), "rgbpXXle_to_rg48": (10, 12, 16), "rgbpXXle_to_r10k": (10, 12, 16),
              "rgbpXXle_to_r12l": (12, 16), "yuv422pXX_to_uyvy": (8, 10, 12, 16)}
    return [(n, d) for n in PO.FROM_NAMES for d in depths.get(n, (0,))]


def roundup16(n):
    return (n + 15) // 16 * 16


class Operand:
    """one plane or the packed side: `whole` = its allocation at a 256-byte aligned address (front canaries, rows + 1 lines at `pitch`,
    back canaries), the first line `off` bytes in; `line` = the bytes of a line the conversion reads or writes, `unit` = a sample"""

    def __init__(self, line, rows, unit, pitch, base_off=0, rng=None):
        self.line, self.rows, self.unit, self.pitch, self.off = line, rows, unit, pitch, GUARD + base_off
        n = self.off + pitch * (rows + 1) + max(0, line - pitch) + (GUARD if rng is None else SLACK)
        self.whole = aligned_bytes(n + n % 2, fill=FILL, rng=rng)

    @property
    def addr(self):
        return self.whole.ctypes.data + self.off

    @property
    def end(self):
        """behind the spare line"""
        return self.off + self.pitch * (self.rows + 1)

    def lines(self):
        assert self.pitch >= self.line
        return self.whole[self.off: self.off + self.rows * self.pitch].reshape(self.rows, self.pitch)

    def samples(self):
        """the samples inside the lines as a 2-D array"""
        v = self.lines()[:, : self.line]
        return v.view("<u2") if self.unit == 2 else v

    def tail(self):
        """everything from the first line on, contiguous"""
        return self.whole[self.off:]

    def like(self, data=None):
        """the same geometry at the same residue of the address; all FILL, or holding `data` (a whole allocation)"""
        o = Operand.__new__(Operand)
        o.line, o.rows, o.unit, o.pitch, o.off = self.line, self.rows, self.unit, self.pitch, self.off
        o.whole = aligned_bytes(self.whole.size, fill=FILL)
        if data is not None:
            o.whole[:] = data
        return o


class Case:
    """one call: kind "from" (planes -> packed) or "to" (packed -> planes), the operands, and the arguments beside them"""

    def __init__(self, kind, name, depth, w, h, layout, planes, packed, shifts):
        self.kind, self.name, self.depth, self.w, self.h, self.layout = kind, name, depth, w, h, layout
        self.planes, self.packed, self.shifts = planes, packed, shifts

    @property
    def srcs(self):
        return self.planes if self.kind == "from" else [self.packed]

    @property
    def dsts(self):
        return [self.packed] if self.kind == "from" else self.planes

    @property
    def out_pitch(self):
        """from side: the out_pitch argument (yuv420_to_i420 ignores it, from_planar.c:371-389: its output is one run of bytes)"""
        return self.w if self.name == "yuv420_to_i420" else self.packed.pitch

    def __repr__(self):
        return (f"{self.name}/{self.depth} {self.w}x{self.h} {self.layout} planes " +
                " ".join(f"{p.pitch}+{p.off - GUARD}" for p in self.planes) + f" packed {self.packed.pitch}+{self.packed.off - GUARD}")


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------
def shared_pitch(name, depth):
    """gbrap_to_rgb[a] and rgbpXX_to_rgb at depth 8 stride every plane by in_linesize[0] (from_planar.c:345), the reference's habit, kept on
    purpose: their planes share plane 0's pitch in every layout"""
    return name.startswith("gbrap") or (name == "rgbpXX_to_rgb" and depth == 8)


def from_geometry(name, depth, w, h):
    """-> ([(rows, samples, bytes per sample)] of the planes, (line bytes, rows, unit) of the packed side).  unit: the alignment the
    entry point asks of that side today (csrc/planar.hip: dst & 3 for UYVY and v210) or, where it asks none, the format's own word"""
    fam, out, d, idx = PO.from_info(name, depth)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    if fam == "rgbp":
        planes = [(h, w, 1 if d == 8 else 2)] * (4 if idx[3] >= 0 else 3)
    elif name == "yuv444p_to_vuya":
        planes = [(h, w, 1)] * 3
    elif name in ("yuv420p_to_uyvy", "yuv420_to_i420"):
        planes = [(h, w, 1), (ch, cw, 1), (ch, cw, 1)]
    else:
        planes = [(h, w, 1 if d == 8 else 2), (h, cw, 1 if d == 8 else 2), (h, cw, 1 if d == 8 else 2)]
    if name == "yuv420_to_i420":
        return planes, (w * h + 2 * (w // 2) * (h // 2), 1, 1)
    unit = {"rgb": 1, "r12l": 1, "rg48": 2}.get(name.split("_to_")[1], 4)
    return planes, (PO.out_linesize(name, w), h, unit)


def from_written(name, w):
    """bytes of an output line that are written: width / 6 v210 groups (from_planar.c:309), width / 2 pairs of planar 4:2:2 (:400); else
    the line (R12L: whole groups; yuv420p_to_uyvy at an odd width: Cb Y Cr 0)"""
    if name.endswith("_v210"):
        return 16 * (w // 6)
    if name.startswith("yuv422p"):
        return 4 * (w // 2)
    return PO.out_linesize(name, w)


def to_geometry(name, w, h):
    """-> ([(rows, samples, bytes per sample)] of the planes, (line bytes, tight stride, unit) of the packed source)"""
    cw = (w + 1) // 2
    if name == "uyvy_to_i422":
        return [(h, w, 1), (h, cw, 1), (h, cw, 1)], (4 * cw, 4 * cw, 4)
    planes = [(max(rows, 1), n, np.dtype(dt).itemsize) for rows, n, dt in PO.to_shapes(name, w, h)]
    line = PO.in_linesize(name, w)
    unit = {"r12l": 1, "y216": 2}.get(name.split("_to_")[0], 4)
    return planes, (line, 2 * w if name == "uyvy_to_nv12" else line, unit)  # the reference strides UYVY by 2 * width there (to_planar.c:213)


def size_ok(kind, name, w, h):
    """sizes a conversion takes"""
    if name == "yuv420_to_i420":
        return w % 2 == 0 and h % 2 == 0
    if name == "v210_to_p010le" and w % 6 and h < 5:
        return False  # refused: the reference reads in front of its planes there (to_planar.c:142-148 with y < 4)
    return True


def dispatcher_takes(kind, name, w, h):
    """sizes ug_hip_from_planar / ug_hip_to_planar take: uyvy_to_nv12 walks its source by the reference's 2 * width bytes, at an odd width
    two bytes short of the UYVY line ug_hip_uyvy_to_nv12 reads (and no multiple of 4) -- an odd width is UG_HIP_EINVAL by that name"""
    return size_ok(kind, name, w, h) and not (name == "uyvy_to_nv12" and w % 2)


I420_SIZES = [(560, 4), (96, 6), (16, 10), (50, 8)]  # yuv420_to_i420 takes even sizes only: the same hazards with an even height


def gpu_sizes(kind, name):
    """the sizes of the GPU layout tests a conversion takes by name, never none.  uyvy_to_nv12 and uyvy_to_i420 also run at 96x6: every
    other even width of GPU_SIZES has an odd height, where they are held to the restatement alone (to_ref_ok)"""
    if name == "yuv420_to_i420":
        return list(I420_SIZES)
    extra = V210_SIZES if name == "v210_to_p010le" else [(96, 6)] if name in ("uyvy_to_nv12", "uyvy_to_i420") else []
    return [s for s in GPU_SIZES + extra if dispatcher_takes(kind, name, *s)]


def one_off_sizes(kind, name):
    """the fast-eligible sizes the one_off layout runs at"""
    if name == "yuv420_to_i420":
        return I420_SIZES[:2]
    if name == "v210_to_p010le":
        return [(96, 6)]  # (560 is no multiple of 6 and 3 lines are too few for the margin)
    return ONE_OFF_SIZES + ([(96, 6)] if name in ("uyvy_to_nv12", "uyvy_to_i420") else [])


def _pitches(layout, lines, units, shared):
    """plane pitches of a layout"""
    out = []
    for i, (line, unit) in enumerate(zip(lines, units)):
        if shared and i:
            out.append(out[0])
        elif layout == "tight":
            out.append(line)
        elif layout == "odd":  # line + (1 + i) samples, no two alike, none a multiple of 16
            p = line + (1 + i) * unit
            while p % 16 == 0 or p in out:
                p += 4 * unit
            out.append(p)
        elif layout == "offset":
            out.append(roundup16(line) + 64)
        else:  # one_off
            out.append(roundup16(line))
    return out


def make_case(kind, name, depth, w, h, layout, seed=0, which=None, plane_pitches=None, packed_pitch=None, offs=None):
    """A case in `layout`.  one_off: `which` = the operand one sample / unit past alignment (plane number; len(planes) = the packed side).
    custom: plane_pitches / packed_pitch in bytes, offs = base offsets of [planes..., packed] (default 0)."""
    rng = np.random.default_rng(seed)
    if kind == "from":
        geo, (pline, prows, punit) = from_geometry(name, depth, w, h)
        pstride = pline
    else:
        geo, (pline, pstride, punit) = to_geometry(name, w, h)
        prows = h
    lines, units = [n * sb for _, n, sb in geo], [sb for _, _, sb in geo]
    if layout == "custom":
        pp = list(plane_pitches)
        kp = packed_pitch
        off = list(offs) if offs else [0] * (len(geo) + 1)
    else:
        pp = _pitches(layout, lines, units, shared_pitch(name, depth) if kind == "from" else False)
        if kind == "to" or layout == "tight":
            kp = pstride  # the dispatcher's packed source is always vc_get_linesize apart
        elif layout == "odd":
            kp = pline + punit if (pline + punit) % 16 else pline + 2 * punit
        else:
            kp = roundup16(pline) + (64 if layout == "offset" else 0)
        if layout == "offset":
            off = units + [punit]
        elif layout == "one_off":
            off = [(units + [punit])[k] if k == which else 0 for k in range(len(geo) + 1)]
        else:
            off = [0] * (len(geo) + 1)
    src_rng = lambda is_src: rng if is_src else None
    planes = [Operand(line, rows, unit, p, o, src_rng(kind == "from")) for (rows, _, unit), line, p, o in zip(geo, lines, pp, off)]
    packed = Operand(pline, prows, punit, kp, off[-1], src_rng(kind == "to"))
    if name == "yuv422p10le_to_v210":  # samples are OR-ed in as they are (from_planar.c:307-331): inputs are 10-bit by contract
        for p in planes:
            p.whole.view("<u2")[:] &= 0x3FF
    return Case(kind, name, depth, w, h, layout, planes, packed, [(0, 8, 16), (16, 8, 0), (8, 16, 0)][seed % 3])


def one_off_operands(kind, name, depth, w, h):
    """the operand numbers make_case(..., "one_off", which=) takes"""
    geo = (from_geometry if kind == "from" else to_geometry)(*((name, depth, w, h) if kind == "from" else (name, w, h)))[0]
    return list(range(len(geo) + 1))


def gather(op):
    """the lines of an operand, tight"""
    return np.stack([op.whole[op.off + y * op.pitch: op.off + y * op.pitch + op.line] for y in range(op.rows)])


def tight_twin(case):
    """the same pixels in the `tight` layout: what a layout the reference cannot be pointed at is held to"""
    t = make_case(case.kind, case.name, case.depth, case.w, case.h, "tight", seed=1)
    t.shifts = case.shifts
    for a, b in zip(t.srcs, case.srcs):
        rows = gather(b)
        for y in range(a.rows):
            a.whole[a.off + y * a.pitch: a.off + y * a.pitch + a.line] = rows[y]
    return t


# ---- expectations -----------------------------------------------------------------------------------------------------------------------
class Want:
    """what the destinations must hold: `ops` = Operands of the destinations' geometry; the first held[k] bytes of every line of operand k
    (and `bits` more bits of the byte behind them) equal ops[k]'s; with `untouched`, every other byte of the allocation -- the rest of the
    line, the spare line, the canaries -- must still be FILL"""

    def __init__(self, label, ops, held, bits=0, untouched=True):
        self.label, self.ops, self.held, self.bits, self.untouched = label, ops, held, bits, untouched


def _overlay(case, arrays, label):
    """the arrays a restatement returned (one per destination, 2-D, or flat for a destination of one line), laid into FILL"""
    ops = [d.like() for d in case.dsts]
    for op, a in zip(ops, arrays):
        b = np.ascontiguousarray(a).view(np.uint8).reshape(op.rows, -1)
        op.lines()[:, : b.shape[1]] = b
    return Want(label, ops, [op.line for op in ops])


def _tight_src(case):
    """to side: the packed source as the converters' restatements take it, lines vc_get_linesize apart"""
    op = case.packed
    stride = to_geometry(case.name, case.w, case.h)[1][1]
    if op.pitch == stride:
        return op.tail()
    assert stride == op.line, "lines that overlap cannot be gathered"
    return np.concatenate([gather(op).ravel(), np.zeros(SLACK, np.uint8)])


def restate(case):
    """the restatement on the views inside the lines -> Want"""
    c = case
    if c.kind == "from":
        out = PO.from_planar(c.name, [p.samples() for p in c.planes], c.w, c.h, c.depth, c.shifts)
        if c.name != "yuv420_to_i420":
            full = np.full((c.h, c.packed.line), FILL, np.uint8)
            n = from_written(c.name, c.w)
            full[:, :n] = out[:, :n]
            out = full
        return _overlay(c, [out], "restatement")
    if c.name == "uyvy_to_nv12":  # any source pitch, read where it lies
        return _overlay(c, O.uyvy_to_nv12(c.packed.tail(), c.w, c.h, src_pitch=c.packed.pitch), "restatement")
    if c.name == "uyvy_to_i422":
        return _overlay(c, O.uyvy_to_i422(_tight_src(c), c.w, c.h), "restatement")
    return _overlay(c, PO.to_planar(c.name, _tight_src(c), c.w, c.h), "restatement")


def v210_ragged(case, use_ref):
    """v210_to_p010le with width % 6 != 0: whole lines, padding included, from pyoracle.v210_to_p010le with the pads of this layout"""
    c = case
    pads = [(p.pitch - p.line) // 2 for p in c.planes]
    assert all(p.pitch % 2 == 0 for p in c.planes)
    y, uv = O.v210_to_p010le(_tight_src(c), c.w, c.h, use_ref=use_ref, y_pad=pads[0], uv_pad=pads[1], fill=FILL * 0x101)
    ops = [d.like() for d in c.dsts]
    for op, a in zip(ops, (y, uv)):
        op.lines()[:] = np.ascontiguousarray(a).view(np.uint8).reshape(op.rows, op.pitch)
    return Want("reference (whole lines)" if use_ref else "restatement (whole lines)", ops, [op.pitch for op in ops])


def to_ref_ok(case):
    """to side: may the compiled reference be asked?"""
    c = case
    if c.name in ("uyvy_to_nv12", "uyvy_to_i420", "uyvy_to_i422"):
        return c.w % 2 == 0 and c.h % 2 == 0
    if c.name == "y216_to_p010le":
        return all(p.pitch == p.line for p in c.planes)
    return True


def reference(case):
    """the compiled reference on the very bytes of a tight / odd / offset case -> Want"""
    c = case
    dst = [d.like() for d in c.dsts]
    if c.kind == "from":
        d = O._FromPlanar()
        d.width, d.height, d.out_data, d.out_pitch, d.in_depth = c.w, c.h, dst[0].addr, c.out_pitch, c.depth
        for i, p in enumerate(c.planes):
            d.in_data[i], d.in_linesize[i] = p.addr, p.pitch
        d.rgb_shift[0], d.rgb_shift[1], d.rgb_shift[2] = c.shifts
        fn = getattr(O.ref(c.name == "yuv420p_to_uyvy" and c.w < 16), c.name)
        fn.restype, fn.argtypes = None, [O._FromPlanar]
        fn(d)
        if c.name.endswith("_r12l") and c.w % 8:  # only the bits of real pixels
            return Want("reference (real pixels)", dst, [36 * c.w // 8], bits=36 * c.w % 8, untouched=False)
        return Want("reference", dst, [dst[0].line])
    if c.name == "uyvy_to_i422":
        return _overlay(c, O.uyvy_to_i422(_tight_src(c), c.w, c.h, use_ref=True), "reference")
    d = O._ToPlanar()
    d.width, d.height, d.in_data = c.w, c.h, c.packed.addr
    for i, p in enumerate(dst):
        d.out_data[i], d.out_linesize[i] = p.addr, p.pitch
    fn = getattr(O.ref(), c.name)
    fn.restype, fn.argtypes = None, [O._ToPlanar]
    fn(d)
    return Want("reference", dst, [p.line for p in dst])


def expectations(case, use_ref=None):
    """every Want a result of `case` is held to (see the module's docstring for the rules)"""
    c = case
    use_ref = O.have_ref() if use_ref is None else use_ref
    if c.kind == "to" and c.name == "v210_to_p010le" and c.w % 6:
        return [v210_ragged(c, False)] + ([v210_ragged(c, True)] if use_ref else [])
    wants = [restate(c)]
    if not use_ref or (c.kind == "to" and not to_ref_ok(c)):
        return wants
    if c.layout in LAYOUTS:
        return wants + [reference(c)]
    # one_off, custom: the reference's lines of the same pixels laid out tight
    t = tight_twin(c)
    if c.kind == "to" and not to_ref_ok(t):
        return wants
    rw = reference(t)
    ops = [d.like() for d in c.dsts]
    for op, top, held in zip(ops, rw.ops, rw.held):
        n = held + (1 if rw.bits else 0)
        op.lines()[:, :n] = top.lines()[:, :n]
    return wants + [Want(rw.label + " of the tight twin", ops, rw.held, rw.bits, rw.untouched)]


# ---- comparison -------------------------------------------------------------------------------------------------------------------------
def _where(bad):
    ys, xs = np.nonzero(bad)
    return f"first at line {int(ys[0])} byte {int(xs[0])}; bytes of a line: {sorted(set(xs.tolist()))[:12]}; lines: {sorted(set(ys.tolist()))[:8]}"


def compare(got_wholes, want):
    """got_wholes: the destinations' whole allocations as the code under test left them.  Findings (empty = equal), per operand: bytes that
    differ inside the lines; line padding no longer FILL; the spare line no longer FILL; canaries in front or behind no longer FILL"""
    out = []
    for k, (g, op, held) in enumerate(zip(got_wholes, want.ops, want.held)):
        g = np.asarray(g)
        if g.size != op.whole.size:
            out.append(f"{want.label}: operand {k}: sizes {g.size} / {op.whole.size}")
            continue
        gl, wl = g[op.off: op.off + op.rows * op.pitch].reshape(op.rows, op.pitch), op.lines()
        bad = gl[:, :held] != wl[:, :held]
        if bad.any():
            out.append(f"{want.label}: operand {k}: {int(bad.sum())} bytes differ inside the lines; {_where(bad)}")
        if want.bits and ((gl[:, held] ^ wl[:, held]) & ((1 << want.bits) - 1)).any():
            out.append(f"{want.label}: operand {k}: the last real pixel's bits differ")
        if not want.untouched:
            continue
        pad = gl[:, held:] != FILL
        if pad.any():
            out.append(f"{want.label}: operand {k}: {int(pad.sum())} padding bytes written; {_where(pad)}")
        for name, part in (("of the spare line", g[op.end - op.pitch: op.end]), ("of the canary in front", g[: op.off]), ("of the canary behind", g[op.end:])):
            hit = np.flatnonzero(part != FILL)
            if hit.size:
                out.append(f"{want.label}: operand {k}: {hit.size} bytes {name} written; first at {int(hit[0])}")
    return out


def check(case, got_wholes, use_ref=None):
    """findings of a result against everything it is held to"""
    out = []
    for want in expectations(case, use_ref):
        out += compare(got_wholes, want)
    return out


# ---- the device side --------------------------------------------------------------------------------------------------------------------
def mirror(torch, op, device="cuda"):
    """a device (or, for the helper's own test, CPU) byte tensor holding an operand's whole allocation at a 256-byte aligned address -> (the
    tensor, the address of the first line)"""
    buf = torch.empty(op.whole.size + 256, dtype=torch.uint8, device=device)
    skip = (-buf.data_ptr()) % 256
    view = buf[skip: skip + op.whole.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(op.whole)))
    assert view.data_ptr() % 256 == 0 and op.whole.ctypes.data % 256 == 0
    return view, view.data_ptr() + op.off
