"""The planar shuffles at plane and buffer layouts beyond the tight, aligned one: ug_hip_from_planar / ug_hip_to_planar
(csrc/planar_api.hip) by every name, and the seven entry points of csrc/planar.hip and csrc/pixfmt.hip called directly at every pitch
argument they have.  tests/planar_layout.py lays every operand out as an allocation of its own (canaries, lines at a pitch, a spare
line, canaries; destinations 0xA5, sources random everywhere) and computes the expected bytes on the very same bytes -- the compiled
reference where oracle/_ref is there, the restatement always.  Whole allocations are mirrored to the device at 256-byte aligned
addresses, so every base and pitch has the residue it has on the host; after the call the whole allocation comes back and every byte
of it is looked at.  Every comparison is bit-exact.

What these tests cannot show: this GPU completes a misaligned 16-, 32- or 64-bit access with the right bytes, so a wrong alignment
predicate (one that sends a misaligned operand down a wide-access branch) computes the right result here all the same.  What they do show
is that both branches compute the right bytes at addresses where only one of them may run, that every pitch and every base is honoured
(no swapped, shared, sample-counted or ignored one), and that nothing is stored outside the lines.

The short-pitch refusals: every pointer is a real allocation large enough for the picture at its full line size, so a call that is
wrongly accepted stays inside it and shows as a failed assertion."""
import ctypes as C

import numpy as np
import pytest

import planar_layout as PL
from pitch_layout import FILL

FROM = PL.from_variants()


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _dispatch(hip, case, addrs, pitches, stream):
    """ug_hip_from_planar / ug_hip_to_planar with the operands at `addrs` ([planes..., packed]) and `pitches` -> rc"""
    lib = hip.L.load()
    n = len(case.planes)
    if case.kind == "from":
        d = hip.FromPlanarData()
        d.width, d.height, d.out_data, d.out_pitch, d.in_depth = case.w, case.h, addrs[n], pitches[n], case.depth
        for i in range(n):
            d.in_data[i], d.in_linesize[i] = addrs[i], pitches[i]
        d.rgb_shift[0], d.rgb_shift[1], d.rgb_shift[2] = case.shifts
        return lib.ug_hip_from_planar(case.name.encode(), C.byref(d), stream)
    d = hip.ToPlanarData()
    d.width, d.height, d.in_data = case.w, case.h, addrs[n]
    for i in range(n):
        d.out_data[i], d.out_linesize[i] = addrs[i], pitches[i]
    return lib.ug_hip_to_planar(case.name.encode(), C.byref(d), stream)


# entry point -> (kind, the conversion's name in tests/planar_layout.py)
DIRECT = {
    "ug_hip_uyvy_to_i420": ("to", "uyvy_to_i420"), "ug_hip_v210_to_p010le": ("to", "v210_to_p010le"),
    "ug_hip_yuv420p_to_uyvy": ("from", "yuv420p_to_uyvy"), "ug_hip_yuv422p_to_uyvy": ("from", "yuv422p_to_uyvy"),
    "ug_hip_yuv422p10le_to_v210": ("from", "yuv422p10le_to_v210"), "ug_hip_uyvy_to_i422": ("to", "uyvy_to_i422"),
    "ug_hip_uyvy_to_nv12": ("to", "uyvy_to_nv12"),
}


def _direct(hip, entry, case, addrs, pitches, stream):
    """an entry point called directly: (plane, pitch)... then (dst, dst_pitch) in the decode direction, (src, src_pitch) first in the other"""
    n = len(case.planes)
    pairs = [(addrs[i], pitches[i]) for i in range(n)]
    pairs = pairs + [(addrs[n], pitches[n])] if case.kind == "from" else [(addrs[n], pitches[n])] + pairs
    return getattr(hip.L.load(), entry)(*[x for p in pairs for x in p], case.w, case.h, stream)


def _pitches(case):
    return [p.pitch for p in case.planes] + [case.out_pitch if case.kind == "from" else case.packed.pitch]


def _run(hip, torch, case, entry=None):
    """the product on the mirror of every operand of `case` -> (destinations' whole allocations, findings about the sources)"""
    ops = case.planes + [case.packed]
    mirrors = [PL.mirror(torch, op) for op in ops]
    addrs = [a for _, a in mirrors]
    call = _dispatch if entry is None else (lambda h, c, a, p, s: _direct(h, entry, c, a, p, s))
    rc = call(hip, case, addrs, _pitches(case), _stream(torch))
    torch.cuda.synchronize()
    assert rc == hip.L.SUCCESS, (case, rc, hip.L.last_error())
    back = {id(op): t.cpu().numpy() for op, (t, _) in zip(ops, mirrors)}
    bad = [f"source operand {k} was written" for k, op in enumerate(case.srcs) if not np.array_equal(back[id(op)], op.whole)]
    return [back[id(op)] for op in case.dsts], bad


def _findings(hip, torch, case, entry=None):
    got, bad = _run(hip, torch, case, entry)
    return [f"{case}: {f}" for f in bad + PL.check(case, got)]


def _sizes(kind, name, sizes):
    """of the direct-call sizes, those an entry point takes"""
    return [(w, h) for w, h in sizes if PL.size_ok(kind, name, w, h)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,depth", FROM)
def test_gpu_from_planar_layouts(hip, name, depth):
    import torch
    findings, ran = [], 0
    for i, (w, h) in enumerate(PL.gpu_sizes("from", name)):
        for j, layout in enumerate(PL.LAYOUTS):
            findings += _findings(hip, torch, PL.make_case("from", name, depth, w, h, layout, seed=3 * i + j))
            ran += 1
    assert ran >= 12 and not findings, "\n".join(findings)


@pytest.mark.gpu
@pytest.mark.parametrize("name", PL.PO.TO_NAMES)
def test_gpu_to_planar_layouts(hip, name):
    import torch
    findings, ran = [], 0
    for i, (w, h) in enumerate(PL.gpu_sizes("to", name)):
        for j, layout in enumerate(PL.LAYOUTS):
            findings += _findings(hip, torch, PL.make_case("to", name, 0, w, h, layout, seed=3 * i + j))
            ran += 1
    assert ran >= 12 and not findings, "\n".join(findings)


def _one_off(hip, torch, kind, name, depth):
    """every operand in turn one sample / unit past an aligned address, the others 16-byte aligned: held to the reference's and the
    restatement's lines of the same pixels, and to what the device itself makes of them laid out tight"""
    findings, ran = [], 0
    for w, h in PL.one_off_sizes(kind, name):
        assert PL.dispatcher_takes(kind, name, w, h), (name, w, h)
        for which in PL.one_off_operands(kind, name, depth, w, h):
            case = PL.make_case(kind, name, depth, w, h, "one_off", seed=which, which=which)
            got, bad = _run(hip, torch, case)
            twin = PL.tight_twin(case)
            tight, _ = _run(hip, torch, twin)
            ops = [d.like() for d in case.dsts]
            for op, top, t in zip(ops, twin.dsts, tight):
                op.lines()[:, : op.line] = top.like(t).lines()[:, : op.line]
            bad += PL.compare(got, PL.Want("the device's tight result", ops, [op.line for op in ops]))
            findings += [f"{case}: {f}" for f in bad + PL.check(case, got)]
            ran += 1
    assert ran >= 2, (name, "no case ran")
    return findings


@pytest.mark.gpu
@pytest.mark.parametrize("name,depth", FROM)
def test_gpu_from_planar_one_operand_off(hip, name, depth):
    import torch
    findings = _one_off(hip, torch, "from", name, depth)
    assert not findings, "\n".join(findings)


@pytest.mark.gpu
@pytest.mark.parametrize("name", PL.PO.TO_NAMES)
def test_gpu_to_planar_one_operand_off(hip, name):
    import torch
    findings = _one_off(hip, torch, "to", name, 0)
    assert not findings, "\n".join(findings)


def _direct_cases(kind, name, w, h):
    """every pitch argument of an entry point its own: lines 4 bytes longer and more (no two planes alike), and lines of
    roundup16(line) + 16 bytes and more -- still eligible for the wide-access kernels, with three distinct plane pitches"""
    geo, packed = (PL.from_geometry(name, 0, w, h) if kind == "from" else PL.to_geometry(name, w, h))
    lines = [n * sb for _, n, sb in geo]
    for k, (step, first) in enumerate([(4, lambda line: line + 4), (16, lambda line: PL.roundup16(line) + 16)]):
        pitches = [first(packed[0])]
        for i, line in enumerate(lines):
            p = first(line) + step * i
            while p in pitches:
                p += step
            pitches.append(p)
        yield PL.make_case(kind, name, 0, w, h, "custom", seed=w + k, plane_pitches=pitches[1:], packed_pitch=pitches[0])


@pytest.mark.gpu
@pytest.mark.parametrize("entry", sorted(DIRECT))
def test_gpu_direct_entry_points_honour_every_pitch(hip, entry):
    """the source pitches too, which the dispatchers never pass: the expectation is the reference / restatement on the source lines gathered
    tight (tests/planar_layout.py: expectations)"""
    import torch
    kind, name = DIRECT[entry]
    findings, ran = [], 0
    sizes = [(96, 6), (50, 7), (560, 3)] + ([(390, 2)] if name == "v210_to_p010le" else [])
    for w, h in _sizes(kind, name, sizes):
        for case in _direct_cases(kind, name, w, h):
            assert len(set(_pitches(case))) == len(_pitches(case)), case
            findings += _findings(hip, torch, case, entry)
            ran += 1
    assert ran >= 6 and not findings, "\n".join(findings)


@pytest.mark.gpu
def test_gpu_uyvy_to_nv12_odd_cbcr_plane(hip):
    """the byte-store instantiation (uyvy_to_nv12_kernel<true>): a CbCr plane with an odd pitch, at an odd address, or both"""
    import torch
    findings = []
    for w, h in [(96, 6), (50, 7), (18, 3)]:
        cw = (w + 1) // 2
        for c_pitch, c_off in [(2 * cw + 1, 0), (2 * cw + 2, 1), (2 * cw + 3, 1)]:
            case = PL.make_case("to", "uyvy_to_nv12", 0, w, h, "custom", seed=w + c_pitch, plane_pitches=[w + 2, c_pitch], packed_pitch=4 * cw,
                                offs=[0, c_off, 0])
            assert (case.planes[1].addr | case.planes[1].pitch) & 1
            findings += _findings(hip, torch, case, "ug_hip_uyvy_to_nv12")
    assert not findings, "\n".join(findings)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _roomy(kind, name, depth, w, h):
    """a case whose every operand has room for the picture at its full line size and more: lines of roundup16(line) + 64 bytes"""
    geo, packed = (PL.from_geometry(name, depth, w, h) if kind == "from" else PL.to_geometry(name, w, h))
    pp = [PL.roundup16(n * sb) + 64 for _, n, sb in geo]
    return PL.make_case(kind, name, depth, w, h, "custom", plane_pitches=pp, packed_pitch=PL.roundup16(packed[0]) + 64)


def _refused(hip, torch, case, rows, entry=None):
    """rows: (what, operand number, "pitch" | "addr", value | offset).  The call as it stands succeeds; with one argument changed as a row
    says it is refused with UG_HIP_EINVAL and a message, and every destination byte is still FILL."""
    ops = case.planes + [case.packed]
    call = _dispatch if entry is None else (lambda h, c, a, p, s: _direct(h, entry, c, a, p, s))
    mirrors = [PL.mirror(torch, op) for op in ops]
    rc = call(hip, case, [a for _, a in mirrors], _pitches(case), _stream(torch))
    torch.cuda.synchronize()
    assert rc == hip.L.SUCCESS, (case, "the call the rows start from", rc, hip.L.last_error())
    mirrors = [PL.mirror(torch, op) for op in ops]
    dst_mirrors = [m for op, m in zip(ops, mirrors) if any(op is d for d in case.dsts)]
    bad = []
    for what, k, field, value in rows:
        addrs, pitches = [a for _, a in mirrors], _pitches(case)
        if field == "pitch":
            pitches[k] = value
        else:
            addrs[k] += value
        rc = call(hip, case, addrs, pitches, _stream(torch))
        torch.cuda.synchronize()
        if rc != hip.L.EINVAL:
            bad.append(f"{what}: rc {rc}")
        elif not hip.L.last_error():
            bad.append(f"{what}: no message")
        if any(not bool((t == FILL).all()) for t, _ in dst_mirrors):
            bad.append(f"{what}: a destination was written")
            break  # (what follows would be blamed for it)
    return [f"{case.name} {case.w}x{case.h}: {b}" for b in bad]


def _short_rows(case, needs, skip=()):
    """one row per operand: its pitch one step (a sample; a 32-bit word on the packed side) below the bytes of a line"""
    n = len(case.planes)
    rows = []
    for k, need in enumerate(needs):
        if k in skip:
            continue
        step = 4 if k == n and case.packed.unit == 4 else (case.planes + [case.packed])[k].unit
        assert need - step > 0
        rows.append((f"operand {k}: pitch {need - step} < {need}", k, "pitch", need - step))
    return rows


def _odd_rows(case, ks):
    """16-bit planes: an odd address, an odd line size (long enough)"""
    every = case.planes + [case.packed]
    return [(f"operand {k} at an odd address", k, "addr", 1) for k in ks] + [(f"operand {k}: odd pitch", k, "pitch", every[k].pitch + 1) for k in ks]


def _direct_needs(entry, w):
    cw = (w + 1) // 2
    return {"ug_hip_uyvy_to_i420": [w, cw, cw, 4 * cw], "ug_hip_v210_to_p010le": [2 * w, 2 * w, 16 * ((w + 5) // 6)],
            "ug_hip_yuv420p_to_uyvy": [w, cw, cw, 4 * cw], "ug_hip_yuv422p_to_uyvy": [w, cw, cw, 4 * (w // 2)],
            "ug_hip_yuv422p10le_to_v210": [2 * w, 2 * cw, 2 * cw, 16 * (w // 6)], "ug_hip_uyvy_to_i422": [w, cw, cw, 4 * cw],
            "ug_hip_uyvy_to_nv12": [w, 2 * cw, 4 * cw]}[entry]


@pytest.mark.gpu
@pytest.mark.parametrize("entry", sorted(DIRECT))
def test_gpu_direct_entry_points_refuse_short_pitches(hip, entry):
    import torch
    kind, name = DIRECT[entry]
    w, h = (18, 6) if "v210" in entry else (16, 4)
    case = _roomy(kind, name, 0, w, h)
    n = len(case.planes)
    rows = _short_rows(case, _direct_needs(entry, w))
    word = lambda k: [(f"operand {k} off a 32-bit word", k, "addr", 2), (f"operand {k}: pitch & 3", k, "pitch", case.packed.pitch + 2)]
    if entry == "ug_hip_uyvy_to_i420":  # only src_pitch has a default
        rows += [(f"operand {k}: pitch 0", k, "pitch", 0) for k in range(n)]
    elif entry == "ug_hip_v210_to_p010le":
        rows += _odd_rows(case, [0, 1]) + word(n)
    elif entry == "ug_hip_yuv422p10le_to_v210":
        rows += _odd_rows(case, [0, 1, 2]) + word(n)
    else:  # dst & 3, dst_pitch & 3; src & 3, src_pitch & 3
        rows += word(n)
    if entry == "ug_hip_yuv420p_to_uyvy":
        rows.append(("lines of 32 bytes at 8-byte steps", n, "pitch", 8))
    bad = _refused(hip, torch, case, rows, entry)
    assert not bad, "\n".join(bad)


# one name per family of the dispatchers (csrc/planar_api.hip: FromConv::family, ToConv::family), 16-bit and byte planes both
FROM_FAMILIES = [("gbrp10le_to_rgb", 0), ("gbrp12le_to_r12l", 0), ("gbrap_to_rgba", 0), ("rgbpXX_to_rgb", 8), ("yuv444p_to_vuya", 0),
                 ("yuv422p_to_yuyv", 0), ("yuv422pXX_to_uyvy", 10), ("yuv420p_to_uyvy", 0), ("yuv422p10le_to_v210", 0), ("yuv420_to_i420", 0)]
TO_FAMILIES = ["r12l_to_gbrp12le", "y216_to_p010le", "rgba_to_bgra", "vuya_to_i444", "v210_to_p010le", "uyvy_to_nv12", "uyvy_to_i420"]


@pytest.mark.gpu
@pytest.mark.parametrize("name,depth", FROM_FAMILIES)
def test_gpu_from_planar_refuses_short_pitches(hip, name, depth):
    import torch
    w, h = (18, 6) if name.endswith("v210") else (16, 4)
    case = _roomy("from", name, depth, w, h)
    n = len(case.planes)
    geo, _ = PL.from_geometry(name, depth, w, h)
    needs = [s * sb for _, s, sb in geo] + [PL.from_written(name, w)]
    # gbrap_to_rgb[a] and 8-bit rgbpXX_to_rgb stride every plane by in_linesize[0]; yuv420_to_i420 ignores the value of out_pitch
    skip = set(range(1, n)) if PL.shared_pitch(name, depth) else set()
    rows = _short_rows(case, needs, skip | ({n} if name == "yuv420_to_i420" else set()))
    rows.append(("out_pitch 0", n, "pitch", 0))
    if geo[0][2] == 2:
        rows += _odd_rows(case, range(n))
    bad = _refused(hip, torch, case, rows)
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("name", TO_FAMILIES)
def test_gpu_to_planar_refuses_short_pitches(hip, name):
    import torch
    w, h = (18, 6) if name.startswith("v210") else (16, 4)
    case = _roomy("to", name, 0, w, h)
    rows = _short_rows(case, [p.line for p in case.planes])
    if case.planes[0].unit == 2:
        rows += _odd_rows(case, range(len(case.planes)))
    if name == "uyvy_to_i420":
        rows += [(f"operand {k}: pitch 0", k, "pitch", 0) for k in range(3)]
    bad = _refused(hip, torch, case, rows)
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_gpu_to_planar_uyvy_to_nv12_refuses_an_odd_width(hip):
    """tests/planar_layout.py: dispatcher_takes -- the sizes the layout tests leave out are refused, not converted some other way"""
    import torch
    for w, h in [(515, 2), (1, 1)]:
        case = _roomy("to", "uyvy_to_nv12", 0, w, h)
        mirrors = [PL.mirror(torch, op) for op in case.planes + [case.packed]]
        rc = _dispatch(hip, case, [a for _, a in mirrors], _pitches(case), _stream(torch))
        torch.cuda.synchronize()
        assert rc == hip.L.EINVAL and hip.L.last_error(), (w, h, rc)
        assert all(bool((t == FILL).all()) for t, _ in mirrors[:2]), (w, h)
