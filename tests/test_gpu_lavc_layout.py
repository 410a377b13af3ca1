"""The lavc converters (ug_hip_uv_to_av / ug_hip_av_to_uv: csrc/lavc_conv.hip and the rows it forwards to planar_api.hip, planar.hip and
pixfmt*.hip) at the frame layouts FFmpeg hands out beyond its default allocator's: tight lines, lines a sample or two longer than the
picture, planes a sample past an aligned address.  The compiled reference runs on the very same bytes (tests/lavc_layout.py): planes
and destinations start from 0xA5 on both sides, whole allocations are mirrored to the device at congruent addresses, and every byte of
every line -- padding included -- must equal the reference's, with the canaries in front of and behind each plane intact."""
import ctypes as C

import numpy as np
import pytest

import lavc_layout as LL
import test_lavc_conv as T
from pitch_layout import FILL, GUARD, aligned_bytes


def _np(t):
    return t.cpu().numpy()


def _check_y216_p010le(src, w, h, got_wholes, want):
    """to_av_masked: against the restatement (pinned to the reference on tight planes, tests/test_planar_api.py), the rest of each line
    and the guards still FILL"""
    from oracle import planar_oracle as PO
    ty, tc = PO.to_planar("y216_to_p010le", src, w, h)
    ref = [p.copy() for p in want]
    for p, t in zip(ref, (ty, tc)):
        b = np.ascontiguousarray(t).view(np.uint8).reshape(p.rows, -1)
        p.lines()[:, : b.shape[1]] = b
    return LL.compare_planes(got_wholes, ref, line_bytes=[2 * w, 2 * tc.shape[1]])


@pytest.mark.gpu
@pytest.mark.parametrize("uv,av", T.TO_AV)
def test_gpu_uv_to_av_layouts(hip, uv, av):
    import torch
    r = LL.ref()
    findings = []
    for w, h in LL.SIZES:
        h = LL.to_av_height(uv, av, h)
        src = LL.make_uv_source(r, uv, w, h, w + h)
        dsrc = LL.mirror_bytes(torch, src)
        for layout in LL.LAYOUTS:
            before, want = LL.ref_uv_to_av_laid_out(r, uv, av, [src], w, h, layout)
            wholes, views = LL.mirror_planes(torch, before)
            hip.uv_to_av(uv, av, dsrc, w, h, views)
            torch.cuda.synchronize()
            got = [_np(t) for t in wholes]
            if LL.to_av_masked(uv, av, layout):
                bad = _check_y216_p010le(src, w, h, got, want)
            else:
                bad = LL.compare_planes(got, want)
            findings += [f"{w}x{h} {layout}: {b}" for b in bad]
    assert not findings, "\n".join(findings)


def _run_av_to_uv(hip, torch, r, frp, av, uv, w, h, pitch, off, shifts, cs, rng_):
    """the product on the mirror of the frame `frp` into a destination of FILL laid out as make_dst lays it out -> whole buffer"""
    wholes, views = LL.mirror_planes(torch, LL.frame_planes(r, frp.contents, h))
    host, front = LL.make_dst(h, pitch, off)
    dev = LL.mirror_bytes(torch, host)
    hip.av_to_uv(av, uv, views, w, h, dev[front:], pitch, shifts, colorspace=cs, color_range=rng_)
    torch.cuda.synchronize()
    return _np(dev), front, [_np(t) for t in wholes]


@pytest.mark.gpu
@pytest.mark.parametrize("av,uv", T.FROM_AV)
def test_gpu_av_to_uv_layouts(hip, av, uv):
    import torch
    r = LL.ref()
    findings = []
    for k, (w, h) in enumerate(LL.SIZES):
        line = r.vc_get_linesize(w, r.get_codec_from_name(uv.encode()))
        for j, layout in enumerate(LL.LAYOUTS):
            (cs, rng_), shifts = LL.from_av_params(k + j)
            if av.startswith("yuvj"):
                rng_ = 2
            frp = LL.make_frame_laid_out(r, av, w, h, layout, k, cs, rng_)
            src_before = [p.whole.copy() for p in LL.frame_planes(r, frp.contents, h)]
            pitch, off = LL.dst_layout(layout, line)
            want, front = LL.ref_av_to_uv_laid_out(r, frp, av, uv, h, pitch, off, shifts)
            got, gfront, src_after = _run_av_to_uv(hip, torch, r, frp, av, uv, w, h, pitch, off, shifts, cs, rng_)
            assert gfront == front
            bad = LL.compare_dst(got, want, h, pitch, front, r12l_width=w if LL.from_av_masked(uv, w) else 0)
            if any(not np.array_equal(a, b) for a, b in zip(src_before, src_after)):
                bad.append("the source planes were written")
            if uv in ("RGB", "R12L") and layout == "tight":
                # the ABI takes these destinations at any byte: base + 1 and an odd pitch, held to the reference's lines at the 4-aligned
                # layout above (same source bytes; a destination line's bytes do not depend on its address)
                opitch = line + 1 if line % 2 == 0 else line + 2
                got1, front1, _ = _run_av_to_uv(hip, torch, r, frp, av, uv, w, h, opitch, 1, shifts, cs, rng_)
                twin = aligned_bytes(got1.size, fill=FILL)
                for y in range(h):
                    twin[front1 + y * opitch: front1 + y * opitch + line] = want[front + y * pitch: front + y * pitch + line]
                odd_bad = LL.compare_dst(got1, twin, h, opitch, front1, r12l_width=w if LL.from_av_masked(uv, w) else 0)
                bad += [f"base + 1, pitch {opitch}: {b}" for b in odd_bad]
            r.av_frame_free(C.byref(frp))
            findings += [f"{w}x{h} {layout} cs {cs} range {rng_} shifts {shifts}: {b}" for b in bad]
    assert not findings, "\n".join(findings)


@pytest.mark.gpu
@pytest.mark.parametrize("direction,a,b", [("to", *p) for p in LL.FAST_TO] + [("from", *p) for p in LL.FAST_FROM])
def test_gpu_fast_and_plain_kernels_agree(hip, direction, a, b):
    """launch() takes the 8-pixels-per-lane kernel when the buffer, the pitch and EVERY plane and line size are multiples of 16.  With all of
    them aligned but the last plane (one sample past an aligned address) the plain kernel must run, and gives the same bytes inside the
    lines.  No reference needed; the stand-in only lays the frames out."""
    import torch
    r = LL.ref()
    uv, av = (a, b) if direction == "to" else (b, a)
    fmt = r.ug_stub_pixfmt_by_name(av.encode())
    rng_ = 2 if av.startswith("yuvj") else 1
    for w, h in [(1920, 2), (96, 5)]:
        h = LL.to_av_height(uv, av, h) if direction == "to" else h
        results, keep = [], None
        for layout in ("default", "last_plane_off"):
            if direction == "to":
                with LL.laid_out(r, layout, LL.frame_unit(av)):
                    frp = r.ug_stub_frame_new(fmt, w, h)
                planes = [p.copy() for p in LL.frame_planes(r, frp.contents, h)]
                r.av_frame_free(C.byref(frp))
                for p in planes:
                    p.whole[:] = FILL  # (the default layout comes zeroed)
                wholes, views = LL.mirror_planes(torch, planes)
                hip.uv_to_av(uv, av, LL.mirror_bytes(torch, LL.make_uv_source(r, uv, w, h, 5)), w, h, views)
                torch.cuda.synchronize()
                got = [_np(t) for t in wholes]
                results.append([g[p.off: p.off + p.rows * p.ls].reshape(p.rows, p.ls)[:, : r.ug_stub_plane_line_bytes(fmt, k, w)]
                                for k, (p, g) in enumerate(zip(planes, got))])
                outside = [g.copy() for g in got]
                for k, (p, g) in enumerate(zip(planes, outside)):
                    g[p.off: p.off + p.rows * p.ls].reshape(p.rows, p.ls)[:, : r.ug_stub_plane_line_bytes(fmt, k, w)] = FILL
                    assert (g == FILL).all(), (uv, av, w, h, layout, k, "bytes outside the lines written")
            else:
                frp = LL.make_frame_laid_out(r, av, w, h, layout, 9, 1, rng_)
                planes = LL.frame_planes(r, frp.contents, h)
                if keep is None:  # the same samples in both layouts: the lines of the first frame, which are the shorter ones
                    keep = [p.lines(spare=True).copy() for p in planes]
                for p, kl in zip(planes, keep):
                    p.lines(spare=True)[:, : kl.shape[1]] = kl
                pitch = (r.vc_get_linesize(w, r.get_codec_from_name(uv.encode())) + 15) // 16 * 16
                got, front, _ = _run_av_to_uv(hip, torch, r, frp, av, uv, w, h, pitch, 0, (0, 8, 16), 1, rng_)
                r.av_frame_free(C.byref(frp))
                results.append([got[front: front + h * pitch].reshape(h, pitch)])
                assert (got[:front] == FILL).all() and (got[front + h * pitch:] == FILL).all()
        for k, (x, y) in enumerate(zip(*results)):
            assert np.array_equal(x, y), (a, b, w, h, k, np.argwhere(x != y)[:4])
            assert (x != FILL).any()


@pytest.mark.gpu
@pytest.mark.parametrize("uv,av", LL.READS_DST)
def test_gpu_second_frame_into_the_same_planes(hip, uv, av):
    """k_r10k_to_yuv42Xp10le<2> averages odd pairs with what the chroma planes hold (to_lavc_vid_conv.c:670-677), and the reference reuses
    its output frame from call to call: two different pictures one after the other into the same planes, compared after each.  (The 4:2:2
    row shares the kernel and must not depend on what the planes held.)"""
    import torch
    r = LL.ref()
    for w, h in LL.SIZES:
        srcs = [LL.make_uv_source(r, uv, w, h, seed) for seed in (1, 2)]
        for layout in LL.LAYOUTS:
            states = LL.ref_uv_to_av_laid_out(r, uv, av, srcs, w, h, layout)
            wholes, views = LL.mirror_planes(torch, states[0])
            for n, src in enumerate(srcs):
                hip.uv_to_av(uv, av, LL.mirror_bytes(torch, src), w, h, views)
                torch.cuda.synchronize()
                bad = LL.compare_planes([_np(t) for t in wholes], states[n + 1])
                assert not bad, (w, h, layout, f"after picture {n + 1}", bad)
            alone = LL.ref_uv_to_av_laid_out(r, uv, av, srcs[1:], w, h, layout)[1]
            depends = any(not np.array_equal(x.lines(), y.lines()) for x, y in zip(alone, states[2]))
            assert depends == (av == "yuv420p10le"), "the reference's second picture depends on the first only in the 4:2:0 row"


def _frame(hip, views, w, h):
    f = hip.AvFrame()
    for i, (ptr, ls) in enumerate(views):
        f.data[i], f.linesize[i] = ptr, ls
    f.width, f.height, f.colorspace, f.color_range = w, h, 2, 1
    return f


@pytest.mark.gpu
def test_gpu_lavc_layout_refusals(hip):
    """line sizes and addresses the kernels cannot take are refused with EINVAL before anything is written: the 0xA5 destination and its
    guards stay as they were"""
    import torch
    lib = hip.L.load()
    w, h = 18, 3
    EINVAL = hip.L.EINVAL

    def planes(n, ls, rows=h + 1):
        t = torch.full((GUARD + n * ls * rows + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        return t, [t.data_ptr() + GUARD + i * ls * rows for i in range(n)]

    src = torch.full((GUARD + 4096,), 0x3C, dtype=torch.uint8, device="cuda")
    sp = src.data_ptr() + GUARD

    def to_av(uv, av, n, ls, shift=(0, 0, 0), in_off=0, ls_of=None):
        t, ptrs = planes(n, max(abs(ls), 256))
        views = [(p + shift[i % 3], (ls_of or [ls] * n)[i]) for i, p in enumerate(ptrs)]
        f = _frame(hip, views, w, h)
        rc = lib.ug_hip_uv_to_av(uv.encode(), av.encode(), sp + in_off, C.byref(f), None)
        torch.cuda.synchronize()
        assert rc == EINVAL, (uv, av, ls, shift, in_off, rc)
        assert bool((t == FILL).all()), (uv, av, ls, shift, in_off, "a refused call wrote its planes")

    to_av("UYVY", "yuv444p", 3, 0)                              # linesize 0
    to_av("UYVY", "yuv444p", 3, -64)                            # negative
    to_av("UYVY", "yuv444p", 3, 64, ls_of=[64, 64, 0])          # the last plane's only
    to_av("v210", "yuv422p10le", 3, 64, shift=(0, 1, 0))        # a 16-bit plane at an odd address
    to_av("v210", "yuv422p10le", 3, 64, shift=(0, 0, 1))
    to_av("v210", "yuv422p10le", 3, 63)                         # ... at an odd line size
    to_av("v210", "yuv422p10le", 3, 64, ls_of=[64, 64, 37])
    to_av("R12L", "p210le", 2, 64, shift=(0, 1, 0))
    to_av("v210", "xv30le", 1, 130)                             # a 32-bit packed format off a multiple of 4
    to_av("v210", "xv30le", 1, 128, shift=(2, 0, 0))
    to_av("UYVY", "vuya", 1, 128, shift=(2, 0, 0))
    to_av("R10k", "x2rgb10le", 1, 74)
    for off in (1, 2, 3):                                       # in_data & 3
        to_av("UYVY", "yuv444p", 3, 64, in_off=off)
        to_av("RGB", "gbrp", 3, 64, in_off=off)

    def from_av(av, uv, n, ls, pitch, dst_off=0, shift=(0, 0, 0), ls_of=None):
        t, ptrs = planes(n, 256)
        views = [(p + shift[i % 3], (ls_of or [ls] * n)[i]) for i, p in enumerate(ptrs)]
        f = _frame(hip, views, w, h)
        dst = torch.full((GUARD + 1024 * (h + 1) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        rc = lib.ug_hip_av_to_uv(av.encode(), uv.encode(), dst.data_ptr() + GUARD + dst_off, pitch, C.byref(f), (C.c_int * 3)(0, 8, 16), None)
        torch.cuda.synchronize()
        assert rc == EINVAL, (av, uv, ls, pitch, dst_off, shift, rc)
        assert bool((dst == FILL).all()), (av, uv, ls, pitch, dst_off, "a refused call wrote its destination")

    from_av("yuv444p", "UYVY", 3, 0, 64)                        # linesize 0, negative
    from_av("yuv444p", "UYVY", 3, -64, 64)
    from_av("yuv444p", "UYVY", 3, 64, 0)                        # pitch 0, negative
    from_av("yuv444p", "UYVY", 3, 64, -64)
    from_av("yuv444p10le", "UYVY", 3, 64, 64, shift=(1, 0, 0))  # 16-bit planes at odd addresses / line sizes
    from_av("yuv444p10le", "UYVY", 3, 64, 64, ls_of=[64, 63, 64])
    from_av("p010le", "v210", 2, 64, 128, shift=(0, 1, 0))
    from_av("xv30le", "UYVY", 1, 128, 64, shift=(2, 0, 0))      # 32-bit packed frames
    from_av("xv30le", "UYVY", 1, 126, 64)
    from_av("vuya", "Y416", 1, 128, 256, shift=(1, 0, 0))
    from_av("rgb48le", "RGBA", 1, 128, 128, shift=(1, 0, 0))    # 16-bit samples, packed
    from_av("rgb48le", "R12L", 1, 127, 128)
    for uv, unit in (("UYVY", 4), ("v210", 4), ("RGBA", 4), ("R10k", 4), ("RG48", 2), ("Y416", 2)):  # destination off the codec's unit
        av = "yuv444p10le" if uv in ("R10k", "RG48", "Y416") else "yuv444p"
        ls = 64
        for off in range(1, unit):
            from_av(av, uv, 3, ls, 512, dst_off=off)
            from_av(av, uv, 3, ls, 512 + off)
