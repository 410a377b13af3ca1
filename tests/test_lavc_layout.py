"""The helper of the lavc layout tests (tests/lavc_layout.py) checked on the CPU: the stand-in's layout switch leaves the default layout as it
was, the compiled reference gets through every row x size x layout the GPU tests use, the device mirror keeps addresses congruent, and the
cases held to something else than the reference stay few."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import lavc_layout as LL
import test_lavc_conv as T


def test_default_layout_is_unchanged():
    """mode 0: line sizes rounded up to 64, zeroed planes of linesize * (rows + 1) + 64 bytes that start where they were allocated -- for
    every format of the stand-in's table, before and after the switch was used"""
    r = LL.ref()
    n = r.ug_stub_format_count()
    assert n >= 37
    for use_switch in (False, True):
        if use_switch:
            with LL.laid_out(r, "odd", 2):
                pass
        for i in range(n):
            name = r.ug_stub_format_name(i)
            fmt = r.ug_stub_pixfmt_by_name(name)
            for w, h in ((50, 7), (1920, 2)):
                frp = r.ug_stub_frame_new(fmt, w, h)
                assert frp, name
                planes = LL.frame_planes(r, frp.contents, h)
                assert planes, name
                for k, p in enumerate(planes):
                    lb = r.ug_stub_plane_line_bytes(fmt, k, w)
                    assert lb > 0 and p.ls == (lb + 63) // 64 * 64, (name, k, w)
                    assert p.off == 0 and p.whole.size == p.ls * (p.rows + 1) + 64 and not p.whole.any(), (name, k, w)
                assert r.ug_stub_plane_line_bytes(fmt, len(planes), w) == 0
                r.av_frame_free(C.byref(frp))


@pytest.mark.parametrize("av,unit", [("yuv420p", 1), ("yuv422p10le", 2), ("p010le", 2), ("xv30le", 4), ("y210le", 2), ("gbrap", 1)])
def test_layout_modes(av, unit):
    """the four layouts as the issue states them: line sizes, base addresses, guards, fill"""
    r = LL.ref()
    assert LL.frame_unit(av) == unit
    fmt = r.ug_stub_pixfmt_by_name(av.encode())
    for w, h in LL.SIZES:
        for layout in LL.LAYOUTS + ["last_plane_off"]:
            with LL.laid_out(r, layout, unit, 0xA5):
                frp = r.ug_stub_frame_new(fmt, w, h)
            planes = LL.frame_planes(r, frp.contents, h)
            for k, p in enumerate(planes):
                lb = r.ug_stub_plane_line_bytes(fmt, k, w)
                pad64 = (lb + 63) // 64 * 64
                mode = layout if layout != "last_plane_off" else ("offset" if k == len(planes) - 1 else "default")
                odd = lb + unit + (unit if (lb + unit) % 16 == 0 else 0)
                want_ls, want_off = {"tight": (lb, 256), "odd": (odd, 256), "offset": (pad64 + 64, 256 + unit), "default": (pad64, 256)}[mode]
                assert (p.ls, p.off) == (want_ls, want_off), (av, w, layout, k)
                assert (p.addr - p.off) % 256 == 0 and p.whole.size == p.off + p.ls * (p.rows + 1) + 256
                assert (p.whole == 0xA5).all()
                if mode == "odd":
                    assert p.ls % 16 and p.ls % unit == 0
            r.av_frame_free(C.byref(frp))


@pytest.mark.parametrize("direction", ["to", "from"])
def test_reference_completes_every_case_and_few_are_masked(direction):
    """one child process per direction, so that an assertion of the reference fails this test and not the test run.  Cases held to something
    else than the reference (Y216 -> p010le with padded lines, the tail bits of ragged R12L lines) or skipped stay under 5 % of all cases"""
    T.ref()
    res = subprocess.run([sys.executable, os.path.join(T.HERE, "lavc_layout.py"), direction], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    got = json.loads([l for l in res.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    rows = len(T.TO_AV) if direction == "to" else len(T.FROM_AV)
    assert got["cases"] == rows * len(LL.SIZES) * len(LL.LAYOUTS)
    assert (got["masked"] + got["skipped"]) * 20 < got["cases"], got


def test_mirror_keeps_addresses_congruent_and_strides():
    import torch
    r = LL.ref()
    for av in ("yuv420p10le", "xv30le", "nv12"):
        for layout in LL.LAYOUTS + ["last_plane_off"]:
            frp = LL.make_frame_laid_out(r, av, 50, 7, layout, 3, 1, 1)
            planes = LL.frame_planes(r, frp.contents, 7)
            wholes, views = LL.mirror_planes(torch, planes, device="cpu")
            for p, t, v in zip(planes, wholes, views):
                assert v.data_ptr() % 256 == p.addr % 256 and v.stride(0) == p.ls and v.stride(1) == 1 and tuple(v.shape) == (p.rows, p.ls)
                assert np.array_equal(t.numpy(), p.whole) and np.array_equal(v.numpy(), p.lines())
                assert v.data_ptr() - t.data_ptr() == p.off
            assert not LL.compare_planes([t.numpy() for t in wholes], planes, spare_was=[p.lines(spare=True)[-1] for p in planes])
            r.av_frame_free(C.byref(frp))
    host = LL.aligned_bytes(100, fill=7)[5:]
    assert LL.mirror_bytes(torch, host, device="cpu").data_ptr() % 256 == 5


def test_compare_planes_and_compare_dst_find_what_they_should():
    r = LL.ref()
    with LL.laid_out(r, "odd", 2):
        frp = r.ug_stub_frame_new(r.ug_stub_pixfmt_by_name(b"yuv422p10le"), 18, 3)
    want = [p.copy() for p in LL.frame_planes(r, frp.contents, 3)]
    r.av_frame_free(C.byref(frp))

    def got():
        return [p.whole.copy() for p in want]
    assert LL.compare_planes(got(), want) == []
    g = got()
    g[1][want[1].off + want[1].ls + 3] ^= 1
    assert "plane 1" in LL.compare_planes(g, want)[0] and "line 1 byte 3" in LL.compare_planes(g, want)[0]
    g = got()
    g[0][want[0].off - 1] = 0
    assert "in front of" in LL.compare_planes(g, want)[0]
    g = got()
    g[2][-1] = 0
    assert "behind" in LL.compare_planes(g, want)[0]
    g = got()
    g[0][want[0].off + want[0].ls - 1] = 0  # the last padding byte of line 0
    assert "differ" in LL.compare_planes(g, want)[0]
    assert "padding" in LL.compare_planes(g, want, line_bytes=[36, 18, 18])[0]
    g = got()
    g[0][want[0].off + 3 * want[0].ls] = 0  # the spare line: the product's must stay as it was, the reference's is its own
    assert "behind the last line" in LL.compare_planes(g, want)[0]
    spilled = [p.copy() for p in want]
    spilled[0].whole[want[0].off + 3 * want[0].ls] = 0
    assert LL.compare_planes(got(), spilled) == []

    for layout, line in (("tight", 36), ("odd", 36), ("odd", 44), ("offset", 36)):
        pitch, off = LL.dst_layout(layout, line)
        assert pitch % 4 == 0 and pitch >= line and (layout != "odd" or pitch % 16) and (layout != "offset" or (off, pitch) == (4, 128))
        want_d, front = LL.make_dst(3, pitch, off)
        assert want_d.ctypes.data % 256 == 0 and front == 256 + off
        assert LL.compare_dst(want_d.copy(), want_d, 3, pitch, front) == []
        for at, word in ((front - 1, "in front of"), (front + pitch, "differ"), (want_d.size - 1, "behind")):
            g = want_d.copy()
            g[at] = 0
            assert word in LL.compare_dst(g, want_d, 3, pitch, front)[0]
        g = want_d.copy()
        g[front + 3 * pitch] = 0  # the spare line: the reference's own, the product's stays
        assert "spare line" in LL.compare_dst(g, want_d, 3, pitch, front)[0]
        assert LL.compare_dst(want_d, g, 3, pitch, front) == []
