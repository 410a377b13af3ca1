"""CPU: the colour / mirror filters without a device -- the numpy restatement (tests/pixel_filter_restatement.py) against the reference's compiled
modules (tests/golden/pixel_filter_ref.npz, written by tests/golden/make_pixel_filter_golden.py), 0 bytes differing under two conditions:
  1. matrix ... no-bound-check and matrix2: elements whose exact value lies outside the output type are undefined in the reference and left out;
  2. gamma: the reference never writes the last len % cpus elements (gamma.cpp:133-138; they still hold the harness's 0xA5); cpus from the fixture.
Both shares stay below 5 % per case.  Then the host half of the C ABI: ug_hip_gamma_lut against the tables the fixture implies,
ug_hip_matrix2_preset, the argument rules of ug_hip_pixel_filter (refused before any device call: this machine has none), the export map."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_pixel_filter_golden as gen  # noqa: E402
import pixel_filter_restatement as rs  # noqa: E402

from ultragrid_amd import lib  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "pixel_filter_ref.npz"))
META = json.loads(str(GOLD["meta"]))
CPUS = int(GOLD["cpus"])
IDS = [f"{k}-{m['name']}-{m['codec']}-{m['w']}x{m['h']}" for k, m in enumerate(META)]


def test_fixture_covers_the_cases_of_the_generator():
    assert [(m["name"], m["options"], m["codec"], m["w"], m["h"]) for m in META] == [c[:5] for c in gen.cases()]
    gam = [m for m in META if m["name"] == "gamma" and m["status"] == "new"]
    assert len(gam) == 18 and all(GOLD[m["input"]].size // (2 if m["codec"] == "RG48" else 1) >= 10240 for m in gam)
    assert any(all((m["w"] * m["h"] * 3) % n == 0 for n in range(1, 9)) for m in gam)


@pytest.mark.parametrize("k", range(len(META)), ids=IDS)
def test_restatement_equals_the_reference(k):
    m = META[k]
    data = GOLD[m["input"]]
    want = rs.run_filter(m["name"], "" if m["options"] == "-" else m["options"], m["codec"], m["w"], m["h"], data)
    # what the module hands back: a frame of its own, the input frame, NULL; matrix2 returns its unwritten frame for a codec it does not take
    assert m["status"] == {"unwritten": "new"}.get(want["status"], want["status"])
    if want["status"] in ("null", "same"):
        assert m["out_codec"] == m["codec"]
        return
    assert (m["out_codec"], m["out_w"], m["out_h"]) == (want["codec"], m["w"], m["h"])
    assert m["data_len"] == rs.linesize(want["codec"], m["w"]) * m["h"]
    if want["status"] == "unwritten":
        return
    ref = GOLD[f"out_{k}"]
    left = gen.left_out(want, ref, CPUS, m["name"], m["codec"])
    unchecked = m["name"] == "matrix2" or "no-bound-check" in m["options"]
    if not (unchecked or m["name"] == "gamma"):
        assert not left.any()
    print(f"left out {left.mean():.4%}")
    assert left.mean() < 0.05
    assert int(np.count_nonzero((want["out"] != ref) & ~left)) == 0
    if m["name"] == "gamma":
        assert (ref[left] == 0xA5).all()  # the reference's tail: the pre-fill


def _table(in_bits, out_bits, gamma):
    buf = (C.c_uint8 * ((1 << in_bits) * (out_bits // 8)))()
    assert lib.load().ug_hip_gamma_lut(gamma, in_bits, out_bits, buf) == lib.SUCCESS
    return np.frombuffer(buf, np.uint16 if out_bits == 16 else np.uint8)


@pytest.mark.parametrize("gamma", ["0.45", "1.0", "2.2"])
def test_gamma_lut_equals_the_tables_of_the_reference(gamma):
    """every entry of the reference's four tables that the fixture's frames reach (all 256 of the 8-bit-input ones)"""
    seen = set()
    for k, m in enumerate(META):
        if m["name"] != "gamma" or m["status"] != "new" or m["options"].split(":")[0] != gamma:
            continue
        ib, ob = (16 if m["codec"] == "RG48" else 8), (16 if m["out_codec"] == "RG48" else 8)
        src = GOLD[m["input"]].view(np.uint16 if ib == 16 else np.uint8)
        ref = GOLD[f"out_{k}"].view(np.uint16 if ob == 16 else np.uint8)
        n = src.size - src.size % CPUS
        table = _table(ib, ob, float(gamma))
        assert np.array_equal(table[src[:n]], ref[:n]), (ib, ob)
        assert np.array_equal(table, rs.gamma_lut(float(gamma), ib, ob))
        if ib == 8:
            assert np.unique(src[:n]).size == 256
        seen.add((ib, ob))
    assert seen == {(8, 8), (8, 16), (16, 8), (16, 16)}


def test_gamma_lut_refuses_what_has_no_table():
    buf = (C.c_uint8 * 131072)()
    l = lib.load()
    for g in (0.0, -1.0, float("inf"), float("nan")):
        assert l.ug_hip_gamma_lut(g, 8, 8, buf) == lib.EINVAL  # the reference warns and converts inf (gamma.cpp:170-172): a stated deviation
    assert l.ug_hip_gamma_lut(2.2, 10, 8, buf) == lib.EINVAL and l.ug_hip_gamma_lut(2.2, 8, 12, buf) == lib.EINVAL
    assert l.ug_hip_gamma_lut(2.2, 8, 8, None) == lib.EINVAL


def test_matrix2_preset():
    m = (C.c_double * 9)()
    l = lib.load()
    assert l.ug_hip_matrix2_preset(b"y601_to_y709", m) == lib.SUCCESS
    assert list(m) == [1, -0.11555, -0.207938, 0, 1.01864, 0.114618, 0, 0.075049, 1.025327] == rs.Y601_TO_Y709  # matrix2.c:69-73
    assert l.ug_hip_matrix2_preset(b"y709_to_y601", m) == lib.EINVAL and l.ug_hip_matrix2_preset(None, m) == lib.EINVAL


def test_supported_pairs():
    l = lib.load()
    want = {lib.PXF_MATRIX: {"UYVY", "RGB", "RG48"}, lib.PXF_MATRIX2: {"UYVY", "v210", "Y416"}, lib.PXF_LUT: {"RGB", "RG48"},
            lib.PXF_GRAY: {"UYVY"}, lib.PXF_MIRROR: {"UYVY"}, lib.PXF_FLIP: set(lib.PF_NAMES)}
    for op, names in want.items():
        assert {n for n, f in lib.PF_NAMES.items() if l.ug_hip_pixel_filter_supported(op, f) == 1} == names, op
    assert l.ug_hip_pixel_filter_supported(6, lib.PF_UYVY) == 0 and l.ug_hip_pixel_filter_supported(-1, lib.PF_UYVY) == 0
    assert l.ug_hip_pixel_filter_supported(lib.PXF_FLIP, lib.PF_I420) == 0 and l.ug_hip_pixel_filter_supported(lib.PXF_FLIP, lib.PF_NONE) == 0


_S, _D, _T = 0x7F0000001000, 0x7F0100001000, 0x7F0200001000  # never dereferenced: every case below is refused on its arguments alone
_ID = [1, 0, 0, 0, 1, 0, 0, 0, 1]


def _desc(op=lib.PXF_MATRIX, fmt=lib.PF_RGB, **kw):
    d = dict(src=_S, dst=_D, op=op, format=fmt, out_format=lib.PF_NONE, width=64, lines=16, src_pitch=0, dst_pitch=0, frames=1, src_frame_stride=0,
             dst_frame_stride=0, matrix=(C.c_double * 9)(*_ID), clamp=1, lut_dev=_T)
    d.update(kw)
    if not isinstance(d["matrix"], C.Array):
        d["matrix"] = (C.c_double * 9)(*d["matrix"])
    return lib.PixelFilterDesc(**d)


BIG = 2.0 ** 31 / 98303
REFUSED = [
    ("NULL src", dict(src=None), lib.EINVAL),
    ("NULL dst", dict(dst=None), lib.EINVAL),
    ("op below", dict(op=-1), lib.EINVAL),
    ("op above", dict(op=6), lib.EINVAL),
    ("matrix on RGBA", dict(fmt=lib.PF_RGBA), lib.EUNSUPP),
    ("matrix2 on RGB", dict(op=lib.PXF_MATRIX2), lib.EUNSUPP),
    ("LUT on UYVY", dict(op=lib.PXF_LUT, fmt=lib.PF_UYVY), lib.EUNSUPP),
    ("gray on RGB", dict(op=lib.PXF_GRAY), lib.EUNSUPP),
    ("mirror on v210", dict(op=lib.PXF_MIRROR, fmt=lib.PF_V210), lib.EUNSUPP),
    ("flip on I420", dict(op=lib.PXF_FLIP, fmt=lib.PF_I420), lib.EUNSUPP),
    ("unknown format", dict(fmt=99), lib.EUNSUPP),
    ("matrix RGB out as RG48", dict(out_format=lib.PF_RG48), lib.EUNSUPP),
    ("matrix UYVY out as UYVY", dict(fmt=lib.PF_UYVY, out_format=lib.PF_UYVY), lib.EUNSUPP),
    ("LUT out as UYVY", dict(op=lib.PXF_LUT, out_format=lib.PF_UYVY), lib.EUNSUPP),
    ("LUT without a table", dict(op=lib.PXF_LUT, lut_dev=None), lib.EINVAL),
    ("LUT 16-bit table at an odd address", dict(op=lib.PXF_LUT, out_format=lib.PF_RG48, lut_dev=_T + 1), lib.EINVAL),
    ("matrix NaN", dict(matrix=[1, 0, 0, 0, float("nan"), 0, 0, 0, 1]), lib.EINVAL),
    ("matrix inf", dict(matrix=[1, 0, 0, 0, 1, 0, 0, float("inf"), 1]), lib.EINVAL),
    ("matrix row sum above the bound", dict(matrix=[1, 0, 0, 0, 1, 0, BIG * 0.51, -BIG * 0.51, 0]), lib.EINVAL),
    ("matrix2 row sum above the bound", dict(op=lib.PXF_MATRIX2, fmt=lib.PF_Y416, matrix=[30000, 0, 0, 0, 1, 0, 0, 0, 1]), lib.EINVAL),
    ("width 0", dict(width=0), lib.EINVAL),
    ("width above 65536", dict(width=65537), lib.EINVAL),
    ("lines 0", dict(lines=0), lib.EINVAL),
    ("lines above 65536", dict(lines=65537), lib.EINVAL),
    ("frame above INT_MAX", dict(fmt=lib.PF_RG48, width=65536, lines=65536), lib.EINVAL),
    ("src pitch below the line", dict(src_pitch=191), lib.EINVAL),
    ("dst pitch below the line", dict(dst_pitch=100), lib.EINVAL),
    ("dst pitch below the RGB line of UYVY", dict(fmt=lib.PF_UYVY, dst_pitch=128), lib.EINVAL),
    ("pitch times lines above INT_MAX", dict(src_pitch=2 ** 31 - 1, lines=2), lib.EINVAL),
    ("RG48 odd pitch", dict(fmt=lib.PF_RG48, src_pitch=385), lib.EINVAL),
    ("v210 pitch % 4", dict(op=lib.PXF_MATRIX2, fmt=lib.PF_V210, dst_pitch=258), lib.EINVAL),
    ("RG48 odd src", dict(fmt=lib.PF_RG48, src=_S + 1), lib.EINVAL),
    ("Y416 odd dst", dict(op=lib.PXF_MATRIX2, fmt=lib.PF_Y416, dst=_D + 1), lib.EINVAL),
    ("v210 dst % 4", dict(op=lib.PXF_MATRIX2, fmt=lib.PF_V210, dst=_D + 2), lib.EINVAL),
    ("UYVY matrix odd width", dict(fmt=lib.PF_UYVY, width=63), lib.EINVAL),
    ("frames 0", dict(frames=0), lib.EINVAL),
    ("frames above 65535", dict(frames=65536, src_frame_stride=4096, dst_frame_stride=4096), lib.EINVAL),
    ("src stride below a frame", dict(frames=2, src_frame_stride=64 * 3 * 16 - 1, dst_frame_stride=4096), lib.EINVAL),
    ("dst stride below a frame", dict(frames=2, src_frame_stride=4096, dst_frame_stride=100), lib.EINVAL),
    ("RG48 odd stride", dict(fmt=lib.PF_RG48, frames=2, src_frame_stride=64 * 6 * 16 + 1, dst_frame_stride=64 * 6 * 16), lib.EINVAL),
    ("dst == src", dict(dst=_S), lib.EINVAL),
    ("flip dst == src", dict(op=lib.PXF_FLIP, dst=_S), lib.EINVAL),
    ("gray dst == src", dict(op=lib.PXF_GRAY, fmt=lib.PF_UYVY, dst=_S), lib.EINVAL),
    ("LUT of equal depth dst == src", dict(op=lib.PXF_LUT, dst=_S), lib.EINVAL),
    ("dst inside src", dict(dst=_S + 64 * 3 * 16 - 1), lib.EINVAL),
    ("second frame's dst over the first's src", dict(frames=2, src_frame_stride=4096, dst_frame_stride=4096, dst=_S - 4096 - 1), lib.EINVAL),
]


@pytest.mark.parametrize("what,kw,rc", REFUSED, ids=[r[0] for r in REFUSED])
def test_argument_rules_are_checked_without_a_device(what, kw, rc):
    l = lib.load()
    assert l.ug_hip_pixel_filter(C.byref(_desc(**kw)), None) == rc, (what, lib.last_error())
    assert lib.last_error()


def test_null_descriptor():
    assert lib.load().ug_hip_pixel_filter(None, None) == lib.EINVAL


def test_matrix_just_below_the_bound_passes_the_matrix_rule():
    """(it is refused one rule later, for its NULL source: the order of the checks is matrix, then pointers' alignment and overlap)"""
    l = lib.load()
    ok = [BIG * 0.4999, -BIG * 0.4999, 0, 0, 1, 0, 0, 0, 1]
    assert l.ug_hip_pixel_filter(C.byref(_desc(matrix=ok, dst=_S)), None) == lib.EINVAL and b"overlap" in l.ug_hip_last_error_string()
    bad = [BIG * 0.5001, -BIG * 0.5001, 0, 0, 1, 0, 0, 0, 1]
    assert l.ug_hip_pixel_filter(C.byref(_desc(matrix=bad, dst=_S)), None) == lib.EINVAL and b"matrix" in l.ug_hip_last_error_string()


def test_symbols_are_exported_and_mapped():
    names = ["ug_hip_pixel_filter", "ug_hip_pixel_filter_supported", "ug_hip_gamma_lut", "ug_hip_matrix2_preset"]
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "ultragrid_amd", "libug_mi355x.so")], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1].split("@")[0] for line in out.splitlines() if line.strip()}
    committed = open(os.path.join(ROOT, "ultragrid_amd", "csrc", "libug_mi355x.map")).read()
    for n in names:
        assert n in exported and f"        {n};\n" in committed and n in lib.SYMBOLS
