"""CPU: frame composition without a device -- the numpy restatement (tests/compose_restatement.py) against tests/golden/compose_ref.npz, whose `inside`
cases tests/golden/make_compose_golden.py asserted equal to the reference's compiled modules byte for byte (0 differing, nothing left out, no byte
behind a buffer changed) when it wrote them; the three geometry helpers of the C ABI against the restatement over sweeps; the argument rules of
ug_hip_compose (refused before any device call: this machine has none); the export map."""
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
import compose_restatement as rs  # noqa: E402
import make_compose_golden as gen  # noqa: E402

from ultragrid_amd import lib  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "compose_ref.npz"))
META = json.loads(str(GOLD["meta"]))
IDS = [f"{k}-{m['kind']}-{m['name']}-{m['codec']}-{'x'.join(map(str, m['frames'][0]))}" for k, m in enumerate(META)]
PF = dict(lib.PF_NAMES)


def fixture_inputs(k):
    m = META[k]
    ins = [GOLD[f"in_{m['codec']}_{w}x{h}x{m['tiles']}"] for w, h in m["frames"]]
    overlay = (GOLD[f"logo_{k}"], m["logo"][0], m["logo"][1]) if m["logo"] else None
    return ins, overlay


def test_fixture_covers_the_cases_of_the_generator():
    keys = ("name", "options", "codec", "frames", "mode", "tiles", "kind", "logo")
    assert [[m[x] for x in keys] for m in META] == [[json.loads(json.dumps(c[x])) for x in keys] for c in gen.cases()]
    inside = [m for m in META if m["kind"] == "inside"]
    assert len(inside) >= 100 and {m["name"] for m in inside} == {"crop", "border", "interlace", "interlaced_3d", "split", "logo"}
    # every inside case was run through the reference and stayed in its buffers; every slip of DESIGN.md 4.13 has a deviating case
    assert all("ref_ret" in f and f["ref_pad"] in (0, -1) for m in inside for f in m["frames_meta"])
    dev = {m["name"] for m in META if m["kind"] == "deviating"}
    assert dev == {"crop", "border", "interlaced_3d", "logo"}
    assert all(m.get("ref_fault") or all(f["ref_pad"] > 0 for f in m["frames_meta"]) for m in META if m["name"] == "interlaced_3d" and m["kind"] == "deviating")


def test_logo_widths_inside_and_deviating_are_the_ones_the_segment_arithmetic_gives():
    """logo.c:198-199: dec_width = (lw + 1) / bb * bb against the lw pixels blended per line (+ 1 decoded for an odd UYVY width)"""
    for codec, mod, ok in (("UYVY", 4, {0, 3}), ("RGBA", 4, {0, 3}), ("RGB", 3, {0, 2}), ("RG48", 6, {0, 5})):
        for lw in range(1, 40):
            assert rs.logo_inside(codec, lw) == (lw % mod in ok), (codec, lw)
    for m in META:
        if m["name"] == "logo" and m["codec"] != "v210" and len(m["frames"]) == 1 and m["frames"][0][0] >= m["logo"][0]:
            assert (m["kind"] == "inside") == rs.logo_inside(m["codec"], m["logo"][0]), m


@pytest.mark.parametrize("k", range(len(META)), ids=IDS)
def test_restatement_equals_the_fixture(k):
    m = META[k]
    ins, overlay = fixture_inputs(k)
    if m["codec"] == "v210" and m["name"] in ("border", "logo"):  # a codec the module refuses: false, or the frame as it came
        assert [f["ret"] for f in m["frames_meta"]] == [{"border": "false", "logo": "same"}[m["name"]]]
        return
    want = gen.restate(m, ins, overlay)
    for i, (wf, fm) in enumerate(zip(want, m["frames_meta"])):
        assert (wf is None) == fm["refused"]
        if wf is None:
            continue
        assert (wf["ret"], wf["w"], wf["h"], wf["tile_count"], wf["interlacing"], wf["fps"]) == \
            (fm["ret"], fm["w"], fm["h"], fm["tile_count"], fm["interlacing"], fm["fps"])
        if m["kind"] == "inside":  # what the reference's module answered, as the harness printed it
            assert fm["ref_ret"] == wf["ret"] and fm["ref_desc"][:2] == [wf["w"], wf["h"]] and fm["ref_desc"][2] == m["codec"]
            assert fm["ref_desc"][3:6] == [wf["interlacing"], wf["fps"], wf["tile_count"]]
        if "out" in wf:
            assert int(np.count_nonzero(wf["out"] != GOLD[f"out_{k}_{i}"])) == 0
        else:
            assert f"out_{k}_{i}" not in GOLD.files


# ---------------------------------------------------------------- geometry helpers ----------------------------------------------------------------
def _crop(fmt, *a):
    r = [C.c_int(-7) for _ in range(4)]
    rc = lib.load().ug_hip_crop_geometry(fmt, *a, *[C.byref(v) for v in r])
    return rc, tuple(v.value for v in r)


def _logo(fmt, *a):
    rx, ry = C.c_int(-7), C.c_int(-7)
    rc = lib.load().ug_hip_logo_geometry(fmt, *a, C.byref(rx), C.byref(ry))
    return rc, (rx.value, ry.value)


@pytest.mark.parametrize("codec", ["UYVY", "RGB", "RGBA", "RG48", "v210", "R12L", "Y416", "R10k"])
def test_crop_geometry_equals_the_restatement(codec):
    """every (W, want_w, xoff) with W <= 40 -- v210 and R12L go through get_bpp's doubles (8 / 3, 4.5) --, and the vertical half on its own"""
    for w in list(range(1, 41)) + [96, 1920]:
        for want in list(range(0, w + 3)) if w <= 40 else (0, 6, 47, 95, 100, 1000, 1919):
            for xoff in (0, 1, 2, 3, 5, 7, 8, 12, 17, w - 1, w, w + 5):
                rc, got = _crop(PF[codec], w, 7, want, 3, xoff, 2)
                assert rc == lib.SUCCESS and got == rs.crop_geometry(codec, w, 7, want, 3, xoff, 2), (w, want, xoff, got)
    for h in range(1, 9):
        for want in range(0, h + 2):
            for yoff in range(0, h + 2):
                rc, got = _crop(PF[codec], 48, h, 0, want, 0, yoff)
                assert rc == lib.SUCCESS and got == rs.crop_geometry(codec, 48, h, 0, want, 0, yoff)


@pytest.mark.parametrize("codec", ["UYVY", "RGB", "RGBA", "RG48", "v210", "R12L"])
def test_logo_geometry_equals_the_restatement(codec):
    """every (W, lw, x) with W <= 40, logos wider than the frame included: W - lw < 0 rounds TOWARD ZERO by the block's byte count"""
    for w in range(1, 41):
        for lw in range(1, 46):
            for x in (-1, 0, 1, 2, 3, 4, 5, 6, 7, 11, 12, 35, w - lw, w - lw + 1, w):
                rc, got = _logo(PF[codec], w, 9, lw, 3, x, 2)
                assert rc == lib.SUCCESS and got == rs.logo_geometry(codec, w, 9, lw, 3, x, 2), (w, lw, x, got)
    for h in range(1, 8):
        for lh in range(1, 9):
            for y in (-1, 0, 1, 3, h - lh, h - lh + 1, h):
                rc, got = _logo(PF[codec], 16, h, 4, lh, 4, y)
                assert rc == lib.SUCCESS and got == rs.logo_geometry(codec, 16, h, 4, lh, 4, y)
    bb = rs.BLOCK[codec][0]
    assert _logo(PF[codec], 8, 4, 9, 2, -1, -1)[1] == (0, 2)  # one pixel too wide: -1 / bb * bb == 0, the slip ug_hip_compose refuses
    assert _logo(PF[codec], 8, 4, 8 + bb, 2, -1, -1)[1] == (-bb, 2)


def test_border_pattern_equals_the_restatement():
    rng = np.random.default_rng(5)
    colours = [(0xff, 0xff, 0x00, 0xff), (0, 0, 0, 0), (255, 255, 255, 255)] + [tuple(int(v) for v in rng.integers(0, 256, 4)) for _ in range(200)]
    for codec in ("UYVY", "RGB", "RGBA"):
        for col in colours:
            out = (C.c_ubyte * 4)()
            assert lib.load().ug_hip_border_pattern(PF[codec], (C.c_ubyte * 4)(*col), out) == lib.SUCCESS
            assert bytes(out) == rs.border_pattern(codec, col).tobytes(), (codec, col)
    out = (C.c_ubyte * 4)()
    assert lib.load().ug_hip_border_pattern(lib.PF_V210, (C.c_ubyte * 4)(), out) == lib.EUNSUPP
    assert lib.load().ug_hip_border_pattern(lib.PF_RGB, None, out) == lib.EINVAL and lib.load().ug_hip_border_pattern(lib.PF_RGB, out, None) == lib.EINVAL


def test_geometry_helpers_refuse_what_is_no_geometry():
    for a in ((0, 4, 0, 0, 0, 0), (4, 0, 0, 0, 0, 0), (65537, 4, 0, 0, 0, 0), (8, 4, -1, 0, 0, 0), (8, 4, 0, -1, 0, 0), (8, 4, 0, 0, -1, 0), (8, 4, 0, 0, 0, -1),
              (8, 4, 65537, 0, 0, 0), (8, 4, 0, 0, 2 ** 31 - 1, 0)):
        assert _crop(lib.PF_UYVY, *a)[0] == lib.EINVAL, a
    assert _crop(lib.PF_I420, 8, 4, 0, 0, 0, 0)[0] == lib.EUNSUPP and _crop(99, 8, 4, 0, 0, 0, 0)[0] == lib.EUNSUPP
    assert lib.load().ug_hip_crop_geometry(lib.PF_UYVY, 8, 4, 0, 0, 0, 0, None, None, None, None) == lib.EINVAL
    for a in ((0, 4, 2, 2, 0, 0), (8, 4, 0, 2, 0, 0), (8, 4, 2, 65537, 0, 0), (8, 4, 2, 2, 2 ** 31 - 1, 0), (8, 4, 2, 2, 0, -2 ** 31)):
        assert _logo(lib.PF_UYVY, *a)[0] == lib.EINVAL, a
    assert _logo(lib.PF_I420, 8, 4, 2, 2, 0, 0)[0] == lib.EUNSUPP
    assert lib.load().ug_hip_logo_geometry(lib.PF_UYVY, 8, 4, 2, 2, 0, 0, None, None) == lib.EINVAL


def test_supported_pairs():
    l = lib.load()
    packed = set(lib.PF_NAMES)
    want = {lib.CMP_CROP: packed, lib.CMP_INTERLACE: packed, lib.CMP_INTERLACED_3D: packed, lib.CMP_SPLIT: packed,
            lib.CMP_BORDER: {"UYVY", "RGB", "RGBA"}, lib.CMP_LOGO: {"UYVY", "RGB", "RGBA", "RG48"}}
    for op, names in want.items():
        assert {n for n, f in lib.PF_NAMES.items() if l.ug_hip_compose_supported(op, f) == 1} == names, op
    assert l.ug_hip_compose_supported(6, lib.PF_UYVY) == 0 and l.ug_hip_compose_supported(-1, lib.PF_UYVY) == 0
    assert l.ug_hip_compose_supported(lib.CMP_CROP, lib.PF_I420) == 0 and l.ug_hip_compose_supported(lib.CMP_CROP, lib.PF_UYVY_GL) == 0


# ------------------------------------------------------------------ argument rules ------------------------------------------------------------------
_S, _S2, _D, _T = 0x7F0000001000, 0x7F0080001000, 0x7F0100001000, 0x7F0200001000  # never dereferenced: every case below is refused on its arguments alone
_L = 64 * 2  # the UYVY line of the default descriptor


def _desc(op=lib.CMP_CROP, fmt=lib.PF_UYVY, **kw):
    d = dict(src=_S, src2=_S2, dst=_D, op=op, format=fmt, width=64, lines=16, frames=1, xoff_bytes=8, yoff=2, out_line_bytes=32, out_lines=4, border_w=4,
             border_h=2, logo=_T, logo_w=8, logo_h=4, rect_x=4, rect_y=2, grid_x=2, grid_y=2)
    if op == lib.CMP_LOGO:
        d["src"] = None
    d.update(kw)
    return lib.ComposeDesc(**d)


REFUSED = [
    ("NULL src", dict(src=None), lib.EINVAL),
    ("NULL dst", dict(dst=None), lib.EINVAL),
    ("interlace NULL src2", dict(op=lib.CMP_INTERLACE, src2=None), lib.EINVAL),
    ("interlaced_3d NULL src2", dict(op=lib.CMP_INTERLACED_3D, src2=None), lib.EINVAL),
    ("op below", dict(op=-1), lib.EINVAL),
    ("op above", dict(op=6), lib.EINVAL),
    ("crop on I420", dict(fmt=lib.PF_I420), lib.EUNSUPP),
    ("unknown format", dict(fmt=99), lib.EUNSUPP),
    ("border on v210", dict(op=lib.CMP_BORDER, fmt=lib.PF_V210), lib.EUNSUPP),
    ("border on RG48", dict(op=lib.CMP_BORDER, fmt=lib.PF_RG48), lib.EUNSUPP),
    ("logo on v210", dict(op=lib.CMP_LOGO, fmt=lib.PF_V210), lib.EUNSUPP),
    ("logo on YUYV", dict(op=lib.CMP_LOGO, fmt=lib.PF_YUYV), lib.EUNSUPP),
    ("logo on R12L", dict(op=lib.CMP_LOGO, fmt=lib.PF_R12L), lib.EUNSUPP),
    ("width 0", dict(width=0), lib.EINVAL),
    ("width above 65536", dict(width=65537), lib.EINVAL),
    ("lines 0", dict(lines=0), lib.EINVAL),
    ("lines above 65536", dict(lines=65537), lib.EINVAL),
    ("frame above INT_MAX", dict(op=lib.CMP_INTERLACE, fmt=lib.PF_RG48, width=65536, lines=65536), lib.EINVAL),
    ("src pitch below the line", dict(src_pitch=_L - 1), lib.EINVAL),
    ("dst pitch below the cropped line", dict(dst_pitch=31), lib.EINVAL),
    ("interlace dst pitch below the line", dict(op=lib.CMP_INTERLACE, dst_pitch=_L - 1), lib.EINVAL),
    ("pitch times lines above INT_MAX", dict(src_pitch=2 ** 31 - 1, lines=2, yoff=0, out_lines=1), lib.EINVAL),
    ("frames 0", dict(frames=0), lib.EINVAL),
    ("frames above 65535", dict(frames=65536, src_frame_stride=4096, dst_frame_stride=4096), lib.EINVAL),
    ("src stride below a frame", dict(frames=2, src_frame_stride=_L * 16 - 1, dst_frame_stride=4096), lib.EINVAL),
    ("dst stride below a frame", dict(frames=2, src_frame_stride=4096, dst_frame_stride=32 * 4 - 1), lib.EINVAL),
    ("crop negative xoff", dict(xoff_bytes=-4), lib.EINVAL),
    ("crop negative yoff", dict(yoff=-1), lib.EINVAL),
    ("crop no bytes", dict(out_line_bytes=0), lib.EINVAL),
    ("crop no lines", dict(out_lines=0), lib.EINVAL),
    ("crop beyond the source line", dict(xoff_bytes=_L - 31), lib.EINVAL),
    ("crop beyond the last line", dict(yoff=13), lib.EINVAL),
    ("crop dst == src", dict(dst=_S), lib.EINVAL),
    ("crop dst inside src", dict(dst=_S + _L * 16 - 1), lib.EINVAL),
    ("border negative width", dict(op=lib.CMP_BORDER, border_w=-1), lib.EINVAL),
    ("border negative height", dict(op=lib.CMP_BORDER, border_h=-1), lib.EINVAL),
    ("border wider than the frame", dict(op=lib.CMP_BORDER, border_w=65), lib.EINVAL),
    ("border 2 * border_h above lines", dict(op=lib.CMP_BORDER, border_h=9), lib.EINVAL),
    ("border dst == src", dict(op=lib.CMP_BORDER, dst=_S), lib.EINVAL),
    ("interlace dst == src2", dict(op=lib.CMP_INTERLACE, dst=_S2), lib.EINVAL),
    ("interlace second frame's dst over src2", dict(op=lib.CMP_INTERLACE, frames=2, src_frame_stride=4096, dst_frame_stride=4096, dst=_S2 - 4096 - 1), lib.EINVAL),
    ("interlaced_3d odd lines", dict(op=lib.CMP_INTERLACED_3D, lines=15), lib.EINVAL),
    ("interlaced_3d dst == src", dict(op=lib.CMP_INTERLACED_3D, dst=_S), lib.EINVAL),
    ("split grid 0", dict(op=lib.CMP_SPLIT, grid_x=0), lib.EINVAL),
    ("split negative grid", dict(op=lib.CMP_SPLIT, grid_y=-2), lib.EINVAL),
    ("split grid that does not divide the width", dict(op=lib.CMP_SPLIT, grid_x=3), lib.EINVAL),
    ("split grid that does not divide the lines", dict(op=lib.CMP_SPLIT, grid_y=3), lib.EINVAL),
    ("split v210 tile of half a block", dict(op=lib.CMP_SPLIT, fmt=lib.PF_V210, width=96, grid_x=32), lib.EUNSUPP),
    ("split v210 tile of a fractional byte count", dict(op=lib.CMP_SPLIT, fmt=lib.PF_V210, width=96, grid_x=24), lib.EUNSUPP),
    ("split R12L tile of half a block", dict(op=lib.CMP_SPLIT, fmt=lib.PF_R12L, width=64, grid_x=16), lib.EUNSUPP),
    ("split tile pitch below the tile line", dict(op=lib.CMP_SPLIT, tile_pitch=63), lib.EINVAL),
    ("split tile stride below a tile", dict(op=lib.CMP_SPLIT, tile_stride=64 * 8 - 1), lib.EINVAL),
    ("split dst stride below the tiles", dict(op=lib.CMP_SPLIT, frames=2, src_frame_stride=4096, dst_frame_stride=64 * 8 * 4 - 1), lib.EINVAL),
    ("split dst == src", dict(op=lib.CMP_SPLIT, dst=_S), lib.EINVAL),
    ("logo src that is not dst", dict(op=lib.CMP_LOGO, src=_S), lib.EINVAL),
    ("logo without the overlay", dict(op=lib.CMP_LOGO, logo=None), lib.EINVAL),
    ("logo width 0", dict(op=lib.CMP_LOGO, logo_w=0), lib.EINVAL),
    ("logo height above 65536", dict(op=lib.CMP_LOGO, logo_h=65537), lib.EINVAL),
    ("logo beyond the right edge", dict(op=lib.CMP_LOGO, rect_x=58), lib.EINVAL),
    ("logo beyond the bottom edge", dict(op=lib.CMP_LOGO, rect_y=13), lib.EINVAL),
    ("logo wider than the frame at rect_x 0", dict(op=lib.CMP_LOGO, logo_w=65, rect_x=0), lib.EINVAL),
    ("logo UYVY odd rect_x", dict(op=lib.CMP_LOGO, rect_x=5), lib.EINVAL),
    ("logo RG48 odd dst", dict(op=lib.CMP_LOGO, fmt=lib.PF_RG48, dst=_D + 1), lib.EINVAL),
    ("logo RG48 odd pitch", dict(op=lib.CMP_LOGO, fmt=lib.PF_RG48, dst_pitch=64 * 6 + 1), lib.EINVAL),
    ("logo RG48 odd stride", dict(op=lib.CMP_LOGO, fmt=lib.PF_RG48, frames=2, dst_frame_stride=64 * 6 * 16 + 1), lib.EINVAL),
    ("logo dst pitch below the line", dict(op=lib.CMP_LOGO, dst_pitch=_L - 1), lib.EINVAL),
    ("logo overlay inside the frame", dict(op=lib.CMP_LOGO, logo=_D + 64), lib.EINVAL),
]


@pytest.mark.parametrize("what,kw,rc", REFUSED, ids=[r[0] for r in REFUSED])
def test_argument_rules_are_checked_without_a_device(what, kw, rc):
    l = lib.load()
    assert l.ug_hip_compose(C.byref(_desc(**kw)), None) == rc, (what, lib.last_error())
    assert lib.last_error()


def test_null_descriptor():
    assert lib.load().ug_hip_compose(None, None) == lib.EINVAL


def test_logo_with_a_negative_rectangle_is_success_and_nothing_else():
    """logo.c:195-196: the frame as it is -- no device call (this machine would answer UG_HIP_ERUNTIME to one), after the other rules"""
    l = lib.load()
    for kw in (dict(rect_x=-1), dict(rect_y=-3), dict(rect_x=-4, rect_y=-1), dict(rect_x=-1, logo_w=70)):
        assert l.ug_hip_compose(C.byref(_desc(op=lib.CMP_LOGO, **kw)), None) == lib.SUCCESS, kw
    assert l.ug_hip_compose(C.byref(_desc(op=lib.CMP_LOGO, rect_x=-1, logo=None)), None) == lib.EINVAL


def test_well_formed_calls_pass_the_rules_without_a_gpu():
    """the control of the refusals: the default descriptor of every op gets past validation, which on a machine without a GPU shows as
    UG_HIP_ERUNTIME.  Not run where a GPU is present (the pointers are fake)."""
    l = lib.load()
    n = C.c_int(0)
    if l.ug_hip_device_count(C.byref(n)) == lib.SUCCESS and n.value > 0:
        pytest.skip("a GPU is present: fake device pointers must not be launched on")
    for op in range(6):
        assert l.ug_hip_compose(C.byref(_desc(op=op)), None) == lib.ERUNTIME, (op, lib.last_error())


def test_symbols_are_exported_and_mapped():
    names = ["ug_hip_compose", "ug_hip_compose_supported", "ug_hip_crop_geometry", "ug_hip_logo_geometry", "ug_hip_border_pattern"]
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "ultragrid_amd", "libug_mi355x.so")], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1].split("@")[0] for line in out.splitlines() if line.strip()}
    committed = open(os.path.join(ROOT, "ultragrid_amd", "csrc", "libug_mi355x.map")).read()
    for n in names:
        assert n in exported and f"        {n};\n" in committed and n in lib.SYMBOLS


# ----------------------------------------------- the harness with the reference's own modules (CPU) -----------------------------------------------
_HAVE_HARNESS = pytest.mark.skipif(not os.path.exists(gen.HARNESS), reason="oracle/_ref/ug_compose_harness not built (no reference tree)")


@_HAVE_HARNESS
def test_harness_registry_lists_the_reference_modules():
    r = subprocess.run([gen.HARNESS, "list"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    pp, _, cf = r.stdout.partition("capture filters:")
    assert {"crop", "border", "interlace", "interlaced_3d", "split"} <= set(pp.split()) and {"crop", "interlace", "logo"} <= set(cf.split())


@_HAVE_HARNESS
@pytest.mark.parametrize("k", [k for k, m in enumerate(META) if m["kind"] == "inside"][::7], ids=lambda k: IDS[k])
def test_reference_run_here_equals_the_fixture(k, tmp_path):
    """a sample of the inside cases through the reference's compiled modules on this machine: the bytes the fixture recorded, an untouched pad"""
    m = META[k]
    ins, overlay = fixture_inputs(k)
    pam = gen.make_pam(overlay[0], m["logo"][0], m["logo"][1], m["logo"][3]) if m["logo"] else None
    res, rc, log = gen.run_harness(gen.HARNESS, m["name"], gen.options_of(m, str(tmp_path), pam), m["codec"], m["mode"], m["tiles"],
                                   [(w, h, d) for (w, h), d in zip(m["frames"], ins)], str(tmp_path))
    assert rc == 0 and len(res[m["name"]]) == len(m["frames"]), log
    for i, (r, fm) in enumerate(zip(res[m["name"]], m["frames_meta"])):
        assert r["ret"] == fm["ref_ret"] and r["pad"] in (0, -1)
        assert [r["w"], r["h"], r["codec"], r["interlacing"], r["fps"], r["tile_count"], r["data_len"]] == fm["ref_desc"]
        if "out" in r and f"out_{k}_{i}" in GOLD.files:
            got, want = r["out"], GOLD[f"out_{k}_{i}"]
            if m["name"] == "crop":
                got = got.reshape(fm["h"], -1)[:, : want.size // fm["h"]].reshape(-1)
            assert got.size == want.size and int(np.count_nonzero(got != want)) == 0
