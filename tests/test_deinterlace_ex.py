"""CPU: the pin of the de-interlacers (vc_deinterlace_ex, double_framerate, deinterlace_bob, deinterlace_linear) and of ug_hip_deinterlace's
place in the C ABI.

The chain: the reference's deinterlace.c / temporal-deint.c compiled unmodified and run through its vo_postprocess.c
(tests/golden/make_temporal_deint_golden.py) -> tests/golden/temporal_deint_ref.npz -> tests/deinterlace_restatement.py, byte for byte;
vc_deinterlace_ex of oracle/_ref/libugref.so -> the same restatement; the restatement -> the GPU kernel and modules
(tests/test_gpu_deinterlace_ex.py, tests/test_gpu_deinterlace_module.py).  What a comparison leaves out is a condition."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import deinterlace_restatement as rs  # noqa: E402
import make_temporal_deint_golden as gen  # noqa: E402
from ultragrid_amd import lib  # noqa: E402

GOLD_PATH = os.path.join(HERE, "golden", "temporal_deint_ref.npz")
GOLD = np.load(GOLD_PATH)
CASES = json.loads(str(GOLD["cases"]))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libugref.so")
_P = 0x7F0000001000  # non-NULL, 16-byte aligned, never dereferenced
BASE = {"deinterlace": "deinterlace", "deinterlace_blend": "deinterlace"}


def case_outputs(m):
    """per frame i: ([H, L] input, [out0, out1 or None] as [H, pitch]) of a fixture case"""
    ins, outs, a, b = [], [], 0, 0
    for i, (w, h) in enumerate(m["sizes"]):
        L = gen.linesize(m["codec"], w)
        ins.append(GOLD["in_" + m["id"]][a: a + L * h].reshape(h, L))
        a += L * h
        fr = []
        for k in range(2):
            if m["rets"][i][k] == "1":
                n = (L + m["extra"]) * h
                fr.append(GOLD["out_" + m["id"]][b: b + n].reshape(h, L + m["extra"]))
                b += n
            else:
                fr.append(None)
        outs.append(fr)
    assert a == GOLD["in_" + m["id"]].size and b == GOLD["out_" + m["id"]].size
    return ins, outs


def restated(m, ins):
    cls = rs.FORMATS[m["codec"]][1] if m["codec"] in rs.FORMATS else None
    active = m["inter"] == "merged" or m["opts"] == "force"
    L = ins[0].shape[1]
    out, start = [], 0
    for i in range(1, len(ins) + 1):  # a new size = a reconfigure: the frame before is zero again
        if i == len(ins) or ins[i].shape != ins[start].shape:
            out += rs.module_run(m["name"], m["opts"], cls, active, ins[start].shape[1], ins[start].shape[1] + m["extra"], ins[start:i])
            start = i
    return out, L


def test_fixture_is_small_and_covers_the_cases():
    assert os.path.getsize(GOLD_PATH) < 512 * 1024
    names = {m["name"] for m in CASES}
    assert names == {"deinterlace", "deinterlace_blend", "double_framerate", "deinterlace_bob", "deinterlace_linear"}
    for name in names:
        mine = [m for m in CASES if m["name"] == name]
        assert {m["codec"] for m in mine} >= set(rs.FORMATS) if name != "deinterlace" and name != "deinterlace_blend" else True
        assert any(m["opts"] == "force" and m["inter"] == "prog" for m in mine) and any(m["opts"] == "-" and m["inter"] == "prog" for m in mine)
        assert any(len(set(map(tuple, m["sizes"]))) > 1 for m in mine), "a reconfigure to another size"
        assert any(m["codec"] == "DVS10" for m in mine), "a codec the averages do not take"
    assert {m["codec"] for m in CASES if m["name"] in BASE} >= set(rs.FORMATS)
    assert any(m["opts"] == "d" for m in CASES) and any(m["opts"] == "nodelay" for m in CASES) and any(m["extra"] for m in CASES)
    assert all(len(m["sizes"]) == 3 for m in CASES)


def test_restatement_equals_the_executed_modules():
    """every byte of every output of every case, except -- conditions, not measurements -- the lines of the first double_framerate output after a
    reconfigure that come from the reference's uninitialised buffer (odd lines; with `:d` the blend spreads them over all lines) and the pitch
    gaps (the reference's avg_lines_per_elem writes up to 15 bytes into them).  The share left out stays below 5 %, and is 0 for vc_deinterlace_ex."""
    total = left = gaps = blend_left = 0
    for m in CASES:
        ins, outs = case_outputs(m)
        want, _ = restated(m, ins)
        active = m["inter"] == "merged" or m["opts"] == "force"
        for i, (fr, wfr) in enumerate(zip(outs, want)):
            L = ins[i].shape[1]
            for k in range(2):
                assert (fr[k] is None) == (wfr[k] is None), (m["id"], i, k)
                if fr[k] is None:
                    continue
                keep = np.ones(fr[k].shape[0], bool)
                ex = gen.excluded(m["name"], m["opts"], active, [tuple(s) for s in m["sizes"]], i, k)
                if ex is not None:
                    keep[ex] = False
                    assert m["name"] == "double_framerate"
                bad = np.count_nonzero(fr[k][keep, :L] != wfr[k][keep, :L])
                assert bad == 0, (m["id"], i, k, bad)
                total += fr[k].size
                left += np.count_nonzero(~keep) * L
                gaps += fr[k].shape[0] * m["extra"]
                if m["name"] in BASE:
                    blend_left += np.count_nonzero(~keep) * L + fr[k].shape[0] * m["extra"]
    print(f"compared {total - left - gaps} of {total} bytes; left out {left} (first-output lines) + {gaps} (pitch gaps) = {100 * (left + gaps) / total:.2f} %")
    assert blend_left == 0
    assert left + gaps < 0.05 * total


def test_frame_flow_of_the_modules():
    """postprocess(in) true; postprocess(NULL): the three temporal ones true once, then false -- deinterlace false at once; get_out_desc: the
    input's size and codec; the temporal ones PROGRESSIVE, fps * 2, DISPLAY_PROPERTY_VIDEO_MERGED (0); deinterlace: its frame's description"""
    for m in CASES:
        for (w, h), ret, d in zip(m["sizes"], m["rets"], m["descs"]):
            assert ret == ("100" if m["name"] in BASE else "110"), m["id"]
            assert (int(d[0]), int(d[1]), d[2]) == (w, h, m["codec"]), m["id"]
            if m["name"] in BASE:
                assert (int(d[3]), float(d[4]), int(d[6])) == (3 if m["inter"] == "merged" else 0, 25.0, -1), m["id"]
            else:
                assert (int(d[3]), float(d[4]), int(d[5]), int(d[6])) == (0, 50.0, 1, 0), m["id"]


def _ref():
    if not os.path.exists(REF_SO):
        pytest.skip("oracle/_ref/libugref.so not built (no reference tree)")
    ref = C.CDLL(REF_SO)
    ref.get_codec_from_name.argtypes, ref.get_codec_from_name.restype = [C.c_char_p], C.c_int
    ref.vc_deinterlace_ex.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t]
    ref.vc_deinterlace_ex.restype = C.c_bool
    return ref


LINE_SIZES = [4, 12, 16, 20, 36, 40, 48, 72, 100, 108, 144, 180, 396, 400, 3840]


@pytest.mark.parametrize("name", sorted(rs.FORMATS))
def test_restatement_equals_compiled_vc_deinterlace_ex(name):
    """formats x line sizes (no multiples of 16 / 36 among them) x heights, dst pitch > line size, dst == src: the whole pre-filled destination"""
    ref = _ref()
    _, cls, ref_name = rs.FORMATS[name]
    codec = ref.get_codec_from_name(ref_name.encode())
    assert codec > 0
    rng = np.random.default_rng(len(name))
    n = 0
    for L in LINE_SIZES:
        if L % rs.UNIT[cls]:
            continue
        for H in (1, 2, 3, 5, 8, 13):
            for dp in (L, L + 16):
                src, bg = rng.integers(0, 256, (H, L), dtype=np.uint8), rng.integers(0, 256, (H, dp), dtype=np.uint8)
                dst = bg.copy()
                assert ref.vc_deinterlace_ex(codec, src.ctypes.data, L, dst.ctypes.data, dp, H)
                assert np.array_equal(dst, rs.blend(cls, src, L, bg)), (name, L, H, dp)
                n += 1
            d = src.copy()
            assert ref.vc_deinterlace_ex(codec, d.ctypes.data, L, d.ctypes.data, L, H)
            assert np.array_equal(d, rs.blend(cls, src, L, src)), (name, L, H, "in place")
    assert n >= 100


def test_fixture_regenerates():
    if not os.path.isdir("/root/reference/src") or not os.path.exists(gen.HARNESS):
        pytest.skip("needs the reference tree and oracle/_ref/ug_deint_harness")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "again.npz")
        subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_temporal_deint_golden.py"), out], check=True, capture_output=True)
        again = np.load(out)
        assert sorted(again.files) == sorted(GOLD.files)
        for m in json.loads(str(again["cases"])):
            assert np.array_equal(again["in_" + m["id"]], GOLD["in_" + m["id"]]), m["id"]
            ins, outs = case_outputs(m)
            a = again["out_" + m["id"]]
            active = m["inter"] == "merged" or m["opts"] == "force"
            b = 0
            for i, fr in enumerate(outs):
                for k in range(2):
                    if fr[k] is None:
                        continue
                    mine = a[b: b + fr[k].size].reshape(fr[k].shape)
                    b += fr[k].size
                    keep = np.ones(fr[k].shape[0], bool)
                    ex = gen.excluded(m["name"], m["opts"], active, [tuple(s) for s in m["sizes"]], i, k)
                    if ex is not None:
                        keep[ex] = False  # (uninitialised memory: not the same from run to run)
                    assert np.array_equal(mine[keep], fr[k][keep]), (m["id"], i, k)


def test_header_binding_and_export_map_agree():
    hdr = open(os.path.join(ROOT, "include", "ug_mi355x.h")).read()
    exp = open(os.path.join(ROOT, "ultragrid_amd", "csrc", "libug_mi355x.map")).read()
    for name in ("ug_hip_deinterlace", "ug_hip_deinterlace_supported"):
        assert re.search(r"\bint " + name + r"\(", hdr) and re.search(r"\b" + name + r";", exp) and name in lib.SYMBOLS
        assert hasattr(lib.load(), name)
    assert "#define UG_HIP_ABI_VERSION 5 " in hdr
    fields = re.search(r"struct ug_deinterlace_desc \{(.*?)\};", hdr, re.S).group(1)
    declared = [n for line in fields.splitlines() for n in re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", line.split("/*")[0])]
    assert declared == [f[0] for f in lib.DeinterlaceDesc._fields_], declared
    for k, v in (("BLEND", 0), ("WEAVE", 1), ("BOB", 2), ("LINEAR", 3)):
        assert re.search(rf"#define UG_DEINT_{k}\s+{v}\b", hdr) and getattr(lib, "DEINT_" + k) == v == rs.MODES[k]


def desc(fmt=lib.PF_UYVY, mode=rs.BLEND, lines=8, linesize=64, sp=0, dp=0, frames=1, ss=0, ds=0, src=_P, prev=_P + 0x100000, d0=_P + 0x200000, d1=_P + 0x300000, blend=0):
    return lib.DeinterlaceDesc(src, prev, (C.c_void_p * 2)(d0, d1), fmt, mode, blend, lines, linesize, sp, dp, frames, ss, ds)


def test_absurd_geometry_is_refused():
    """every refusal before a device call (there is no device here: a call that reached one would come back as a runtime error)"""
    f = lib.load().ug_hip_deinterlace
    huge = 2 ** 31
    bad = [
        dict(lines=0), dict(lines=-1), dict(lines=65537), dict(lines=-2 ** 31), dict(linesize=0), dict(linesize=8 * 65536 + 1), dict(linesize=2 ** 63),
        dict(lines=65536, linesize=65536), dict(lines=65536, sp=huge), dict(lines=65536, dp=huge), dict(sp=63), dict(dp=63), dict(sp=2 ** 62), dict(dp=2 ** 63 + 64),
        dict(frames=0), dict(frames=-1), dict(frames=65536), dict(frames=2, ss=8 * 64 - 1, ds=8 * 64), dict(frames=2, ss=8 * 64, ds=8 * 64 - 1),
        dict(frames=3, ss=2 ** 63, ds=8 * 64), dict(frames=3, ss=8 * 64, ds=2 ** 63), dict(mode=-1), dict(mode=4), dict(src=None), dict(d0=None),
        dict(mode=rs.WEAVE, prev=None), dict(mode=rs.BOB, d1=None), dict(mode=rs.WEAVE, lines=7), dict(mode=rs.BOB, lines=1), dict(mode=rs.LINEAR, lines=1),
        dict(fmt=lib.PF_RG48, linesize=63), dict(fmt=lib.PF_RG48, src=_P + 1), dict(fmt=lib.PF_V210, linesize=66), dict(fmt=lib.PF_R12L, dp=70, linesize=36),
        dict(fmt=lib.PF_R10K, d0=_P + 0x200002), dict(fmt=lib.PF_RG48, frames=2, ss=8 * 64 + 1, ds=8 * 64),
        dict(d0=_P + 64), dict(d0=_P, dp=128), dict(mode=rs.BOB, d1=_P + 0x200000 + 64), dict(mode=rs.WEAVE, prev=_P + 0x200000), dict(mode=rs.LINEAR, d0=_P),
    ]
    for kw in bad:
        d = desc(**kw)
        rc = f(C.byref(d), None)
        assert rc == lib.EINVAL, (kw, rc, lib.last_error())
    for fmt in (lib.PF_I420, lib.PF_YUV444, lib.PF_UYVY_RAW, lib.PF_DVS10, lib.PF_NONE, 99):
        d = desc(fmt=fmt)
        assert f(C.byref(d), None) == lib.EUNSUPP, fmt
        assert lib.load().ug_hip_deinterlace_supported(fmt, rs.BLEND) == 0
    assert f(None, None) == lib.EINVAL
    for name, (pf, _cls, _r) in rs.FORMATS.items():
        for mode in range(4):
            assert lib.load().ug_hip_deinterlace_supported(pf, mode) == 1, name
        assert lib.load().ug_hip_deinterlace_supported(pf, 4) == 0 and lib.load().ug_hip_deinterlace_supported(pf, -1) == 0


# ---- the reference's slips, one test each ----

def test_slip_blend_leaves_line_ends_unwritten():
    """vc_deinterlace_ex: R12L walks linesize / 36 groups of EIGHT words (a group has nine) -- the last ninth of a line is never written; v210 and
    R10k leave linesize % 16 bytes; the 16-bit formats too from 16 bytes on (x86-64 build).  Reproduced: the destination keeps its bytes there"""
    assert rs.written_bytes("r12l", False, 36) == 28 and rs.written_bytes("r12l", False, 72) == 60 and rs.written_bytes("r12l", False, 108) == 96
    assert rs.written_bytes("r12l", False, 8640) == 8640 // 36 * 32  # 1920 pixels: 240 groups of 8 words, a multiple of 3 words
    assert rs.written_bytes("v210", False, 100) == 96 and rs.written_bytes("r10k", False, 36) == 32
    assert rs.written_bytes("u16", False, 36) == 32 and rs.written_bytes("u16", False, 12) == 12 and rs.written_bytes("u8", False, 37) == 37
    m = next(m for m in CASES if m["id"] == "blend_R12L")
    ins, outs = case_outputs(m)
    L, H = ins[0].shape[1], ins[0].shape[0]
    W = rs.written_bytes("r12l", False, L)
    assert W < L
    for fr in outs:
        assert np.all(fr[0][: H - 1, W:L] == 0xA5), "the reference wrote where its loop does not reach"
        assert np.array_equal(fr[0][H - 1, :L], fr[0][H - 2, :L])


def test_slip_linear_r10k_walks_four_lines():
    """avg_lines, R10k: linesize / 4 groups of 4 words = four lines' worth per call, past the frame at the bottom (the harness allocates six lines
    more).  What stays of it inside a frame of pitch == linesize: every line is rewritten by a later step, so the frame equals the one-line average
    of the stand-in in EVERY line -- no line of this case is left out.  (With a pitch gap the overrun would land in it: the case has none.)
    The averaged words are read with ntohl and stored in host order: those lines are byte-swapped, which the stand-in reproduces"""
    m = next(m for m in CASES if m["id"] == "linear_R10k")
    assert m["extra"] == 0
    ins, outs = case_outputs(m)
    want, _ = restated(m, ins)
    for fr, w in zip(outs, want):
        assert np.array_equal(fr[0], w[0]) and np.array_equal(fr[1], w[1])
    a = np.array([[0x12, 0x34, 0x56, 0x78] * 4], np.uint8)  # (a line of 16 bytes: vc_deinterlace_ex writes whole groups of 4 words)
    assert rs.avg_line("r10k", True, a, a).tolist() == [[0x78, 0x56, 0x34, 0x12] * 4] and rs.avg_line("r10k", False, a, a).tolist() == a.tolist()


def test_slip_avg_lines_per_elem_rounds_the_line_up():
    """avg_lines_per_elem walks the line size rounded up to 16 bytes: behind a 120-byte line it writes 8 bytes more -- into the pitch gap of the
    fixture's case.  The stand-in writes linesize bytes (the restatement leaves 0xA5 there); and its average is (c1 >> 1) + (c2 >> 1) + (c1 & 1)"""
    m = next(m for m in CASES if m["id"] == "nodelay_deinterlace_linear")
    ins, outs = case_outputs(m)
    L, H = ins[0].shape[1], ins[0].shape[0]
    assert L == 120 and m["extra"] == 16
    want, _ = restated(m, ins)
    for fr, w in zip(outs, want):
        averaged = [y for y in range(H) if y % 2 == 1 and y < 2 * ((H - 1) // 2)]
        assert averaged and all(np.any(fr[0][y, L: L + 8] != 0xA5) for y in averaged), "the reference stayed inside the line"
        assert np.all(fr[0][:, L + 8:] == 0xA5) and np.all(w[0][:, L:] == 0xA5)
    a, b = np.array([[1, 255, 0, 3]], np.uint8), np.array([[0, 255, 1, 2]], np.uint8)
    assert rs.avg_line("u8", True, a, b).tolist() == [[1, 255, 0, 3]] and rs.avg_line("u8", False, a, b).tolist() == [[1, 255, 1, 3]]


def test_slip_weave_with_an_odd_height_is_refused():
    """perform_df with an odd height copies one line past both buffers and leaves the last line unwritten: refused"""
    d = desc(mode=rs.WEAVE, lines=9)
    assert lib.load().ug_hip_deinterlace(C.byref(d), None) == lib.EINVAL and "even" in lib.last_error()


def test_slip_first_output_weaves_with_a_zeroed_frame():
    """the first output after a reconfigure: the reference weaves with a buffer it never initialised; the stand-in's frame before the first is
    zero.  The even lines are this frame's in both"""
    m = next(m for m in CASES if m["id"] == "df_UYVY")
    ins, outs = case_outputs(m)
    want, L = restated(m, ins)
    assert np.array_equal(outs[0][0][0::2, :L], ins[0][0::2]) and np.array_equal(want[0][0][0::2, :L], ins[0][0::2])
    assert np.all(want[0][0][1::2, :L] == 0)
    assert np.array_equal(outs[1][0][1::2, :L], ins[0][1::2]), "from the second frame on the odd lines are the previous frame's"


def test_slip_one_line_and_no_line():
    """vc_deinterlace_ex with one line copies; with none `lines - 1` underflows: UG_HIP_EINVAL"""
    src, bg = np.arange(40, dtype=np.uint8).reshape(1, 40), np.full((1, 48), 7, np.uint8)
    out = rs.blend("u8", src, 40, bg)
    assert np.array_equal(out[0, :40], src[0]) and np.all(out[0, 40:] == 7)
    d = desc(lines=0)
    assert lib.load().ug_hip_deinterlace(C.byref(d), None) == lib.EINVAL
