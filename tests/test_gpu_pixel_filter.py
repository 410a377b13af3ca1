"""GPU: ug_hip_pixel_filter against the numpy restatement (tests/pixel_filter_restatement.py), 0 bytes differing: every case of the reference
fixture (also against the reference's own bytes, under the fixture's two conditions), pictures wider than a workgroup's 64 units and higher than
its 4 lines, frames = 1 and 3 with strides, pitched and deliberately misaligned buffers (tests/pitch_layout.py: every byte outside the lines keeps
its fill), and the dwordx4 path against the word / byte path on the same data."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_pixel_filter_golden as gen  # noqa: E402
import pitch_layout as pl  # noqa: E402
import pixel_filter_restatement as rs  # noqa: E402

from ultragrid_amd import codec, lib  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(HERE, "golden", "pixel_filter_ref.npz"))
META = json.loads(str(GOLD["meta"]))
CPUS = int(GOLD["cpus"])
OPS = {"matrix": lib.PXF_MATRIX, "matrix2": lib.PXF_MATRIX2, "gamma": lib.PXF_LUT, "grayscale": lib.PXF_GRAY, "mirror": lib.PXF_MIRROR, "flip": lib.PXF_FLIP}
PF = dict(lib.PF_NAMES)
ELEM = {"RG48": 2, "Y416": 2, "v210": 4, "R10k": 4}


def device_run(name, options, codec_name, w, h, data):
    """the case through codec.pixel_filter, as the module would call it -> bytes"""
    src = torch.from_numpy(np.ascontiguousarray(data)).cuda()
    kw = {}
    if name in ("matrix", "matrix2"):
        m, check = rs.parse_matrix(options, name == "matrix2")
        kw = dict(matrix=m, clamp=check)
    elif name == "gamma":
        g, _, depth = options.partition(":")
        kw = dict(gamma=float(g), out_fmt={"": lib.PF_NONE, "8": lib.PF_RGB, "16": lib.PF_RG48}[depth])
    out = codec.pixel_filter(OPS[name], PF[codec_name], src, w, h, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


RUNNABLE = [k for k, m in enumerate(META) if m["status"] == "new" and f"out_{k}" in GOLD.files and lib.load().ug_hip_pixel_filter_supported(OPS[m["name"]], PF[m["codec"]])]


def test_the_fixture_cases_run_here():
    """every case the reference transforms runs on the device too"""
    assert len(RUNNABLE) == sum(1 for k, m in enumerate(META) if f"out_{k}" in GOLD.files) == len(META) - 5


@pytest.mark.parametrize("k", RUNNABLE, ids=[f"{k}-{META[k]['name']}-{META[k]['codec']}-{META[k]['w']}x{META[k]['h']}" for k in RUNNABLE])
def test_fixture_case(k):
    m = META[k]
    opts = "" if m["options"] == "-" else m["options"]
    data = GOLD[m["input"]]
    want = rs.run_filter(m["name"], opts, m["codec"], m["w"], m["h"], data)
    got = device_run(m["name"], opts, m["codec"], m["w"], m["h"], data)
    assert got.size == want["out"].size
    assert int(np.count_nonzero(got != want["out"])) == 0  # nothing left out
    ref = GOLD[f"out_{k}"]
    left = gen.left_out(want, ref, CPUS, m["name"], m["codec"])
    assert left.mean() < 0.05
    assert int(np.count_nonzero((got != ref) & ~left)) == 0


# (label, module name, options, codec, width, lines): wider than 64 units of a lane, more than one workgroup of lines, a partial last unit
M = "1.31:-0.62:0.18:-1.94:0.77:1.05:0.4:1.66:-1.23"
KINDS = [
    ("matrix-uyvy", "matrix", M, "UYVY", 1098, 9),
    ("matrix-uyvy-unchecked", "matrix", M + ":no-bound-check", "UYVY", 1098, 5),
    ("matrix-rgb", "matrix", M, "RGB", 1101, 9),
    ("matrix-rgb-unchecked", "matrix", M + ":no-bound-check", "RGB", 1101, 5),
    ("matrix-rg48", "matrix", M, "RG48", 555, 9),
    ("matrix-rg48-unchecked", "matrix", M + ":no-bound-check", "RG48", 555, 5),
    ("matrix2-uyvy", "matrix2", gen.MATRIX2_M, "UYVY", 1098, 9),
    ("matrix2-y416", "matrix2", "y601_to_y709", "Y416", 301, 9),
    ("matrix2-v210", "matrix2", "y601_to_y709", "v210", 500, 9),
    ("gamma-8-8", "gamma", "2.2", "RGB", 1101, 9),
    ("gamma-8-16", "gamma", "0.45:16", "RGB", 1101, 9),
    ("gamma-16-16", "gamma", "2.2", "RG48", 555, 9),
    ("gamma-16-8", "gamma", "0.45:8", "RG48", 555, 9),
    ("grayscale", "grayscale", "", "UYVY", 1098, 9),
    ("mirror", "mirror", "", "UYVY", 1098, 9),
    ("mirror-whole-units", "mirror", "", "UYVY", 1088, 5),
    ("flip-rgb", "flip", "", "RGB", 1101, 9),
    ("flip-v210", "flip", "", "v210", 500, 6),
]
KIDS = [k[0] for k in KINDS]


def _frames(kind, frames, seed):
    """random input frames and their restated outputs (random bytes: the unchecked forms wrap around, which the restatement states too)"""
    _, name, opts, cn, w, h = kind
    rng = np.random.default_rng(seed)
    n = rs.linesize(cn, w) * h
    ins = [np.frombuffer(rng.bytes(n), np.uint8).copy() for _ in range(frames)]
    outs = [rs.run_filter(name, opts, cn, w, h, f) for f in ins]
    return ins, [o["out"] for o in outs], outs[0]["codec"]


def _call(kind, out_codec, src_t, src_off, sp, sstride, dst_t, dst_off, dp, dstride, frames, expect=lib.SUCCESS):
    _, name, opts, cn, w, h = kind
    m, check, lut = [0.0] * 9, True, None
    if name in ("matrix", "matrix2"):
        m, check = rs.parse_matrix(opts, name == "matrix2")
    if name == "gamma":
        g = float(opts.partition(":")[0])
        lut = codec.gamma_lut(g, 16 if cn == "RG48" else 8, 16 if out_codec == "RG48" else 8).cuda()
    d = lib.PixelFilterDesc(src_t.data_ptr() + src_off, dst_t.data_ptr() + dst_off, OPS[name], PF[cn], PF[out_codec], w, h, sp, dp, frames, sstride, dstride,
                            (C.c_double * 9)(*m), int(check), lut.data_ptr() if lut is not None else None)
    rc = lib.load().ug_hip_pixel_filter(C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == expect, lib.last_error()


def _run_layout(kind, frames, sp, dp, src_off, dst_off, sgap, dgap, seed=7):
    """`frames` pictures at these pitches, offsets (from 256-byte aligned device addresses) and gaps between the frames -> findings (empty = good)"""
    _, name, opts, cn, w, h = kind
    ins, outs, oc = _frames(kind, frames, seed)
    sl, dl = rs.linesize(cn, w), rs.linesize(oc, w)
    sp, dp = sp or sl, dp or dl
    sstride, dstride = sp * h + sgap, dp * h + dgap
    rng = np.random.default_rng(seed + 1)
    src = pl.aligned_bytes(src_off + sstride * frames + pl.SLACK, rng=rng)
    for f in range(frames):
        for y in range(h):
            at = src_off + f * sstride + y * sp
            src[at: at + sl] = ins[f][y * sl: (y + 1) * sl]
    front = pl.GUARD + dst_off
    total = front + dstride * (frames - 1) + dp * h + pl.GUARD
    want = pl.aligned_bytes(total, fill=pl.FILL)
    for f in range(frames):
        for y in range(h):
            at = front + f * dstride + y * dp
            want[at: at + dl] = outs[f][y * dl: (y + 1) * dl]
    src_t = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    dst_t = torch.full((total,), pl.FILL, dtype=torch.uint8, device="cuda")
    assert src_t.data_ptr() % 256 == 0 and dst_t.data_ptr() % 256 == 0
    _call(kind, oc, src_t, src_off, sp, sstride, dst_t, front, dp, dstride, frames)
    return pl.compare_frames(dst_t.cpu().numpy(), want, frames, dstride, h, dp, dl, front=front)


@pytest.mark.parametrize("kind", KINDS, ids=KIDS)
def test_packed_one_and_three_frames_with_strides(kind):
    assert _run_layout(kind, 1, 0, 0, 0, 0, 0, 0) == []
    e_in, e_out = ELEM.get(kind[3], 1), 4
    assert _run_layout(kind, 3, 0, 0, 0, 0, 16 * 5, 16 * 3) == []        # strides that keep every frame 16-byte aligned where the frame is
    assert _run_layout(kind, 3, 0, 0, 0, 0, e_in * 3, e_out * 3) == []    # ... and strides that do not


@pytest.mark.parametrize("layout", ["padded16", "odd_pitch", "src_off", "dst_off"])
@pytest.mark.parametrize("kind", KINDS, ids=KIDS)
def test_pitched_and_misaligned_buffers(kind, layout):
    _, name, opts, cn, w, h = kind
    oc = rs.run_filter(name, opts, cn, 2 if cn != "v210" else 48, 1, np.zeros(rs.linesize(cn, 2 if cn != "v210" else 48), np.uint8))["codec"]
    ei, eo = (1, 1) if name == "flip" else (ELEM.get(cn, 1), ELEM.get(oc, 1))
    sl, dl = rs.linesize(cn, w), rs.linesize(oc, w)
    if layout == "odd_pitch":  # lines start at every residue the element allows: no dwordx4 tier
        sp, dp = sl + ei, dl + eo
        sp += ei if sp % 16 == 0 else 0
        dp += eo if dp % 16 == 0 else 0
        so = do = 0
    else:
        sp, dp = (sl + 15) // 16 * 16 + 16, (dl + 15) // 16 * 16 + 32
        so, do = (ei if layout == "src_off" else 0), (eo if layout == "dst_off" else 0)
    assert _run_layout(kind, 2, sp, dp, so, do, 16 * 2, 16 * 4) == []


@pytest.mark.parametrize("kind", KINDS, ids=KIDS)
def test_aligned_and_unaligned_paths_agree(kind):
    """the same frame once where every unit is 16-byte aligned (pitches rounded up to 16) and once an element off on both sides"""
    _, name, opts, cn, w, h = kind
    ins, outs, oc = _frames(kind, 1, 11)
    sl, dl = rs.linesize(cn, w), rs.linesize(oc, w)
    sp, dp = (sl + 15) // 16 * 16, (dl + 15) // 16 * 16
    ei, eo = (1, 1) if name == "flip" else (ELEM.get(cn, 1), ELEM.get(oc, 1))
    got = []
    for so, do in ((0, 0), (ei, eo)):
        src = np.zeros(so + sp * h + 16, np.uint8)
        for y in range(h):
            src[so + y * sp: so + y * sp + sl] = ins[0][y * sl: (y + 1) * sl]
        src_t = torch.from_numpy(src).cuda()
        dst_t = torch.full((do + dp * h + 16,), pl.FILL, dtype=torch.uint8, device="cuda")
        _call(kind, oc, src_t, so, sp, 0, dst_t, do, dp, 0, 1)
        d = dst_t.cpu().numpy()[do: do + dp * h].reshape(h, dp)
        assert (d[:, dl:] == pl.FILL).all()
        got.append(d[:, :dl].reshape(-1).copy())
    assert np.array_equal(got[0], got[1])
    assert np.array_equal(got[0], outs[0])


def test_codec_wrapper_uploads_the_table_and_names_the_output():
    rng = np.random.default_rng(3)
    data = np.frombuffer(rng.bytes(3 * 37 * 4), np.uint8).copy()
    out = codec.pixel_filter(lib.PXF_LUT, lib.PF_RGB, torch.from_numpy(data).cuda(), 37, 4, gamma=2.2, out_fmt=lib.PF_RG48)
    assert out.is_cuda and out.numel() == 2 * data.size
    assert np.array_equal(out.cpu().numpy(), rs.lut(data, 8, rs.gamma_lut(2.2, 8, 16)))
    out = codec.pixel_filter(lib.PXF_MATRIX2, lib.PF_UYVY, torch.from_numpy(data[: 4 * 18 * 4]).cuda(), 36, 4, matrix=codec.matrix2_preset("y601_to_y709"))
    assert np.array_equal(out.cpu().numpy(), rs.matrix2("UYVY", data[: 4 * 18 * 4], rs.Y601_TO_Y709)[0])
