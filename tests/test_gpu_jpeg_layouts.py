"""GPU: JPEG sampling layouts beyond 4:4:4 / 4:2:2 / 4:2:0 -- 4:4:0, 4:1:1, 4:1:0 and subsampled R,G,B streams.  The decoder's planes against the
decode oracle (libjpeg's integer IDCT) bit for bit, its packed outputs against the numpy restatement of the replication rule
(tests/jpeg_layout_restatement.py), the receiving modules, a 4:2:2 stream against its transpose, and the kernels the old layouts keep."""
import ctypes as C
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from jpeg_bitstream import ZIGZAG
from jpeg_layout_bitstream import LAYOUTS, geometry, layout_coefs, layout_stream, picture, write_layout_jpeg
from jpeg_layout_restatement import expected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEC_HARNESS = os.path.join(ROOT, "oracle", "_ref", "ug_dec_harness")
needs_dec_harness = pytest.mark.skipif(not os.path.exists(DEC_HARNESS), reason="oracle/_ref/ug_dec_harness not built")

SIZES = [(1, 1), (17, 9), (150, 70), (1920, 1080)]


def _ratios(data, po):
    info = po.jpeg_decode_planes(data)[0]
    hmax, vmax = max(info["h"]), max(info["v"])
    return [(hmax // hs, vmax // vs) for hs, vs in zip(info["h"], info["v"])]


def _decode_to(dec, data, fmt, w, h, pitch, shifts=(0, 8, 16)):
    """ug_hip_jpeg_decoder_decode_sized into a destination of `pitch` bytes per line with guard bytes around every line: returns (h, line bytes)"""
    import torch
    from ultragrid_amd import codec, lib as L
    ls = codec.linesize(fmt, w)
    dst = torch.full((pitch * h + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    L.check(L.load().ug_hip_jpeg_decoder_decode_sized(dec._h, data, len(data), w, h, fmt, C.c_void_p(dst.data_ptr()), pitch, *shifts,
                                                      codec._stream()), "ug_hip_jpeg_decoder_decode_sized")
    torch.cuda.synchronize()
    buf = dst.cpu().numpy()
    rows = buf[: pitch * h].reshape(h, pitch)
    assert (rows[:, ls:] == 0xA5).all() and (buf[pitch * h:] == 0xA5).all(), "bytes outside the picture written"
    return rows[:, :ls]


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("ri", [0, 1, 5])
@pytest.mark.parametrize("nonint", [False, True], ids=["interleaved", "nonint"])
@pytest.mark.parametrize("code", list(LAYOUTS))
def test_gpu_planes_equal_the_oracle(hip, po, code, nonint, ri, size):
    w, h = size
    rgb = "adobe" if (w + ri) % 2 else None  # both kinds of stream, without doubling the matrix
    data = layout_stream(po, w, h, code, restart=ri, nonint=nonint, rgb=rgb)
    _, crop, _ = po.jpeg_decode_planes(data)
    dec = hip.JpegDecoder()
    got = [p.cpu().numpy() for p in dec.planes(data)]
    dec.close()
    assert len(got) == 3
    for c in range(3):
        assert np.array_equal(got[c], crop[c]), f"component {c}"


OUT_SIZES = [(1, 1), (17, 9), (150, 70), (61, 33)]
# the layouts layout_pack_kernel serves (the others keep their kernels and their own pinned conventions, e.g. at odd widths)
NEW_LAYOUTS = [(code, None) for code in (440, 411, 410)] + [(code, "ids") for code in (422, 420, 440, 411, 410)]


@pytest.mark.gpu
@pytest.mark.parametrize("size", OUT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("code,rgb", NEW_LAYOUTS, ids=[f"{c}-{'rgb' if r else 'ycc'}" for c, r in NEW_LAYOUTS])
def test_gpu_outputs_equal_the_restatement(hip, po, code, rgb, size):
    """every packed output, at the line size and at two display pitches (one that is not a multiple of 4), against the replication rule over the
    oracle's planes; RGBA also with other shifts.  Y'CbCr -> RGB / RGBA at an odd width: the UYVY -> RGB[A] stage (vc_copylineUYVYtoRGB[A]: a
    whole pair per step) leaves the last pixel of a line unwritten, as it does for every other layout"""
    from ultragrid_amd import codec, lib as L
    w, h = size
    data = layout_stream(po, w, h, code, restart=3, rgb=rgb, seed=1)
    _, crop, _ = po.jpeg_decode_planes(data)
    ratios = _ratios(data, po)
    dec = hip.JpegDecoder()
    for out in ("RGB", "RGBA", "UYVY"):
        fmt = getattr(L, "PF_" + out)
        ls = codec.linesize(fmt, w)
        for shifts in ([(0, 8, 16), (16, 8, 0)] if out == "RGBA" else [(0, 8, 16)]):
            want = expected(po, crop, ratios, w, h, rgb is not None, out, shifts)
            n = ls - (ls // w if rgb is None and out != "UYVY" and w % 2 else 0)
            for pitch in (ls, ls + 13, ls + 64):
                got = _decode_to(dec, data, fmt, w, h, pitch, shifts)
                assert np.array_equal(got[:, :n], want[:, :n]) and (got[:, n:] == 0xA5).all(), (out, shifts, pitch)
    dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nonint", [False, True], ids=["interleaved", "nonint"])
@pytest.mark.parametrize("code", [440, 411, 410, 420])
def test_gpu_outputs_1080p(hip, po, code, nonint):
    """a full-size frame, R,G,B and Y'CbCr, UYVY and RGBA"""
    from ultragrid_amd import codec, lib as L
    w, h = 1920, 1080
    dec = hip.JpegDecoder()
    for rgb in (None, "adobe"):
        data = layout_stream(po, w, h, code, restart=5, nonint=nonint, rgb=rgb, seed=2)
        _, crop, _ = po.jpeg_decode_planes(data)
        ratios = _ratios(data, po)
        for out in ("UYVY", "RGBA"):
            fmt = getattr(L, "PF_" + out)
            got = _decode_to(dec, data, fmt, w, h, codec.linesize(fmt, w))
            assert np.array_equal(got, expected(po, crop, ratios, w, h, rgb is not None, out)), (rgb, out)
    dec.close()


@pytest.mark.gpu
def test_gpu_subsampled_rgb_decodes(hip, po):
    """GPUJPEG's streams for RGB input with subsampling=420 / 422 (R,G,B components, the first one at 2x2 / 2x1): decoded, not refused"""
    from ultragrid_amd import lib as L
    w, h = 96, 64
    for code in (420, 422):
        for nonint in (False, True):
            data = layout_stream(po, w, h, code, restart=4, nonint=nonint, rgb="both")
            assert hip.jpeg_read_info(data)["is_rgb"]
            dec = hip.JpegDecoder()
            got = dec.decode(data, L.PF_RGB).cpu().numpy().reshape(h, 3 * w)
            dec.close()
            _, crop, _ = po.jpeg_decode_planes(data)
            assert np.array_equal(got, expected(po, crop, _ratios(data, po), w, h, True, "RGB"))


@pytest.mark.gpu
def test_gpu_refusals_write_nothing(hip, po):
    """I420 output stays for 4:2:0 streams; a refused output leaves the destination as it was"""
    from ultragrid_amd import lib as L
    w, h = 40, 24
    data = layout_stream(po, w, h, 440, restart=2)
    dec = hip.JpegDecoder()
    with pytest.raises(L.UgHipError):
        dec.decode(data, L.PF_I420)
    with pytest.raises(L.UgHipError):
        _decode_to(dec, data, L.PF_V210, w, h, 4096)
    dec.close()


def _transpose_coefs(coefs, gw, gh):
    """the blocks of a (gh x gw)-block grid, transposed as jpegtran -transpose does: grid and every block's coefficients"""
    zz = np.array(ZIGZAG)
    nat_of = np.empty(64, int)
    nat_of[zz] = np.arange(64)                       # natural index -> zig-zag position
    t_nat = (zz % 8) * 8 + zz // 8                    # natural index of the transposed coefficient at each zig-zag position
    blocks = coefs.reshape(gh, gw, 64).transpose(1, 0, 2)
    return np.ascontiguousarray(blocks[..., nat_of[t_nat]]).reshape(-1, 64)


@pytest.mark.gpu
@pytest.mark.parametrize("nonint", [False, True], ids=["interleaved", "nonint"])
def test_gpu_440_is_the_transposed_422(hip, po, nonint):
    """a Y'CbCr 4:2:2 stream and its jpegtran-style transpose (4:4:0: luma 1x2, the blocks and their coefficients transposed): the planes of the
    one are the transposed planes of the other up to one code value (libjpeg's IDCT is separable, but its two passes round between them),
    and both equal the oracle's"""
    w, h = 144, 80
    ql, qc = po.jpeg_qtable(80, 0), po.jpeg_qtable(80, 1)
    f422 = ((2, 1), (1, 1), (1, 1))
    c422 = layout_coefs(po, picture(w, h, 3), f422, ql, qc, None)
    d422 = write_layout_jpeg(w, h, f422, ql, qc, c422, restart=4, nonint=nonint)
    grids = geometry(w, h, f422)[4]
    c440 = [_transpose_coefs(c, gw, gh) for c, (gw, gh) in zip(c422, grids)]
    qt_t = [np.ascontiguousarray(np.asarray(q).reshape(8, 8).T).ravel() for q in (ql, qc)]  # the quantisers transposed with the coefficients
    d440 = write_layout_jpeg(h, w, ((1, 2), (1, 1), (1, 1)), qt_t[0], qt_t[1], c440, restart=4, nonint=nonint)
    assert hip.jpeg_read_info(d440)["subsampling"] == 440
    dec = hip.JpegDecoder()
    p422 = [p.cpu().numpy() for p in dec.planes(d422)]
    p440 = [p.cpu().numpy() for p in dec.planes(d440)]
    dec.close()
    o422, o440 = po.jpeg_decode_planes(d422)[1], po.jpeg_decode_planes(d440)[1]
    for c in range(3):
        assert np.array_equal(p422[c], o422[c]) and np.array_equal(p440[c], o440[c])
        assert p440[c].shape == p422[c].T.shape
        diff = np.abs(p440[c].astype(int) - p422[c].T.astype(int))
        assert diff.max() <= 1 and (diff == 0).mean() > 0.9


@needs_dec_harness
@pytest.mark.gpu
@pytest.mark.parametrize("code,sub,rgb", [(420, 4200, "both"), (422, 4220, "both"), (440, 4440, None), (411, 4220, None), (410, 4200, None),
                                          (444, 4440, None), (420, 4200, None)])
def test_gpu_receiving_module_probe_and_decode(tmp_path, hip, po, code, sub, rgb):
    """jpeg_mi355x inside the receiver's framework: the probe's code (the table next to gpujpeg.c:236-258) and the frame, UYVY and RGBA"""
    w, h = 128, 72
    data = layout_stream(po, w, h, code, restart=4, rgb=rgb, seed=4)
    src = tmp_path / "f.jpg"
    src.write_bytes(data)
    _, crop, _ = po.jpeg_decode_planes(data)
    for out in ("UYVY", "RGBA"):
        dst = tmp_path / f"{out}.raw"
        ls = po.linesize(w, out)
        r = subprocess.run([DEC_HARNESS, "JPEG", out, str(w), str(h), str(src), str(dst), str(ls)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        assert f"depth=8 subsampling={sub} rgb={int(rgb is not None)}" in r.stdout, r.stdout
        got = np.fromfile(dst, np.uint8)[: ls * h].reshape(h, ls)
        assert np.array_equal(got, expected(po, crop, _ratios(data, po), w, h, rgb is not None, out))


@needs_dec_harness
@pytest.mark.gpu
@pytest.mark.parametrize("code", [420, 422])
@pytest.mark.parametrize("out", ["DXT1", "DXT5"])
def test_gpu_jpeg_to_dxt_subsampled_rgb(tmp_path, hip, po, code, out):
    """jpeg_to_dxt_mi355x on subsampled R,G,B streams: the DXT oracle on the replicated picture, bottom-up as the transcoder writes it"""
    w, h = 128, 64
    data = layout_stream(po, w, h, code, restart=4, rgb="both", seed=5)
    src, dst = tmp_path / "f.jpg", tmp_path / "out.dxt"
    src.write_bytes(data)
    r = subprocess.run([DEC_HARNESS, "JPEG", out, str(w), str(h), str(src), str(dst)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    _, crop, _ = po.jpeg_decode_planes(data)
    pic = expected(po, crop, _ratios(data, po), w, h, True, "RGB").ravel()
    want = po.dxt_encode(po.IN_RGB, po.OUT_DXT1 if out == "DXT1" else po.OUT_DXT5YCOCG, pic, w, -h, ties="away")
    assert np.array_equal(np.fromfile(dst, np.uint8), want)


# ---- the old layouts keep their kernels ----
_TRACE_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import torch
from oracle import pyoracle as po
from jpeg_layout_bitstream import layout_stream
from ultragrid_amd import codec, lib as L
code, rgb = int(sys.argv[1]), (sys.argv[2] if sys.argv[2] != "-" else None)
dec = codec.JpegDecoder()
data = layout_stream(po, 64, 32, code, restart=2, rgb=rgb)
for out in (L.PF_UYVY, L.PF_RGBA):
    dec.decode(data, out)
torch.cuda.synchronize()
"""


def _kernels_of(tmp_path, code, rgb):
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    script = tmp_path / "one.py"
    script.write_text(_TRACE_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, "tests")))
    outdir = tmp_path / f"trace_{code}_{rgb}"
    r = subprocess.run([exe, "--kernel-trace", "--output-format", "csv", "-d", str(outdir), "-o", "run", "--", sys.executable, str(script), str(code),
                        rgb or "-"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    files = glob.glob(str(outdir / "**" / "*kernel_trace.csv"), recursive=True)
    assert files, r.stdout[-2000:]
    return "\n".join(open(f).read() for f in files)


@pytest.mark.gpu
@pytest.mark.parametrize("code,rgb,new", [(422, None, False), (420, None, False), (444, None, False), (444, "adobe", False),
                                          (440, None, True), (420, "adobe", True)])
def test_gpu_old_layouts_keep_their_kernels(tmp_path, hip, code, rgb, new):
    """a kernel trace: the layouts the decoder took before go through the kernels they went through (their bytes are pinned by the older
    tests); layout_pack_kernel runs for the new ones only"""
    trace = _kernels_of(tmp_path, code, rgb)
    assert ("layout_pack_kernel" in trace) == new
    assert "idct_kernel" in trace
