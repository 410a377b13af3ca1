"""GPU: ug_hip_dxt_decode at a destination pitch -- the multiple-of-4 kernels and the EDGE instantiations (csrc/dxt_decode.hip: put_row_edge
picks 128-bit, 64-bit or unaligned 32-bit row stores from the pitch) against oracle/dxt_decode_oracle.c laid line by line into the
pitched buffer, canaries in front, behind and in every line's padding (tests/pitch_layout.py); and the pitch / alignment refusals of
include/ug_mi355x.h as a table."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pitch_layout as pl  # noqa: E402
from ultragrid_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
BPP = {"RGB": 3, "BGR": 3, "RGBA": 4, "UYVY": 2}
SIZES = [(64, 16), (66, 9), (10, 7), (64, 6)]   # multiples of 4; EDGE with the right and bottom blocks cut; EDGE with whole block columns


def _fmt(po, L, fmt):
    return {"dxt1": (po.OUT_DXT1, L.DXT1, 8), "dxt1_yuv": (po.OUT_DXT1_YUV, L.DXT1_YUV, 8), "dxt5ycocg": (po.OUT_DXT5YCOCG, L.DXT5_YCOCG, 16)}[fmt]


def _blocks(po, fmt, in_p, bsize, w, h, rng):
    """every other block oracle-encoded picture content, the rest arbitrary bytes (both alpha modes, 3-colour DXT1 blocks)"""
    if fmt == "dxt1_yuv":
        enc = po.dxt_encode(po.IN_UYVY_RAW, po.OUT_DXT1, synth.frame("S2", "UYVY", w, h), w, h)
    else:
        enc = po.dxt_encode(po.IN_RGB, in_p, synth.frame("S2", "RGB", w, h), w, h)
    blocks = enc.reshape(-1, bsize).copy()
    assert blocks.shape[0] == ((w + 3) // 4) * ((h + 3) // 4)
    blocks[1::2] = rng.integers(0, 256, blocks[1::2].shape, dtype=np.uint8)
    return blocks.reshape(-1)


def _pitches(out, w, h):
    line = w * BPP[out]
    p = [line, (line + 15) // 16 * 16 + 32]
    if (w & 3) or (h & 3):
        p += [line + 4] if out in ("RGBA", "UYVY") else [line + 1, line + 13]
    return p


def _accepts(out, w, h, pitch):
    """the header's rule"""
    if pitch < w * BPP[out]:
        return False
    if (w & 3) or (h & 3):
        return pitch % 4 == 0 if out in ("RGBA", "UYVY") else True
    return pitch % {"RGBA": 16, "UYVY": 8, "RGB": 4, "BGR": 4}[out] == 0


def _decode(L, in_l, out, dsrc_ptr, dst, front, w, h, pitch, sh=(0, 8, 16)):
    import torch
    ddst = torch.from_numpy(dst).cuda()
    assert ddst.data_ptr() % 256 == 0
    rc = L.load().ug_hip_dxt_decode(in_l, L.PF_NAMES[out], dsrc_ptr, ddst.data_ptr() + front, w, h, pitch, *sh, None)
    torch.cuda.synchronize()
    return rc, ddst.cpu().numpy()


@pytest.mark.parametrize("out", ["RGB", "BGR", "RGBA", "UYVY"])
@pytest.mark.parametrize("fmt", ["dxt1", "dxt1_yuv", "dxt5ycocg"])
def test_decode_at_a_destination_pitch(hip, po, fmt, out):
    import torch
    L = hip.L
    in_p, in_l, bsize = _fmt(po, L, fmt)
    rng = np.random.default_rng(23)
    problems, n = [], 0
    for (w, h) in SIZES:
        blocks = _blocks(po, fmt, in_p, bsize, w, h, rng)
        dsrc = torch.from_numpy(blocks).cuda()
        line = w * BPP[out]
        for sh in (pl.SHIFTS if out == "RGBA" else pl.SHIFTS[:1]):
            packed = po.dxt_decode(in_p, out, blocks, w, h, sh).reshape(h, line)   # decoding is position-local: nothing reads past a line
            for pitch in _pitches(out, w, h):
                assert _accepts(out, w, h, pitch), (out, w, h, pitch)
                want, front = pl.make_dst(h, pitch, 0)
                want[front: front + h * pitch].reshape(h, pitch)[:, :line] = packed
                dst, _ = pl.make_dst(h, pitch, 0)
                rc, got = _decode(L, in_l, out, dsrc.data_ptr(), dst, front, w, h, pitch, sh)
                if rc != 0:
                    problems.append((w, h, pitch, "rc", rc, L.last_error()))
                    continue
                found = pl.compare(got, want, h, pitch, line, front)
                if found:
                    problems.append((w, h, pitch, sh, found))
                n += 1
    assert not problems, (fmt, out, problems)
    assert n >= 2 * 1 + 3 * 2   # one aligned size at two pitches, three EDGE sizes at three or four


# (out, width, height, pitches refused, pitches accepted) from csrc/dxt_decode.hip: ug_hip_dxt_decode_ex
PITCH_TABLE = [
    ("RGBA", 64, 16, [256 + 4, 256 + 8, 256 + 12, 256 + 2, 252, 128], [256, 256 + 16]),
    ("UYVY", 64, 16, [128 + 4, 128 + 12, 128 + 2, 124, 120], [128, 128 + 8]),
    ("RGB", 64, 16, [192 + 1, 192 + 2, 192 + 3, 188], [192, 192 + 4]),
    ("BGR", 64, 16, [192 + 1, 192 + 2, 192 + 3, 188], [192, 192 + 4]),
    ("RGBA", 66, 9, [264 + 1, 264 + 2, 264 + 3, 260, 256], [264, 264 + 4, 264 + 8]),
    ("UYVY", 66, 9, [132 + 1, 132 + 2, 132 + 3, 128], [132, 132 + 4]),
    ("RGB", 66, 9, [197, 196, 192], [198, 199, 200, 201]),
    ("BGR", 10, 7, [29, 28, 16], [30, 31, 32, 33]),
    ("RGBA", 64, 6, [256 + 2, 252, 240], [256, 256 + 4, 256 + 16]),
    ("UYVY", 64, 6, [128 + 2, 124, 120], [128, 128 + 4, 128 + 8]),
]


@pytest.mark.parametrize("fmt", ["dxt1", "dxt5ycocg"])
def test_pitch_and_alignment_refusals(hip, po, fmt):
    """what the header states: each refusal is UG_HIP_EINVAL and leaves the destination untouched; each accepted pitch decodes like the
    packed call"""
    import torch
    L = hip.L
    in_p, in_l, bsize = _fmt(po, L, fmt)
    rng = np.random.default_rng(29)
    problems = []
    for out, w, h, refused, accepted in PITCH_TABLE:
        line = w * BPP[out]
        blocks = _blocks(po, fmt, in_p, bsize, w, h, rng)
        dsrc = torch.zeros(blocks.size + 64, dtype=torch.uint8, device="cuda")
        dsrc[: blocks.size] = torch.from_numpy(blocks).cuda()
        packed = po.dxt_decode(in_p, out, blocks, w, h).reshape(h, line)
        room = max(refused + accepted + [line])
        for pitch in refused:
            assert not _accepts(out, w, h, pitch)
            dst, front = pl.make_dst(h, room, 0)
            rc, got = _decode(L, in_l, out, dsrc.data_ptr(), dst, front, w, h, pitch)
            if rc != L.EINVAL or not (got == pl.FILL).all():
                problems.append((out, w, h, "pitch", pitch, "rc", rc, "written", int((got != pl.FILL).sum())))
        for pitch in accepted:
            assert _accepts(out, w, h, pitch)
            want, front = pl.make_dst(h, pitch, 0)
            want[front: front + h * pitch].reshape(h, pitch)[:, :line] = packed
            dst, _ = pl.make_dst(h, pitch, 0)
            rc, got = _decode(L, in_l, out, dsrc.data_ptr(), dst, front, w, h, pitch)
            found = [("rc", rc, L.last_error())] if rc != 0 else pl.compare(got, want, h, pitch, line, front)
            if found:
                problems.append((out, w, h, "pitch", pitch, found))
        # the destination base: 16 bytes; the source: 16 bytes (DXT5), 8 bytes (DXT1)
        src_need = 16 if fmt == "dxt5ycocg" else 8
        pitch = accepted[0]
        for dst_off, src_off in [(4, 0), (8, 0), (1, 0), (0, 4), (0, 1), (0, src_need // 2)]:
            dst, front = pl.make_dst(h, room, 0)
            rc, got = _decode(L, in_l, out, dsrc.data_ptr() + src_off, dst, front + dst_off, w, h, pitch)
            if rc != L.EINVAL or not (got == pl.FILL).all():
                problems.append((out, w, h, "offsets", dst_off, src_off, "rc", rc, "written", int((got != pl.FILL).sum())))
        if fmt == "dxt1":   # an 8-byte aligned DXT1 source that is not 16-byte aligned is taken
            shifted = torch.zeros(blocks.size + 64, dtype=torch.uint8, device="cuda")
            shifted[8: 8 + blocks.size] = torch.from_numpy(blocks).cuda()
            want, front = pl.make_dst(h, pitch, 0)
            want[front: front + h * pitch].reshape(h, pitch)[:, :line] = packed
            dst, _ = pl.make_dst(h, pitch, 0)
            rc, got = _decode(L, in_l, out, shifted.data_ptr() + 8, dst, front, w, h, pitch)
            found = [("rc", rc, L.last_error())] if rc != 0 else pl.compare(got, want, h, pitch, line, front)
            if found:
                problems.append((out, w, h, "source + 8", found))
    assert not problems, (fmt, problems)
