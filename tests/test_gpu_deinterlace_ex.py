"""GPU: ug_hip_deinterlace byte for byte (0 bytes differing: integer arithmetic) against the numpy restatement (tests/deinterlace_restatement.py)
and -- BLEND, where oracle/_ref/libugref.so is built -- against the reference's compiled vc_deinterlace_ex itself: every supported format x
every mode (WEAVE with and without the blend) x line sizes that are no multiple of 16 / 36 / 4, pitched and misaligned destinations, batches,
dst == src, and 1920x1080 / 3840x2160 frames.  Every destination is pre-filled and lies between guard bytes; the WHOLE buffer is compared."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import deinterlace_restatement as rs  # noqa: E402
from ultragrid_amd import lib as L  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 64
REF_SO = os.path.join(HERE, "..", "oracle", "_ref", "libugref.so")
VARIANTS = [("BLEND", rs.BLEND, False), ("WEAVE", rs.WEAVE, False), ("WEAVE:d", rs.WEAVE, True), ("BOB", rs.BOB, False), ("LINEAR", rs.LINEAR, False)]
LINE_SIZES = {"u8": [16, 21, 36, 100, 399, 400], "u16": [16, 18, 36, 100, 398, 400], "v210": [16, 20, 36, 100, 128, 400],
              "r10k": [16, 20, 36, 100, 256, 400], "r12l": [16, 20, 36, 72, 100, 108, 144, 396, 400]}
HEIGHTS = [2, 3, 4, 5, 12, 13, 16, 17, 33, 34]


def _ref():
    if not os.path.exists(REF_SO):
        return None
    ref = C.CDLL(REF_SO)
    ref.get_codec_from_name.argtypes, ref.get_codec_from_name.restype = [C.c_char_p], C.c_int
    ref.vc_deinterlace_ex.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t]
    ref.vc_deinterlace_ex.restype = C.c_bool
    return ref


def gpu(pf, mode, src, prev, Lb, bgs, blend=False, in_place=False):
    """src / prev: [frames, H, sp]; bgs: what the destinations hold before, [frames, H, dp] each.  Returns the destinations after the call
    (guards checked).  in_place: BLEND over the source itself."""
    frames, H, sp = src.shape
    dsrc = torch.from_numpy(src.reshape(-1)).cuda()
    dprev = torch.from_numpy(prev.reshape(-1)).cuda() if prev is not None else None
    guard = np.full(GUARD, 0x5A, np.uint8)
    ddst = [None if in_place else torch.from_numpy(np.concatenate([guard, bg.reshape(-1), guard])).cuda() for bg in bgs]
    dp = sp if in_place else bgs[0].shape[2]
    ptr = [dsrc.data_ptr() if in_place else t.data_ptr() + GUARD for t in ddst]
    d = L.DeinterlaceDesc(dsrc.data_ptr(), dprev.data_ptr() if dprev is not None else None, (C.c_void_p * 2)(ptr[0], ptr[1] if len(ptr) > 1 else None),
                          pf, mode, int(blend), H, Lb, sp, dp, frames, sp * H, dp * H)
    rc = L.load().ug_hip_deinterlace(C.byref(d), None)
    assert rc == L.SUCCESS, (rc, L.last_error())
    torch.cuda.synchronize()
    if in_place:
        return [dsrc.cpu().numpy().reshape(src.shape)]
    out = []
    for t, bg in zip(ddst, bgs):
        a = t.cpu().numpy()
        assert np.all(a[:GUARD] == 0x5A) and np.all(a[-GUARD:] == 0x5A), "guard bytes around a destination were written"
        out.append(a[GUARD:-GUARD].reshape(bg.shape))
    return out


def check(name, cls, pf, vname, mode, blend, Lb, H, frames, sp, dp, rng, ref=None, codec=0, in_place=False):
    src = rng.integers(0, 256, (frames, H, sp), dtype=np.uint8)
    prev = rng.integers(0, 256, (frames, H, sp), dtype=np.uint8) if mode == rs.WEAVE else None
    n_out = 1 if mode == rs.BLEND else 2
    bgs = [src] if in_place else [rng.integers(0, 256, (frames, H, dp), dtype=np.uint8) for _ in range(n_out)]
    got = gpu(pf, mode, src, prev, Lb, bgs, blend, in_place)
    bad = 0
    for f in range(frames):
        want = rs.run(cls, mode, src[f], Lb, [b[f] for b in bgs], None if prev is None else prev[f], blend)
        for k in range(n_out):
            bad += int(np.count_nonzero(got[k][f] != want[k]))
        if ref is not None and mode == rs.BLEND and sp == Lb:  # the compiled reference itself (its source pitch is the line size)
            d = np.ascontiguousarray(bgs[0][f]).copy()
            assert ref.vc_deinterlace_ex(codec, np.ascontiguousarray(src[f]).ctypes.data, Lb, d.ctypes.data, dp, H)
            bad += int(np.count_nonzero(got[0][f] != d))
    assert bad == 0, f"{name} {vname} L={Lb} H={H} frames={frames} sp={sp} dp={dp} in_place={in_place}: {bad} bytes differ"


@pytest.mark.parametrize("name", sorted(rs.FORMATS))
def test_every_mode_and_geometry(name):
    pf, cls, ref_name = rs.FORMATS[name]
    ref = _ref()
    codec = ref.get_codec_from_name(ref_name.encode()) if ref else 0
    rng = np.random.default_rng(sum(name.encode()))
    unit, n = rs.UNIT[cls], 0
    assert L.load().ug_hip_deinterlace_supported(pf, rs.LINEAR) == 1
    for vname, mode, blend in VARIANTS:
        for Lb in LINE_SIZES[cls]:
            for H in ([1] if mode == rs.BLEND else []) + HEIGHTS:
                if mode == rs.WEAVE and H % 2:
                    continue
                # the destination pitch: the line size; 16-byte aligned with a gap (the dwordx4 path where the line size allows); off by one element
                dp = (Lb, (Lb + 15) // 16 * 16 + 16, Lb + unit)[n % 3]
                sp = Lb if n % 4 else (Lb + 15) // 16 * 16 + 32
                check(name, cls, pf, vname, mode, blend, Lb, H, (1, 8)[n % 2], sp, dp, rng, ref, codec)
                n += 1
            if mode == rs.BLEND:
                for H in (1, 2, 13, 34):
                    check(name, cls, pf, vname, mode, blend, Lb, H, (1, 8)[H % 2], Lb, Lb, rng, in_place=True)
    assert n >= 200


@pytest.mark.parametrize("frames", [1, 8])
@pytest.mark.parametrize("w,h", [(1920, 1080), (3840, 2160)])
@pytest.mark.parametrize("name", ["UYVY", "v210", "R12L", "RG48"])
def test_full_frames(name, w, h, frames):
    pf, cls, ref_name = rs.FORMATS[name]
    ref = _ref()
    codec = ref.get_codec_from_name(ref_name.encode()) if ref else 0
    Lb = L.load().ug_hip_linesize(pf, w)
    rng = np.random.default_rng(w + frames)
    for vname, mode, blend in VARIANTS:
        check(name, cls, pf, vname, mode, blend, Lb, h, frames, Lb, Lb, rng, ref, codec)


def test_unsupported_format_is_refused():
    d = L.DeinterlaceDesc(0x1000, None, (C.c_void_p * 2)(0x2000, None), L.PF_I420, rs.BLEND, 0, 4, 16, 0, 0, 1, 0, 0)
    assert L.load().ug_hip_deinterlace(C.byref(d), None) == L.EUNSUPP
    assert L.load().ug_hip_deinterlace_supported(L.PF_I420, rs.BLEND) == 0
