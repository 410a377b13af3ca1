"""GPU: ug_hip_pixfmt_convert and ug_hip_pixfmt_convert_batch at pitches and base addresses that move the dispatch between its tiers
(csrc/pixfmt.hip: try_fast, launch_generic; csrc/pixfmt_ext.hip: pixfmt_ext_convert): every pair of decoders[] and the identity copies
against the reference run on the same pitched bytes (tests/pitch_layout.py), byte for byte, with canaries in front of the destination,
behind it and in every line's padding; the alignment rule of every pair; batches as one tall picture up to and past the line counts at
which the launch changes."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pitch_layout as pl  # noqa: E402

pytestmark = pytest.mark.gpu
PAIRS = pl.all_pairs()
SIZES = [(96, 5), (100, 5), (7, 5), (1366, 5), (96, 1)]   # 5 lines: the y guard of the 64 x 4 workgroups
DONE = {}   # pair -> comparisons made (test_every_pair_ran)


def _need(po, i, o):
    if not po.have_ref() and not pl.restated(i, o):
        pytest.skip("oracle/_ref not built")


def _upload(buf):
    import torch
    dev = torch.from_numpy(buf).cuda()
    assert dev.data_ptr() % 256 == 0
    return dev


def _convert(L, i, o, src, so, dst, front, w, h, sp, dp, sh):
    """one ug_hip_pixfmt_convert call on device copies of the two host buffers -> (rc, the whole destination buffer afterwards)"""
    import torch
    dsrc, ddst = _upload(src), _upload(dst)
    rc = L.load().ug_hip_pixfmt_convert(L.PF_NAMES[i], L.PF_NAMES[o], dsrc.data_ptr() + so, ddst.data_ptr() + front, w, h, sp, dp, *sh, None)
    torch.cuda.synchronize()
    return rc, ddst.cpu().numpy()


def _shifts(o):
    return pl.SHIFTS if o in ("RGB", "RGBA") else pl.SHIFTS[:1]


def run_layouts(hip, po, i, o):
    L = hip.L
    problems, n = [], 0
    for (w, h) in SIZES:
        if not pl.width_ok(i, o, w):
            continue
        sz = pl.Sizes(po, i, o, w)
        for name in pl.LAYOUTS:
            sp, dp, so, do = pl.layout(name, i, o, sz)
            for sh in _shifts(o):
                src = pl.make_src(h, sp, so, np.random.default_rng(w + 7 * h + sh[0]))
                want, front = pl.ref_convert_pitched(po, i, o, src, so, w, h, sp, dp, sh, dst_off=do)
                dst, _ = pl.make_dst(h, dp, do)
                rc, got = _convert(L, i, o, src, so, dst, front, w, h, sp, dp, sh)
                if rc != 0:
                    problems.append((w, h, name, sh, "rc", rc, L.last_error()))
                    continue
                found = pl.compare(got, want, h, dp, sz.written_len, front)
                if found:
                    problems.append((w, h, name, sh, (sp, dp, so, do), found))
                n += 1
    return problems, n


def run_alignment_rule(hip, po, i, o):
    """A base or a pitch that is off a format's own alignment by 1 (and by 2 for the 32-bit formats), one argument at a time.  The pairs of
    csrc/pixfmt_ext.hip refuse what is below their rule (pl.ext_rule) with UG_HIP_EINVAL and write nothing; whatever is accepted -- the
    17 pairs of csrc/pixfmt.hip and the copies work bytewise and take every address and pitch -- converts exactly like an aligned call."""
    L = hip.L
    w, h = 96, 5
    sz = pl.Sizes(po, i, o, w)
    rule = (1, 1) if (i, o) in pl.CORE_PAIRS or (i, o) in pl.COPIES else pl.ext_rule(i, o)
    sp0, dp0, _, _ = pl.layout("padded16", i, o, sz)
    problems = []
    for side in (0, 1):
        a = max(rule[side], pl.natural_align(o if side else i, bool(side)))
        for off in [k for k in (1, 2) if k < a]:
            for what in ("base", "pitch"):
                sp, dp = sp0 + (off if (side, what) == (0, "pitch") else 0), dp0 + (off if (side, what) == (1, "pitch") else 0)
                so, do = (off if (side, what) == (0, "base") else 0), (off if (side, what) == (1, "base") else 0)
                sh = pl.SHIFTS[0]
                src = pl.make_src(h, sp, so, np.random.default_rng(off + 3 * side))
                dst, front = pl.make_dst(h, dp, do)
                rc, got = _convert(L, i, o, src, so, dst, front, w, h, sp, dp, sh)
                tag = ("src" if side == 0 else "dst", what, off)
                if off % rule[side]:
                    if rc != L.EINVAL:
                        problems.append((tag, "not refused", rc))
                    if not (got == pl.FILL).all():
                        problems.append((tag, "refused, yet the destination was written"))
                else:
                    want, _ = pl.ref_convert_pitched(po, i, o, src, so, w, h, sp, dp, sh, dst_off=do, scratch=True)
                    found = [("rc", rc, L.last_error())] if rc != 0 else pl.compare(got, want, h, dp, sz.written_len, front)
                    if found:
                        problems.append((tag, "accepted", found))
    return problems


def run_pair(hip, po, i, o):
    L = hip.L
    assert L.load().ug_hip_pixfmt_supported(L.PF_NAMES[i], L.PF_NAMES[o]) == 1
    problems, n = run_layouts(hip, po, i, o)
    problems += run_alignment_rule(hip, po, i, o)
    DONE[(i, o)] = n
    assert not problems, (i, o, problems)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_pair_at_pitches_and_base_offsets(hip, po, pair):
    _need(po, *pair)
    run_pair(hip, po, *pair)


def test_every_pair_ran(hip, po):
    """with oracle/_ref there, no pair is left out and at least 64 pairs x 5 sizes x 4 layouts comparisons were made (pairs deselected from
    this run are made up for here)"""
    if not po.have_ref():
        pytest.skip("oracle/_ref not built")
    for pair in PAIRS:
        if pair not in DONE:
            run_pair(hip, po, *pair)
    assert len(DONE) == 64 and all(DONE.values())
    # (DVS10 -> UYVY takes 96-pixel lines only: 2 sizes; the RGB and RGBA outputs run both shift triples)
    assert sum(DONE.values()) >= 64 * 5 * 4, sum(DONE.values())


# ------------------------------------------------ batches as one tall picture ------------------------------------------------
# one pair per kernel family: fast tier; generic_vec_kernel; xvec_kernel; the R12L pixel and quad kernels; the copy
BATCH_PAIRS = [("v210", "UYVY"), ("UYVY", "RGBA"), ("RGBA", "UYVY"), ("v210", "RG48"), ("R10k", "RGB"), ("R12L", "RGB"), ("RGB", "R12L"),
               ("UYVY", "UYVY")]


def _batch(hip, po, i, o, w, h, frames, sp, dp, sstride, dstride, pitch_args, seed):
    """`frames` pictures at the given strides through ug_hip_pixfmt_convert_batch against the reference, line by line on the same bytes"""
    import torch
    L = hip.L
    sz = pl.Sizes(po, i, o, w)
    sh = pl.SHIFTS[0]
    src = pl.aligned_bytes(frames * sstride + pl.SLACK, rng=np.random.default_rng(seed))
    front = pl.GUARD
    dst = pl.aligned_bytes(front + frames * dstride + pl.GUARD, fill=pl.FILL)
    want = dst.copy()
    dec = pl.line_converter(po, i, o)
    s0, d0, n = src.ctypes.data, want.ctypes.data + front, sz.written_len
    for f in range(frames):
        sf, df = s0 + f * sstride, d0 + f * dstride
        for y in range(h):
            dec(df + y * dp, sf + y * sp, n, *sh)
    dsrc, ddst = _upload(src), _upload(dst)
    rc = L.load().ug_hip_pixfmt_convert_batch(L.PF_NAMES[i], L.PF_NAMES[o], dsrc.data_ptr(), ddst.data_ptr() + front, w, h, *pitch_args, *sh,
                                              frames, sstride, dstride, None)
    assert rc == 0, (i, o, L.last_error())
    torch.cuda.synchronize()
    got = ddst.cpu().numpy()
    if dstride == dp * h:
        found = pl.compare(got, want, h * frames, dp, sz.written_len, front)
    else:
        found = pl.compare_frames(got, want, frames, dstride, h, dp, sz.written_len, front)
    assert not found, (i, o, w, h, frames, found)


@pytest.mark.parametrize("extra", [0, 48], ids=["one_launch", "frame_by_frame"])
@pytest.mark.parametrize("pair", BATCH_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_batch_at_padded_pitches(hip, po, pair, extra):
    """96 x 6 x 4 frames at padded 16-byte pitches: one picture apart (the single launch, with padding) and 48 bytes further apart (frame by
    frame); the gaps between the frames stay untouched"""
    _need(po, *pair)
    w, h, frames = 96, 6, 4
    sp, dp, _, _ = pl.layout("padded16", *pair, pl.Sizes(po, *pair, w))
    _batch(hip, po, *pair, w, h, frames, sp, dp, sp * h + extra, dp * h + extra, (sp, dp), seed=extra + 1)


@pytest.mark.parametrize("lines", [(8192, 8), (65535, 4), (52429, 5)], ids=["65536_lines", "262140_lines", "262145_lines"])
@pytest.mark.parametrize("pair", BATCH_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_batch_line_count_edges(hip, po, pair, lines):
    """24-pixel lines (a whole unit of every one of these kernels), packed, every line different: 65536 lines -- one past what the fast tier
    takes; 262140 -- the last single launch; 262145 -- frame by frame.  The whole output is compared."""
    _need(po, *pair)
    h, frames = lines
    sz = pl.Sizes(po, *pair, 24)
    _batch(hip, po, *pair, 24, h, frames, sz.src_line, sz.dst_line, sz.src_line * h, sz.dst_line * h, (0, 0), seed=h)
