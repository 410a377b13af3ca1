"""GPU: ug_hip_pixfmt_convert_batch on packed batches whose line count crosses the two thresholds of its front end (csrc/pixfmt.hip):
frames one picture apart are ONE picture of height * frames lines -- up to 65535 lines the fast tier may take it, above that the generic
kernels do, and past 4 * 65535 lines the call converts frame by frame.  48-pixel lines, one pair per kernel family and RGBA -> UYVY_GL;
frames 0, 1, the middle and the last one against the reference converter on the same bytes (tests/pitch_layout.py; UYVY_GL: the
restatement of the shader), the whole output against single-frame ug_hip_pixfmt_convert calls, canaries at both ends."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pitch_layout as pl  # noqa: E402
import uyvy_glsl_restatement as rs_uyvy  # noqa: E402

pytestmark = pytest.mark.gpu
WIDTH = 48
# fast tier; fast tier over 10-bit words; RGB source; a pair of csrc/pixfmt_ext.hip; the shader's UYVY
PAIRS = [("UYVY", "RGBA"), ("v210", "UYVY"), ("RGB", "UYVY"), ("R10k", "RGB"), ("RGBA", "UYVY_GL")]
# height x frames = 65535: the last with the fast tier; 65536: the first without; 262140: the last single launch; 262144: frame by frame
SHAPES = [(4369, 15), (4096, 16), (4369, 60), (4096, 64)]
assert [h * n for h, n in SHAPES] == [65535, 65536, 262140, 262144]


def _pf(L, name):
    return L.PF_UYVY_GL if name == "UYVY_GL" else L.PF_NAMES[name]


def _sizes(po, i, o):
    """-> (source line, destination line) bytes"""
    if o == "UYVY_GL":
        return WIDTH * 4, WIDTH * 2
    sz = pl.Sizes(po, i, o, WIDTH)
    assert sz.dst_line == sz.written_len
    return sz.src_line, sz.dst_line


def _need(po, i, o):
    if o != "UYVY_GL" and not po.have_ref() and not pl.restated(i, o):
        pytest.skip("oracle/_ref not built")


def _reference_frame(po, i, o, src, f, h, sl, dl):
    """frame f of the packed batch in `src` by the reference: the pair's line converter, line by line on the same bytes"""
    if o == "UYVY_GL":
        return rs_uyvy.rgb_to_uyvy_gl(src[f * sl * h: (f + 1) * sl * h], WIDTH, h, 4)
    out = pl.aligned_bytes(dl * h, fill=pl.FILL)
    dec = pl.line_converter(po, i, o)
    s0, d0 = src.ctypes.data + f * sl * h, out.ctypes.data
    for y in range(h):
        dec(d0 + y * dl, s0 + y * sl, dl, *pl.SHIFTS[0])
    return out


def _batch(hip, i, o, src, h, frames, sl, dl):
    """the packed batch through ug_hip_pixfmt_convert_batch and through one ug_hip_pixfmt_convert call per frame -> the two whole
    destination buffers (GUARD canaries at both ends)"""
    import torch
    L = hip.L
    lib = L.load()
    dsrc = torch.from_numpy(src).cuda()
    outs = []
    for batched in (True, False):
        ddst = torch.full((pl.GUARD + dl * h * frames + pl.GUARD,), pl.FILL, dtype=torch.uint8, device="cuda")
        assert dsrc.data_ptr() % 256 == 0 and ddst.data_ptr() % 256 == 0
        d0 = ddst.data_ptr() + pl.GUARD
        if batched:
            rc = lib.ug_hip_pixfmt_convert_batch(_pf(L, i), _pf(L, o), dsrc.data_ptr(), d0, WIDTH, h, 0, 0, *pl.SHIFTS[0], frames, sl * h, dl * h, None)
            assert rc == 0, (i, o, h, frames, L.last_error())
        else:
            for f in range(frames):
                rc = lib.ug_hip_pixfmt_convert(_pf(L, i), _pf(L, o), dsrc.data_ptr() + f * sl * h, d0 + f * dl * h, WIDTH, h, 0, 0, *pl.SHIFTS[0], None)
                assert rc == 0, (i, o, h, f, L.last_error())
        torch.cuda.synchronize()
        outs.append(ddst.cpu().numpy())
    return outs


def _source(sl, lines, seed):
    return pl.aligned_bytes(sl * lines + pl.SLACK, rng=np.random.default_rng(seed))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_packed_batch_across_the_line_thresholds(hip, po, pair, shape):
    i, o = pair
    _need(po, i, o)
    h, frames = shape
    assert o == "UYVY_GL" or hip.L.load().ug_hip_pixfmt_supported(_pf(hip.L, i), _pf(hip.L, o)) == 1
    sl, dl = _sizes(po, i, o)
    src = _source(sl, h * frames, seed=h + frames)
    got, single = _batch(hip, i, o, src, h, frames, sl, dl)
    G = pl.GUARD
    assert np.all(got[:G] == pl.FILL) and np.all(got[G + dl * h * frames:] == pl.FILL), "canaries of the batch"
    assert np.all(single[:G] == pl.FILL) and np.all(single[G + dl * h * frames:] == pl.FILL), "canaries of the single calls"
    for f in sorted({0, 1, frames // 2, frames - 1}):
        want = _reference_frame(po, i, o, src, f, h, sl, dl)
        part = got[G + f * dl * h: G + (f + 1) * dl * h]
        bad = np.flatnonzero(part != want)
        assert bad.size == 0, (i, o, h, frames, f, bad.size, "first at line", int(bad[0]) // dl, "byte", int(bad[0]) % dl)
    bad = np.flatnonzero(got != single)
    assert bad.size == 0, (i, o, h, frames, bad.size, "first at line", (int(bad[0]) - G) // dl)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_65535_and_65536_lines_agree(hip, po, pair):
    """the same packed lines as 15 frames of 4369 (65535 lines: the fast tier where the pair has one) and as 16 frames of 4096 (65536: the
    generic kernels): the 65535 lines both batches hold come out the same"""
    i, o = pair
    _need(po, i, o)
    sl, dl = _sizes(po, i, o)
    src = _source(sl, 65536, seed=7)
    a, _ = _batch(hip, i, o, src, *SHAPES[0], sl, dl)
    b, _ = _batch(hip, i, o, src, *SHAPES[1], sl, dl)
    n = pl.GUARD + 65535 * dl
    assert np.array_equal(a[:n], b[:n])
    assert np.all(a[n:] == pl.FILL) and np.all(b[n + dl:] == pl.FILL) and np.any(b[n: n + dl] != pl.FILL)
