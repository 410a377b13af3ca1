"""tests/pitch_layout.py checked on the CPU: compare() notices each way a kernel can get a pitched destination wrong, and the pitched
reference is the packed reference when the pitch is the line size."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pitch_layout as pl  # noqa: E402

H, PITCH, LEN, UNIT = 5, 112, 72, 6   # a 24-pixel RGB line in a pitch with 40 bytes of padding


def _pair():
    """(want, got): a correct destination and an independent copy of it"""
    rng = np.random.default_rng(3)
    want, front = pl.make_dst(H, PITCH, 0)
    for y in range(H):
        want[front + y * PITCH: front + y * PITCH + LEN] = rng.integers(0, 256, LEN)
    return want, want.copy(), front


def test_compare_accepts_a_correct_buffer():
    want, got, front = _pair()
    assert pl.compare(got, want, H, PITCH, LEN, front) == []
    want[front + LEN + 3] = 0   # a reference may spill behind dst_len: that is its own business
    assert pl.compare(got, want, H, PITCH, LEN, front) == []


def test_compare_notices_a_changed_padding_byte():
    want, got, front = _pair()
    got[front + 2 * PITCH + PITCH - 1] ^= 1
    f = pl.compare(got, want, H, PITCH, LEN, front)
    assert len(f) == 1 and "padding" in f[0] and "line 2" in f[0]


def test_compare_notices_a_line_at_the_packed_address():
    want, got, front = _pair()
    line = got[front + 3 * PITCH: front + 3 * PITCH + LEN].copy()
    got[front + 3 * PITCH: front + 3 * PITCH + LEN] = pl.FILL        # not where it belongs ...
    got[front + 3 * LEN: front + 4 * LEN] = line                     # ... but where a packed picture has it
    f = pl.compare(got, want, H, PITCH, LEN, front)
    assert any("differ inside the lines" in x for x in f)


def test_compare_notices_a_byte_past_written_len():
    want, got, front = _pair()
    got[front + 4 * PITCH + LEN] = 0
    f = pl.compare(got, want, H, PITCH, LEN, front)
    assert len(f) == 1 and "padding" in f[0] and f"byte {LEN}" in f[0]


def test_compare_notices_an_unwritten_last_unit():
    want, got, front = _pair()
    got[front + 1 * PITCH + LEN - UNIT: front + 1 * PITCH + LEN] = pl.FILL
    f = pl.compare(got, want, H, PITCH, LEN, front)
    assert len(f) == 1 and "differ inside the lines" in f[0] and "line 1" in f[0]


def test_compare_notices_touched_guards():
    want, got, front = _pair()
    got[front - 1] = 0
    got[front + H * PITCH] = 0
    f = pl.compare(got, want, H, PITCH, LEN, front)
    assert len(f) == 2 and "in front of" in f[0] and "behind" in f[1]
    assert pl.compare(got[:-1], want, H, PITCH, LEN, front) != []


def test_pair_lists():
    import test_gpu_pixfmt_ext as ext
    pairs = pl.all_pairs()
    assert len(pl.decoder_pairs()) == 61 and len(pairs) == 64 and len(set(pairs)) == 64
    gold = np.load(os.path.join(HERE, "golden", "pixfmt_ref.npz"))
    assert sorted(pl.CORE_PAIRS) == sorted({tuple(k.split("_")[1:3]) for k in gold.files if k.startswith("in_")})
    assert set(pl.CORE_PAIRS) | set(ext.PAIRS) | {("DVS10", "UYVY")} == set(pl.decoder_pairs())


def test_layouts(po):
    for (i, o) in pl.CORE_PAIRS if not po.have_ref() else pl.all_pairs():
        for w in (96, 100, 7, 1366):
            sz = pl.Sizes(po, i, o, w)
            for name in pl.LAYOUTS:
                sp, dp, so, do = pl.layout(name, i, o, sz)
                assert sp >= max(sz.src_line, sz.src_size) and dp >= max(sz.dst_line, sz.dst_size) and dp > sz.written_len
                assert sp % pl.natural_align(i, False) == 0 and dp % pl.natural_align(o, True) == 0
                if name == "odd_pitch":
                    assert sp % 16 and dp % 16 and (so, do) == (0, 0)
                else:
                    assert sp % 16 == 0 and dp % 16 == 0
                    assert (so != 0, do != 0) == (name == "src_off", name == "dst_off") and so < 16 and do < 16


@pytest.mark.parametrize("scratch", [False, True], ids=["in_place", "scratch"])
def test_pitched_reference_equals_the_packed_one(po, scratch, monkeypatch):
    """pitch == line size, even widths: the same bytes as po.ref_convert_frame (core pairs) / the line loop of tests/test_gpu_pixfmt_ext.py
    (the other pairs).  Without oracle/_ref: the restatement of the core pairs."""
    import test_gpu_pixfmt_ext as ext
    monkeypatch.setattr(ext, "FILL", pl.FILL)   # bytes a converter leaves alone inside dst_len: the same canary on both sides
    pairs = pl.all_pairs() if po.have_ref() else pl.CORE_PAIRS + pl.COPIES
    for (i, o) in pairs:
        for (w, h) in [(96, 3), (100, 2), (1366, 2)]:
            if not pl.width_ok(i, o, w):
                continue
            sz = pl.Sizes(po, i, o, w)
            for sh in pl.SHIFTS:
                src = pl.make_src(h, sz.src_line, 0, np.random.default_rng(w))
                src[sz.src_line * h:] = 0   # what the packed references put behind the last line (converters read past its last pixel)
                want, front = pl.ref_convert_pitched(po, i, o, src, 0, w, h, sz.src_line, sz.dst_line, sh, scratch=scratch)
                if not po.have_ref():
                    packed = po.convert_frame(i, o, src[: sz.src_line * h], w, h, sh)
                    unwritten = want[front: front + sz.dst_line * h] == pl.FILL   # the packed restatement starts from zeros
                    packed[unwritten & (packed == 0)] = pl.FILL
                elif (i, o) in pl.CORE_PAIRS or (i, o) in pl.COPIES:
                    packed = po.ref_convert_frame(i, o, src[: sz.src_line * h], w, h, sh, scalar=(i, o) in pl.CORE_PAIRS)
                else:
                    packed = ext.ref_frame(po, i, o, src, w, h, sh)[0]
                got = want[front: front + sz.dst_line * h].reshape(h, sz.dst_line)[:, : sz.written_len]
                assert np.array_equal(got, packed.reshape(h, sz.dst_line)[:, : sz.written_len]), (i, o, w, sh)
                assert (want[:front] == pl.FILL).all()


def test_pitched_reference_on_every_layout(po):
    """the reference runs on every layout the GPU tests use, and a line's result depends on the line's own bytes and at most SLACK bytes
    behind them -- the same picture at two different layouts converts to the same lines wherever the reference reads nothing past them"""
    pairs = pl.all_pairs() if po.have_ref() else pl.CORE_PAIRS + pl.COPIES
    for (i, o) in pairs:
        w, h = 96, 3
        sz = pl.Sizes(po, i, o, w)
        lines = np.random.default_rng(9).integers(0, 256, (h, sz.src_size), dtype=np.uint8)
        outs = []
        for name in pl.LAYOUTS:
            sp, dp, so, do = pl.layout(name, i, o, sz)
            src = pl.make_src(h, sp, so, np.random.default_rng(1))
            for y in range(h):
                src[so + y * sp: so + y * sp + sz.src_size] = lines[y]
            want, front = pl.ref_convert_pitched(po, i, o, src, so, w, h, sp, dp, (0, 8, 16), dst_off=do)
            assert front == pl.GUARD + do
            outs.append(want[front: front + dp * h].reshape(h, dp)[:, : sz.written_len].copy())
            assert (want[:front] == pl.FILL).all() and (want[front + dp * h:] == pl.FILL).all()
        for other in outs[1:]:
            assert np.array_equal(outs[0], other), (i, o)


def test_restated_pitched_reference_equals_the_compiled_one(po):
    """where oracle/_ref is absent the GPU tests hold the core pairs and the copies to the restatement: on every size and layout they use
    it gives the bytes of the compiled reference inside dst_len, the bytes a converter leaves alone there included"""
    if not po.have_ref():
        pytest.skip("oracle/_ref not built")
    for (i, o) in pl.CORE_PAIRS + pl.COPIES:
        for (w, h) in [(96, 5), (100, 5), (7, 5), (1366, 5), (96, 1)]:
            sz = pl.Sizes(po, i, o, w)
            for name in pl.LAYOUTS:
                sp, dp, so, do = pl.layout(name, i, o, sz)
                for sh in pl.SHIFTS:
                    src = pl.make_src(h, sp, so, np.random.default_rng(w + h))
                    a, front = pl.ref_convert_pitched(po, i, o, src, so, w, h, sp, dp, sh, dst_off=do, use_ref=True)
                    b, _ = pl.ref_convert_pitched(po, i, o, src, so, w, h, sp, dp, sh, dst_off=do, use_ref=False)
                    c, _ = pl.ref_convert_pitched(po, i, o, src, so, w, h, sp, dp, sh, dst_off=do, use_ref=False, scratch=True)
                    for other in (b, c):
                        lines = lambda v: v[front: front + dp * h].reshape(h, dp)[:, : sz.written_len]  # noqa: E731
                        assert np.array_equal(lines(a), lines(other)), (i, o, w, name, sh)
                        assert (other[:front] == pl.FILL).all()   # (behind dst_len both write whole last groups: compare() never reads that)


class _Const:
    """an `rng` whose bytes are all one value: two of them differ in every byte they supply"""

    def __init__(self, v):
        self.v = v

    def bytes(self, n):
        return bytes([self.v]) * n


@pytest.mark.parametrize("line,h,pitch,off,stride,n", [(72, 5, 72, 0, 72 * 5, 1), (72, 5, 112, 0, 112 * 5 + 80, 3), (1044, 9, 1048, 4, 1048 * 9 + 12, 3),
                                                       (144, 16, 157, 1, 157 * 16 + 12, 3)])
def test_place_frames(line, h, pitch, off, stride, n):
    """extraction gives the frames back; every byte outside the lines comes from the rng (it differs between two rngs that differ everywhere, and
    between two seeds wherever two random bytes differ: all but about one in 256), every byte inside from the frames; the buffer is 256-byte aligned
    and ends SLACK bytes behind the last line"""
    frames = [np.random.default_rng(10 + f).integers(0, 256, line * h, dtype=np.uint8) for f in range(n)]
    a = pl.place_frames(frames, line, h, pitch, off, stride, _Const(0x11))
    b = pl.place_frames(frames, line, h, pitch, off, stride, _Const(0x22))
    assert a.ctypes.data % 256 == 0 and a.size == b.size == off + (n - 1) * stride + pitch * h + pl.SLACK
    for buf in (a, b):
        back = pl.extract_frames(buf, n, line, h, pitch, off, stride)
        assert all(np.array_equal(x, y) for x, y in zip(back, frames))
    inside = pl.frame_mask(n, line, h, pitch, off, stride, a.size)
    assert inside.sum() == n * h * line
    assert (a[~inside] == 0x11).all() and (b[~inside] == 0x22).all() and np.array_equal(a[inside], b[inside])
    c = pl.place_frames(frames, line, h, pitch, off, stride, np.random.default_rng(1))
    d = pl.place_frames(frames, line, h, pitch, off, stride, np.random.default_rng(2))
    assert np.array_equal(c[inside], d[inside]) and np.array_equal(c[inside], a[inside])
    outside = int((~inside).sum())
    assert outside >= pl.SLACK + off
    # two independent uniform bytes coincide with probability 1 / 256: over `outside` bytes more than 1 / 256 + 5 sigma of them would be no chance
    same = int((c[~inside] == d[~inside]).sum())
    assert same <= outside / 256 + 5 * (outside / 256) ** 0.5, (same, outside)
    assert len(set(c[~inside].tolist())) > 64   # random, not a constant
