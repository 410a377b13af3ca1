"""GPU parity on content built for the seam of the pair location (dxt_encode.hip, UG_DXT_PAIR_ZONE / UG_DXT_BITS_INDEX): the DXT5-YCoCg
colour stage finds the zone of a 4:2:2 pixel pair once, from the pair's even pixel, and reads the table row from float bits.
UYVY and v210 -> DXT5-YCoCg, both tie rules, byte for byte against the oracle; and which waves leave the fast stages
(ug_hip_dxt_encode_stats) must be what it was before the change -- the precondition is a property of the content."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [(512, 32), (510, 30)]   # two full waves per block row; w % 4 == 2 and h % 4 == 2: the EDGE instantiation, cut pair at the right edge

# (colour full form, alpha full form) waves of one ties-even encode of each frame, as the build BEFORE the pair location reported them
# for the same seeded frames (ug_hip_dxt_encode_stats; printed by this test before it asserts).  Colour counts of 0 and of > 0 both occur:
# the frames reach the fast colour stage with and without flat blocks, and the full form too.
PARENT_STATS = {
    ("sixths_extreme_luma", "UYVY", 512, 32): (0, 0),
    ("sixths_extreme_luma", "v210", 512, 32): (0, 0),
    ("sixths_exact_extreme_luma", "UYVY", 512, 32): (1, 0),
    ("sixths_exact_extreme_luma", "v210", 512, 32): (1, 0),
    ("short_segments_extreme_luma", "UYVY", 512, 32): (16, 0),
    ("short_segments_extreme_luma", "v210", 512, 32): (24, 0),
    ("short_segments_one_luma", "UYVY", 512, 32): (16, 16),
    ("short_segments_one_luma", "v210", 512, 32): (24, 24),
    ("flat_among_busy", "UYVY", 512, 32): (0, 15),
    ("flat_among_busy", "v210", 512, 32): (0, 19),
    ("one_chroma_extreme_luma_among_busy", "UYVY", 512, 32): (4, 15),
    ("one_chroma_extreme_luma_among_busy", "v210", 512, 32): (4, 19),
    ("sixths_extreme_luma", "UYVY", 510, 30): (4, 0),
    ("sixths_extreme_luma", "v210", 510, 30): (4, 0),
    ("sixths_exact_extreme_luma", "UYVY", 510, 30): (4, 0),
    ("sixths_exact_extreme_luma", "v210", 510, 30): (4, 0),
    ("short_segments_extreme_luma", "UYVY", 510, 30): (16, 0),
    ("short_segments_extreme_luma", "v210", 510, 30): (24, 0),
    ("short_segments_one_luma", "UYVY", 510, 30): (16, 16),
    ("short_segments_one_luma", "v210", 510, 30): (24, 23),
    ("flat_among_busy", "UYVY", 510, 30): (0, 11),
    ("flat_among_busy", "v210", 510, 30): (0, 16),
    ("one_chroma_extreme_luma_among_busy", "UYVY", 510, 30): (1, 11),
    ("one_chroma_extreme_luma_among_busy", "v210", 510, 30): (1, 16),
}


def pack_uyvy(y, u, v):
    """y: (h, w), u / v: (h, w / 2) bytes -> UYVY"""
    h, w = y.shape
    out = np.empty((h, w // 2, 4), np.uint8)
    out[..., 0] = u; out[..., 1] = y[:, 0::2]; out[..., 2] = v; out[..., 3] = y[:, 1::2]
    return out.ravel()


def pack_v210(y, u, v, low):
    """the same picture as 10-bit samples whose top 8 bits are the bytes (low: (h, 2 w) values 0..3, the bits the encoder drops)"""
    h, w = y.shape
    s = np.zeros((h, (2 * w + 11) // 12 * 12), np.uint32)   # U Y0 V Y1 ..., padded to whole 6-pixel groups
    s[:, 0:2 * w:4] = u; s[:, 1:2 * w:4] = y[:, 0::2]; s[:, 2:2 * w:4] = v; s[:, 3:2 * w:4] = y[:, 1::2]
    s[:, :2 * w] = s[:, :2 * w] << 2 | low
    words = s[:, 0::3] | (s[:, 1::3] << 10) | (s[:, 2::3] << 20)
    out = np.zeros((h, (w + 47) // 48 * 128 // 4), np.uint32)
    out[:, : words.shape[1]] = words
    return out.view(np.uint8).ravel()


def frames_for(w, h):
    """name -> (y, u, v): luma per pixel, chroma per horizontal pair, built block by block (blocks of 4 x 4 px = 4 x 2 chroma samples)"""
    rng = np.random.default_rng(4220 + w)
    bw, bh = (w + 3) // 4, (h + 3) // 4

    def planes(yb, ub, vb):  # (bh, bw, 4, 4), (bh, bw, 4, 2) x 2 -> pictures cut to w x h
        y = yb.transpose(0, 2, 1, 3).reshape(4 * bh, 4 * bw)[:h, :w]
        u = ub.transpose(0, 2, 1, 3).reshape(4 * bh, 2 * bw)[:h, : w // 2]
        v = vb.transpose(0, 2, 1, 3).reshape(4 * bh, 2 * bw)[:h, : w // 2]
        return tuple(np.ascontiguousarray(np.clip(p, 0, 255).astype(np.uint8)) for p in (y, u, v))

    def extreme_luma():
        """the two lumas of every pair at opposite extremes: the pair's Co / Cg differ as much as rounding lets them"""
        ends = np.array([[0, 255], [255, 0], [16, 235], [235, 16]])
        return ends[rng.integers(0, 4, (bh, bw, 4, 2))].reshape(bh, bw, 4, 4)

    out = {}
    # 1. chroma ON the palette segment at multiples of 1/6 of it (every zone border, every bisector), +- 1 LSB
    a = rng.integers(0, 256, (bh, bw, 1, 1, 2)).astype(np.float64)
    b = rng.integers(0, 256, (bh, bw, 1, 1, 2)).astype(np.float64)
    t = rng.integers(0, 7, (bh, bw, 4, 2, 1)) / 6.0
    uv = np.rint(a + (b - a) * t) + rng.integers(-1, 2, (bh, bw, 4, 2, 2))
    out["sixths_extreme_luma"] = planes(extreme_luma(), uv[..., 0], uv[..., 1])
    # the same without the +- 1: both end points are pixels, the others sit on the borders as exactly as bytes allow
    uv = np.rint(a + (b - a) * t)
    out["sixths_exact_extreme_luma"] = planes(extreme_luma(), uv[..., 0], uv[..., 1])
    # 2. short segments: two chroma values per block, 0..8 byte steps apart in U and in V (a 5-bit end point step is about 8 / scale bytes:
    #    from coincident end points over two chroma values, through the shortest non-zero segments, to a few steps -- the recorded counts
    #    below show both sides of the stage's precondition are met)
    base = rng.integers(8, 240, (bh, bw, 1, 1, 2))
    delta = rng.integers(0, 9, (bh, bw, 1, 1, 2))
    pick = rng.integers(0, 2, (bh, bw, 4, 2, 1))
    uv = base + delta * pick
    out["short_segments_extreme_luma"] = planes(extreme_luma(), uv[..., 0], uv[..., 1])
    out["short_segments_one_luma"] = planes(np.broadcast_to(rng.integers(16, 236, (bh, bw, 1, 1)), (bh, bw, 4, 4)), uv[..., 0], uv[..., 1])
    # 3. waves that mix flat blocks (one Y, U, V: coincident end points, full form for the one value inside the fast stage), blocks
    #    of ONE chroma sample under extreme lumas (Co / Cg differ by rounding only: not flat, end points coincide) and busy ones
    yb = rng.integers(0, 256, (bh, bw, 4, 4))
    ub = rng.integers(0, 256, (bh, bw, 4, 2)); vb = rng.integers(0, 256, (bh, bw, 4, 2))
    n = np.arange(bh * bw).reshape(bh, bw)
    flat = n % 7 == 3
    yb[flat] = rng.integers(0, 256, (int(flat.sum()), 1, 1)); ub[flat] = rng.integers(0, 256, (int(flat.sum()), 1, 1)); vb[flat] = rng.integers(0, 256, (int(flat.sum()), 1, 1))
    out["flat_among_busy"] = planes(yb, ub, vb)
    yb, ub, vb = yb.copy(), ub.copy(), vb.copy()
    one = (n % 67 == 5) & (n // bw % 2 == 0)   # rare: each one sends its whole wave to the full form
    yb[one] = extreme_luma()[one]; ub[one] = rng.integers(0, 256, (int(one.sum()), 1, 1)); vb[one] = rng.integers(0, 256, (int(one.sum()), 1, 1))
    out["one_chroma_extreme_luma_among_busy"] = planes(yb, ub, vb)
    return out


def sources(w, h):
    """(frame name, format name) -> packed bytes"""
    rng = np.random.default_rng(99 + w)
    out = {}
    for name, (y, u, v) in frames_for(w, h).items():
        out[name, "UYVY"] = pack_uyvy(y, u, v)
        out[name, "v210"] = pack_v210(y, u, v, rng.integers(0, 4, (h, 2 * w)).astype(np.uint32))
    return out


def stats_of(l, hip, pf, src, w, h):
    import torch
    from ultragrid_amd import lib as L
    st = (C.c_ulonglong * 2)()
    assert l.ug_hip_dxt_encode_stats(None, 1) == 0
    got = hip.dxt_encode(pf, L.DXT5_YCOCG, torch.from_numpy(src).cuda(), w, h).cpu().numpy()
    assert l.ug_hip_dxt_encode_stats(st, 1) == 0
    return got, (int(st[0]), int(st[1]))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pair_location_on_its_seams(hip, po, size):
    import torch
    from ultragrid_amd import lib as L
    l = L.load()
    w, h = size
    fmts = {"UYVY": (L.PF_UYVY, po.IN_UYVY), "v210": (L.PF_V210, po.IN_V210)}
    seen, bad = {}, []
    for (name, fmt), src in sources(w, h).items():
        pf, pin = fmts[fmt]
        got, st = stats_of(l, hip, pf, src, w, h)
        seen[name, fmt, w, h] = st
        print(f'    ("{name}", "{fmt}", {w}, {h}): {st},')
        want = po.dxt_encode(pin, po.OUT_DXT5YCOCG, src, w, h)
        if not np.array_equal(got, want):
            bad.append((name, fmt, "even", int(np.count_nonzero(got != want))))
        got = hip.dxt_encode(pf, L.DXT5_YCOCG, torch.from_numpy(src).cuda(), w, h, ties=L.TIES_AWAY).cpu().numpy()
        want = po.dxt_encode(pin, po.OUT_DXT5YCOCG, src, w, h, ties="away")
        if not np.array_equal(got, want):
            bad.append((name, fmt, "away", int(np.count_nonzero(got != want))))
    assert not bad, bad
    moved = {k: (v, PARENT_STATS.get(k)) for k, v in seen.items() if PARENT_STATS.get(k) != v}
    assert not moved, f"full-form wave counts (now, before the change): {moved}"

