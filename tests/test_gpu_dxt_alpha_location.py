"""GPU parity on content built for the seam of the alpha stage's location form (dxt_encode.hip, encode_dxt5ycocg): from a 4:2:2 source the
DXT5-YCoCg encoder takes the 3-bit alpha count of a pixel from RN(7 u), u its location between the ends, where 7 u stays more than eps away
from a half-integer for every pixel of the block, and a wave that holds an uncertified block forms the thresholds and evaluates the
reference's comparison for every pixel.  UYVY and v210 -> DXT5-YCoCg, both tie rules, byte for byte against the oracle, at 512 x 32 and
510 x 30, on frames whose blocks are chosen with the CPU model of tests/test_dxt_alpha_location_bound.py:
  near_thresholds   every wave holds a pixel within eps / 4 of a threshold, and each of the seven thresholds has such pixels on either side
                    of it: the counter of ug_hip_dxt_encode_stats_alpha (waves that went on to the thresholds) is every wave;
  decided_and_clamped  every pixel is at least 4 eps from every threshold, and pixels lie beyond both ends (u clamps at 0 and at 1): 0;
  midpoint          flat chroma, three luma levels with the middle one halfway, which puts a pixel ON the middle threshold: every wave;
  range_below_2^-10  the wave test in front of the stage fails everywhere: the counter is 0 and counts[1] every wave, as before.
The factor 4 on either side keeps what is asserted independent of how the GPU's fma and reciprocal and the model's round.  The seam frames
of the pair location (tests/test_gpu_dxt_pair_zone.py) and the frames of the projection (tests/test_gpu_dxt_pair_projection.py) go through
as well; counts[0..3] of ug_hip_dxt_encode_stats_ex must be what the library returned before the alpha stage had this form (PARENT_COUNTS,
taken by running these frames through that library once), and the build that forces the linear count (libug_mi355x_alphalinear.so) gives the
same bytes with the counter at 0."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dxt_alpha_location_bound import frame_midpoint, frame_narrow, location_stage, margins, waves_of  # noqa: E402
from test_gpu_dxt_pair_cov import PLACED, SIZES, pack_uyvy, pack_v210, planes, wave_evaluations  # noqa: E402
from test_gpu_dxt_pair_projection import FRAMES as PROJECTION_FRAMES  # noqa: E402
from test_gpu_dxt_pair_zone import frames_for  # noqa: E402

pytestmark = pytest.mark.gpu
D = np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS_FNS = ("ug_hip_abi_version", "ug_hip_dxt_encode_batch_ex", "ug_hip_dxt_encode_stats", "ug_hip_dxt_encode_stats_ex", "ug_hip_dxt_encode_stats_alpha")

# counts[0..3] of ug_hip_dxt_encode_stats_ex (colour full form, alpha full form, exact covariance, per-pixel distances) of one ties-even
# encode of each frame below by the library as it was before this stage's location form: (frame, format, width, height) -> counts
PARENT_COUNTS = {
    ("near_thresholds", "UYVY", 512, 32): (0, 0, 0, 0), ("near_thresholds", "v210", 512, 32): (0, 0, 0, 0),
    ("decided_and_clamped", "UYVY", 512, 32): (0, 0, 1, 1), ("decided_and_clamped", "v210", 512, 32): (0, 0, 1, 1),
    ("midpoint", "UYVY", 512, 32): (0, 0, 16, 0), ("midpoint", "v210", 512, 32): (0, 0, 24, 0),
    ("range_below_2^-10", "UYVY", 512, 32): (0, 16, 0, 0), ("range_below_2^-10", "v210", 512, 32): (0, 24, 0, 0),
    ("sixths_extreme_luma", "UYVY", 512, 32): (0, 0, 0, 0), ("sixths_extreme_luma", "v210", 512, 32): (0, 0, 0, 0),
    ("sixths_exact_extreme_luma", "UYVY", 512, 32): (1, 0, 0, 1), ("sixths_exact_extreme_luma", "v210", 512, 32): (1, 0, 0, 1),
    ("short_segments_extreme_luma", "UYVY", 512, 32): (16, 0, 6, 0), ("short_segments_extreme_luma", "v210", 512, 32): (24, 0, 7, 0),
    ("short_segments_one_luma", "UYVY", 512, 32): (16, 16, 0, 0), ("short_segments_one_luma", "v210", 512, 32): (24, 24, 0, 0),
    ("flat_among_busy", "UYVY", 512, 32): (0, 15, 0, 0), ("flat_among_busy", "v210", 512, 32): (0, 19, 0, 0),
    ("one_chroma_extreme_luma_among_busy", "UYVY", 512, 32): (4, 15, 0, 0), ("one_chroma_extreme_luma_among_busy", "v210", 512, 32): (4, 19, 0, 0),
    ("projection_near_bisectors", "UYVY", 512, 32): (0, 0, 0, 16), ("projection_near_bisectors", "v210", 512, 32): (0, 0, 0, 24),
    ("projection_decided_and_clamped", "UYVY", 512, 32): (0, 14, 0, 0), ("projection_decided_and_clamped", "v210", 512, 32): (0, 19, 0, 0),
    ("projection_one_chroma_extreme_luma", "UYVY", 512, 32): (16, 0, 16, 0), ("projection_one_chroma_extreme_luma", "v210", 512, 32): (24, 0, 24, 0),
    ("near_thresholds", "UYVY", 510, 30): (0, 0, 0, 0), ("near_thresholds", "v210", 510, 30): (0, 0, 0, 0),
    ("decided_and_clamped", "UYVY", 510, 30): (0, 0, 0, 0), ("decided_and_clamped", "v210", 510, 30): (0, 0, 0, 0),
    ("midpoint", "UYVY", 510, 30): (0, 0, 16, 0), ("midpoint", "v210", 510, 30): (0, 0, 24, 0),
    ("range_below_2^-10", "UYVY", 510, 30): (0, 16, 0, 0), ("range_below_2^-10", "v210", 510, 30): (0, 24, 0, 0),
    ("sixths_extreme_luma", "UYVY", 510, 30): (4, 0, 0, 1), ("sixths_extreme_luma", "v210", 510, 30): (4, 0, 0, 2),
    ("sixths_exact_extreme_luma", "UYVY", 510, 30): (4, 0, 0, 1), ("sixths_exact_extreme_luma", "v210", 510, 30): (4, 0, 0, 0),
    ("short_segments_extreme_luma", "UYVY", 510, 30): (16, 0, 6, 0), ("short_segments_extreme_luma", "v210", 510, 30): (24, 0, 6, 0),
    ("short_segments_one_luma", "UYVY", 510, 30): (16, 16, 0, 0), ("short_segments_one_luma", "v210", 510, 30): (24, 23, 0, 0),
    ("flat_among_busy", "UYVY", 510, 30): (0, 11, 0, 0), ("flat_among_busy", "v210", 510, 30): (0, 16, 0, 0),
    ("one_chroma_extreme_luma_among_busy", "UYVY", 510, 30): (1, 11, 2, 0), ("one_chroma_extreme_luma_among_busy", "v210", 510, 30): (1, 16, 2, 0),
    ("projection_near_bisectors", "UYVY", 510, 30): (0, 0, 0, 16), ("projection_near_bisectors", "v210", 510, 30): (0, 0, 0, 24),
    ("projection_decided_and_clamped", "UYVY", 510, 30): (0, 16, 0, 0), ("projection_decided_and_clamped", "v210", 510, 30): (0, 21, 0, 0),
    ("projection_one_chroma_extreme_luma", "UYVY", 510, 30): (16, 0, 16, 0), ("projection_one_chroma_extreme_luma", "v210", 510, 30): (24, 0, 24, 0),
}


def margin_over_eps(s):
    """per pixel: distance of 7 u to the nearest threshold over eps, as the larger and as the smaller of the fp32 and the float64 form"""
    m32, m64 = margins(s)
    eps = s["eps"].astype(D)[..., None]
    return np.maximum(m32, m64) / eps, np.minimum(m32, m64) / eps


@functools.lru_cache(maxsize=None)
def near_threshold_pool(po):
    """seeded search: blocks with a pixel within eps / 4 of a threshold.  The luma lattice of byte sources meets a threshold on its own only
    halfway between the ends (the inset moves every other one off it by 1 / 510), so the rest are chance meetings within some 2e-7 of luma:
    candidates are blocks of three kinds of chroma pair (Y0, Y1, U, V), screened with the location in float64, and the strict model has the
    word on the few that pass.  Rows 2, 3 of every block repeat row 1, as the last block row of a height = 2 mod 4 is read: one pool serves
    whole and cut blocks.  One block for each threshold m = 1 .. 7 (t = m - 1/2) and side of it -> (yb, ub, vb) of shape (14, 4, 4 | 2)"""
    rng = np.random.default_rng(6100)
    n = 1500000
    yy = rng.integers(30, 190, (n, 1, 1)) + rng.integers(0, 40, (n, 3, 2))    # (Y0, Y1) of the three kinds of pair
    uv = rng.integers(90, 150, (n, 1, 1)) + rng.integers(0, 16, (n, 3, 2))    # their (U, V)
    yl, cu, cv = 1.1643 * (yy / 255.0 - 0.0625), uv[..., 0:1] / 255.0 - 0.5, uv[..., 1:2] / 255.0 - 0.5
    a = (yl + ((1.7926 - 2 * 0.5328) * cv + (2.1124 - 2 * 0.2132) * cu) / 4.0).reshape(n, 6)   # (r + 2 g + b) / 4
    mn, mx = a.min(1), a.max(1)
    inset = (mx - mn) / 32.0 - (16.0 / 255.0) / 32.0
    mn, mx = np.clip(mn + inset, 0, 1), np.clip(mx - inset, 0, 1)
    t = np.clip(7.0 - (a - mn[:, None]) * 7.0 / (mx - mn)[:, None], 0.0, 7.0)
    near = (0.5 - np.abs(t - np.rint(t))).min(1) < (2.2e-6 + 5.7e-6 / (mx - mn)) / 4.0
    yy, uv = yy[near], uv[near]
    kinds = np.array([[0, 1], [2, 0], [2, 0], [2, 0]])   # the kind of pair at (row, pair of the row)
    yb, ub, vb = yy[:, kinds].reshape(-1, 4, 4), uv[:, kinds, 0], uv[:, kinds, 1]
    s = location_stage(po, *planes(yb[None], ub[None], vb[None], 4 * len(yb), 4))
    worst, _ = margin_over_eps(s)
    worst, wide, t64 = worst[0], s["wide"][0], s["t64"][0]
    t = np.take_along_axis(t64, worst.argmin(-1)[:, None], -1)[:, 0]
    ok = wide & (worst.min(-1) <= 0.25)
    picked = []
    for m in range(1, 8):
        for above in (False, True):
            at = np.flatnonzero(ok & (np.floor(t) == m - 1) & ((t > m - 0.5) if above else (t < m - 0.5)))
            assert len(at), (m, above, int(near.sum()))
            picked.append(at[0])
    return yb[picked], ub[picked], vb[picked]


def frame_near_thresholds(po, w, h):
    rng = np.random.default_rng(61 + w)
    bw, bh = (w + 3) // 4, (h + 3) // 4
    yb, ub, vb = rng.integers(0, 256, (bh, bw, 4, 4)), rng.integers(0, 256, (bh, bw, 4, 2)), rng.integers(0, 256, (bh, bw, 4, 2))
    at = np.zeros((bh, bw), bool); at[:, PLACED] = True
    n = 0
    for by in range(bh):
        py, pu, pv = near_threshold_pool(po)
        for bx in PLACED:
            yb[by, bx], ub[by, bx], vb[by, bx] = py[n % len(py)], pu[n % len(py)], pv[n % len(py)]
            n += 1
    y, u, v = planes(yb, ub, vb, w, h)
    s = location_stage(po, y, u, v)
    worst, _ = margin_over_eps(s)
    assert s["wide"].all() and (worst.min(-1)[at] <= 0.25).all(), float(worst.min(-1)[at].max())   # every wave reaches the stage and holds such a pixel
    t = s["t64"][(worst <= 0.25) & at[..., None]]
    for m in range(1, 8):   # each threshold, from either side
        assert ((np.floor(t) == m - 1) & (t < m - 0.5)).any() and ((np.floor(t) == m - 1) & (t > m - 0.5)).any(), m
    return y, u, v


def frame_decided_and_clamped(po, w, h):
    rng = np.random.default_rng(62 + w)
    bw, bh = (w + 3) // 4, (h + 3) // 4
    yb, ub, vb = rng.integers(0, 256, (bh, bw, 4, 4)), rng.integers(0, 256, (bh, bw, 4, 2)), rng.integers(0, 256, (bh, bw, 4, 2))
    for _ in range(50):
        y, u, v = planes(yb, ub, vb, w, h)
        s = location_stage(po, y, u, v)
        _, least = margin_over_eps(s)
        bad = ~(s["wide"] & (least.min(-1) >= 4.0))
        if not bad.any():
            break
        m = int(bad.sum())
        yb[bad], ub[bad], vb[bad] = rng.integers(0, 256, (m, 4, 4)), rng.integers(0, 256, (m, 4, 2)), rng.integers(0, 256, (m, 4, 2))
    assert not bad.any()
    below, above = (s["t32"] < 0) & (s["t64"] < 0), (s["t32"] > 1) & (s["t64"] > 7)
    assert below.sum() > 100 and above.sum() > 100, (int(below.sum()), int(above.sum()))   # u clamps at 0 and at 1
    return y, u, v


def frame_midpoint_everywhere(po, w, h):
    y, u, v = frame_midpoint(w, h)
    s = location_stage(po, y, u, v)
    worst, _ = margin_over_eps(s)
    assert s["wide"].all() and waves_of(worst.min(-1) <= 0.25, False).any(-1).all()   # every wave holds a pixel within eps / 4
    return y, u, v


def frame_range_below(po, w, h):
    y, u, v = frame_narrow(w, h, True)
    assert not location_stage(po, y, u, v)["wide"].any()
    return y, u, v


FRAMES = {"near_thresholds": (frame_near_thresholds, "all"), "decided_and_clamped": (frame_decided_and_clamped, "none"),
          "midpoint": (frame_midpoint_everywhere, "all"), "range_below_2^-10": (frame_range_below, "none")}


def bound(path):
    """a build of the library bound for the calls below, as ultragrid_amd.lib binds the product"""
    from ultragrid_amd import lib as L
    so = C.CDLL(path)
    for fn in STATS_FNS:
        getattr(so, fn).restype, getattr(so, fn).argtypes = L.SYMBOLS[fn]
    assert so.ug_hip_abi_version() == L.ABI_VERSION
    return so


def linear_build():
    path = os.path.join(ROOT, "ultragrid_amd", "libug_mi355x_alphalinear.so")
    assert os.path.exists(path), "libug_mi355x_alphalinear.so is not built"
    return bound(path)


def encode(so, pf, src, w, h, ties, po):
    """-> (blocks, counts[0..3] and the alpha location's counter of this one encode)"""
    import torch
    from ultragrid_amd import lib as L
    dev = torch.from_numpy(np.ascontiguousarray(src, dtype=np.uint8)).cuda()
    dst = torch.zeros(po.dxt_size(po.OUT_DXT5YCOCG, w, h), dtype=torch.uint8, device="cuda")
    st, alpha = (C.c_ulonglong * 4)(), C.c_ulonglong(0)
    assert so.ug_hip_dxt_encode_stats_ex(None, 0, 1) == 0
    rc = so.ug_hip_dxt_encode_batch_ex(pf, L.DXT5_YCOCG, dev.data_ptr(), dst.data_ptr(), w, h, 0, 1, 0, 0, ties, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert so.ug_hip_dxt_encode_stats_ex(st, 4, 0) == 0 and so.ug_hip_dxt_encode_stats_alpha(C.byref(alpha), 1) == 0
    return dst.cpu().numpy(), tuple(int(x) for x in st) + (int(alpha.value),)


def run_frame(po, name, y, u, v, w, h):
    """both formats, both tie rules, the product and the linear build against the oracle -> ({format: counts of the product's ties-even
    encode}, complaints)"""
    from ultragrid_amd import lib as L
    product, linear = L.load(), linear_build()
    low = np.random.default_rng(99 + w).integers(0, 4, (h, 2 * w)).astype(np.uint32)
    srcs = {"UYVY": (L.PF_UYVY, po.IN_UYVY, pack_uyvy(y, u, v)), "v210": (L.PF_V210, po.IN_V210, pack_v210(y, u, v, low))}
    bad, counts = [], {}
    for fmt, (pf, pin, src) in srcs.items():
        for ties, tname in ((L.TIES_EVEN, "even"), (L.TIES_AWAY, "away")):
            want = po.dxt_encode(pin, po.OUT_DXT5YCOCG, src, w, h, ties=tname)
            got, st = encode(product, pf, src, w, h, ties, po)
            if not np.array_equal(got, want):
                bad.append((name, fmt, tname, "product", int(np.count_nonzero(got != want))))
            if ties == L.TIES_EVEN:
                counts[fmt] = st
                print(f"{name} {fmt} {w}x{h}: colour full form {st[0]}, alpha full form {st[1]}, exact covariance {st[2]}, per-pixel distances {st[3]}, "
                      f"alpha thresholds {st[4]} of {wave_evaluations(fmt, w, h)} waves")
            elif st[4] != counts[fmt][4]:   # the same waves under the other tie rule
                bad.append((name, fmt, "alpha threshold waves under ties even / away", counts[fmt][4], st[4]))
            got, st = encode(linear, pf, src, w, h, ties, po)
            if not np.array_equal(got, want):
                bad.append((name, fmt, tname, "alphalinear", int(np.count_nonzero(got != want))))
            if st[4] != 0:
                bad.append((name, fmt, tname, "alphalinear counts alpha threshold waves", st[4]))
    return counts, bad


def moved_counts(name, counts, w, h):
    return {(name, fmt): (st[:4], PARENT_COUNTS.get((name, fmt, w, h))) for fmt, st in counts.items() if st[:4] != PARENT_COUNTS.get((name, fmt, w, h))}


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(FRAMES))
def test_location_form_on_its_seam(hip, po, name, size):
    w, h = size
    build, expect = FRAMES[name]
    counts, bad = run_frame(po, name, *build(po, w, h), w, h)
    assert not bad, bad
    for fmt, st in counts.items():
        assert st[4] == (wave_evaluations(fmt, w, h) if expect == "all" else 0), (fmt, st, wave_evaluations(fmt, w, h))
        if name == "range_below_2^-10":
            assert st[1] == wave_evaluations(fmt, w, h), (fmt, st)   # every wave at the explicit monotonicity check, as before
    moved = moved_counts(name, counts, w, h)
    assert not moved, f"counts[0..3] (now, the parent's): {moved}"


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_seam_frames_of_the_pair_location_keep_the_parents_counts(hip, po, size):
    w, h = size
    bad, moved = [], {}
    for name, (y, u, v) in frames_for(w, h).items():
        counts, b = run_frame(po, name, y, u, v, w, h)
        bad += b
        moved.update(moved_counts(name, counts, w, h))
    assert not bad, bad
    assert not moved, f"counts[0..3] (now, the parent's): {moved}"


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_frames_of_the_projection_keep_the_parents_counts(hip, po, size):
    w, h = size
    bad, moved = [], {}
    for name, (build, _) in PROJECTION_FRAMES.items():
        counts, b = run_frame(po, "projection_" + name, *build(po, w, h), w, h)
        bad += b
        moved.update(moved_counts("projection_" + name, counts, w, h))
    assert not bad, bad
    assert not moved, f"counts[0..3] (now, the parent's): {moved}"


def test_alpha_counter_and_its_resets(hip, po):
    from ultragrid_amd import lib as L
    l = L.load()
    w, h = SIZES[0]
    src = pack_uyvy(*frame_midpoint_everywhere(po, w, h))
    every = wave_evaluations("UYVY", w, h)
    st, two, alpha = (C.c_ulonglong * 4)(), (C.c_ulonglong * 2)(), C.c_ulonglong(7)

    def count_after_encode():
        import torch
        dev = torch.from_numpy(src).cuda()
        dst = torch.zeros(po.dxt_size(po.OUT_DXT5YCOCG, w, h), dtype=torch.uint8, device="cuda")
        assert l.ug_hip_dxt_encode_batch_ex(L.PF_UYVY, L.DXT5_YCOCG, dev.data_ptr(), dst.data_ptr(), w, h, 0, 1, 0, 0, L.TIES_EVEN, torch.cuda.current_stream().cuda_stream) == 0
        assert l.ug_hip_dxt_encode_stats_alpha(C.byref(alpha), 0) == 0
        return int(alpha.value)
    assert l.ug_hip_dxt_encode_stats_alpha(None, 1) == 0 and l.ug_hip_dxt_encode_stats_alpha(C.byref(alpha), 0) == 0 and alpha.value == 0
    assert count_after_encode() == every and count_after_encode() == 2 * every   # it accumulates until a reset
    assert l.ug_hip_dxt_encode_stats(two, 1) == 0 and l.ug_hip_dxt_encode_stats_alpha(C.byref(alpha), 0) == 0 and alpha.value == 0
    assert count_after_encode() == every
    assert l.ug_hip_dxt_encode_stats_ex(st, 4, 1) == 0 and l.ug_hip_dxt_encode_stats_alpha(C.byref(alpha), 0) == 0 and alpha.value == 0
    assert count_after_encode() == every
    assert l.ug_hip_dxt_encode_stats_alpha(C.byref(alpha), 1) == 0 and alpha.value == every   # its own reset returns the count, then clears all five
    assert l.ug_hip_dxt_encode_stats_alpha(C.byref(alpha), 0) == 0 and alpha.value == 0
    assert l.ug_hip_dxt_encode_stats_ex(st, 4, 0) == 0 and [int(x) for x in st] == [0, 0, 0, 0]
