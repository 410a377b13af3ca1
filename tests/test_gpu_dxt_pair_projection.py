"""GPU parity on content built for the seam of the colour stage's projection form (dxt_encode.hip, encode_dxt5ycocg): from a 4:2:2 source the
DXT5-YCoCg encoder takes the colour index of a chroma pair from the projection of its even pixel on the palette segment where 3 s stays more
than eps away from a half-integer, and a wave that holds an uncertified block evaluates the reference's two distances for every pixel.  UYVY
and v210 -> DXT5-YCoCg, both tie rules, byte for byte against the oracle, at 512 x 32 and 510 x 30, on frames whose blocks are chosen with
the CPU model of tests/test_dxt_pair_projection_bound.py:
  near_bisectors    every wave holds a pair within eps / 4 of a bisector, and each of the three bisectors (1/6, 1/2, 5/6 of the segment) has
                    such pairs on either side of it: counts[3] of ug_hip_dxt_encode_stats_ex (waves that went on to the per-pixel
                    distances) is every wave;
  decided_and_clamped  every pair is at least 4 eps from every bisector or its block is flat, and pixels lie beyond both ends of the
                    segment (s clamps at 0 and at 1): counts[3] is 0;
  one_chroma_extreme_luma  one chroma sample per block under extreme lumas: the stage is not reached, counts[3] is 0 and counts[0] every wave.
The factor 4 on either side keeps what is asserted independent of how the GPU's fma, reciprocal and square root and the model's round.  The
seam frames of the pair location (tests/test_gpu_dxt_pair_zone.py) and the frames of the diagonal stage (tests/test_gpu_dxt_pair_cov.py) go
through as well, and their counts[0..2] must be what the parent returned: the values those tests pin."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dxt_pair_projection_bound import margins, projection_stage  # noqa: E402
from test_gpu_dxt_pair_cov import ENDS, FRAMES as COV_FRAMES, PLACED, SIZES, planes, wave_evaluations  # noqa: E402
from test_gpu_dxt_pair_linear import frame_one_chroma_unreached, run_frame, waves_inside  # noqa: E402
from test_gpu_dxt_pair_zone import PARENT_STATS, frames_for  # noqa: E402

pytestmark = pytest.mark.gpu
D = np.float64


def margin_over_eps(s):
    """per pair: distance of 3 s to the nearest bisector over eps, as the larger and as the smaller of the fp32 and the float64 form"""
    m32, m64 = margins(s)
    with np.errstate(divide="ignore", invalid="ignore"):
        eps = s["eps"].astype(D)[..., None]
        return np.maximum(m32, m64) / eps, np.minimum(m32, m64) / eps


@functools.lru_cache(maxsize=None)
def near_bisector_pool(po, cut_rows):
    """seeded search: blocks whose eight (U, V) samples lie 0..11 byte steps from a base value, under extreme lumas, inside the stage's
    precondition, not flat, with a pair within eps / 4 of a bisector.  cut_rows: rows 2, 3 repeat row 1 (the last block row of a height = 2
    mod 4 is read that way).  One block for each bisector (3 s = 1/2, 3/2, 5/2) and side of it -> (yb, ub, vb) of shape (6, 4, 4 | 2)"""
    rng = np.random.default_rng(5171 + cut_rows)
    bh, bw = 256, 512
    uv = rng.integers(8, 236, (bh, bw, 1, 1, 2)) + rng.integers(0, 12, (bh, bw, 4, 2, 2))
    yb = ENDS[rng.integers(0, 4, (bh, bw, 4, 2))].reshape(bh, bw, 4, 4)
    if cut_rows:
        uv[:, :, 2:] = uv[:, :, 1:2]
        yb[:, :, 2:] = yb[:, :, 1:2]
    s = projection_stage(po, *planes(yb, uv[..., 0], uv[..., 1], 4 * bw, 4 * bh))
    worst, _ = margin_over_eps(s)
    at_pair = worst.argmin(-1)
    t = 3.0 * np.take_along_axis(s["t64"], at_pair[..., None], -1)[..., 0]
    ok = s["pre"] & ~s["flat"] & (worst.min(-1) <= 0.25)
    picked = []
    for k in range(3):
        for side in (False, True):
            with np.errstate(invalid="ignore"):
                at = np.argwhere(ok & (np.floor(t) == k) & ((t > k + 0.5) == side))
            assert len(at), (k, side)
            picked.append(at[0])
    at = np.array(picked)
    return yb[at[:, 0], at[:, 1]], uv[at[:, 0], at[:, 1], ..., 0], uv[at[:, 0], at[:, 1], ..., 1]


def frame_near_bisectors(po, w, h):
    rng = np.random.default_rng(43 + w)
    bw, bh = (w + 3) // 4, (h + 3) // 4
    yb, ub, vb = rng.integers(0, 256, (bh, bw, 4, 4)), rng.integers(0, 256, (bh, bw, 4, 2)), rng.integers(0, 256, (bh, bw, 4, 2))
    whole, cut = near_bisector_pool(po, False), near_bisector_pool(po, True)
    at = np.zeros((bh, bw), bool); at[:, PLACED] = True
    for _ in range(50):
        n = 0
        for by in range(bh):
            py, pu, pv = cut if (h % 4 and by == bh - 1) else whole
            for bx in PLACED:
                yb[by, bx], ub[by, bx], vb[by, bx] = py[n % len(py)], pu[n % len(py)], pv[n % len(py)]
                n += 1
        y, u, v = planes(yb, ub, vb, w, h)
        s = projection_stage(po, y, u, v)
        bad = ~s["pre"] & ~at   # every wave has to reach the stage: no block outside its precondition
        if not bad.any():
            break
        m = int(bad.sum())
        yb[bad], ub[bad], vb[bad] = rng.integers(0, 256, (m, 4, 4)), rng.integers(0, 256, (m, 4, 2)), rng.integers(0, 256, (m, 4, 2))
    worst, _ = margin_over_eps(s)
    assert s["pre"].all() and not s["flat"][at].any() and (worst.min(-1)[at] <= 0.25).all(), float(worst.min(-1)[at].max())
    t = 3.0 * s["t64"][(worst <= 0.25) & at[..., None]]
    for k in range(3):   # each bisector, from either side
        assert ((np.floor(t) == k) & (t < k + 0.5)).any() and ((np.floor(t) == k) & (t > k + 0.5)).any(), k
    return y, u, v


def frame_decided_and_clamped(po, w, h):
    rng = np.random.default_rng(44 + w)
    bw, bh = (w + 3) // 4, (h + 3) // 4
    yb, ub, vb = rng.integers(0, 256, (bh, bw, 4, 4)), rng.integers(0, 256, (bh, bw, 4, 2)), rng.integers(0, 256, (bh, bw, 4, 2))
    flat = np.arange(bh * bw).reshape(bh, bw) % 5 == 2   # wholly flat blocks: one Y, U, V
    for p in (yb, ub, vb):
        p[flat] = rng.integers(0, 256, (int(flat.sum()), 1, 1))
    for _ in range(50):
        y, u, v = planes(yb, ub, vb, w, h)
        s = projection_stage(po, y, u, v)
        _, least = margin_over_eps(s)
        bad = ~(s["pre"] & ((least.min(-1) >= 4.0) | s["flat"]))
        if not bad.any():
            break
        m = int(bad.sum())
        yb[bad], ub[bad], vb[bad] = rng.integers(0, 256, (m, 4, 4)), rng.integers(0, 256, (m, 4, 2)), rng.integers(0, 256, (m, 4, 2))
    assert not bad.any() and s["flat"][flat].all()
    live = ~s["flat"][..., None]
    below, above = live & (s["t32"] < 0) & (s["t64"] < 0), live & (s["t32"] > 1) & (s["t64"] > 1)
    assert below.sum() > 100 and above.sum() > 100, (int(below.sum()), int(above.sum()))   # s clamps at 0 and at 1, in most blocks
    return y, u, v


FRAMES = {"near_bisectors": (frame_near_bisectors, "all"), "decided_and_clamped": (frame_decided_and_clamped, "none"),
          "one_chroma_extreme_luma": (frame_one_chroma_unreached, "none")}


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(FRAMES))
def test_projection_form_on_its_seam(hip, po, name, size):
    w, h = size
    build, expect = FRAMES[name]
    y, u, v = build(po, w, h)
    if name != "one_chroma_extreme_luma":
        pre = projection_stage(po, y, u, v)["pre"]
        assert all(waves_inside(pre, fmt) == wave_evaluations(fmt, w, h) for fmt in ("UYVY", "v210"))
    counts, bad = run_frame(po, name, y, u, v, w, h)
    assert not bad, bad
    for fmt, st in counts.items():
        assert st[3] == (wave_evaluations(fmt, w, h) if expect == "all" else 0), (fmt, st, wave_evaluations(fmt, w, h))
        assert st[0] == (wave_evaluations(fmt, w, h) if name == "one_chroma_extreme_luma" else 0), (fmt, st)   # every wave in the full form, or none


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_seam_frames_of_the_pair_location_keep_the_parents_counts(hip, po, size):
    w, h = size
    bad, moved = [], {}
    for name, (y, u, v) in frames_for(w, h).items():
        counts, b = run_frame(po, name, y, u, v, w, h)
        bad += b
        for fmt, st in counts.items():
            if tuple(st[:2]) != tuple(PARENT_STATS[name, fmt, w, h]):
                moved[name, fmt] = (st, PARENT_STATS[name, fmt, w, h])
    assert not bad, bad
    assert not moved, f"full-form wave counts (now, the parent's): {moved}"


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_frames_of_the_diagonal_stage_keep_the_parents_counts(hip, po, size):
    w, h = size
    bad = []
    for name, (build, expect) in COV_FRAMES.items():
        counts, b = run_frame(po, name, *build(w, h), w, h)
        bad += b
        for fmt, st in counts.items():
            assert st[2] == (wave_evaluations(fmt, w, h) if expect == "all" else 0), (name, fmt, st)
    assert not bad, bad
