"""GPU parity for the difference domain of the DXT5-YCoCg encoder's chroma-pair side (dxt_encode.hip, encode_dxt5ycocg): from a 4:2:2
source the pixels stay (4 Y, r - b, 2 g - r - b), the box ends go through the two monotone maps to Co / Cg, the diagonal's rough sum and the
colour stage's projection take the differences as they are, and only the reference-form sides form Co / Cg per pixel.  UYVY and v210 ->
DXT5-YCoCg at 512 x 32 and 510 x 30 (the EDGE instantiation), both tie rules, the product and the build that forces the linear alpha count,
byte for byte against the oracle, on
  co_flat_*         blocks whose Co is exactly flat while r - b is not, with a negative rough sum (found by enumeration,
                    tests/test_dxt_pair_difference_bound.py): in every lane, and among blocks the diagonal's certificate decides.  (Their Cg
                    spread is of rounding size too, and exchanged Cg ends quantise to the same codes on every such block looked at: these
                    frames take the lanes through the rule `swap = rough < 0 and hx != 0`, the CPU model is what asserts its ends);
  the seam frames of the pair location, the frames tests/test_gpu_dxt_pair_projection.py and tests/test_gpu_dxt_pair_cov.py build on either
  side of their certificates (one chroma sample per block under extreme lumas among them: the full form);
  all_flat          one (Y, U, V) per block.
counts[0..2] of ug_hip_dxt_encode_stats_ex and the alpha counter must be what the library returned BEFORE the difference domain
(PARENT_COUNTS: these frames through that library, once); counts[3] is pinned on the frames that keep a factor 4 from the projection's
certificate on either side, and printed for the others: the location rounds differently, so a pair next to the certificate's edge may fall
on its other side.  One frame goes through the vertically mirrored encode as well."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dxt_pair_difference_bound import block_values, co_flat_blocks, co_flat_planes, diagonal_model  # noqa: E402
from test_gpu_dxt_alpha_location import run_frame  # noqa: E402
from test_gpu_dxt_pair_cov import FRAMES as COV_FRAMES, PLACED, SIZES, frame_decided, pack_uyvy, pack_v210, wave_evaluations  # noqa: E402
from test_gpu_dxt_pair_projection import FRAMES as PROJECTION_FRAMES  # noqa: E402
from test_gpu_dxt_pair_zone import frames_for  # noqa: E402

pytestmark = pytest.mark.gpu

# (colour full form, alpha full form, exact covariance, per-pixel distances, alpha thresholds) waves of one ties-even encode of each frame
# by the library as it was before the difference domain: (frame, format, width, height) -> counts
PARENT_COUNTS = {
    ("co_flat_everywhere", "UYVY", 512, 32): (16, 16, 0, 0, 0),
    ("co_flat_everywhere", "v210", 512, 32): (24, 24, 0, 0, 0),
    ("co_flat_among_decided", "UYVY", 512, 32): (16, 16, 0, 0, 0),
    ("co_flat_among_decided", "v210", 512, 32): (24, 24, 0, 0, 0),
    ("all_flat", "UYVY", 512, 32): (0, 16, 0, 0, 0),
    ("all_flat", "v210", 512, 32): (0, 24, 0, 0, 0),
    ("co_flat_everywhere", "UYVY", 510, 30): (16, 16, 0, 0, 0),
    ("co_flat_everywhere", "v210", 510, 30): (24, 24, 0, 0, 0),
    ("co_flat_among_decided", "UYVY", 510, 30): (16, 16, 0, 0, 0),
    ("co_flat_among_decided", "v210", 510, 30): (24, 21, 0, 0, 3),
    ("all_flat", "UYVY", 510, 30): (0, 16, 0, 0, 0),
    ("all_flat", "v210", 510, 30): (0, 24, 0, 0, 0),
    ("sixths_extreme_luma", "UYVY", 512, 32): (0, 0, 0, 0, 1),
    ("sixths_extreme_luma", "v210", 512, 32): (0, 0, 0, 0, 1),
    ("sixths_exact_extreme_luma", "UYVY", 512, 32): (1, 0, 0, 1, 0),
    ("sixths_exact_extreme_luma", "v210", 512, 32): (1, 0, 0, 1, 0),
    ("short_segments_extreme_luma", "UYVY", 512, 32): (16, 0, 6, 0, 0),
    ("short_segments_extreme_luma", "v210", 512, 32): (24, 0, 7, 0, 0),
    ("short_segments_one_luma", "UYVY", 512, 32): (16, 16, 0, 0, 0),
    ("short_segments_one_luma", "v210", 512, 32): (24, 24, 0, 0, 0),
    ("flat_among_busy", "UYVY", 512, 32): (0, 15, 0, 0, 1),
    ("flat_among_busy", "v210", 512, 32): (0, 19, 0, 0, 5),
    ("one_chroma_extreme_luma_among_busy", "UYVY", 512, 32): (4, 15, 0, 0, 1),
    ("one_chroma_extreme_luma_among_busy", "v210", 512, 32): (4, 19, 0, 0, 5),
    ("sixths_extreme_luma", "UYVY", 510, 30): (4, 0, 0, 1, 0),
    ("sixths_extreme_luma", "v210", 510, 30): (4, 0, 0, 2, 0),
    ("sixths_exact_extreme_luma", "UYVY", 510, 30): (4, 0, 0, 1, 0),
    ("sixths_exact_extreme_luma", "v210", 510, 30): (4, 0, 0, 0, 0),
    ("short_segments_extreme_luma", "UYVY", 510, 30): (16, 0, 6, 0, 0),
    ("short_segments_extreme_luma", "v210", 510, 30): (24, 0, 6, 0, 0),
    ("short_segments_one_luma", "UYVY", 510, 30): (16, 16, 0, 0, 0),
    ("short_segments_one_luma", "v210", 510, 30): (24, 23, 0, 0, 1),
    ("flat_among_busy", "UYVY", 510, 30): (0, 11, 0, 0, 5),
    ("flat_among_busy", "v210", 510, 30): (0, 16, 0, 0, 8),
    ("one_chroma_extreme_luma_among_busy", "UYVY", 510, 30): (1, 11, 2, 0, 5),
    ("one_chroma_extreme_luma_among_busy", "v210", 510, 30): (1, 16, 2, 0, 8),
    ("projection_near_bisectors", "UYVY", 512, 32): (0, 0, 0, 16, 0),
    ("projection_near_bisectors", "v210", 512, 32): (0, 0, 0, 24, 0),
    ("projection_decided_and_clamped", "UYVY", 512, 32): (0, 14, 0, 0, 2),
    ("projection_decided_and_clamped", "v210", 512, 32): (0, 19, 0, 0, 5),
    ("projection_one_chroma_extreme_luma", "UYVY", 512, 32): (16, 0, 16, 0, 0),
    ("projection_one_chroma_extreme_luma", "v210", 512, 32): (24, 0, 24, 0, 0),
    ("projection_near_bisectors", "UYVY", 510, 30): (0, 0, 0, 16, 0),
    ("projection_near_bisectors", "v210", 510, 30): (0, 0, 0, 24, 0),
    ("projection_decided_and_clamped", "UYVY", 510, 30): (0, 16, 0, 0, 0),
    ("projection_decided_and_clamped", "v210", 510, 30): (0, 21, 0, 0, 3),
    ("projection_one_chroma_extreme_luma", "UYVY", 510, 30): (16, 0, 16, 0, 0),
    ("projection_one_chroma_extreme_luma", "v210", 510, 30): (24, 0, 24, 0, 0),
    ("cov_near_zero", "UYVY", 512, 32): (8, 0, 16, 0, 0),
    ("cov_near_zero", "v210", 512, 32): (8, 0, 24, 0, 0),
    ("cov_decided", "UYVY", 512, 32): (0, 16, 0, 0, 0),
    ("cov_decided", "v210", 512, 32): (0, 22, 0, 0, 2),
    ("cov_one_chroma_extreme_luma", "UYVY", 512, 32): (16, 0, 16, 0, 0),
    ("cov_one_chroma_extreme_luma", "v210", 512, 32): (24, 0, 24, 0, 0),
    ("cov_near_zero", "UYVY", 510, 30): (9, 0, 16, 0, 1),
    ("cov_near_zero", "v210", 510, 30): (8, 0, 24, 0, 1),
    ("cov_decided", "UYVY", 510, 30): (0, 15, 0, 0, 1),
    ("cov_decided", "v210", 510, 30): (0, 18, 0, 0, 6),
    ("cov_one_chroma_extreme_luma", "UYVY", 510, 30): (16, 0, 16, 0, 0),
    ("cov_one_chroma_extreme_luma", "v210", 510, 30): (24, 0, 24, 0, 0),
}
PINNED_3 = ("projection_near_bisectors", "projection_decided_and_clamped")   # a factor 4 from the projection's certificate on either side


def frame_co_flat_everywhere(w, h):
    _, _, rows = co_flat_blocks()
    bw, bh = (w + 3) // 4, (h + 3) // 4
    y, u, v = co_flat_planes(rows, bw, bh)
    d, e, _, _ = block_values(y, u, v)
    m = diagonal_model(d, e)
    assert (m["hx"] == 0).all() and (d.max(-1) > d.min(-1)).all() and m["swap_without_rule"].all() and not m["swap"].any()
    return y[:h, :w], u[:h, : w // 2], v[:h, : w // 2]


def frame_co_flat_among_decided(w, h):
    """the blocks above at PLACED among blocks at least a factor 4 inside the diagonal's certificate: no wave forms the exact sum, so the
    lanes of the Co-flat blocks take the rule and their neighbours the sign of rough"""
    _, _, rows = co_flat_blocks()
    y, u, v = (p.copy() for p in frame_decided(w, h))
    n = 0
    for by in range((h + 3) // 4):
        for bx in PLACED:
            fy, fu, fv = co_flat_planes(rows[n % len(rows)][None], 1, 1)
            rows_here = y[4 * by:4 * by + 4].shape[0]
            y[4 * by:4 * by + 4, 4 * bx:4 * bx + 4] = fy[:rows_here]
            u[4 * by:4 * by + 4, 2 * bx:2 * bx + 2] = fu[:rows_here]
            v[4 * by:4 * by + 4, 2 * bx:2 * bx + 2] = fv[:rows_here]
            n += 1
    d, e, _, _ = block_values(y, u, v)
    m = diagonal_model(d, e)
    at = np.zeros(m["hx"].shape, bool); at[:, PLACED] = True   # (the four lines of such a block are alike: the cut last block row holds it as well)
    assert (m["hx"][at] == 0).all() and m["swap_without_rule"][at].all() and not m["swap"][at].any() and m["certified"].all()
    return y, u, v


def frame_all_flat(w, h):
    rng = np.random.default_rng(77 + w)
    bw, bh = (w + 3) // 4, (h + 3) // 4
    up = lambda p, k: np.ascontiguousarray(np.repeat(np.repeat(p, 4, axis=0), k, axis=1).astype(np.uint8))
    yb, ub, vb = (rng.integers(0, 256, (bh, bw)) for _ in range(3))
    return up(yb, 4)[:h, :w], up(ub, 2)[:h, : w // 2], up(vb, 2)[:h, : w // 2]


def builders(po, w, h):
    """frame name -> a call that builds (y, u, v)"""
    out = {"co_flat_everywhere": lambda: frame_co_flat_everywhere(w, h), "co_flat_among_decided": lambda: frame_co_flat_among_decided(w, h),
           "all_flat": lambda: frame_all_flat(w, h)}
    out.update({name: (lambda name=name: frames_for(w, h)[name]) for name in GROUPS["pair_location_seams"]})
    out.update({"projection_" + name: (lambda build=build: build(po, w, h)) for name, (build, _) in PROJECTION_FRAMES.items()})
    out.update({"cov_" + name: (lambda build=build: build(w, h)) for name, (build, _) in COV_FRAMES.items()})
    return out


GROUPS = {"co_flat_and_flat": ("co_flat_everywhere", "co_flat_among_decided", "all_flat"),
          "pair_location_seams": ("sixths_extreme_luma", "sixths_exact_extreme_luma", "short_segments_extreme_luma", "short_segments_one_luma",
                                  "flat_among_busy", "one_chroma_extreme_luma_among_busy"),
          "projection": tuple("projection_" + n for n in PROJECTION_FRAMES), "diagonal": tuple("cov_" + n for n in COV_FRAMES)}


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("group", list(GROUPS))
def test_difference_domain_keeps_bytes_and_counters(hip, po, group, size):
    w, h = size
    build = builders(po, w, h)
    bad, moved = [], {}
    for name in GROUPS[group]:
        counts, b = run_frame(po, name, *build[name](), w, h)
        bad += b
        for fmt, st in counts.items():
            print(f'    ("{name}", "{fmt}", {w}, {h}): {st},')
            if name.startswith("co_flat"):   # what these frames are for: no wave forms the reference's covariance, the ends come from the rule
                assert st[2] == 0, (name, fmt, st)
            want = PARENT_COUNTS.get((name, fmt, w, h))
            keep = (0, 1, 2, 4) + ((3,) if name in PINNED_3 else ())
            if want is None or any(st[k] != want[k] for k in keep):
                moved[name, fmt] = (st, want)
    assert not bad, bad
    assert not moved, f"counts (now, the parent's): {moved}"


@pytest.mark.parametrize("fmt", ["UYVY", "v210"])
def test_vertical_mirror(hip, po, fmt):
    import torch
    from ultragrid_amd import lib as L
    w, h = SIZES[1]
    y, u, v = frame_co_flat_among_decided(w, h)
    low = np.random.default_rng(99 + w).integers(0, 4, (h, 2 * w)).astype(np.uint32)
    pf, pin, src = (L.PF_UYVY, po.IN_UYVY, pack_uyvy(y, u, v)) if fmt == "UYVY" else (L.PF_V210, po.IN_V210, pack_v210(y, u, v, low))
    for ties, tname in ((None, "even"), (L.TIES_AWAY, "away")):
        got = hip.dxt_encode(pf, L.DXT5_YCOCG, torch.from_numpy(src).cuda(), w, -h, ties=ties).cpu().numpy()
        assert np.array_equal(got, po.dxt_encode(pin, po.OUT_DXT5YCOCG, src, w, -h, ties=tname)), (fmt, tname)
    assert wave_evaluations(fmt, w, h) > 0
