"""GPU parity on content built for the seam of the colour stage's linear form (dxt_encode.hip, encode_dxt5ycocg): from a 4:2:2 source the
DXT5-YCoCg encoder takes the open comparison of a chroma pair from the sign of one linear form of its even pixel where an error bound decides
it for both pixels, and a wave that holds an undecided block evaluates the reference's two distances for every pixel.  UYVY and v210 ->
DXT5-YCoCg, both tie rules, byte for byte against the oracle, on three frames per size whose blocks are chosen with the CPU model of tests/test_dxt_pair_linear_bound.py: a pair next to its
bisector in every wave, every pair decided or the block flat, one chroma sample per block under extreme lumas (the stage is not reached) --
and the counter of waves that went on to the per-pixel distances (counts[3] of ug_hip_dxt_encode_stats_ex) must be all of them, none,
none.  The frames keep a factor 4 from the certificate's threshold on either side, so what is asserted does not depend on how the GPU's
fma, reciprocal and square root and the model's round.  The six seam frames of tests/test_gpu_dxt_pair_zone.py go through as well."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dxt_pair_linear_bound import colour_stage  # noqa: E402
from test_gpu_dxt_pair_cov import ENDS, PLACED, SIZES, frame_one_chroma, pack_uyvy, pack_v210, planes, wave_evaluations  # noqa: E402
from test_gpu_dxt_pair_zone import frames_for  # noqa: E402

pytestmark = pytest.mark.gpu


def least_over_eps(s):
    """per block: the least |L| of its eight pairs over eps, as the larger and as the smaller of the fp32 and the float64 form"""
    with np.errstate(divide="ignore", invalid="ignore"):
        r32 = np.abs(s["L32"].astype(np.float64)).min(-1) / s["eps"]
        r64 = np.abs(s["L64"]).min(-1) / s["eps"]
    return np.maximum(r32, r64), np.minimum(r32, r64)


@functools.lru_cache(maxsize=None)
def near_bisector_pool(po, cut_rows, want=6):
    """seeded search: blocks whose eight (U, V) samples lie 0..11 byte steps from a base value, under extreme lumas, inside the stage's
    precondition, not flat, with a pair whose |L| <= eps / 4.  cut_rows: rows 2, 3 repeat row 1 (the last block row of a height = 2 mod 4
    is read that way).  -> (yb, ub, vb) of shape (want, 4, 4 | 2)"""
    rng = np.random.default_rng(2711 + cut_rows)
    bh, bw = 128, 512
    uv = rng.integers(8, 236, (bh, bw, 1, 1, 2)) + rng.integers(0, 12, (bh, bw, 4, 2, 2))
    yb = ENDS[rng.integers(0, 4, (bh, bw, 4, 2))].reshape(bh, bw, 4, 4)
    if cut_rows:
        uv[:, :, 2:] = uv[:, :, 1:2]
        yb[:, :, 2:] = yb[:, :, 1:2]
    s = colour_stage(po, *planes(yb, uv[..., 0], uv[..., 1], 4 * bw, 4 * bh))
    worst, _ = least_over_eps(s)
    ok = s["pre"] & ~s["flat"] & (worst <= 0.25)
    at = np.argwhere(ok)
    assert len(at) >= want, len(at)
    at = at[np.argsort(worst[ok], kind="stable")[:want]]
    return yb[at[:, 0], at[:, 1]], uv[at[:, 0], at[:, 1], ..., 0], uv[at[:, 0], at[:, 1], ..., 1]


def frame_near_bisector(po, w, h):
    rng = np.random.default_rng(41 + w)
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
        s = colour_stage(po, y, u, v)
        bad = ~s["pre"] & ~at   # every wave has to reach the linear form: no block outside the stage's precondition
        if not bad.any():
            break
        m = int(bad.sum())
        yb[bad], ub[bad], vb[bad] = rng.integers(0, 256, (m, 4, 4)), rng.integers(0, 256, (m, 4, 2)), rng.integers(0, 256, (m, 4, 2))
    worst, _ = least_over_eps(s)
    assert s["pre"].all() and not s["flat"][at].any() and (worst[at] <= 0.25).all(), float(worst[at].max())
    return y, u, v


def frame_decided(po, w, h):
    rng = np.random.default_rng(42 + w)
    bw, bh = (w + 3) // 4, (h + 3) // 4
    yb, ub, vb = rng.integers(0, 256, (bh, bw, 4, 4)), rng.integers(0, 256, (bh, bw, 4, 2)), rng.integers(0, 256, (bh, bw, 4, 2))
    flat = np.arange(bh * bw).reshape(bh, bw) % 5 == 2   # wholly flat blocks: one Y, U, V
    for p in (yb, ub, vb):
        p[flat] = rng.integers(0, 256, (int(flat.sum()), 1, 1))
    for _ in range(50):
        y, u, v = planes(yb, ub, vb, w, h)
        s = colour_stage(po, y, u, v)
        _, least = least_over_eps(s)
        bad = ~(s["pre"] & ((least >= 4.0) | s["flat"]))
        if not bad.any():
            break
        m = int(bad.sum())
        yb[bad], ub[bad], vb[bad] = rng.integers(0, 256, (m, 4, 4)), rng.integers(0, 256, (m, 4, 2)), rng.integers(0, 256, (m, 4, 2))
    assert not bad.any() and s["flat"][flat].all()
    return y, u, v


def waves_inside(pre, fmt):
    """number of waves all of whose blocks are inside the stage's precondition (pre: (bh, bw) per block): UYVY has one block per lane, 64
    consecutive blocks to a wave; v210 three per lane, a wave passes the stage once for block k = 0, 1, 2 of its lanes: columns k, k + 3, ..."""
    cols = [pre] if fmt == "UYVY" else [pre[:, k::3] for k in range(3)]
    n = 0
    for c in cols:
        c = np.concatenate([c, np.ones((c.shape[0], (-c.shape[1]) % 64), bool)], axis=1).reshape(c.shape[0], -1, 64)
        n += int(c.all(-1).sum())
    return n


def frame_one_chroma_unreached(po, w, h):
    """ONE chroma sample per block under extreme lumas: not flat, and the end points of most blocks coincide -- every wave holds such a
    block, so none reaches the fast colour stage"""
    y, u, v = frame_one_chroma(w, h)
    s = colour_stage(po, y, u, v)
    assert not s["flat"].any() and waves_inside(s["pre"], "UYVY") == 0 and waves_inside(s["pre"], "v210") == 0
    return y, u, v


FRAMES = {"near_bisector": (frame_near_bisector, "all"), "decided": (frame_decided, "none"), "one_chroma_extreme_luma": (frame_one_chroma_unreached, "none")}


def encode(so, pf, src, w, h, ties, po, reset=True):
    """-> (blocks, the four counters of this one encode)"""
    import torch
    from ultragrid_amd import lib as L
    dev = torch.from_numpy(np.ascontiguousarray(src, dtype=np.uint8)).cuda()
    dst = torch.zeros(po.dxt_size(po.OUT_DXT5YCOCG, w, h), dtype=torch.uint8, device="cuda")
    st = (C.c_ulonglong * 4)()
    assert so.ug_hip_dxt_encode_stats_ex(None, 0, 1) == 0
    rc = so.ug_hip_dxt_encode_batch_ex(pf, L.DXT5_YCOCG, dev.data_ptr(), dst.data_ptr(), w, h, 0, 1, 0, 0, ties, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert so.ug_hip_dxt_encode_stats_ex(st, 4, 1 if reset else 0) == 0
    return dst.cpu().numpy(), tuple(int(x) for x in st)


def run_frame(po, name, y, u, v, w, h):
    """both formats, both tie rules, the product against the oracle -> ({format: counts of the ties-even encode}, complaints)"""
    from ultragrid_amd import lib as L
    product = L.load()
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
                print(f"{name} {fmt} {w}x{h}: colour full form {st[0]}, alpha full form {st[1]}, exact covariance {st[2]}, "
                      f"per-pixel distances {st[3]} of {wave_evaluations(fmt, w, h)} waves")
            elif st[3] != counts[fmt][3]:   # the same waves under the other tie rule
                bad.append((name, fmt, "per-pixel distance waves under ties even / away", counts[fmt][3], st[3]))
    return counts, bad


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(FRAMES))
def test_linear_form_on_its_seam(hip, po, name, size):
    w, h = size
    build, expect = FRAMES[name]
    counts, bad = run_frame(po, name, *build(po, w, h), w, h)
    assert not bad, bad
    for fmt, st in counts.items():
        assert st[3] == (wave_evaluations(fmt, w, h) if expect == "all" else 0), (fmt, st, wave_evaluations(fmt, w, h))
        if name == "one_chroma_extreme_luma":
            assert st[0] == wave_evaluations(fmt, w, h), (fmt, st)   # every wave in the full form


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_seam_frames_of_the_pair_location(hip, po, size):
    w, h = size
    bad = []
    for name, (y, u, v) in frames_for(w, h).items():
        bad += run_frame(po, name, y, u, v, w, h)[1]
    assert not bad, bad


def test_fourth_counter_and_its_resets(hip, po):
    import torch  # noqa: F401
    from ultragrid_amd import lib as L
    l = L.load()
    w, h = SIZES[0]
    src = pack_uyvy(*frame_near_bisector(po, w, h))
    st, two = (C.c_ulonglong * 5)(), (C.c_ulonglong * 2)()
    assert l.ug_hip_dxt_encode_stats_ex(st, 5, 0) != 0   # n = 5 is refused, n = 4 accepted
    _, first = encode(l, L.PF_UYVY, src, w, h, L.TIES_EVEN, po, reset=False)
    assert first[3] == wave_evaluations("UYVY", w, h)
    assert l.ug_hip_dxt_encode_stats(two, 1) == 0 and l.ug_hip_dxt_encode_stats_ex(st, 4, 0) == 0 and int(st[3]) == 0   # the older reset clears it
    _, again = encode(l, L.PF_UYVY, src, w, h, L.TIES_EVEN, po, reset=True)
    assert again == first
    assert l.ug_hip_dxt_encode_stats_ex(st, 4, 0) == 0 and [int(x) for x in st[:4]] == [0, 0, 0, 0]   # and so does this one
