"""GPU parity on content built for the seam of the diagonal stage (dxt_encode.hip, UG_DXT_PAIR_COV): from a 4:2:2 source the DXT5-YCoCg
encoder takes the sign of SelectYCoCgDiagonal's covariance from one product per chroma pair where an error bound decides it, and a wave that
holds an undecided block forms the reference's 16-term sum.  UYVY and v210 -> DXT5-YCoCg, both tie rules, byte for byte against the oracle,
on three frames per size whose blocks are chosen with the CPU model of tests/test_dxt_pair_cov_bound.py: covariance next to zero in every
wave (both signs), decided everywhere, and chroma spreads of rounding size everywhere -- and the counter of waves that formed the exact sum
(ug_hip_dxt_encode_stats_ex) must be all of them, none, all of them.  The frames keep a factor 4 from the certificate's threshold on
either side, so what is asserted does not depend on how the GPU's fma and the model's round."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dxt_pair_cov_bound import diagonal_stage, eps_of  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(512, 32), (510, 30)]   # two full waves per block row; w % 4 == 2 and h % 4 == 2: the EDGE instantiation, cut pair at the right edge
PLACED = (0, 1, 2, 64, 65, 66)   # block columns that reach every wave of a block row: UYVY waves 0 and 1 (one block per lane), v210 blocks 0, 1, 2 of a lane
ENDS = np.array([[0, 255], [255, 0], [16, 235], [235, 16]])


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


def planes(yb, ub, vb, w, h):
    """blocks (bh, bw, 4, 4), (bh, bw, 4, 2) x 2 -> pictures cut to w x h"""
    bh, bw = yb.shape[:2]
    y = yb.transpose(0, 2, 1, 3).reshape(4 * bh, 4 * bw)[:h, :w]
    u = ub.transpose(0, 2, 1, 3).reshape(4 * bh, 2 * bw)[:h, : w // 2]
    v = vb.transpose(0, 2, 1, 3).reshape(4 * bh, 2 * bw)[:h, : w // 2]
    return tuple(np.ascontiguousarray(p.astype(np.uint8)) for p in (y, u, v))


def two_rough_over_eps(s):
    """max over the fp32 and the float64 accumulation of |2 rough| / eps per block (inf where eps == 0), and the same as a minimum"""
    eps = eps_of(s)
    with np.errstate(divide="ignore", invalid="ignore"):
        r32 = np.where(eps > 0, np.abs(2.0 * s["rough32"].astype(np.float64)) / eps, np.inf)
        r64 = np.where(eps > 0, np.abs(2.0 * s["rough64"]) / eps, np.inf)
    return np.maximum(r32, r64), np.minimum(r32, r64)


@functools.lru_cache(maxsize=None)
def near_zero_pool(cut_rows, want=6):
    """seeded search: blocks whose eight (U, V) samples lie 0..3 byte steps from a base value, under extreme lumas, with hx hy > 0 and
    |2 rough| <= eps / 4; `want` of each sign of the reference's cov.  cut_rows: rows 2, 3 repeat row 1 (the last block row of a height
    = 2 mod 4 is read that way; its four distinct samples, two of them weighted three times, leave few blocks that near zero, and a sign
    may be missing among them: the whole block rows of the same frame hold both).  -> (yb, ub, vb) of shape (<= 2 want, 4, 4 | 2)"""
    rng = np.random.default_rng(1605 + cut_rows)
    n = 400000
    uv = rng.integers(8, 245, (n, 1, 1, 2)) + rng.integers(0, 4, (n, 4, 2, 2))
    if cut_rows:
        uv[:, 2:] = uv[:, 1:2]
    # candidates worth the strict model: Co, Cg as the linear functions of (U, V) they are but for rounding
    u, v = uv[..., 0].reshape(n, 8) / 255.0, uv[..., 1].reshape(n, 8) / 255.0
    co, cg = -1.0562 * u + 0.8963 * v, -0.6347 * u - 0.71455 * v
    hx, hy = np.ptp(co, axis=1), np.ptp(cg, axis=1)
    lin = ((co - (co.max(1) + co.min(1))[:, None] / 2) * (cg - (cg.max(1) + cg.min(1))[:, None] / 2)).sum(1)
    best = np.flatnonzero((hx * hy > 0) & (np.abs(2 * lin) <= 0.5 * 1e-5 * (hx + hy)))   # twice the margin asked for below
    uv = uv[best]
    yb = ENDS[rng.integers(0, 4, (len(best), 4, 2))].reshape(-1, 4, 4)
    if cut_rows:
        yb[:, 2:] = yb[:, 1:2]
    s = diagonal_stage(*planes(yb[None], uv[None, ..., 0], uv[None, ..., 1], 4 * len(best), 4))
    worst, _ = two_rough_over_eps(s)
    ok = ((s["hx"] * s["hy"] > 0) & (worst <= 0.25))[0]
    neg, pos = np.flatnonzero(ok & (s["cov"][0] < 0)), np.flatnonzero(ok & (s["cov"][0] > 0))
    assert (len(neg) >= want and len(pos) >= want) if not cut_rows else len(neg) + len(pos) >= want, (len(neg), len(pos))
    pick = np.concatenate([neg[np.argsort(worst[0][neg], kind="stable")[:want]], pos[np.argsort(worst[0][pos], kind="stable")[:want]]])
    return yb[pick], uv[pick][..., 0], uv[pick][..., 1]


def frame_near_zero(w, h):
    rng = np.random.default_rng(31 + w)
    bw, bh = (w + 3) // 4, (h + 3) // 4
    yb, ub, vb = rng.integers(0, 256, (bh, bw, 4, 4)), rng.integers(0, 256, (bh, bw, 4, 2)), rng.integers(0, 256, (bh, bw, 4, 2))
    whole, cut = near_zero_pool(False), near_zero_pool(True)
    n = 0
    for by in range(bh):
        py, pu, pv = cut if (h % 4 and by == bh - 1) else whole
        for bx in PLACED:
            k = (n % 2) * (len(py) // 2) + (n // 2) % (len(py) // 2)   # a pool of both signs holds them in halves: they alternate
            yb[by, bx], ub[by, bx], vb[by, bx] = py[k], pu[k], pv[k]
            n += 1
    y, u, v = planes(yb, ub, vb, w, h)
    s = diagonal_stage(y, u, v)
    worst, _ = two_rough_over_eps(s)
    at = np.zeros((bh, bw), bool); at[:, PLACED] = True
    assert (worst[at] <= 0.25).all() and (s["hx"] * s["hy"] > 0)[at].all(), float(worst[at].max())
    assert (s["cov"][at] < 0).any() and (s["cov"][at] > 0).any()
    return y, u, v


def frame_decided(w, h):
    rng = np.random.default_rng(32 + w)
    bw, bh = (w + 3) // 4, (h + 3) // 4
    yb, ub, vb = rng.integers(0, 256, (bh, bw, 4, 4)), rng.integers(0, 256, (bh, bw, 4, 2)), rng.integers(0, 256, (bh, bw, 4, 2))
    flat = np.arange(bh * bw).reshape(bh, bw) % 5 == 2   # wholly flat blocks: one Y, U, V
    for p in (yb, ub, vb):
        p[flat] = rng.integers(0, 256, (int(flat.sum()), 1, 1))
    for _ in range(50):
        y, u, v = planes(yb, ub, vb, w, h)
        s = diagonal_stage(y, u, v)
        _, least = two_rough_over_eps(s)
        bad = ~((least >= 4.0) | (s["hx"] * s["hy"] == 0))
        if not bad.any():
            break
        m = int(bad.sum())
        yb[bad], ub[bad], vb[bad] = rng.integers(0, 256, (m, 4, 4)), rng.integers(0, 256, (m, 4, 2)), rng.integers(0, 256, (m, 4, 2))
    assert not bad.any() and ((s["hx"] == 0) & (s["hy"] == 0))[flat].all()
    return y, u, v


def frame_one_chroma(w, h):
    """ONE chroma sample per block under extreme lumas: Co / Cg spread by rounding only, and by some (hx hy > 0) in every block"""
    rng = np.random.default_rng(33 + w)
    bw, bh = (w + 3) // 4, (h + 3) // 4
    yb = ENDS[rng.integers(0, 4, (bh, bw, 4, 2))].reshape(bh, bw, 4, 4)
    ub, vb = np.broadcast_to(rng.integers(0, 256, (bh, bw, 1, 1)), (bh, bw, 4, 2)).copy(), np.broadcast_to(rng.integers(0, 256, (bh, bw, 1, 1)), (bh, bw, 4, 2)).copy()
    for _ in range(200):
        y, u, v = planes(yb, ub, vb, w, h)
        s = diagonal_stage(y, u, v)
        bad = s["hx"] * s["hy"] == 0
        if not bad.any():
            break
        m = int(bad.sum())
        yb[bad] = ENDS[rng.integers(0, 4, (m, 4, 2))].reshape(m, 4, 4)
        ub[bad], vb[bad] = rng.integers(0, 256, (m, 1, 1)), rng.integers(0, 256, (m, 1, 1))
    worst, _ = two_rough_over_eps(s)
    assert not bad.any() and (worst <= 0.25).all() and float(max(s["hx"].max(), s["hy"].max())) < 1e-6
    return y, u, v


def wave_evaluations(fmt, w, h):
    """how often a wave passes the stage in one encode: once per block row and wave for UYVY (one block per lane), once per block row, wave
    and block of the lane for v210 (three blocks per lane) -- the unit in which ug_hip_dxt_encode_stats counts, too"""
    bw, bh = (w + 3) // 4, (h + 3) // 4
    if fmt == "UYVY":
        return bh * ((bw + 63) // 64)
    return bh * sum(((bw - k + 2) // 3 + 63) // 64 for k in range(3))


FRAMES = {"near_zero": (frame_near_zero, "all"), "decided": (frame_decided, "none"), "one_chroma_extreme_luma": (frame_one_chroma, "all")}


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(FRAMES))
def test_diagonal_on_its_seam(hip, po, name, size):
    import torch
    from ultragrid_amd import lib as L
    l = L.load()
    w, h = size
    build, expect = FRAMES[name]
    y, u, v = build(w, h)
    low = np.random.default_rng(99 + w).integers(0, 4, (h, 2 * w)).astype(np.uint32)
    srcs = {"UYVY": (L.PF_UYVY, po.IN_UYVY, pack_uyvy(y, u, v)), "v210": (L.PF_V210, po.IN_V210, pack_v210(y, u, v, low))}
    bad, counts = [], {}
    for fmt, (pf, pin, src) in srcs.items():
        st = (C.c_ulonglong * 3)()
        assert l.ug_hip_dxt_encode_stats_ex(None, 0, 1) == 0
        got = hip.dxt_encode(pf, L.DXT5_YCOCG, torch.from_numpy(src).cuda(), w, h).cpu().numpy()
        assert l.ug_hip_dxt_encode_stats_ex(st, 3, 1) == 0
        counts[fmt] = int(st[2])
        print(f"{name} {fmt} {w}x{h}: colour full form {int(st[0])}, alpha full form {int(st[1])}, exact covariance {int(st[2])} of {wave_evaluations(fmt, w, h)} waves")
        want = po.dxt_encode(pin, po.OUT_DXT5YCOCG, src, w, h)
        if not np.array_equal(got, want):
            bad.append((fmt, "even", int(np.count_nonzero(got != want))))
        got = hip.dxt_encode(pf, L.DXT5_YCOCG, torch.from_numpy(src).cuda(), w, h, ties=L.TIES_AWAY).cpu().numpy()
        want = po.dxt_encode(pin, po.OUT_DXT5YCOCG, src, w, h, ties="away")
        if not np.array_equal(got, want):
            bad.append((fmt, "away", int(np.count_nonzero(got != want))))
        assert l.ug_hip_dxt_encode_stats_ex(st, 3, 0) == 0 and int(st[2]) == counts[fmt]   # the same waves under the other tie rule ...
        two = (C.c_ulonglong * 2)()
        assert l.ug_hip_dxt_encode_stats(two, 1) == 0 and l.ug_hip_dxt_encode_stats_ex(st, 3, 0) == 0 and int(st[2]) == 0   # ... and either reset clears all three
    assert not bad, bad
    for fmt in srcs:
        assert counts[fmt] == (wave_evaluations(fmt, w, h) if expect == "all" else 0), (fmt, counts[fmt], wave_evaluations(fmt, w, h))
