"""From a 4:2:2 source the DXT5-YCoCg encoder takes the 2-bit colour index of a chroma pair from the projection of its even pixel on the palette
segment (dxt_encode.hip, encode_dxt5ycocg, the chroma-pair side of the fast colour stage): s = fma(Co, ka, fma(Cg, kb, kc)) with the clamp
modifier, r = fma(s, 3, 2^23) holds j = RN(3 s) = 0 .. 3, which picks c0, c2, c3, c1, and fma(s, 3, -j) is the distance of 3 s to that
integer.  A block is certified where 3 s stays more than
    eps = (8.5e-6 sqrt(vv) + 7.2e-6 sqrt(dmax) + 4.3e-6 dmax) / vv        (thirds of the segment)
away from a half-integer for all eight pairs, or it is flat; a wave that holds an uncertified block evaluates the reference's two distances
for every pixel in the zone RN(clamp(3 s - 1/2, 0, 2)), as before.  This restates the stage in strict numpy.float32, one IEEE operation per
statement (the machinery of tests/test_dxt_pair_linear_bound.py: palettes rebuilt from the oracle's own end-point bits), over video-like,
random and seam content, and checks that
(a) the restatement's colour indices are the oracle's on every pixel,
(b) no certified pair decides otherwise than the reference for either of its pixels,
(c) the fp32 projection stays within eps / 4 of the same quantity formed in float64 from the fp32 palette (both limited to [-1/2, 7/2]: all
    three bisectors lie inside, and beyond it the clamp decides),
(d) for each of the three bisectors, the float64 projection margin 3 s - (k + 1/2) and the float64 half-difference of the true squared
    distances to the two palette entries, scaled by 9 / vv, stay within eps / 4 of each other: the colinearity term,
(e) the content is not vacuous: S2 and S1 each hold uncertified pairs and pairs within 4 eps of a bisector,
(f) at most 0.12 of the waves of the video-like frame hold an uncertified block."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dxt_pair_chroma_bound import F, K_OFFSET, K_INV255, ycocg_of_pair  # noqa: E402
from test_dxt_pair_cov_bound import pad_planes  # noqa: E402
from test_dxt_pair_linear_bound import ZONE_PAIRS, contents, fma, palette_index, sq_dist  # noqa: E402
from test_gpu_dxt_pair_zone import pack_uyvy  # noqa: E402

D = np.float64
EPS_SEG, EPS_DIAG, EPS_DMAX = F(8.5e-6), F(7.2e-6), F(4.3e-6)   # the kernel's kProjEpsSeg, kProjEpsDiag, kProjEpsDmax
J_TO_INDEX = np.array([0, 2, 3, 1], np.uint32)                   # c0, c2, c3, c1 along the segment
BISECTORS = ((0, 2), (2, 3), (3, 1))                             # palette entries on either side of 3 s = 1/2, 3/2, 5/2, in the segment's order
WAVE_SHARE_CAP = 0.12


def projection_stage(po, y, u, v):
    """bytes (y: (h, w), u / v: (h, w / 2)) -> the fast colour stage per 4 x 4 block, as the kernel states it.  Arrays of shape (bh, bw) per
    block, (bh, bw, 8) per pair, (bh, bw, 16) per pixel (pixel i = 4 row + column, pair j = pixels 2 j, 2 j + 1)"""
    h0, w0 = y.shape
    out = po.dxt_encode(po.IN_UYVY, po.OUT_DXT5YCOCG, pack_uyvy(y, u, v), w0, h0)
    y, u, v = pad_planes(y, u, v)
    h, w = y.shape
    bh, bw = h // 4, w // 4
    words = np.ascontiguousarray(out).view("<u4").reshape(bh, bw, 4)
    w_end, w_idx = words[..., 2], words[..., 3]
    to_float = lambda b: b.astype(F) * K_INV255
    co0, cg0, co1, cg1 = ycocg_of_pair(to_float(y[:, 0::2]), to_float(y[:, 1::2]), to_float(u), to_float(v))
    co = np.empty((h, w), F); cg = np.empty((h, w), F)
    co[:, 0::2] = co0; co[:, 1::2] = co1; cg[:, 0::2] = cg0; cg[:, 1::2] = cg1
    blocks = lambda p: p.reshape(bh, 4, bw, 4).transpose(0, 2, 1, 3).reshape(bh, bw, 16)
    co, cg = blocks(co), blocks(cg)
    mn_co, mx_co, mn_cg, mx_cg = co.min(-1), co.max(-1), cg.min(-1), cg.max(-1)

    # the palette from the end points the reference emitted (EmitEndPointsYCoCgDXT5's dequantisation, kernel statements)
    c0, c1 = w_end & 0xFFFF, w_end >> 16
    rfs = F(1.0) / ((c0 & 31) + 1).astype(F)   # 1, 1/2, 1/4
    inv255 = F(1.0 / 255.0)

    def ends(c):
        i0, i1 = (c >> 11) & 31, (c >> 5) & 63
        i0, i1 = (i0 << 3) | (i0 >> 2), (i1 << 2) | (i1 >> 4)
        return [(i.astype(F) * inv255 - K_OFFSET) * rfs + K_OFFSET for i in (i0, i1)]   # the product by rfs is exact: fma or not
    (x0, y0), (x1, y1) = ends(c0), ends(c1)
    q1, q2 = F(1.0 / 3.0), F(2.0 / 3.0)
    w1, w2 = F(1.0) - q1, F(1.0) - q2
    px = [x0, x1, x0 * w1 + x1 * q1, x0 * w2 + x1 * q2]
    py = [y0, y1, y0 * w1 + y1 * q1, y0 * w2 + y1 * q2]
    assert all(p.dtype == F for p in px + py)

    # the stage's precondition (unchanged)
    vx, vy = x1 - x0, y1 - y0
    vv = vx * vx + vy * vy
    e0 = np.maximum(np.maximum(mx_co, x0), x1) - np.minimum(np.minimum(mn_co, x0), x1)
    e1 = np.maximum(np.maximum(mx_cg, y0), y1) - np.minimum(np.minimum(mn_cg, y0), y1)
    dmax = e0 * e0 + e1 * e1
    flat = (mn_co == mx_co) & (mn_cg == mx_cg)
    pre = ((vv >= F(1e-5)) & (vv * F(256.0) > dmax)) | flat
    pad = (-bw) % 64   # UYVY: one block per lane, a wave is 64 consecutive blocks of a block row
    waves = lambda b, fill: np.concatenate([b, np.full((bh, pad), fill, bool)], axis=1).reshape(bh, -1, 64)
    in_fast = np.repeat(waves(pre, True).all(-1), 64, axis=1)[:, :bw]

    with np.errstate(all="ignore"):
        co_e, cg_e = co[..., 0::2], cg[..., 0::2]
        # the projection: one per pair, index from float bits
        rvv = F(1.0) / vv
        ka, kb = vx * rvv, vy * rvv
        kc = fma(-x0, ka, -y0 * kb)
        t32 = fma(co_e, ka[..., None], fma(cg_e, kb[..., None], kc[..., None]))   # unclamped
        s = np.nan_to_num(np.clip(t32, F(0), F(1)))   # a NaN (vv == 0: flat) clamps to 0 on the GPU
        j = np.rint(s.astype(D) * 3.0)                # fma(s, 3, 2^23): RN to the integer, ties to even
        dist = fma(s, F(3.0), (-j).astype(F))         # kIndexBias - r = -j exactly
        sd = np.sqrt(dmax)
        eps = fma(sd, fma(sd, EPS_DMAX, EPS_DIAG), EPS_SEG * np.sqrt(vv)) * rvv
        assert dist.dtype == F and eps.dtype == F
        cert_pair = np.abs(dist) < (F(0.5) - eps)[..., None]
        proj_idx = np.repeat(J_TO_INDEX[j.astype(np.intp)], 2, axis=-1)
        # the same projection in float64 from the fp32 palette, about c0
        vx64, vy64 = vx.astype(D), vy.astype(D)
        vv64 = vx64 * vx64 + vy64 * vy64
        t64 = ((co_e.astype(D) - x0.astype(D)[..., None]) * vx64[..., None] + (cg_e.astype(D) - y0.astype(D)[..., None]) * vy64[..., None]) / vv64[..., None]
        # half of |p - A|^2 - |p - B|^2 in float64 for each bisector, scaled to thirds of the segment
        half = []
        for a, b in BISECTORS:
            ax, ay, bx, by = (q.astype(D)[..., None] for q in (px[a], py[a], px[b], py[b]))
            half.append(((bx - ax) * (co_e.astype(D) - (ax + bx) / 2) + (by - ay) * (cg_e.astype(D) - (ay + by) / 2)) * (9.0 / vv64[..., None]))

        # the exact side, as before: zone from the projection scaled by 3/2, the reference's open comparison for every pixel
        inv = F(1.5) * (F(1.0) / vv)
        za, zb = vx * inv, vy * inv
        zc = fma(-x0, za, fma(-y0, zb, F(-0.25)))
        sz = np.clip(fma(co_e, za[..., None], fma(cg_e, zb[..., None], zc[..., None])), F(0), F(1))
        zone = np.nan_to_num(np.rint(sz.astype(D) * 2.0)).astype(np.intp)
        zone_px = np.repeat(zone, 2, axis=-1)
        pal32 = lambda p, k: np.take_along_axis(np.stack([p[a_b[k]] for a_b in ZONE_PAIRS], -1), zone_px, -1)
        bit = sq_dist(co, cg, pal32(px, 0), pal32(py, 0)) > sq_dist(co, cg, pal32(px, 1), pal32(py, 1))
        exact_idx = np.choose(zone_px, [2 * bit, 2 + bit, 1 + 2 * bit]).astype(np.uint32)
        d = [sq_dist(co, cg, px[k][..., None], py[k][..., None]) for k in range(4)]
        full_idx = palette_index(*d)
        flat_idx = np.broadcast_to(full_idx[..., :1], full_idx.shape)
    cert_block = cert_pair.all(-1) | flat
    wave_cert = np.repeat(waves(cert_block | ~in_fast, True).all(-1), 64, axis=1)[:, :bw]
    fast_idx = np.where(wave_cert[..., None], proj_idx, exact_idx)
    idx = np.where(in_fast[..., None], np.where(flat[..., None], flat_idx, fast_idx), full_idx)
    want = (w_idx[..., None] >> (2 * np.arange(16, dtype=np.uint32))) & 3
    return {"idx": idx, "want": want, "t32": t32, "t64": t64, "half": half, "dist": dist, "eps": eps, "cert_pair": cert_pair, "cert_block": cert_block,
            "proj_idx": proj_idx, "flat": flat, "pre": pre, "in_fast": in_fast, "vv": vv, "dmax": dmax}


def margins(s):
    """per pair: distance of 3 s to the nearest half-integer, (fp32 form, float64 form); the clamp counts as decided (margin 1/2)"""
    m32 = 0.5 - np.abs(s["dist"].astype(D))
    t = np.clip(3.0 * s["t64"], 0.0, 3.0)
    return m32, 0.5 - np.abs(t - np.rint(t))


def wave_share_uncertified(s):
    """share of waves (64 consecutive blocks of a block row, UYVY's one block per lane) that reach the stage and hold an uncertified
    block: the waves ug_hip_dxt_encode_stats_ex counts in counts[3]"""
    bad = ~s["cert_block"] & s["in_fast"]
    bh, bw = bad.shape
    bad = np.concatenate([bad, np.zeros((bh, (-bw) % 64), bool)], axis=1).reshape(bh, -1, 64)
    return float(bad.any(-1).mean())


@pytest.fixture(scope="module")
def stages(po):
    return {name: projection_stage(po, *planes) for name, planes in contents().items()}


def test_content_is_what_the_issue_names(stages):
    assert len(stages) == 8 and stages["S2"]["idx"].shape == (128, 960, 16) and stages["sixths_extreme_luma"]["dist"].shape == (8, 128, 8)


def test_restatement_gives_the_oracles_indices(stages):
    for name, s in stages.items():
        wrong = int((s["idx"] != s["want"]).sum())
        print(f"{name}: {wrong} of {s['idx'].size} colour indices differ from the oracle's; {100 * s['in_fast'].mean():.1f} % of blocks in the fast stage")
        assert wrong == 0, (name, wrong)


def test_certified_pairs_decide_as_the_reference(stages):
    for name, s in stages.items():
        live = (s["in_fast"] & ~s["flat"])[..., None]
        c = live & s["cert_pair"]
        differs = (s["proj_idx"][..., 0::2] != s["want"][..., 0::2]) | (s["proj_idx"][..., 1::2] != s["want"][..., 1::2])
        wrong, miss = c & differs, live & ~s["cert_pair"] & differs
        print(f"{name}: {int(c.sum())} of {int(live.sum()) * 8} pairs certified, {int(wrong.sum())} of them decide otherwise than the reference; "
              f"{int(miss.sum())} uncertified pairs would")
        assert not wrong.any(), (name, int(wrong.sum()))


def test_fp32_projection_is_within_a_quarter_of_eps_of_float64(stages):
    for name, s in stages.items():
        live = s["in_fast"] & ~s["flat"]
        if not live.any():
            print(f"{name}: no block reaches the projection")
            continue
        lim = lambda t: np.clip(3.0 * t.astype(D), -0.5, 3.5)
        d = np.abs(lim(s["t32"]) - lim(s["t64"]))[live]
        worst = float((d / s["eps"].astype(D)[live][:, None]).max())
        print(f"{name}: max |3 s32 - 3 s64| / eps = {worst:.4g}")
        assert worst <= 0.25, (name, worst)


def test_colinearity_term_is_within_a_quarter_of_eps(stages):
    for name, s in stages.items():
        live = s["in_fast"] & ~s["flat"]
        if not live.any():
            continue
        eps = s["eps"].astype(D)[live][:, None]
        for k, half in enumerate(s["half"]):
            d = np.abs((3.0 * s["t64"] - (k + 0.5)) - half)[live]
            worst = float((d / eps).max())
            print(f"{name}: bisector at {2 * k + 1}/6: max |margin - 9 H / vv| / eps = {worst:.4g}")
            assert worst <= 0.25, (name, k, worst)


def test_content_is_not_vacuous(stages):
    for name in ("S2", "S1"):
        s = stages[name]
        live = (s["in_fast"] & ~s["flat"])[..., None]
        m32, _ = margins(s)
        uncertified = int((live & ~s["cert_pair"]).sum())
        close = int((live & (m32 < 4.0 * s["eps"].astype(D)[..., None])).sum())
        print(f"{name}: {uncertified} uncertified pairs, {close} within 4 eps of a bisector, of {int(live.sum()) * 8}")
        assert uncertified > 0 and close > 0, (name, uncertified, close)


def test_video_like_frames_are_certified_almost_everywhere(stages):
    share = wave_share_uncertified(stages["S2"])
    blocks = float((~stages["S2"]["cert_block"] & stages["S2"]["in_fast"]).mean())
    print(f"S2: {100 * blocks:.4f} % of blocks, {100 * share:.3f} % of waves uncertified; S1: {100 * wave_share_uncertified(stages['S1']):.3f} % of waves")
    for name in list(stages)[2:]:
        print(f"{name}: {100 * wave_share_uncertified(stages[name]):.1f} % of waves uncertified, {100 * (1 - stages[name]['in_fast'].mean()):.1f} % of blocks in the full form")
    assert share <= WAVE_SHARE_CAP, share
