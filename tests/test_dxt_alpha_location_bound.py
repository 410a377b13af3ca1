"""From a 4:2:2 source the DXT5-YCoCg encoder takes the 3-bit alpha count of a pixel from its location among the thresholds (dxt_encode.hip,
encode_dxt5ycocg, the chroma-pair side of the alpha stage): with the reference's ends mn, mx (after the inset) and R = mx - mn,
    u = clamp01(fma(Y4, -inv / 4, fma(mn, inv, 1))),  inv = rcp(R),       r = fma(u, 7, 2^23) holds c = RN(7 u) = 0 .. 7,
and fma(u, 7, -c) is the distance of 7 u to that integer.  The thresholds lie at the half-integers of t = 7 - (a - mn) * 7 / R, so c is the
reference's count #{k : a <= ab_k} wherever 7 u is not next to a half-integer, and a block is certified where it stays more than
    eps = 2.2e-6 + 5.7e-6 / R        (steps of R / 7)
away from one for all sixteen pixels; a wave that holds an uncertified block forms the thresholds and evaluates the reference's comparison
for every pixel in the row RN(clamp(t - 1/2, 0, 7)), as before.  This restates the stage in strict numpy.float32, one IEEE operation per
statement, over video-like, random and seam content and over frames built for the stage's own edges (range next to 2^-10, ends clamped at 0,
at 1 and at both, luma far outside the ends, a luma level halfway between two others under flat chroma), and checks that
(a) the restatement's 48-bit alpha index field is the oracle's on every block,
(b) no certified pixel's RN(7 u) differs from the reference's count,
(c) the fp32 7 u stays within eps / 4 of the same quantity formed in float64 from the fp32 ends (both limited to [-1/2, 15/2]: all seven
    thresholds lie inside, and beyond it the clamp decides),
(d) for each of the seven thresholds, the float64 location margin t - (m - 1/2) and the float64 distance of Y4 to the reference's own fp32
    threshold, in steps, stay within eps / 4 of each other: the term that covers the thresholds' rounding,
(e) the content is not vacuous: S2 and S1 each hold uncertified pixels and pixels within 4 eps of a threshold,
(f) at most 0.10 of the waves of the video-like frame hold an uncertified block,
(g) the midpoint frame is uncertified in every wave: content with flat chroma and few luma levels pays both sides, and that is stated."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dxt_pair_cov_bound import pad_planes  # noqa: E402,F401  (ycocg_blocks_yuv reads a cut picture through it)
from test_dxt_pair_linear_bound import contents  # noqa: E402
from test_dxt_pow2_fold_bound import ALL_WIDE, F, alpha_stage, clamp01, fma, ycocg_blocks_yuv  # noqa: E402
from test_gpu_dxt_pair_cov import planes  # noqa: E402
from test_gpu_dxt_pair_zone import pack_uyvy  # noqa: E402

D = np.float64
EPS_FIXED, EPS_RANGE = F(2.2e-6), F(5.7e-6)  # the kernel's kAlphaEpsFixed, kAlphaEpsRange
WAVE_SHARE_CAP = 0.10
# row g of the exact side's table holds D_(g + 1), thresholds descending: ab_2, ab_3, .., ab_7, ab_1, then -inf (index into ab[0..6] = ab_1..ab_7)
ROW_TO_AB = (1, 2, 3, 4, 5, 6, 0)


def waves_of(per_block, fill):
    """(bh, bw) -> (bh, waves, 64): UYVY has one block per lane, a wave is 64 consecutive blocks of a block row"""
    bh, bw = per_block.shape
    return np.concatenate([per_block, np.full((bh, (-bw) % 64), fill, bool)], axis=1).reshape(bh, -1, 64)


def spread_waves(per_wave, bw):
    return np.repeat(per_wave, 64, axis=1)[:, :bw]


def location_stage(po, y, u, v):
    """bytes (y: (h, w), u / v: (h, w / 2)) -> the alpha index stage per 4 x 4 block, as the kernel states it for a chroma-pair loader.
    Arrays of shape (bh, bw) per block, (bh, bw, 16) per pixel (pixel i = 4 row + column), (bh, bw, 7) per threshold m = 1 .. 7 (descending)"""
    h0, w0 = y.shape
    out = po.dxt_encode(po.IN_UYVY, po.OUT_DXT5YCOCG, pack_uyvy(y, u, v), w0, h0)
    y4 = ycocg_blocks_yuv(y, u, v)[0]
    bh, bw = y4.shape[:2]
    words = np.ascontiguousarray(out).view("<u4").reshape(bh, bw, 4).astype(np.uint64)
    field = (words[..., 0] >> np.uint64(16)) | (words[..., 1] << np.uint64(16))
    want = ((field[..., None] >> (np.uint64(3) * np.arange(16, dtype=np.uint64))) & np.uint64(7)).astype(np.uint32)

    s = alpha_stage(y4)
    mn, mx, ab4 = s["mn_k"], s["mx_k"], s["ab4"]   # the reference's ends; 4 x its thresholds ab_1 .. ab_7, bit for bit
    rng = mx - mn
    assert rng.dtype == F
    wide = rng > ALL_WIDE
    in_stage = spread_waves(waves_of(wide, True).all(-1), bw)   # the wave test in front of both sides
    ref_count = sum((s["y"] <= t[..., None]).astype(np.uint32) for t in s["ab"])   # glsl:262-312 on the reference's own Y and ab_k

    with np.errstate(all="ignore"):
        # the location: one per pixel, count from float bits
        inv = F(1.0) / rng
        t0, ninv = fma(mn, inv, F(1.0)), inv * F(-0.25)
        t32 = fma(y4, ninv[..., None], t0[..., None])           # unclamped
        uu = np.nan_to_num(clamp01(t32))                         # a NaN (range 0: not in the stage) clamps to 0 on the GPU
        c = np.rint(uu.astype(D) * 7.0)                          # fma(u, 7, 2^23): RN to the integer, ties to even
        dist = fma(uu, F(7.0), (-c).astype(F))                   # kIndexBias - r = -c exactly
        eps = fma(EPS_RANGE, inv, EPS_FIXED)
        assert dist.dtype == F and eps.dtype == F and ninv.dtype == F
        cert_px = np.abs(dist) < (F(0.5) - eps)[..., None]
        loc_count = c.astype(np.uint32)
        # the same location in float64 from the fp32 ends, and per threshold the distance of Y4 to the reference's fp32 4 D_m, in steps
        mn64, r64 = mn.astype(D)[..., None], rng.astype(D)[..., None]
        t64 = 7.0 - (y4.astype(D) * 0.25 - mn64) * 7.0 / r64
        d4 = np.stack([ab4[ROW_TO_AB[m - 1]] for m in range(1, 8)], -1).astype(D)                       # 4 D_1 .. 4 D_7
        # margin - distance = (t - (m - 1/2)) - (4 D_m - Y4) * 7 / (4 R) does not depend on the pixel: 7 + 7 mn / R - (m - 1/2) - 7 (4 D_m) / (4 R)
        threshold_term = 7.0 + 7.0 * mn64 / r64 - (np.arange(1, 8) - 0.5) - 7.0 * d4 / (4.0 * r64)

        # the exact side, as before: row from the location shifted by half a step, the reference's comparison on its own threshold
        t0x = fma(mn, inv, F(6.5 / 7.0))
        g = np.rint(np.nan_to_num(clamp01(fma(y4, ninv[..., None], t0x[..., None]))).astype(D) * 7.0).astype(np.intp)
        rows = np.stack([ab4[k] for k in ROW_TO_AB] + [np.full(rng.shape, -np.inf, F)], -1)
        exact_count = g.astype(np.uint32) + (y4 <= np.take_along_axis(rows, g, -1)).astype(np.uint32)
        linear_count = sum((y4 <= t[..., None]).astype(np.uint32) for t in ab4)   # narrow waves: the reference's form on Y4
    cert_block = cert_px.all(-1)
    wave_cert = spread_waves(waves_of(cert_block | ~in_stage, True).all(-1), bw)
    count = np.where(in_stage[..., None], np.where(wave_cert[..., None], loc_count, exact_count), linear_count)
    c1 = (count + 1) & 7
    idx = c1 ^ (c1 < 2)   # glsl:281-290
    return {"idx": idx, "want": want, "t32": t32, "t64": t64, "dist": dist, "eps": eps, "cert_px": cert_px, "cert_block": cert_block,
            "loc_count": loc_count, "ref_count": ref_count, "threshold_term": threshold_term, "wide": wide, "in_stage": in_stage,
            "range": rng, "mn": mn, "mx": mx, "y4": y4}


def margins(s):
    """per pixel: distance of 7 u to the nearest half-integer, (fp32 form, float64 form); the clamp counts as decided (margin 1/2)"""
    m32 = 0.5 - np.abs(s["dist"].astype(D))
    t = np.clip(s["t64"], 0.0, 7.0)
    return m32, 0.5 - np.abs(t - np.rint(t))


def wave_share_uncertified(s):
    """share of waves that reach the stage and hold an uncertified block: the waves ug_hip_dxt_encode_stats_alpha counts"""
    return float(waves_of(~s["cert_block"] & s["in_stage"], False).any(-1).mean())


# ---------------------------------------------------------------------------------------------------------------------------------
# frames for the stage's own edges, 512 x 32 unless cut: blocks (bh, bw, 4, 4) of Y and (bh, bw, 4, 2) of U, V bytes
# ---------------------------------------------------------------------------------------------------------------------------------
def narrow_pool():
    """two-level blocks whose clamped range lies next to 2^-10: the lower end clamps at 0 and the upper one comes out just above it.
    -> ((ya, yb, u, v) with the range just above 2^-10, the same just below), found by evaluating the model over every candidate"""
    ya, yb, u, v = (p.ravel() for p in np.meshgrid(np.arange(0, 8), np.arange(8, 24), np.arange(96, 160, 3), np.arange(96, 160, 3), indexing="ij"))
    n = len(ya)
    yblk = np.where(np.arange(16).reshape(4, 4) % 3 == 0, ya[:, None, None], yb[:, None, None])
    y, uu, vv = planes(yblk[None], np.broadcast_to(u[:, None, None], (n, 4, 2))[None], np.broadcast_to(v[:, None, None], (n, 4, 2))[None], 4 * n, 4)
    s = alpha_stage(ycocg_blocks_yuv(y, uu, vv)[0])
    rng = (s["mx_k"] - s["mn_k"])[0].astype(D)
    above = np.flatnonzero((rng > 2.0 ** -10) & (rng < 1.5 * 2.0 ** -10))
    below = np.flatnonzero((rng < 2.0 ** -10) & (rng > 0.5 * 2.0 ** -10))
    assert len(above) and len(below), (len(above), len(below))
    a, b = above[np.argmin(rng[above])], below[np.argmax(rng[below])]
    return tuple(int(p[a]) for p in (ya, yb, u, v)), tuple(int(p[b]) for p in (ya, yb, u, v))


def frame_narrow(w, h, below):
    bw, bh = (w + 3) // 4, (h + 3) // 4
    ya, yb, u, v = narrow_pool()[1 if below else 0]
    yblk = np.where(np.arange(16).reshape(4, 4) % 3 == 0, ya, yb)
    return planes(np.broadcast_to(yblk, (bh, bw, 4, 4)), np.full((bh, bw, 4, 2), u), np.full((bh, bw, 4, 2), v), w, h)


def frame_clamped(w, h, low, high, seed):
    """random luma between ends that clamp: y bytes <= 8 (luma below 0 after the inset) and / or >= 244 (above 1)"""
    rng = np.random.default_rng(seed + w)
    bw, bh = (w + 3) // 4, (h + 3) // 4
    yb = rng.integers(40 if not low else 24, 216 if not high else 232, (bh, bw, 4, 4))
    at = rng.integers(0, 16, (bh, bw, 2))
    flat = yb.reshape(bh, bw, 16)
    if low:
        np.put_along_axis(flat, at[..., :1], rng.integers(0, 9, (bh, bw, 1)), -1)
    if high:
        np.put_along_axis(flat, (at[..., 1:] + (at[..., 1:] == at[..., :1])) % 16, rng.integers(244, 256, (bh, bw, 1)), -1)
    ub, vb = rng.integers(112, 144, (bh, bw, 4, 2)), rng.integers(112, 144, (bh, bw, 4, 2))
    return planes(flat.reshape(bh, bw, 4, 4), ub, vb, w, h)


def frame_far_outside(w, h):
    """extreme lumas under extreme chroma: both ends clamp and pixels lie a third of the range beyond them"""
    rng = np.random.default_rng(77 + w)
    bw, bh = (w + 3) // 4, (h + 3) // 4
    yb = np.array([0, 255, 16, 235, 60, 128, 200])[rng.integers(0, 7, (bh, bw, 4, 4))]
    ub, vb = np.array([0, 255, 128])[rng.integers(0, 3, (bh, bw, 4, 2))], np.array([0, 255, 128])[rng.integers(0, 3, (bh, bw, 4, 2))]
    return planes(yb, ub, vb, w, h)


def frame_midpoint(w, h):
    """flat chroma, three luma levels with the middle one halfway: in real arithmetic that pixel sits ON the middle threshold (m = 4, ab_5)"""
    rng = np.random.default_rng(78 + w)
    bw, bh = (w + 3) // 4, (h + 3) // 4
    lo = rng.integers(30, 100, (bh, bw, 1))
    half = rng.integers(10, 50, (bh, bw, 1))
    level = rng.integers(0, 3, (bh, bw, 16))
    level[..., :3] = (0, 1, 2)   # every block holds all three
    yb = (lo + half * level).reshape(bh, bw, 4, 4)
    return planes(yb, np.full((bh, bw, 4, 2), 128), np.full((bh, bw, 4, 2), 128), w, h)


def edge_frames(w=512, h=32):
    return {"range_above_2^-10": frame_narrow(w, h, False), "range_below_2^-10": frame_narrow(w, h, True),
            "clamped_at_0": frame_clamped(w, h, True, False, 71), "clamped_at_1": frame_clamped(w, h, False, True, 72),
            "clamped_at_both": frame_clamped(w, h, True, True, 73), "far_outside": frame_far_outside(w, h), "midpoint": frame_midpoint(w, h)}


@pytest.fixture(scope="module")
def stages(po):
    frames = contents()
    frames.update(edge_frames())
    return {name: location_stage(po, *p) for name, p in frames.items()}


def test_content_is_what_the_issue_names(stages):
    assert len(stages) == 15 and stages["S2"]["idx"].shape == (128, 960, 16) and stages["midpoint"]["dist"].shape == (8, 128, 16)
    above, below = stages["range_above_2^-10"]["range"], stages["range_below_2^-10"]["range"]
    print(f"narrow frames: range {float(above.max()):.6g} and {float(below.min()):.6g} around 2^-10 = {2.0 ** -10:.6g}")
    assert stages["range_above_2^-10"]["in_stage"].all() and not stages["range_below_2^-10"]["in_stage"].any()
    assert (above > ALL_WIDE).all() and (above < F(1.5) * ALL_WIDE).all() and (below < ALL_WIDE).all() and (below > F(0.5) * ALL_WIDE).all()
    for name, at0, at1 in (("clamped_at_0", True, False), ("clamped_at_1", False, True), ("clamped_at_both", True, True), ("far_outside", True, True)):
        s = stages[name]
        share0, share1 = float((s["mn"] == 0).mean()), float((s["mx"] == 1).mean())
        print(f"{name}: lower end clamped in {100 * share0:.0f} %, upper end in {100 * share1:.0f} % of blocks")
        assert (share0 > 0.8) == at0 or name == "far_outside", (name, share0)
        assert (share1 > 0.8) == at1 or name == "far_outside", (name, share1)
    s = stages["far_outside"]
    far = ((s["t32"] < -1.0 / 3) | (s["t32"] > 4.0 / 3)).mean()   # the unclamped u: beyond an end by a third of the range
    both = ((s["mn"] == 0) & (s["mx"] == 1)).mean()
    print(f"far_outside: both ends clamped in {100 * both:.0f} % of blocks, {100 * far:.1f} % of pixels a third of the range beyond an end")
    assert both > 0.3 and far > 0.02


def test_restatement_gives_the_oracles_index_field(stages):
    for name, s in stages.items():
        wrong = int((s["idx"] != s["want"]).any(-1).sum())
        print(f"{name}: {wrong} of {s['idx'].shape[0] * s['idx'].shape[1]} alpha index fields differ from the oracle's; "
              f"{100 * s['in_stage'].mean():.1f} % of blocks in the stage")
        assert wrong == 0, (name, wrong)


def test_certified_pixels_count_as_the_reference(stages):
    for name, s in stages.items():
        live = s["in_stage"][..., None]
        differs = s["loc_count"] != s["ref_count"]
        wrong, miss = live & s["cert_px"] & differs, live & ~s["cert_px"] & differs
        print(f"{name}: {int((live & s['cert_px']).sum())} of {int(live.sum()) * 16} pixels certified, {int(wrong.sum())} of them count otherwise "
              f"than the reference; {int(miss.sum())} uncertified pixels would")
        assert not wrong.any(), (name, int(wrong.sum()))


def test_fp32_location_is_within_a_quarter_of_eps_of_float64(stages):
    for name, s in stages.items():
        live = s["in_stage"]
        if not live.any():
            print(f"{name}: no block reaches the location")
            continue
        lim = lambda t: np.clip(t, -0.5, 7.5)
        d = np.abs(lim(7.0 * s["t32"].astype(D)) - lim(s["t64"]))[live]
        worst = float((d / s["eps"].astype(D)[live][:, None]).max())
        print(f"{name}: max |7 u32 - t64| / eps = {worst:.4g}")
        assert worst <= 0.25, (name, worst)


def test_threshold_term_is_within_a_quarter_of_eps(stages):
    for name, s in stages.items():
        live = s["in_stage"]
        if not live.any():
            continue
        ratio = np.abs(s["threshold_term"][live]) / s["eps"].astype(D)[live][:, None]
        worst = ratio.max(0)
        print(f"{name}: max |margin - distance to the fp32 threshold| / eps for m = 1 .. 7: " + " ".join(f"{x:.3f}" for x in worst))
        assert float(worst.max()) <= 0.25, (name, worst)


def test_content_is_not_vacuous(stages):
    for name in ("S2", "S1"):
        s = stages[name]
        live = s["in_stage"][..., None]
        m32, _ = margins(s)
        uncertified = int((live & ~s["cert_px"]).sum())
        close = int((live & (m32 < 4.0 * s["eps"].astype(D)[..., None])).sum())
        print(f"{name}: {uncertified} uncertified pixels, {close} within 4 eps of a threshold, of {int(live.sum()) * 16}")
        assert uncertified > 0 and close > 0, (name, uncertified, close)


def test_video_like_frames_are_certified_almost_everywhere(stages):
    share = wave_share_uncertified(stages["S2"])
    s = stages["S2"]
    rng = s["range"][s["in_stage"]]
    print(f"S2: {100 * float((~s['cert_block'] & s['in_stage']).mean()):.4f} % of blocks, {100 * share:.3f} % of waves uncertified; "
          f"S1: {100 * wave_share_uncertified(stages['S1']):.3f} % of waves; S2 block ranges: 1st percentile {np.percentile(rng, 1):.3f}, "
          f"median {np.median(rng):.3f}, 90th {np.percentile(rng, 90):.3f}; {int((~s['wide']).sum())} blocks not wide")
    for name in list(stages)[2:]:
        print(f"{name}: {100 * wave_share_uncertified(stages[name]):.1f} % of waves uncertified, {100 * (1 - stages[name]['in_stage'].mean()):.1f} % of blocks outside the stage")
    assert share <= WAVE_SHARE_CAP, share


def test_midpoint_frame_is_uncertified_in_every_wave(stages):
    s = stages["midpoint"]
    assert s["in_stage"].all()
    share = wave_share_uncertified(s)
    at_mid = (~s["cert_px"] & (np.abs(s["t64"] - 3.5) < 1e-3)).sum()
    print(f"midpoint: {100 * share:.1f} % of waves, {100 * float((~s['cert_block']).mean()):.1f} % of blocks uncertified; "
          f"{int(at_mid)} of {int((~s['cert_px']).sum())} uncertified pixels at the middle threshold")
    assert share == 1.0
