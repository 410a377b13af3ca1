"""From a 4:2:2 source the DXT5-YCoCg encoder takes the open comparison da > db of its fast colour stage ONCE per chroma pair, from the sign of
a linear form of the pair's even pixel (dxt_encode.hip, UG_DXT_PAIR_LINEAR): L = fma(-Co, m.x, fma(-Cg, m.y, c)) with m = A - B and
c = fma(m.x, s.x, m.y * s.y) / 2, s = A + B, is half of |p - A|^2 - |p - B|^2 up to an error the kernel's comment bounds by
eps = 1e-6 sqrt(vv) + 2^-21 dmax; a block whose eight |L| all exceed eps, or which is flat, is certified, and a wave that holds an uncertified
block evaluates the reference's two distances for every pixel.  This restates the stage in strict numpy.float32, one IEEE operation per
statement (conversion statements as tests/test_dxt_pair_chroma_bound.py writes them, palettes rebuilt from the oracle's own end-point bits
with the kernel's statements, fma through one float64 product and sum rounded once), and checks over video-like, random and seam content that
(a) the restatement's colour indices are the oracle's on every pixel, (b) no certified pair decides otherwise than the reference for either
of its pixels, (c) the fp32 L stays within eps / 4 of the one formed in float64, and (d) the certificate is not vacuous: fewer than a tenth of
the waves of a video-like frame hold an uncertified block."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dxt_pair_chroma_bound import F, K_OFFSET, K_INV255, ycocg_of_pair  # noqa: E402
from test_dxt_pair_cov_bound import pad_planes, uyvy_planes  # noqa: E402
from test_gpu_dxt_pair_zone import frames_for, pack_uyvy  # noqa: E402

D = np.float64
EPS_VV, EPS_DMAX = F(1e-6), F(2.0 ** -21)   # the kernel's eps = fma(dmax, 2^-21, 1e-6 * sqrt(vv))
ZONE_PAIRS = ((0, 2), (2, 3), (1, 3))        # palette entries (A, B) of the open comparison of zone 0, 1, 2: d0 > d2, d2 > d3, d1 > d3


def fma(a, b, c):
    """__builtin_fmaf: the product of two fp32 is exact in float64; the sum is rounded to float64, then to fp32 (where that differs from the
    one rounding of a true fma it does so by one fp32 ulp of the sum: far inside what (b) and (c) leave)"""
    return (np.asarray(a, F).astype(D) * np.asarray(b, F).astype(D) + np.asarray(c, F).astype(D)).astype(F)


def palette_index(d0, d1, d2, d3):
    """compress_dxt5ycocg_fp.glsl:237-244"""
    b0, b1, b2, b3, b4 = d0 > d3, d1 > d2, d0 > d2, d1 > d3, d2 > d3
    return (b0 & b4).astype(np.uint32) | (((b1 & b2) | (b0 & b3)).astype(np.uint32) << 1)


def sq_dist(co, cg, px, py):
    """glsl:231-235, the reference's operation order"""
    tx, ty = co - px, cg - py
    d = tx * tx + ty * ty
    assert d.dtype == F
    return d


def colour_stage(po, y, u, v):
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

    # the stage's precondition (unchanged by the linear form)
    vx, vy = x1 - x0, y1 - y0
    vv = vx * vx + vy * vy
    e0 = np.maximum(np.maximum(mx_co, x0), x1) - np.minimum(np.minimum(mn_co, x0), x1)
    e1 = np.maximum(np.maximum(mx_cg, y0), y1) - np.minimum(np.minimum(mn_cg, y0), y1)
    dmax = e0 * e0 + e1 * e1
    flat = (mn_co == mx_co) & (mn_cg == mx_cg)
    pre = ((vv >= F(1e-5)) & (vv * F(256.0) > dmax)) | flat
    pad = (-bw) % 64   # UYVY: one block per lane, a wave is 64 consecutive blocks of a block row
    wave_pre = np.concatenate([pre, np.ones((bh, pad), bool)], axis=1).reshape(bh, -1, 64).all(-1)
    in_fast = np.repeat(wave_pre, 64, axis=1)[:, :bw]

    with np.errstate(all="ignore"):
        # location: one projection per pair, row from float bits (zone = RN(clamp(3 s - 1/2, 0, 2)))
        inv = F(1.5) * (F(1.0) / vv)
        ka, kb = vx * inv, vy * inv
        kc = fma(-x0, ka, fma(-y0, kb, F(-0.25)))
        co_e, cg_e = co[..., 0::2], cg[..., 0::2]
        s = np.clip(fma(co_e, ka[..., None], fma(cg_e, kb[..., None], kc[..., None])), F(0), F(1))
        zone = np.nan_to_num(np.rint(s.astype(D) * 2.0)).astype(np.intp)   # (bh, bw, 8); a NaN (vv == 0) clamps to 0 on the GPU
        # rows: (m.x, m.y, c) per zone
        rows = []
        for a, b in ZONE_PAIRS:
            mx, my, sx, sy = px[a] - px[b], py[a] - py[b], px[a] + px[b], py[a] + py[b]
            rows.append((mx, my, F(0.5) * fma(mx, sx, my * sy)))
        pick = lambda k: np.take_along_axis(np.stack([r[k] for r in rows], -1), zone, -1)
        L32 = fma(-co_e, pick(0), fma(-cg_e, pick(1), pick(2)))
        assert L32.dtype == F
        # the same in float64 from the fp32 palette: half of |p - A|^2 - |p - B|^2
        pal = lambda p, k: np.take_along_axis(np.stack([p[a_b[k]] for a_b in ZONE_PAIRS], -1).astype(D), zone, -1)
        ax, ay, bx, by = pal(px, 0), pal(py, 0), pal(px, 1), pal(py, 1)
        L64 = (bx - ax) * (co_e.astype(D) - (ax + bx) / 2) + (by - ay) * (cg_e.astype(D) - (ay + by) / 2)
        eps = fma(dmax, EPS_DMAX, EPS_VV * np.sqrt(vv))
        assert eps.dtype == F

        # the reference's open comparison for every pixel, in the pair's zone
        zone_px = np.repeat(zone, 2, axis=-1)
        pal32 = lambda p, k: np.take_along_axis(np.stack([p[a_b[k]] for a_b in ZONE_PAIRS], -1), zone_px, -1)
        bit = sq_dist(co, cg, pal32(px, 0), pal32(py, 0)) > sq_dist(co, cg, pal32(px, 1), pal32(py, 1))
        fast_idx = np.choose(zone_px, [2 * bit, 2 + bit, 1 + 2 * bit]).astype(np.uint32)
        d = [sq_dist(co, cg, px[k][..., None], py[k][..., None]) for k in range(4)]
        full_idx = palette_index(*d)
        flat_idx = np.broadcast_to(full_idx[..., :1], full_idx.shape)
    idx = np.where(in_fast[..., None], np.where(flat[..., None], flat_idx, fast_idx), full_idx)
    want = (w_idx[..., None] >> (2 * np.arange(16, dtype=np.uint32))) & 3
    return {"idx": idx, "want": want, "L32": L32, "L64": L64, "eps": eps, "bit": bit, "flat": flat, "pre": pre, "in_fast": in_fast,
            "vv": vv, "dmax": dmax}


def certified_blocks(s):
    """the kernel's certificate, per block: the least |L| of the eight pairs against eps, or flat"""
    return (np.abs(s["L32"]).min(-1) > s["eps"]) | s["flat"]


def wave_share_uncertified(s):
    """share of waves (64 consecutive blocks of a block row, UYVY's one block per lane) that reach the linear form and hold an uncertified
    block: the waves ug_hip_dxt_encode_stats_ex counts in counts[3]"""
    bad = ~certified_blocks(s) & s["in_fast"]
    bh, bw = bad.shape
    bad = np.concatenate([bad, np.zeros((bh, (-bw) % 64), bool)], axis=1).reshape(bh, -1, 64)
    return float(bad.any(-1).mean())


def contents():
    from ultragrid_amd import synth
    out = {"S2": uyvy_planes(synth.s2_video("UYVY", 3840, 512, salt=100), 3840, 512),
           "S1": uyvy_planes(synth.s1_random("UYVY", 3840, 512, salt=3), 3840, 512)}
    out.update(frames_for(512, 32))
    return out


@pytest.fixture(scope="module")
def stages(po):
    return {name: colour_stage(po, *planes) for name, planes in contents().items()}


def test_content_is_what_the_issue_names(stages):
    assert len(stages) == 8 and stages["S2"]["idx"].shape == (128, 960, 16) and stages["sixths_extreme_luma"]["L32"].shape == (8, 128, 8)


def test_restatement_gives_the_oracles_indices(stages):
    for name, s in stages.items():
        wrong = int((s["idx"] != s["want"]).sum())
        print(f"{name}: {wrong} of {s['idx'].size} colour indices differ from the oracle's; {100 * s['in_fast'].mean():.1f} % of blocks in the fast stage")
        assert wrong == 0, (name, wrong)


def test_certified_pairs_decide_as_the_reference(stages):
    for name, s in stages.items():
        live = (s["in_fast"] & ~s["flat"])[..., None]
        c = live & (np.abs(s["L32"]) > s["eps"][..., None])
        mine = s["L32"] > 0
        wrong = c & ((mine != s["bit"][..., 0::2]) | (mine != s["bit"][..., 1::2]))
        # the uncertified ones that would have decided otherwise: what the certificate is for
        miss = live & ~c & ((mine != s["bit"][..., 0::2]) | (mine != s["bit"][..., 1::2]))
        print(f"{name}: {int(c.sum())} of {int(live.sum()) * 8} pairs certified, {int(wrong.sum())} of them decide otherwise than the reference; "
              f"{int(miss.sum())} uncertified pairs would")
        assert not wrong.any(), (name, int(wrong.sum()))


def test_distance_between_the_forms_is_within_a_quarter_of_eps(stages):
    for name, s in stages.items():
        live = s["in_fast"] & ~s["flat"]
        if not live.any():
            print(f"{name}: no block reaches the linear form")
            continue
        d = np.abs(s["L32"].astype(D) - s["L64"])[live]
        worst = float((d / s["eps"].astype(D)[live][:, None]).max())
        print(f"{name}: max |L32 - L64| / eps = {worst:.4g}")
        assert worst <= 0.25, (name, worst)


def test_video_like_frames_are_certified_almost_everywhere(stages):
    """a cap, so that this file cannot pass with the shortcut never taken: 4.5 % of the waves of this frame hold an uncertified block"""
    share = wave_share_uncertified(stages["S2"])
    blocks = float((~certified_blocks(stages["S2"]) & stages["S2"]["in_fast"]).mean())
    print(f"S2: {100 * blocks:.4f} % of blocks, {100 * share:.3f} % of waves uncertified; S1: {100 * wave_share_uncertified(stages['S1']):.3f} % of waves")
    for name in list(stages)[2:]:
        print(f"{name}: {100 * wave_share_uncertified(stages[name]):.1f} % of waves uncertified, {100 * (1 - stages[name]['in_fast'].mean()):.1f} % of blocks in the full form")
    assert share < 0.10, share
