"""encode_dxt5ycocg folds the reference's products by powers of two into the fma of the neighbouring sum and keeps the luma at
Y4 = r + 2 g + b = 4 Y through the alpha stage (dxt_encode.hip, UG_DXT_POW2_FOLD).  That is exact as long as no such product underflows.
This restates both forms in strict numpy.float32, one IEEE operation per statement -- fma() below rounds once, by way of float64 --
and compares BIT PATTERNS:
  * the floor: over every (y, u, v) byte triple of the YUV front ends and every (r, g, b) of the RGB ones, a non-zero |t + b| is never
    below 2^-100, so the deleted * 0.25 never met a denormal.  The minimum found is 3 * 2^-28 = 1.118e-08 for YUV and 1 / 255 = 3.922e-03
    for RGB;
  * the dequantised end points, for every code and every scale;
  * the box ends, the six thresholds of the 4 x domain (= 4 x the reference's) and every pixel-against-threshold comparison, the chroma
    end points and the three insets, over video-like and random frames and over blocks built for the seams: luma range on both sides
    of 2^-10, ends that clamp at 0 and at 1."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dxt_pair_cov_bound import pad_planes, uyvy_planes  # noqa: E402

F = np.float32
K_INV255 = F(0.00392156862745)
K_OFFSET = F(128.0 / 255.0)
K_INSET_C = F((8.0 / 255.0) / 16.0)
K_INSET_Y = F((16.0 / 255.0) / 32.0)
INV7 = F(1.0 / 7.0)
INV255 = F(1.0 / 255.0)
ALL_WIDE = F(0.0009765625)   # the kernel's wave test: range > 2^-10


def fma(a, b, c):
    """__builtin_fmaf(a, b, c), one rounding: the product of two fp32 is exact in float64, and the float64 sum of that product and an fp32
    addend, rounded again to fp32, equals the single rounding whenever the product itself fits fp32 (53 >= 2 * 24 + 2 bits: the double
    rounding of a sum is innocuous) -- which is every product here: one factor is a power of two.  Unlike a * b + c in fp32 it does NOT
    round or flush the product first, so a product that left fp32's normal range would show as a difference."""
    a, b, c = (np.asarray(x, F).astype(np.float64) for x in (a, b, c))
    return (a * b + c).astype(F)


def bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def to_float(b):
    return np.asarray(b).astype(F) * K_INV255


def yuv_to_rgb(y, u, v):
    """yuv_pair_to_rgb / Loader3<true>::block, per pixel"""
    U, V = u - F(0.5), v - F(0.5)
    Y = F(1.1643) * (y - F(0.0625))
    return Y + F(1.7926) * V, (Y - F(0.2132) * U) - F(0.5328) * V, Y + F(2.1124) * U


def ycocg4(r, g, b):
    """ConvertRGBToYCoCg as encode_dxt5ycocg writes it, the luma left at Y4 = t + b (the reference's Y is Y4 * 0.25)"""
    y4 = fma(g, 2.0, r) + b
    co = fma(r - b, 0.5, K_OFFSET)
    cg = fma(fma(g, 2.0, -r) - b, 0.25, K_OFFSET)
    assert y4.dtype == F and co.dtype == F and cg.dtype == F
    return y4, co, cg


def clamp01(v):
    return np.minimum(F(1.0), np.maximum(F(0.0), v))


# ---------------------------------------------------------------------------------------------------------------------------------
# the floor
# ---------------------------------------------------------------------------------------------------------------------------------
def test_no_luma_sum_is_near_the_denormals():
    uu, vv = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    u, v = to_float(uu.ravel()), to_float(vv.ravel())
    least = {"YUV": np.inf, "RGB": np.inf}
    for first in range(256):
        y4, _, _ = ycocg4(*yuv_to_rgb(to_float(np.array([first])), u, v))
        y4r, _, _ = ycocg4(to_float(np.array([first])), u, v)   # (r, g, b) = (first, uu, vv)
        for name, s in (("YUV", y4), ("RGB", y4r)):
            m = np.abs(s[s != 0])
            least[name] = min(least[name], float(m.min())) if m.size else least[name]
            assert same(s * F(0.25) * F(4.0), s)   # and the reference's own * 0.25 was exact, every time
    print(f"smallest non-zero |t + b|: YUV {least['YUV']:.4g} = 2^{np.log2(least['YUV']):.2f}, RGB {least['RGB']:.4g}")
    assert least["YUV"] >= 2.0 ** -100 and least["RGB"] >= 2.0 ** -100, least
    assert least["YUV"] == 3 * 2.0 ** -28 and abs(least["RGB"] - 1.0 / 255.0) < 1e-9, least   # the figures of the docstring


# ---------------------------------------------------------------------------------------------------------------------------------
# dequantised end points
# ---------------------------------------------------------------------------------------------------------------------------------
def test_dequantised_end_points_for_every_code_and_scale():
    five, six = np.arange(32), np.arange(64)
    codes = np.concatenate([(five << 3) | (five >> 2), (six << 2) | (six >> 4)])
    n = 0
    for rfs in (1.0, 0.5, 0.25):
        d = codes.astype(F) * INV255 - K_OFFSET
        ref = d * F(rfs) + K_OFFSET
        assert ref.dtype == F and same(ref, fma(d, rfs, K_OFFSET)), rfs
        n += codes.size
    assert n == 288


# ---------------------------------------------------------------------------------------------------------------------------------
# the stages over block content
# ---------------------------------------------------------------------------------------------------------------------------------
def blocks_of(p):
    h, w = p.shape
    return p.reshape(h // 4, 4, w // 4, 4).transpose(0, 2, 1, 3).reshape(h // 4, w // 4, 16)


def ycocg_blocks_yuv(y, u, v):
    """4:2:2 byte planes (y: (h, w), u / v: (h, w / 2)) -> Y4, Co, Cg per block, (bh, bw, 16), as the encoder reads a cut picture"""
    y, u, v = pad_planes(y, u, v)
    r, g, b = yuv_to_rgb(to_float(y), to_float(np.repeat(u, 2, axis=1)), to_float(np.repeat(v, 2, axis=1)))
    return tuple(blocks_of(p) for p in ycocg4(r, g, b))


def ycocg_blocks_rgb(rgb):
    """(h, w, 3) bytes, h and w multiples of 4"""
    return tuple(blocks_of(p) for p in ycocg4(to_float(rgb[..., 0]), to_float(rgb[..., 1]), to_float(rgb[..., 2])))


def alpha_stage(y4):
    """(..., 16) of Y4 -> the reference's statements on Y = Y4 / 4 and the kernel's on Y4"""
    y = y4 * F(0.25)
    mn, mx = y.min(-1), y.max(-1)
    inset = (mx - mn) * F(0.03125) - K_INSET_Y
    mn, mx = clamp01(mn + inset), clamp01(mx - inset)
    rng = mx - mn
    mid = rng / F(14.0)
    ab = [mn + mid] + [(F(8 - k) * mx + F(k - 1) * mn) * INV7 + mid for k in range(2, 8)]
    # the kernel
    mn4, mx4 = y4.min(-1), y4.max(-1)
    inset_k = fma(mx4 - mn4, 0.0078125, -K_INSET_Y)
    mn_k, mx_k = clamp01(fma(mn4, 0.25, inset_k)), clamp01(fma(mx4, 0.25, -inset_k))
    mid_k = (mx_k - mn_k) / F(14.0)
    ab4 = [fma(mid_k, 4.0, mn_k * F(4.0))]
    for k in range(2, 8):
        cx, cn = F(4 * (8 - k)), F(4 * (k - 1))
        s = fma(mn_k, cn, cx * mx_k) if (k <= 3 or k == 5) else fma(mx_k, cx, cn * mn_k)
        ab4.append(fma(mid_k, 4.0, s * INV7))
    for a in ab + ab4 + [inset, mn, mx]:
        assert a.dtype == F
    return {"y": y, "y4": y4, "inset": inset, "inset_k": inset_k, "mn": mn, "mx": mx, "mn_k": mn_k, "mx_k": mx_k, "range": rng, "ab": ab, "ab4": ab4}


def scale_of(co, cg):
    """ScaleYCoCg's float(scale) per block"""
    m = np.maximum(np.maximum(np.abs(co.min(-1) - K_OFFSET), np.abs(cg.min(-1) - K_OFFSET)),
                   np.maximum(np.abs(co.max(-1) - K_OFFSET), np.abs(cg.max(-1) - K_OFFSET)))
    return np.where(m < F(32.0 / 255.0), F(4.0), np.where(m < F(64.0 / 255.0), F(2.0), F(1.0))).astype(F)


def chroma_ends(mx, mn, fs):
    """the end points and inset of one chroma axis in both forms -> [(reference, kernel), ...]"""
    a, b = (mx - K_OFFSET) * fs + K_OFFSET, (mn - K_OFFSET) * fs + K_OFFSET
    ak, bk = fma(mx - K_OFFSET, fs, K_OFFSET), fma(mn - K_OFFSET, fs, K_OFFSET)
    assert a.dtype == F and b.dtype == F
    return [(a, ak), (b, bk), ((a - b) * F(0.0625) - K_INSET_C, fma(ak - bk, 0.0625, -K_INSET_C))]


def luma_seam_blocks():
    """constant 4:2:2 blocks (y, u, v) whose luma box, after the inset, has both ends at or next to a clamp: -> dict of (n, 3) byte triples,
    `below` / `above`: 0 < range <= 2^-10 and 2^-10 < range < 2^-9 (either side of the wave test of the fast alpha stage), found by
    enumeration near luma 16 (bottom clamp) and luma 235 (top clamp); `zero`: both ends clamp to the same bound (bytes 0-4 and 251-255)"""
    ys = np.concatenate([np.arange(0, 24), np.arange(228, 256)])
    y, u, v = (a.ravel() for a in np.meshgrid(ys, np.arange(112, 145), np.arange(112, 145), indexing="ij"))
    y4, _, _ = ycocg4(*yuv_to_rgb(to_float(y), to_float(u), to_float(v)))
    s = alpha_stage(np.repeat(y4[:, None], 16, axis=1))
    t = np.stack([y, u, v], axis=1)
    rng = s["range"]
    out = {"below": t[(rng > 0) & (rng <= ALL_WIDE)], "above": t[(rng > ALL_WIDE) & (rng < 2 * ALL_WIDE)],
           "zero": t[(rng == 0) & ((y <= 4) | (y >= 251))]}
    for name, a in out.items():
        assert len(a) >= 8 and (a[:, 0] < 128).any() and (a[:, 0] > 128).any(), (name, len(a))   # both clamps in every class
    return out


def seam_frame(w, h, salt=0):
    """4:2:2 planes of w x h: every block row holds, in both halves of its width, constant blocks of the three classes above, blocks of random
    luma bytes in 0-4, in 251-255 and in both (ends that clamp at 0, at 1, at both), and ordinary blocks -- except block rows 4 and 5
    (where there are that many), which hold no block at or under the wave test: their waves stay in the fast alpha stage"""
    rng = np.random.default_rng(2400 + w + salt)
    bw, bh = (w + 3) // 4, (h + 3) // 4
    yb, ub, vb = rng.integers(16, 236, (bh, bw, 4, 4)), rng.integers(96, 160, (bh, bw, 4, 2)), rng.integers(96, 160, (bh, bw, 4, 2))
    pool = luma_seam_blocks()
    low, high = np.arange(0, 5), np.arange(251, 256)
    for by in range(bh):
        for bx in range(bw):
            kind = (bx + 3 * by) % 8
            wide_only = by in (4, 5)
            if kind == 0 and not wide_only:
                t = pool["below"][rng.integers(len(pool["below"]))]
            elif kind == 1:
                t = pool["above"][rng.integers(len(pool["above"]))]
            elif kind == 2 and not wide_only:
                t = pool["zero"][rng.integers(len(pool["zero"]))]
            else:
                t = None
            if t is not None:
                yb[by, bx], ub[by, bx], vb[by, bx] = t[0], t[1], t[2]
            elif kind == 3 and not wide_only:
                yb[by, bx] = low[rng.integers(0, 5, (4, 4))]
            elif kind == 4 and not wide_only:
                yb[by, bx] = high[rng.integers(0, 5, (4, 4))]
            elif kind == 5:
                yb[by, bx] = np.concatenate([low, high])[rng.integers(0, 10, (4, 4))]
    y = yb.transpose(0, 2, 1, 3).reshape(4 * bh, 4 * bw)[:h, :w]
    u = ub.transpose(0, 2, 1, 3).reshape(4 * bh, 2 * bw)[:h, : w // 2]
    v = vb.transpose(0, 2, 1, 3).reshape(4 * bh, 2 * bw)[:h, : w // 2]
    return tuple(np.ascontiguousarray(p.astype(np.uint8)) for p in (y, u, v))


@pytest.fixture(scope="module")
def content():
    """name -> (Y4, Co, Cg) per block"""
    from ultragrid_amd import synth
    out = {"S2": ycocg_blocks_yuv(*uyvy_planes(synth.s2_video("UYVY", 512, 64, salt=100), 512, 64)),
           "S1": ycocg_blocks_yuv(*uyvy_planes(synth.s1_random("UYVY", 512, 64, salt=3), 512, 64)),
           "S1_rgb": ycocg_blocks_rgb(synth.s1_random("RGB", 512, 64, salt=4).reshape(64, 512, 3)),
           "seams": ycocg_blocks_yuv(*seam_frame(512, 64)),
           "seams_cut": ycocg_blocks_yuv(*seam_frame(510, 30))}
    for name, tri in luma_seam_blocks().items():   # every block of the enumeration, not only the ones a frame drew
        y4, co, cg = ycocg4(*yuv_to_rgb(*(to_float(tri[:, k]) for k in range(3))))
        out["pool_" + name] = tuple(np.repeat(p[None, :, None], 16, axis=2) for p in (y4, co, cg))
    return out


def test_content_holds_the_seams(content):
    s = alpha_stage(content["seams"][0])
    rng = s["range"]
    assert ((rng > 0) & (rng <= ALL_WIDE)).sum() >= 20 and ((rng > ALL_WIDE) & (rng < 2 * ALL_WIDE)).sum() >= 20 and (rng == 0).sum() >= 20
    assert ((s["mn"] == 0) & (s["mx"] == 1)).sum() >= 20 and ((s["mn"] == 0) & (s["mx"] < 1)).sum() >= 20 and ((s["mn"] > 0) & (s["mx"] == 1)).sum() >= 20
    assert (rng[4:6] > ALL_WIDE).all()
    assert content["S2"][0].shape == (16, 128, 16)


def test_box_ends_thresholds_and_comparisons(content):
    for name, (y4, _, _) in content.items():
        s = alpha_stage(y4)
        assert same(s["inset"], s["inset_k"]) and same(s["mn"], s["mn_k"]) and same(s["mx"], s["mx_k"]), name
        moved = 0
        for k in range(7):
            assert same(s["ab4"][k], s["ab"][k] * F(4.0)), (name, k + 1)   # * 4 of an fp32 below 2 is exact
            moved += int(((s["y4"] <= s["ab4"][k][..., None]) != (s["y"] <= s["ab"][k][..., None])).sum())
        print(f"{name}: {s['mn'].size} blocks, {moved} comparisons decide otherwise in the 4 x domain")
        assert moved == 0, (name, moved)


def test_chroma_end_points_and_insets(content):
    for name, (_, co, cg) in content.items():
        real = scale_of(co, cg)
        assert name != "S2" or len(np.unique(real)) == 3   # a video-like frame takes every scale
        for fs in (real, F(1.0), F(2.0), F(4.0)):
            # Cg in both orders: the diagonal may have swapped its ends
            for mx, mn in ((co.max(-1), co.min(-1)), (cg.max(-1), cg.min(-1)), (cg.min(-1), cg.max(-1))):
                for ref, ker in chroma_ends(mx, mn, fs):
                    assert same(ref, ker), (name, float(np.max(fs)))
