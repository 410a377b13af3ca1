"""The DXT5-YCoCg colour stage locates a 4:2:2 pixel pair on the palette segment ONCE, from its even pixel (dxt_encode.hip,
UG_DXT_PAIR_ZONE).  That rests on a bound: the Co / Cg of the two pixels of a pair -- which share U and V and differ in luma only --
differ by rounding alone.  The kernel's comment uses |dCo|, |dCg| < 5e-7; this recomputes both pixels with the kernel's statements
(yuv_pair_to_rgb, then ConvertRGBToYCoCg as encode_dxt5ycocg writes it) in strict numpy.float32, one IEEE operation per statement,
over EVERY (U, V) and a fixed set of luma pairs that holds the extremes, for UYVY bytes and for the v210 sample path."""
import numpy as np

# The figure of the kernel's derivation comment (3.5 * 2^-23 and 4 * 2^-23 by rounding analysis).  With the stage's precondition vv >= 1e-5
# it moves the projection by at most BOUND * sqrt(2) / sqrt(1e-5) < 2.3e-4 of the segment, against a margin of 1/12.
BOUND = 5e-7
F = np.float32
K_INV255 = F(0.00392156862745)
K_OFFSET = F(128.0 / 255.0)


def fma(a, b, c):
    """the kernel's __builtin_fmaf(a, b, c) for b a power of two: a * b is exact in fp32, so the fused form and this two-step form
    round once, alike (the argument of the kernel's own comment on these statements)"""
    assert float(b) in (2.0, 0.5, 0.25)
    return (a * F(b) + c).astype(F)


def ycocg_of_pair(y0, y1, u, v):
    """bytes / 255 -> (Co0, Cg0, Co1, Cg1), statements of yuv_pair_to_rgb and of encode_dxt5ycocg's conversion loop"""
    U, V = u - F(0.5), v - F(0.5)
    rv, gu, gv, bu = F(1.7926) * V, F(0.2132) * U, F(0.5328) * V, F(2.1124) * U
    out = []
    for y in (y0, y1):
        Y = F(1.1643) * (y - F(0.0625))
        r, g, b = Y + rv, (Y - gu) - gv, Y + bu
        co = fma(r - b, 0.5, K_OFFSET)
        cg = fma(fma(g, 2.0, -r) - b, 0.25, K_OFFSET)
        out += [co, cg]
        assert co.dtype == F and cg.dtype == F
    return out


def luma_pairs():
    rng = np.random.default_rng(422)
    fixed = [(0, 255), (255, 0), (16, 235), (235, 16), (1, 254), (254, 1), (0, 0), (255, 255), (0, 1), (127, 128), (16, 16), (235, 235)]
    rnd = [tuple(int(x) for x in rng.integers(0, 256, 2)) for _ in range(55)]
    return fixed + rnd


def max_pair_difference(to_float):
    """to_float: byte-valued integer array -> the float the loader hands to yuv_pair_to_rgb"""
    uu, vv = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    u, v = to_float(uu.ravel()), to_float(vv.ravel())
    worst_co = worst_cg = 0.0
    for y0, y1 in luma_pairs():
        co0, cg0, co1, cg1 = ycocg_of_pair(to_float(np.array([y0])), to_float(np.array([y1])), u, v)
        worst_co = max(worst_co, float(np.abs(co0.astype(np.float64) - co1.astype(np.float64)).max()))
        worst_cg = max(worst_cg, float(np.abs(cg0.astype(np.float64) - cg1.astype(np.float64)).max()))
    return worst_co, worst_cg


def test_uyvy_pair_chroma_differs_by_rounding_only():
    # LoaderUYVYTyped / LoaderUYVY: float(byte) * kInv255
    co, cg = max_pair_difference(lambda b: b.astype(F) * K_INV255)
    print(f"UYVY: max |dCo| = {co:.4g}, max |dCg| = {cg:.4g} (bound {BOUND:g})")
    assert co <= BOUND and cg <= BOUND, (co, cg)


def test_v210_pair_chroma_differs_by_rounding_only():
    """Loader<UG_PF_V210>::samp keeps the top 8 bits of a 10-bit sample, three samples to a word: (w >> (10 k + 2)) & 0xff.  The values
    it hands to yuv_pair_to_rgb are therefore the bytes again -- the bound is the UYVY one by construction -- and what this adds is the
    extraction itself: every byte, at each of the three positions of a word, under every value of the two dropped bits and with the
    neighbouring samples all ones, comes back as that byte."""
    def samp(b, k, low):
        word = np.uint32(0x3FFFFFFF) & ~np.uint32(0x3FF << (10 * k)) | ((b.astype(np.uint32) << 2 | np.uint32(low)) << np.uint32(10 * k))
        return ((word >> np.uint32(10 * k + 2)) & np.uint32(0xFF))
    every = np.arange(256)
    for k in range(3):
        for low in range(4):
            assert np.array_equal(samp(every, k, low), every), (k, low)
    co, cg = max_pair_difference(lambda b: samp(b, 1, 3).astype(F) * K_INV255)
    print(f"v210: max |dCo| = {co:.4g}, max |dCg| = {cg:.4g} (bound {BOUND:g})")
    assert co <= BOUND and cg <= BOUND, (co, cg)
