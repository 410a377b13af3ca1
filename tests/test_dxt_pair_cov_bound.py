"""From a 4:2:2 source the DXT5-YCoCg encoder takes the SIGN of SelectYCoCgDiagonal's covariance from one product per chroma pair
(dxt_encode.hip, UG_DXT_PAIR_COV): rough = the fma sum of tx ty over the eight EVEN pixels of the block, half of the reference's 16-term
sum up to an error the kernel's comment bounds by eps = 1e-5 (hx + hy + hx hy); a block with |2 rough| > eps, or with an exactly flat
chroma axis, is certified, every other block gets the reference's sum.  This restates the stage in strict numpy.float32, one IEEE operation
per statement (conversion statements as tests/test_dxt_pair_chroma_bound.py writes them), and checks over video-like, random and seam
content that (a) every certified block decides as the reference does, (b) the distance between the two sums stays under eps / 4, and
(c) the certificate is not vacuous: all but a few waves of a video-like frame are certified."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dxt_pair_chroma_bound import F, K_INV255, ycocg_of_pair  # noqa: E402
from test_gpu_dxt_pair_zone import frames_for  # noqa: E402

EPS_K = 1e-5   # the kernel compares |rough| with EPS_K / 2 * fma(hx, hy, hx + hy)


def pad_planes(y, u, v):
    """the picture as the encoder reads it when width or height is no multiple of 4: lines past the picture repeat the last line; in the
    block cut by the right edge (width = 2 mod 4) the missing pair repeats the last pixel, Y1 under its pair's chroma"""
    h, w = y.shape
    assert w % 2 == 0 and u.shape == v.shape == (h, w // 2)
    if w % 4:
        y = np.concatenate([y, y[:, -1:], y[:, -1:]], axis=1)
        u = np.concatenate([u, u[:, -1:]], axis=1)
        v = np.concatenate([v, v[:, -1:]], axis=1)
    if h % 4:
        n = 4 - h % 4
        y, u, v = (np.concatenate([p] + [p[-1:]] * n, axis=0) for p in (y, u, v))
    return y, u, v


def uyvy_planes(buf, w, h):
    b = buf.reshape(h, w // 2, 4)
    y = np.empty((h, w), np.uint8)
    y[:, 0::2] = b[..., 1]; y[:, 1::2] = b[..., 3]
    return y, b[..., 0], b[..., 2]


def diagonal_stage(y, u, v):
    """bytes (y: (h, w), u / v: (h, w / 2)) -> per 4 x 4 block, arrays of shape (h / 4, w / 4): the reference's cov (fp32, sequential),
    the kernel's rough sum in fp32 and in float64, hx, hy (fp32)"""
    y, u, v = pad_planes(y, u, v)
    h, w = y.shape
    to_float = lambda b: b.astype(F) * K_INV255
    co0, cg0, co1, cg1 = ycocg_of_pair(to_float(y[:, 0::2]), to_float(y[:, 1::2]), to_float(u), to_float(v))
    co = np.empty((h, w), F); cg = np.empty((h, w), F)
    co[:, 0::2] = co0; co[:, 1::2] = co1; cg[:, 0::2] = cg0; cg[:, 1::2] = cg1

    def blocks(p):  # -> (bh, bw, 16), pixel i = 4 row + column
        return p.reshape(h // 4, 4, w // 4, 4).transpose(0, 2, 1, 3).reshape(h // 4, w // 4, 16)
    co, cg = blocks(co), blocks(cg)
    mn_co, mx_co, mn_cg, mx_cg = co.min(-1), co.max(-1), cg.min(-1), cg.max(-1)
    midx, midy = (mx_co + mn_co) * F(0.5), (mx_cg + mn_cg) * F(0.5)
    tx, ty = co - midx[..., None], cg - midy[..., None]
    assert tx.dtype == F and ty.dtype == F
    cov = np.zeros(midx.shape, F)
    for i in range(16):
        cov = cov + tx[..., i] * ty[..., i]
    assert cov.dtype == F
    # fma(tx, ty, rough): the product of two fp32 is exact in float64; the sum is rounded to float64, then to fp32 (where that differs
    # from the one rounding of a true fma it does so by one fp32 ulp of the sum: far inside what (a) and (b) leave)
    rough32 = np.zeros(midx.shape, F)
    rough64 = np.zeros(midx.shape, np.float64)
    for i in range(0, 16, 2):
        prod = tx[..., i].astype(np.float64) * ty[..., i].astype(np.float64)
        rough32 = (prod + rough32.astype(np.float64)).astype(F)
        rough64 = rough64 + prod
    return {"cov": cov, "rough32": rough32, "rough64": rough64, "hx": mx_co - mn_co, "hy": mx_cg - mn_cg}


def eps_of(s):
    hx, hy = s["hx"].astype(np.float64), s["hy"].astype(np.float64)
    return EPS_K * (hx + hy + hx * hy)


def certified(s, rough="rough32"):
    """the kernel's certificate, its own fp32 statements for rough32"""
    hx, hy = s["hx"], s["hy"]
    if rough == "rough32":
        bound = F(0.5 * EPS_K) * ((hx.astype(np.float64) * hy.astype(np.float64) + (hx + hy).astype(np.float64)).astype(F))
        return (np.abs(s[rough]) > bound) | (hx * hy == 0)
    return (np.abs(s[rough]) > 0.5 * eps_of(s)) | (hx * hy == 0)


def wave_share_uncertified(s):
    """share of waves (64 consecutive blocks of a block row, UYVY's one block per lane) that hold an uncertified block"""
    c = certified(s)
    bh, bw = c.shape
    pad = (-bw) % 64
    c = np.concatenate([c, np.ones((bh, pad), bool)], axis=1).reshape(bh, -1, 64)
    return float((~c.all(-1)).mean())


def contents():
    from ultragrid_amd import synth
    out = {"S2": uyvy_planes(synth.s2_video("UYVY", 3840, 512, salt=100), 3840, 512),
           "S1": uyvy_planes(synth.s1_random("UYVY", 3840, 512, salt=3), 3840, 512)}
    out.update(frames_for(512, 32))
    return out


@pytest.fixture(scope="module")
def stages():
    return {name: diagonal_stage(*planes) for name, planes in contents().items()}


def test_content_is_what_the_issue_names(stages):
    assert len(stages) == 8 and stages["S2"]["cov"].shape == (128, 960) and stages["sixths_extreme_luma"]["cov"].shape == (8, 128)


@pytest.mark.parametrize("rough", ["rough32", "rough64"])
def test_certified_blocks_decide_as_the_reference(stages, rough):
    for name, s in stages.items():
        c = certified(s, rough)
        wrong = c & ((s[rough] < 0) != (s["cov"] < 0))
        print(f"{name}: {int(c.sum())} of {c.size} blocks certified ({rough}), {int(wrong.sum())} of them decide otherwise than the reference")
        assert not wrong.any(), (name, rough, int(wrong.sum()))


@pytest.mark.parametrize("rough", ["rough32", "rough64"])
def test_distance_between_the_sums_is_within_a_quarter_of_eps(stages, rough):
    for name, s in stages.items():
        d = np.abs(2.0 * s[rough].astype(np.float64) - s["cov"].astype(np.float64))
        eps = eps_of(s)
        flat = eps == 0   # one chroma value in the block: both sums are exactly 0
        assert not d[flat].any()
        worst = float((d[~flat] / eps[~flat]).max()) if (~flat).any() else 0.0
        print(f"{name}: max |2 rough - cov| / eps = {worst:.4g} ({rough})")
        assert worst <= 0.25, (name, rough, worst)


def test_video_like_frames_are_certified_almost_everywhere(stages):
    """a cap, so that this file cannot pass with the shortcut never taken: 0.62 % of the waves of this frame hold an uncertified block"""
    share = wave_share_uncertified(stages["S2"])
    blocks = float((~certified(stages["S2"])).mean())
    print(f"S2: {100 * blocks:.4f} % of blocks, {100 * share:.3f} % of waves uncertified; S1: {100 * wave_share_uncertified(stages['S1']):.3f} % of waves")
    assert share < 0.02, share
