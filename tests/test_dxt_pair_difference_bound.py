"""From a 4:2:2 source the DXT5-YCoCg encoder keeps the chroma of a pixel as the differences the reference forms on its way to Co / Cg
(dxt_encode.hip, encode_dxt5ycocg, the chroma-pair side):  d = r - b,  e = fma(g, 2, -r) - b,  Co = fma(d, 1/2, off),  Cg = fma(e, 1/4, off).
The box is taken over d and e and its four ends go through the two maps; the diagonal's rough sum and the colour stage's projection take d
and e of the even pixels as they are, with the 1/2, 1/4 and off folded into their constants; only the reference-form sides form Co / Cg per
pixel.  This restates that in strict numpy.float32, one IEEE operation per statement (conversion statements as
tests/test_dxt_pair_chroma_bound.py writes them, fma through one float64 product and sum rounded once as tests/test_dxt_pair_linear_bound.py
does), over the video-like and the random 3840 x 512 frame and the seam frames of the pair location, and checks that
(1) the ends f(min d), f(max d) are min f(d), max f(d) bit for bit on every block, and f is monotone over EVERY d and e a (y, u, v) of bytes
    gives (so over every pair of pixels a block can hold),
(2) the projection from (d, e) stays within eps / 4 of the float64 projection of the reference's fp32 Co / Cg for BOTH pixels of every pair,
    no certified pair decides otherwise than the oracle for either pixel, and at most 0.12 of the waves of the video-like frame hold an
    uncertified block,
(3) rough / 4 (the sum over the even pixels in the difference domain is 8 x the one in Co / Cg) stays within eps / 4 of the reference's
    16-term covariance where the block is certified, and no certified block decides the swap otherwise than the reference,
(4) blocks exist whose Co is exactly flat while d is not, with a negative rough sum -- found by enumeration over (u, v, y) -- and on them
    the rule `swap = rough < 0 and hx != 0` gives the reference's ends where `rough < 0` alone does not."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dxt_pair_chroma_bound import F, K_INV255, K_OFFSET, ycocg_of_pair  # noqa: E402
from test_dxt_pair_cov_bound import EPS_K, diagonal_stage, pad_planes  # noqa: E402
from test_dxt_pair_linear_bound import contents, fma  # noqa: E402
from test_dxt_pair_projection_bound import EPS_DIAG, EPS_DMAX, EPS_SEG, J_TO_INDEX, WAVE_SHARE_CAP  # noqa: E402
from test_gpu_dxt_pair_zone import pack_uyvy  # noqa: E402

D = np.float64
EPS_ABS = 1.5e-12   # the absolute part of the diagonal's eps (the product of two differences of rounding size), in Co Cg units
HALF, QUARTER = F(0.5), F(0.25)


def co_of(d):
    """fma(d, 1/2, off): the product is exact, one rounding"""
    return (d * HALF + K_OFFSET).astype(F)


def cg_of(e):
    return (e * QUARTER + K_OFFSET).astype(F)


def differences(y, u, v):
    """bytes / 255 of one pixel under its pair's chroma -> (d, e): the statements of yuv_pair_to_rgb and of the conversion's chroma-pair side"""
    U, V = u - F(0.5), v - F(0.5)
    rv, gu, gv, bu = F(1.7926) * V, F(0.2132) * U, F(0.5328) * V, F(2.1124) * U
    Y = F(1.1643) * (y - F(0.0625))
    r, g, b = Y + rv, (Y - gu) - gv, Y + bu
    d = r - b
    e = (g * F(2.0) + (-r)) - b   # fma(g, 2, -r): 2 g is exact
    assert d.dtype == F and e.dtype == F
    return d, e


def block_values(y, u, v):
    """bytes (y: (h, w), u / v: (h, w / 2)) -> d, e, Co, Cg of shape (bh, bw, 16) (pixel i = 4 row + column); Co / Cg are asserted to be
    the reference's own (ycocg_of_pair)"""
    y, u, v = pad_planes(y, u, v)
    h, w = y.shape
    to_float = lambda b: b.astype(F) * K_INV255
    d = np.empty((h, w), F); e = np.empty((h, w), F)
    d[:, 0::2], e[:, 0::2] = differences(to_float(y[:, 0::2]), to_float(u), to_float(v))
    d[:, 1::2], e[:, 1::2] = differences(to_float(y[:, 1::2]), to_float(u), to_float(v))
    co0, cg0, co1, cg1 = ycocg_of_pair(to_float(y[:, 0::2]), to_float(y[:, 1::2]), to_float(u), to_float(v))
    assert np.array_equal(co_of(d[:, 0::2]), co0) and np.array_equal(co_of(d[:, 1::2]), co1)
    assert np.array_equal(cg_of(e[:, 0::2]), cg0) and np.array_equal(cg_of(e[:, 1::2]), cg1)
    blocks = lambda p: p.reshape(h // 4, 4, w // 4, 4).transpose(0, 2, 1, 3).reshape(h // 4, w // 4, 16)
    d, e = blocks(d), blocks(e)
    return d, e, co_of(d), cg_of(e)


def diagonal_model(d, e):
    """the diagonal stage in the difference domain, per block: box ends through the maps, rough over the even pixels, certificate, swap"""
    mn_d, mx_d, mn_e, mx_e = d.min(-1), d.max(-1), e.min(-1), e.max(-1)
    mn_co, mx_co, mn_cg, mx_cg = co_of(mn_d), co_of(mx_d), cg_of(mn_e), cg_of(mx_e)
    hx, hy = mx_co - mn_co, mx_cg - mn_cg
    mid_d, mid_e = (mx_d + mn_d) * HALF, (mx_e + mn_e) * HALF
    tx, ty = d[..., 0::2] - mid_d[..., None], e[..., 0::2] - mid_e[..., None]
    assert tx.dtype == F and ty.dtype == F
    rough32, rough64 = np.zeros(hx.shape, F), np.zeros(hx.shape, D)
    for j in range(8):
        rough32 = fma(tx[..., j], ty[..., j], rough32)
        rough64 = rough64 + tx[..., j].astype(D) * ty[..., j].astype(D)
    bound = fma(fma(hx, hy, hx + hy), F(4.0 * EPS_K), F(4.0 * EPS_ABS))   # 8 x half of eps
    certified = (np.abs(rough32) > bound) | (hx * hy == 0)
    return {"ends": (mn_co, mx_co, mn_cg, mx_cg), "hx": hx, "hy": hy, "rough32": rough32, "rough64": rough64, "certified": certified,
            "swap": (rough32 < 0) & (hx != 0), "swap_without_rule": rough32 < 0}


def eps_diagonal(hx, hy):
    hx, hy = hx.astype(D), hy.astype(D)
    return EPS_K * (hx + hy + hx * hy) + EPS_ABS


def waves(b, fill):
    """(bh, bw) per block -> (bh, waves, 64): UYVY's one block per lane, a wave is 64 consecutive blocks of a block row"""
    bh, bw = b.shape
    return np.concatenate([b, np.full((bh, (-bw) % 64), fill, bool)], axis=1).reshape(bh, -1, 64)


def projection_model(po, y, u, v, d, e, co, cg):
    """the colour stage's projection in the difference domain, per pair, against the palette rebuilt from the oracle's end-point bits (the
    statements of tests/test_dxt_pair_projection_bound.py for the palette, the precondition and eps)"""
    h0, w0 = y.shape
    out = po.dxt_encode(po.IN_UYVY, po.OUT_DXT5YCOCG, pack_uyvy(y, u, v), w0, h0)
    bh, bw = d.shape[:2]
    words = np.ascontiguousarray(out).view("<u4").reshape(bh, bw, 4)
    w_end, w_idx = words[..., 2], words[..., 3]
    c0, c1 = w_end & 0xFFFF, w_end >> 16
    rfs = F(1.0) / ((c0 & 31) + 1).astype(F)
    inv255 = F(1.0 / 255.0)

    def ends(c):
        i0, i1 = (c >> 11) & 31, (c >> 5) & 63
        i0, i1 = (i0 << 3) | (i0 >> 2), (i1 << 2) | (i1 >> 4)
        return [(i.astype(F) * inv255 - K_OFFSET) * rfs + K_OFFSET for i in (i0, i1)]
    (x0, y0), (x1, y1) = ends(c0), ends(c1)
    mn_co, mx_co, mn_cg, mx_cg = co.min(-1), co.max(-1), cg.min(-1), cg.max(-1)
    vx, vy = x1 - x0, y1 - y0
    vv = vx * vx + vy * vy
    e0 = np.maximum(np.maximum(mx_co, x0), x1) - np.minimum(np.minimum(mn_co, x0), x1)
    e1 = np.maximum(np.maximum(mx_cg, y0), y1) - np.minimum(np.minimum(mn_cg, y0), y1)
    dmax = e0 * e0 + e1 * e1
    flat = (mn_co == mx_co) & (mn_cg == mx_cg)
    pre = ((vv >= F(1e-5)) & (vv * F(256.0) > dmax)) | flat
    in_fast = np.repeat(waves(pre, True).all(-1), 64, axis=1)[:, :bw]
    with np.errstate(all="ignore"):
        rvv = F(1.0) / vv
        ka, kb = vx * rvv, vy * rvv
        ka2, kb4 = ka * HALF, kb * QUARTER                          # exact
        kc = fma(K_OFFSET - x0, ka, (K_OFFSET - y0) * kb)           # formed about off, rounded twice
        t32 = fma(d[..., 0::2], ka2[..., None], fma(e[..., 0::2], kb4[..., None], kc[..., None]))
        s = np.nan_to_num(np.clip(t32, F(0), F(1)))
        j = np.rint(s.astype(D) * 3.0)
        dist = fma(s, F(3.0), (-j).astype(F))
        sd = np.sqrt(dmax)
        eps = fma(sd, fma(sd, EPS_DMAX, EPS_DIAG), EPS_SEG * np.sqrt(vv)) * rvv
        cert_pair = np.abs(dist) < (F(0.5) - eps)[..., None]
        vx64, vy64 = vx.astype(D)[..., None], vy.astype(D)[..., None]
        t64 = ((co.astype(D) - x0.astype(D)[..., None]) * vx64 + (cg.astype(D) - y0.astype(D)[..., None]) * vy64) / (vx64 * vx64 + vy64 * vy64)
    want = (w_idx[..., None] >> (2 * np.arange(16, dtype=np.uint32))) & 3
    return {"t32": t32, "t64": t64, "eps": eps, "cert_pair": cert_pair, "cert_block": cert_pair.all(-1) | flat, "flat": flat, "in_fast": in_fast,
            "proj_idx": J_TO_INDEX[j.astype(np.intp)], "want": want}


@pytest.fixture(scope="module")
def stages(po):
    out = {}
    for name, (y, u, v) in contents().items():
        d, e, co, cg = block_values(y, u, v)
        out[name] = {"d": d, "e": e, "co": co, "cg": cg, "diag": diagonal_model(d, e), "ref": diagonal_stage(y, u, v),
                     "proj": projection_model(po, y, u, v, d, e, co, cg)}
    return out


def test_content_is_what_the_issue_names(stages):
    assert len(stages) == 8 and stages["S2"]["d"].shape == (128, 960, 16) and stages["sixths_extreme_luma"]["d"].shape == (8, 128, 16)


def test_box_ends_through_the_maps_are_the_reference_s(stages):
    for name, s in stages.items():
        got = s["diag"]["ends"]
        want = (s["co"].min(-1), s["co"].max(-1), s["cg"].min(-1), s["cg"].max(-1))
        for g, w_ in zip(got, want):
            assert g.dtype == F and np.array_equal(g.view(np.uint32), w_.view(np.uint32)), name


def test_the_maps_are_monotone_over_every_byte_triple():
    """every (y, u, v): the d and e of all 2^24 triples, sorted, map to non-decreasing Co and Cg -- so min and max commute with the maps for
    any two pixels whatever (the pixels of a block among them), bit for bit; no NaN, and -0 maps to off as +0 does"""
    byte = np.arange(256).astype(F) * K_INV255
    ds, es = [], []
    for ub in range(256):
        d, e = differences(byte[None, :, None], byte[ub], byte[None, None, :])   # (1, y, v)
        ds.append(np.unique(d)); es.append(np.unique(e))
    for vals, f in ((np.unique(np.concatenate(ds)), co_of), (np.unique(np.concatenate(es)), cg_of)):
        assert np.isfinite(vals).all() and len(vals) > 65536
        out = f(vals)
        assert (np.diff(out) >= 0).all()
        assert len(np.unique(out)) < len(vals)   # the maps do merge neighbours: the case of test (4)
    assert co_of(np.array([-0.0], F)).view(np.uint32)[0] == co_of(np.array([0.0], F)).view(np.uint32)[0] == np.array([K_OFFSET]).view(np.uint32)[0]


def test_difference_projection_is_within_a_quarter_of_eps_of_float64_for_both_pixels(stages):
    for name, s in stages.items():
        p = s["proj"]
        live = p["in_fast"] & ~p["flat"]
        if not live.any():
            print(f"{name}: no block reaches the projection")
            continue
        lim = lambda t: np.clip(3.0 * t.astype(D), -0.5, 3.5)
        eps = p["eps"].astype(D)[live][:, None]
        worst = max(float((np.abs(lim(p["t32"]) - lim(p["t64"][..., h::2]))[live] / eps).max()) for h in (0, 1))
        print(f"{name}: max |3 s32 - 3 s64| / eps over both pixels of the pairs = {worst:.4g}")
        assert worst <= 0.25, (name, worst)


def test_certified_pairs_decide_as_the_oracle(stages):
    for name, s in stages.items():
        p = s["proj"]
        live = (p["in_fast"] & ~p["flat"])[..., None]
        c = live & p["cert_pair"]
        differs = (p["proj_idx"] != p["want"][..., 0::2]) | (p["proj_idx"] != p["want"][..., 1::2])
        wrong = c & differs
        print(f"{name}: {int(c.sum())} of {int(live.sum()) * 8} pairs certified, {int(wrong.sum())} of them decide otherwise than the oracle; "
              f"{int((live & ~p['cert_pair'] & differs).sum())} uncertified pairs would")
        assert not wrong.any(), (name, int(wrong.sum()))


def test_video_like_frame_stays_under_the_projection_tests_cap(stages):
    p = stages["S2"]["proj"]
    bad = ~p["cert_block"] & p["in_fast"]
    share = float(waves(bad, False).any(-1).mean())
    print(f"S2: {100 * bad.mean():.4f} % of blocks, {100 * share:.3f} % of waves hold an uncertified pair")
    assert share <= WAVE_SHARE_CAP, share


def test_scaled_rough_is_within_a_quarter_of_eps_of_the_covariance(stages):
    for name, s in stages.items():
        m, ref = s["diag"], s["ref"]
        assert np.array_equal(m["hx"], ref["hx"]) and np.array_equal(m["hy"], ref["hy"])
        c = m["certified"] & (m["hx"] * m["hy"] != 0)
        eps = eps_diagonal(m["hx"], m["hy"])
        for rough in ("rough32", "rough64"):
            dist = np.abs(m[rough].astype(D) / 4.0 - ref["cov"].astype(D))
            worst = float((dist[c] / eps[c]).max()) if c.any() else 0.0
            print(f"{name}: max |rough / 4 - cov| / eps over {int(c.sum())} certified blocks = {worst:.4g} ({rough})")
            assert worst <= 0.25, (name, rough, worst)


def test_certified_blocks_swap_as_the_reference(stages):
    for name, s in stages.items():
        m, ref = s["diag"], s["ref"]
        wrong = m["certified"] & (m["swap"] != (ref["cov"] < 0)) & (m["hy"] != 0)   # with Cg flat the swap exchanges equal values
        share = float((~waves(m["certified"], True).all(-1)).mean())
        print(f"{name}: {int(m['certified'].sum())} of {m['certified'].size} blocks certified, {int(wrong.sum())} of them swap otherwise than the "
              f"reference; {100 * share:.3f} % of waves form the exact sum")
        assert not wrong.any(), (name, int(wrong.sum()))
    assert float((~waves(stages["S2"]["diag"]["certified"], True).all(-1)).mean()) < 0.02   # the cap tests/test_dxt_pair_cov_bound.py states


@functools.lru_cache(maxsize=None)
def co_flat_blocks(limit=64):
    """enumeration: every (u, v), every luma y against each of four fixed ones.  A block whose pairs alternate between (y, y) and (y', y')
    under the one (u, v) holds two d, two e; kept where the two Co are equal, the two d are not and the two Cg differ.
    -> (count of such (u, v, y, y'), count with rough < 0, the first `limit` of those as rows (u, v, y, y'))"""
    byte = np.arange(256).astype(F) * K_INV255
    found = negative = 0
    rows = []
    for ub in range(256):
        d, e = differences(byte[None, :], byte[ub], byte[:, None])   # (v, y)
        co, cg = co_of(d), cg_of(e)
        for yb in (0, 255, 16, 235):
            m = (co == co[:, yb:yb + 1]) & (d != d[:, yb:yb + 1]) & (cg != cg[:, yb:yb + 1])
            if not m.any():
                continue
            found += int(m.sum())
            vi, yi = np.nonzero(m)
            blocks_d = np.stack([d[vi, yi], d[vi, yb]], -1)[:, [0, 0, 1, 1] * 4]
            blocks_e = np.stack([e[vi, yi], e[vi, yb]], -1)[:, [0, 0, 1, 1] * 4]
            neg = diagonal_model(blocks_d, blocks_e)["swap_without_rule"]
            negative += int(neg.sum())
            rows += [(ub, int(a), int(b), yb) for a, b in zip(vi[neg][: max(0, limit - len(rows))], yi[neg])]
    return found, negative, np.array(rows)


def co_flat_planes(rows, bw, bh):
    """blocks of co_flat_blocks as pictures: block n takes row n (cyclically); pairs alternate between (y, y) and (y', y')"""
    r = rows[np.arange(bw * bh) % len(rows)].reshape(bh, bw, 4)
    ub, vb = np.broadcast_to(r[..., 0, None, None], (bh, bw, 4, 2)), np.broadcast_to(r[..., 1, None, None], (bh, bw, 4, 2))
    yb = np.stack([r[..., 2], r[..., 2], r[..., 3], r[..., 3]], -1)[:, :, None, :].repeat(4, axis=2)
    planes = lambda p: np.ascontiguousarray(p.transpose(0, 2, 1, 3).reshape(4 * bh, -1).astype(np.uint8))
    return planes(yb), planes(ub), planes(vb)


def test_co_flat_blocks_with_a_spread_in_d_keep_the_reference_s_ends():
    found, negative, rows = co_flat_blocks()
    print(f"(u, v, y, y') with equal Co, unequal d and unequal Cg: {found}, of them with rough < 0: {negative}")
    assert found > 0 and negative > 0 and len(rows) == 64   # they exist for UYVY bytes: the rule is needed, not only kept
    y, u, v = co_flat_planes(rows, 64, 1)
    d, e, co, cg = block_values(y, u, v)
    m, ref = diagonal_model(d, e), diagonal_stage(y, u, v)
    assert (m["hx"] == 0).all() and (m["hy"] > 0).all() and (d.max(-1) > d.min(-1)).all()
    assert m["certified"].all() and m["swap_without_rule"].all()
    assert not (ref["cov"] < 0).any() and not ref["cov"].any()   # the reference: every tx is 0, cov is +-0, no swap
    assert not m["swap"].any()                                    # the rule: the reference's ends
