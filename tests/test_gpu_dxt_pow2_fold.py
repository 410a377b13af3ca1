"""GPU parity on content built for the folded products of encode_dxt5ycocg (dxt_encode.hip): products by powers of two inside the
fma of the neighbouring sum, the luma kept at 4 Y through the alpha stage.  UYVY, v210, YUV444, RGB and RGBA -> DXT5-YCoCg, both tie rules,
512 x 32 and 510 x 30 (two waves per block row; the EDGE lane), byte for byte against the oracle, on frames built on the CPU and checked with
the model of tests/test_dxt_pow2_fold_bound.py:
  * every block of a frame takes scale 1, or 2, or 4 (chroma amplitude >= 64 / 255, in [32, 64) / 255, < 32 / 255 around the offset), and one
    frame mixes the three: the chroma end points, their dequantisation and insets under every factor;
  * luma boxes whose range after the inset lies just under and just over 2^-10, the wave test of the fast alpha stage, boxes that collapse
    (both ends clamped to one bound, from luma bytes 0-4 and 251-255) and boxes whose ends clamp at 0, at 1 and at both, spread so that some
    waves stay in the fast stage and others leave it: the fast stage, the binary search and -- where libug_mi355x_alphalinear.so is built --
    the linear count all compare in the 4 x domain.  (The RGB front ends cannot bring a box under 2^-10: their frame holds the clamps.)"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_dxt_pow2_fold_bound as M  # noqa: E402
from test_gpu_dxt_pair_zone import pack_uyvy, pack_v210  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(512, 32), (510, 30)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def unblock(b, w, h, per_row):
    """(bh, bw, 4, per_row[, c]) -> picture cut to h rows, w * per_row / 4 columns"""
    bh, bw = b.shape[:2]
    p = np.swapaxes(b, 1, 2).reshape((4 * bh, per_row * bw) + b.shape[4:])
    return np.ascontiguousarray(p[:h, : w * per_row // 4].astype(np.uint8))


@functools.lru_cache(maxsize=None)
def yuv_frames(w, h):
    """name -> (y, u, v) byte planes, 4:2:2"""
    rng = np.random.default_rng(5200 + w)
    bw, bh = (w + 3) // 4, (h + 3) // 4
    n = np.arange(bh * bw).reshape(bh, bw)

    def chroma(amp, lead):
        """random samples within amp bytes of 128; sample (0, 0) of every block -- which a cut block keeps -- at +- lead in U and -+ lead in V"""
        uv = 128 + rng.integers(-amp, amp + 1, (bh, bw, 4, 2, 2))
        if lead:
            sign = rng.integers(0, 2, (bh, bw)) * 2 - 1
            uv[:, :, 0, 0, 0] = 128 + sign * lead
            uv[:, :, 0, 0, 1] = 128 - sign * lead
        return np.clip(uv, 0, 255)
    by_scale = {1: chroma(127, 102), 2: chroma(20, 23), 4: chroma(12, 0)}
    out, want = {}, {}
    for s, uv in by_scale.items():
        out[f"scale{s}"] = (rng.integers(0, 256, (bh, bw, 4, 4)), uv[..., 0], uv[..., 1])
        want[f"scale{s}"] = np.full((bh, bw), s)
    pick = (n + n // bw) % 3
    uv = np.choose(pick[:, :, None, None, None], [by_scale[1], by_scale[2], by_scale[4]])
    out["scales_mixed"] = (rng.integers(0, 256, (bh, bw, 4, 4)), uv[..., 0], uv[..., 1])
    want["scales_mixed"] = np.choose(pick, [1, 2, 4])
    planes = {k: (unblock(yb, w, h, 4), unblock(ub, w, h, 2), unblock(vb, w, h, 2)) for k, (yb, ub, vb) in out.items()}
    for k, p in planes.items():
        _, co, cg = M.ycocg_blocks_yuv(*p)
        assert np.array_equal(M.scale_of(co, cg), want[k]), k
    planes["luma_seams_and_clamps"] = M.seam_frame(w, h)
    s = M.alpha_stage(M.ycocg_blocks_yuv(*planes["luma_seams_and_clamps"])[0])
    r = s["range"]
    assert ((r > 0) & (r <= M.ALL_WIDE)).sum() >= 8 and ((r > M.ALL_WIDE) & (r < 2 * M.ALL_WIDE)).sum() >= 8 and (r == 0).sum() >= 8
    assert ((s["mn"] == 0) & (s["mx"] == 1)).any() and ((s["mn"] == 0) & (s["mx"] < 1)).any() and ((s["mn"] > 0) & (s["mx"] == 1)).any()
    assert (r[4:6] > M.ALL_WIDE).all() and (r[:4] <= M.ALL_WIDE).any(axis=1).all()   # block rows that stay in the fast stage, rows that leave it
    return planes


@functools.lru_cache(maxsize=None)
def rgb_frames(w, h):
    """name -> (h, w, 3) bytes, from luma and chroma offsets in bytes: r = L + co - cg, g = L + cg, b = L - co - cg, so that Co - off = co / 255
    and Cg - off = cg / 255 up to rounding"""
    rng = np.random.default_rng(5300 + w)
    bw, bh = (w + 3) // 4, (h + 3) // 4
    n = np.arange(bh * bw).reshape(bh, bw)

    def block_rgb(amp, lead):
        c = rng.integers(-amp, amp + 1, (bh, bw, 4, 4, 2))
        if lead:
            c[:, :, 0, 0, 0] = (rng.integers(0, 2, (bh, bw)) * 2 - 1) * lead
            c[:, :, 0, 0, 1] = 0
        room = np.abs(c).sum(-1)
        lum = rng.integers(0, 256, (bh, bw, 4, 4))
        lum = np.clip(lum, room, 255 - room)
        return np.stack([lum + c[..., 0] - c[..., 1], lum + c[..., 1], lum - c[..., 0] - c[..., 1]], axis=-1)
    by_scale = {1: block_rgb(40, 80), 2: block_rgb(20, 45), 4: block_rgb(12, 0)}
    pick = (n + n // bw) % 3
    out = {f"scale{s}": b for s, b in by_scale.items()}
    out["scales_mixed"] = np.choose(pick[:, :, None, None, None], [by_scale[1], by_scale[2], by_scale[4]])
    want = {"scale1": np.full((bh, bw), 1), "scale2": np.full((bh, bw), 2), "scale4": np.full((bh, bw), 4), "scales_mixed": np.choose(pick, [1, 2, 4])}
    # luma ends that clamp: blocks next to black, next to white, and of both and ordinary ones (wide boxes, which the inset shrinks)
    ends = rng.integers(0, 256, (bh, bw, 4, 4, 3))
    kind = (n + 3 * (n // bw)) % 4
    dark, light = rng.integers(0, 4, ends.shape), rng.integers(252, 256, ends.shape)
    both = np.where(rng.integers(0, 2, (bh, bw, 4, 4, 1)) == 1, dark, light)
    dark[:, :, 0, 0], light[:, :, 0, 0], both[:, :, 0, 0], both[:, :, 0, 1] = 0, 255, 0, 255   # pixels that a cut block keeps
    for k, src in ((0, dark), (1, light), (2, both)):
        ends[kind == k] = src[kind == k]
    out["clamps"] = ends
    frames = {k: unblock(b, w, h, 4) for k, b in out.items()}

    def model(rgb):
        return M.ycocg_blocks_rgb(np.pad(rgb, ((0, -h % 4), (0, -w % 4), (0, 0)), mode="edge"))
    for k, f in frames.items():
        assert f.min() >= 0 and f.max() <= 255
        if k in want:
            _, co, cg = model(f)
            assert np.array_equal(M.scale_of(co, cg), want[k]), k
    s = M.alpha_stage(model(frames["clamps"])[0])
    assert (s["mn"] == 0).sum() >= 8 and (s["mx"] == 1).sum() >= 8   # (never both: a box from 0 to 1 is inset by 1 / 32 - 1 / 510 > 0)
    return frames


def sources(po, w, h):
    """(frame, format) -> (library format, oracle format, packed bytes)"""
    from ultragrid_amd import lib as L
    rng = np.random.default_rng(77 + w)
    out = {}
    for name, (y, u, v) in yuv_frames(w, h).items():
        out[name, "UYVY"] = (L.PF_UYVY, po.IN_UYVY, pack_uyvy(y, u, v))
        out[name, "v210"] = (L.PF_V210, po.IN_V210, pack_v210(y, u, v, rng.integers(0, 4, (h, 2 * w)).astype(np.uint32)))
        out[name, "YUV444"] = (L.PF_YUV444, po.IN_YUV444, np.stack([y, np.repeat(u, 2, axis=1), np.repeat(v, 2, axis=1)], axis=-1).ravel())
    for name, rgb in rgb_frames(w, h).items():
        out[name, "RGB"] = (L.PF_RGB, po.IN_RGB, rgb.ravel())
        out[name, "RGBA"] = (L.PF_RGBA, po.IN_RGBA, np.concatenate([rgb, rng.integers(0, 256, (h, w, 1)).astype(np.uint8)], axis=-1).ravel())
    return out


@functools.lru_cache(maxsize=None)
def variant(name):
    """a variant build of the library, bound as ultragrid_amd.lib binds the product; None where it has not been built"""
    from ultragrid_amd import lib as L
    path = os.path.join(ROOT, "ultragrid_amd", f"libug_mi355x_{name}.so")
    if not os.path.exists(path):
        return None
    so = C.CDLL(path)
    for fn in ("ug_hip_abi_version", "ug_hip_dxt_encode_batch_ex", "ug_hip_dxt_encode_stats_ex"):
        getattr(so, fn).restype, getattr(so, fn).argtypes = L.SYMBOLS[fn]
    assert so.ug_hip_abi_version() == L.ABI_VERSION
    return so


def encode(so, pf, src, w, h, ties, po):
    """-> (blocks, the three counters of this one encode)"""
    import torch
    from ultragrid_amd import lib as L
    dev = torch.from_numpy(np.ascontiguousarray(src, dtype=np.uint8)).cuda()
    dst = torch.zeros(po.dxt_size(po.OUT_DXT5YCOCG, w, h), dtype=torch.uint8, device="cuda")
    st = (C.c_ulonglong * 3)()
    assert so.ug_hip_dxt_encode_stats_ex(None, 0, 1) == 0
    rc = so.ug_hip_dxt_encode_batch_ex(pf, L.DXT5_YCOCG, dev.data_ptr(), dst.data_ptr(), w, h, 0, 1, 0, 0, ties, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert so.ug_hip_dxt_encode_stats_ex(st, 3, 1) == 0
    return dst.cpu().numpy(), tuple(int(x) for x in st)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_folded_encoder_on_its_seams(hip, po, size):
    from ultragrid_amd import lib as L
    w, h = size
    product, linear = L.load(), variant("alphalinear")
    bad, left_fast = [], 0
    for (name, fmt), (pf, pin, src) in sources(po, w, h).items():
        for ties, tname in ((L.TIES_EVEN, "even"), (L.TIES_AWAY, "away")):
            want = po.dxt_encode(pin, po.OUT_DXT5YCOCG, src, w, h, ties=tname)
            got, st = encode(product, pf, src, w, h, ties, po)
            if not np.array_equal(got, want):
                bad.append((name, fmt, tname, "product", int(np.count_nonzero(got != want))))
            if name == "luma_seams_and_clamps" and ties == L.TIES_EVEN:
                print(f"{name} {fmt} {w}x{h}: colour full form {st[0]}, alpha full form {st[1]}, exact covariance {st[2]} waves")
                left_fast += st[1] > 0
            if linear is not None:
                got, _ = encode(linear, pf, src, w, h, ties, po)
                if not np.array_equal(got, want):
                    bad.append((name, fmt, tname, "alphalinear", int(np.count_nonzero(got != want))))
    print(f"{w}x{h}: alphalinear library {'compared' if linear is not None else 'not built'}")
    assert not bad, bad
    assert left_fast == 3, left_fast   # UYVY, v210 and YUV444: waves of the seam frame did leave the fast alpha stage
