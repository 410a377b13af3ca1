"""numpy restatement of the JPEG decoder's output stage for the sampling layouts layout_pack_kernel takes (csrc/jpeg_decode.hip): component
planes of any integral ratio -> packed UG_PF_RGB / UG_PF_RGBA / UG_PF_UYVY.  The rule is REPLICATION: a component sample covers its rx x ry
pixels.  R,G,B streams: the pixel's R, G, B bytes (RGBA: at the shifts, the byte they leave 0xFF); UYVY through vc_copylineRGBtoUYVY's
integer arithmetic on the pixel pair.  Y'CbCr streams: UYVY with the pair's chroma (a + b) // 2.  Odd widths: the last pair's second pixel is
its first.  Y'CbCr -> RGB / RGBA is the UYVY form through the pixel-format converter (oracle.pyoracle.convert_frame)."""
import numpy as np


def replicate(plane, rx, ry, w, h):
    """a component plane (at least ceil(h / ry) x ceil(w / rx)) on the full pixel grid"""
    return np.repeat(np.repeat(np.asarray(plane), ry, axis=0), rx, axis=1)[:h, :w]


def full_planes(planes, ratios, w, h):
    return [replicate(p, rx, ry, w, h).astype(np.int64) for p, (rx, ry) in zip(planes, ratios)]


def _pairs(a, w):
    """first and second pixel of every pair of a line (the last pair of an odd width: its first pixel twice)"""
    i = np.arange((w + 1) // 2)
    return a[:, 2 * i], a[:, np.minimum(2 * i + 1, w - 1)]


def _uyvy(u, y1, v, y2):
    h = u.shape[0]
    return np.stack([u, y1, v, y2], -1).astype(np.uint8).reshape(h, -1)


def rgb_to_rgb(full):
    return np.stack(full, -1).astype(np.uint8).reshape(full[0].shape[0], -1)


def rgb_to_rgba(full, shifts=(0, 8, 16)):
    rs, gs, bs = shifts
    rest = 0xFFFFFFFF ^ (0xFF << rs) ^ (0xFF << gs) ^ (0xFF << bs)
    word = (rest | (full[0] << rs) | (full[1] << gs) | (full[2] << bs)).astype(np.uint32)
    return word.view(np.uint8).reshape(word.shape[0], -1)


def rgb_to_uyvy(full, w):
    """vc_copylineToUYVY (pixfmt_conv.c:1008-1053) on 8-bit R, G, B: Q14 BT.709 limited range"""
    r, g, b = full
    y = ((r * 2992 + g * 10063 + b * 1016) >> 14) + 16
    u = r * -1649 + g * -5547 + b * 7196
    v = r * 7195 + g * -6536 + b * -659
    y1, y2 = _pairs(y, w)
    ua, ub = _pairs(u, w)
    va, vb = _pairs(v, w)
    su, sv = ua + ub, va + vb
    # C '/' truncates toward zero, '>>' floors
    su = np.where(su < 0, -((-su) // 2), su // 2)
    sv = np.where(sv < 0, -((-sv) // 2), sv // 2)
    return _uyvy(((su >> 14) + 128) & 0xFF, y1 & 0xFF, ((sv >> 14) + 128) & 0xFF, y2 & 0xFF)


def ycc_to_uyvy(full, w):
    y1, y2 = _pairs(full[0], w)
    ua, ub = _pairs(full[1], w)
    va, vb = _pairs(full[2], w)
    return _uyvy((ua + ub) // 2, y1, (va + vb) // 2, y2)


def expected(po, planes, ratios, w, h, rgb, out, shifts=(0, 8, 16)):
    """the packed picture (h, line bytes) the decoder writes for `out` in "RGB", "RGBA", "UYVY" """
    full = full_planes(planes, ratios, w, h)
    if rgb:
        return {"RGB": lambda: rgb_to_rgb(full), "RGBA": lambda: rgb_to_rgba(full, shifts), "UYVY": lambda: rgb_to_uyvy(full, w)}[out]()
    uyvy = ycc_to_uyvy(full, w)
    if out == "UYVY":
        return uyvy
    return po.convert_frame("UYVY", out, uyvy.ravel(), w, h, shifts).reshape(h, -1)
