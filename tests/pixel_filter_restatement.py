"""numpy restatement of the reference's colour / mirror capture filters (src/capture_filter/matrix.c, matrix2.c, gamma.cpp, grayscale.c,
mirror.c, flip.c), float64 in the reference's operation order -- what ug_hip_pixel_filter and the *_mi355x modules are held to, and what is
itself held to the reference's compiled modules through tests/golden/pixel_filter_ref.npz (tests/test_pixel_filter.py).

The conversion rule (include/ug_mi355x.h): double -> integer is truncation toward zero to int32, then the low 8 or 16 bits.  Where the exact
value lies outside the output type's range the reference's conversion is undefined: those elements are reported in `undefined`.
Every function takes and returns flat uint8 arrays of whole lines (vc_get_linesize) and works line by line at any width; for v210 that equals
the reference only at multiples of 48 (matrix2.c:216 hands the decoder the frame as one line)."""
import math

import numpy as np

Y601_TO_Y709 = [1, -0.11555, -0.207938, 0, 1.01864, 0.114618, 0, 0.075049, 1.025327]  # matrix2.c:69-73


def linesize(codec, w):
    """vc_get_linesize (video_codec.c:507-521) of the codecs the cases use"""
    if codec == "UYVY":
        return (w + 1) // 2 * 4
    if codec == "v210":
        return (w + 47) // 48 * 128
    return {"RGB": 3, "RG48": 6, "Y416": 8, "RGBA": 4, "R10k": 4}[codec] * (w if codec != "R10k" else (w + 63) // 64 * 64)


def _cvt(v, bits):
    """the conversion rule -> (low `bits` bits, undefined where trunc(v) is outside 0 .. 2^bits - 1)"""
    t = np.trunc(v)
    assert (np.abs(t) < 2.0 ** 31).all()
    i = t.astype(np.int64)
    return (i & ((1 << bits) - 1)).astype(np.uint16 if bits == 16 else np.uint8), (i < 0) | (i >= (1 << bits))


def _clamp255(v, dtype):
    """int val = v; CLAMP(val, 0, 255) (matrix.c:158-161)"""
    t = np.trunc(v)
    assert (np.abs(t) < 2.0 ** 31).all()
    return np.clip(t.astype(np.int64), 0, 255).astype(dtype)


def matrix(codec, data, m, clamp):
    """matrix.c:146-308 -> (out bytes, undefined mask over the out ELEMENTS flattened); UYVY comes out as RGB"""
    m = [float(x) for x in m]
    if codec == "UYVY":
        a = data.reshape(-1, 4).astype(np.float64)
        u, v = a[:, 0] - 128, a[:, 2] - 128
        cols = []
        for y in (a[:, 1] - 16, a[:, 3] - 16):
            for c in range(3):
                cols.append(m[3 * c] * y + m[3 * c + 1] * u + m[3 * c + 2] * v)
        val = np.stack(cols, axis=1)
        dtype = np.uint8
    else:
        dtype = np.uint8 if codec == "RGB" else np.uint16
        a = data.view(dtype).reshape(-1, 3).astype(np.float64)
        val = np.stack([m[3 * c] * a[:, 0] + m[3 * c + 1] * a[:, 1] + m[3 * c + 2] * a[:, 2] for c in range(3)], axis=1)
    if clamp:
        out = _clamp255(val, dtype)
        return out.reshape(-1).view(np.uint8), np.zeros(out.size, bool)
    out, undef = _cvt(val, 8 if dtype == np.uint8 else 16)
    return out.reshape(-1).view(np.uint8), undef.reshape(-1)


def _matrix2_y416(px, m):
    """matrix2.c:219-237 on an (n, 4) uint16 array of U Y V A -> ((n, 4) uint16, (n, 4) undefined)"""
    u, y, v = px[:, 0].astype(np.float64) - (1 << 15), px[:, 1].astype(np.float64) - (1 << 12), px[:, 2].astype(np.float64) - (1 << 15)
    un = (1 << 15) + m[3] * y + m[4] * u + m[5] * v
    yn = (1 << 12) + m[0] * y + m[1] * u + m[2] * v
    vn = (1 << 15) + m[6] * y + m[7] * u + m[8] * v
    out, undef = _cvt(np.stack([un, yn, vn, np.full_like(un, 65535.0)], axis=1), 16)
    return out, undef


def matrix2(codec, data, m):
    """matrix2.c:167-243 -> (out bytes, undefined mask over the out elements: bytes (UYVY), uint16 (Y416), 32-bit words (v210))"""
    m = [float(x) for x in m]
    if codec == "UYVY":
        a = data.reshape(-1, 4).astype(np.float64)
        u, y1, v, y2 = a[:, 0] - 128, a[:, 1] - 16, a[:, 2] - 128, a[:, 3] - 16
        y = (y1 + y2) / 2
        val = np.stack([128 + m[3] * y + m[4] * u + m[5] * v, 16 + m[0] * y1 + m[1] * u + m[2] * v,
                        128 + m[6] * y + m[7] * u + m[8] * v, 16 + m[0] * y2 + m[1] * u + m[2] * v], axis=1)
        out, undef = _cvt(val, 8)
        return out.reshape(-1), undef.reshape(-1)
    if codec == "Y416":
        out, undef = _matrix2_y416(data.view(np.uint16).reshape(-1, 4), m)
        return out.reshape(-1).view(np.uint8), undef.reshape(-1)
    assert codec == "v210"
    w = data.view(np.uint32).reshape(-1, 4)
    w0, w1, w2, w3 = (w[:, i] for i in range(4))
    f = lambda x, s: (x >> s) & 0x3ff  # noqa: E731
    Y = [f(w0, 10), f(w1, 0), f(w1, 20), f(w2, 10), f(w3, 0), f(w3, 20)]
    U = [f(w0, 0), f(w1, 10), f(w2, 20)]
    V = [f(w0, 20), f(w2, 0), f(w3, 10)]
    # vc_copylineV210toY416 (pixfmt_conv.c:2834-2882): sample << 6, the pair's chroma for both pixels
    px = np.stack([np.stack([U[i // 2] << 6, Y[i] << 6, V[i // 2] << 6, np.full_like(w0, 0xFFFF)], axis=1) for i in range(6)], axis=1)  # (n, 6, 4)
    out, undef = _matrix2_y416(px.reshape(-1, 4).astype(np.uint16), m)
    s = out.reshape(-1, 24).astype(np.uint32)
    undef = undef.reshape(-1, 24)
    # vc_copylineY416toV210 (:3004-3031)
    u = [((s[:, 8 * i] + s[:, 8 * i + 4]) // 2) >> 6 for i in range(3)]
    v = [((s[:, 8 * i + 2] + s[:, 8 * i + 6]) // 2) >> 6 for i in range(3)]
    y = [s[:, 8 * (i // 2) + 1 + 4 * (i % 2)] >> 6 for i in range(6)]
    d = np.stack([u[0] | y[0] << 10 | v[0] << 20, y[1] | u[1] << 10 | y[2] << 20, v[1] | y[3] << 10 | u[2] << 20, y[4] | v[2] << 10 | y[5] << 20], axis=1)
    # the samples of pixel i of a group feed: words 0 (pixels 0, 1), 1 (1, 2, 3), 2 (2, 3, 4, 5), 3 (4, 5): a word is undefined if one of its sources is
    pu = undef.reshape(-1, 6, 4)[:, :, :3].any(axis=2)
    wu = np.stack([pu[:, 0] | pu[:, 1], pu[:, 1] | pu[:, 2] | pu[:, 3], pu[:, 2] | pu[:, 3] | pu[:, 4] | pu[:, 5], pu[:, 4] | pu[:, 5]], axis=1)
    return d.astype(np.uint32).reshape(-1).view(np.uint8), wu.reshape(-1)


def gamma_lut(gamma, in_bits, out_bits):
    """gamma.cpp:74-93 with the C library's pow (math.pow calls it; numpy's power is its own)"""
    mi, mo = (1 << in_bits) - 1, (1 << out_bits) - 1
    return np.array([int(math.pow(i / mi, gamma) * mo) for i in range(mi + 1)], np.uint16 if out_bits == 16 else np.uint8)


def lut(data, in_bits, table):
    """gamma.cpp:119-126 over EVERY element"""
    return table[data.view(np.uint16 if in_bits == 16 else np.uint8)].reshape(-1).view(np.uint8)


def grayscale(data):
    out = data.copy()
    out[0::2] = 127
    return out


def mirror(data, w, h):
    L = linesize("UYVY", w)
    a = data.reshape(h, L // 4, 4)[:, ::-1, :]
    return np.ascontiguousarray(a[:, :, [0, 3, 2, 1]]).reshape(-1)


def flip(data, h):
    return np.ascontiguousarray(data.reshape(h, -1)[::-1]).reshape(-1)


def parse_matrix(options, allow_preset):
    """matrix.c:88-116 / matrix2.c:105-136 -> (m or None, check_bounds)"""
    m, check = [], True
    for item in [t for t in options.split(":") if t]:
        if allow_preset and not m and item == "y601_to_y709":
            return list(Y601_TO_Y709), True
        if len(m) == 9:
            if not allow_preset and item == "no-bound-check":
                check = False
            break
        m.append(float(item))
    return (m if len(m) == 9 else None), check


def run_filter(name, options, codec, w, h, data):
    """A module as a whole -> dict(status, codec, out, undefined, elem):
    status `new` (a frame of the module's own: codec, out bytes, undefined mask over elements of `elem` bytes), `same` (the input frame handed
    back), `null` (refused), `unwritten` (matrix2: the output frame as allocated).  `name` without the _mi355x suffix."""
    data = np.ascontiguousarray(data, np.uint8).reshape(-1)
    res = lambda out, oc=codec, undef=None, elem=1: dict(status="new", codec=oc, out=out, undefined=undef, elem=elem)  # noqa: E731
    if name == "matrix":
        m, check = parse_matrix(options, False)
        if codec not in ("UYVY", "RGB", "RG48"):
            return dict(status="null")
        out, undef = matrix(codec, data, m, check)
        return res(out, "RGB" if codec == "UYVY" else codec, undef, 2 if codec == "RG48" else 1)
    if name == "matrix2":
        m, _ = parse_matrix(options, True)
        if codec not in ("UYVY", "v210", "Y416"):
            return dict(status="unwritten", codec=codec)
        out, undef = matrix2(codec, data, m)
        return res(out, codec, undef, {"UYVY": 1, "Y416": 2, "v210": 4}[codec])
    if name == "gamma":
        if codec not in ("RGB", "RG48"):
            return dict(status="null")
        g, _, depth = options.partition(":")
        ib = 16 if codec == "RG48" else 8
        ob = int(depth) if depth else ib
        return res(lut(data, ib, gamma_lut(float(g), ib, ob)), "RG48" if ob == 16 else "RGB")
    if name in ("grayscale", "mirror"):
        if codec != "UYVY":
            return dict(status="same", codec=codec, out=data)
        return res(grayscale(data) if name == "grayscale" else mirror(data, w, h))
    assert name == "flip"
    return res(flip(data, h))
