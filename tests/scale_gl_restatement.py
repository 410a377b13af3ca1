"""numpy restatement of UltraGrid's `scale` video postprocessor (src/vo_postprocess/scale.c) as the product's ug_hip_scale computes it,
pinned to the module executed on Mesa llvmpipe (tests/golden/scale_gl_ref.npz, tests/test_scale_gl.py).

Texel view (scale.c:190-216, :255-280): a picture is a texture of 4-byte texels -- one RGBA pixel, or one U Y0 V Y1 pair of UYVY -- and an
INTERLACED_MERGED picture puts two lines side by side in one texel row (width x 2, height / 2), so the vertical filter stays in one field.

GL_LINEAR with GL_CLAMP_TO_EDGE over one full-viewport quad, texture coordinates 0..1, no vertical flip (:286-305), in llvmpipe's integer
fixed point, per axis (n_in texels -> n_out texels):
    p  = round_half_up((2 x + 1) * n_in * 128 / n_out) - 128      the sample position in 1/256 texel, texel centres at multiples of 256
    i0 = p >> 8 (floor), i1 = i0 + 1, both clamped to 0 .. n_in - 1; w = p & 255
    lerp(a, b, w) = (a * (256 - w) + b * w + 128) >> 8            per byte
    texel = lerp(lerp(t[j0][i0], t[j0][i1], wx), lerp(t[j1][i0], t[j1][i1], wx), wy)
The GL modulate by the default white colour is exact.  llvmpipe computes p from fp32 texture coordinates; the exact rational form above
is the rule the kernel and this file use: next to a rounding tie the two can differ by one position step, at most 1 LSB per byte (the fixture's
RGBA 300x20 -> 107x7 case: 7 of 2 996 bytes; tests/test_scale_gl.py pins them).

Slips of the reference not reproduced (tests/test_scale_gl.py records each):
  - odd UYVY widths: the reference's texture is w // 2 texels wide over lines of vc_get_linesize = (w + 1) // 2 pairs (rows shear on upload
    and on read-back); here a line is (w + 1) // 2 texels, in and out;
  - INTERLACED_MERGED with an odd OUTPUT height: the reference renders out_h // 2 texel rows and leaves the last line unwritten; refused here.
  - tile_count > 1: the reference writes out->tiles[i] of a one-tile output frame.
  (An odd INPUT height with INTERLACED_MERGED drops the last line, as the reference does: a texel row needs two lines.)
"""
import numpy as np

UYVY, RGBA = "UYVY", "RGBA"


def texels_per_line(codec: str, width: int) -> int:
    return (width + 1) // 2 if codec == UYVY else width


def linesize(codec: str, width: int) -> int:
    return 4 * texels_per_line(codec, width)


def axis(n_in: int, n_out: int):
    """(i0, i1, w) per output texel of one axis"""
    x = np.arange(n_out, dtype=np.int64)
    num = (2 * x + 1) * n_in * 128
    p = (2 * num + n_out) // (2 * n_out) - 128
    i0 = p >> 8
    w = p & 255
    return np.clip(i0, 0, n_in - 1), np.clip(i0 + 1, 0, n_in - 1), w


def lerp(a, b, w):
    return (a * (256 - w) + b * w + 128) >> 8


def resample(tex: np.ndarray, ow: int, oh: int) -> np.ndarray:
    """tex: (th, tw, 4) uint8 texels -> (oh, ow, 4) uint8"""
    th, tw = tex.shape[:2]
    i0, i1, wx = axis(tw, ow)
    j0, j1, wy = axis(th, oh)
    t = tex.astype(np.int64)
    wx = wx[None, :, None]
    top = lerp(t[j0][:, i0], t[j0][:, i1], wx)
    bot = lerp(t[j1][:, i0], t[j1][:, i1], wx)
    return lerp(top, bot, wy[:, None, None]).astype(np.uint8)


def to_texels(src, codec: str, w: int, h: int, merged: bool, pitch: int = 0) -> np.ndarray:
    """picture bytes (h lines `pitch` apart, 0 = packed) -> the texture the stand-in samples"""
    tpl = texels_per_line(codec, w)
    pitch = pitch or 4 * tpl
    a = np.frombuffer(np.ascontiguousarray(src).tobytes(), np.uint8)
    a = np.concatenate([a, np.zeros(max(0, pitch * h - a.size), np.uint8)])[: pitch * h]
    lines = a.reshape(h, pitch)[:, : 4 * tpl].reshape(h, tpl, 4)
    if merged:
        lines = lines[: h // 2 * 2].reshape(h // 2, 2 * tpl, 4)
    return lines


def scale(src, codec: str, w: int, h: int, ow: int, oh: int, merged: bool = False, src_pitch: int = 0) -> np.ndarray:
    """the stand-in's output: oh lines of linesize(codec, ow) bytes, flat"""
    if merged and oh % 2:
        raise ValueError("INTERLACED_MERGED with an odd output height is refused")
    tex = to_texels(src, codec, w, h, merged, src_pitch)
    otw, oth = texels_per_line(codec, ow) * (2 if merged else 1), oh // 2 if merged else oh
    out = resample(tex, otw, oth)
    return out.reshape(oh, linesize(codec, ow)).reshape(-1)


def reference_gl(src, codec: str, w: int, h: int, ow: int, oh: int, merged: bool, req_pitch: int):
    """what the reference module writes into an output buffer of req_pitch * oh bytes pre-filled with 0xA5, slips included (odd UYVY widths:
    textures of w // 2 texels read from / written to packed memory; odd merged heights: h // 2 and oh // 2 texel rows) -- for the slip tests.
    Returns (bytes, determinate): `determinate` is False where the module copies bytes of its temporary buffer that GL never wrote (scale.c:244
    mallocs it; the sheared read-back of an odd UYVY width leaves its tail as it was)."""
    tw = w // 2 if codec == UYVY else w
    otw = ow // 2 if codec == UYVY else ow
    th, oth = (h // 2, oh // 2) if merged else (h, oh)
    tw, otw = (2 * tw, 2 * otw) if merged else (tw, otw)
    a = np.frombuffer(np.ascontiguousarray(src).tobytes(), np.uint8)
    tex = a[: th * tw * 4].reshape(th, tw, 4)  # glTexSubImage2D reads rows of tw texels from the packed frame
    rows = resample(tex, otw, oth).reshape(-1)  # glReadPixels writes rows of otw texels
    out = np.full(req_pitch * oh + 4096, 0xA5, np.uint8)
    known = np.ones(out.size, bool)
    ls = linesize(codec, ow)
    if req_pitch == ls:
        out[: rows.size] = rows
    else:  # scale.c:294-303: read back into a temporary buffer of ls * oh bytes, then ls bytes per line for out_h lines
        tmp = np.zeros(ls * oh, np.uint8)
        tmp_known = np.zeros(ls * oh, bool)
        tmp[: rows.size] = rows
        tmp_known[: rows.size] = True
        for y in range(oh):
            out[y * req_pitch: y * req_pitch + ls] = tmp[y * ls: (y + 1) * ls]
            known[y * req_pitch: y * req_pitch + ls] = tmp_known[y * ls: (y + 1) * ls]
    return out[: req_pitch * oh], known[: req_pitch * oh]
