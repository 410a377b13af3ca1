"""numpy fp32 restatement of `-c uyvy` (src/video_compress/uyvy.cpp): dxt_compress/rgba_to_yuv422.glsl on RGB / RGBA pictures, as the
product's UG_PF_UYVY_GL output computes it.  Output pair i of line y = the shader on pixels 2i and 2i + 1 of line y (for odd widths the
second pixel of the last pair is the last pixel: CLAMP_TO_EDGE), every operation in float32 in the shader's order, no fused multiply-add,
float -> unorm8 with clamping and ties to even (llvmpipe); lines of vc_get_linesize(w, UYVY) = (w + 1) // 2 * 4 bytes.  Alpha is ignored.

Pinned to the shader executed by llvmpipe through tests/golden/uyvy_glsl_ref.npz (tests/test_uyvy_glsl.py)."""
import numpy as np

F = np.float32


def _unorm8(x):
    x = np.clip(x, F(0), F(1))
    return np.rint(x * F(255)).astype(np.uint8)  # numpy rint: round half to even


def _yuv(rgb):
    """rgb: (..., 3) uint8 -> Y, U, V float32, the shader's statements (texel fetch v * (1 / 255.0), as llvmpipe converts unorm8)"""
    c = rgb.astype(F) * (F(1) / F(255))
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    y = F(1.0 / 16.0) + ((r * F(0.2126) + g * F(0.7152)) + b * F(0.0722)) * F(0.8588)
    u = F(0.5) + ((-r * F(0.1145) - g * F(0.3854)) + b * F(0.5)) * F(0.8784)
    v = F(0.5) + ((r * F(0.5) - g * F(0.4541)) - b * F(0.0458)) * F(0.8784)
    return y, u, v


def rgb_to_uyvy_gl(src: np.ndarray, w: int, h: int, bpp: int, pitch: int = 0) -> np.ndarray:
    """src: bytes of h lines of `pitch` (0: packed, w * bpp) bytes, bpp 3 (RGB) or 4 (RGBA) -> UYVY bytes, h lines of (w + 1) // 2 * 4"""
    pitch = pitch or w * bpp
    a = np.frombuffer(np.ascontiguousarray(src).tobytes(), np.uint8)[: pitch * (h - 1) + w * bpp]
    a = np.concatenate([a, np.zeros(pitch * h - a.size, np.uint8)]).reshape(h, pitch)[:, : w * bpp].reshape(h, w, bpp)[..., :3]
    pairs = (w + 1) // 2
    i1 = 2 * np.arange(pairs)
    i2 = np.minimum(i1 + 1, w - 1)
    y1, u1, v1 = _yuv(a[:, i1])
    y2, u2, v2 = _yuv(a[:, i2])
    u = u1 * F(0.5) + u2 * F(0.5)  # mix(a, b, 0.5) = a * (1 - 0.5) + b * 0.5
    v = v1 * F(0.5) + v2 * F(0.5)
    out = np.stack([_unorm8(u), _unorm8(y1), _unorm8(v), _unorm8(y2)], axis=-1)
    return out.reshape(h, pairs * 4).reshape(-1)


def gl_skewed_rgba(rgb_packed: np.ndarray, w: int, h: int) -> np.ndarray:
    """the RGBA texture the reference builds from packed RGB lines when 3 w % 4 != 0: GL reads GL_RGB lines at its default 4-byte
    GL_UNPACK_ALIGNMENT (uyvy.cpp:241 never sets it), i.e. line y from byte y * ((3 w + 3) & ~3) -- past the buffer, zeros here"""
    stride = (3 * w + 3) & ~3
    buf = np.zeros(stride * h, np.uint8)
    flat = np.ascontiguousarray(rgb_packed).reshape(-1)[: 3 * w * h]
    buf[: flat.size] = flat
    rgb = buf.reshape(h, stride)[:, : 3 * w].reshape(h, w, 3)
    return np.concatenate([rgb, np.full((h, w, 1), 255, np.uint8)], axis=-1).reshape(-1)
