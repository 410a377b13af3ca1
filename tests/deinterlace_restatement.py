"""numpy restatement of the reference's de-interlacers: vc_deinterlace_ex (src/video_codec.c:722-854) and the three temporal filters of
src/vo_postprocess/temporal-deint.c (double_framerate, deinterlace_bob, deinterlace_linear), element by element -- what ug_hip_deinterlace and
the *_mi355x modules are held to.  Frames are 2-D uint8 arrays [lines, pitch]; a destination is passed in with the bytes it held before
(`bg`) because the reference leaves parts of some lines unwritten (written_bytes)."""
import numpy as np

BLEND, WEAVE, BOB, LINEAR = 0, 1, 2, 3
MODES = {"BLEND": BLEND, "WEAVE": WEAVE, "BOB": BOB, "LINEAR": LINEAR}
# name -> (ug_pixfmt_t, element class, the reference's codec name)
FORMATS = {
    "RGBA": (1, "u8", "RGBA"), "UYVY": (2, "u8", "UYVY"), "YUYV": (3, "u8", "YUYV"), "RGB": (4, "u8", "RGB"), "BGR": (5, "u8", "BGR"),
    "VUYA": (15, "u8", "VUYA"), "RG48": (7, "u16", "RG48"), "Y216": (13, "u16", "Y216"), "Y416": (14, "u16", "Y416"),
    "v210": (6, "v210", "v210"), "R10k": (11, "r10k", "R10k"), "R12L": (12, "r12l", "R12L"),
}
UNIT = {"u8": 1, "u16": 2, "v210": 4, "r10k": 4, "r12l": 4}


def written_bytes(cls: str, linear: bool, L: int) -> int:
    """how many bytes of a line an AVERAGED line writes -- the reference's loop bounds (the rest of the destination line keeps its bytes)"""
    if cls == "u8":
        return L
    if cls == "u16":  # vc_deinterlace_ex's tail loop never runs behind a vector loop that ran (x86-64, -msse4.1; :759,769)
        return L if linear or L < 16 else L // 16 * 16
    if cls == "v210":
        return L // 16 * 16
    if cls == "r10k":  # avg_lines walks 4 lines' worth (temporal-deint.c:385-387): the stand-in's one line
        return L if linear else L // 16 * 16
    n = L // 16 * 4 if linear else L // 36 * 8  # r12l: words the loop walks; the last one is stored only if it ends on a sample boundary
    return 4 * (n - (n % 3 != 0))


def _avg_elems(a, b):
    return (a + b + 1) // 2


def _r12l_samples(v: np.ndarray) -> np.ndarray:
    """[n, 3 g] words -> [n, 8 g] 12-bit samples: 8 samples lie in 3 words, the third and the sixth across a word boundary"""
    w = v.reshape(v.shape[0], -1, 3).astype(np.uint64)
    w0, w1, w2 = w[..., 0], w[..., 1], w[..., 2]
    s = [w0 & 0xFFF, w0 >> 12 & 0xFFF, w0 >> 24 | (w1 & 0xF) << 8, w1 >> 4 & 0xFFF, w1 >> 16 & 0xFFF, w1 >> 28 | (w2 & 0xFF) << 4,
         w2 >> 8 & 0xFFF, w2 >> 20]
    return np.stack(s, axis=-1)


def avg_line(cls: str, linear: bool, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """the averaged bytes [0, written_bytes) of lines a and b (a = the upper ones): [n, L] -> [n, W]; one line each: [L] -> [W]"""
    if a.ndim == 1:
        return avg_line(cls, linear, a[None, :], b[None, :])[0]
    n, L = a.shape
    W = written_bytes(cls, linear, L)
    a, b = np.ascontiguousarray(a[:, :W] if cls != "r12l" else a), np.ascontiguousarray(b[:, :W] if cls != "r12l" else b)
    if W == 0:
        return np.zeros((n, 0), np.uint8)
    if cls in ("u8", "u16"):
        dt = np.uint8 if cls == "u8" else np.dtype("<u2")
        x, y = a.view(dt).astype(np.uint32), b.view(dt).astype(np.uint32)
        r = x // 2 + y // 2 + (x % 2 + x % 2) // 2 if linear else _avg_elems(x, y)  # avg_lines_per_elem is not the rounded average
        return r.astype(dt).view(np.uint8)
    if cls == "v210":
        x, y = a.view("<u4").astype(np.uint64), b.view("<u4").astype(np.uint64)
        r = (_avg_elems(x >> 20, y >> 20) << 20) | (_avg_elems(x >> 10 & 0x3FF, y >> 10 & 0x3FF) << 10) | _avg_elems(x & 0x3FF, y & 0x3FF)
        return (r & 0xFFFFFFFF).astype("<u4").view(np.uint8)
    if cls == "r10k":
        x, y = a.view(">u4").astype(np.uint64), b.view(">u4").astype(np.uint64)
        r = (_avg_elems(x >> 22, y >> 22) << 22) | (_avg_elems(x >> 12 & 0x3FF, y >> 12 & 0x3FF) << 12) | (_avg_elems(x >> 2 & 0x3FF, y >> 2 & 0x3FF) << 2)
        # avg_lines reads the words with ntohl and stores the result as it is (temporal-deint.c:388-393): its lines come out byte-swapped
        return (r & 0xFFFFFFFF).astype("<u4" if linear else ">u4").view(np.uint8)
    # r12l: a little-endian bit stream of 12-bit samples over the words the loop walks (padded with zero words to whole groups of 3: the samples
    # that lie inside the written bytes never reach the padding)
    n_words = L // 16 * 4 if linear else L // 36 * 8
    pad = (-n_words) % 3
    def words(v):
        return np.concatenate([v[:, : n_words * 4].view("<u4"), np.zeros((n, pad), "<u4")], axis=1)
    r = _avg_elems(_r12l_samples(words(a)), _r12l_samples(words(b)))  # [n, g, 8]
    o0 = r[..., 0] | r[..., 1] << 12 | (r[..., 2] & 0xFF) << 24
    o1 = r[..., 2] >> 8 | r[..., 3] << 4 | r[..., 4] << 16 | (r[..., 5] & 0xF) << 28
    o2 = r[..., 5] >> 4 | r[..., 6] << 8 | r[..., 7] << 20
    out = np.stack([o0, o1, o2], axis=-1).reshape(n, -1).astype("<u4").view(np.uint8)
    return out[:, :W]


def blend(cls: str, src: np.ndarray, L: int, bg: np.ndarray) -> np.ndarray:
    """vc_deinterlace_ex(src -> a destination that held `bg`); in place: bg = src"""
    H = src.shape[0]
    out = bg.copy()
    if H == 1:
        out[0, :L] = src[0, :L]
        return out
    W = written_bytes(cls, False, L)
    out[: H - 1, :W] = avg_line(cls, False, src[: H - 1, :L], src[1:, :L])
    out[H - 1, :L] = out[H - 2, :L]
    return out


def weave(cls: str, cur: np.ndarray, prev: np.ndarray, L: int, bgs, deint: bool = False):
    """perform_df: the frames postprocess(in) and postprocess(NULL) leave (even number of lines)"""
    H = cur.shape[0]
    assert H % 2 == 0
    o0, o1 = bgs[0].copy(), bgs[1].copy()
    o0[0::2, :L] = cur[0::2, :L]
    o0[1::2, :L] = prev[1::2, :L]
    o1[:, :L] = cur[:, :L]
    if deint:
        o0, o1 = blend(cls, o0, L, o0), blend(cls, o1, L, o1)
    return o0, o1


def bob(cls: str, src: np.ndarray, L: int, bgs):
    H = src.shape[0]
    assert H >= 2
    o0, o1 = bgs[0].copy(), bgs[1].copy()
    y = 0
    while y < H - 1:  # postprocess(in): every even line twice
        o0[y, :L] = o0[y + 1, :L] = src[y, :L]
        y += 2
    if y < H:
        o0[y, :L] = o0[y - 1, :L]
    o1[0, :L] = src[1, :L]  # postprocess(NULL): the first odd line up, then every odd line twice
    y = 1
    while y < H - 1:
        o1[y, :L] = o1[y + 1, :L] = src[y, :L]
        y += 2
    if y < H:
        o1[y, :L] = o1[y - 1, :L]
    return o0, o1


def linear(cls, src: np.ndarray, L: int, bgs):
    """cls None: a codec avg_lines does not take -- the line above instead of the average (the reference's "fallback bob")"""
    H = src.shape[0]
    assert H >= 2
    W = written_bytes(cls, True, L) if cls else L
    outs = []
    for first, bg in ((0, bgs[0]), (1, bgs[1])):
        o = bg.copy()
        y = first
        if first:
            o[0, :L] = src[1, :L]
        while y < H - 2:
            o[y, :L] = src[y, :L]
            o[y + 1, :W] = avg_line(cls, True, src[y, :L], src[y + 2, :L]) if cls else src[y, :L]
            y += 2
        last = y  # "last line(s) if needed": the source pointer does not advance (temporal-deint.c:462-465) -- two lines left get the same line
        while y < H:
            o[y, :L] = src[last, :L]
            y += 1
        outs.append(o)
    return outs[0], outs[1]


def run(cls: str, mode: int, src: np.ndarray, L: int, bgs, prev=None, deint: bool = False):
    """both outputs of `mode` (BLEND: one) for destinations that held bgs"""
    if mode == BLEND:
        return (blend(cls, src, L, bgs[0]),)
    if mode == WEAVE:
        return weave(cls, src, prev, L, bgs, deint)
    return bob(cls, src, L, bgs) if mode == BOB else linear(cls, src, L, bgs)


def module_run(name: str, opts: str, cls, active: bool, L: int, pitch: int, frames):
    """What a *_mi355x postprocessor hands out for consecutive input frames ([H, L] arrays; a new size = a reconfigure) into output frames
    pre-filled with 0xA5: a list of (postprocess(in)'s frame, postprocess(NULL)'s frame or None).  name: the reference's module name; cls None: a
    codec the averages do not take; active: INTERLACED_MERGED input or `force`.  The frame before the first one is zero."""
    outs, prev = [], None
    for f in frames:
        H = f.shape[0]
        if prev is None or prev.shape != f.shape:
            prev = np.zeros_like(f)
        bg = np.full((H, pitch), 0xA5, np.uint8)
        plain = bg.copy()
        plain[:, :L] = f
        if name in ("deinterlace", "deinterlace_blend"):
            outs.append((blend(cls, f, L, bg) if active and cls else plain, None))
        elif not active:
            outs.append((plain, plain.copy()))
        elif name == "double_framerate":
            outs.append(weave(cls, f, prev, L, (bg, bg), deint=opts == "d" and cls is not None))
        elif name == "deinterlace_bob":
            outs.append(bob(cls, f, L, (bg, bg)))
        else:
            outs.append(linear(cls, f, L, (bg, bg)))
        prev = f
    return outs
