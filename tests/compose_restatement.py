"""numpy restatement of the reference's geometric and compositing filters (src/vo_postprocess/crop.c, border.c, interlace.c, 3d-interlaced.c,
split.c with src/utils/vf_split.cpp, src/capture_filter/logo.c) and of their geometry -- what ug_hip_compose and its three host helpers are held
to.  The line converters of LOGO and of BORDER's UYVY word are the pixfmt oracle's (oracle/pixfmt_oracle.c through oracle.pyoracle), RG48's two
are stated here (vc_copylineRG48toRGB takes the high bytes, vc_copylineRGBtoRG48 writes them over zero low bytes, pixfmt_conv.c:2031-2043, 1353-1363).

Every function takes and returns flat uint8 arrays of whole lines (vc_get_linesize).  Where the reference leaves its buffers the functions state
what ug_hip_compose does instead (include/ug_mi355x.h "Deviations"); logo_inside() / dec_width() say for which logos that is the reference too."""
import numpy as np

from oracle import pyoracle as po

# block bytes, block pixels, h_align (video_codec.c:120-206)
BLOCK = {"RGBA": (4, 1, 1), "UYVY": (4, 2, 2), "YUYV": (4, 2, 2), "RGB": (3, 1, 1), "BGR": (3, 1, 1), "v210": (16, 6, 48), "R10k": (4, 1, 64),
         "R12L": (36, 8, 8), "Y216": (8, 2, 2), "Y416": (8, 1, 1), "VUYA": (4, 1, 1), "RG48": (6, 1, 1), "DVS10": (16, 6, 48)}


def linesize(codec, w):
    """vc_get_linesize (video_codec.c:507-521)"""
    bb, bp, ha = BLOCK[codec]
    w = (w + ha - 1) // ha * ha
    return (w + bp - 1) // bp * bb


def bpp(codec):
    """get_bpp (video_codec.c:309-320): a double"""
    return BLOCK[codec][0] / BLOCK[codec][1]


def _tdiv(a, b):
    """C's integer division: toward zero"""
    q = abs(a) // b
    return q if a >= 0 else -q


# ------------------------------------------------------------------ geometry ------------------------------------------------------------------
def crop_geometry(codec, in_w, in_h, want_w, want_h, xoff, yoff):
    """crop.c:141-148, 170-173 -> (out_w, out_h, xoff_bytes, yoff); Python floats are the reference's doubles"""
    bb = BLOCK[codec][0]
    w = min(want_w, in_w) if want_w else in_w
    h = min(want_h, in_h) if want_h else in_h
    ls = int(w * bpp(codec)) // bb * bb
    w = int(ls / bpp(codec))
    xo = in_w - w if xoff + w > in_w else xoff
    xb = int(xo * bpp(codec)) // bb * bb
    yo = in_h - h if yoff + h > in_h else yoff
    return w, h, xb, yo


def logo_geometry(codec, frame_w, frame_h, logo_w, logo_h, x, y):
    """logo.c:182-193 -> (rect_x, rect_y): the pixel position rounded by the block's BYTE count, toward zero"""
    bb = BLOCK[codec][0]
    rx, ry = x, y
    if rx < 0 or rx + logo_w > frame_w:
        rx = frame_w - logo_w
    rx = _tdiv(rx, bb) * bb
    if ry < 0 or ry + logo_h > frame_h:
        ry = frame_h - logo_h
    return rx, ry


def dec_width(codec, logo_w):
    """logo.c:198-199: the pixels per line of the reference's RGB segment"""
    bb = BLOCK[codec][0]
    return (logo_w + 1) // bb * bb


def logo_inside(codec, logo_w):
    """the reference blends logo_w pixels per line of a segment dec_width wide, and its UYVY coder reads one pixel more for an odd width"""
    need = logo_w + (1 if codec == "UYVY" and logo_w % 2 else 0)
    return dec_width(codec, logo_w) >= need


def border_pattern(codec, rgba):
    """border.c:161-166 -> 4 bytes"""
    rgba = np.asarray(rgba, np.uint8)
    if codec in ("RGB", "RGBA"):
        return rgba.copy()
    assert codec == "UYVY"
    return po.convert_frame("RGBA", "UYVY", np.concatenate([rgba, rgba]), 2, 1)[:4].copy()


# --------------------------------------------------------------------- ops ---------------------------------------------------------------------
def crop(codec, data, in_w, in_h, out_lines, xoff_bytes, yoff, line_bytes):
    """crop.c:175-179 with line_bytes for req_pitch"""
    ls = linesize(codec, in_w)
    assert 0 <= xoff_bytes and xoff_bytes + line_bytes <= ls and 0 <= yoff and yoff + out_lines <= in_h
    rows = np.asarray(data, np.uint8)[: ls * in_h].reshape(in_h, ls)
    return rows[yoff: yoff + out_lines, xoff_bytes: xoff_bytes + line_bytes].reshape(-1).copy()


def interlace(codec, first, second, w, h):
    """interlace.c:172-181: even lines from the first frame the module received, odd ones from the second"""
    ls = linesize(codec, w)
    out = np.asarray(first, np.uint8)[: ls * h].reshape(h, ls).copy()
    out[1::2] = np.asarray(second, np.uint8)[: ls * h].reshape(h, ls)[1::2]
    return out.reshape(-1)


def interlaced_3d(codec, eye0, eye1, w, h):
    """3d-interlaced.c:152-169 per byte, lines at the line size (the deviation: the reference packs 16-byte steps across lines)"""
    assert h % 2 == 0
    ls = linesize(codec, w)
    out = np.zeros((h, ls), np.uint8)
    for x in range(h):
        t = np.asarray((eye0, eye1)[x % 2], np.uint8)[: ls * h].reshape(h, ls).astype(np.uint16)
        out[x] = (t[x // 2 * 2] + t[x // 2 * 2 + 1] + 1) >> 1
    return out.reshape(-1)


def split_tile_bytes(codec, tile_w):
    """tile_width * get_bpp as vf_split.cpp:104-106 passes it to memcpy, or None where that is no whole number of blocks of a fractional format"""
    bb, bp, _ = BLOCK[codec]
    if bb % bp and tile_w % bp:
        return None
    return tile_w * bb // bp


def split(codec, data, w, h, gx, gy, fill=0):
    """vf_split.cpp:79-108 -> list of gx * gy tiles, each tile_h lines of vc_get_linesize(tile_w) bytes; the bytes past tile_w * get_bpp (an odd
    UYVY tile width) are not written: they hold `fill`"""
    assert w % gx == 0 and h % gy == 0
    tw, th = w // gx, h // gy
    n, ls, tls = split_tile_bytes(codec, tw), linesize(codec, w), linesize(codec, tw)
    rows = np.asarray(data, np.uint8)[: ls * h].reshape(h, ls)
    tiles = []
    for ty in range(gy):
        for tx in range(gx):
            t = np.full((th, tls), fill, np.uint8)
            t[:, :n] = rows[ty * th: (ty + 1) * th, tx * n: (tx + 1) * n]
            tiles.append(t.reshape(-1))
    return tiles


def border(codec, data, w, h, bw, bh, pattern):
    """border.c:158-208"""
    assert codec in ("UYVY", "RGB", "RGBA") and 0 <= bw <= w and 0 <= 2 * bh <= h
    ls = linesize(codec, w)
    out = np.asarray(data, np.uint8)[: ls * h].reshape(h, ls).copy()
    pat = np.asarray(pattern, np.uint8)[: 3 if codec == "RGB" else 4]
    full = np.resize(pat, ls)  # the pattern repeated from byte 0 of the line
    side = (bw + 1) // 2 * 4 if codec == "UYVY" else bw * pat.size
    if bh:
        out[:bh] = full
        out[h - bh:] = full
    if side:
        out[:, :side] = full[:side]
        out[:, ls - side:] = full[ls - side:]
    return out.reshape(-1)


def _decode(codec, seg, npix):
    if codec == "RG48":
        return seg.reshape(-1, 2)[: 3 * npix, 1].copy()
    return po.convert_frame(codec, "RGB", seg, npix, 1)[: 3 * npix].copy()


def _encode(codec, rgb, npix):
    if codec == "RG48":
        out = np.zeros((3 * npix, 2), np.uint8)
        out[:, 1] = rgb[: 3 * npix]
        return out.reshape(-1)
    return po.convert_frame("RGB", codec, rgb, npix, 1)[: linesize(codec, npix)].copy()


def logo(codec, data, w, h, overlay, lw, lh, rect_x, rect_y):
    """logo.c:198-230 with every logo pixel blended over its own decoded frame pixel: the reference wherever logo_inside().  In place on a copy."""
    ls = linesize(codec, w)
    out = np.asarray(data, np.uint8)[: ls * h].copy()
    if rect_x < 0 or rect_y < 0:
        return out
    assert rect_x + lw <= w and rect_y + lh <= h and (codec != "UYVY" or rect_x % 2 == 0)
    ov = np.asarray(overlay, np.uint8)[: 4 * lw * lh].reshape(lh, lw, 4).astype(np.int64)
    npix = lw + (lw % 2 if codec == "UYVY" else 0)  # the coder works on whole pairs: vc_get_linesize(lw)
    off, nbytes = linesize(codec, rect_x) if rect_x else 0, linesize(codec, npix)
    for y in range(lh):
        at = (rect_y + y) * ls + off
        rgb = _decode(codec, out[at: at + nbytes].copy(), npix).reshape(npix, 3).astype(np.int64)
        a = ov[y, :, 3:4]
        rgb[:lw] = (rgb[:lw] * (255 - a) + ov[y, :, :3] * a) // 255
        out[at: at + nbytes] = _encode(codec, rgb.astype(np.uint8).reshape(-1), npix)
    return out


# ------------------------------------------------------------------- modules -------------------------------------------------------------------
def parse_crop(options):
    """crop.c:98-124 -> (width, height, xoff, yoff)"""
    v = dict(width=0, height=0, xoff=0, yoff=0)
    for item in filter(None, options.split(":")):
        key, _, val = item.partition("=")
        if key == "size":
            v["width"], v["height"] = (int(x) for x in val.split("x"))
        else:
            v[key.lower()] = int(val)
    return v["width"], v["height"], v["xoff"], v["yoff"]


def parse_border(options):
    """border.c:73-125 -> (border_w, border_h, R,G,B,A): a six-digit colour is read from its SECOND digit on (`color += 1` twice over, :90-95), so
    rrggbb gives r2g1, g2b1, b2; width and height are rounded up to even"""
    bw, bh, colour = 10, 10, [0xff, 0xff, 0x00, 0xff]
    for item in filter(None, options.split(":")):
        key, _, val = item.partition("=")
        if key.lower() == "color":
            c = val[1:] if val.startswith("#") else val
            assert len(c) == 6
            colour[:3] = [int(c[1:3], 16), int(c[3:5], 16), int(c[5:6], 16)]
        elif key.lower() == "width":
            bw = (int(val) + 1) // 2 * 2
        else:
            assert key.lower() == "height"
            bh = (int(val) + 1) // 2 * 2
    return bw, bh, colour


FILL = 0xA5  # what the harness and the tests put into every output buffer beforehand: bytes a module leaves alone still hold it


class Module:
    """one state of a module: frame(w, h, tiles) -> dict(ret, w, h, tile_count, interlacing, fps, out); `overlay` = (R,G,B,A bytes, lw, lh) for logo.
    ret: pp true / false, cf new / same / null.  interlacing 0 = PROGRESSIVE, 3 = INTERLACED_MERGED (types.h)"""

    def __init__(self, name, options, codec, overlay=None):
        self.name, self.options, self.codec, self.overlay = name, "" if options == "-" else options, codec, overlay
        self.first, self.size = None, None  # interlace: the frame waiting for its pair; a size change starts a new pair

    def frame(self, w, h, tiles, fps=25.0):
        c, t0 = self.codec, tiles[0]
        if self.size != (w, h):
            self.first, self.size = None, (w, h)
        r = dict(ret="true", w=w, h=h, tile_count=1, interlacing=0, fps=fps)
        if self.name == "crop":
            ow, oh, xb, yo = crop_geometry(c, w, h, *parse_crop(self.options))
            lb = min(linesize(c, ow), linesize(c, w) - xb)
            r.update(w=ow, h=oh, out=crop(c, t0, w, h, oh, xb, yo, lb), line_bytes=lb)
        elif self.name == "border":
            bw, bh, colour = parse_border(self.options)
            r["out"] = border(c, t0, w, h, bw, bh, border_pattern(c, colour))
        elif self.name == "interlace":
            r.update(interlacing=3, fps=fps / 2)
            if self.first is None:
                self.first = np.array(t0, np.uint8)
                r["ret"] = "false"
            else:
                r["out"] = interlace(c, self.first, t0, w, h)
                self.first = None
        elif self.name == "interlaced_3d":
            r["out"] = interlaced_3d(c, t0, tiles[1], w, h)
        elif self.name == "split":
            gx, gy = (int(x) for x in self.options.split(":"))
            r.update(w=w // gx, h=h // gy, tile_count=gx * gy, out=np.concatenate(split(c, t0, w, h, gx, gy, fill=FILL)))
        else:
            assert self.name == "logo"
            ov, lw, lh = self.overlay
            pos = [int(x) for x in self.options.split(":")[1:3]]
            x, y = (pos + [-1, -1])[:2] if pos else (-1, -1)
            if len(pos) == 1:
                y = -1
            rx, ry = logo_geometry(c, w, h, lw, lh, x, y)
            r.update(ret="same", out=logo(c, t0, w, h, ov, lw, lh, rx, ry), rect=(rx, ry))
        return r
