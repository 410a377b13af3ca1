"""Reference writer of four-component (R, G, B, alpha) baseline JPEG streams: the layout subsampling=4444 asks of the encoder -- the R,G,B 4:4:4
stream of tests/jpeg_bitstream.py with a fourth component 'A' behind, every component 1x1 with quantiser and Huffman table 0.  Built from that
module's pieces; the module itself stays as it is."""
import io
import struct

import numpy as np

from jpeg_bitstream import AC_C, AC_L, DC_C, DC_L, ZIGZAG, _Bits, _block, _codes

IDS = (0x52, 0x47, 0x42, 0x41)  # 'R', 'G', 'B', 'A'


def write_jpeg4444(width, height, ql, qc, coefs, restart=0, nonint=False):
    """coefs: four (n_blocks, 64) int16 zig-zag arrays over the 8x8-block grid (ceil(w / 8) x ceil(h / 8), raster order), R, G, B, A.
    Interleaved: both quantiser tables and all four Huffman tables in the header (as the R,G,B writer), one scan of MCUs of four blocks.
    nonint: one scan per component (T.81 A.2.2), the header carries table 0 only.  restart counts MCUs (interleaved) / blocks (nonint)."""
    bw_, bh_ = (width + 7) // 8, (height + 7) // 8
    n = bw_ * bh_
    out = io.BytesIO()
    out.write(b"\xff\xd8")
    out.write(b"\xff\xee" + struct.pack(">H5sHHHB", 14, b"Adobe", 100, 0, 0, 0))
    for tid, qt in ((0, ql),) + (() if nonint else ((1, qc),)):
        out.write(b"\xff\xdb" + struct.pack(">HB", 67, tid) + bytes(int(qt[i]) for i in ZIGZAG))
    out.write(b"\xff\xc0" + struct.pack(">HBHHB", 20, 8, height, width, 4) + b"".join(bytes([i, 0x11, 0]) for i in IDS))
    tables = ((0, 0, DC_L), (1, 0, AC_L)) + (() if nonint else ((0, 1, DC_C), (1, 1, AC_C)))
    for (tc, th, (bits, vals)) in tables:
        out.write(b"\xff\xc4" + struct.pack(">HB", 19 + len(vals), (tc << 4) | th) + bytes(bits) + bytes(vals))
    if restart:
        out.write(b"\xff\xdd" + struct.pack(">HH", 4, restart))
    dcl, acl = _codes(*DC_L), _codes(*AC_L)

    def scan(comps):
        bw = _Bits()
        pred = [0] * 4
        for u in range(n):
            if restart and u and u % restart == 0:
                bw.flush()
                out.write(bytes(bw.buf))
                out.write(bytes([0xFF, 0xD0 + ((u // restart - 1) & 7)]))
                bw = _Bits()
                pred = [0] * 4
            for c in comps:
                pred[c] = _block(bw, coefs[c][u], pred[c], dcl, acl)
        bw.flush()
        out.write(bytes(bw.buf))

    if nonint:
        for c in range(4):
            out.write(b"\xff\xda" + struct.pack(">HB", 8, 1) + bytes([IDS[c], 0x00, 0, 63, 0]))
            scan((c,))
    else:
        out.write(b"\xff\xda" + struct.pack(">HB", 14, 4) + b"".join(bytes([i, 0x00]) for i in IDS) + bytes([0, 63, 0]))
        scan((0, 1, 2, 3))
    out.write(b"\xff\xd9")
    return out.getvalue()


def coefs4444(po, rgba, ql):
    """the four coefficient planes of an (h, w, 4) RGBA picture: the oracle's FDCT + quantiser per channel, table-0 divisors"""
    div = po.jpeg_divisors(ql)
    return [po.jpeg_fdct_quant_plane(np.ascontiguousarray(rgba[..., c]), div) for c in range(4)]


def rgba_picture(w, h, seed=0):
    """smooth colour + a soft alpha ramp + a little noise: every path of the coder, streams of a realistic size"""
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(xx / 20.0) * np.cos(yy / 15.0), 128 + 90 * np.cos(xx / 33.0 + yy / 21.0), 128 + 80 * np.sin(yy / 9.0),
                     255 * (xx + yy) / max(1, w + h - 2)], -1)
    return (base + np.random.default_rng(seed + w * h).normal(0, 3, base.shape)).clip(0, 255).astype(np.uint8)
