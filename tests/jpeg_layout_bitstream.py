"""Reference writer of three-component baseline JPEG streams with any sampling factors (T.81 A.1.1, A.2): per-component H x V, one
interleaved scan or one scan per component, restart intervals, Y'CbCr (JFIF, ids 1, 2, 3, the chroma tables for Cb and Cr) or R,G,B (table 0
for every component; marked by Adobe APP14 transform 0 and / or the component ids 'R', 'G', 'B').  Built from tests/jpeg_bitstream.py's
pieces; that module stays as it is.  Not part of the product."""
import io
import struct

import numpy as np

from jpeg_bitstream import AC_C, AC_L, DC_C, DC_L, ZIGZAG, _Bits, _block, _codes

# the layouts read_info has a code for: code -> (luma H, V), chroma 1x1, plus others with the same chroma ratio
LAYOUTS = {
    444: ((1, 1), (1, 1)),
    422: ((2, 1), (1, 1)),
    420: ((2, 2), (1, 1)),
    440: ((1, 2), (1, 1)),
    411: ((4, 1), (1, 1)),
    410: ((4, 2), (1, 1)),
}


def geometry(width, height, factors):
    """(hmax, vmax, mcu_w, mcu_h, [(grid blocks w, h)], [(component width, height)])"""
    hmax, vmax = max(f[0] for f in factors), max(f[1] for f in factors)
    mw, mh = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    grids = [(mw * hs, mh * vs) for hs, vs in factors]
    sizes = [(-(-width * hs // hmax), -(-height * vs // vmax)) for hs, vs in factors]
    return hmax, vmax, mw, mh, grids, sizes


def write_layout_jpeg(width, height, factors, ql, qc, coefs, restart=0, nonint=False, rgb=None):
    """factors: three (H, V).  coefs: three (blocks, 64) int16 zig-zag arrays, raster order over each component's MCU-padded block grid
    (geometry()).  rgb: None (Y'CbCr), "adobe" (Adobe transform 0, ids 1, 2, 3), "ids" (ids 'R', 'G', 'B', no Adobe marker), "both".
    restart counts MCUs (interleaved) or the component's blocks (one scan per component)."""
    hmax, vmax, mw, mh, grids, sizes = geometry(width, height, factors)
    out = io.BytesIO()
    out.write(b"\xff\xd8")
    if rgb in ("adobe", "both"):
        out.write(b"\xff\xee" + struct.pack(">H5sHHHB", 14, b"Adobe", 100, 0, 0, 0))
    elif rgb is None:
        out.write(b"\xff\xe0" + struct.pack(">H5sBBBHHBB", 16, b"JFIF\0", 1, 1, 0, 1, 1, 0, 0))
    ids = (0x52, 0x47, 0x42) if rgb in ("ids", "both") else (1, 2, 3)
    t = (0, 0, 0) if rgb else (0, 1, 1)
    for tid, qt in ((0, ql),) + (() if rgb else ((1, qc),)):
        out.write(b"\xff\xdb" + struct.pack(">HB", 67, tid) + bytes(int(qt[i]) for i in ZIGZAG))
    out.write(b"\xff\xc0" + struct.pack(">HBHHB", 17, 8, height, width, 3) +
              b"".join(bytes([ids[c], (factors[c][0] << 4) | factors[c][1], t[c]]) for c in range(3)))
    for (tc, th, (bits, vals)) in ((0, 0, DC_L), (1, 0, AC_L)) + (() if rgb else ((0, 1, DC_C), (1, 1, AC_C))):
        out.write(b"\xff\xc4" + struct.pack(">HB", 19 + len(vals), (tc << 4) | th) + bytes(bits) + bytes(vals))
    if restart:
        out.write(b"\xff\xdd" + struct.pack(">HH", 4, restart))
    tabs = [(_codes(*DC_L), _codes(*AC_L)), (_codes(*DC_C), _codes(*AC_C))]

    def scan(units, blocks_of):
        """units: number of data units / MCUs; blocks_of(u) -> [(component, block index)] in coding order"""
        bw = _Bits()
        pred = [0, 0, 0]
        for u in range(units):
            if restart and u and u % restart == 0:
                bw.flush()
                out.write(bytes(bw.buf))
                out.write(bytes([0xFF, 0xD0 + ((u // restart - 1) & 7)]))
                bw = _Bits()
                pred = [0, 0, 0]
            for c, b in blocks_of(u):
                dc, ac = tabs[t[c]]
                pred[c] = _block(bw, coefs[c][b], pred[c], dc, ac)
        bw.flush()
        out.write(bytes(bw.buf))

    if nonint:
        for c in range(3):
            out.write(b"\xff\xda" + struct.pack(">HB", 8, 1) + bytes([ids[c], t[c] * 0x11, 0, 63, 0]))
            b1w, b1h = -(-sizes[c][0] // 8), -(-sizes[c][1] // 8)
            gw = grids[c][0]
            scan(b1w * b1h, lambda u, c=c, b1w=b1w, gw=gw: [(c, (u // b1w) * gw + u % b1w)])
    else:
        out.write(b"\xff\xda" + struct.pack(">HB", 12, 3) + b"".join(bytes([ids[c], t[c] * 0x11]) for c in range(3)) + bytes([0, 63, 0]))

        def mcu(u):
            my, mx = divmod(u, mw)
            return [(c, (my * vs + by) * grids[c][0] + mx * hs + bx) for c, (hs, vs) in enumerate(factors) for by in range(vs) for bx in range(hs)]
        scan(mw * mh, mcu)
    out.write(b"\xff\xd9")
    return out.getvalue()


def downsample(plane, rx, ry):
    """block averaging over rx x ry (edges replicated to whole blocks), rounded half up: ceil(h / ry) x ceil(w / rx)"""
    h, w = plane.shape
    ph, pw = -(-h // ry) * ry, -(-w // rx) * rx
    p = np.pad(plane.astype(np.int32), ((0, ph - h), (0, pw - w)), mode="edge")
    s = p.reshape(ph // ry, ry, pw // rx, rx).sum(axis=(1, 3))
    return ((s + (rx * ry) // 2) // (rx * ry)).astype(np.uint8)


def layout_coefs(po, picture, factors, ql, qc, rgb):
    """the coefficient planes of an (h, w, 3) picture (its channels taken as the three components as they are): each channel downsampled to
    its component's size, then the oracle's FDCT + quantiser over the component's MCU-padded block grid"""
    h, w, _ = picture.shape
    hmax, vmax, _, _, grids, _ = geometry(w, h, factors)
    out = []
    for c, (hs, vs) in enumerate(factors):
        plane = downsample(np.ascontiguousarray(picture[..., c]), hmax // hs, vmax // vs)
        div = po.jpeg_divisors(ql if (rgb or c == 0) else qc)
        out.append(po.jpeg_fdct_quant_plane(plane, div, grids[c][0], grids[c][1]))
    return out


def picture(w, h, seed=0):
    """smooth colour with a little noise: every path of the coder, streams of a realistic size"""
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(xx / 23.0) * np.cos(yy / 17.0), 128 + 90 * np.cos(xx / 31.0 + yy / 19.0), 128 + 80 * np.sin(yy / 11.0 + xx / 41.0)], -1)
    return (base + np.random.default_rng(seed + 7 * w + h).normal(0, 3, base.shape)).clip(0, 255).astype(np.uint8)


def layout_stream(po, w, h, code, restart=0, nonint=False, rgb=None, q=75, seed=0, factors=None):
    """a stream of the layout `code` (LAYOUTS) or of explicit factors"""
    if factors is None:
        y, c = LAYOUTS[code]
        factors = (y, c, c)
    ql, qc = po.jpeg_qtable(q, 0), po.jpeg_qtable(q, 1)
    x = picture(w, h, seed)
    return write_layout_jpeg(w, h, factors, ql, qc, layout_coefs(po, x, factors, ql, qc, rgb), restart=restart, nonint=nonint, rgb=rgb)
