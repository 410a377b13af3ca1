"""GPU: ug_hip_compose against the numpy restatement (tests/compose_restatement.py) and the fixture (tests/golden/compose_ref.npz, whose `inside`
cases are the reference's own bytes), 0 bytes differing: every case of the fixture through codec.compose as a module would call it, the six ops at
the widths where the unit, word and byte paths and more than one workgroup meet, frames = 1 and 3 with padded strides, pitched and deliberately
misaligned buffers (tests/pitch_layout.py: every byte outside the written lines keeps its fill), LOGO in place."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import compose_restatement as rs  # noqa: E402
import make_compose_golden as gen  # noqa: E402
import pitch_layout as pl  # noqa: E402

from ultragrid_amd import codec, lib  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(HERE, "golden", "compose_ref.npz"))
META = json.loads(str(GOLD["meta"]))
IDS = [f"{k}-{m['kind']}-{m['name']}-{m['codec']}-{'x'.join(map(str, m['frames'][0]))}" for k, m in enumerate(META)]
PF = dict(lib.PF_NAMES)
OPS = {"crop": lib.CMP_CROP, "border": lib.CMP_BORDER, "logo": lib.CMP_LOGO, "interlace": lib.CMP_INTERLACE, "interlaced_3d": lib.CMP_INTERLACED_3D,
       "split": lib.CMP_SPLIT}
RUNNABLE = [k for k, m in enumerate(META) if not (m["codec"] == "v210" and m["name"] in ("border", "logo"))]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def module_run(m, k):
    """the frames of a fixture case through codec.compose, with the state a module keeps (interlace's first frame, logo's uploaded overlay)
    -> per frame the bytes, None where nothing comes out, or the UgHipError"""
    op, fmt, out, first, size = OPS[m["name"]], PF[m["codec"]], [], None, None
    overlay = _dev(GOLD[f"logo_{k}"]) if m["logo"] else None
    for w, h in m["frames"]:
        data = GOLD[f"in_{m['codec']}_{w}x{h}x{m['tiles']}"]
        n = data.size // m["tiles"]
        try:
            if m["name"] == "crop":
                r = codec.compose(op, fmt, _dev(data), w, h, crop=rs.parse_crop(m["options"]))
            elif m["name"] == "border":
                bw, bh, colour = rs.parse_border("" if m["options"] == "-" else m["options"])
                r = codec.compose(op, fmt, _dev(data), w, h, border=(bw, bh, colour))
            elif m["name"] == "interlace":
                if size != (w, h):
                    first, size = None, (w, h)
                if first is None:
                    first, r = _dev(data), None
                else:
                    r, first = codec.compose(op, fmt, first, w, h, src2=_dev(data)), None
            elif m["name"] == "interlaced_3d":
                r = codec.compose(op, fmt, _dev(data[:n]), w, h, src2=_dev(data[n:]))
            elif m["name"] == "split":
                gx, gy = (int(x) for x in m["options"].split(":"))
                dst = torch.full((rs.linesize(m["codec"], w // gx) * h * gx,), rs.FILL, dtype=torch.uint8, device="cuda")
                r = codec.compose(op, fmt, _dev(data), w, h, grid=(gx, gy), dst=dst)
            else:
                pos = [int(x) for x in m["options"].split(":") if x] + [-1, -1]
                r = codec.compose(op, fmt, _dev(data), w, h, logo=(overlay, m["logo"][0], m["logo"][1], pos[0], pos[1]))
            torch.cuda.synchronize()
            out.append(None if r is None else r.cpu().numpy())
        except lib.UgHipError as e:
            out.append(e)
    return out


@pytest.mark.parametrize("k", RUNNABLE, ids=[IDS[k] for k in RUNNABLE])
def test_fixture_case(k):
    m = META[k]
    got = module_run(m, k)
    for i, (g, fm) in enumerate(zip(got, m["frames_meta"])):
        if fm["refused"]:  # a geometry where the reference leaves its buffers and nothing can be stated: refused before any device call
            assert isinstance(g, lib.UgHipError) and g.rc == lib.EINVAL, (i, g)
        elif f"out_{k}_{i}" not in GOLD.files:
            assert g is None and fm["ret"] == "false"
        else:
            want = GOLD[f"out_{k}_{i}"]
            assert not isinstance(g, Exception), g
            assert g.size == want.size and int(np.count_nonzero(g != want)) == 0, (i, int(np.count_nonzero(g != want)))


# ------------------------------------------------- the ops on pitched, offset and strided buffers -------------------------------------------------
WIDTHS = {"UYVY": (2, 6, 34, 130), "RGB": (1, 5, 43), "RGBA": (1, 6, 33), "RG48": (1, 3, 21), "v210": (48, 96)}
HEIGHT = {2: 1, 6: 2, 34: 3, 130: 5, 1: 1, 5: 4, 43: 3, 33: 6, 3: 2, 21: 5, 48: 4, 96: 6}


def _rand(n, rng):
    return np.frombuffer(rng.bytes(n), np.uint8).copy()


class Case:
    """one op on one geometry: the descriptor's own fields, the input tiles of a frame and the expected output of a frame as (lines, bytes per line)"""

    def __init__(self, op, cn, w, h, **prm):
        self.op, self.cn, self.w, self.h, self.prm = op, cn, w, h, prm
        self.ls = rs.linesize(cn, w)
        self.fields, self.two, self.overlay = {}, op in ("interlace", "interlaced_3d"), None
        if op == "crop":
            ow, oh, xb, yo = rs.crop_geometry(cn, w, h, *prm["crop"])
            self.lb, self.ol = min(rs.linesize(cn, ow), self.ls - xb), oh
            self.fields = dict(xoff_bytes=xb, yoff=yo, out_line_bytes=self.lb, out_lines=oh)
        elif op == "split":
            gx, gy = prm["grid"]
            self.lb, self.ol, self.tp = rs.split_tile_bytes(cn, w // gx), h * gx, rs.linesize(cn, w // gx)
            self.fields = dict(grid_x=gx, grid_y=gy)
        else:
            self.lb, self.ol = self.ls, h
            if op == "border":
                self.pattern = rs.border_pattern(cn, prm["colour"])
                self.fields = dict(border_w=prm["bw"], border_h=prm["bh"], fill=(C.c_ubyte * 4)(*self.pattern))
            if op == "logo":
                lw, lh, x, y = prm["logo"]
                rx, ry = rs.logo_geometry(cn, w, h, lw, lh, x, y)
                self.fields = dict(logo_w=lw, logo_h=lh, rect_x=rx, rect_y=ry)

    def make(self, rng):
        if self.op == "logo" and self.overlay is None:
            lw, lh = self.prm["logo"][:2]
            self.overlay = _rand(4 * lw * lh, rng)
            if self.prm.get("alpha") is not None:
                self.overlay[3::4] = self.prm["alpha"]
        return [_rand(self.ls * self.h, rng) for _ in range(2 if self.two else 1)]

    def expect(self, tiles):
        c, w, h, t0 = self.cn, self.w, self.h, tiles[0]
        if self.op == "crop":
            f = self.fields
            out = rs.crop(c, t0, w, h, f["out_lines"], f["xoff_bytes"], f["yoff"], f["out_line_bytes"])
        elif self.op == "border":
            out = rs.border(c, t0, w, h, self.prm["bw"], self.prm["bh"], self.pattern)
        elif self.op == "interlace":
            out = rs.interlace(c, t0, tiles[1], w, h)
        elif self.op == "interlaced_3d":
            out = rs.interlaced_3d(c, t0, tiles[1], w, h)
        elif self.op == "split":
            gx, gy = self.prm["grid"]
            return np.concatenate(rs.split(c, t0, w, h, gx, gy)).reshape(self.ol, self.tp)[:, : self.lb]
        else:
            lw, lh = self.prm["logo"][:2]
            out = rs.logo(c, t0, w, h, self.overlay, lw, lh, self.fields["rect_x"], self.fields["rect_y"])
        return out.reshape(self.ol, self.lb)


def run_layout(case, frames=1, sp=0, dp=0, src_off=0, dst_off=0, sgap=0, dgap=0, seed=7, expect=lib.SUCCESS):
    """`frames` pictures at these pitches, offsets (from 256-byte aligned device addresses) and gaps between the frames -> findings (empty = good).
    SPLIT: dp is the tile pitch, the tiles lie back to back.  LOGO: the destination holds the frames beforehand."""
    rng = np.random.default_rng(seed)
    ins = [case.make(rng) for _ in range(frames)]
    outs = [case.expect(t) for t in ins]
    sl, h, lb, ol = case.ls, case.h, case.lb, case.ol
    nat = case.tp if case.op == "split" else lb
    sp, dp = sp or sl, dp or nat
    sstride, dstride = sp * h + sgap, dp * ol + dgap
    srcs = []
    for t in range(2 if case.two else 1):
        src = pl.aligned_bytes(src_off + sstride * frames + pl.SLACK, rng=rng)
        for f in range(frames):
            for y in range(h):
                at = src_off + f * sstride + y * sp
                src[at: at + sl] = ins[f][t][y * sl: (y + 1) * sl]
        srcs.append(_dev(src))
    front = pl.GUARD + dst_off
    total = front + dstride * (frames - 1) + dp * ol + pl.GUARD
    want, start = pl.aligned_bytes(total, fill=pl.FILL), pl.aligned_bytes(total, fill=pl.FILL)
    for f in range(frames):
        for y in range(ol):
            at = front + f * dstride + y * dp
            want[at: at + lb] = outs[f][y]
            if case.op == "logo":
                start[at: at + lb] = ins[f][0][y * sl: (y + 1) * sl]
    dst_t = _dev(start)
    assert all(s.data_ptr() % 256 == 0 for s in srcs) and dst_t.data_ptr() % 256 == 0
    d = lib.ComposeDesc(src=srcs[0].data_ptr() + src_off, src2=srcs[1].data_ptr() + src_off if case.two else None, dst=dst_t.data_ptr() + front,
                        op=OPS[case.op], format=PF[case.cn], width=case.w, lines=h, src_pitch=sp, dst_pitch=dp, frames=frames, src_frame_stride=sstride,
                        dst_frame_stride=dstride, **case.fields)
    if case.op == "split":
        d.dst_pitch, d.tile_pitch = 0, dp
    if case.op == "logo":
        ov = _dev(case.overlay)
        d.src, d.logo = None, ov.data_ptr()
    rc = lib.load().ug_hip_compose(C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == expect, lib.last_error()
    return pl.compare_frames(dst_t.cpu().numpy(), want, frames, dstride, ol, dp, lb, front=front)


def _cases():
    out = []
    for cn, widths in WIDTHS.items():
        for w in widths:
            h = HEIGHT[w]
            blk = 48 if cn == "v210" else 2
            out.append(Case("crop", cn, w, h, crop=(0, 0, 0, 0)))                                   # offset 0, the whole frame
            out.append(Case("crop", cn, w, h, crop=(max(blk, w // 2), max(1, h // 2), w, h)))       # clamped at the right and bottom edge
            out.append(Case("crop", cn, w, h, crop=(max(blk, w // 3), 1, 3 if cn != "v210" else 20, h - 1)))  # an offset that rounds down to a block
            for hh in (2, 6):
                out.append(Case("interlace", cn, w, hh))
                out.append(Case("interlaced_3d", cn, w, hh))
            out.append(Case("interlace", cn, w, 5))
            for g in ((1, 1), (2, 1), (1, 2), (2, 3)):
                ww = w if w % g[0] == 0 else w + 1
                if cn == "v210" or ww % g[0] == 0:
                    out.append(Case("split", cn, ww, 6, grid=g))
            if cn in ("UYVY", "RGB", "RGBA"):
                for bw, bh, hh in ((2, 2, 5), (4, 2, 4), (w, 0, 3), (0, 1, 2), (1, 3, 6), (3, 0, 1)):
                    if bw <= w:
                        out.append(Case("border", cn, w, hh, bw=bw, bh=bh, colour=(0x12, 0xc4, 0xe6, 0x7f)))
    for cn, w in (("UYVY", 16), ("UYVY", 8), ("UYVY", 10)):  # line sizes 32, 16 and 20
        out += [Case("interlace", cn, w, 6), Case("interlaced_3d", cn, w, 6)]
    for cn, (w, h) in (("UYVY", (34, 5)), ("UYVY", (130, 6)), ("RGB", (43, 4)), ("RGBA", (33, 6)), ("RG48", (21, 5))):
        for lw, lh in ((1, 1), (3, 2), (4, 3), (7, 2), (8, 1)):
            for alpha in (None, 0, 255):
                out.append(Case("logo", cn, w, h, logo=(lw, lh, -1, -1), alpha=alpha))
        for x, y in ((8, 1), (w - 2, h), (6, 1), (13, 0)):  # interior, pushed back in, moved by the rounding by block bytes
            out.append(Case("logo", cn, w, h, logo=(4, 3, x, y)))
        out.append(Case("logo", cn, w, h, logo=(w, h, -1, -1)))  # as large as the frame
        out.append(Case("logo", cn, w, h, logo=(w - 1, h, 0, 0)))
    return out


CASES = _cases()
CIDS = [f"{c.op}-{c.cn}-{c.w}x{c.h}-" + "-".join(str(v).replace(" ", "") for k, v in sorted(c.prm.items()) if k != "colour") for c in CASES]


def _elem(case):
    return 2 if case.op == "logo" and case.cn == "RG48" else 1


@pytest.mark.parametrize("case", CASES, ids=CIDS)
def test_packed_one_and_three_frames_with_strides(case):
    assert run_layout(case) == []
    assert run_layout(case, frames=3, sgap=16 * 5, dgap=16 * 3) == []   # strides that keep every frame 16-byte aligned where the frame is
    assert run_layout(case, frames=3, sgap=3, dgap=2 * 3) == []          # ... and strides that do not


@pytest.mark.parametrize("layout", ["padded16", "odd_pitch", "src_off", "dst_off"])
@pytest.mark.parametrize("case", CASES, ids=CIDS)
def test_pitched_and_misaligned_buffers(case, layout):
    e = _elem(case)
    nat = case.tp if case.op == "split" else case.lb
    if layout == "odd_pitch":  # lines start at every residue: no dwordx4 tier
        sp, dp = case.ls + 1, nat + e
        sp += 1 if sp % 16 == 0 else 0
        dp += e if dp % 16 == 0 else 0
        so = do = 0
    else:
        sp, dp = (case.ls + 15) // 16 * 16 + 16, (nat + 15) // 16 * 16 + 32
        so, do = (1 if layout == "src_off" else 0), (e if layout == "dst_off" else 0)
    assert run_layout(case, frames=2, sp=sp, dp=dp, src_off=so, dst_off=do, sgap=16 * 2, dgap=16 * 4) == []


def test_split_tiles_at_a_stride_of_their_own():
    """tile_stride above tile_pitch * tile lines: the gaps between the tiles keep their fill"""
    rng = np.random.default_rng(3)
    w, h, gx, gy = 34, 6, 2, 3
    data = _rand(rs.linesize("UYVY", w) * h, rng)
    tiles = rs.split("UYVY", data, w, h, gx, gy, fill=pl.FILL)
    tp, th, ts = 48, h // gy, 48 * (h // gy) + 40
    dst = torch.full((ts * gx * gy,), pl.FILL, dtype=torch.uint8, device="cuda")
    src = _dev(data)
    d = lib.ComposeDesc(src=src.data_ptr(), dst=dst.data_ptr(), op=lib.CMP_SPLIT, format=lib.PF_UYVY, width=w, lines=h, frames=1, grid_x=gx, grid_y=gy,
                        tile_pitch=tp, tile_stride=ts)
    assert lib.load().ug_hip_compose(C.byref(d), torch.cuda.current_stream().cuda_stream) == lib.SUCCESS, lib.last_error()
    torch.cuda.synchronize()
    got = dst.cpu().numpy().reshape(gx * gy, ts)
    want = np.full((gx * gy, ts), pl.FILL, np.uint8)
    for t, tile in enumerate(tiles):
        want[t, : tp * th].reshape(th, tp)[:, :36] = tile.reshape(th, 36)
    assert int(np.count_nonzero(got != want)) == 0


def test_logo_outside_the_frame_leaves_it_or_is_refused():
    rng = np.random.default_rng(4)
    frame = _rand(rs.linesize("UYVY", 34) * 5, rng)
    ov = _dev(_rand(4 * 40 * 6, rng))
    t = _dev(frame)
    codec.compose(lib.CMP_LOGO, lib.PF_UYVY, t, 34, 5, logo=(ov, 4, 6, -1, -1))  # higher than the frame: rect_y < 0
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), frame)
    with pytest.raises(lib.UgHipError) as e:  # one pixel wider: the reference's rect_x = -1 / 4 * 4 = 0
        codec.compose(lib.CMP_LOGO, lib.PF_UYVY, t, 34, 5, logo=(ov, 35, 2, -1, -1))
    assert e.value.rc == lib.EINVAL
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), frame)


def test_codec_wrapper_crops_and_draws():
    rng = np.random.default_rng(6)
    data = _rand(rs.linesize("v210", 96) * 4, rng)
    out = codec.compose(lib.CMP_CROP, lib.PF_V210, _dev(data), 96, 4, crop=(48, 2, 50, 3))
    ow, oh, xb, yo = rs.crop_geometry("v210", 96, 4, 48, 2, 50, 3)
    assert (ow, oh, xb, yo) == codec.crop_geometry(lib.PF_V210, 96, 4, 48, 2, 50, 3)
    assert np.array_equal(out.cpu().numpy(), rs.crop("v210", data, 96, 4, oh, xb, yo, 128))
    rgb = _rand(3 * 43 * 6, rng)
    out = codec.compose(lib.CMP_BORDER, lib.PF_RGB, _dev(rgb), 43, 6, border=(10, 2, (1, 2, 3, 4)))
    assert np.array_equal(out.cpu().numpy(), rs.border("RGB", rgb, 43, 6, 10, 2, (1, 2, 3, 4)))


def test_default_descriptors_of_the_argument_rule_tests_succeed_on_real_buffers():
    """the control of tests/test_compose.py's refusals where a GPU is present: the descriptor those cases vary, with device buffers behind its
    pointers, is taken by every op (there the same check answers UG_HIP_ERUNTIME on a machine without a GPU, and is not run on one with)"""
    import test_compose as tc
    src, src2 = (torch.zeros(64 * 2 * 16, dtype=torch.uint8, device="cuda") for _ in range(2))
    dst = torch.zeros(64 * 2 * 16, dtype=torch.uint8, device="cuda")
    logo = torch.zeros(8 * 4 * 4, dtype=torch.uint8, device="cuda")
    for op in range(6):
        kw = dict(dst=dst.data_ptr(), logo=logo.data_ptr())
        if op != lib.CMP_LOGO:
            kw.update(src=src.data_ptr(), src2=src2.data_ptr())
        rc = lib.load().ug_hip_compose(C.byref(tc._desc(op=op, **kw)), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == lib.SUCCESS, (op, lib.last_error())
