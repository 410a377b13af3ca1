#!/usr/bin/env python3
"""Writes tests/golden/compose_ref.npz: the reference's geometric / compositing filters (crop, border, interlace, interlaced_3d, split, logo, compiled
unmodified into oracle/_ref/ug_compose_harness) run on the CPU over the cases below.  Data only: per case the option string, codec, sizes, the input
bytes (and logo), what came back per frame (true / false / new / same, the returned description) and the output bytes.

Two kinds of case (tests/compose_restatement.py; include/ug_mi355x.h "Deviations"):
  inside     geometries where the reference stays in its buffers.  Asserted HERE, per frame: the restatement equals the reference's bytes with 0
             differing and nothing left out, the returned description is the restated one, and no byte behind a buffer the harness handed out
             changed (its `pad` count).  A failure means the table of slips is wrong, not the cap.
  deviating  the rest: the reference is not run (logo: its blend leaves the malloc'ed segment; border: negative memcpy lengths), or run only to record
             that it left its buffer or faulted (`ref_pad` > 0, `ref_fault`: interlaced_3d at a line size that is no multiple of 16 hands pavgb a
             misaligned memory operand).  The fixture stores the restatement's bytes.
    python3 tests/golden/make_compose_golden.py
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import compose_restatement as rs  # noqa: E402

HARNESS = os.path.join(ROOT, "oracle", "_ref", "ug_compose_harness")
OUT = os.path.join(HERE, "compose_ref.npz")
FRAME = {"UYVY": (34, 5), "RGB": (43, 3), "RGBA": (33, 4), "RG48": (21, 5)}
LOGOS = [(1, 1), (3, 2), (4, 3), (7, 2), (8, 1)]


def case(name, options, codec, frames, mode="pp", tiles=1, kind="inside", run_ref=None, logo=None):
    """frames: [(w, h)] pushed through one state; logo: (lw, lh, alpha kind, channels)"""
    return dict(name=name, options=options, codec=codec, frames=[list(f) for f in frames], mode=mode, tiles=tiles, kind=kind,
                run_ref=(kind == "inside") if run_ref is None else run_ref, logo=logo)


def cases():
    out = []
    # ---- crop: offset 0, an offset clamped at the right and bottom edge, one that rounds down to a block; both registrations; a size change ----
    for codec, (w, h) in list(FRAME.items()) + [("v210", (96, 3))]:
        cw = 48 if codec == "v210" else 10
        out.append(case("crop", f"size={cw}x2", codec, [(w, h)]))
        out.append(case("crop", f"size={cw}x2:xoff={w - 3}:yoff={h - 1}", codec, [(w, h)]))
        out.append(case("crop", f"width={cw - 1}:height=1:xoff=7:yoff=1", codec, [(w, h)], mode="cf"))
    out.append(case("crop", "size=9x3:xoff=3", "UYVY", [(34, 5), (130, 4), (6, 2)]))
    out.append(case("crop", "size=6x2:xoff=60", "v210", [(96, 3)], kind="deviating"))  # linesize(6) = 128 bytes from byte 160 of a 256-byte line
    # ---- border: 2x2, 4x2, 2 * border_h == H, border_w == W, the colour parser, what does not fit, a codec it refuses ----
    for codec, (w, h) in (("UYVY", (34, 5)), ("RGB", (43, 6)), ("RGBA", (33, 4))):
        out.append(case("border", "width=2:height=2", codec, [(w, h)]))
        out.append(case("border", "width=4:height=2:color=#12c4e6", codec, [(w, h)]))
        out.append(case("border", "width=3:height=1:color=80ff40", codec, [(w, 4), (6, 4)]))  # rounded up to 4 x 2: 2 * border_h == H, then border_w < W = 6
    out.append(case("border", "width=6:height=2", "UYVY", [(6, 5)]))   # border_w == W
    out.append(case("border", "width=6:height=0", "RGBA", [(6, 3)]))
    out.append(case("border", "width=5:height=2", "RGB", [(6, 4)]))    # 6 x 2
    out.append(case("border", "-", "UYVY", [(34, 5)], kind="deviating"))  # 10 x 10 on 5 lines: memcpy of a negative length
    out.append(case("border", "width=8:height=2", "RGB", [(6, 4)], kind="deviating"))  # border_w > W: writes in front of the line
    out.append(case("border", "width=2:height=2", "v210", [(48, 4)]))   # refused codec
    # ---- interlace: 2 and 6 lines, line sizes 16, 32, 20; the false / true sequence ----
    for codec, w in (("UYVY", 8), ("UYVY", 16), ("UYVY", 10), ("RGB", 43), ("RGBA", 33), ("RG48", 21), ("v210", 48)):
        out.append(case("interlace", "-", codec, [(w, 2)] * 2))
        out.append(case("interlace", "-", codec, [(w, 6)] * 4 + [(w, 5)] * 3))  # two pairs, a size change, a pair and a half
    # ---- interlaced_3d: line sizes that are multiples of 16 and even heights are the reference; the rest shears or overruns there ----
    for codec, w in (("UYVY", 8), ("UYVY", 16), ("RGBA", 4), ("RG48", 8), ("v210", 48), ("v210", 96)):
        out.append(case("interlaced_3d", "-", codec, [(w, 2), (w, 6)], tiles=2))
    for codec, w in (("UYVY", 10), ("RGB", 43), ("RGBA", 33), ("RG48", 21)):
        out.append(case("interlaced_3d", "-", codec, [(w, 2)], tiles=2, kind="deviating", run_ref=True))
        out.append(case("interlaced_3d", "-", codec, [(w, 6)], tiles=2, kind="deviating", run_ref=True))
    # ---- split ----
    for codec, w in (("UYVY", 34), ("RGB", 6), ("RGBA", 6), ("RG48", 6), ("v210", 96)):
        for grid in ("1:1", "2:1", "1:2", "2:3"):
            out.append(case("split", grid, codec, [(w, 6)]))
    out.append(case("split", "2:1", "UYVY", [(34, 6), (12, 2)]))
    # ---- logo ----
    for codec, (w, h) in FRAME.items():
        for lw, lh in LOGOS + ([(5, 2), (6, 2), (11, 1)] if codec == "RG48" else []):
            kind = "inside" if rs.logo_inside(codec, lw) else "deviating"
            for alpha in ("random", "0", "255"):
                out.append(case("logo", "", codec, [(w, h)], mode="cf", kind=kind, logo=(lw, lh, alpha, 4)))
        lw, lh = {"UYVY": (4, 3), "RGB": (3, 2), "RGBA": (4, 3), "RG48": (6, 2)}[codec]
        for pos in ("8:1", f"{w - 2}:{h}", "6:1", "7", f"{w - lw}:{h - lh}"):  # interior, pushed back in, moved by the rounding, x only, the far corner
            out.append(case("logo", pos, codec, [(w, h)], mode="cf", logo=(lw, lh, "random", 4)))
        out.append(case("logo", "", codec, [(w, h), (w, h)], mode="cf", logo=(lw, lh, "random", 3)))  # three channels in the file; two frames, one state
        out.append(case("logo", "", codec, [(lw, lh)], mode="cf", logo=(lw, lh, "random", 4)))         # as large as the frame
        out.append(case("logo", "", codec, [(lw - 1, lh)], mode="cf", logo=(lw, lh, "random", 4)))     # wider than the frame: rect_x = -1 rounds to 0 in the reference; refused here
        out[-1].update(kind="deviating", run_ref=False)
        out.append(case("logo", "", codec, [(w, lh - 1)], mode="cf", logo=(lw, lh, "random", 4)))      # higher than the frame: left as it is
    out.append(case("logo", "", "v210", [(48, 2)], mode="cf", logo=(4, 2, "random", 4)))                # no decoder to RGB and back: the frame as it is
    return out


def make_logo(lw, lh, alpha, channels, rng):
    """-> (the R,G,B,A overlay as logo.c:92-96 holds it, the bytes of the .pam file)"""
    px = np.frombuffer(rng.bytes(lw * lh * 4), np.uint8).copy().reshape(-1, 4)
    if alpha != "random":
        px[:, 3] = int(alpha)
    if channels == 3:
        px[:, 3] = 255  # vc_copylineRGBtoRGBA with shifts 0, 8, 16
    return px.reshape(-1), make_pam(px.reshape(-1), lw, lh, channels)


def make_pam(overlay, lw, lh, channels):
    """the .pam file of an R,G,B,A overlay: all four channels, or its first three"""
    tupl = "RGB_ALPHA" if channels == 4 else "RGB"
    head = f"P7\nWIDTH {lw}\nHEIGHT {lh}\nDEPTH {channels}\nMAXVAL 255\nTUPLTYPE {tupl}\nENDHDR\n".encode()
    return head + np.asarray(overlay, np.uint8).reshape(-1, 4)[:, :channels].tobytes()


def run_harness(harness, names, options, codec, mode, tiles, frames, tmp, env_extra=None, timeout=120):
    """frames: [(w, h, bytes of all tiles)] -> ({name: [dict(ret, w, h, codec, interlacing, fps, tile_count, data_len, mode, pad, out)]}, rc, log)"""
    args = [harness, "run", names, options or "-", codec, mode, str(tiles), os.path.join(tmp, "out")]
    for i, (w, h, data) in enumerate(frames):
        path = os.path.join(tmp, f"in{i}.raw")
        np.asarray(data, np.uint8).tofile(path)
        args += [str(w), str(h), path]
    p = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, **(env_extra or {})), timeout=timeout)
    res = {}
    for line in p.stdout.splitlines():
        t = line.split()
        if len(t) == 13 and t[1] == "frame":
            r = dict(ret=t[11][4:], w=int(t[3]), h=int(t[4]), codec=t[5], interlacing=int(t[6]), fps=float(t[7]), tile_count=int(t[8]), data_len=int(t[9]),
                     mode=int(t[10]), pad=int(t[12][4:]))
            if r["ret"] in ("new", "same", "true"):
                r["out"] = np.fromfile(os.path.join(tmp, f"out.{t[0]}.{t[2]}"), np.uint8)
            res.setdefault(t[0], []).append(r)
    return res, p.returncode, p.stdout + p.stderr


def options_of(c, tmp, pam):
    """the option string the module gets: logo's starts with the file"""
    if c["name"] != "logo":
        return c["options"]
    path = os.path.join(tmp, "logo.pam")
    with open(path, "wb") as f:
        f.write(pam)
    return path + (":" + c["options"] if c["options"] else "")


def restate(c, inputs, overlay):
    """the case through tests/compose_restatement.py -> per frame its dict, or None where ug_hip_compose refuses the geometry"""
    m = rs.Module(c["name"], ("x:" + c["options"]).rstrip(":") if c["name"] == "logo" else c["options"], c["codec"], overlay)
    out = []
    for (w, h), data in zip(c["frames"], inputs):
        n = rs.linesize(c["codec"], w) * h
        try:
            out.append(m.frame(w, h, [data[t * n: (t + 1) * n] for t in range(c["tiles"])]))
            if c["mode"] == "cf" and out[-1]["ret"] == "true":
                out[-1]["ret"] = "new"  # a capture filter answers with a frame of its own
        except AssertionError:
            out.append(None)
    return out


def main():
    if not os.path.exists(HARNESS):
        raise SystemExit(f"{HARNESS} not built")
    rng = np.random.default_rng(20261019)
    meta, arrays = [], {}
    counts = dict(inside=0, deviating=0)
    for k, c in enumerate(cases()):
        inputs = []
        for w, h in c["frames"]:
            key = f"in_{c['codec']}_{w}x{h}x{c['tiles']}"
            if key not in arrays:
                arrays[key] = np.frombuffer(rng.bytes(rs.linesize(c["codec"], w) * h * c["tiles"]), np.uint8).copy()
            inputs.append(arrays[key])
        overlay, pam = None, None
        if c["logo"]:
            lw, lh, alpha, ch = c["logo"]
            ov, pam = make_logo(lw, lh, alpha, ch, rng)
            arrays[f"logo_{k}"] = ov
            overlay = (ov, lw, lh)
        supported = c["codec"] != "v210" or c["name"] not in ("border", "logo")
        want = restate(c, inputs, overlay) if supported else [None] * len(c["frames"])
        ref = None
        if c["run_ref"]:
            with tempfile.TemporaryDirectory() as tmp:
                res, rc, log = run_harness(HARNESS, c["name"], options_of(c, tmp, pam), c["codec"], c["mode"], c["tiles"],
                                           [(w, h, d) for (w, h), d in zip(c["frames"], inputs)], tmp)
            if c["kind"] == "deviating" and rc == -11:
                c = dict(c, ref_fault=True)  # the reference itself faults here (interlaced_3d: pavgb's memory operand must be 16-byte aligned)
            elif rc != 0 or len(res.get(c["name"], [])) != len(c["frames"]):
                raise SystemExit(f"case {k} {c}: harness rc={rc}\n{log}")
            else:
                ref = res[c["name"]]
        frames_meta = []
        for i, wf in enumerate(want):
            fm = dict(refused=wf is None)
            if wf is not None:
                fm.update(ret=wf["ret"], w=wf["w"], h=wf["h"], tile_count=wf["tile_count"], interlacing=wf["interlacing"], fps=wf["fps"])
                if "out" in wf:
                    arrays[f"out_{k}_{i}"] = wf["out"]
            if ref is not None:
                r = ref[i]
                fm.update(ref_ret=r["ret"], ref_pad=r["pad"], ref_desc=[r["w"], r["h"], r["codec"], r["interlacing"], r["fps"], r["tile_count"], r["data_len"]])
                if c["kind"] == "inside" and supported:
                    assert wf is not None, (k, c, i)
                    assert r["ret"] == wf["ret"], (k, c, i, r["ret"], wf["ret"])
                    assert (r["w"], r["h"], r["tile_count"], r["interlacing"], r["fps"], r["codec"]) == \
                        (wf["w"], wf["h"], wf["tile_count"], wf["interlacing"], wf["fps"], c["codec"]), (k, c, i, r, wf)
                    assert r["pad"] in (0, -1), f"case {k} {c} frame {i}: the reference changed {r['pad']} bytes behind its buffer: not an inside case"
                    if "out" in wf:
                        got = r["out"]
                        if c["name"] == "crop":  # the module's frame is lines of vc_get_linesize(out width); crop writes line_bytes of each
                            got = got.reshape(wf["h"], -1)[:, : wf["line_bytes"]].reshape(-1)
                        assert got.size == wf["out"].size, (k, c, i, got.size, wf["out"].size)
                        bad = int(np.count_nonzero(got != wf["out"]))
                        assert bad == 0, f"case {k} {c} frame {i}: {bad} bytes differ from the reference: not an inside case, or the restatement is wrong"
                elif not supported:
                    fm.update(ret=r["ret"])
                    if "out" in r:
                        assert np.array_equal(r["out"], inputs[i]), (k, c)  # a refused codec: the frame as it came
            frames_meta.append(fm)
        counts[c["kind"]] += 1
        print(f"case {k:3d} {c['kind']:9s} {c['name']:13s} {c['options'][:28]:28s} {c['codec']:5s} {c['frames']} logo={c['logo']} "
              f"ref={'-' if ref is None else [(r['ret'], r['pad']) for r in ref]}")
        meta.append(dict(c, frames_meta=frames_meta))
    # the boundary of the 3d slip: every deviating interlaced_3d run faulted or left the output buffer
    for m in meta:
        if m["name"] == "interlaced_3d" and m["kind"] == "deviating":
            assert m.get("ref_fault") or all(f["ref_pad"] > 0 for f in m["frames_meta"]), m
    np.savez_compressed(OUT, meta=np.array(json.dumps(meta)), **arrays)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(meta)} cases ({counts})")


if __name__ == "__main__":
    main()
