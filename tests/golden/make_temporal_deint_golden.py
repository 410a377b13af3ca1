#!/usr/bin/env python3
"""Writes tests/golden/temporal_deint_ref.npz: the reference's OWN de-interlacing postprocessors executed on the CPU.

src/vo_postprocess/deinterlace.c and temporal-deint.c are compiled unmodified (ultragrid_amd/module/Makefile: oracle/_ref/ug_deint_harness,
the reference's files where they lie) and driven through the reference's src/vo_postprocess.c: per case three consecutive frames, for each
postprocess(in) and postprocess(NULL), into output frames pre-filled with 0xA5.  The fixture holds the input frames and the output frames only
(recorded results, no program text).  Needs the reference tree; no GPU (only the reference's module names are run).

    python3 tests/golden/make_temporal_deint_golden.py [out.npz]

Prints the share of bytes that tests/test_deinterlace_ex.py leaves out when it compares the restatement with these results (the conditions
of DESIGN.md 4.11: the first output after a reconfigure of double_framerate -- its odd lines, with `:d` all of it --, and pitch gaps)."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deinterlace_restatement as rs  # noqa: E402

HARNESS = os.path.join(ROOT, "oracle", "_ref", "ug_deint_harness")
# codec -> (bytes per block, pixels per block, width alignment): vc_get_linesize (video_codec.c:120-206, :507-521)
BLOCK = {"RGBA": (4, 1, 1), "UYVY": (4, 2, 2), "YUYV": (4, 2, 2), "RGB": (3, 1, 1), "BGR": (3, 1, 1), "VUYA": (4, 1, 1), "RG48": (6, 1, 1),
         "Y216": (8, 2, 2), "Y416": (8, 1, 1), "v210": (16, 6, 48), "R10k": (4, 1, 64), "R12L": (36, 8, 8), "DVS10": (16, 6, 48)}
TEMPORAL = ("double_framerate", "deinterlace_bob", "deinterlace_linear")


def linesize(codec: str, w: int) -> int:
    bb, bp, ha = BLOCK[codec]
    w = (w + ha - 1) // ha * ha
    return (w + bp - 1) // bp * bb


def case_list():
    """(id, name, options, codec, interlacing, extra pitch, [(w, h)] * 3)"""
    cases = []
    widths = {"RGBA": 5, "UYVY": 8, "YUYV": 10, "RGB": 7, "BGR": 11, "VUYA": 25, "RG48": 3, "Y216": 6, "Y416": 12, "v210": 48, "R10k": 64, "R12L": 16}
    heights = [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13]
    for i, (codec, w) in enumerate(widths.items()):
        h, he = heights[i % 12], heights[(i * 5 + 2) % 12] // 2 * 2
        if codec == "R10k":
            h, he = 5, 2
        extra = 16 if codec == "R12L" else 0  # (not R10k: avg_lines walks four lines' worth -- with a gap it would land there)
        cases.append((f"blend_{codec}", "deinterlace" if i % 2 else "deinterlace_blend", "-", codec, "merged", 0, [(w, max(h, 2))] * 3))
        cases.append((f"df_{codec}", "double_framerate", "-", codec, "merged", extra, [(w, he)] * 3))
        cases.append((f"bob_{codec}", "deinterlace_bob", "-", codec, "merged", extra, [(w, h)] * 3))
        cases.append((f"linear_{codec}", "deinterlace_linear", "-", codec, "merged", extra, [(w, 6 if codec == "R10k" else 13 - i % 12)] * 3))
    for codec in ("UYVY", "RG48", "v210", "R10k", "R12L"):
        cases.append((f"dfd_{codec}", "double_framerate", "d", codec, "merged", 0, [(widths[codec], 2 if codec in ("v210", "R10k") else 8)] * 3))
    for name in ("deinterlace", "deinterlace_blend") + TEMPORAL:
        cases.append((f"force_{name}", name, "force", "UYVY", "prog", 0, [(16, 6)] * 3))
        cases.append((f"prog_{name}", name, "-", "UYVY", "prog", 0, [(16, 6)] * 3))
        cases.append((f"reconf_{name}", name, "-", "R12L", "merged", 0, [(16, 6), (16, 6), (24, 10)]))
        cases.append((f"unsupp_{name}", name, "-", "DVS10", "merged", 0, [(48, 5 if name != "double_framerate" else 4)] * 3))
    for name in TEMPORAL:
        cases.append((f"nodelay_{name}", name, "nodelay", "RGB", "merged", 16 if name == "deinterlace_linear" else 0, [(40, 8)] * 3))
    cases.append(("unsupp_dfd", "double_framerate", "d", "DVS10", "merged", 0, [(48, 4)] * 3))
    cases.append(("linear_wide", "deinterlace_linear", "-", "UYVY", "merged", 0, [(200, 4)] * 3))  # 400-byte lines
    return cases


def excluded(name, opts, active, case_frames, i, k):
    """the lines of output k of frame i that a comparison with the reference leaves out: the first postprocess(in) frame after a reconfigure of
    double_framerate holds the lines of a buffer the reference never initialised -- its odd lines, and through the blend of `:d` every line"""
    if name != "double_framerate" or not active or k != 0 or (i > 0 and case_frames[i] == case_frames[i - 1]):
        return None
    return slice(None) if opts == "d" else slice(1, None, 2)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "temporal_deint_ref.npz")
    if not os.path.exists(HARNESS):
        raise SystemExit(f"{HARNESS} not built: python -c 'import __graft_entry__ as g; g.build()' (needs the reference tree)")
    rng = np.random.default_rng(12)
    data, meta = {}, []
    total = left_out = gaps = 0
    with tempfile.TemporaryDirectory() as tmp:
        for cid, name, opts, codec, inter, extra, sizes in case_list():
            args, ins = [], []
            for i, (w, h) in enumerate(sizes):
                frame = rng.integers(0, 256, linesize(codec, w) * h, dtype=np.uint8)
                path = os.path.join(tmp, f"{cid}.{i}.in")
                frame.tofile(path)
                ins.append(frame)
                args += [str(w), str(h), path]
            prefix = os.path.join(tmp, cid)
            r = subprocess.run([HARNESS, "run", name, opts, codec, inter, str(extra), prefix, "1"] + args, capture_output=True, text=True)
            if r.returncode != 0:
                raise SystemExit(f"{cid}: harness rc={r.returncode}\n{r.stdout}\n{r.stderr}")
            rets = [ln.split("ret=")[1] for ln in r.stdout.splitlines() if " frame " in ln]
            descs = [ln.split()[3:10] for ln in r.stdout.splitlines() if " frame " in ln]
            data["in_" + cid] = np.concatenate(ins)
            active = inter == "merged" or opts == "force"
            outs = []
            for i, (w, h) in enumerate(sizes):
                L = linesize(codec, w)
                for k in range(2):
                    path = f"{prefix}.{name}.{i}.{k}"
                    if os.path.exists(path):
                        outs.append(np.fromfile(path, np.uint8))  # (rets says which exist: in the order frame, output)
                        total += (L + extra) * h
                        gaps += extra * h
                        ex = excluded(name, opts, active, sizes, i, k)
                        if ex is not None:
                            left_out += len(range(h)[ex]) * L
            data["out_" + cid] = np.concatenate(outs)
            meta.append(dict(id=cid, name=name, opts=opts, codec=codec, inter=inter, extra=extra, sizes=sizes, rets=rets, descs=descs))
    data["cases"] = np.array(json.dumps(meta))
    np.savez_compressed(out_path, **data)
    blend_total = sum(1 for m in meta if m["name"].startswith("deinterlace") and m["name"] in ("deinterlace", "deinterlace_blend"))
    print(f"{out_path}: {len(meta)} cases ({blend_total} of vc_deinterlace_ex: nothing left out), {os.path.getsize(out_path)} bytes")
    print(f"bytes of the module-level outputs: {total}; left out: uninitialised first-output lines {left_out} ({100 * left_out / total:.2f} %), "
          f"pitch gaps {gaps} ({100 * gaps / total:.2f} %); together {100 * (left_out + gaps) / total:.2f} %")
    assert left_out + gaps < 0.05 * total, "more than 5 % of the bytes would be left out: change the case list"
    _ = rs


if __name__ == "__main__":
    main()
