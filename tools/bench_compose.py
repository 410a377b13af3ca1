#!/usr/bin/env python3
"""Kernel time of ug_hip_compose at 1920x1080 and 3840x2160 against a copy twin, and the reference's CPU modules on the same sizes.

  kernel   every op, 1 and 8 frames per launch; sources rotate over >= 600 MB so that no launch finds its input in a cache: us per frame and the
           fraction of 8 TB/s on algorithmic bytes (every source byte the op needs read once, every output byte written once).  The destination
           of a row is ONE buffer (the twin's too): it can stay in the last-level cache, so that fraction is no HBM write rate; the ratio is fair
  copy     in the same run, beside each kernel row: a plain device-to-device copy that reads and writes the same number of bytes -- (in + out) / 2
           bytes copied, so its traffic is the kernel's in + out -- and the ratio kernel / copy
  cpu      where oracle/_ref/ug_compose_harness exists: the reference's module of the same name on frames of that size, wall-clock ms inside
           vo_postprocess() / capture_filter()
Prints one JSON line per measurement.  python tools/bench_compose.py [--iters N] [--only LABEL:WIDTH:FRAMES] [--no-cpu]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ultragrid_amd import codec, lib as L  # noqa: E402

PEAK = 8.0e12
ROTATE_BYTES = 600e6
SIZES = [(1920, 1080), (3840, 2160)]
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ug_compose_harness")
LOGO = (256, 128)
# (label, op, format, the reference's module, its options, codec name, cf | pp, tiles per input frame)
ROWS = [
    ("crop-UYVY", L.CMP_CROP, L.PF_UYVY, "crop", "size={w2}x{h2}:xoff=100:yoff=50", "UYVY", "pp", 1),
    ("border-UYVY", L.CMP_BORDER, L.PF_UYVY, "border", "width=10:height=10", "UYVY", "pp", 1),
    ("border-RGB", L.CMP_BORDER, L.PF_RGB, "border", "width=10:height=10", "RGB", "pp", 1),
    ("interlace-UYVY", L.CMP_INTERLACE, L.PF_UYVY, "interlace", "-", "UYVY", "pp", 1),
    ("interlace-v210", L.CMP_INTERLACE, L.PF_V210, "interlace", "-", "v210", "pp", 1),
    ("interlaced_3d-UYVY", L.CMP_INTERLACED_3D, L.PF_UYVY, "interlaced_3d", "-", "UYVY", "pp", 2),
    ("split-UYVY", L.CMP_SPLIT, L.PF_UYVY, "split", "2:2", "UYVY", "pp", 1),
    ("logo-UYVY", L.CMP_LOGO, L.PF_UYVY, "logo", None, "UYVY", "cf", 1),
    ("logo-RGBA", L.CMP_LOGO, L.PF_RGBA, "logo", None, "RGBA", "cf", 1),
]


def time_ms(fn, iters):
    for i in range(3):
        fn(i)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def kernel_row(lib, stream, row, w, h, frames, iters):
    label, op, fmt = row[:3]
    ls = lib.ug_hip_linesize(fmt, w)
    ib = ls * h
    d0 = dict(op=op, format=fmt, width=w, lines=h, frames=frames, src_frame_stride=ib)
    two = op in (L.CMP_INTERLACE, L.CMP_INTERLACED_3D)
    read, ob = ib, ib  # bytes the op needs per frame, bytes it writes
    if op == L.CMP_CROP:
        ow, oh, xb, yo = codec.crop_geometry(fmt, w, h, w // 2, h // 2, 100, 50)
        lb = lib.ug_hip_linesize(fmt, ow)
        d0.update(xoff_bytes=xb, yoff=yo, out_line_bytes=lb, out_lines=oh)
        read = ob = lb * oh
    elif op == L.CMP_BORDER:
        d0.update(border_w=10, border_h=10, fill=(C.c_ubyte * 4)(*codec.border_pattern(fmt, (0xff, 0xff, 0, 0xff))))
    elif op == L.CMP_INTERLACED_3D:
        read = 2 * ib
    elif op == L.CMP_SPLIT:
        d0.update(grid_x=2, grid_y=2)
    elif op == L.CMP_LOGO:
        bpp = ls // w
        read = ob = LOGO[0] * LOGO[1] * bpp
        overlay = torch.randint(0, 256, (LOGO[0] * LOGO[1] * 4,), dtype=torch.uint8, device="cuda")
        rx, ry = codec.logo_geometry(fmt, w, h, LOGO[0], LOGO[1])
        d0.update(logo=overlay.data_ptr(), logo_w=LOGO[0], logo_h=LOGO[1], rect_x=rx, rect_y=ry, dst_frame_stride=ib)
        read += LOGO[0] * LOGO[1] * 4
    sets = max(2, int(-(-ROTATE_BYTES // (ib * frames * (2 if two else 1)))))
    src = torch.randint(0, 256, (sets, ib * frames), dtype=torch.uint8, device="cuda")
    src2 = torch.randint(0, 256, (sets, ib * frames), dtype=torch.uint8, device="cuda") if two else None
    dst = None if op == L.CMP_LOGO else torch.empty(ib * frames, dtype=torch.uint8, device="cuda")
    descs = []
    for i in range(sets):
        d = L.ComposeDesc(**d0)
        if op == L.CMP_LOGO:
            d.dst = src[i].data_ptr()
        else:
            d.src, d.dst, d.dst_frame_stride = src[i].data_ptr(), dst.data_ptr(), ob if op != L.CMP_SPLIT else ib
            if two:
                d.src2 = src2[i].data_ptr()
        descs.append(d)

    def k(i):
        L.check(lib.ug_hip_compose(C.byref(descs[i % sets]), stream), "ug_hip_compose")
    half = max(16, (read + ob) // 2 * frames)
    csets = max(2, min(4096, int(-(-ROTATE_BYTES // half))))
    csrc = torch.randint(0, 256, (csets, half), dtype=torch.uint8, device="cuda")
    cdst = torch.empty(half, dtype=torch.uint8, device="cuda")

    def twin(i):
        cdst.copy_(csrc[i % csets])
    ms, cms = time_ms(k, iters) / frames, time_ms(twin, iters) / frames
    return {"what": "kernel", "row": label, "size": f"{w}x{h}", "frames": frames, "us_per_frame": round(ms * 1e3, 2), "copy_us_per_frame": round(cms * 1e3, 2),
            "ratio_to_copy": round(ms / cms, 2), "read_MB": round(read / 1e6, 3), "written_MB": round(ob / 1e6, 3), "frac_8TBps": round((read + ob) / (ms * 1e-3) / PEAK, 4)}


def cpu_row(lib, row, w, h, reps):
    label, _, fmt, name, options, cn, mode, tiles = row
    n = lib.ug_hip_linesize(fmt, w) * h * tiles
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "in.raw")
        torch.randint(16, 236, (n,), dtype=torch.uint8).numpy().tofile(path)
        if name == "logo":
            pam = os.path.join(tmp, "logo.pam")
            with open(pam, "wb") as f:
                f.write(f"P7\nWIDTH {LOGO[0]}\nHEIGHT {LOGO[1]}\nDEPTH 4\nMAXVAL 255\nTUPLTYPE RGB_ALPHA\nENDHDR\n".encode())
                f.write(torch.randint(0, 256, (LOGO[0] * LOGO[1] * 4,), dtype=torch.uint8).numpy().tobytes())
            options = pam
        options = options.format(w2=w // 2, h2=h // 2)
        args = [HARNESS, "run", name, options, cn, mode, str(tiles), os.path.join(tmp, "out")] + [str(w), str(h), path] * (2 * reps)
        r = subprocess.run(args, capture_output=True, text=True, timeout=600)
    ms = [ln.split("ms_per_frame=")[1] for ln in r.stdout.splitlines() if "ms_per_frame=" in ln]
    return {"what": "cpu", "row": label, "size": f"{w}x{h}", "module": name, "ms_per_input_frame": float(ms[0]) if ms else None, "rc": r.returncode}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_compose.py needs a GPU")
    lib = L.load()
    stream = torch.cuda.current_stream().cuda_stream
    only = args.only.split(":") if args.only else None
    for row in ROWS:
        for w, h in SIZES:
            for frames in (1, 8):
                if only and [row[0], str(w), str(frames)] != only:
                    continue
                print(json.dumps(kernel_row(lib, stream, row, w, h, frames, args.iters)), flush=True)
                torch.cuda.empty_cache()
    if only or args.no_cpu or not os.path.exists(HARNESS):
        return
    for row in ROWS:
        for w, h in SIZES:
            print(json.dumps(cpu_row(lib, row, w, h, args.cpu_reps)), flush=True)


if __name__ == "__main__":
    main()
