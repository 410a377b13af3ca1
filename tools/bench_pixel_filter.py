#!/usr/bin/env python3
"""Kernel time of ug_hip_pixel_filter at 3840x2160 against a copy twin, and the reference's CPU modules on the same size.

  kernel   every op x format, 1 and 8 frames per launch; sources rotate over >= 600 MB so that no launch finds its input in a cache: us per
           frame and the fraction of 8 TB/s on algorithmic bytes (every source byte read once, every output byte written once)
  copy     in the same run, beside each kernel row: a plain device-to-device copy that reads and writes the same number of bytes -- (in + out) / 2
           bytes copied, so its traffic is the kernel's in + out -- and the ratio kernel / copy
  cpu      where oracle/_ref/ug_cfilter_harness exists: the reference's module of the same name on one frame of that size, wall-clock ms inside
           capture_filter() (`--cpu-reps` calls; the harness prints the CPU count, which is the number of threads of the reference's gamma)
Prints one JSON line per measurement.  python tools/bench_pixel_filter.py [--iters N] [--only LABEL:FRAMES] [--no-cpu]
(--only: one kernel row, for a counter pass: rocprofv3 --pmc TCC_EA0_RDREQ_sum WRITE_SIZE -- python tools/bench_pixel_filter.py --only matrix-RGB:8)
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
W, H = 3840, 2160
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ug_cfilter_harness")
M = [1.31, -0.62, 0.18, -1.94, 0.77, 1.05, 0.4, 1.66, -1.23]
MS = ":".join(str(x) for x in M)
# (label, op, format, out format, clamp, (lut in bits, out bits) or None, the reference's module, its options, its codec)
ROWS = [
    ("matrix-UYVY", L.PXF_MATRIX, L.PF_UYVY, L.PF_RGB, 1, None, "matrix", MS, "UYVY"),
    ("matrix-RGB", L.PXF_MATRIX, L.PF_RGB, L.PF_RGB, 1, None, "matrix", MS, "RGB"),
    ("matrix-RGB-unchecked", L.PXF_MATRIX, L.PF_RGB, L.PF_RGB, 0, None, "matrix", MS + ":no-bound-check", "RGB"),
    ("matrix-RG48", L.PXF_MATRIX, L.PF_RG48, L.PF_RG48, 1, None, "matrix", MS, "RG48"),
    ("matrix2-UYVY", L.PXF_MATRIX2, L.PF_UYVY, L.PF_UYVY, 0, None, "matrix2", "y601_to_y709", "UYVY"),
    ("matrix2-Y416", L.PXF_MATRIX2, L.PF_Y416, L.PF_Y416, 0, None, "matrix2", "y601_to_y709", "Y416"),
    ("matrix2-v210", L.PXF_MATRIX2, L.PF_V210, L.PF_V210, 0, None, "matrix2", "y601_to_y709", "v210"),
    ("gamma-8-8", L.PXF_LUT, L.PF_RGB, L.PF_RGB, 0, (8, 8), "gamma", "2.2", "RGB"),
    ("gamma-8-16", L.PXF_LUT, L.PF_RGB, L.PF_RG48, 0, (8, 16), "gamma", "2.2:16", "RGB"),
    ("gamma-16-16", L.PXF_LUT, L.PF_RG48, L.PF_RG48, 0, (16, 16), "gamma", "2.2", "RG48"),
    ("gamma-16-8", L.PXF_LUT, L.PF_RG48, L.PF_RGB, 0, (16, 8), "gamma", "2.2:8", "RG48"),
    ("grayscale-UYVY", L.PXF_GRAY, L.PF_UYVY, L.PF_UYVY, 0, None, "grayscale", "-", "UYVY"),
    ("mirror-UYVY", L.PXF_MIRROR, L.PF_UYVY, L.PF_UYVY, 0, None, "mirror", "-", "UYVY"),
    ("flip-UYVY", L.PXF_FLIP, L.PF_UYVY, L.PF_UYVY, 0, None, "flip", "-", "UYVY"),
    ("flip-v210", L.PXF_FLIP, L.PF_V210, L.PF_V210, 0, None, "flip", "-", "v210"),
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


def kernel_row(lib, stream, row, frames, iters):
    label, op, fmt, ofmt, clamp, lut_bits, *_ = row
    ib, ob = lib.ug_hip_linesize(fmt, W) * H, lib.ug_hip_linesize(ofmt, W) * H
    sets = max(2, int(-(-ROTATE_BYTES // (ib * frames))))
    src = torch.randint(0, 256, (sets, ib * frames), dtype=torch.uint8, device="cuda")
    dst = torch.empty(ob * frames, dtype=torch.uint8, device="cuda")
    lut = codec.gamma_lut(2.2, *lut_bits).cuda() if lut_bits else None
    descs = [L.PixelFilterDesc(src[i].data_ptr(), dst.data_ptr(), op, fmt, ofmt, W, H, 0, 0, frames, ib, ob, (C.c_double * 9)(*M), clamp,
                               lut.data_ptr() if lut is not None else None) for i in range(sets)]

    def k(i):
        L.check(lib.ug_hip_pixel_filter(C.byref(descs[i % sets]), stream), "ug_hip_pixel_filter")
    half = (ib + ob) // 2 * frames
    csets = max(2, int(-(-ROTATE_BYTES // half)))
    csrc = torch.randint(0, 256, (csets, half), dtype=torch.uint8, device="cuda")
    cdst = torch.empty(half, dtype=torch.uint8, device="cuda")

    def twin(i):
        cdst.copy_(csrc[i % csets])
    ms, cms = time_ms(k, iters) / frames, time_ms(twin, iters) / frames
    return {"what": "kernel", "row": label, "frames": frames, "us_per_frame": round(ms * 1e3, 2), "copy_us_per_frame": round(cms * 1e3, 2),
            "ratio_to_copy": round(ms / cms, 2), "read_MB": round(ib / 1e6, 2), "written_MB": round(ob / 1e6, 2), "frac_8TBps": round((ib + ob) / (ms * 1e-3) / PEAK, 3)}


def cpu_row(lib, row, reps):
    label, _, fmt, *_rest, name, options, cn = row
    n = lib.ug_hip_linesize(fmt, W) * H
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "in.raw")
        torch.randint(16, 236, (n,), dtype=torch.uint8).numpy().tofile(path)
        r = subprocess.run([HARNESS, "run", name, options, cn, "cf", os.path.join(tmp, "out"), str(reps), str(W), str(H), path], capture_output=True, text=True, timeout=600)
    ms = [ln.split("ms_per_frame=")[1] for ln in r.stdout.splitlines() if "ms_per_frame=" in ln]
    cpus = [ln[5:] for ln in r.stdout.splitlines() if ln.startswith("cpus=")]
    return {"what": "cpu", "row": label, "module": name, "ms_per_frame": float(ms[0]) if ms else None, "cpus": int(cpus[0]) if cpus else None, "rc": r.returncode}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pixel_filter.py needs a GPU")
    lib = L.load()
    stream = torch.cuda.current_stream().cuda_stream
    only = args.only.split(":") if args.only else None
    for row in ROWS:
        for frames in (1, 8):
            if only and [row[0], str(frames)] != only:
                continue
            print(json.dumps(kernel_row(lib, stream, row, frames, args.iters)), flush=True)
            torch.cuda.empty_cache()
    if only or args.no_cpu or not os.path.exists(HARNESS):
        return
    for row in ROWS:
        if row[0] == "matrix2-v210":  # the reference writes three times its output frame there (matrix2.c:239-241): not run outside the padded harness
            continue
        print(json.dumps(cpu_row(lib, row, args.cpu_reps)), flush=True)


if __name__ == "__main__":
    main()
