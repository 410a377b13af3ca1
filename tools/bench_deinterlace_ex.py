#!/usr/bin/env python3
"""Kernel time of ug_hip_deinterlace and the postprocess path against its copy-only twin.

  kernel   every mode (WEAVE with and without the blend) x UYVY, RGB, RG48, v210, R10k, R12L at 1920x1080 and 3840x2160, 1 and 8 frames per
           launch; sources (and the previous frames) rotate over >= 600 MB so that no launch finds its input in a cache: us per frame and the
           fraction of 8 TB/s on algorithmic bytes (every source line read once -- WEAVE: this frame + the odd lines of the previous one --, every
           output byte written once)
  call     one frame through pinned host memory as the modules do it: upload, one launch, download of both outputs -- against the same copies alone
Prints one JSON line per measurement.  python tools/bench_deinterlace_ex.py [--iters N] [--only MODE:FMT:LINES:FRAMES] [--no-call]
(--only: one kernel row, for a counter pass: rocprofv3 --pmc TCC_EA0_RDREQ_sum WRITE_SIZE -- python tools/bench_deinterlace_ex.py --only LINEAR:UYVY:2160:1)
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ultragrid_amd import lib as L  # noqa: E402

PEAK = 8.0e12
ROTATE_BYTES = 600e6
VARIANTS = [("BLEND", L.DEINT_BLEND, 0), ("WEAVE", L.DEINT_WEAVE, 0), ("WEAVE:d", L.DEINT_WEAVE, 1), ("BOB", L.DEINT_BOB, 0), ("LINEAR", L.DEINT_LINEAR, 0)]
FORMATS = [("UYVY", L.PF_UYVY), ("RGB", L.PF_RGB), ("RG48", L.PF_RG48), ("v210", L.PF_V210), ("R10k", L.PF_R10K), ("R12L", L.PF_R12L)]
SIZES = [(1920, 1080), (3840, 2160)]


def algorithmic_bytes(mode, frame_bytes):
    """(read, written) per frame"""
    if mode == L.DEINT_BLEND:
        return frame_bytes, frame_bytes
    return (frame_bytes * 3 // 2 if mode == L.DEINT_WEAVE else frame_bytes), 2 * frame_bytes


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


def kernel_row(lib, stream, vname, mode, blend, fname, fmt, w, h, frames, iters):
    ls = lib.ug_hip_linesize(fmt, w)
    fb = ls * h
    sets = max(2, int(-(-ROTATE_BYTES // (fb * frames))))
    src = torch.randint(0, 256, (sets, fb * frames), dtype=torch.uint8, device="cuda")
    dst = [torch.empty(fb * frames, dtype=torch.uint8, device="cuda") for _ in range(2)]
    descs = [L.DeinterlaceDesc(src[i].data_ptr(), src[(i + 1) % sets].data_ptr(), (C.c_void_p * 2)(dst[0].data_ptr(), dst[1].data_ptr()), fmt, mode, blend, h, ls,
                               0, 0, frames, fb, fb) for i in range(sets)]

    def k(i):
        L.check(lib.ug_hip_deinterlace(C.byref(descs[i % sets]), stream), "ug_hip_deinterlace")
    ms = time_ms(k, iters) / frames
    rd, wr = algorithmic_bytes(mode, fb)
    return {"what": "kernel", "mode": vname, "fmt": fname, "lines": h, "frames": frames, "us_per_frame": round(ms * 1e3, 2),
            "read_MB": round(rd / 1e6, 2), "written_MB": round(wr / 1e6, 2), "frac_8TBps": round((rd + wr) / (ms * 1e-3) / PEAK, 3)}


def call_row(lib, stream, vname, mode, blend, fname, fmt, w, h, iters):
    ls = lib.ug_hip_linesize(fmt, w)
    fb = ls * h
    n_out = 1 if mode == L.DEINT_BLEND else 2
    hin = torch.randint(0, 256, (fb,), dtype=torch.uint8).pin_memory()
    hout = [torch.empty(fb, dtype=torch.uint8).pin_memory() for _ in range(n_out)]
    dev = [torch.zeros(fb, dtype=torch.uint8, device="cuda") for _ in range(2)]
    dst = [torch.empty(fb, dtype=torch.uint8, device="cuda") for _ in range(2)]
    descs = [L.DeinterlaceDesc(dev[i].data_ptr(), dev[1 - i].data_ptr(), (C.c_void_p * 2)(dst[0].data_ptr(), dst[1].data_ptr()), fmt, mode, blend, h, ls, 0, 0, 1, 0, 0)
             for i in range(2)]

    def call(i):
        dev[i % 2].copy_(hin, non_blocking=True)
        L.check(lib.ug_hip_deinterlace(C.byref(descs[i % 2]), stream), "ug_hip_deinterlace")
        for k in range(n_out):
            hout[k].copy_(dst[k], non_blocking=True)
        torch.cuda.current_stream().synchronize()

    def twin(i):
        dev[i % 2].copy_(hin, non_blocking=True)
        for k in range(n_out):
            hout[k].copy_(dst[k], non_blocking=True)
        torch.cuda.current_stream().synchronize()
    t_call, t_twin = time_ms(call, iters), time_ms(twin, iters)
    return {"what": "call", "mode": vname, "fmt": fname, "lines": h, "ms": round(t_call, 4), "copies_ms": round(t_twin, 4), "ratio": round(t_call / t_twin, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-call", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_deinterlace_ex.py needs a GPU")
    lib = L.load()
    stream = torch.cuda.current_stream().cuda_stream
    only = args.only.split(":") if args.only else None
    for vname, mode, blend in VARIANTS:
        for fname, fmt in FORMATS:
            for w, h in SIZES:
                for frames in (1, 8):
                    if only and [vname.replace(":", ""), fname, str(h), str(frames)] != [only[0].replace(":", "")] + only[1:]:
                        continue
                    print(json.dumps(kernel_row(lib, stream, vname, mode, blend, fname, fmt, w, h, frames, args.iters)), flush=True)
                    torch.cuda.empty_cache()
    if only or args.no_call:
        return
    for vname, mode, blend in VARIANTS:
        for fname, fmt in (("UYVY", L.PF_UYVY), ("R12L", L.PF_R12L)):
            for w, h in SIZES:
                print(json.dumps(call_row(lib, stream, vname, mode, blend, fname, fmt, w, h, max(10, args.iters // 5))), flush=True)


if __name__ == "__main__":
    main()
