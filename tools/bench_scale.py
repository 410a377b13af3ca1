#!/usr/bin/env python3
"""Kernel time of ug_hip_scale (`-p scale`) and the whole postprocess path against its copy-only twin.

  kernel   4K -> 1080p, 1080p -> 4K, 8K -> 4K; RGBA and UYVY; 1 and 8 frames per launch: ms per frame and the fraction of 8 TB/s on
           algorithmic bytes (input + output once)
  call     one frame through pinned host memory: upload, kernel, download (what the module's postprocess does) against the upload and
           download of the same bytes alone
Prints one JSON line per measurement.  python tools/bench_scale.py [--iters N]
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
SIZES = {"4K->1080p": (3840, 2160, 1920, 1080), "1080p->4K": (1920, 1080, 3840, 2160), "8K->4K": (7680, 4320, 3840, 2160)}


def linesize(fmt, w):
    return L.load().ug_hip_linesize(fmt, w)


def time_ms(fn, iters):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    lib = L.load()
    stream = torch.cuda.current_stream().cuda_stream
    for name, (w, h, ow, oh) in SIZES.items():
        for fname, fmt in (("RGBA", L.PF_RGBA), ("UYVY", L.PF_UYVY)):
            sb, db = linesize(fmt, w) * h, linesize(fmt, ow) * oh
            for frames in (1, 8):
                src = torch.randint(0, 256, (sb * frames,), dtype=torch.uint8, device="cuda")
                dst = torch.empty(db * frames, dtype=torch.uint8, device="cuda")
                d = L.ScaleDesc(src.data_ptr(), dst.data_ptr(), fmt, 0, w, h, ow, oh, 0, 0, frames, sb, db)

                def k():
                    L.check(lib.ug_hip_scale(C.byref(d), stream), "ug_hip_scale")
                ms = time_ms(k, args.iters) / frames
                print(json.dumps({"what": "kernel", "case": name, "fmt": fname, "frames": frames, "ms_per_frame": round(ms, 4),
                                  "frac_8TBps": round((sb + db) / (ms * 1e-3) / PEAK, 3)}), flush=True)
            # the postprocess path, one frame: pinned in -> device -> kernel -> device -> pinned out, and the copies alone
            hin = torch.randint(0, 256, (sb,), dtype=torch.uint8).pin_memory()
            hout = torch.empty(db, dtype=torch.uint8).pin_memory()
            src = torch.empty(sb, dtype=torch.uint8, device="cuda")
            dst = torch.empty(db, dtype=torch.uint8, device="cuda")
            d = L.ScaleDesc(src.data_ptr(), dst.data_ptr(), fmt, 0, w, h, ow, oh, 0, 0, 1, 0, 0)

            def call():
                src.copy_(hin, non_blocking=True)
                L.check(lib.ug_hip_scale(C.byref(d), stream), "ug_hip_scale")
                hout.copy_(dst, non_blocking=True)

            def twin():
                src.copy_(hin, non_blocking=True)
                hout.copy_(dst, non_blocking=True)
            t_call, t_twin = time_ms(call, args.iters), time_ms(twin, args.iters)
            print(json.dumps({"what": "call", "case": name, "fmt": fname, "ms": round(t_call, 4), "copies_ms": round(t_twin, 4),
                              "ratio": round(t_call / t_twin, 3)}), flush=True)


if __name__ == "__main__":
    main()
