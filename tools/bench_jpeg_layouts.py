#!/usr/bin/env python3
"""JPEG decode of the sampling layouts layout_pack_kernel serves (4:4:0, 4:1:1, 4:1:0, subsampled R,G,B) against 4:2:0 Y'CbCr of the same
picture and size: whole-frame decode from pinned host memory to a device-resident destination, RGBA and UYVY, and the planes-only decode
(UG_PF_NONE) whose difference is the output stage.  Streams come from tests/jpeg_layout_bitstream.py (q75, restart 4 by default); --cache DIR
keeps them between runs (the writer is pure Python).  Prints one line per leg and the ratios to 4:2:0 Y'CbCr.  For the kernel alone, run under
rocprofv3 --kernel-trace --stats and read layout_pack_kernel's time."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from ultragrid_amd import lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--size", default="3840x2160")
ap.add_argument("--q", type=int, default=75)
ap.add_argument("--ri", type=int, default=4)
ap.add_argument("--seconds", type=float, default=0.5)
ap.add_argument("--cache", default="", help="directory for the generated streams")
a = ap.parse_args()
w, h = (int(x) for x in a.size.split("x"))
LEGS = [("ycc", 420), ("ycc", 440), ("ycc", 411), ("ycc", 410), ("rgb", 420), ("rgb", 422), ("rgb", 444)]


def stream(kind, code):
    path = os.path.join(a.cache, f"{kind}{code}_{w}x{h}_q{a.q}_r{a.ri}.jpg") if a.cache else ""
    if path and os.path.exists(path):
        return open(path, "rb").read()
    from oracle import pyoracle as po
    from jpeg_layout_bitstream import layout_stream
    data = layout_stream(po, w, h, code, restart=a.ri, rgb="both" if kind == "rgb" else None, q=a.q)
    if path:
        os.makedirs(a.cache, exist_ok=True)
        open(path, "wb").write(data)
    return data


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < a.seconds:
        fn()
        n += 1
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


l = L.load()
st = torch.cuda.current_stream().cuda_stream
dst = torch.empty(4 * w * h + 64, dtype=torch.uint8, device="cuda")
res = {}
for kind, code in LEGS:
    data = stream(kind, code)
    pinned = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).pin_memory()
    dec = C.c_void_p()
    assert l.ug_hip_jpeg_decoder_create(C.byref(dec)) == 0
    for out in ("NONE", "UYVY", "RGBA"):
        fmt = getattr(L, "PF_" + out)

        def decode():
            assert l.ug_hip_jpeg_decoder_decode(dec, C.c_void_p(pinned.data_ptr()), len(data), fmt, C.c_void_p(dst.data_ptr()), 0, 0, 8, 16, st) == 0

        us = timed(decode)
        res[(kind, code, out)] = us
        print(f"jpeg decode {w}x{h} {kind} {code} q{a.q} restart {a.ri} -> {out}: {us:.1f} us per frame, stream {len(data)} B", flush=True)
    l.ug_hip_jpeg_decoder_destroy(dec)
for (kind, code, out), us in res.items():
    base = res[("ycc", 420, out)]
    stage, base_stage = us - res[(kind, code, "NONE")], base - res[("ycc", 420, "NONE")]
    print(f"{kind} {code} -> {out}: {us / base:.3f} x 4:2:0 Y'CbCr whole frame" + ("" if out == "NONE" else f"; output stage {stage:.1f} us (4:2:0 Y'CbCr {base_stage:.1f})"))
