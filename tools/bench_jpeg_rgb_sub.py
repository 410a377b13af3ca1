#!/usr/bin/env python3
"""R, G, B at 4:2:0 / 4:2:2 (create_ex with UG_JPEG_INPUT_RGB, RGB input) against the R, G, B 4:4:4 stream and the 4:2:0 Y'CbCr stream of the
same picture, same session: device-resident input, encode per frame at one frame per call and n frames per call, both scan layouts (Y'CbCr 4:2:0:
one interleaved scan, from UYVY).  --only frontend: only the R, G, B 4:2:x encodes (for a kernel trace of rgb_jpeg42x_kernel).  The samples of the
4:2:x R, G, B path are unpinned towards libgpujpeg (its preprocessor is not in the reference tree)."""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from oracle import pyoracle as po
from ultragrid_amd import lib as L, synth

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="1920x1080,3840x2160")
ap.add_argument("--n", type=int, default=8)
ap.add_argument("--q", type=int, default=75)
ap.add_argument("--ri", type=int, default=4)
ap.add_argument("--seconds", type=float, default=0.5)
ap.add_argument("--only", choices=["all", "frontend"], default="all")
a = ap.parse_args()
l = L.load()
st = torch.cuda.current_stream().cuda_stream
YCC = "Y'CbCr 420"


def timed(fn, per):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < a.seconds:
        fn()
        n += 1
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (n * per) * 1e6


for size in a.sizes.split(","):
    w, h = (int(x) for x in size.split("x"))
    rgb = np.ascontiguousarray(synth.frame("S2", "RGB", w, h)).ravel()
    uyvy = po.convert_frame("RGB", "UYVY", rgb, w, h)
    legs = [(f"RGB {sub}", sub, L.JPEG_INPUT_RGB | fl, L.PF_RGB, rgb, lay) for sub in (420, 422)
            for fl, lay in ((0, "interleaved"), (L.JPEG_NONINTERLEAVED, "one scan per component"))]
    if a.only == "all":
        legs += [("RGB 444", 444, fl, L.PF_RGB, rgb, lay) for fl, lay in ((0, "interleaved"), (L.JPEG_NONINTERLEAVED, "one scan per component"))]
        legs += [(YCC, 420, 0, L.PF_UYVY, uyvy, "interleaved")]
    res = {}
    for name, sub, flags, pf, pic, lay in legs:
        base = torch.from_numpy(pic).cuda()
        line = pic.size // h
        src = torch.stack([torch.roll(base, line * 37 * f) for f in range(a.n)])
        enc = C.c_void_p()
        assert l.ug_hip_jpeg_encoder_create_ex(w, h, a.q, a.ri, sub, 0, flags, C.byref(enc)) == 0
        cap = l.ug_hip_jpeg_encoder_max_size(enc)
        stride = (min(cap, w * h * 4 + 4096) + 15) // 16 * 16
        out = torch.empty((a.n, stride), dtype=torch.uint8, device="cuda")
        lens, one = (C.c_size_t * a.n)(), C.c_size_t(0)

        def single():
            assert l.ug_hip_jpeg_encoder_encode(enc, pf, src[0].data_ptr(), 0, out[0].data_ptr(), stride, C.byref(one), st) == 0

        def batch():
            assert l.ug_hip_jpeg_encoder_encode_batch(enc, pf, a.n, src.data_ptr(), 0, src.shape[1], out.data_ptr(), stride, stride, lens, st) == 0

        for nm, fn, per in (("n=1", single, 1), (f"n={a.n}", batch, a.n)):
            us = timed(fn, per)
            res[(name, lay, nm)] = us
            print(f"jpeg encode {w}x{h} {name} q{a.q} restart {a.ri} {lay}, {nm}: {us:.1f} us per frame, stream {one.value or lens[0]} B", flush=True)
        l.ug_hip_jpeg_encoder_destroy(enc)
    if a.only == "all":
        for (name, lay, nm), us in res.items():
            if name.startswith("RGB 42"):
                ref = res.get(("RGB 444", lay, nm))
                print(f"ratio {w}x{h} {name} / RGB 444, {lay}, {nm}: {us / ref:.2f}; / {YCC} {nm}: {us / res[(YCC, 'interleaved', nm)]:.2f}")
