#!/usr/bin/env python3
"""R, G, B + alpha (subsampling 4444, RGBA input) against its R,G,B 4:4:4 twin, same session, same picture: encode per frame at one frame per
call and n frames per call, both layouts (interleaved, one scan per component); decode per frame with restart intervals and without.
Prints one line per leg and the 4444 / 444 ratios (the ideal is 4/3, the block count)."""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from ultragrid_amd import lib as L, synth

ap = argparse.ArgumentParser()
ap.add_argument("--size", default="3840x2160")
ap.add_argument("--n", type=int, default=8)
ap.add_argument("--q", type=int, default=75)
ap.add_argument("--ri", type=int, default=4)
ap.add_argument("--seconds", type=float, default=0.5)
ap.add_argument("--only", choices=["all", "encode", "decode"], default="all", help="profile runs: one side only")
a = ap.parse_args()
l = L.load()
w, h = (int(x) for x in a.size.split("x"))
st = torch.cuda.current_stream().cuda_stream
rgb = synth.frame("S2", "RGB", w, h).reshape(h, w, 3)
yy, xx = np.mgrid[0:h, 0:w]
alpha = (255 * (xx + yy) / (w + h - 2)).astype(np.uint8)
pics = {444: np.ascontiguousarray(rgb).ravel(), 4444: np.concatenate([rgb, alpha[..., None]], -1).ravel()}
pf = {444: L.PF_RGB, 4444: L.PF_RGBA}


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


res = {}
if a.only in ("all", "encode"):
    for flags, lay in ((0, "interleaved"), (L.JPEG_NONINTERLEAVED, "one scan per component")):
        for sub in (444, 4444):
            base = torch.from_numpy(pics[sub]).cuda()
            line = (4 if sub == 4444 else 3) * w
            src = torch.stack([torch.roll(base, line * 37 * f) for f in range(a.n)])
            enc = C.c_void_p()
            assert l.ug_hip_jpeg_encoder_create_ex(w, h, a.q, a.ri, sub, 0, flags, C.byref(enc)) == 0
            cap = l.ug_hip_jpeg_encoder_max_size(enc)
            stride = (min(cap, w * h * 4 + 4096) + 15) // 16 * 16
            out = torch.empty((a.n, stride), dtype=torch.uint8, device="cuda")
            lens, one = (C.c_size_t * a.n)(), C.c_size_t(0)

            def single():
                assert l.ug_hip_jpeg_encoder_encode(enc, pf[sub], src[0].data_ptr(), 0, out[0].data_ptr(), stride, C.byref(one), st) == 0

            def batch():
                assert l.ug_hip_jpeg_encoder_encode_batch(enc, pf[sub], a.n, src.data_ptr(), 0, src.shape[1], out.data_ptr(), stride, stride, lens, st) == 0

            for name, fn, per in (("n=1", single, 1), (f"n={a.n}", batch, a.n)):
                us = timed(fn, per)
                res[("enc", lay, name, sub)] = us
                print(f"jpeg encode {w}x{h} {sub} q{a.q} restart {a.ri} {lay}, {name}: {us:.1f} us per frame, stream {one.value or lens[0]} B", flush=True)
            l.ug_hip_jpeg_encoder_destroy(enc)
if a.only in ("all", "decode"):
    for ri in (a.ri, 0):
        for sub in (444, 4444):
            enc = C.c_void_p()
            assert l.ug_hip_jpeg_encoder_create_ex(w, h, a.q, ri, sub, 0, 0, C.byref(enc)) == 0
            cap = l.ug_hip_jpeg_encoder_max_size(enc)
            buf = torch.empty(cap, dtype=torch.uint8, device="cuda")
            n = C.c_size_t(0)
            assert l.ug_hip_jpeg_encoder_encode(enc, pf[sub], torch.from_numpy(pics[sub]).cuda().data_ptr(), 0, buf.data_ptr(), cap, C.byref(n), st) == 0
            l.ug_hip_jpeg_encoder_destroy(enc)
            data = bytes(buf[: n.value].cpu().numpy())
            dec = C.c_void_p()
            assert l.ug_hip_jpeg_decoder_create(C.byref(dec)) == 0
            dst = torch.empty(4 * w * h, dtype=torch.uint8, device="cuda")
            pinned = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).pin_memory()

            def decode():
                assert l.ug_hip_jpeg_decoder_decode(dec, C.c_void_p(pinned.data_ptr()), len(data), pf[sub] if sub == 444 else L.PF_RGBA, dst.data_ptr(), 0, 0, 8, 16, st) == 0

            us = timed(decode, 1)
            res[("dec", ri, sub)] = us
            print(f"jpeg decode {w}x{h} {sub} q{a.q} restart {ri} -> {'RGB' if sub == 444 else 'RGBA'}: {us:.1f} us per frame, stream {len(data)} B", flush=True)
            l.ug_hip_jpeg_decoder_destroy(dec)
for k, v in res.items():
    if k[-1] == 4444:
        print(f"ratio 4444/444 {' '.join(str(x) for x in k[:-1])}: {v / res[k[:-1] + (444,)]:.2f}")
