#!/usr/bin/env python3
"""RGB / RGBA -> UG_PF_UYVY_GL (`-c uyvy`'s conversion, csrc/uyvy_gl.hip) kernel timings.

Rows: 4K and 8K, one frame per launch (ug_hip_pixfmt_convert) and 8 frames per launch (ug_hip_pixfmt_convert_batch, frames one picture
apart = one launch), RGB and RGBA input.  Source and destination rings of frames span >= 600 MB each, so every launch reads and writes
memory that is not in the 256 MB last-level cache.  Time = GPU time between two events around `iters` launches, per frame.
Algorithmic bytes per frame = w * h * (3 or 4) read + w * h * 2 written; frac = (bytes / time) / 8 TB/s; target 0.6.
    python tools/bench_uyvy.py [--iters N] [--out FILE]
Counters (a run of their own): rocprofv3 --pmc TCC_EA0_RDREQ_sum TCC_EA0_WRREQ_sum ... -- python tools/bench_uyvy.py --only 4K-RGB-x8
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ultragrid_amd import lib  # noqa: E402

PEAK = 8e12
TARGET = 0.6
RING_BYTES = 600 << 20


def row(l, w, h, fmt, batch, iters):
    bpp = 3 if fmt == lib.PF_RGB else 4
    sbytes, dbytes = w * h * bpp, (w + 1) // 2 * 4 * h
    per_launch = batch
    slots = max(2, -(-RING_BYTES // (dbytes * per_launch)) + 1)
    src = torch.randint(0, 256, (slots * per_launch * sbytes,), dtype=torch.uint8, device="cuda")
    dst = torch.empty((slots * per_launch * dbytes,), dtype=torch.uint8, device="cuda")
    s, d = src.data_ptr(), dst.data_ptr()

    def launch(i):
        k = i % slots
        so, do = s + k * per_launch * sbytes, d + k * per_launch * dbytes
        if batch == 1:
            rc = l.ug_hip_pixfmt_convert(fmt, lib.PF_UYVY_GL, so, do, w, h, 0, 0, 0, 8, 16, None)
        else:
            rc = l.ug_hip_pixfmt_convert_batch(fmt, lib.PF_UYVY_GL, so, do, w, h, 0, 0, 0, 8, 16, batch, sbytes, dbytes, None)
        assert rc == 0, rc

    for i in range(2 * slots):
        launch(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        launch(i)
    e1.record()
    torch.cuda.synchronize()
    us_frame = e0.elapsed_time(e1) * 1e3 / (iters * batch)
    gbs = (sbytes + w * h * 2) / (us_frame * 1e-6) / 1e9
    frac = gbs * 1e9 / PEAK
    return dict(row=f"{'4K' if w == 3840 else '8K'}-{'RGB' if bpp == 3 else 'RGBA'}-x{batch}", us_per_frame=round(us_frame, 2),
                GBps=round(gbs, 1), frac_8TBps=round(frac, 3), target=TARGET, met=frac >= TARGET, ring_MB=round(slots * per_launch * dbytes / 2**20))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    l = lib.load()
    rows = []
    for w, h in ((3840, 2160), (7680, 4320)):
        for fmt in (lib.PF_RGB, lib.PF_RGBA):
            for batch in (1, 8):
                name = f"{'4K' if w == 3840 else '8K'}-{'RGB' if fmt == lib.PF_RGB else 'RGBA'}-x{batch}"
                if a.only and a.only != name:
                    continue
                r = row(l, w, h, fmt, batch, a.iters)
                rows.append(r)
                print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
