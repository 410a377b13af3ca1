#!/usr/bin/env python3
"""LDGM FEC timings (profiles/r07_ldgm.txt): the ug_hip_ldgm_* coder against the reference's CPU session.

Per configuration (k, m, c of src/rtp/ldgm.cpp's suggested_configurations; frame sizes of its JPEG / UYVY rows) and loss rate:
  dev      encode / decode of a device buffer, GPU time between two events on the stream (the kernels, plus the schedule upload on decode)
  host     ug_hip_ldgm_encode_host / _decode_host on a pinned host buffer, wall time of the call: PCIe copies included (what the plugin pays)
  ref_cpu  the reference's LDGM_session_cpu through its own ldgm class (oracle/_ref/ug_ldgm_harness, one thread, encode_video_frame /
           decode as UltraGrid calls them), wall time per call
  plugin   the same harness with ldgm-device=GPU: this repository's ldgm_gpu library inside the reference's ldgm class
Algorithmic bytes of encode: edges x ps read + m x ps written (edges = data entries of pcm); of decode: the members read plus the packets
written by the schedule.  GB/s = those bytes over the dev time.
    python tools/bench_ldgm.py [--quick] [--iters N]
Kernel times of their own: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_ldgm.py --quick
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ultragrid_amd import codec, lib  # noqa: E402

HARNESS = os.path.join(ROOT, "oracle", "_ref", "ug_ldgm_harness")
UYVY1080, UYVY4K, UYVY8K = 1920 * 1080 * 2, 3840 * 2160 * 2, 7680 * 4320 * 2
CONFIGS = [  # label, payload bytes, k, m, c
    ("JPEG60 1500 2%", 144000, 750, 120, 5),
    ("JPEG80 1500 5%", 177000, 1250, 375, 6),
    ("JPEG90 1500 10%", 217000, 1500, 750, 8),
    ("1080p UYVY 9000 5%", UYVY1080, 1000, 300, 6),
    ("1080p UYVY 1500 10%", UYVY1080, 1500, 1500, 8),
    ("4K UYVY 9000 10%", UYVY4K, 1000, 500, 7),
    ("8K UYVY k=1500", UYVY8K, 1500, 450, 6),
]
LOSSES = (0.0, 0.02, 0.05, 0.10)


def matrix(tmp, k, m, c):
    """the reference's generator, through the harness (the matrix is a by-product of its first encode)"""
    p = os.path.join(tmp, "p.bin")
    open(p, "wb").write(bytes(64))
    env = dict(os.environ, UG_LDGM_MATRIX_DIR=tmp, UG_PARAM="ldgm-device=CPU")
    subprocess.run([HARNESS, "encode", str(k), str(m), str(c), "1", p, os.path.join(tmp, "o.bin")], env=env, check=True, capture_output=True)
    raw = open(os.path.join(tmp, f"ldgm_matrix-{k}-{m}-{c}-1.bin"), "rb").read()
    nl = raw.index(b"\n")
    kf, mf, wf = (int(x) for x in raw[:nl].split())
    return np.frombuffer(raw[nl + 1: nl + 1 + 4 * mf * wf], "<i4").reshape(mf, wf).copy()


def harness_time(tmp, k, m, c, size, loss, iters, gpu):
    env = dict(os.environ, UG_LDGM_MATRIX_DIR=tmp, UG_PARAM="ldgm-device=GPU" if gpu else "ldgm-device=CPU")
    r = subprocess.run([HARNESS, "time", str(k), str(m), str(c), "1", str(size), str(loss * 100), str(iters)], env=env,
                       capture_output=True, text=True, timeout=600)
    line = [l for l in r.stdout.splitlines() if l.startswith("encode_ms=")]
    if r.returncode != 0 or not line:
        return None
    return dict(kv.split("=") for kv in line[0].split())


def ev_time(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def wall(fn, iters):
    fn()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    return (time.perf_counter() - t) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--no-ref", action="store_true", help="skip the harness rows")
    a = ap.parse_args()
    configs = CONFIGS[:1] + CONFIGS[3:4] + CONFIGS[-1:] if a.quick else CONFIGS
    losses = (0.0, 0.05) if a.quick else LOSSES
    iters = 10 if a.quick else a.iters
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    print(f"# {torch.cuda.get_device_name(0)}; times in ms per call; iters={iters}")
    with tempfile.TemporaryDirectory() as tmp:
        for label, size, k, m, c in configs:
            pcm = matrix(tmp, k, m, c)
            ps = -(-(size + 24 + 4) // (4 * k)) * 4
            edges = int(((pcm >= 0) & (pcm < k)).sum())
            coder = codec.LdgmCoder(k, m, pcm)
            rng = np.random.default_rng(1)
            host = torch.from_numpy(rng.integers(0, 256, (k + m) * ps, dtype=np.uint8)).pin_memory()
            dev = host.cuda()
            coder.encode(dev)
            host.copy_(dev.cpu())
            clean = dev.clone()
            enc_dev = ev_time(lambda: coder.encode(dev), iters)
            enc_bytes = (edges + m) * ps
            hp = host.data_ptr()
            enc_host = wall(lambda: lib.check(L.ug_hip_ldgm_encode_host(coder._h, hp, ps, st), "encode_host"), iters)
            print(f"{label:22s} k={k} m={m} c={c} ps={ps} w_f={pcm.shape[1]} edges={edges}")
            print(f"  encode  dev {enc_dev:8.4f}  host {enc_host:8.4f}  alg {enc_bytes / 1e6:8.2f} MB  {enc_bytes / enc_dev / 1e6:8.1f} GB/s")
            for loss in losses:
                rx = (rng.random(k + m) >= loss).astype(np.uint8)
                coder.decode(dev, rx)
                levels = coder.stats()["levels"]
                rec = np.zeros(k + m, np.uint8)
                okc = C.c_int()

                def dec_dev():
                    coder.decode(dev, rx)

                dd = ev_time(dec_dev, iters)
                hb = host.numpy().copy()
                hbp = hb.ctypes.data  # pageable: what the plugin hands over on decode (the receiver's buffer)
                dh = wall(lambda: lib.check(L.ug_hip_ldgm_decode_host(coder._h, hbp, ps, rx.ctypes.data, rec.ctypes.data, C.byref(okc), st),
                                            "decode_host"), iters)
                nrec = int(rec.sum())
                dec_bytes = nrec * ps * (pcm.shape[1])  # upper bound: members read per recovery
                ref = "" if a.no_ref else harness_time(tmp, k, m, c, size, loss, max(3, iters // 5), False)
                plug = "" if a.no_ref else harness_time(tmp, k, m, c, size, loss, max(3, iters // 5), True)
                print(f"  decode {loss * 100:4.1f}%  dev {dd:8.4f}  host {dh:8.4f}  levels {levels:3d}  rec {nrec:4d}  all_known {okc.value}"
                      f"  <= {dec_bytes / 1e6:7.2f} MB")
                if ref:
                    print(f"      ref_cpu encode {float(ref['encode_ms']):8.4f} decode {float(ref['decode_ms']):8.4f} ({ref['decoded']})"
                          + (f"   plugin encode {float(plug['encode_ms']):8.4f} decode {float(plug['decode_ms']):8.4f} ({plug['decoded']})" if plug else ""))
            dev.copy_(clean)
            coder.close()


if __name__ == "__main__":
    main()
