#!/usr/bin/env python3
"""bench.py -- headline benchmark: Mpixels/s encode (UYVY -> DXT5-YCoCg, 4K) on MI355X.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    (N > 1: either under python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ..., or as plain
     `python bench.py --gpus N`, which then starts the N ranks itself the same way)

A plain run sets up, warms up, times the K steps and prints the line (the driver contract fields, `config` and `roofline`); nothing else.
--dump-outputs DIR: after the timed steps, rank 0 writes what the timed path computed as DIR/<name>.npy (float32; float64 for stream
lengths), whole where it fits, else a fixed seeded sample, at most 64 MB in all (dump_outputs()).  The inputs are seeded: the same
arguments give the same inputs on every run, so that two builds can be compared output for output.
--full adds the legs below (parity_check, configs, e2e, cpu_baseline, cpu_reference), each after the timed region; --no-* switch them off
one by one.

One "step" = passes of the hot path (fused UYVY unpack + YUV->RGB + RGB->YCoCg + DXT5 block encode,
ug_hip_dxt_encode_batch: one launch = `--frames` = 16 distinct synthetic 3840x2160 UYVY frames, BASELINE.json
configs[2]) over `--batches` = 4 resident batches in turn, as many launches as make >= 50 ms of GPU work (calibrated for 60 at steady clocks)
(`config.launches_per_step`), all input already resident in HBM.  Frames are independent, so ranks shard them
with no collective (weak scaling: every rank encodes its own batches).

Prints ONE JSON line (rank 0) with the driver contract fields plus
  roofline     -- algorithmic bytes (3.0 B/px: 2 read + 1 written) x pixels per
                  launch / average launch duration measured with HIP events on the launch stream;
and, with --full only:
  e2e          -- the PCIe-inclusive rate (pinned host -> H2D -> kernel -> D2H, 3 frames in flight per GPU, all ranks at once) for
                  8K UYVY (the target's literal configuration), 8K v210 and 4K UYVY: fps per GPU and in total, PCIe GB/s -- reported
                  beside `value`, never as `value`;
  cpu_baseline -- the CPU oracle (oracle/dxt_oracle.c, "port": the reference has no CPU DXT encoder)
                  timed on this box's host cores on a bounded sample (rank 0, at every N).
Additive keys of the default N = 1 line with --full (`value` / `roofline` are computed exactly as before, and first):
  parity_check -- frame 0 of the timed batch, as the timed kernel left it, compared byte for byte with oracle/dxt_oracle.c AFTER the timed region;
  configs      -- the other BASELINE configurations under the same clock: ~1 s of timed launches each (HIP events on the launch stream) ->
                  ms_per_launch, frac of 8 TB/s, launches_timed (the code paths of --workload);
  e2e.latency_ms_depth1 -- one frame in flight: H2D + kernel + D2H of one frame, stage by stage, beside the depth-3 rates;
  roofline.valu.frac_of_measured_peak -- the VALU rate against what a pure v_add_f32 stream issues on this chip (profiles/valu_microbench_mi355x.txt),
                  next to the nominal 2 wave-instructions per clock and CU.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

W, H = 3840, 2160
ALG_BYTES_PER_PX = 3.0     # UYVY 2 B/px read + DXT5 1 B/px written
# --workload: the default is the configuration BASELINE.json's metric is quoted on (configs[2]); configs[4]
# (7680x4320 v210 -> DXT5-YCoCg, frames sharded over the GPUs) is available for the scaling study.
WORKLOADS = {
    "4k-uyvy": dict(w=3840, h=2160, fmt="UYVY", bpp=3.0, frames=16, name="3840x2160 UYVY->YCoCg->DXT5 fused encode (BASELINE.json configs[2])"),
    "8k-v210": dict(w=7680, h=4320, fmt="v210", bpp=16 / 6 + 1, frames=4, name="7680x4320 v210 unpack->YCoCg->DXT5 fused encode (BASELINE.json configs[4])"),
    "4k-uyvy-jpeg420": dict(w=3840, h=2160, fmt="UYVY", out="JPEG420", bpp=5.0, frames=8,
                            name="3840x2160 UYVY->planar 4:2:0 + 8x8 FDCT + quantise, fused (BASELINE.json configs[3]); one launch per frame"),
    "4k-uyvy-jpeg-encode": dict(w=3840, h=2160, fmt="UYVY", out="JPEGENC", bpp=2.0 + 1531222 / (3840 * 2160), frames=8,
                                name="3840x2160 UYVY -> JPEG 4:2:0 q75 restart 4, the whole encoder (forward DCT + quantiser + Huffman coding + byte stuffing fused, "
                                     "stream assembly; ug_hip_jpeg_encoder_encode_batch, 8 frames per call, one synchronisation per call inside the timed region)"),
    "1080p-rgb-dxt1": dict(w=1920, h=1080, fmt="RGB", out="DXT1", bpp=3.5, frames=64, name="1920x1080 RGB->DXT1 encode (BASELINE.json configs[1])"),
}
HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: 8 TB/s spec
VALU_PEAK = 256 * 2 * 2.4e9  # wave64 VALU instructions per second: 256 CUs x 4 SIMD-32 x one wave64 op per 2 cycles x 2.4 GHz
# what the SIMDs deliver on a dependent-free stream of full-rate fp32 operations, measured (tools/valu_microbench.hip, profiles/valu_microbench_mi355x.txt:
# v_add_f32 1.492, v_mul_f32 1.448, v_mov_b32 1.775 wave-instr/clk/CU; half-rate classes -- v_min3, v_cvt, v_perm, v_bfe, DPP -- 0.95-0.97)
VALU_MEASURED_PEAK = 256 * 1.492 * 2.4e9


def make_frames(n: int, rank: int, fmt: str = "UYVY", w: int = W, h: int = H) -> np.ndarray:
    """n distinct legal-range video-noise frames (S2); up to 4 generated bases, the rest are row-rotations
    by multiples of 4 lines (distinct bytes in memory, same statistics)."""
    from ultragrid_amd import synth
    cache = f"/tmp/ug_bench_frames_{fmt}_{w}x{h}_{n}_{rank}.npy"   # same bytes every time; only saves generation time on repeat runs
    if os.path.exists(cache):
        return np.load(cache)
    ls = synth.linesize(fmt, w)
    gen = synth.s1_random if fmt == "RGB" else synth.s2_video   # RGB: uniform random bytes (S1), every block at full range
    bases = [gen(fmt, w, h, salt=100 * rank + i).reshape(h, ls) for i in range(min(n, 4 if w <= 3840 else 2))]
    out = np.empty((n, h, ls), np.uint8)
    for i in range(n):
        out[i] = np.roll(bases[i % len(bases)], 4 * 37 * (i // len(bases)), axis=0)
    out = out.reshape(n, -1)
    try:
        np.save(cache, out)
    except OSError:
        pass
    return out


def cpu_baseline(frame: np.ndarray, fmt: str, w: int, h: int, target_s: float = 12.0, out: str = "DXT5") -> dict:
    """The C oracle on the host cores: block rows dealt to OpenMP threads (row bands, as the reference parallelises its CPU
    conversions, src/utils/parallel_conv.c:64-85).  The thread count is calibrated (the box may expose more logical CPUs than
    its cpuset lets run); `cores` reports the count that was used for the timed sample."""
    from oracle import pyoracle as po
    ncpu = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    pin = {"UYVY": po.IN_UYVY, "v210": po.IN_V210, "RGB": po.IN_RGB}[fmt]
    pout = po.OUT_DXT5YCOCG if out == "DXT5" else po.OUT_DXT1

    def one(threads: int) -> float:
        t0 = time.perf_counter()
        po.dxt_encode(pin, pout, frame, w, h, threads=threads)
        return time.perf_counter() - t0

    one(1 if ncpu == 1 else min(ncpu, 8))                                  # warm (page in, spawn the team)
    cands = sorted({t for t in (1, 4, 8, 16, 32, 64, 128, 256, ncpu) if t <= ncpu})
    best_t, best = 1, float("inf")
    for t in cands:
        dt = min(one(t), one(t))
        if dt < best:
            best_t, best = t, dt
    n, t0 = 0, time.perf_counter()
    while n < 3 or time.perf_counter() - t0 < target_s:      # bounded by time, not by a frame count guessed from one call
        po.dxt_encode(pin, pout, frame, w, h, threads=best_t)
        n += 1
    dt = time.perf_counter() - t0
    return {"value": round(n * w * h / dt / 1e6, 2), "unit": "Mpixels/s", "cores": best_t, "kind": "port",
            "sample": f"{n} x {w}x{h} {fmt}->{'DXT5-YCoCg' if out == 'DXT5' else 'DXT1'} frames through oracle/dxt_oracle.c (gcc -O2, strict fp32, OpenMP dynamic "
                      f"row bands; {best_t} threads = best of {cands} on {ncpu} visible CPUs), {dt:.1f} s"}


def cpu_reference(fmt: str, w: int, h: int) -> dict | None:
    """The reference's OWN CPU code for the pixel-format half of this workload, where it has one (the DXT encoders exist as GLSL / CUDA only):
    the line converter its CPU path runs on such frames (UYVY -> RGB, v210 -> UYVY, RGB -> UYVY), from oracle/_ref/libugref.so -- pixfmt_conv.c
    compiled from the reference tree with its -O3 -msse4.1 --, over even row bands with the reference's own parallel_pix_conv()
    (src/utils/parallel_conv.c:64-85); the best thread count is reported.  None when the compiled reference is not there."""
    import ctypes as C
    from oracle import pyoracle as po
    if not po.have_ref():
        return None
    i, o = {"UYVY": ("UYVY", "RGB"), "v210": ("v210", "UYVY"), "RGB": ("RGB", "UYVY")}[fmt]
    r = po.ref()
    r.parallel_pix_conv.restype = None
    r.parallel_pix_conv.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    ci, co = po.REF_CODEC[i], po.REF_CODEC[o]
    fn = r.get_decoder_from_to(ci, co)
    sls, dls = r.vc_get_linesize(w, ci), r.vc_get_linesize(w, co)
    from ultragrid_amd import synth
    src = np.concatenate([synth.s1_random(i, w, h, salt=1), np.zeros(64, np.uint8)])
    dst = np.zeros(dls * h + 64, np.uint8)
    ncpu = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    cands = sorted({t for t in (1, 8, 16, 32, 64, 128, ncpu) if t <= ncpu})
    best_t, best = 1, float("inf")
    for t in cands:
        r.parallel_pix_conv(h, dst.ctypes.data, dls, src.ctypes.data, sls, fn, t)   # spawn / warm
        n, t0 = 0, time.perf_counter()
        while n < 5 or time.perf_counter() - t0 < 0.3:
            r.parallel_pix_conv(h, dst.ctypes.data, dls, src.ctypes.data, sls, fn, t)
            n += 1
        dt = (time.perf_counter() - t0) / n
        if dt < best:
            best_t, best = t, dt
    return {"value": round(w * h / best / 1e6, 1), "unit": "Mpixels/s", "cores": best_t, "kind": "reference",
            "sample": f"{w}x{h} {i}->{o} by the reference's own line converter (pixfmt_conv.c from the reference tree, -O3 -msse4.1) over parallel_pix_conv row bands; "
                      f"{best_t} threads = best of {cands} on {ncpu} visible CPUs; the pixel-format half of the workload only (the reference has no CPU DXT encoder)"}


def e2e_leg(workloads, rank: int, dist, device_for_gather: str, seconds: float) -> dict:
    """PCIe-inclusive leg (never `value`): every rank drives ITS GPU from pinned host frames -- allocated after the
    process is bound to the GPU's NUMA node -- with 3 frames in flight (H2D -> fused kernel -> D2H), all ranks at the same time,
    so that at N > 1 the host-side limit (PCIe root complexes, DRAM bandwidth, NUMA) shows up instead of a trivially linear kernel
    curve (scheme: gpujpeg.cpp:446-466,643-722)."""
    from ultragrid_amd import pipeline
    affinity = os.sched_getaffinity(0) if hasattr(os, "sched_getaffinity") else None
    try:
        node = pipeline.gpu_numa_node(torch.cuda.current_device())
        bound = pipeline.bind_to_numa_node(node)
    except (OSError, ValueError):
        node, bound = -1, 0
    res = {}
    for wl in workloads:
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        try:
            # the leg and, BESIDE it, the same traffic without the kernel (what the link alone gives for this in/out byte mix, all ranks at once like the
            # leg itself): copy 0.7 s, half the leg, copy, the other half, copy -- the ceiling is the best of the three
            r = pipeline.run(wl, depth=3, seconds=seconds, salt=17 * rank, mode="split", copy_only_runs=3, copy_only_seconds=0.7)
            ceil = r["copy_only_fps"]
        except Exception as e:   # a rank that cannot run its leg reports 0 fps; the collectives below still see every rank
            print(f"bench.py: e2e leg {wl} failed on rank {rank}: {e}", file=sys.stderr, flush=True)
            _, _, oid, w_, h_ = pipeline.WORKLOADS[wl]
            r = {"fps": 0.0, "pcie_gbs": 0.0, "in_flight": 3, "bytes_in_per_frame": 0, "bytes_out_per_frame": 0, "seconds": 0.0, "copy_only_fps_runs": []}
            ceil = 0.0
        from ultragrid_amd import shard
        rates = shard.gather_rates([r["fps"], r["pcie_gbs"], ceil], dist, device_for_gather)
        per = [round(x[0], 1) for x in rates]
        pcie = [round(x[1], 2) for x in rates]
        ceils = [round(x[2], 1) for x in rates]
        w, h = pipeline.WORKLOADS[wl][3], pipeline.WORKLOADS[wl][4]
        res[wl] = {"fps_total": round(sum(per), 1), "fps_per_gpu": per, "mpixels_per_s_total": round(sum(per) * w * h / 1e6, 1),
                   "pcie_gbs_total": round(sum(pcie), 2), "pcie_gbs_per_gpu": pcie, "in_flight": r["in_flight"],
                   "copy_only_fps_per_gpu": ceils, "copy_only_runs": r.get("copy_only_fps_runs", []), "frac_of_copy_only": round(sum(per) / sum(ceils), 3) if sum(ceils) else None,
                   "bytes_in_per_frame": r["bytes_in_per_frame"], "bytes_out_per_frame": r["bytes_out_per_frame"], "seconds": r["seconds"]}
    # the box's link by itself (rank 0's GPU; pure copies, 2 in flight per direction); the other ranks wait: both barriers are reached whatever the probe does
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    lp = None
    if rank == 0:
        try:
            lp = pipeline.link_probe(seconds=0.5, streams=2)
        except Exception as e:
            print(f"bench.py: link probe failed: {e}", file=sys.stderr, flush=True)
    if dist is not None:
        dist.barrier()
    if lp is not None:
        res["link_gbs_h2d"], res["link_gbs_d2h"], res["link_gbs_bidir_each"] = lp["h2d_gbs"], lp["d2h_gbs"], lp["bidir_each_gbs"]
    # one frame in flight (VERDICT r4 next #2c): what a display-rate source waits for between handing a frame over and holding its compressed form
    lat = {}
    for wl in workloads:
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        if rank == 0:
            try:
                lat[wl] = pipeline.latency_depth1(wl, frames=24, salt=5)
            except Exception as e:
                print(f"bench.py: latency leg {wl} failed: {e}", file=sys.stderr, flush=True)
    if dist is not None:
        dist.barrier()
    if lat:
        res["latency_ms_depth1"] = lat
    res["path"] = ("pinned host frame -> H2D -> fused unpack+encode kernel -> D2H, 3 frames in flight per GPU, all ranks concurrently; "
                   "one upload, one compute and one download stream with events between the stages of a frame (tools/e2e_bench.py --sweep: better than a stream per frame); copy_only_fps = the same copies without the kernel, best of the three 0.7 s runs "
                   "(copy_only_runs, rank 0's) taken before, between and after the two halves of the leg they bound (the link's ceiling for that byte mix); link_gbs_* = pure copies on rank 0's GPU")
    res["numa_node_rank0"] = node
    res["cpus_bound_rank0"] = bound
    if affinity is not None and bound:
        os.sched_setaffinity(0, affinity)   # the CPU baseline that follows is not meant to run on one NUMA node only
    return res


def setup_workload(name: str, frames: int, batches: int, rank: int) -> dict:
    """B resident batches of F distinct frames of the workload in HBM and launch(b): one pass of its hot path over batch b on torch's current stream"""
    from ultragrid_amd import codec, lib
    stream_bytes, enc = [0], None
    wl = WORKLOADS[name]
    W, H = wl["w"], wl["h"]
    ALG_BYTES_PER_PX = wl["bpp"]
    F = frames or wl["frames"]
    B = max(1, batches)
    out_name = wl.get("out", "DXT5")
    # B resident batches of F distinct frames: a few generated bases, the rest row-rotations made on the device
    host = make_frames(min(F, 4 if W <= 3840 else 2), rank, wl["fmt"], W, H)
    frame_bytes = host.shape[1]
    ls = frame_bytes // H
    bases = torch.from_numpy(host).cuda().view(host.shape[0], H, ls)
    src = torch.empty((B, F, H, ls), dtype=torch.uint8, device="cuda")
    for b in range(B):
        for i in range(F):
            k = b * F + i
            src[b, i] = torch.roll(bases[k % bases.shape[0]], 4 * 37 * (k // bases.shape[0]), dims=0)
    del bases
    src = src.view(B, F * frame_bytes)
    out_bytes = {"DXT5": W * H, "DXT1": W * H // 2, "JPEG420": W * H * 3, "JPEGENC": 16}[out_name]
    dst = torch.empty((B, F * out_bytes), dtype=torch.uint8, device="cuda")
    pf = lib.PF_NAMES[wl["fmt"]]
    oid = lib.DXT5_YCOCG if out_name == "DXT5" else lib.DXT1

    def launch(b: int):
        codec.dxt_encode_batch(pf, oid, src[b], W, H, F, frame_bytes, dst=dst[b])

    if out_name == "JPEG420":   # the JPEG front end: UYVY -> 4:2:0 (uyvy_to_i420 rounding) -> FDCT -> quantise, int16 coefficients out
        div = codec.jpeg_divisors_device(75, "cuda")
        mw, mh = (W + 15) // 16, (H + 15) // 16
        nblk = mw * mh
        oy = torch.empty((F, 4 * nblk, 64), dtype=torch.int16, device="cuda")
        ocb, ocr = torch.empty((F, nblk, 64), dtype=torch.int16, device="cuda"), torch.empty((F, nblk, 64), dtype=torch.int16, device="cuda")
        fn = lib.load().ug_hip_uyvy_to_jpeg42x_coeffs_batch

        def launch(b: int):  # noqa: F811  (one launch over the F frames of the batch, grid.z = frame)
            rc = fn(420, src[b].data_ptr(), 0, W, H, div.data_ptr(), oy.data_ptr(), ocb.data_ptr(), ocr.data_ptr(), F, frame_bytes,
                    4 * nblk * 128, nblk * 128, torch.cuda.current_stream().cuda_stream)
            assert rc == 0, lib.last_error()

    if out_name == "JPEGENC":   # the whole JPEG encoder: F frames per (synchronous) call, streams into a per-batch buffer
        import ctypes as C
        l_ = lib.load()
        enc = C.c_void_p()
        assert l_.ug_hip_jpeg_encoder_create_sub(W, H, 75, 4, 420, C.byref(enc)) == 0, lib.last_error()
        stride = (W * H + 4096 + 15) // 16 * 16          # a 4K q75 stream is ~1.5 MB; the capacity a caller would give a 4:2:0 frame of video
        jout = torch.empty((B, F, stride), dtype=torch.uint8, device="cuda")
        lens = (C.c_size_t * F)()

        def launch(b: int):  # noqa: F811
            rc = l_.ug_hip_jpeg_encoder_encode_batch(enc, pf, F, src[b].data_ptr(), 0, frame_bytes, jout[b].data_ptr(), stride, stride, lens,
                                                     torch.cuda.current_stream().cuda_stream)
            assert rc == 0, lib.last_error()
            assert all(lens[f] <= stride for f in range(F)), "a stream did not fit its slice: the call would be timed on a truncated stream"
            stream_bytes[0] = sum(lens[f] for f in range(F))

    # (the device buffers a workload needs live as long as its launch closure does)
    ws = dict(wl=wl, W=W, H=H, F=F, B=B, bpp=ALG_BYTES_PER_PX, out_name=out_name, frame_bytes=frame_bytes, out_bytes=out_bytes, launch=launch,
              stream_bytes=stream_bytes, host=host, src=src, dst=dst, enc=enc)
    if out_name == "JPEG420":
        ws["coef"] = (oy, ocb, ocr)
    if out_name == "JPEGENC":
        ws["jout"], ws["lens"], ws["stride"] = jout, lens, stride
    return ws


def time_launches(launch, B: int, seconds: float) -> tuple:
    """~0.2 s of launches to reach steady clocks, then `seconds` of back-to-back launches between two HIP events on the launch stream
    (torch's current stream): (average ms per launch, launches timed)"""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.2:
        for i in range(4 * B):
            launch(i % B)
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(8 * B):
        launch(i % B)
    e1.record()
    torch.cuda.synchronize()
    n = max(B, int(seconds * 1e3 / max(e0.elapsed_time(e1) / (8 * B), 1e-3)) // B * B)
    e0.record()
    for i in range(n):
        launch(i % B)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, n


def parity_check(ws: dict) -> dict:
    """frame 0 of batch 0 as the timed kernel left it in its output buffer, against oracle/dxt_oracle.c on the same input bytes (the checker, after the
    timed region; DXT workloads)"""
    from oracle import pyoracle as po
    W, H, fmt = ws["W"], ws["H"], ws["wl"]["fmt"]
    torch.cuda.synchronize()
    src0 = ws["src"][0][: ws["frame_bytes"]].cpu().numpy()
    got = ws["dst"][0][: ws["out_bytes"]].cpu().numpy()
    pin = {"UYVY": po.IN_UYVY, "v210": po.IN_V210, "RGB": po.IN_RGB}[fmt]
    pout = po.OUT_DXT5YCOCG if ws["out_name"] == "DXT5" else po.OUT_DXT1
    t0 = time.perf_counter()
    ncpu = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    want = po.dxt_encode(pin, pout, src0, W, H, threads=min(ncpu, 16))
    return {"frames": 1, "bytes_compared": int(want.size), "bytes_differing": int(np.count_nonzero(got != want)) if got.size == want.size else int(max(got.size, want.size)),
            "checker": "oracle/dxt_oracle.c (dxt_encode) on frame 0 of resident batch 0, output of the last timed launch over that batch", "cpu_s": round(time.perf_counter() - t0, 3)}


def _jpeg_oracle_coeffs(src0: np.ndarray, W: int, H: int, quality: int = 75):
    """what the JPEG oracle computes for one UYVY frame, 4:2:0: uyvy_to_i420 (the reference's rounding) + AAN FDCT + quantiser, per component,
    (blocks in raster order of the MCU-padded grid, 64) int16 in zig-zag order"""
    from oracle import pyoracle as po
    y, u, v = po.uyvy_to_i420(src0, W, H)
    mw, mh = (W + 15) // 16, (H + 15) // 16
    dl, dc = po.jpeg_divisors(po.jpeg_qtable(quality, 0)), po.jpeg_divisors(po.jpeg_qtable(quality, 1))
    return po.jpeg_fdct_quant_plane(y, dl, 2 * mw, 2 * mh), po.jpeg_fdct_quant_plane(u, dc, mw, mh), po.jpeg_fdct_quant_plane(v, dc, mw, mh)


def parity_check_jpeg420(ws: dict) -> dict:
    """BASELINE configs[3]: the Y / Cb / Cr coefficients of frame 0 as the LAST timed launch left them (it ran over the last resident batch) against
    po.uyvy_to_i420 + po.jpeg_fdct_quant_plane on the same input bytes; after the timed region"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    b = ws["B"] - 1
    src0 = ws["src"][b][: ws["frame_bytes"]].cpu().numpy()
    want = _jpeg_oracle_coeffs(src0, ws["W"], ws["H"])
    got = [c[0].cpu().numpy() for c in ws["coef"]]
    differing = sum(int(np.count_nonzero(g != w_)) if g.shape == w_.shape else int(max(g.size, w_.size)) for g, w_ in zip(got, want))
    return {"frames": 1, "coefficients_compared": int(sum(w_.size for w_ in want)), "coefficients_differing": differing,
            "checker": "oracle/pixfmt_oracle.c (uyvy_to_i420) + oracle/jpeg_oracle.c (jpeg_fdct_quant_plane) on frame 0 of the last resident batch, output of the last timed launch; "
                       "the FDCT / quantiser oracle is pinned to libjpeg-turbo's float DCT, unpinned towards libgpujpeg", "cpu_s": round(time.perf_counter() - t0, 3)}


def parity_check_jpegenc(ws: dict) -> dict:
    """the whole encoder: frame 0's STREAM as the last timed call wrote it, entropy-decoded by oracle/jpeg_decode_oracle.c back to the quantised
    coefficients it codes, against the coefficients the FDCT oracle computes for the same input bytes; plus the stream lengths of that call"""
    from oracle import pyoracle as po
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    b = ws["B"] - 1
    lens = [int(ws["lens"][f]) for f in range(ws["F"])]
    stream = bytes(ws["jout"][b, 0, : lens[0]].cpu().numpy())
    src0 = ws["src"][b][: ws["frame_bytes"]].cpu().numpy()
    want = _jpeg_oracle_coeffs(src0, ws["W"], ws["H"])
    try:
        info, got = po.jpeg_decode_coeffs(stream)
        ok_hdr = info["width"] == ws["W"] and info["height"] == ws["H"] and info["h"] == [2, 1, 1] and info["v"] == [2, 1, 1]
        differing = sum(int(np.count_nonzero(g != w_)) if g.shape == w_.shape else int(max(g.size, w_.size)) for g, w_ in zip(got, want)) if ok_hdr else int(sum(w_.size for w_ in want))
    except ValueError:
        differing = int(sum(w_.size for w_ in want))
    return {"frames": 1, "coefficients_compared": int(sum(w_.size for w_ in want)), "coefficients_differing": differing, "stream_bytes": lens[0], "lens": lens,
            "ends_with_eoi": stream[-2:] == b"\xff\xd9",
            "checker": "oracle/jpeg_decode_oracle.c (entropy decoder: the stream of frame 0 of the last timed call -> the quantised coefficients it codes) == "
                       "oracle/pixfmt_oracle.c + oracle/jpeg_oracle.c on the same input bytes; unpinned towards libgpujpeg like the FDCT itself", "cpu_s": round(time.perf_counter() - t0, 3)}


def other_configs(rank: int, seconds: float) -> dict:
    """the BASELINE configurations that are not this line's `value`, each through its --workload code path for ~`seconds` of timed launches"""
    res = {}
    for name in ("1080p-rgb-dxt1", "4k-uyvy-jpeg420", "4k-uyvy-jpeg-encode", "8k-v210"):
        ws = setup_workload(name, 0, 4, rank)
        for b in range(ws["B"]):
            ws["launch"](b)
        torch.cuda.synchronize()
        ms, n = time_launches(ws["launch"], ws["B"], seconds)
        px = ws["F"] * ws["W"] * ws["H"]
        alg = ws["bpp"] * px if ws["out_name"] != "JPEGENC" else 2 * px + ws["stream_bytes"][0]
        res[name] = {"workload": ws["wl"]["name"], "frames_per_launch": ws["F"], "ms_per_launch": round(ms, 5), "launches_timed": n,
                     "algorithmic_bytes_per_launch": int(alg), "achieved_gbs": round(alg / (ms * 1e-3) / 1e9, 1), "frac": round(alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                     "mpixels_per_s": round(px / (ms * 1e-3) / 1e6, 1), "fps": round(ws["F"] / (ms * 1e-3), 1)}
        if ws["out_name"] in ("DXT5", "DXT1"):
            res[name]["parity_check"] = parity_check(ws)
        if ws["out_name"] == "JPEG420":
            res[name]["parity_check"] = parity_check_jpeg420(ws)
        if ws["out_name"] == "JPEGENC":
            res[name]["parity_check"] = parity_check_jpegenc(ws)
        if ws["out_name"] == "JPEGENC":
            res[name]["note"] = "the whole encoder per (synchronous) call of 8 frames; the FDCT / quantiser stage is unpinned towards libgpujpeg (pinned to libjpeg-turbo's float DCT)"
            from ultragrid_amd import lib
            lib.load().ug_hip_jpeg_encoder_destroy(ws["enc"])
        del ws
        torch.cuda.empty_cache()
    return res


def load_pmc(pmc_key, root: str = ROOT) -> dict:
    """The counter entry of one bench workload from profiles/pmc_traffic.json (rocprofv3 --pmc passes, tools/gpu_session.sh <tag> pmc) --
    quoted only while the kernel sources it names are the ones of this tree."""
    pmc = {}
    pmc_path = os.path.join(root, "profiles", "pmc_traffic.json")   # written from rocprofv3 --pmc passes (tools/pmc_collect.sh)
    if pmc_key and os.path.exists(pmc_path):
        try:
            pmc = json.load(open(pmc_path)).get(pmc_key) or {}
            if not isinstance(pmc, dict):
                pmc = {"traffic": pmc}
        except Exception:
            pmc = {}
    if pmc.get("kernel_sources_sha16"):
        # the counters name the sources they were taken on (tools/pmc_to_json.py): counters of another build are not quoted
        import hashlib
        h = hashlib.sha256()
        files = pmc.get("kernel_sources") if isinstance(pmc.get("kernel_sources"), list) else []   # (a hash without its file list -- a hand-edited entry -- is stale, not fatal)
        try:
            for f in files:
                h.update(open(os.path.join(root, str(f)), "rb").read())
            now = h.hexdigest()[:16] if files else None
        except OSError:
            now = None
        if now != pmc["kernel_sources_sha16"]:
            pmc = {"source": f"STALE, not quoted: profiles/pmc_traffic.json[{pmc_key}] was taken on another build of {', '.join(map(str, files)) or '(no file list)'} "
                             f"(sha16 {pmc['kernel_sources_sha16']} then, {now} now); re-run tools/gpu_session.sh <tag> pmc"}
        else:
            pmc = dict(pmc, source=pmc.get("source", "") + f"; kernel sources sha16 {now} = the build timed here")
    return pmc


DUMP_MAX_ELEMS = 12 << 20   # --dump-outputs: 12 Mi float32 values in all (48 MiB + headers, under 64 MB)
DUMP_SEED = 20240611


def dump_outputs(ws: dict, launches_per_step: int, out_dir: str) -> dict:
    """--dump-outputs: what the timed launches handed their caller, as `out_dir`/<name>.npy, 1-D float32 (the values are bytes / int16
    coefficients, exact in float32).  DXT: the blocks of every resident batch; JPEG420: the Y / Cb / Cr coefficients of the last launch;
    JPEGENC: the streams of the last call back to back, and their lengths (float64).  An array that does not fit the common budget of
    DUMP_MAX_ELEMS values is sampled: one position drawn (seeded) in each of k equal slices of it, the same positions on every run.
    Returns {name: [values written, values in the output]}."""
    torch.cuda.synchronize()
    out_name = ws["out_name"]
    extra = {}
    if out_name in ("DXT5", "DXT1"):
        arrays = {f"{out_name.lower()}_blocks": ws["dst"].reshape(-1)}
    elif out_name == "JPEG420":
        arrays = dict(zip(("coef_y", "coef_cb", "coef_cr"), (c.reshape(-1) for c in ws["coef"])))
    else:
        b = (launches_per_step - 1) % ws["B"]            # the batch of the last call of the step
        lens = [int(ws["lens"][f]) for f in range(ws["F"])]
        arrays = {"jpeg_streams": torch.cat([ws["jout"][b, f, :n] for f, n in enumerate(lens)])}
        extra["jpeg_stream_lens"] = np.asarray(lens, np.float64)
    total = sum(int(t.numel()) for t in arrays.values())
    os.makedirs(out_dir, exist_ok=True)
    written = {}
    for i, (name, t) in enumerate(arrays.items()):
        n = int(t.numel())
        k = min(n, max(1, n * DUMP_MAX_ELEMS // total))
        if k < n:
            step = n // k
            pos = np.arange(k, dtype=np.int64) * step + np.random.Generator(np.random.PCG64(DUMP_SEED + i)).integers(0, step, k)
            t = t[torch.from_numpy(pos).to(t.device)]
        np.save(os.path.join(out_dir, name + ".npy"), t.cpu().numpy().astype(np.float32))
        written[name] = [k, n]
    for name, a in extra.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
        written[name] = [a.size, a.size]
    return written


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=0, help="distinct frames per launch (batch); 0 = workload default")
    ap.add_argument("--batches", type=int, default=4, help="distinct resident batches the launches of a step cycle through")
    ap.add_argument("--launches-per-step", type=int, default=0, help="kernel launches per step; 0 = as many as make a step >= 50 ms of GPU work")
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="4k-uyvy")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path computed as DIR/<name>.npy (float32, at most 64 MB; rank 0)")
    ap.add_argument("--full", action="store_true", help="also run the legs after the timed region: parity_check, configs, e2e, cpu_baseline, "
                    "cpu_reference (each can be switched off with its --no-* option)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-e2e", action="store_true", help="skip the PCIe-inclusive leg")
    ap.add_argument("--e2e-seconds", type=float, default=2.0)
    ap.add_argument("--no-configs", action="store_true", help="skip the `configs` leg (the other BASELINE configurations, ~1 s of timed launches each; default N = 1 line only)")
    ap.add_argument("--configs-seconds", type=float, default=1.0)
    ap.add_argument("--no-parity-check", action="store_true", help="skip the oracle comparison of frame 0 after the timed region")
    ap.add_argument("--dist-backend", default="nccl", help="nccl (= RCCL, default) | gloo (single-GPU smoke test of the N>1 path)")
    ap.add_argument("--all-ranks-on-device0", action="store_true", help="smoke test only: every rank uses cuda:0")
    ap.add_argument("--force-dist", action="store_true", help="initialise the process group (RCCL) at world size 1 too, so that the barrier, "
                    "agree_max, gather_rates and max-over-ranks collectives run on cuda tensors on a 1-GPU box")
    args = ap.parse_args()

    # `python bench.py --gpus N` without a launcher: start the N ranks ourselves (one process per GPU under torch.distributed.run on
    # 127.0.0.1); rank 0 of that job prints the one JSON line on our stdout, and its exit code is ours.
    from ultragrid_amd import shard as _shard
    relaunch = _shard.self_launch_command(args.gpus, os.environ, [os.path.abspath(__file__), *sys.argv[1:]], sys.executable)
    if relaunch is not None:
        import subprocess
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // args.gpus)))   # the launcher would force 1: rank 0's CPU baseline is OpenMP
        raise SystemExit(subprocess.call(relaunch, env=env))

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} was started under a launcher with WORLD_SIZE={world}: the two must agree")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the product path has no CPU fallback)")
    if args.all_ranks_on_device0:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1 or args.force_dist:
        import torch.distributed as dist  # RCCL: used ONLY for the timing barrier + max-over-ranks, not on the data path
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world == 1:   # --force-dist under plain `python bench.py`: a one-rank group
            os.environ.setdefault("MASTER_PORT", str(29500 + os.getpid() % 2000))
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(args.dist_backend)
    coll_dev = "cuda" if args.dist_backend == "nccl" else "cpu"

    from ultragrid_amd import codec, lib
    lib.load()

    ws = setup_workload(args.workload, args.frames, args.batches, rank)
    wl, W, H, F, B, ALG_BYTES_PER_PX = ws["wl"], ws["W"], ws["H"], ws["F"], ws["B"], ws["bpp"]
    out_name, frame_bytes, out_bytes, launch, stream_bytes, host = ws["out_name"], ws["frame_bytes"], ws["out_bytes"], ws["launch"], ws["stream_bytes"], ws["host"]

    # calibrate the launches of a step: >= 50 ms of GPU work per step, so that box noise averages out and gpu_busy registers
    for b in range(B):
        launch(b)
    torch.cuda.synchronize()
    L = args.launches_per_step
    if L <= 0:
        # the estimate is taken at the clocks the timed steps will run at: ~0.2 s of launches first (a cold GPU is ~20 % slower for the
        # first tens of milliseconds), then 64 launches per batch timed; aim at 60 ms so that a step stays above 50
        import time as _t
        t_ramp = _t.perf_counter()
        while _t.perf_counter() - t_ramp < 0.2:
            for i in range(8 * B):
                launch(i % B)
            torch.cuda.synchronize()
        c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        c0.record()
        for i in range(64 * B):
            launch(i % B)
        c1.record()
        torch.cuda.synchronize()
        est = c0.elapsed_time(c1) / (64 * B)
        L = max(B, int(np.ceil(60.0 / max(est, 1e-3) / B)) * B)
    from ultragrid_amd import shard
    L = shard.agree_max(L, dist, coll_dev)   # same step on every rank

    def step():
        for i in range(L):
            launch(i % B)

    for _ in range(args.warmup):
        step()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    count = [0]

    def timed_step():
        if count[0] == 0:
            ev0.record()              # same stream the kernel is launched on (torch current stream)
        step()
        count[0] += 1
        if count[0] == args.steps:
            ev1.record()

    # barrier + synchronize on both sides of exactly K steps, MAX over ranks (ultragrid_amd/shard.py)
    wall = shard.timed_steps(timed_step, args.steps, torch.cuda.synchronize, dist, device=coll_dev)
    kern_ms = ev0.elapsed_time(ev1) / (args.steps * L)   # average launch duration (back-to-back launches on one stream)
    if rank == 0 and args.dump_outputs:
        dump_outputs(ws, L, args.dump_outputs)

    # ---- additive legs (--full), all after the timed region ----
    parity = None
    if args.full and rank == 0 and not args.no_parity_check and out_name in ("DXT5", "DXT1"):
        parity = parity_check(ws)
    ws.clear()
    launch = None   # (with it go the resident batches: the closure held them)
    torch.cuda.empty_cache()
    configs = None
    if args.full and world == 1 and not args.no_configs and args.workload == "4k-uyvy":   # the default N = 1 line only: at N > 1 nothing is added to what the ranks wait for
        configs = other_configs(rank, args.configs_seconds)

    e2e = None
    if args.full and not args.no_e2e and out_name in ("DXT5", "DXT1"):
        torch.cuda.empty_cache()
        # 8k-uyvy = the north star's literal target configuration (>= 60 fps 8K UYVY -> DXT5-YCoCg on one MI355X)
        e2e = e2e_leg(["8k-uyvy", "8k-v210", "4k-uyvy"], rank, dist, coll_dev, args.e2e_seconds)

    if rank == 0:
        px_per_launch = F * W * H
        px_per_step = px_per_launch * L * world
        value = px_per_step * args.steps / wall / 1e6
        achieved = ALG_BYTES_PER_PX * px_per_launch / (kern_ms * 1e-3) / 1e9
        read_bpp = {"UYVY": 2.0, "v210": 16 / 6, "RGB": 3.0}[wl["fmt"]]
        pmc_key = {"4k-uyvy": f"uyvy_dxt5_4k_x{F}", "8k-v210": f"v210_dxt5_8k_x{F}", "1080p-rgb-dxt1": f"rgb_dxt1_1080p_x{F}",
                   "4k-uyvy-jpeg420": f"uyvy_jpeg420_4k_x{F}", "4k-uyvy-jpeg-encode": f"uyvy_jpeg_encode_4k_x{F}"}.get(args.workload)
        pmc = load_pmc(pmc_key)
        roof = {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": pmc.get("traffic"), "traffic_source": pmc.get("source"),
                "kernel": ("uyvy_jpeg_fast_batch_kernel<420>" if out_name == "JPEG420" else "jpeg_code_kernel<3,420> + jpeg_gather_kernel (one call)" if out_name == "JPEGENC"
                           else f"dxt_encode_kernel<{wl['fmt']},{'DXT5_YCOCG' if out_name == 'DXT5' else 'DXT1'}>"),
                "ms_per_launch": round(kern_ms, 5), "launches_timed": args.steps * L,
                "algorithmic_bytes_per_launch": int(ALG_BYTES_PER_PX * px_per_launch),
                "algorithmic_bytes_per_px": round(ALG_BYTES_PER_PX, 4)}
        if out_name == "JPEGENC":
            roof["bound"] = "valu"
            roof["algorithmic_bytes_per_launch"] = int(2 * px_per_launch + stream_bytes[0])
            roof["achieved"] = round(roof["algorithmic_bytes_per_launch"] / (kern_ms * 1e-3) / 1e9, 1)
            roof["frac"] = round(roof["achieved"] / HBM_PEAK_GBS, 4)
            roof["us_per_frame"] = round(kern_ms * 1e3 / F, 2)
            ipw = pmc.get("valu_instr_per_wave")
            roof["note"] = ("the whole encoder per call of F frames, the call's own synchronisation included (ms_per_launch = time per call); algorithmic bytes = 2 B/px in + "
                            f"the stream bytes out; VALU-bound (DESIGN.md 4.5): {ipw if ipw else '~1 800'} instructions per wave of 64 blocks in jpeg_code_kernel, half of them the "
                            "forward DCT + quantiser; `traffic` = that kernel's HBM bytes per launch (the gather kernel moves the stream once more)")
        elif out_name != "JPEG420":
            # The DXT encoders are VALU-issue bound, not HBM bound: `frac` above stays the contract's
            # algorithmic-bytes / 8 TB/s figure; `hbm_read_frac` is the north star's own definition (input bytes only);
            # `valu_frac` = wave-instructions issued per second / (256 CU x 2 wave-instr/clk x 2.4 GHz).
            units = (W // 4 + (3 if wl["fmt"] == "v210" else 1) * 64 - 1) // ((3 if wl["fmt"] == "v210" else 1) * 64)
            waves = F * units * (H // 4)
            roof["bound"] = "valu"
            roof["hbm_read_frac"] = round(read_bpp * px_per_launch / (kern_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
            ipw = pmc.get("valu_instr_per_wave")
            roof["valu"] = {"instr_per_wave": ipw, "waves_per_launch": waves, "peak_wave_instr_per_s": VALU_PEAK,
                            "peak_def": "256 CU x 2 wave64 VALU instr / clk / CU x 2.4 GHz", "source": pmc.get("source")}
            if ipw:
                rate = ipw * waves / (kern_ms * 1e-3)
                roof["valu"]["wave_instr_per_s"] = round(rate, 0)
                roof["valu_frac"] = round(rate / VALU_PEAK, 4)
                roof["valu"]["measured_peak_wave_instr_per_s"] = VALU_MEASURED_PEAK
                roof["valu"]["measured_peak_def"] = ("256 CU x 1.492 wave64 v_add_f32 / clk / CU x 2.4 GHz: what a dependent-free full-rate fp32 stream issues on this chip "
                                                     "(profiles/valu_microbench_mi355x.txt; half-rate classes issue 0.95-0.97)")
                roof["valu"]["frac_of_measured_peak"] = round(rate / VALU_MEASURED_PEAK, 4)
            ratio = f"{pmc['traffic'] / (ALG_BYTES_PER_PX * px_per_launch):.3f}x" if pmc.get("traffic") else "not measured for this workload"
            roof["note"] = ("VALU-issue-bound kernel: the bit-exactness contract (every shader operation one separately rounded fp32 operation, no FMA) "
                            f"fixes ~65 VALU instructions per pixel against 3 B/px; HBM traffic / algorithmic bytes = {ratio} (DESIGN.md 4.1)")
        else:
            ratio = f"{pmc['traffic'] / (ALG_BYTES_PER_PX * px_per_launch):.3f}x" if pmc.get("traffic") else "not measured"
            roof["note"] = f"HBM-bound kernel (DESIGN.md 4.3); HBM traffic / algorithmic bytes = {ratio}"
        if out_name == "JPEGENC":
            out_bytes = stream_bytes[0] // F   # (average stream of the last call)
        out = {
            "metric": {"4k-uyvy": "Mpixels/s encode (UYVY->DXT5-YCoCg, 4K)", "8k-v210": "Mpixels/s encode (v210->DXT5-YCoCg, 8K)",
                       "1080p-rgb-dxt1": "Mpixels/s encode (RGB->DXT1, 1080p)",
                       "4k-uyvy-jpeg420": "Mpixels/s (UYVY->4:2:0->FDCT+quantise, 4K)",
                       "4k-uyvy-jpeg-encode": "Mpixels/s (UYVY->JPEG 4:2:0 q75 stream, 4K)"}[args.workload],
            "value": round(value, 1), "unit": "Mpixels/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(wall / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": wl["name"],
                       "launches_per_step": L, "frames_per_launch": F, "resident_batches": B, "frame_bytes_in": frame_bytes, "frame_bytes_out": out_bytes,
                       "input": ("S1 uniform random bytes" if wl["fmt"] == "RGB" else "S2 legal-range video noise") + f", {B * F} distinct frames resident in HBM",
                       "fps": round(value * 1e6 / (W * H), 1), "ties": "even (library default, pinned to the executed reference shaders)",
                       "parallelism": f"frames sharded over {world} GPU(s), no collective"},
            "roofline": roof,
        }
        if parity is not None:
            out["parity_check"] = parity
        if configs is not None:
            out["configs"] = configs
        if e2e is not None:
            out["e2e"] = e2e
        if dist is not None:
            out["config"]["dist"] = {"backend": args.dist_backend + (" (RCCL)" if args.dist_backend == "nccl" else ""), "world": world,
                                     "collectives": "barrier + all_reduce(MAX) around the timed steps, all_reduce(MAX) of the step size, all_gather of per-rank "
                                                    "e2e rates; on " + coll_dev + " tensors; never frame data"}
        if args.full and not args.no_cpu_baseline and out_name not in ("JPEG420", "JPEGENC"):   # rank 0, at every world size (the other ranks wait in destroy_process_group)
            out["cpu_baseline"] = cpu_baseline(host[0], wl["fmt"], W, H, out=out_name)
            try:
                ref = cpu_reference(wl["fmt"], W, H)
            except Exception as e:   # the compiled reference is optional equipment
                ref = None
                print(f"bench.py: cpu_reference skipped: {e}", file=sys.stderr, flush=True)
            if ref is not None:
                out["cpu_reference"] = ref
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
