#!/usr/bin/env python3
"""Writes tests/golden/pixel_filter_ref.npz: the reference's six colour / mirror capture filters (matrix, matrix2, gamma, grayscale, mirror, flip,
compiled unmodified into oracle/_ref/ug_cfilter_harness) run on the CPU over the cases below.  The fixture holds data only: per case the option
string, codec and size, the input bytes, what the module returned (a new frame, the same frame, NULL) and the output bytes and codec -- and the
CPU count of the machine that generated it (the number of slices of gamma's apply_lut, gamma.cpp:132-138).

The modules run as capture filters with UG_CFILTER_PAD=1 (ug_cfilter_harness.c): the output frame they malloc is pre-filled with 0xA5, so the tail
gamma leaves unwritten is recognisable, and is three times as long as asked for, which is what matrix2's v210 path writes (matrix2.c:239-241).

Two conditions on the comparison (tests/test_pixel_filter.py applies them; this script prints the share of bytes each leaves out and fails
above 5 % per case):
  1. matrix ... no-bound-check and matrix2: elements whose exact value lies outside the output type are undefined in the reference;
  2. gamma: the last len % cpus elements are not written by the reference.
    python3 tests/golden/make_pixel_filter_golden.py
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import pixel_filter_restatement as rs  # noqa: E402

HARNESS = os.path.join(ROOT, "oracle", "_ref", "ug_cfilter_harness")
OUT = os.path.join(HERE, "pixel_filter_ref.npz")
CAP = 0.05

RANDOM_M = "1.31:-0.62:0.18:-1.94:0.77:1.05:0.4:1.66:-1.23"            # |m| <= 2
NEGATIVE_M = "-1:-0.5:-0.25:-2:-1:-0.125:-0.75:-1.5:-0.0625"          # everything clamps to 0
IDENTITY_M = "1:0:0:0:1:0:0:0:1"
YUV_TO_RGB_M = "1.0:0.02:0.9:1.0:-0.2:-0.4:1.0:1.1:0.01"             # no-bound-check on UYVY: video-range input stays mostly inside 0..255
MIX_M = "0.7:0.25:-0.04:0.2:0.7:0.08:-0.03:0.3:0.71"                  # no-bound-check on RGB / RG48: rows sum to about 1, small negative weights
MATRIX2_M = "1.02:0.03:-0.04:0.01:0.97:0.05:-0.02:0.06:1.01"


def cases():
    """(name, options, codec, w, h, input kind)"""
    out = []
    hs = {2: 1, 6: 2, 34: 3, 130: 5, 1: 1, 5: 4, 43: 3, 3: 2, 21: 5, 7: 4, 48: 2, 96: 3}
    uyvy, rgb, rg48, y416, v210 = (2, 6, 34, 130), (1, 5, 43), (1, 3, 21), (1, 7), (48, 96)
    for codec, widths in (("UYVY", uyvy), ("RGB", rgb), ("RG48", rg48)):
        for w in widths:
            out.append(("matrix", RANDOM_M, codec, w, hs[w], "random"))
        w = widths[-1]
        out.append(("matrix", IDENTITY_M, codec, w, hs[w], "random"))
        out.append(("matrix", NEGATIVE_M, codec, w, hs[w], "random"))
        out.append(("matrix", (YUV_TO_RGB_M if codec == "UYVY" else MIX_M) + ":no-bound-check", codec, w, hs[w], "video"))
        out.append(("matrix", RANDOM_M + ":no-bounds-check", codec, widths[1], hs[widths[1]], "random"))  # the help text's spelling: an excess initializer, bounds stay checked
    for codec, widths in (("UYVY", uyvy), ("Y416", y416), ("v210", v210)):
        for w in widths:
            out.append(("matrix2", "y601_to_y709", codec, w, hs[w], "video"))
        out.append(("matrix2", MATRIX2_M, codec, widths[-1], hs[widths[-1]], "video"))
    for g in ("0.45", "1.0", "2.2"):
        for depth in ("", ":8", ":16"):
            for codec in ("RGB", "RG48"):
                w, h = (56, 65) if (g, depth, codec) == ("2.2", "", "RGB") else (65, 53)  # 56 * 65 * 3 = 840 * 13: divisible by every n <= 8; 65 * 53 * 3 = 10335 is odd: a tail wherever there are two CPUs
                out.append(("gamma", g + depth, codec, w, h, "ramp"))
    for w in uyvy:
        out += [("grayscale", "-", "UYVY", w, hs[w], "random"), ("mirror", "-", "UYVY", w, hs[w], "random"), ("flip", "-", "UYVY", w, hs[w], "random")]
    out += [("flip", "-", "RGB", 43, 3, "random"), ("flip", "-", "RG48", 21, 5, "random"), ("flip", "-", "v210", 96, 3, "random")]
    # a codec each module does not take
    out += [("matrix", RANDOM_M, "RGBA", 6, 2, "random"), ("matrix2", "y601_to_y709", "RGB", 5, 4, "random"), ("gamma", "2.2", "UYVY", 6, 2, "random"),
            ("grayscale", "-", "RGB", 5, 4, "random"), ("mirror", "-", "RGBA", 6, 2, "random"), ("flip", "-", "R10k", 6, 2, "random")]
    return out


def make_input(codec, w, h, kind, rng):
    n = rs.linesize(codec, w) * h
    if kind == "ramp":  # every 8-bit value, a spread of 16-bit ones; compresses
        if codec == "RG48":
            return ((np.arange(n // 2, dtype=np.uint64) * 65535 // (n // 2 - 1) + rng.integers(0, 3, n // 2).astype(np.uint64)).clip(0, 65535)).astype(np.uint16).view(np.uint8)
        return (np.arange(n) * 255 // (n - 1) + rng.integers(0, 2, n)).clip(0, 255).astype(np.uint8)
    if kind == "random":
        return np.frombuffer(rng.bytes(n), np.uint8).copy()
    # video range: luma 16..235, chroma around the middle
    if codec == "UYVY":
        a = rng.integers(16, 236, n).astype(np.uint8)
        a[0::2] = rng.integers(96, 161, a[0::2].size)
        return a
    if codec == "RGB":
        return rng.integers(16, 236, n).astype(np.uint8)
    if codec == "RG48":
        return rng.integers(16 << 8, 236 << 8, n // 2).astype(np.uint16).view(np.uint8)
    if codec == "Y416":
        a = rng.integers(16 << 8, 236 << 8, n // 2).astype(np.uint16).reshape(-1, 4)
        a[:, 0] = rng.integers(96 << 8, 161 << 8, a.shape[0])
        a[:, 2] = rng.integers(96 << 8, 161 << 8, a.shape[0])
        return a.reshape(-1).view(np.uint8)
    assert codec == "v210"
    y, c = lambda k: rng.integers(64, 941, k).astype(np.uint32), lambda k: rng.integers(384, 641, k).astype(np.uint32)  # noqa: E731
    g = n // 16
    words = np.stack([c(g) | y(g) << 10 | c(g) << 20, y(g) | c(g) << 10 | y(g) << 20, c(g) | y(g) << 10 | c(g) << 20, y(g) | c(g) << 10 | y(g) << 20], axis=1)
    return words.astype(np.uint32).reshape(-1).view(np.uint8)


def run_harness(harness, names, options, codec, mode, frames, tmp, env_extra=None, timeout=120):
    """frames: [(w, h, bytes)] -> (cpus, {name: [dict(status, w, h, codec, data_len, out)]}, returncode, stdout)"""
    args = [harness, "run", names, options, codec, mode, os.path.join(tmp, "out"), "1"]
    for i, (w, h, data) in enumerate(frames):
        path = os.path.join(tmp, f"in{i}.raw")
        np.asarray(data, np.uint8).tofile(path)
        args += [str(w), str(h), path]
    env = dict(os.environ, UG_CFILTER_PAD="1", **(env_extra or {}))
    p = subprocess.run(args, capture_output=True, text=True, env=env, timeout=timeout)
    cpus, res = None, {}
    for line in p.stdout.splitlines():
        t = line.split()
        if line.startswith("cpus="):
            cpus = int(line[5:])
        elif len(t) == 11 and t[1] == "frame":
            status = t[10][4:]
            r = dict(status=status, w=int(t[3]), h=int(t[4]), codec=t[5], interlacing=int(t[6]), fps=float(t[7]), tile_count=int(t[8]), data_len=int(t[9]))
            path = os.path.join(tmp, f"out.{t[0]}.{t[2]}")
            if status in ("new", "same", "true"):
                r["out"] = np.fromfile(path, np.uint8)
            res.setdefault(t[0], []).append(r)
    return cpus, res, p.returncode, p.stdout + p.stderr


def left_out(r, ref_out, cpus, name, codec):
    """-> the mask over the output BYTES that the comparison with the reference leaves out (conditions 1 and 2)"""
    mask = np.zeros(ref_out.size, bool)
    if r["status"] != "new":
        return mask
    if r.get("undefined") is not None:
        mask |= np.repeat(r["undefined"], r["elem"])
    if name == "gamma":
        elem = 2 if r["codec"] == "RG48" else 1
        n = ref_out.size // elem
        tail = n % cpus
        if tail:
            mask[(n - tail) * elem:] = True
    return mask


def main():
    if not os.path.exists(HARNESS):
        raise SystemExit(f"{HARNESS} not built")
    rng = np.random.default_rng(20261017)
    meta, arrays, inputs = [], {}, {}
    cpus_seen = None
    worst = {1: 0.0, 2: 0.0}
    for k, (name, options, codec, w, h, kind) in enumerate(cases()):
        key = f"{codec}_{w}x{h}_{kind}"
        if key not in inputs:
            inputs[key] = make_input(codec, w, h, kind, rng)
            arrays["in_" + key] = inputs[key]
        data = inputs[key]
        with tempfile.TemporaryDirectory() as tmp:
            cpus, res, rc, log = run_harness(HARNESS, name, options, codec, "cf", [(w, h, data)], tmp)
        if cpus is None or name not in res:
            raise SystemExit(f"case {k} {name}:{options} {codec} {w}x{h}: harness rc={rc}\n{log}")
        cpus_seen = cpus
        ref = res[name][0]
        m = dict(name=name, options=options, codec=codec, w=w, h=h, input="in_" + key, status=ref["status"], out_codec=ref["codec"], out_w=ref["w"], out_h=ref["h"],
                 data_len=ref["data_len"])
        want = rs.run_filter(name, "" if options == "-" else options, codec, w, h, data)
        expect_status = {"unwritten": "new"}.get(want["status"], want["status"])
        assert ref["status"] == expect_status, (m, want["status"])
        if ref["status"] == "new" and want["status"] == "new":
            arrays[f"out_{k}"] = ref["out"]
            mask = left_out(want, ref["out"], cpus, name, codec)
            share = float(mask.mean())
            cond = 2 if name == "gamma" else 1
            worst[cond] = max(worst[cond], share)
            bad = int(np.count_nonzero((want["out"] != ref["out"]) & ~mask))
            print(f"case {k:3d} {name:9s} {options[:40]:40s} {codec:5s} {w:3d}x{h:<3d} left out {100 * share:5.2f} %  differing {bad}")
            if share >= CAP:
                raise SystemExit(f"case {k}: {100 * share:.2f} % of the bytes left out, the cap is {100 * CAP:.0f} %")
            if name == "gamma" and not (ref["out"][mask] == 0xA5).all():
                raise SystemExit(f"case {k}: the reference wrote into the tail")
        else:
            print(f"case {k:3d} {name:9s} {options[:40]:40s} {codec:5s} {w:3d}x{h:<3d} -> {ref['status']} ({ref['codec']})")
        meta.append(m)
    print(f"left out, worst case: condition 1 (unchecked conversions) {100 * worst[1]:.2f} %, condition 2 (gamma's tail, {cpus_seen} CPUs) {100 * worst[2]:.2f} %")
    np.savez_compressed(OUT, meta=np.array(json.dumps(meta)), cpus=np.array(cpus_seen), **arrays)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(meta)} cases")


if __name__ == "__main__":
    main()
