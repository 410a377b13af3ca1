#!/usr/bin/env python3
"""Writes tests/golden/ldgm_ref.npz from the reference's own LDGM code: its matrix generator (ldgm/matrix-gen) and its CPU coding session
(ldgm/src/ldgm-session{,-cpu}.cpp, tanner.cpp), compiled into a temporary directory with a small driver of ours and run there.

Per configuration i (k, m, c, seed -- the defaults 512/384/5 and several of src/rtp/ldgm.cpp's suggested_configurations, plus small ones):
    kmcs{i}   [k, m, c, seed]
    pcm{i}    (m, w_f) int32: the matrix as LDGM_session::set_pcMatrix reads it
    buf{i}    the buffer LDGM_session::encode_hdr_frame returns for a random frame: size header, payload, padding, parity
    rx{i}     (L, k + m) uint8: loss maps (1 = packet received whole)
    fs{i}     (L,) int32: LDGM_session_cpu::decode_frame's *frame_size for each map (0 = not every data packet known)
    dec{i}    (L, k * ps) uint8: the data region after that decode (lost packets were 0xA5 going in)

    python3 tests/golden/make_ldgm_golden.py [--ref <UltraGrid source tree>]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# our driver: gen <k> <m> <c> <seed> <matrix>  |  enc <k> <m> <c> <matrix> <frame> <out>  |  dec <k> <m> <c> <matrix> <buf> <mask> <out>
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>
#include "ldgm-session-cpu.h"
#include "../matrix-gen/matrix-generator.h"

static std::vector<char> slurp(const char *p)
{
        std::vector<char> v;
        FILE *f = fopen(p, "rb");
        if (!f) { perror(p); exit(2); }
        char b[65536];
        size_t n;
        while ((n = fread(b, 1, sizeof b, f)) > 0) v.insert(v.end(), b, b + n);
        fclose(f);
        return v;
}
static void dump(const char *p, const void *d, size_t n)
{
        FILE *f = fopen(p, "wb");
        if (!f || fwrite(d, 1, n, f) != n) { perror(p); exit(2); }
        fclose(f);
}

int main(int argc, char **argv)
{
        if (argc == 7 && !strcmp(argv[1], "gen"))
                return generate_ldgm_matrix(argv[6], atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), 0);
        if (argc < 6) return 2;
        const int k = atoi(argv[2]), m = atoi(argv[3]), c = atoi(argv[4]);
        LDGM_session_cpu s;
        s.set_params(k, m, c);
        s.set_pcMatrix(argv[5]);
        if (argc == 8 && !strcmp(argv[1], "enc")) {
                std::vector<char> fr = slurp(argv[6]);
                int out_size = 0;
                // encode_hdr_frame, the form ldgm::encode_video_frame uses (encode_frame zeroes 4 k bytes past the payload, beyond the end of
                // the buffer where the parity is shorter than that)
                char *out = s.encode_hdr_frame(fr.data(), 0, fr.data(), (int) fr.size(), &out_size);
                dump(argv[7], out, out_size);
                s.free_out_buf(out);
                return 0;
        }
        if (argc == 9 && !strcmp(argv[1], "dec")) {
                std::vector<char> buf = slurp(argv[6]), mask = slurp(argv[7]);
                const int ps = (int) buf.size() / (k + m);
                std::map<int, int> valid;
                for (int i = 0; i < k + m; ++i)
                        if (mask[i]) valid[i * ps] = ps;
                int frame_size = -1;
                s.decode_frame(buf.data(), (int) buf.size(), &frame_size, valid);
                std::vector<char> out(sizeof(int) + (size_t) k * ps);
                memcpy(out.data(), &frame_size, sizeof(int));
                memcpy(out.data() + sizeof(int), buf.data(), (size_t) k * ps);
                dump(argv[8], out.data(), out.size());
                return 0;
        }
        return 2;
}
"""

CONFIGS = [  # k, m, c, seed, payload bytes
    (512, 384, 5, 1, 512 * 12 - 4 - 100),   # the defaults (ldgm.cpp DEFAULT_K / _M / _C); padding in the last packet
    (750, 120, 5, 1, 750 * 20 - 4),         # JPEG 60, 2 %
    (1500, 450, 6, 1, 1500 * 8 - 4 - 7),    # JPEG 60, 5 %
    (1000, 500, 7, 1, 1000 * 16 - 4),       # JPEG 60, 10 % / uncompressed 9000, 10 %
    (1250, 375, 6, 1, 1250 * 4 - 4),        # JPEG 80, 5 %
    (1500, 750, 8, 1, 1500 * 12 - 4 - 333), # JPEG 80 / 90, 10 %
    (1500, 1500, 8, 1, 1500 * 4 - 4),       # uncompressed 1500, 10 %
    (64, 64, 3, 7, 64 * 36 - 4),            # the smallest k and m ldgm.cpp takes, another seed
]


def read_matrix(path):
    raw = open(path, "rb").read()
    nl = raw.index(b"\n")
    k, m, wf = (int(x) for x in raw[:nl].split())
    pcm = np.frombuffer(raw[nl + 1: nl + 1 + 4 * m * wf], dtype="<i4").reshape(m, wf).copy()
    return k, m, wf, pcm


def loss_maps(k, m, rng):
    n = k + m
    maps = []
    for p in (0.0, 0.02, 0.05, 0.12, 0.3):
        maps.append((rng.random(n) >= p).astype(np.uint8))
    b = np.ones(n, np.uint8)  # a burst in the data and a run of lost parity
    s = int(rng.integers(0, k - k // 20))
    b[s: s + k // 20] = 0
    b[k + m // 3: k + m // 3 + m // 10] = 0
    maps.append(b)
    maps.append(np.ones(n, np.uint8) * (np.arange(n) >= k).astype(np.uint8))  # every data packet lost
    return maps


def build(ref, tmp):
    drv = os.path.join(tmp, "driver.cpp")
    open(drv, "w").write(DRIVER)
    srcs = [os.path.join(ref, "ldgm", "src", f) for f in ("ldgm-session.cpp", "ldgm-session-cpu.cpp", "tanner.cpp")]
    srcs += [os.path.join(ref, "ldgm", "matrix-gen", f) for f in ("matrix-generator.cpp", "ldpc-matrix.cpp")]
    exe = os.path.join(tmp, "ldgm_driver")
    subprocess.check_call(["g++", "-std=gnu++17", "-O2", "-msse4.1", "-w", "-I", os.path.join(ref, "ldgm", "src"), drv] + srcs + ["-o", exe])
    return exe


def run(exe, *args):
    subprocess.check_call([exe] + [str(a) for a in args], stdout=subprocess.DEVNULL)


def generate(ref, configs=CONFIGS, seed=1234):
    """{name: array} as in the module docstring, computed by the reference's code"""
    rng = np.random.default_rng(seed)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(ref, tmp)
        for i, (k, m, c, sd, size) in enumerate(configs):
            mat = os.path.join(tmp, f"m{i}.bin")
            run(exe, "gen", k, m, c, sd, mat)
            kf, mf, wf, pcm = read_matrix(mat)
            assert (kf, mf) == (k, m)
            frame = rng.integers(0, 256, size, dtype=np.uint8)
            fr = os.path.join(tmp, "frame.bin")
            frame.tofile(fr)
            enc = os.path.join(tmp, "enc.bin")
            run(exe, "enc", k, m, c, mat, fr, enc)
            buf = np.fromfile(enc, np.uint8)
            ps = buf.size // (k + m)
            rx, fs, dec = [], [], []
            for mask in loss_maps(k, m, rng):
                lossy = buf.copy().reshape(k + m, ps)
                lossy[mask == 0] = 0xA5
                lb, mk, o = (os.path.join(tmp, x) for x in ("lossy.bin", "mask.bin", "dec.bin"))
                lossy.tofile(lb)
                mask.tofile(mk)
                run(exe, "dec", k, m, c, mat, lb, mk, o)
                res = np.fromfile(o, np.uint8)
                rx.append(mask)
                fs.append(int(res[:4].view("<i4")[0]))
                dec.append(res[4:])
            out[f"kmcs{i}"] = np.array([k, m, c, sd], np.int32)
            out[f"pcm{i}"] = pcm
            out[f"buf{i}"] = buf
            out[f"rx{i}"] = np.array(rx)
            out[f"fs{i}"] = np.array(fs, np.int32)
            out[f"dec{i}"] = np.array(dec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("UG_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(HERE, "ldgm_ref.npz"))
    a = ap.parse_args()
    data = generate(a.ref)
    np.savez_compressed(a.out, **data)
    print(a.out, sum(v.nbytes for v in data.values()), "bytes", file=sys.stderr)


if __name__ == "__main__":
    main()
