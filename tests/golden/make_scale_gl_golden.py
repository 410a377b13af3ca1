#!/usr/bin/env python3
"""Generate tests/golden/scale_gl_ref.npz: UltraGrid's `scale` video postprocessor (src/vo_postprocess/scale.c) executed on Mesa llvmpipe.

scale.c is compiled UNMODIFIED in a temporary directory against the reference's headers, with tools/scale_gl_shim/GL/glew.h in front of
them, and linked with tools/scale_gl_run.c (a DRI-swrast context, the module's registration, the frame helpers it calls).  The runner
drives init("<out_w>:<out_h>") -> reconfigure -> getf -> postprocess -> postprocess(NULL) -> get_out_desc -> done on one frame.

Run where the reference tree and Mesa's swrast_dri.so exist:
    python tests/golden/make_scale_gl_golden.py [out.npz]

Arrays, per case key:
  in_<key>     the input tile(s): tiles x vc_get_linesize(w) * h bytes
  gl_<key>     the output tile as the module left it: req_pitch * out_h bytes, pre-filled with 0xA5
  meta_<key>   int32 [uyvy, w, h, merged, out_w, out_h, req_pitch, tiles, postprocess ret, postprocess(NULL) ret, desc w, desc h,
               desc interlacing, desc tile_count, display mode, bytes the module wrote into output slot 1 (tiles > 1)]
"""
import os
import subprocess
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("UG_REFERENCE", "/root/reference")
SCALE_C = os.path.join(REF, "src", "vo_postprocess", "scale.c")

# (codec, w, h, merged, out_w, out_h, extra pitch bytes, tiles)
CASES = [
    ("RGBA", 64, 32, 0, 32, 16, 0, 1),     # down by 2
    ("RGBA", 64, 32, 0, 37, 23, 0, 1),     # down, non-integer ratios
    ("RGBA", 17, 9, 0, 40, 29, 0, 1),      # up, non-integer ratios
    ("RGBA", 48, 40, 0, 7, 5, 0, 1),       # down by more than 2 (still 2 x 2 texels per sample)
    ("RGBA", 5, 3, 0, 1, 1, 0, 1),         # 1 x 1 output
    ("RGBA", 5, 3, 0, 2, 1, 0, 1),         # 2 x 1 output
    ("RGBA", 1, 1, 0, 9, 4, 0, 1),         # 1 x 1 input
    ("RGBA", 64, 32, 0, 37, 23, 20, 1),    # req_pitch != line size (scale.c:294-303)
    ("RGBA", 64, 36, 0, 192, 108, 0, 1),  # up by 3
    ("RGBA", 200, 120, 0, 71, 43, 0, 1),   # larger non-integer ratio
    ("RGBA", 300, 20, 0, 107, 7, 0, 1),    # llvmpipe's fp32 coordinates land on the other side of a rounding tie (1 LSB)
    ("UYVY", 64, 16, 0, 40, 10, 0, 1),
    ("UYVY", 96, 20, 0, 50, 13, 0, 1),
    ("UYVY", 20, 6, 0, 2, 1, 0, 1),        # one texel out
    ("UYVY", 96, 20, 0, 50, 13, 36, 1),
    ("RGBA", 64, 32, 1, 48, 20, 0, 1),     # INTERLACED_MERGED
    ("UYVY", 64, 32, 1, 48, 20, 0, 1),
    ("UYVY", 40, 12, 1, 90, 30, 8, 1),
    # slips of the reference
    ("UYVY", 33, 9, 0, 50, 13, 0, 1),      # odd input width: rows shear on upload
    ("UYVY", 64, 16, 0, 41, 10, 0, 1),     # odd output width: rows shear on read-back
    ("UYVY", 64, 16, 0, 41, 10, 12, 1),    # ... and through the temporary buffer
    ("RGBA", 64, 33, 1, 48, 20, 0, 1),     # odd input height, merged: last line dropped
    ("RGBA", 64, 32, 1, 48, 21, 0, 1),     # odd output height, merged: last line not written
    ("RGBA", 32, 16, 0, 24, 12, 0, 2),     # tile_count 2: the loop writes out->tiles[1]
]


def build(d: str) -> str:
    obj, exe = os.path.join(d, "scale.o"), os.path.join(d, "scale_gl_run")
    inc = ["-I", os.path.join(ROOT, "tools", "scale_gl_shim"), "-I", os.path.join(REF, "src")]
    subprocess.check_call(["gcc", "-std=gnu2x", "-O1", "-D_GNU_SOURCE"] + inc + ["-c", SCALE_C, "-o", obj])
    subprocess.check_call(["gcc", "-std=gnu2x", "-O1", "-D_GNU_SOURCE"] + inc + [os.path.join(ROOT, "tools", "scale_gl_run.c"), obj, "-ldl", "-o", exe])
    return exe


def linesize(codec, w):
    return (w + 1) // 2 * 4 if codec == "UYVY" else 4 * w


def run(exe, d, codec, w, h, merged, ow, oh, pitch, tiles, src):
    a, b = os.path.join(d, "in.raw"), os.path.join(d, "out.raw")
    src.tofile(a)
    r = subprocess.run([exe, codec, str(w), str(h), "merged" if merged else "prog", str(ow), str(oh), str(pitch), a, b, str(tiles)],
                       capture_output=True, text=True, check=True)
    f = r.stdout.split()
    assert f[0] == "out" and "llvmpipe" in r.stdout, r.stdout
    kv = dict(x.split("=", 1) for x in f[7:] if "=" in x)
    meta = [int(f[1]), int(f[2]), int(f[4]), int(f[5]), int(f[6]), int(kv["spare_written"])]
    return np.fromfile(b, np.uint8), [int(kv["ret"]), int(kv["null"])] + meta


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "scale_gl_ref.npz")
    arrays = {}
    with tempfile.TemporaryDirectory() as d:
        exe = build(d)
        for codec, w, h, merged, ow, oh, extra, tiles in CASES:
            key = f"{codec}_{w}x{h}{'m' if merged else 'p'}_{ow}x{oh}_p{extra}_t{tiles}"
            rng = np.random.default_rng(zlib.crc32(key.encode()))
            src = rng.integers(0, 256, tiles * linesize(codec, w) * h, dtype=np.uint8)
            pitch = linesize(codec, ow) + extra
            gl, meta = run(exe, d, codec, w, h, merged, ow, oh, pitch, tiles, src)
            arrays["in_" + key] = src
            arrays["gl_" + key] = gl
            arrays["meta_" + key] = np.array([codec == "UYVY", w, h, merged, ow, oh, pitch, tiles] + meta, np.int32)
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
