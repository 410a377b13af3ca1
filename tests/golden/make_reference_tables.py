#!/usr/bin/env python3
"""The (input, output) format pairs of the reference's conversion tables -- decoders[] of src/pixfmt_conv.c and the two tables of
src/libavcodec/{to,from}_lavc_vid_conv.c -- read from its source, and tests/golden/reference_tables.json, the same pairs committed so that
tests/test_gpu_pixfmt_ext.py and tests/test_lavc_conv.py check them where the reference tree is absent.
Regenerate where the reference tree exists:  python tests/golden/make_reference_tables.py <reference tree>"""
import json
import os
import re
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_tables.json")


def from_source(src: str):
    """{table: [[from, to], ...]} parsed from the reference's src/ directory, or None where it is absent"""
    if not os.path.exists(os.path.join(src, "pixfmt_conv.c")) or not os.path.isdir(os.path.join(src, "libavcodec")):
        return None
    txt = open(os.path.join(src, "pixfmt_conv.c")).read()
    tab = txt[txt.index("static const struct decoder_item decoders[]"):]
    tab = tab[: tab.index("};")]
    decoders = [[i, o] for _, i, o in re.findall(r"\{ *(\w+), *(\w+), *(\w+) *\}", tab)]
    to_av = [[c, f] for c, f, _ in re.findall(r"\{ *(\w+), *AV_PIX_FMT_(\w+), *(\w+) *\}", open(os.path.join(src, "libavcodec", "to_lavc_vid_conv.c")).read())
             if c != "VIDEO_CODEC_NONE"]
    from_av = [[f, c] for f, c, _, _ in re.findall(r"\{ *AV_PIX_FMT_(\w+), *(\w+),\s*(\w+),\s*(\w+) *\}",
                                                   open(os.path.join(src, "libavcodec", "from_lavc_vid_conv.c")).read())]
    return {"pixfmt_decoders": decoders, "to_lavc": to_av, "from_lavc": from_av}


def tables(src: str) -> dict:
    """the committed pairs; where the reference's src/ directory exists, they must be what its source says"""
    committed = json.load(open(GOLDEN))
    live = from_source(src)
    assert live is None or live == committed, "tests/golden/reference_tables.json differs from the reference source: regenerate it"
    return committed


if __name__ == "__main__":
    t = from_source(os.path.join(sys.argv[1], "src"))
    assert t is not None, "usage: make_reference_tables.py <reference tree>"
    with open(GOLDEN, "w") as f:
        json.dump(t, f)
        f.write("\n")
    print({k: len(v) for k, v in t.items()})
