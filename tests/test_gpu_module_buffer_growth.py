"""GPU: the buffers of a module state (mi355x_buf_reserve, module/mi355x_gpu_state.h) that grow, are kept, and grow again.  Each case is ONE
harness run that sends the sizes small, large, small, larger (or the largest once more) through ONE state of a *_mi355x module and of the
reference's CPU module of the same name: the reserve call of the first frame allocates, the third finds a larger buffer in hand and keeps it,
the others grow or keep.  Per frame: what came back, its description and its bytes equal the reference module's, the bytes equal the
restatement (tests/pixel_filter_restatement.py, tests/compose_restatement.py), 0 bytes differing, nothing written behind a buffer (pad=0).
Every size is one the reference itself handles inside its buffers: run alone on the CPU, its names answer these frames with pad=0 and no refusal."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import compose_restatement as crs  # noqa: E402
import make_compose_golden as cgen  # noqa: E402
import make_pixel_filter_golden as pgen  # noqa: E402
import pixel_filter_restatement as prs  # noqa: E402

pytestmark = pytest.mark.gpu


def uyvy_frames(sizes, seed):
    rng = np.random.default_rng(seed)
    return [(w, h, np.frombuffer(rng.bytes(crs.linesize("UYVY", w) * h), np.uint8)) for w, h in sizes]


def desc(x):
    return {k: v for k, v in x.items() if k != "out"}


@pytest.mark.skipif(not os.path.exists(pgen.HARNESS), reason="oracle/_ref/ug_cfilter_harness not built (no reference tree)")
@pytest.mark.parametrize("mode", ["cf", "pp"])
def test_flip_through_one_state_small_large_small_larger(tmp_path, mode):
    frames = uyvy_frames([(2, 1), (64, 8), (2, 1), (64, 16)], 31)
    _, res, rc, log = pgen.run_harness(pgen.HARNESS, "flip+flip_mi355x", "-", "UYVY", mode, frames, str(tmp_path))
    assert rc == 0 and len(res["flip"]) == len(res["flip_mi355x"]) == len(frames), log
    for (w, h, data), r, o in zip(frames, res["flip"], res["flip_mi355x"]):
        assert desc(r) == desc(o), (desc(r), desc(o))
        assert o["status"] == ("new" if mode == "cf" else "true") and (o["w"], o["h"], o["codec"], o["data_len"]) == (w, h, "UYVY", data.size)
        want = prs.run_filter("flip", "", "UYVY", w, h, data)["out"]
        assert int(np.count_nonzero(o["out"] != r["out"])) == 0 and int(np.count_nonzero(o["out"] != want)) == 0


def compose_case(tmp_path, name, options, frames, rets):
    res, rc, log = cgen.run_harness(cgen.HARNESS, f"{name}+{name}_mi355x", options, "UYVY", "pp", 1, frames, str(tmp_path))
    assert rc == 0 and len(res[name]) == len(res[name + "_mi355x"]) == len(frames), log
    module = crs.Module(name, options, "UYVY")
    for i, ((w, h, data), r, o) in enumerate(zip(frames, res[name], res[name + "_mi355x"])):
        want = module.frame(w, h, [data])
        assert desc(r) == desc(o), (i, desc(r), desc(o))
        assert o["pad"] == 0 and r["pad"] == 0, (i, o["pad"], r["pad"])
        assert o["ret"] == want["ret"] == rets[i], (i, o["ret"], want["ret"])
        assert (o["w"], o["h"], o["tile_count"], o["interlacing"], o["fps"], o["codec"]) == (want["w"], want["h"], 1, want["interlacing"], want["fps"], "UYVY")
        assert ("out" in o) == ("out" in r) == ("out" in want), i
        if "out" in want:
            assert o["out"].size == r["out"].size == want["out"].size
            assert int(np.count_nonzero(o["out"] != r["out"])) == 0 and int(np.count_nonzero(o["out"] != want["out"])) == 0, i


@pytest.mark.skipif(not os.path.exists(cgen.HARNESS), reason="oracle/_ref/ug_compose_harness not built (no reference tree)")
def test_crop_through_one_state_small_large_small_large(tmp_path):
    """(the fourth frame repeats the largest size: the last call keeps what it has)"""
    compose_case(tmp_path, "crop", "width=4:height=2", uyvy_frames([(8, 4), (64, 16), (8, 4), (64, 16)], 32), ["true"] * 4)


@pytest.mark.skipif(not os.path.exists(cgen.HARNESS), reason="oracle/_ref/ug_compose_harness not built (no reference tree)")
def test_interlace_pairs_through_one_state_small_large_small(tmp_path):
    """two frames of each size -- the path with two device inputs: false for the first frame of a pair, the woven frame for the second"""
    compose_case(tmp_path, "interlace", "-", uyvy_frames([(10, 6), (10, 6), (32, 8), (32, 8), (10, 6), (10, 6)], 33), ["false", "true"] * 3)
