"""GPU: the *_mi355x colour / mirror modules through the reference's own capture_filter.c and vo_postprocess.c (oracle/_ref/ug_cfilter_harness),
as capture filters and as postprocessors, each against the reference's CPU module of the same name IN THE SAME RUN -- the same frames through
`matrix2` and `matrix2_mi355x` in one process -- and against the restatement: every case of the fixture's list, the sizes of a codec one after the
other through one state (a format change between frames), what comes back for a codec a module does not take (NULL, the same frame, matrix2's
unwritten frame) and the returned descriptions.  0 bytes differing.  Left out of the comparison with the reference, as conditions (DESIGN.md
4.12): unchecked conversions whose exact value is outside the output type, and gamma's last len % cpus elements (cpus: the count the harness
prints); against the restatement nothing is left out."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_pixel_filter_golden as gen  # noqa: E402
import pixel_filter_restatement as rs  # noqa: E402

pytestmark = pytest.mark.gpu
HARNESS = gen.HARNESS
GOLD = np.load(os.path.join(HERE, "golden", "pixel_filter_ref.npz"))
META = json.loads(str(GOLD["meta"]))
needs_harness = pytest.mark.skipif(not os.path.exists(HARNESS), reason="oracle/_ref/ug_cfilter_harness not built (no reference tree)")


def groups():
    """the fixture's cases by (module, options, codec): the sizes of a group go through ONE state, one after the other"""
    g = {}
    for m in META:
        g.setdefault((m["name"], m["options"], m["codec"]), []).append(m)
    return g


GROUPS = groups()
GIDS = {k: f"{k[0]}-{k[2]}-{i}" for i, k in enumerate(GROUPS)}
# as postprocessors: one group per module and codec it takes (the wrapper's get_out_desc asserts on a NULL frame: the refusals are capture-filter cases)
PP = {}
for key, ms in GROUPS.items():
    if ms[0]["status"] != "null":
        PP.setdefault((key[0], key[2], "no-bound-check" in key[1]), key)
PP_KEYS = list(PP.values())


def check_group(tmp, key, mode):
    name, options, codec = key
    ms = GROUPS[key]
    frames = [(m["w"], m["h"], GOLD[m["input"]]) for m in ms]
    ours = name + "_mi355x"
    refused = ms[0]["status"] == "null"
    if refused:  # a NULL ends a run: one process each
        cpus, res, rc, log = gen.run_harness(HARNESS, name, options, codec, mode, frames[:1], str(tmp))
        _, res2, rc2, log2 = gen.run_harness(HARNESS, ours, options, codec, mode, frames[:1], str(tmp))
        assert (rc, rc2) == (4, 4), (log, log2)
        res.update(res2)
    else:
        cpus, res, rc, log = gen.run_harness(HARNESS, name + "+" + ours, options, codec, mode, frames, str(tmp))
        assert rc == 0, log
    assert cpus and len(res[name]) == len(res[ours]) == (1 if refused else len(frames)), log
    for m, (w, h, data), r, o in zip(ms, frames, res[name], res[ours]):
        desc = lambda x: {k: v for k, v in x.items() if k != "out"}  # noqa: E731
        assert desc(r) == desc(o), (desc(r), desc(o))                 # what came back, and its description
        want = rs.run_filter(name, "" if options == "-" else options, codec, w, h, data)
        new = "new" if mode == "cf" else "true"
        assert o["status"] == {"unwritten": new, "new": new, "same": "same" if mode == "cf" else "true", "null": "null"}[want["status"]]
        if want["status"] in ("null", "unwritten"):
            continue
        if want["status"] == "same":
            if mode == "cf":
                assert np.array_equal(o["out"], data) and np.array_equal(r["out"], data)
            else:  # the wrapper hands nothing over: the output frame keeps its fill, with both
                assert (o["out"] == 0xA5).all() and (r["out"] == 0xA5).all()
            continue
        assert (o["codec"], o["data_len"]) == (want["codec"], want["out"].size)
        assert int(np.count_nonzero(o["out"] != want["out"])) == 0   # against the restatement: nothing left out
        left = gen.left_out(want, r["out"], cpus, name, codec)
        assert left.mean() < 0.05, (cpus, left.mean())
        assert int(np.count_nonzero((o["out"] != r["out"]) & ~left)) == 0


@needs_harness
@pytest.mark.parametrize("key", list(GROUPS), ids=[GIDS[k] for k in GROUPS])
def test_capture_filter_against_the_reference_module_in_the_same_run(tmp_path, key):
    check_group(tmp_path, key, "cf")


@needs_harness
@pytest.mark.parametrize("key", PP_KEYS, ids=[GIDS[k] for k in PP_KEYS])
def test_postprocessor_against_the_reference_module_in_the_same_run(tmp_path, key):
    check_group(tmp_path, key, "pp")


@needs_harness
def test_option_strings_are_refused_as_the_reference_refuses_them(tmp_path):
    """init's return: too few numbers, a wrong depth, an option where none is taken -- with both modules; gamma <= 0 with ours only (a stated deviation)"""
    frame = [(2, 1, np.zeros(4, np.uint8))]
    for name, options, codec in (("matrix", "1:2:3", "UYVY"), ("matrix2", "1:0:0:0:1:0:0:0", "UYVY"), ("gamma", "2.2:12", "RGB"), ("grayscale", "x", "UYVY"),
                                 ("mirror", "1", "UYVY"), ("flip", "up", "UYVY")):
        for n in (name, name + "_mi355x"):
            _, res, rc, log = gen.run_harness(HARNESS, n, options, codec, "cf", frame, str(tmp_path))
            assert rc == 2 and not res, (n, options, rc, log)
    _, res, rc, log = gen.run_harness(HARNESS, "gamma_mi355x", "0", "RGB", "cf", [(2, 1, np.zeros(6, np.uint8))], str(tmp_path))
    assert rc == 2 and not res, log
