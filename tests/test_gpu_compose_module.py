"""GPU: the *_mi355x composition modules through the reference's own vo_postprocess.c and capture_filter.c (oracle/_ref/ug_compose_harness), each
beside the reference's CPU module of the same name IN THE SAME RUN -- the same frames through `crop` and `crop_mi355x` in one process -- over the
fixture's `inside` cases: what came back (true / false / new / same), the returned descriptions, the output bytes, the bytes behind the buffers;
interlace's false / true sequence, a size change between frames through one state, a codec a module refuses.  The `deviating` cases run the
MI355X module alone, against the restatement (tests/compose_restatement.py).  0 bytes differing."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import compose_restatement as rs  # noqa: E402
import make_compose_golden as gen  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(gen.HARNESS), reason="oracle/_ref/ug_compose_harness not built (no reference tree)")]
GOLD = np.load(os.path.join(HERE, "golden", "compose_ref.npz"))
META = json.loads(str(GOLD["meta"]))
IDS = [f"{k}-{m['kind']}-{m['name']}-{m['mode']}-{m['codec']}-{'x'.join(map(str, m['frames'][0]))}" for k, m in enumerate(META)]


def run(k, names, tmp):
    m = META[k]
    ins = [GOLD[f"in_{m['codec']}_{w}x{h}x{m['tiles']}"] for w, h in m["frames"]]
    pam = gen.make_pam(GOLD[f"logo_{k}"], m["logo"][0], m["logo"][1], m["logo"][3]) if m["logo"] else None
    res, rc, log = gen.run_harness(gen.HARNESS, names, gen.options_of(m, str(tmp), pam), m["codec"], m["mode"], m["tiles"],
                                   [(w, h, d) for (w, h), d in zip(m["frames"], ins)], str(tmp))
    assert rc == 0, log
    return ins, res, log


def written(m, fm, out):
    """the bytes of an output the module is held to: crop writes the part of the output's line that the source line holds"""
    if m["name"] == "crop":
        ow, oh, xb, _ = rs.crop_geometry(m["codec"], *m["frames"][fm["i"]], *rs.parse_crop(m["options"]))
        lb = min(rs.linesize(m["codec"], ow), rs.linesize(m["codec"], m["frames"][fm["i"]][0]) - xb)
        return out.reshape(oh, -1)[:, :lb].reshape(-1)
    return out


@pytest.mark.parametrize("k", range(len(META)), ids=IDS)
def test_module_beside_the_reference_module_in_the_same_run(tmp_path, k):
    m = META[k]
    ours = m["name"] + "_mi355x"
    beside = m["kind"] == "inside"
    ins, res, log = run(k, m["name"] + "+" + ours if beside else ours, tmp_path)
    assert len(res[ours]) == len(m["frames"]), log
    for i, (o, fm) in enumerate(zip(res[ours], m["frames_meta"])):
        fm = dict(fm, i=i)
        if beside:
            r = res[m["name"]][i]
            desc = lambda x: {key: v for key, v in x.items() if key != "out"}  # noqa: E731
            assert desc(r) == desc(o), (i, desc(r), desc(o))                    # what came back, its description, the pad
            assert ("out" in r) == ("out" in o)
            if "out" in r:
                assert int(np.count_nonzero(written(m, fm, r["out"]) != written(m, fm, o["out"]))) == 0
        assert o["pad"] in (0, -1), (i, o["pad"])
        if fm["refused"]:  # where ug_hip_compose refuses: false from a postprocessor, the frame as it came from logo
            assert o["ret"] == ("false" if m["mode"] == "pp" else "same"), (i, o["ret"])
            if "out" in o:
                assert np.array_equal(o["out"], ins[i])
            continue
        assert o["ret"] == fm["ret"], (i, o["ret"], fm["ret"])
        if "w" in fm:
            assert (o["w"], o["h"], o["tile_count"], o["interlacing"], o["fps"], o["codec"]) == (fm["w"], fm["h"], fm["tile_count"], fm["interlacing"], fm["fps"], m["codec"])
        if f"out_{k}_{i}" in GOLD.files:
            want = GOLD[f"out_{k}_{i}"]
            got = written(m, fm, o["out"])
            assert got.size == want.size and int(np.count_nonzero(got != want)) == 0, (i, int(np.count_nonzero(got != want)))
        else:
            assert "out" not in o or m["codec"] == "v210"


def test_interlace_as_a_capture_filter_beside_the_reference(tmp_path):
    """through capture_filter/vo_pp_wrapper.h, as the reference registers its own: NULL for the first frame of a pair, a woven frame for the second"""
    rng = np.random.default_rng(8)
    frames = [(10, 6, np.frombuffer(rng.bytes(20 * 6), np.uint8)) for _ in range(4)]
    res, rc, log = gen.run_harness(gen.HARNESS, "interlace+interlace_mi355x", "-", "UYVY", "cf", 1, frames, str(tmp_path))
    assert rc == 0, log
    r, o = res["interlace"], res["interlace_mi355x"]
    assert [x["ret"] for x in r] == [x["ret"] for x in o] == ["null", "new", "null", "new"]
    for i in (1, 3):
        assert (o[i]["interlacing"], o[i]["fps"]) == (r[i]["interlacing"], r[i]["fps"]) == (3, 12.5)
        want = rs.interlace("UYVY", frames[i - 1][2], frames[i][2], 10, 6)
        assert np.array_equal(o[i]["out"], want) and np.array_equal(r[i]["out"], want)


def test_option_strings_are_refused_as_the_reference_refuses_them(tmp_path):
    frame = [(2, 2, np.zeros(8, np.uint8))]
    for name, options, mode in (("crop", "size=10", "pp"), ("crop", "bogus=1", "cf"), ("border", "color=12345", "pp"), ("border", "thick=2", "pp"),
                                ("split", "2", "pp"), ("interlaced_3d", "x", "pp"), ("logo", "/nonexistent/logo.pam", "cf"), ("logo", "logo.png", "cf")):
        for n in (name, name + "_mi355x"):
            res, rc, log = gen.run_harness(gen.HARNESS, n, options, "UYVY", mode, 2 if name == "interlaced_3d" else 1, frame, str(tmp_path))
            assert rc == 2 and not res, (n, options, rc, log)
