"""GPU: the *_mi355x de-interlacing postprocessors through the reference's own vo_postprocess.c (oracle/_ref/ug_deint_harness), each against
the reference's CPU module of the same name IN THE SAME RUN -- the same three frames through `double_framerate` and `double_framerate_mi355x` --
and against the restatement: every case of the fixture's list (all formats, `force` on progressive input, progressive input without it, `:d`,
`nodelay`, a reconfigure to another size, a codec the averages do not take, req_pitch equal to and larger than the line size), and
postprocess(NULL) twice (the second false).  0 bytes differing.  Left out of the comparison with the reference, as conditions:
the first double_framerate output after a reconfigure (the reference's uninitialised buffer) and the pitch gaps; against the restatement
nothing is left out and the gaps must hold their 0xA5."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import deinterlace_restatement as rs  # noqa: E402
import make_temporal_deint_golden as gen  # noqa: E402

pytestmark = pytest.mark.gpu
HARNESS = gen.HARNESS
GOLD = np.load(os.path.join(HERE, "golden", "temporal_deint_ref.npz"))
CASES = json.loads(str(GOLD["cases"]))


def run_case(tmp, m, names, extra=None):
    """the case's frames through `names` in one process; returns {name: (rets, descs, [[out0, out1 or None] per frame])}, the inputs"""
    extra = m["extra"] if extra is None else extra
    args, ins, a = [], [], 0
    for i, (w, h) in enumerate(m["sizes"]):
        L = gen.linesize(m["codec"], w)
        frame = GOLD["in_" + m["id"]][a: a + L * h]
        a += L * h
        path = os.path.join(tmp, f"{m['id']}.{i}.in")
        frame.tofile(path)
        ins.append(frame.reshape(h, L))
        args += [str(w), str(h), path]
    prefix = os.path.join(tmp, m["id"])
    r = subprocess.run([HARNESS, "run", "+".join(names), m["opts"], m["codec"], m["inter"], str(extra), prefix, "1"] + args,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (m["id"], r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    res = {}
    for name in names:
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith(name + " frame ")]
        rets = [ln.split("ret=")[1] for ln in lines]
        outs = []
        for i, (w, h) in enumerate(m["sizes"]):
            L = gen.linesize(m["codec"], w)
            fr = []
            for k in range(2):
                path = f"{prefix}.{name}.{i}.{k}"
                fr.append(np.fromfile(path, np.uint8).reshape(h, L + extra) if rets[i][k] == "1" else None)
            outs.append(fr)
        res[name] = (rets, [ln.split()[3:10] for ln in lines], outs)
    return res, ins


def restated(m, ins, extra):
    cls = rs.FORMATS[m["codec"]][1] if m["codec"] in rs.FORMATS else None
    active = m["inter"] == "merged" or m["opts"] == "force"
    out, start = [], 0
    for i in range(1, len(ins) + 1):
        if i == len(ins) or ins[i].shape != ins[start].shape:
            out += rs.module_run(m["name"], m["opts"], cls, active, ins[start].shape[1], ins[start].shape[1] + extra, ins[start:i])
            start = i
    return out


@pytest.mark.skipif(not os.path.exists(HARNESS), reason="oracle/_ref/ug_deint_harness not built (no reference tree)")
def test_every_name_against_the_reference_module_in_the_same_run(tmp_path):
    total = left = 0
    for m in CASES:
        mine = m["name"] + "_mi355x"
        res, ins = run_case(str(tmp_path), m, [m["name"], mine])
        (rrets, rdescs, routs), (grets, gdescs, gouts) = res[m["name"]], res[mine]
        assert grets == rrets == m["rets"], (m["id"], grets, rrets)  # postprocess(NULL) twice: the second false
        assert gdescs == rdescs, (m["id"], gdescs, rdescs)
        want = restated(m, ins, m["extra"])
        active = m["inter"] == "merged" or m["opts"] == "force"
        for i in range(len(ins)):
            L = ins[i].shape[1]
            for k in range(2):
                if gouts[i][k] is None:
                    assert routs[i][k] is None
                    continue
                bad = int(np.count_nonzero(gouts[i][k] != want[i][k]))
                assert bad == 0, f"{m['id']} frame {i} output {k}: {bad} bytes differ from the restatement"
                keep = np.ones(gouts[i][k].shape[0], bool)
                ex = gen.excluded(m["name"], m["opts"], active, [tuple(s) for s in m["sizes"]], i, k)
                if ex is not None:
                    keep[ex] = False
                bad = int(np.count_nonzero(gouts[i][k][keep, :L] != routs[i][k][keep, :L]))
                assert bad == 0, f"{m['id']} frame {i} output {k}: {bad} bytes differ from the reference module"
                total += gouts[i][k].size
                left += int(np.count_nonzero(~keep)) * L + gouts[i][k].shape[0] * m["extra"]
    print(f"left out of the comparison with the reference: {100 * left / total:.2f} % of {total} bytes")
    assert left < 0.05 * total


@pytest.mark.skipif(not os.path.exists(HARNESS), reason="oracle/_ref/ug_deint_harness not built (no reference tree)")
def test_pitched_output_where_the_reference_takes_none(tmp_path):
    """req_pitch larger than the line size for `deinterlace` (the reference asserts req_pitch == line size), `:d` (the reference blends at the
    line size) and the plain copy of progressive input (the reference copies packed): the stand-in honours the pitch -- against the restatement"""
    n = 0
    for m in CASES:
        if not (m["name"] in ("deinterlace", "deinterlace_blend") or m["opts"] == "d" or (m["inter"] == "prog" and m["opts"] != "force")):
            continue
        mine = m["name"] + "_mi355x"
        res, ins = run_case(str(tmp_path), m, [mine], extra=32)
        rets, _descs, outs = res[mine]
        assert rets == m["rets"]
        want = restated(m, ins, 32)
        for i in range(len(ins)):
            for k in range(2):
                if outs[i][k] is not None:
                    assert np.array_equal(outs[i][k], want[i][k]), (m["id"], i, k)
                    n += 1
    assert n >= 60
