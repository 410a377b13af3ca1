"""The helper of the planar layout tests (tests/planar_layout.py) checked on the CPU: every layout has the addresses and pitches it claims,
compare() reports each of its four kinds of finding, and the restatement equals the compiled reference in every layout for every
conversion under the helper's rules -- which pins the restatement for the machine without the reference tree."""
import numpy as np
import pytest

import planar_layout as PL
from pitch_layout import FILL, GUARD

FROM = PL.from_variants()


def _cases(kind, name, depth, sizes, layouts=PL.LAYOUTS):
    for i, (w, h) in enumerate(sizes):
        if PL.size_ok(kind, name, w, h):
            for j, layout in enumerate(layouts):
                yield PL.make_case(kind, name, depth, w, h, layout, seed=3 * i + j)


def test_variants_are_all_there():
    assert len(FROM) == 39 and len({n for n, _ in FROM}) == 28 and len(PL.PO.TO_NAMES) == 9


def test_every_conversion_has_gpu_sizes_it_takes():
    """no name is left without a case: at least four sizes each, every one taken, a ragged one among them, and for the names whose reference
    wants even sizes one that is even both ways"""
    for kind, name in [("from", n) for n, _ in FROM] + [("to", n) for n in PL.PO.TO_NAMES]:
        sizes = PL.gpu_sizes(kind, name)
        assert len(sizes) >= 4 and all(PL.dispatcher_takes(kind, name, w, h) for w, h in sizes), (name, sizes)
        assert any(w % 8 for w, _ in sizes) and any(w >= 512 for w, _ in sizes), (name, sizes)
        one = PL.one_off_sizes(kind, name)
        assert one and all(PL.dispatcher_takes(kind, name, w, h) for w, h in one), (name, one)
        if name in ("uyvy_to_nv12", "uyvy_to_i420", "yuv420_to_i420"):
            assert any(w % 2 == 0 and h % 2 == 0 for w, h in sizes) and any(w % 2 == 0 and h % 2 == 0 for w, h in one), name


@pytest.mark.parametrize("kind,name,depth", [("from", "gbrp12le_to_r12l", 0), ("from", "gbrap_to_rgba", 0), ("from", "rgbpXX_to_rgb", 8),
                                             ("from", "yuv420p_to_uyvy", 0), ("from", "yuv422p10le_to_v210", 0), ("from", "yuv420_to_i420", 0),
                                             ("to", "v210_to_p010le", 0), ("to", "uyvy_to_nv12", 0), ("to", "vuya_to_i444", 0),
                                             ("to", "r12l_to_gbrp16le", 0)])
def test_layouts_are_what_they_claim(kind, name, depth):
    for w, h in [(96, 6), (50, 8), (18, 6)]:
        ops = {}
        for layout in PL.LAYOUTS + ["one_off"]:
            for which in (PL.one_off_operands(kind, name, depth, w, h) if layout == "one_off" else [None]):
                c = PL.make_case(kind, name, depth, w, h, layout, which=which)
                every = c.planes + [c.packed]
                ops[layout] = every
                for k, op in enumerate(every):
                    what = (name, w, h, layout, which, k)
                    assert op.whole.ctypes.data % 256 == 0, what
                    assert op.whole.size >= op.off + (op.rows + 1) * op.pitch + GUARD and op.off >= GUARD, what
                    is_src = op in c.srcs
                    assert is_src or (op.whole == FILL).all(), what
                    assert not is_src or len(np.unique(op.whole)) > 16, what
                    base = op.addr % 256
                    packed_src = kind == "to" and op is c.packed
                    if layout == "tight":
                        assert base == 0 and (packed_src or op.pitch == op.line), what
                    elif layout == "odd":
                        assert base == 0 and (packed_src or (op.pitch > op.line and op.pitch % 16 and (op.pitch - op.line) % op.unit == 0)), what
                    elif layout == "offset":
                        assert base == op.unit and (packed_src or (op.pitch == PL.roundup16(op.line) + 64)), what
                    else:
                        assert base == (op.unit if k == which else 0) and (packed_src or op.pitch % 16 == 0), what
                    if packed_src:  # the dispatcher's packed source has no pitch of its own
                        assert op.pitch == (2 * w if name == "uyvy_to_nv12" else op.line), what
        odd = [op.pitch for op in ops["odd"][:-1]]
        if PL.shared_pitch(name, depth):
            assert len(set(odd)) == 1, (name, odd)
        else:
            assert len(set(odd)) == len(odd), (name, "two planes share a pitch", odd)


def test_compare_reports_each_kind_of_finding():
    c = PL.make_case("to", "vuya_to_i444", 0, 18, 3, "offset")
    want = PL.restate(c)
    good = [op.whole.copy() for op in want.ops]
    assert PL.compare(good, want) == []
    op = want.ops[1]
    spots = {"differ inside the lines": op.off + op.pitch + 5, "padding bytes written": op.off + op.line + 1,
             "of the spare line written": op.off + op.rows * op.pitch + 2, "of the canary in front written": op.off - 1,
             "of the canary behind written": op.end}
    for text, at in spots.items():
        bad = [g.copy() for g in good]
        bad[1][at] ^= 0xFF
        found = PL.compare(bad, want)
        assert len(found) == 1 and text in found[0] and "operand 1" in found[0], (text, found)
    # bits of a ragged R12L line: only those of real pixels count, and nothing outside them is looked at
    c = PL.make_case("from", "gbrp12le_to_r12l", 0, 9, 2, "tight")
    w = PL.restate(c)
    ragged = PL.Want("real pixels", w.ops, [36 * 9 // 8], bits=4, untouched=False)
    g = [w.ops[0].whole.copy()]
    g[0][w.ops[0].off + 40] ^= 0xF0
    g[0][w.ops[0].off + 41] ^= 0xFF
    g[0][5] ^= 0xFF
    assert PL.compare(g, ragged) == []
    g[0][w.ops[0].off + 40] ^= 0x01
    assert "last real pixel" in PL.compare(g, ragged)[0]


def test_mirror_is_aligned_and_whole():
    import torch
    c = PL.make_case("from", "gbrp10le_to_rgb", 0, 17, 3, "offset")
    for op in c.planes + [c.packed]:
        t, addr = PL.mirror(torch, op, device="cpu")
        assert t.data_ptr() % 256 == 0 and addr % 256 == op.addr % 256 == op.unit
        assert np.array_equal(t.numpy(), op.whole)


def test_tight_twin_holds_the_same_pixels():
    c = PL.make_case("from", "yuv420p_to_uyvy", 0, 50, 7, "custom", plane_pitches=[54, 33, 37], packed_pitch=104, offs=[0, 1, 0, 4])
    t = PL.tight_twin(c)
    for a, b in zip(t.planes, c.planes):
        assert a.pitch == a.line and np.array_equal(a.samples(), b.samples())
    assert np.array_equal(PL.restate(t).ops[0].samples(), PL.restate(c).ops[0].samples())


@pytest.mark.parametrize("name,depth", FROM)
def test_from_restatement_is_layout_independent(name, depth):
    """runs without oracle/_ref: the restatement of a laid-out case equals that of the same pixels laid out tight"""
    for c in _cases("from", name, depth, PL.FROM_SIZES, ["odd", "offset"]):
        assert np.array_equal(PL.restate(c).ops[0].samples(), PL.restate(PL.tight_twin(c)).ops[0].samples()), c


@pytest.mark.parametrize("name", PL.TO_NAMES)
def test_to_restatement_is_layout_independent(name):
    for c in _cases("to", name, 0, PL.TO_SIZES, ["odd", "offset"]):
        if name == "v210_to_p010le" and c.w % 6:
            continue  # whole lines: the padding is part of the result
        for a, b in zip(PL.restate(c).ops, PL.restate(PL.tight_twin(c)).ops):
            assert np.array_equal(a.samples(), b.samples()), c


@pytest.mark.parametrize("name,depth", FROM)
def test_from_restatement_vs_reference_in_every_layout(po, name, depth):
    if not po.have_ref():
        pytest.skip("oracle/_ref not built")
    findings = []
    for c in _cases("from", name, depth, PL.FROM_SIZES):
        wants = PL.expectations(c)
        assert len(wants) == 2, c
        findings += [f"{c}: {f}" for f in PL.compare([op.whole for op in wants[0].ops], wants[1])]
    assert not findings, "\n".join(findings)


@pytest.mark.parametrize("name", PL.TO_NAMES)
def test_to_restatement_vs_reference_in_every_layout(po, name):
    if not po.have_ref():
        pytest.skip("oracle/_ref not built")
    findings, asked = [], 0
    for c in _cases("to", name, 0, PL.TO_SIZES):
        wants = PL.expectations(c)
        asked += len(wants) - 1
        for w in wants[1:]:
            findings += [f"{c}: {f}" for f in PL.compare([op.whole for op in wants[0].ops], w)]
    assert asked and not findings, "\n".join(findings)


@pytest.mark.parametrize("kind,name,depth,size", [("from", "gbrp16le_to_rg48", 0, (96, 5)), ("from", "yuv420p_to_uyvy", 0, (560, 3)),
                                                  ("to", "uyvy_to_nv12", 0, (96, 6)), ("to", "r12l_to_rgbp12le", 0, (96, 5))])
def test_one_off_is_held_to_the_tight_result(po, kind, name, depth, size):
    """the one_off layout's expectation is the tight twin's, carried over line by line"""
    w, h = size
    for which in PL.one_off_operands(kind, name, depth, w, h):
        c = PL.make_case(kind, name, depth, w, h, "one_off", seed=which, which=which)
        wants = PL.expectations(c)
        assert len(wants) == (2 if po.have_ref() else 1)
        for wt in wants[1:]:
            assert PL.compare([op.whole for op in wants[0].ops], wt) == [], (c, wt.label)
