"""GPU parity and counters for the slot form of the colour stage's reference side (dxt_encode.hip, encode_dxt5ycocg, chroma-pair loaders): a wave
that holds an uncertified chroma pair keeps the projection's index for every certified pair and evaluates the reference's two distances only
for the two pixels of each pair slot (0 .. 7) in which one of its blocks holds an uncertified pair; only the uncertified lanes take the result.
ug_hip_dxt_encode_stats_pair_slots counts those (wave, slot) evaluations.  UYVY and v210 -> DXT5-YCoCg at 512 x 32 and 510 x 30 (the EDGE
instantiation: cut pair at the right edge, cut rows in the last block row), both tie rules, byte for byte against the oracle, on frames built
block by block with the CPU model of tests/test_dxt_pair_projection_bound.py.  A near pair lies within eps / 4 of a bisector, every other pair
at least 4 eps away or in a flat block: the factor 4 on either side keeps the expected counts independent of how the GPU's fma, reciprocal and
square root and the model's round.  What a frame is expected to count is read off the model of the finished frame (the slots in which some
lane of a wave holds a near pair); what the frame was built for is asserted on that model as well.
  one_slot[k]            every wave holds exactly one block with one near pair, in slot k (a cut last block row repeats row 1 in rows 2, 3: there
                         the pair sits in slot k % 2); the pairs of a pool block are exchanged to bring its pair to the slot and the block goes
                         through the model again; each frame meets all three bisectors from either side
  two_lanes_two_slots    two blocks of a wave, near pairs in slots 1 and 6 (cut rows: 1 and 0): 2 evaluations per wave
  all_slots              one block per wave has all eight pairs near: 8 per wave
  misdecided             every wave holds a near pair whose index from the projection is NOT the oracle's in at least one pixel (exact ties at
                         1/6 and 5/6 of the segment among them), brought to every slot the model confirms, slots 0 and 7 among them: the
                         frame that fails if an uncertified lane does not take the distances' result.  One size also mirrored.
  flat_beside_uncertified  a flat block next to the near block: the flat lane requests no slot
and the frames of tests/test_gpu_dxt_pair_projection.py through the new counter.  Frames are per format: a format's waves hold other blocks."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dxt_pair_projection_bound import projection_stage  # noqa: E402
from test_gpu_dxt_pair_cov import ENDS, FRAMES as COV_FRAMES, PLACED, SIZES, pack_uyvy, pack_v210, planes, wave_evaluations  # noqa: E402
from test_gpu_dxt_pair_linear import encode  # noqa: E402
from test_gpu_dxt_pair_projection import FRAMES as PROJECTION_FRAMES, margin_over_eps  # noqa: E402
from test_gpu_dxt_pair_zone import frames_for  # noqa: E402

pytestmark = pytest.mark.gpu
FORMATS = ("UYVY", "v210")
# block columns of a block row that reach every wave once, and the step to a second block of the same wave: UYVY holds one block per lane (64
# consecutive columns to a wave), v210 three per lane and a wave passes the stage once for block k = 0, 1, 2 of its lanes (columns k, k + 3, ...)
ANCHORS = {"UYVY": ((PLACED[0], PLACED[3]), 1), "v210": (PLACED[:3], 3)}


def wave_groups(fmt, bw):
    cols = [np.arange(bw)] if fmt == "UYVY" else [np.arange(k, bw, 3) for k in range(3)]
    return [c[i:i + 64] for c in cols for i in range(0, len(c), 64)]


def classify(s):
    """-> (near, far): (bh, bw, 8) per pair.  near: within eps / 4 of a bisector in a block that reaches the projection; far: at least 4 eps
    away, or the block is flat (its lanes request no slot)"""
    with np.errstate(invalid="ignore"):
        worst, least = margin_over_eps(s)
        live = (s["pre"] & ~s["flat"])[..., None]
        return (worst <= 0.25) & live, (least >= 4.0) | ~live


def bisector_and_side(s, near):
    """the set of (bisector 0 .. 2, side) of the near pairs"""
    t = 3.0 * s["t64"][near]
    return {(int(k), bool(side)) for k, side in zip(np.floor(t), t > np.floor(t) + 0.5)}


def model_of_blocks(po, blocks):
    """a list of (yb, ub, vb) blocks -> the model of a frame that holds them in one block row"""
    yb, ub, vb = (np.stack([b[i] for b in blocks])[None] for i in range(3))
    return projection_stage(po, *planes(yb, ub, vb, 4 * len(blocks), 4))


def swap_pairs(block, a, b):
    """the block with chroma pairs a and b (pair j: row j // 2, columns 2 (j % 2), 2 (j % 2) + 1) exchanged, lumas included"""
    yb, ub, vb = (np.array(p).copy() for p in block)
    for p, width in ((yb, 2), (ub, 1), (vb, 1)):
        q = p.reshape(8, width)
        q[[a, b]] = q[[b, a]]
    return yb, ub, vb


@functools.lru_cache(maxsize=None)
def single_pool(po, cut_rows, want=3):
    """seeded search, as near_bisector_pool: blocks inside the stage's precondition, not flat, with exactly ONE near pair and seven far ones.
    cut_rows: rows 2, 3 repeat row 1, so the one pair lies in row 0.  -> {(bisector, side): [(block, pair), ...]}"""
    rng = np.random.default_rng(9031 + cut_rows)
    bh, bw = 256, 512
    uv = rng.integers(8, 236, (bh, bw, 1, 1, 2)) + rng.integers(0, 12, (bh, bw, 4, 2, 2))
    yb = ENDS[rng.integers(0, 4, (bh, bw, 4, 2))].reshape(bh, bw, 4, 4)
    if cut_rows:
        uv[:, :, 2:] = uv[:, :, 1:2]
        yb[:, :, 2:] = yb[:, :, 1:2]
    s = projection_stage(po, *planes(yb, uv[..., 0], uv[..., 1], 4 * bw, 4 * bh))
    near, far = classify(s)
    ok = (near.sum(-1) == 1) & (near | far).all(-1)
    out = {}
    for by, bx in np.argwhere(ok):
        pair = int(near[by, bx].argmax())
        (cat,) = bisector_and_side({"t64": s["t64"][by, bx]}, near[by, bx])
        if len(out.setdefault(cat, [])) < want:
            out[cat].append(((yb[by, bx], uv[by, bx, ..., 0], uv[by, bx, ..., 1]), pair))
    assert len(out) == 6, sorted(out)
    return out


@functools.lru_cache(maxsize=None)
def slot_blocks(po, cut_rows):
    """the blocks of single_pool with their near pair brought to slot k, each checked again with the model: the end points depend on sums over
    the pixels in their order.  -> {(k, (bisector, side)): block}, k = 0 .. 7 (cut rows: 0, 1)"""
    tried = [(k, cat, swap_pairs(block, pair, k)) for cat, found in sorted(single_pool(po, cut_rows).items()) for block, pair in found
             for k in range(2 if cut_rows else 8)]
    s = model_of_blocks(po, [t[2] for t in tried])
    near, far = classify(s)
    out = {}
    for n, (k, cat, block) in enumerate(tried):
        only_k = near[0, n, k] and near[0, n].sum() == 1 and (near | far)[0, n].all()   # (the repeated rows of a cut block are pairs 4 .. 7 to the model)
        if only_k and bisector_and_side({"t64": s["t64"][0, n]}, near[0, n]) == {cat}:
            out.setdefault((k, cat), block)
    return out


@functools.lru_cache(maxsize=None)
def short_segment_pool(po, cut_rows):
    """seeded search among blocks of two chroma values 0 .. 8 byte steps apart under extreme lumas (short palette segments: a wide eps), inside
    the stage's precondition, every pair near or far.  -> (blocks whose eight pairs are all near, [(block, pairs whose index from the
    projection differs from the oracle's in a pixel and that are near)])"""
    all_near, misdecided = [], []
    for seed in range(12):
        rng = np.random.default_rng(7000 + seed + 100 * cut_rows)
        bh, bw = 128, 512
        yb = ENDS[rng.integers(0, 4, (bh, bw, 4, 2))].reshape(bh, bw, 4, 4)
        uv = rng.integers(8, 240, (bh, bw, 1, 1, 2)) + rng.integers(0, 9, (bh, bw, 1, 1, 2)) * rng.integers(0, 2, (bh, bw, 4, 2, 1))
        if cut_rows:
            uv[:, :, 2:] = uv[:, :, 1:2]
            yb[:, :, 2:] = yb[:, :, 1:2]
        s = projection_stage(po, *planes(yb, uv[..., 0], uv[..., 1], 4 * bw, 4 * bh))
        near, far = classify(s)
        differs = (s["proj_idx"][..., 0::2] != s["want"][..., 0::2]) | (s["proj_idx"][..., 1::2] != s["want"][..., 1::2])
        wrong = differs & near & (near | far).all(-1)[..., None]
        block = lambda by, bx: (yb[by, bx], uv[by, bx, ..., 0], uv[by, bx, ..., 1])
        all_near += [block(by, bx) for by, bx in np.argwhere(near.all(-1))]
        misdecided += [(block(by, bx), tuple(np.flatnonzero(wrong[by, bx]))) for by, bx in np.argwhere(wrong.any(-1))]
        if len(all_near) >= 2 and len(misdecided) >= 4:
            break
    assert len(all_near) >= 2 and len(misdecided) >= 2, (len(all_near), len(misdecided))
    return all_near, misdecided


@functools.lru_cache(maxsize=None)
def misdecided_blocks(po, cut_rows):
    """the misdecided blocks of short_segment_pool with a misdecided pair brought to every slot the model confirms (cut rows: as found).
    -> {slot: [block, ...]} of blocks that hold a near pair in that slot whose projection index is not the oracle's"""
    found = short_segment_pool(po, cut_rows)[1]
    tried = [(block, pairs) for block, pairs in found]
    if not cut_rows:
        tried += [(swap_pairs(block, pairs[0], k), None) for block, pairs in found for k in range(8) if k != pairs[0]]
    s = model_of_blocks(po, [t[0] for t in tried])
    near, far = classify(s)
    differs = (s["proj_idx"][..., 0::2] != s["want"][..., 0::2]) | (s["proj_idx"][..., 1::2] != s["want"][..., 1::2])
    out = {}
    for n, (block, _) in enumerate(tried):
        if (near | far)[0, n].all():
            for k in np.flatnonzero(differs[0, n] & near[0, n]):
                out.setdefault(int(k), []).append(block)
    return out


@functools.lru_cache(maxsize=None)
def decided_blocks(po, w, h):
    """the background: every block inside the stage's precondition and every pair far (flat blocks among them)"""
    rng = np.random.default_rng(61 + w)
    bw, bh = (w + 3) // 4, (h + 3) // 4
    yb, ub, vb = rng.integers(0, 256, (bh, bw, 4, 4)), rng.integers(0, 256, (bh, bw, 4, 2)), rng.integers(0, 256, (bh, bw, 4, 2))
    flat = np.arange(bh * bw).reshape(bh, bw) % 11 == 7
    for p in (yb, ub, vb):
        p[flat] = rng.integers(0, 256, (int(flat.sum()), 1, 1))
    for _ in range(50):
        s = projection_stage(po, *planes(yb, ub, vb, w, h))
        bad = ~(s["pre"] & classify(s)[1].all(-1))
        if not bad.any():
            break
        m = int(bad.sum())
        yb[bad], ub[bad], vb[bad] = rng.integers(0, 256, (m, 4, 4)), rng.integers(0, 256, (m, 4, 2)), rng.integers(0, 256, (m, 4, 2))
    assert not bad.any()
    return yb, ub, vb


def build(po, fmt, w, h, blocks_at):
    """the background with blocks_at(n, cut_rows) -> [block, ...] put at the n-th anchor and the columns `step` further on.
    -> (y, u, v), the model, near pairs (bh, bw, 8), placed blocks (bh, bw)"""
    yb, ub, vb = (p.copy() for p in decided_blocks(po, w, h))
    bh, bw = yb.shape[:2]
    anchors, step = ANCHORS[fmt]
    placed = np.zeros((bh, bw), bool)
    n = 0
    for by in range(bh):
        for bx in anchors:
            for i, block in enumerate(blocks_at(n, bool(h % 4) and by == bh - 1)):
                yb[by, bx + i * step], ub[by, bx + i * step], vb[by, bx + i * step] = block
                placed[by, bx + i * step] = True
            n += 1
    y, u, v = planes(yb, ub, vb, w, h)
    s = projection_stage(po, y, u, v)
    near, far = classify(s)
    assert s["pre"].all() and (near | far).all() and not near[~placed].any()   # every wave reaches the stage; nothing between near and far
    return (y, u, v), s, near, placed


def expected(near, fmt):
    """-> (waves that hold a near pair, (wave, slot) evaluations) of one encode"""
    waves = slots = 0
    for row in near:
        for cols in wave_groups(fmt, near.shape[1]):
            waves += int(row[cols].any())
            slots += int(row[cols].any(0).sum())
    return waves, slots


def run(po, name, fmt, planes_, w, h):
    """both tie rules against the oracle -> (counts[0 .. 3] of the ties-even encode, its slot evaluations, complaints)"""
    from ultragrid_amd import lib as L
    so = L.load()
    y, u, v = planes_
    low = np.random.default_rng(99 + w).integers(0, 4, (h, 2 * w)).astype(np.uint32)
    pf, pin, src = (L.PF_UYVY, po.IN_UYVY, pack_uyvy(y, u, v)) if fmt == "UYVY" else (L.PF_V210, po.IN_V210, pack_v210(y, u, v, low))
    bad, seen = [], []
    for ties, tname in ((L.TIES_EVEN, "even"), (L.TIES_AWAY, "away")):
        got, st = encode(so, pf, src, w, h, ties, po, reset=False)
        n = C.c_ulonglong(0)
        assert so.ug_hip_dxt_encode_stats_pair_slots(C.byref(n), 1) == 0
        want = po.dxt_encode(pin, po.OUT_DXT5YCOCG, src, w, h, ties=tname)
        if not np.array_equal(got, want):
            bad.append((name, fmt, tname, int(np.count_nonzero(got != want))))
        seen.append((st, int(n.value)))
    if seen[0] != seen[1]:   # the same waves and slots under either tie rule
        bad.append((name, fmt, "counters under ties even / away", seen))
    print(f"{name} {fmt} {w}x{h}: colour full form {seen[0][0][0]}, per-pixel distance waves {seen[0][0][3]}, slot evaluations {seen[0][1]} "
          f"of {wave_evaluations(fmt, w, h)} waves")
    return seen[0][0], seen[0][1], bad


def check(po, name, fmt, w, h, frame, per_wave):
    planes_, s, near, _ = frame
    waves, slots = expected(near, fmt)
    assert waves == wave_evaluations(fmt, w, h), (name, fmt, waves)   # what the frame is for: every wave holds a near pair
    if per_wave is not None:
        assert slots == per_wave * waves, (name, fmt, slots, waves)
    st, evaluations, bad = run(po, name, fmt, planes_, w, h)
    assert not bad, bad
    assert st[0] == 0 and st[3] == waves and evaluations == slots, (name, fmt, st, evaluations, (waves, slots))
    return s, near


def one_slot(po, k, size):
    w, h = size
    cats = sorted({cat for _, cat in slot_blocks(po, False)})

    def blocks_at(n, cut):
        pool, slot = slot_blocks(po, cut), (k % 2 if cut else k)
        have = [cat for cat in cats if (slot, cat) in pool]
        return [pool[slot, have[(k + n) % len(have)]]]
    for fmt in FORMATS:
        frame = build(po, fmt, w, h, blocks_at)
        s, near = check(po, f"one_slot[{k}]", fmt, w, h, frame, 1)
        whole = near[: h // 4]
        assert whole[..., k].sum() == whole.sum() == frame[3][: h // 4].sum()   # one near pair per placed block, in slot k
        assert len(bisector_and_side(s, near)) == 6   # all three bisectors from either side


def two_lanes_two_slots(po, size):
    w, h = size

    def blocks_at(n, cut):
        pool = slot_blocks(po, cut)
        pick = lambda slot: next(pool[key] for key in sorted(pool)[n % 3:] + sorted(pool) if key[0] == slot)
        return [pick(1), pick(0 if cut else 6)]
    for fmt in FORMATS:
        _, near = check(po, "two_lanes_two_slots", fmt, w, h, build(po, fmt, w, h, blocks_at), 2)
        whole = near[: h // 4]
        assert whole[..., 1].sum() == whole[..., 6].sum() == whole.sum() // 2


def all_slots(po, size):
    w, h = size

    def blocks_at(n, cut):
        pool = short_segment_pool(po, cut)[0]
        return [pool[n % len(pool)]]
    for fmt in FORMATS:
        frame = build(po, fmt, w, h, blocks_at)
        _, near = check(po, "all_slots", fmt, w, h, frame, 8)
        assert near[frame[3]].all()


def misdecided_frame(po, fmt, w, h):
    def blocks_at(n, cut):
        pool = misdecided_blocks(po, cut)
        slots = sorted(pool)
        found = pool[slots[n % len(slots)]]
        return [found[(n // len(slots)) % len(found)]]
    return build(po, fmt, w, h, blocks_at)


def misdecided(po, size):
    w, h = size
    assert {0, 7} <= set(misdecided_blocks(po, False)), sorted(misdecided_blocks(po, False))
    print("slots with a misdecided pair:", sorted(misdecided_blocks(po, False)), "cut rows:", sorted(misdecided_blocks(po, True)))
    for fmt in FORMATS:
        frame = misdecided_frame(po, fmt, w, h)
        s, near = check(po, "misdecided", fmt, w, h, frame, None)
        differs = (s["proj_idx"][..., 0::2] != s["want"][..., 0::2]) | (s["proj_idx"][..., 1::2] != s["want"][..., 1::2])
        wrong = differs & near
        assert expected(wrong, fmt)[0] == wave_evaluations(fmt, w, h)   # in every wave the projection alone would give another byte
        at = np.flatnonzero(wrong[: h // 4].any((0, 1)))
        assert {0, 7} <= set(at), at
        t = 3.0 * s["t64"][wrong]
        print(f"misdecided {fmt} {w}x{h}: {int(wrong.sum())} pairs in slots {at.tolist()}, at 3 s = {sorted(set(np.round(t, 2)))}")


def misdecided_mirrored(hip, po, fmt):
    import torch
    from ultragrid_amd import lib as L
    w, h = SIZES[1]
    y, u, v = misdecided_frame(po, fmt, w, h)[0]
    low = np.random.default_rng(99 + w).integers(0, 4, (h, 2 * w)).astype(np.uint32)
    pf, pin, src = (L.PF_UYVY, po.IN_UYVY, pack_uyvy(y, u, v)) if fmt == "UYVY" else (L.PF_V210, po.IN_V210, pack_v210(y, u, v, low))
    got = hip.dxt_encode(pf, L.DXT5_YCOCG, torch.from_numpy(src).cuda(), w, -h).cpu().numpy()
    assert np.array_equal(got, po.dxt_encode(pin, po.OUT_DXT5YCOCG, src, w, -h, ties="even")), fmt


def flat_beside_uncertified(po, size):
    w, h = size
    rng = np.random.default_rng(83)
    flats = rng.integers(0, 256, (16, 3))

    def blocks_at(n, cut):
        pool = slot_blocks(po, cut)
        yv, uv_, vv_ = flats[n % len(flats)]
        flat = (np.full((4, 4), yv), np.full((4, 2), uv_), np.full((4, 2), vv_))
        return [pool[sorted(pool)[n % len(pool)]], flat]
    for fmt in FORMATS:
        frame = build(po, fmt, w, h, blocks_at)
        s, near = check(po, "flat_beside_uncertified", fmt, w, h, frame, 1)
        assert (s["flat"] & frame[3]).sum() == frame[3].sum() // 2 and not near[s["flat"]].any()


def projection_frame_through_the_slot_counter(po, name, size):
    w, h = size
    y, u, v = PROJECTION_FRAMES[name][0](po, w, h)
    for fmt in FORMATS:
        st, evaluations, bad = run(po, name, fmt, (y, u, v), w, h)
        assert not bad, bad
        if name == "near_bisectors":
            assert st[3] == wave_evaluations(fmt, w, h) and st[3] <= evaluations <= 8 * st[3], (fmt, st, evaluations)
        else:
            assert st[3] == 0 and evaluations == 0, (fmt, st, evaluations)


def test_slot_counter_and_its_resets(hip, po):
    from ultragrid_amd import lib as L
    so = L.load()
    w, h = SIZES[0]
    (y, u, v), _, near, _ = build(po, "UYVY", w, h, lambda n, cut: [short_segment_pool(po, cut)[0][0]])
    src = pack_uyvy(y, u, v)
    waves, slots = expected(near, "UYVY")
    n, two, four = C.c_ulonglong(0), (C.c_ulonglong * 2)(), (C.c_ulonglong * 4)()
    read = lambda reset: (so.ug_hip_dxt_encode_stats_pair_slots(C.byref(n), reset), int(n.value))
    _, st = encode(so, L.PF_UYVY, src, w, h, L.TIES_EVEN, po, reset=False)
    assert st[3] == waves and read(0) == (0, slots) and read(1) == (0, slots) and read(0) == (0, 0)   # its own reset returns the count and clears it
    assert so.ug_hip_dxt_encode_stats_pair_slots(None, 0) == 0
    assert so.ug_hip_dxt_encode_stats_ex(four, 4, 0) == 0 and int(four[3]) == 0                         # ... and the older counters with it
    encode(so, L.PF_UYVY, src, w, h, L.TIES_EVEN, po, reset=False)
    assert read(0) == (0, slots) and so.ug_hip_dxt_encode_stats(two, 1) == 0 and read(0) == (0, 0)       # the oldest reset clears it
    encode(so, L.PF_UYVY, src, w, h, L.TIES_EVEN, po, reset=False)
    assert read(0) == (0, slots) and so.ug_hip_dxt_encode_stats_ex(None, 0, 1) == 0 and read(0) == (0, 0)   # and so does this one
    assert so.ug_hip_dxt_encode_stats_ex(four, 5, 0) != 0   # n = 5 stays refused


def rehoused_counters_still_count_every_wave(po, size):
    """colour full form, alpha full form and exact covariance are kept in slotted lines now: on the frames that put every wave there the
    sums are every wave, through either function, and a reset clears them"""
    from ultragrid_amd import lib as L
    so = L.load()
    w, h = size
    frames = {"cov_near_zero": (COV_FRAMES["near_zero"][0](w, h), (2,)), "cov_one_chroma_extreme_luma": (COV_FRAMES["one_chroma_extreme_luma"][0](w, h), (0, 2))}
    if (w, h) == SIZES[0]:
        frames["short_segments_one_luma"] = (frames_for(w, h)["short_segments_one_luma"], (0, 1))   # both full forms in every wave
    for name, ((y, u, v), full) in frames.items():
        low = np.random.default_rng(99 + w).integers(0, 4, (h, 2 * w)).astype(np.uint32)
        for fmt, pf, src in (("UYVY", L.PF_UYVY, pack_uyvy(y, u, v)), ("v210", L.PF_V210, pack_v210(y, u, v, low))):
            _, st = encode(so, pf, src, w, h, L.TIES_EVEN, po, reset=False)
            two = (C.c_ulonglong * 2)()
            assert so.ug_hip_dxt_encode_stats(two, 0) == 0 and (int(two[0]), int(two[1])) == st[:2], (name, fmt, st)
            print(f"{name} {fmt} {w}x{h}: {st} of {wave_evaluations(fmt, w, h)} waves")
            for i in full:
                assert st[i] == wave_evaluations(fmt, w, h), (name, fmt, i, st)
            assert so.ug_hip_dxt_encode_stats(two, 1) == 0 and so.ug_hip_dxt_encode_stats(two, 0) == 0 and (int(two[0]), int(two[1])) == (0, 0)
            four = (C.c_ulonglong * 4)()
            assert so.ug_hip_dxt_encode_stats_ex(four, 4, 0) == 0 and [int(x) for x in four] == [0, 0, 0, 0]


# One pytest item per frame kind (one_slot: per size): the sizes, formats and slots are looped over inside, every assertion names its case.
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_slot(hip, po, size):
    for k in range(8):
        one_slot(po, k, size)


def test_two_lanes_two_slots(hip, po):
    for size in SIZES:
        two_lanes_two_slots(po, size)


def test_all_slots(hip, po):
    for size in SIZES:
        all_slots(po, size)


def test_misdecided(hip, po):
    for size in SIZES:
        misdecided(po, size)
    for fmt in FORMATS:
        misdecided_mirrored(hip, po, fmt)


def test_flat_beside_uncertified(hip, po):
    for size in SIZES:
        flat_beside_uncertified(po, size)


def test_frames_of_the_projection_test_through_the_slot_counter(hip, po):
    for name in PROJECTION_FRAMES:
        for size in SIZES:
            projection_frame_through_the_slot_counter(po, name, size)


def test_rehoused_counters_still_count_every_wave(hip, po):
    for size in SIZES:
        rehoused_counters_still_count_every_wave(po, size)
