"""The slot form of the colour stage's reference side (dxt_encode.hip, encode_dxt5ycocg, chroma-pair loaders).  The certificate of the index
taken from the projection is per pair: `worst` is the maximum over a block's eight pairs and eps depends on the block's vv and dmax alone.
So a wave that holds an uncertified pair keeps the projection's index for every certified pair and evaluates the reference's two distances
only for the pixels of the pair slots (0 .. 7) in which one of its blocks holds an uncertified pair, and only the uncertified lanes take the
result.  This restates that form with the strict-fp32 model of tests/test_dxt_pair_projection_bound.py (projection_stage) -- per pair the
projection's index where the pair is certified, else the exact side's; flat and full-form blocks as before -- over every frame of contents()
and checks that
(a) the indices are the oracle's on every pixel,
(b) no pixel of a certified pair differs from the oracle, whatever the rest of its wave holds,
(c) S2 and S1 each hold uncertified pairs: the check is not vacuous,
(d) at most WAVE_SHARE_CAP of the waves of the video-like frame S2 hold an uncertified pair (the waves that take the side at all),
(e) such a wave evaluates fewer than 2 of its eight slots on average, on S2 and on S1: what the gain of the form rests on."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dxt_pair_linear_bound import contents  # noqa: E402
from test_dxt_pair_projection_bound import WAVE_SHARE_CAP, projection_stage, wave_share_uncertified  # noqa: E402

MEAN_SLOTS_CAP = 2.0


def slot_form(s):
    """-> (colour index per pixel in the slot form, uncertified pairs that reach the stage: (bh, bw, 8))"""
    live = (s["in_fast"] & ~s["flat"])[..., None]
    # the model's own index is the exact side's for every pair of a wave that holds an uncertified block, the flat form's in flat blocks and
    # the full form's outside the stage: an uncertified pair always lies in such a wave, so only certified pairs are replaced here
    keep = np.repeat(live & s["cert_pair"], 2, axis=-1)
    return np.where(keep, s["proj_idx"], s["idx"]), live & ~s["cert_pair"]


def slots_per_wave(uncertified):
    """per wave (64 consecutive blocks of a block row, UYVY's one block per lane): number of pair slots in which some lane is uncertified"""
    bh, bw, _ = uncertified.shape
    u = np.concatenate([uncertified, np.zeros((bh, (-bw) % 64, 8), bool)], axis=1).reshape(bh, -1, 64, 8)
    return u.any(2).sum(-1)


@pytest.fixture(scope="module")
def stages(po):
    return {name: projection_stage(po, *planes) for name, planes in contents().items()}


def test_slot_form_gives_the_oracles_indices(stages):
    assert len(stages) == 8
    for name, s in stages.items():
        idx, _ = slot_form(s)
        wrong = int((idx != s["want"]).sum())
        print(f"{name}: {wrong} of {idx.size} colour indices of the slot form differ from the oracle's")
        assert wrong == 0, (name, wrong)


def test_certified_pairs_keep_the_projections_index_in_any_wave(stages):
    for name, s in stages.items():
        live = (s["in_fast"] & ~s["flat"])[..., None]
        certified = np.repeat(live & s["cert_pair"], 2, axis=-1)
        wrong = int((certified & (s["proj_idx"] != s["want"])).sum())
        beside = np.repeat(~s["cert_block"] & s["in_fast"] & ~s["flat"], 16).reshape(certified.shape) & certified
        print(f"{name}: {int(certified.sum())} pixels in certified pairs, {wrong} differ from the oracle; {int(beside.sum())} of them share a block "
              f"with an uncertified pair; {int((live & ~s['cert_pair']).sum()) * 2} pixels in uncertified pairs")
        assert wrong == 0, (name, wrong)


def test_content_holds_uncertified_pairs(stages):
    for name in ("S2", "S1"):
        _, uncertified = slot_form(stages[name])
        pixels = 2 * int(uncertified.sum())
        print(f"{name}: {pixels} pixels in uncertified pairs")
        assert pixels > 0, name


def test_few_waves_take_the_side_and_few_slots_each(stages):
    share = wave_share_uncertified(stages["S2"])
    print(f"S2: {100 * share:.3f} % of waves hold an uncertified pair (cap {100 * WAVE_SHARE_CAP:.0f} %)")
    assert share <= WAVE_SHARE_CAP, share
    for name in ("S2", "S1"):
        n = slots_per_wave(slot_form(stages[name])[1])
        taken = n[n > 0]
        hist = {int(k): int((taken == k).sum()) for k in np.unique(taken)}
        print(f"{name}: {len(taken)} of {n.size} waves uncertified ({100 * len(taken) / n.size:.2f} %), mean {taken.mean():.4f} slots per such wave, "
              f"waves by slots {hist}")
        assert len(taken) > 0 and taken.mean() < MEAN_SLOTS_CAP, (name, float(taken.mean()))
    for name, s in stages.items():
        n = slots_per_wave(slot_form(s)[1])
        print(f"{name}: {int(n.sum())} slot evaluations in {int((n > 0).sum())} waves of {n.size}")
