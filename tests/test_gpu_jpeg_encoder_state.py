"""The state a JPEG encoder carries from call to call: the colour-stage buffer, the slot buffer, the buffers of the wave-per-segment path
(freed whenever a larger batch grows the work buffers), the buffers of the lane-per-block coders, the generation counter of the look-back
words and the batch capacity.  One long-lived encoder per configuration is walked through a fixed sequence of calls; after every call each
stream must be the stream a FRESH encoder gives for that frame in a one-frame call (fresh encoders are pinned to the test writers and to
libjpeg elsewhere in the suite).  tests/test_gpu_jpeg.py::test_batches_of_varying_size_on_one_encoder does this for 4:2:x UYVY batches only."""
import pytest

from ultragrid_amd import lib as L
from ultragrid_amd import synth

pytestmark = pytest.mark.gpu

W, H = 208, 88           # 13 x 6 MCUs at 4:2:0: a short last workgroup and a short last segment
CALLS = (1, 3, 1, 16, 2, 1)  # frames per call; the third one reads its frame 4 bytes into a larger allocation (UYVY, RGBA)
N = 16

# id: (subsampling, input, internal_cs, flags, restart, quality, noise)
CONFIGS = {
    "420-uyvy-r4": (420, "UYVY", 0, 0, 4, 75, False),
    "422-uyvy-bt601-r4": (422, "UYVY", L.JPEG_CS_YCBCR_BT601, 0, 4, 75, False),                  # the colour stage -> cs_tmp
    "444-uyvy-r8": (444, "UYVY", 0, L.JPEG_INPUT_UYVY, 8, 75, False),                             # UYVY -> 4:4:4 -> cs_tmp
    "444-rgb-nonint-r8": (444, "RGB", 0, L.JPEG_NONINTERLEAVED, 8, 75, False),
    "420-rgb-nonint-r50": (420, "RGB", 0, L.JPEG_INPUT_RGB | L.JPEG_NONINTERLEAVED, 50, 75, False),  # segments of 50 blocks of one component: the block coder
    "420-uyvy-r0": (420, "UYVY", 0, 0, 0, 75, False),                                             # one segment: the one-segment parallel coder
    "420-uyvy-r50": (420, "UYVY", 0, 0, 50, 75, False),                                           # 300 blocks per segment, two segments: the segment-parallel fill
    "4444-rgba-r8": (4444, "RGBA", 0, 0, 8, 75, False),
    "420-uyvy-q100-noise-r4": (420, "UYVY", 0, 0, 4, 100, True),                                  # > 64 bytes per block: batches overflow their slots
}
PF = {"UYVY": L.PF_UYVY, "RGB": L.PF_RGB, "RGBA": L.PF_RGBA}
_cache = {}


def _frames_and_reference(hip, name):
    """16 distinct frames of the configuration on the device, and the stream of each from an encoder of its own (computed once)."""
    import numpy as np
    import torch
    if name not in _cache:
        sub, fmt, cs, flags, ri, q, noise = CONFIGS[name]
        line = synth.linesize(fmt, W)
        if noise:
            host = np.stack([synth.s1_random(fmt, W, H, salt=f) for f in range(N)])
        else:
            base = synth.s2_video("UYVY", W, H) if fmt == "UYVY" else synth.s1_random(fmt, W, H)
            host = np.stack([np.roll(base, line * 5 * f) for f in range(N)])
        dev = torch.from_numpy(host).cuda()
        want = []
        for f in range(N):
            fresh = hip.JpegEncoder(W, H, q, ri, subsampling=sub, internal_cs=cs, flags=flags)
            want.append(fresh.encode(dev[f], PF[fmt]))
            fresh.close()
        assert len(set(want)) == N
        _cache[name] = (dev, want)
    return _cache[name]


def _walk(hip, name):
    import torch
    sub, fmt, cs, flags, ri, q, _ = CONFIGS[name]
    dev, want = _frames_and_reference(hip, name)
    enc = hip.JpegEncoder(W, H, q, ri, subsampling=sub, internal_cs=cs, flags=flags)
    first = 0
    for call, n in enumerate(CALLS):
        idx = [(first + i) % N for i in range(n)]
        first += n + 1
        if n == 1:
            src = dev[idx[0]]
            if call == 2 and fmt != "RGB":  # an aligned frame ran fused just before: now the unfused front end (UYVY), a misaligned source (RGBA)
                big = torch.zeros(src.numel() + 64, dtype=torch.uint8, device="cuda")
                big[4:4 + src.numel()] = src
                src = big[4:4 + src.numel()]
                assert src.data_ptr() % 16 == 4
            got = [enc.encode(src, PF[fmt])]
        else:
            got = enc.encode_batch(dev[idx].contiguous(), PF[fmt])
        for i, g in zip(idx, got):
            assert g == want[i], (name, call, n, i, len(g), len(want[i]))
    enc.close()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_one_encoder_through_calls_of_varying_size(hip, name):
    _walk(hip, name)


@pytest.mark.parametrize("name", ["420-rgb-nonint-r50", "420-uyvy-r50"])
def test_one_encoder_through_calls_of_varying_size_on_the_wave_per_segment_coder(hip, name, monkeypatch):
    """UG_JPEG_WAVE_KERNEL=1: entropy_wave_kernel + compact_kernel through the same sequence (at this picture size the segment-parallel fill
    takes every long interval otherwise).  The reference streams are those of the default path: the coders' streams are identical by design."""
    _frames_and_reference(hip, name)
    monkeypatch.setenv("UG_JPEG_WAVE_KERNEL", "1")
    _walk(hip, name)
