"""GPU: the LDGM coder (ug_hip_ldgm_*, csrc/ldgm.hip) against the reference's CPU session (tests/golden/ldgm_ref.npz) and the numpy
restatement (tests/ldgm_restatement.py); and the ldgm_gpu library inside the reference's own `ldgm` class (oracle/_ref/ug_ldgm_harness)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, given, settings, strategies as st

from ultragrid_amd import codec, lib

import ldgm_restatement as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ldgm_ref.npz")
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ug_ldgm_harness")


def random_pcm(k, m, wf, rng):
    """rows as the reference's generator lays them out: data packets, then parity k + r and k + r - 1, padded with -1"""
    pcm = np.full((m, wf), -1, np.int32)
    for r in range(m):
        d = rng.choice(k, size=min(wf - 2, k), replace=False) if wf > 2 else []
        pcm[r, : len(d)] = d
        pcm[r, len(d)] = k + r
        if r > 0:
            pcm[r, len(d) + 1] = k + r - 1
    return pcm


def encode_np(buf, k, m, pcm):
    """the restatement's encode, vectorised over rows (R.encode is the row loop; equal by construction, checked below)"""
    ps = buf.size // (k + m)
    pk = buf.reshape(k + m, ps)
    s = np.zeros((m, ps), np.uint8)
    for j in range(pcm.shape[1]):
        idx = pcm[:, j]
        sel = (idx >= 0) & (idx < k)
        s[sel] ^= pk[idx[sel]]
    out = pk.copy()
    out[k:] = np.bitwise_xor.accumulate(s, axis=0)
    return out.reshape(-1)


def gpu_encode(coder, buf):
    t = torch.from_numpy(buf.copy()).cuda()
    coder.encode(t)
    return t.cpu().numpy()


def golden():
    z = np.load(GOLDEN)
    return z, len([f for f in z.files if f.startswith("kmcs")])


def test_encode_equals_the_reference_session():
    z, n = golden()
    for i in range(n):
        k, m = (int(x) for x in z[f"kmcs{i}"][:2])
        buf, pcm = z[f"buf{i}"], z[f"pcm{i}"]
        fresh = buf.copy()
        fresh[k * (buf.size // (k + m)):] = 0x5A  # whatever the parity region holds going in
        coder = codec.LdgmCoder(k, m, pcm)
        assert np.array_equal(gpu_encode(coder, fresh), buf), (i, k, m)
        assert coder.stats()["launches"] == 2 and coder.stats()["copies"] == 0


@pytest.mark.parametrize("k,m,wf,ps", [
    (64, 64, 5, 4), (64, 48, 8, 12), (512, 384, 9, 20), (300, 200, 128, 36), (1000, 500, 16, 148), (1500, 1500, 10, 4),
    (8191, 4000, 20, 8), (8191, 100, 128, 4), (64, 64, 7, 65532), (96, 80, 6, 65528), (128, 1000, 12, 1500), (257, 129, 3, 4148),
])
def test_encode_geometries(k, m, wf, ps):
    rng = np.random.default_rng(k * 7 + m + ps)
    pcm = random_pcm(k, m, wf, rng)
    buf = rng.integers(0, 256, (k + m) * ps, dtype=np.uint8)
    want = encode_np(buf, k, m, pcm)
    if k * ps <= 1 << 20 and m <= 1000:
        assert np.array_equal(want, R.encode(buf, k, m, pcm))
    assert np.array_equal(gpu_encode(codec.LdgmCoder(k, m, pcm), buf), want)


def test_encode_of_a_misaligned_device_buffer():
    """a buffer that starts 4 bytes into an allocation: the 4-byte column path, whatever ps is"""
    rng = np.random.default_rng(3)
    k, m, ps = 200, 100, 64
    pcm = random_pcm(k, m, 7, rng)
    buf = rng.integers(0, 256, (k + m) * ps, dtype=np.uint8)
    t = torch.zeros(buf.size + 4, dtype=torch.uint8, device="cuda")
    t[4:] = torch.from_numpy(buf).cuda()
    coder = codec.LdgmCoder(k, m, pcm)
    L = lib.load()
    lib.check(L.ug_hip_ldgm_encode(coder._h, t.data_ptr() + 4, ps, torch.cuda.current_stream().cuda_stream), "encode")
    assert np.array_equal(t[4:].cpu().numpy(), encode_np(buf, k, m, pcm))


@settings(max_examples=40, deadline=None, suppress_health_check=list(HealthCheck))
@given(k=st.integers(64, 2000), m=st.integers(64, 1500), wf=st.integers(3, 128), ps4=st.integers(1, 600), seed=st.integers(0, 2 ** 31))
def test_encode_hypothesis(k, m, wf, ps4, seed):
    rng = np.random.default_rng(seed)
    ps = 4 * ps4
    pcm = random_pcm(k, m, wf, rng)
    buf = rng.integers(0, 256, (k + m) * ps, dtype=np.uint8)
    assert np.array_equal(gpu_encode(codec.LdgmCoder(k, m, pcm), buf), encode_np(buf, k, m, pcm))


def check_decode(coder, clean, k, m, pcm, rx):
    """decode on the device against the restatement; returns (ours all known, the reference's 4 sweeps all known)"""
    ps = clean.size // (k + m)
    lossy = clean.copy().reshape(k + m, ps)
    lossy[rx == 0] = 0xA5
    t = torch.from_numpy(lossy.reshape(-1).copy()).cuda()
    rec, ok = coder.decode(t, rx)
    got = t.cpu().numpy().reshape(k + m, ps)
    known = R.peel_fixpoint(k, m, pcm, rx)
    rxb = rx.astype(bool)
    # the recovered data packets are exactly the fixpoint's, and byte for byte the originals
    assert np.array_equal(rec[:k], known[:k] & ~rxb[:k])
    assert ok == bool(known[:k].all())
    assert np.array_equal(got[:k][known[:k]], clean.reshape(k + m, ps)[:k][known[:k]])
    # packets that arrived are never written; parity is written only where recovered (and then correctly)
    assert np.array_equal(got[rxb], lossy[rxb])
    assert not (rec & rxb).any()
    assert np.array_equal(got[rec], clean.reshape(k + m, ps)[rec])
    # where the reference's 4 sweeps succeed, ours does, with the same bytes
    _, fs4, done4 = R.decode_sweeps(lossy.reshape(-1), k, m, pcm, rx)
    assert (known[:k] | ~done4[:k]).all()  # never less
    if fs4:
        assert ok and int(got[0, :4].view("<i4")[0]) == fs4
    return ok, bool(fs4)


def test_decode_equals_the_reference_session():
    z, n = golden()
    for i in range(n):
        k, m = (int(x) for x in z[f"kmcs{i}"][:2])
        buf, pcm = z[f"buf{i}"], z[f"pcm{i}"]
        ps = buf.size // (k + m)
        coder = codec.LdgmCoder(k, m, pcm)
        for rx, fs, dec in zip(z[f"rx{i}"], z[f"fs{i}"], z[f"dec{i}"]):
            ok, ref_ok = check_decode(coder, buf, k, m, pcm, rx)
            assert ref_ok == bool(fs)
            if fs:  # the reference decoded the frame: identical data region
                lossy = buf.copy().reshape(k + m, ps)
                lossy[rx == 0] = 0xA5
                t = torch.from_numpy(lossy.reshape(-1)).cuda()
                coder.decode(t, rx)
                assert np.array_equal(t.cpu().numpy()[: k * ps], dec)


@pytest.mark.parametrize("loss", [0.01, 0.05, 0.1, 0.2, 0.4])
def test_decode_random_losses(loss):
    z, n = golden()
    rng = np.random.default_rng(int(loss * 1000))
    for i in range(n):
        k, m = (int(x) for x in z[f"kmcs{i}"][:2])
        buf, pcm = z[f"buf{i}"], z[f"pcm{i}"]
        coder = codec.LdgmCoder(k, m, pcm)
        for _ in range(3):
            check_decode(coder, buf, k, m, pcm, (rng.random(k + m) >= loss).astype(np.uint8))


def test_decode_bursts_and_lost_parity_runs():
    z, n = golden()
    rng = np.random.default_rng(11)
    for i in range(n):
        k, m = (int(x) for x in z[f"kmcs{i}"][:2])
        buf, pcm = z[f"buf{i}"], z[f"pcm{i}"]
        coder = codec.LdgmCoder(k, m, pcm)
        for burst in (1, k // 50 + 1, k // 10):
            rx = np.ones(k + m, np.uint8)
            s = int(rng.integers(0, k - burst + 1))
            rx[s: s + burst] = 0
            run = int(rng.integers(1, m // 4 + 2))
            p = int(rng.integers(k, k + m - run + 1))
            rx[p: p + run] = 0
            check_decode(coder, buf, k, m, pcm, rx)


def test_fixpoint_recovers_where_four_sweeps_do_not():
    """an intended difference: a chain whose links run against the sweep order (row r recovers data 63 - r from data 62 - r) takes one
    sweep per link.  The reference gives up after 4 sweeps; peeling to the fixpoint recovers the whole frame."""
    k, m, ps = 64, 64, 16
    pcm = np.full((m, 4), -1, np.int32)
    for r in range(m):
        pcm[r, 0] = 63 - r
        if r < 63:
            pcm[r, 1] = 62 - r
        pcm[r, 2] = k + r
        if r > 0:
            pcm[r, 3] = k + r - 1
    rng = np.random.default_rng(2)
    clean = encode_np(rng.integers(0, 256, (k + m) * ps, dtype=np.uint8), k, m, pcm)
    rx = np.ones(k + m, np.uint8)
    rx[10:k] = 0
    coder = codec.LdgmCoder(k, m, pcm)
    ok, ref_ok = check_decode(coder, clean, k, m, pcm, rx)
    assert ok and not ref_ok
    assert coder.stats()["levels"] == 54  # one level per link: no host round trip between them


def test_no_loss_decode_issues_no_device_work():
    z, _ = golden()
    k, m = (int(x) for x in z["kmcs0"][:2])
    buf, pcm = z["buf0"], z["pcm0"]
    coder = codec.LdgmCoder(k, m, pcm)
    t = torch.from_numpy(buf.copy()).cuda()
    rx = np.ones(k + m, np.uint8)
    rx[k + 5: k + 20] = 0  # lost parity only: still nothing to do
    rec, ok = coder.decode(t, rx)
    assert ok and not rec.any()
    assert coder.stats() == dict(launches=0, copies=0, levels=0)
    # the host form likewise
    hb = buf.copy()
    okc = C.c_int()
    lib.check(lib.load().ug_hip_ldgm_decode_host(coder._h, hb.ctypes.data, buf.size // (k + m), rx.ctypes.data, None, C.byref(okc), None), "decode_host")
    assert okc.value == 1 and coder.stats() == dict(launches=0, copies=0, levels=0)
    # and with one data packet lost: schedule upload + a launch per level
    rx[3] = 0
    rec, ok = coder.decode(t, rx)
    st_ = coder.stats()
    assert ok and rec[3] and st_["copies"] == 1 and st_["launches"] == st_["levels"] >= 1


def test_host_forms_equal_the_device_forms():
    z, _ = golden()
    k, m = (int(x) for x in z["kmcs2"][:2])
    buf, pcm = z["buf2"], z["pcm2"]
    ps = buf.size // (k + m)
    coder = codec.LdgmCoder(k, m, pcm)
    L = lib.load()
    hb = buf.copy()
    hb[k * ps:] = 0
    lib.check(L.ug_hip_ldgm_encode_host(coder._h, hb.ctypes.data, ps, None), "encode_host")
    assert np.array_equal(hb, buf)
    assert coder.stats()["copies"] == 2 and coder.stats()["launches"] == 2
    rng = np.random.default_rng(9)
    rx = (rng.random(k + m) >= 0.05).astype(np.uint8)
    lossy = buf.copy().reshape(k + m, ps)
    lossy[rx == 0] = 0xA5
    hb = lossy.reshape(-1).copy()
    rec = np.zeros(k + m, np.uint8)
    okc = C.c_int()
    lib.check(L.ug_hip_ldgm_decode_host(coder._h, hb.ctypes.data, ps, rx.ctypes.data, rec.ctypes.data, C.byref(okc), None), "decode_host")
    known = R.peel_fixpoint(k, m, pcm, rx)
    h = hb.reshape(k + m, ps)
    assert np.array_equal(h[:k][known[:k]], buf.reshape(k + m, ps)[:k][known[:k]])
    # only the recovered data packets came back: lost parity stays as it was in the host buffer
    assert np.array_equal(h[k:], lossy[k:])
    assert coder.stats()["copies"] == 3  # buffer up, schedule up, recovered packets down


def test_two_sessions_on_two_streams():
    z, _ = golden()
    jobs = []
    for i in (3, 5):
        k, m = (int(x) for x in z[f"kmcs{i}"][:2])
        jobs.append((k, m, z[f"pcm{i}"], z[f"buf{i}"]))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    coders = [codec.LdgmCoder(k, m, pcm) for k, m, pcm, _ in jobs]
    rng = np.random.default_rng(4)
    outs, masks, bufs = [], [], []
    for rnd in range(4):
        for (k, m, pcm, buf), s, cd in zip(jobs, streams, coders):
            fresh = buf.copy()
            fresh[k * (buf.size // (k + m)):] = 0
            with torch.cuda.stream(s):
                t = torch.from_numpy(fresh).cuda(non_blocking=False)
                cd.encode(t)
                rx = (rng.random(k + m) >= 0.03).astype(np.uint8)
                t2 = t.clone()
                cd.decode(t2, rx)  # recovers in place from the encoded buffer (lost packets hold their true bytes anyway)
                outs.append((t, t2))
                masks.append(rx)
                bufs.append(buf)
    torch.cuda.synchronize()
    for (t, t2), buf in zip(outs, bufs):
        assert np.array_equal(t.cpu().numpy(), buf)
        assert np.array_equal(t2.cpu().numpy(), buf)


def test_coder_refuses_host_tensors():
    z, _ = golden()
    k, m = (int(x) for x in z["kmcs7"][:2])
    coder = codec.LdgmCoder(k, m, z["pcm7"])
    with pytest.raises(ValueError):
        coder.encode(torch.from_numpy(z["buf7"].copy()))


# ---- the ldgm_gpu library in the reference's own ldgm class ----

needs_harness = pytest.mark.skipif(not os.path.exists(HARNESS), reason="oracle/_ref/ug_ldgm_harness not built (needs /root/reference)")


def _h(tmp_path, args, gpu):
    env = dict(os.environ, UG_LDGM_MATRIX_DIR=str(tmp_path))
    env["UG_PARAM"] = "ldgm-device=GPU,mi355x-device=0" if gpu else "ldgm-device=CPU"
    r = subprocess.run([HARNESS] + [str(a) for a in args], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


@needs_harness
@pytest.mark.parametrize("k,m,c,size", [(512, 384, 5, 144000), (750, 120, 5, 177000), (1000, 500, 7, 1920 * 1080 * 2), (1500, 450, 6, 217000),
                                        (256, 256, 5, 1920), (64, 64, 3, 37)])  # the last two: audio-sized frames (ps 8 and 4)
def test_harness_gpu_equals_cpu_and_cross_decodes(tmp_path, k, m, c, size):
    rng = np.random.default_rng(size)
    (tmp_path / "p.bin").write_bytes(rng.integers(0, 256, size, dtype=np.uint8).tobytes())
    rc = _h(tmp_path, ["encode", k, m, c, 1, tmp_path / "p.bin", tmp_path / "cpu.bin"], False)
    rg = _h(tmp_path, ["encode", k, m, c, 1, tmp_path / "p.bin", tmp_path / "gpu.bin"], True)
    assert "[LDGM MI355X]" not in rg.stdout + rg.stderr
    cpu, gpu = (tmp_path / "cpu.bin").read_bytes(), (tmp_path / "gpu.bin").read_bytes()
    sym = lambda r: [l for l in r.stdout.splitlines() if l.startswith("symbol_size=")]  # (the CPU session prints a banner of its own)
    assert sym(rc) == sym(rg) and sym(rc) and cpu == gpu
    buf = np.frombuffer(cpu, np.uint8)
    ps = buf.size // (k + m)
    for loss in (0.0, 0.02, 0.05):
        rx = (rng.random(k + m) >= loss).astype(np.uint8)
        if loss == 0.05:
            rx[k + m // 2: k + m // 2 + m // 20] = 0
        lossy = buf.copy().reshape(k + m, ps)
        lossy[rx == 0] = 0xA5
        (tmp_path / "in.bin").write_bytes(lossy.tobytes())
        (tmp_path / "mask.bin").write_bytes(rx.tobytes())
        a = _h(tmp_path, ["decode", k, m, c, 1, tmp_path / "in.bin", tmp_path / "mask.bin", tmp_path / "dc.bin"], False)
        b = _h(tmp_path, ["decode", k, m, c, 1, tmp_path / "in.bin", tmp_path / "mask.bin", tmp_path / "dg.bin"], True)
        dc, dg = (tmp_path / "dc.bin").read_bytes(), (tmp_path / "dg.bin").read_bytes()
        if "ok=1" in a.stdout:  # the CPU session decoded it (a GPU-encoded stream, byte-identical): so does the library, identically
            assert "ok=1" in b.stdout and dc == dg
            assert np.array_equal(np.frombuffer(dg, np.uint8)[4:], buf[: k * ps])
        assert ("ok=1" in b.stdout) or ("ok=1" not in a.stdout)


@needs_harness
def test_harness_refuses_packets_above_65535_bytes(tmp_path):
    """k = 64 and a 4.2 MB frame: 65540 B packets, which LDGM_session::packet_size (unsigned short) cannot hold"""
    k, m = 64, 64
    size = 64 * 65540 - 4 - 24
    (tmp_path / "p.bin").write_bytes(bytes(size))
    r = _h(tmp_path, ["encode", k, m, 3, 1, tmp_path / "p.bin", tmp_path / "gpu.bin"], True)
    out = r.stdout + r.stderr
    assert "65535" in out and "parity not computed" in out
    buf = np.frombuffer((tmp_path / "gpu.bin").read_bytes(), np.uint8)
    assert buf.size == (k + m) * 65540 and not buf[k * 65540:].any()
