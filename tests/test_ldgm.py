"""CPU: LDGM FEC -- the numpy restatement (tests/ldgm_restatement.py) against the reference's CPU session (tests/golden/ldgm_ref.npz, and a
live run where the reference tree exists), the C ABI's argument checks (no GPU needed), and the built harness / plugin."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from ultragrid_amd import lib

import ldgm_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ldgm_ref.npz")
REF = "/root/reference"
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ug_ldgm_harness")
PLUGIN = os.path.join(ROOT, "oracle", "_ref", "ultragrid_ldgm_gpu.so")


def _configs():
    z = np.load(GOLDEN)
    n = len([f for f in z.files if f.startswith("kmcs")])
    return z, range(n)


def test_fixture_covers_the_configurations():
    z, idx = _configs()
    kmcs = {tuple(int(x) for x in z[f"kmcs{i}"][:3]) for i in idx}
    assert (512, 384, 5) in kmcs                                     # ldgm.cpp defaults
    assert {(750, 120, 5), (1500, 450, 6), (1000, 500, 7), (1500, 750, 8), (1500, 1500, 8)} <= kmcs   # suggested_configurations
    assert len(kmcs) >= 8


@pytest.mark.parametrize("i", range(8))
def test_restatement_encode_equals_the_reference(i):
    z, _ = _configs()
    k, m = (int(x) for x in z[f"kmcs{i}"][:2])
    buf, pcm = z[f"buf{i}"], z[f"pcm{i}"]
    ps = buf.size // (k + m)
    payload = int(buf[:4].view("<i4")[0])
    assert ps == R.packet_size(payload, k) and ps % 4 == 0
    fresh = buf.copy()
    fresh[k * ps:] = 0
    assert np.array_equal(R.encode(fresh, k, m, pcm), buf)


@pytest.mark.parametrize("i", range(8))
def test_restatement_decode_equals_the_reference(i):
    z, _ = _configs()
    k, m = (int(x) for x in z[f"kmcs{i}"][:2])
    buf, pcm = z[f"buf{i}"], z[f"pcm{i}"]
    ps = buf.size // (k + m)
    for rx, fs, dec in zip(z[f"rx{i}"], z[f"fs{i}"], z[f"dec{i}"]):
        lossy = buf.copy().reshape(k + m, ps)
        lossy[rx == 0] = 0xA5
        out, got_fs, done = R.decode_sweeps(lossy.reshape(-1), k, m, pcm, rx)
        assert got_fs == fs
        assert np.array_equal(out[: k * ps], dec)
        # the fixpoint recovers at least what 4 sweeps do, and every recovered data packet is the original
        known = R.peel_fixpoint(k, m, pcm, rx)
        assert (known | ~done).all()
        outf, fsf, donef = R.decode_fixpoint(lossy.reshape(-1), k, m, pcm, rx)
        assert np.array_equal(donef[:k], known[:k])  # (the sweeps stop once every data packet is known)
        d = outf.reshape(k + m, ps)[:k]
        assert np.array_equal(d[known[:k]], buf.reshape(k + m, ps)[:k][known[:k]])


def test_valid_data_rule():
    k, m, ps = 4, 2, 8
    # adjacent entries merge; a packet counts only if ONE merged interval covers it; overlapping entries do not merge
    rx = R.received_from_intervals({0: 4, 4: 4, 8: 3, 16: 8, 24: 20, 40: 4}, k, m, ps)
    assert rx.tolist() == [1, 0, 1, 1, 1, 0]
    rx = R.received_from_intervals({0: 12, 8: 8, 32: 16}, k, m, ps)
    assert rx.tolist() == [1, 1, 0, 0, 1, 1]


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "ldgm")), reason="needs the reference tree")
def test_fixture_equals_a_live_run_of_the_reference():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_ldgm_golden as G
    live = G.generate(REF)
    z = np.load(GOLDEN)
    assert set(live) == set(z.files)
    for name in z.files:
        assert np.array_equal(live[name], z[name]), name


def _refused(rc, what):
    assert rc == lib.EINVAL, what
    return lib.last_error()


def test_abi_refuses_bad_arguments_without_a_gpu():
    l = lib.load()
    s = C.c_void_p()
    pcm = np.full((4, 4), -1, np.int32)
    pcm[:, 0] = [0, 1, 2, 3]
    pcm[:, 1] = [4, 5, 6, 7]
    pp = pcm.ctypes.data
    assert "k must" in _refused(l.ug_hip_ldgm_create(0, 0, 4, pp, 4, C.byref(s)), "k = 0")
    assert "k must" in _refused(l.ug_hip_ldgm_create(0, 8192, 4, pp, 4, C.byref(s)), "k > 8191")
    assert "k must" in _refused(l.ug_hip_ldgm_create(0, 4, 0, pp, 4, C.byref(s)), "m = 0")
    assert "w_f" in _refused(l.ug_hip_ldgm_create(0, 4, 4, pp, 1, C.byref(s)), "w_f < 2")
    assert "w_f" in _refused(l.ug_hip_ldgm_create(0, 4, 4, pp, 129, C.byref(s)), "w_f > 128")
    assert "NULL" in _refused(l.ug_hip_ldgm_create(0, 4, 4, None, 4, C.byref(s)), "NULL pcm")
    assert "device" in _refused(l.ug_hip_ldgm_create(-1, 4, 4, pp, 4, C.byref(s)), "device < 0")
    for bad in (-2, 8):
        p2 = pcm.copy()
        p2[2, 3] = bad
        assert "pcm entry" in _refused(l.ug_hip_ldgm_create(0, 4, 4, p2.ctypes.data, 4, C.byref(s)), f"pcm entry {bad}")
    assert s.value is None
    rx = np.ones(8, np.uint8)
    ok = C.c_int()
    for ps in (0, -4, 6, 65536, 65540):
        assert "packet size" in _refused(l.ug_hip_ldgm_encode(None, 16, ps, None), f"ps {ps}")
        assert "packet size" in _refused(l.ug_hip_ldgm_encode_host(None, 16, ps, None), f"ps {ps}")
        assert "packet size" in _refused(l.ug_hip_ldgm_decode(None, 16, ps, rx.ctypes.data, None, C.byref(ok), None), f"ps {ps}")
        assert "packet size" in _refused(l.ug_hip_ldgm_decode_host(None, 16, ps, rx.ctypes.data, None, C.byref(ok), None), f"ps {ps}")
    assert "NULL" in _refused(l.ug_hip_ldgm_encode(None, 16, 64, None), "NULL session")
    assert "NULL" in _refused(l.ug_hip_ldgm_stats(None, None, None, None), "NULL session")
    l.ug_hip_ldgm_destroy(None)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src")), reason="needs the reference tree")
def test_harness_and_plugin_are_built():
    assert os.path.exists(HARNESS) and os.path.exists(PLUGIN)
    # the library registers itself from a static constructor and needs the C ABI of libug_mi355x.so
    und = subprocess.run(["nm", "-D", "--undefined-only", PLUGIN], capture_output=True, text=True, check=True).stdout
    assert "ug_hip_ldgm_encode_host" in und and "ug_hip_ldgm_decode_host" in und and "register_library" in und


@pytest.mark.skipif(not os.path.exists(HARNESS), reason="oracle/_ref/ug_ldgm_harness not built")
def test_harness_cpu_session_equals_the_restatement(tmp_path):
    """the reference's own ldgm class, CPU session, through the harness: the buffer is the restatement's, matrix in a directory of ours"""
    rng = np.random.default_rng(5)
    payload = rng.integers(0, 256, 7000, dtype=np.uint8)
    (tmp_path / "p.bin").write_bytes(payload.tobytes())
    env = dict(os.environ, UG_LDGM_MATRIX_DIR=str(tmp_path))
    r = subprocess.run([HARNESS, "encode", "256", "128", "5", "1", str(tmp_path / "p.bin"), str(tmp_path / "e.bin")],
                       capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stderr
    mat = tmp_path / "ldgm_matrix-256-128-5-1.bin"
    assert mat.exists()
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_ldgm_golden as G
    _, _, _, pcm = G.read_matrix(str(mat))
    buf = np.fromfile(tmp_path / "e.bin", np.uint8)
    hdr_len = 24  # the video payload header in front of the tile (ldgm.cpp:447-455)
    want = R.encode(R.frame_buffer(buf[4: 4 + hdr_len].tobytes() + payload.tobytes(), 256, 128), 256, 128, pcm)
    assert np.array_equal(buf, want)
