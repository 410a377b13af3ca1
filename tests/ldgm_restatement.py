"""numpy restatement of the reference's LDGM coder (ldgm/src/ldgm-session{,-cpu}.cpp): the buffer layout of encode_hdr_frame, the staircase
encoder, the CPU session's 4-sweep decoder and its valid_data rule, and peeling to the fixpoint (what ug_hip_ldgm_decode recovers).

pcm: (m, w_f) int32, rows padded with -1; row r lists its data packets (< k), then parity k + r and k + r - 1.
A buffer: (k + m) packets of ps bytes -- a 4-byte size header, the payload, zero padding to a multiple of 4 k, then the parity.
"""
import numpy as np


def packet_size(payload: int, k: int) -> int:
    """LDGM_session::encode_hdr_frame: header + payload rounded up to a multiple of 4 k, divided by k"""
    return -(-(payload + 4) // (4 * k)) * 4


def frame_buffer(payload: bytes, k: int, m: int) -> np.ndarray:
    ps = packet_size(len(payload), k)
    buf = np.zeros((k + m) * ps, np.uint8)
    buf[:4] = np.frombuffer(np.int32(len(payload)).tobytes(), np.uint8)
    buf[4: 4 + len(payload)] = np.frombuffer(payload, np.uint8)
    return buf


def encode(buf: np.ndarray, k: int, m: int, pcm: np.ndarray) -> np.ndarray:
    """LDGM_session_cpu::encode: parity p_r = s_0 ^ ... ^ s_r, s_r = XOR of row r's data packets.  Returns a copy with the parity written."""
    ps = buf.size // (k + m)
    out = buf.copy().reshape(k + m, ps)
    acc = np.zeros(ps, np.uint8)
    for r in range(m):
        for idx in pcm[r]:
            if 0 <= idx < k:
                acc ^= out[idx]
        out[k + r] = acc
    return out.reshape(-1)


def received_from_intervals(valid: dict, k: int, m: int, ps: int) -> np.ndarray:
    """decode_frame's valid_data rule (ldgm-session-cpu.cpp:316-380): entries whose end meets the next one's start merge; packet i counts
    as received if the last merged interval starting at or before i * ps reaches (i + 1) * ps."""
    merged = []
    items = sorted(valid.items())
    i = 0
    while i < len(items):
        start, length = items[i]
        i += 1
        while i < len(items) and start + length == items[i][0]:
            length += items[i][1]
            i += 1
        merged.append((start, length))
    rx = np.zeros(k + m, np.uint8)
    starts = [s for s, _ in merged]
    for p in range(k + m):
        j = int(np.searchsorted(starts, p * ps, side="right")) - 1
        if j >= 0 and merged[j][0] + merged[j][1] >= (p + 1) * ps:
            rx[p] = 1
    return rx


def _members(pcm, r):
    return [int(x) for x in pcm[r] if x > -1]


def decode_sweeps(buf: np.ndarray, k: int, m: int, pcm: np.ndarray, received: np.ndarray, sweeps: int = 4):
    """LDGM_session_cpu::decode_frame: missing data packets zeroed, then up to `sweeps` passes over the rows in order (a packet recovered
    in a pass is known for the rows after it).  Returns (buffer after decoding, frame_size, done flags of the k + m packets)."""
    ps = buf.size // (k + m)
    out = buf.copy().reshape(k + m, ps)
    done = received.astype(bool).copy()
    out[:k][~done[:k]] = 0
    it = 0
    changed = True
    while not done[:k].all() and it < sweeps and changed:  # (a sweep that recovers nothing leaves every later one nothing to do)
        changed = False
        for r in range(m):
            mem = _members(pcm, r)
            unknown = [j for j in mem if not done[j]]
            if len(unknown) != 1:
                continue
            t = unknown[0]
            acc = np.zeros(ps, np.uint8)
            count = 0
            for j in mem:
                if j != t:
                    acc ^= out[j]
                    count += 1
            out[t] = acc
            if count > 0:
                done[t] = True
                changed = True
        it += 1
    fs = int(out.reshape(-1)[:4].view("<i4")[0]) if done[:k].all() else 0
    return out.reshape(-1), fs, done


def peel_fixpoint(k: int, m: int, pcm: np.ndarray, received: np.ndarray) -> np.ndarray:
    """The packets known after peeling to the fixpoint (a row whose members are all known but one recovers it; a row with one member
    recovers nothing, as in the reference)."""
    known = received.astype(bool).copy()
    rows = [_members(pcm, r) for r in range(m)]
    changed = True
    while changed:
        changed = False
        for mem in rows:
            unknown = [j for j in mem if not known[j]]
            if len(unknown) == 1 and len(mem) >= 2:
                known[unknown[0]] = True
                changed = True
    return known


def decode_fixpoint(buf: np.ndarray, k: int, m: int, pcm: np.ndarray, received: np.ndarray):
    """decode_sweeps with as many sweeps as it takes: the bytes ug_hip_ldgm_decode recovers"""
    return decode_sweeps(buf, k, m, pcm, received, sweeps=k + m + 1)
