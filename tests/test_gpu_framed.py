"""GPU: length-prefixed stream framing on CipherState tables --
noise_gpu_framed_seal / noise_gpu_framed_open (csrc/framed_kernels.hip,
csrc/framed_calls.hpp).

A connection carries frames pack('>H', len + 16) + ct || tag under its session's
key and in-order nonce.  Expected frames come from the CPU oracle and the plain
rules of include/noise_gpu.h written out in Python below (the walk, the slots
under max_rec, n++ per record of a session in slot order, refused at 2^64-2);
neither is the code under test.

Shapes: 65 connections (two waves) and 300 (five tiles over the scan), 0 to
about 40 frames each, L of 16, 17, 79, 80, 1040 and 65535, tails of 0, 1 and 2
bytes and a frame less its last byte, bad lengths 0 and 15 first, in the middle
and last, max_rec at the total, one below, inside a connection, 1 and 70 above,
offsets 0, 1, 2 and 14 mod 16; 4200 records of 0 to 65519 bytes for the
classified records path (threshold 2048) on unaligned records."""
import os
import struct
import subprocess

import numpy as np
import pytest

import noise_amd

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

OK, BAD_MAC, BAD_KEY, NONCE = noise_amd.REC_OK, noise_amd.REC_BAD_MAC, noise_amd.REC_BAD_KEY, noise_amd.REC_NONCE
EMPTY = getattr(noise_amd, "REC_EMPTY", 6)
F_OK, F_BAD_LEN, F_FULL, F_REFUSED = 0, 1, 2, 3
LIMIT = (1 << 64) - 2
REC = noise_amd.record_dtype()
MISALIGN = np.array([0, 1, 2, 14])  # connection offsets mod 16, by connection index mod 4
CANARY = 0xA5
LS = [16, 17, 79, 80, 1040]


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    noise_amd.load()
    torch.cuda.set_device(0)


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def _host(t, dtype=np.uint8):
    return t.cpu().numpy().view(dtype)


def _fill(n, value, dtype=torch.uint8):
    return torch.full((n,), value, dtype=dtype, device="cuda")


def make_keys(nsess, rng, keyless=()):
    keys = rng.integers(0, 256, (nsess, 32), dtype=np.uint8)
    keys[:, 0] |= 1
    for s in keyless:
        keys[s] = 0
    return keys


def make_table(keys, ctr):
    t = noise_amd.CipherStateTable(len(keys))
    t.set(0, len(keys), _dev(keys.reshape(-1)), 32, _dev(np.asarray(ctr, np.uint64)))
    return t


def counters(t):
    d = torch.zeros(t.nsess, dtype=torch.int64, device="cuda")
    t.get(0, t.nsess, d_n=d)
    torch.cuda.synchronize()
    return _host(d, np.uint64).copy()


def place(sizes, gap=16):
    """Offsets of ranges of `sizes` bytes, at least `gap` canary bytes apart, at 0, 1, 2, 14 mod 16."""
    off, at = [], 16
    for j, n in enumerate(sizes):
        at = (at + 15) // 16 * 16 + int(MISALIGN[j % 4])
        off.append(at)
        at += int(n) + gap
    return np.array(off, np.uint64), at + 16


def host_frames(oracle, key, n0, plains):
    """What transport::append_frame makes of consecutive encrypt_with_ad outputs."""
    out = b""
    for k, p in enumerate(plains):
        ct = oracle.encrypt(key, n0 + k, b"", p)
        out += struct.pack(">H", len(ct)) + ct
    return out


# ---- the plain loops ---------------------------------------------------------------
def walk(b):
    pos, frames, bad = 0, [], False
    while True:
        if len(b) - pos < 2:
            break
        L = b[pos] << 8 | b[pos + 1]
        if L < 16:
            bad = True
            break
        if len(b) - pos - 2 < L:
            break
        frames.append((pos, L))
        pos += 2 + L
    return frames, bad


def assign_slots(count, max_rec):
    first, nframes, total = [], [], 0
    for c in count:
        f = min(total, max_rec)
        first.append(f)
        nframes.append(min(c, max_rec - f))
        total += c
    return first, nframes, total


def next_nonce(keys, ctr, s):
    """CipherState's rule for the next record of session s: (status, nonce)."""
    if s >= len(keys) or not keys[s].any():
        return BAD_KEY, 0
    if int(ctr[s]) == LIMIT:
        return NONCE, 0
    n = int(ctr[s])
    ctr[s] = (n + 1) % (1 << 64)
    return OK, n


def cap_of(which, count):
    total = sum(count)
    if which == "mid":  # inside the first connection of three frames or more behind the middle
        run = 0
        for c in count:
            if run >= total // 2 and c >= 3:
                return run + 1
            run += c
        return max(total - 2, 1)
    return {"total": max(total, 1), "total-1": max(total - 1, 1), "one": 1, "total+70": total + 70}[which]


# ---- open ----------------------------------------------------------------------------
def run_open(t, keys, ctr, sess, conns, cap, in_place, oracle, len_sum=0):
    """conns: the received bytes of each connection.  Checks everything the call
    writes against the loops; ctr is moved.  Returns (statuses, plaintext per connection, consumed)."""
    nconn = len(conns)
    walked = [walk(b) for b in conns]
    count = [len(w[0]) for w in walked]
    max_rec = cap if isinstance(cap, int) else cap_of(cap, count)
    first, nframes, total = assign_slots(count, max_rec)
    taken = min(total, max_rec)
    woff, wtotal = place([len(b) for b in conns])
    plen = [sum(L - 16 for _, L in walked[j][0][:nframes[j]]) for j in range(nconn)]
    poff, ptotal = place(plen)
    wire = np.full(wtotal, CANARY, np.uint8)
    for j, b in enumerate(conns):
        wire[int(woff[j]):int(woff[j]) + len(b)] = np.frombuffer(b, np.uint8)
    want_out = wire.copy() if in_place else np.full(ptotal, CANARY, np.uint8)
    skip = np.zeros(len(want_out), bool)
    want_st = np.full(max_rec, EMPTY, np.uint8)
    want = np.zeros(max_rec, REC)
    want["key_idx"][taken:], want["reserved"][taken:] = 0xffffffff, EMPTY
    first_bad, consumed, cstat, plains = list(nframes), [0] * nconn, [F_OK] * nconn, [b""] * nconn
    for j in range(nconn):
        at = 0
        for k in range(nframes[j]):
            pos, L = walked[j][0][k]
            i = first[j] + k
            in_off = int(woff[j]) + pos + 2
            out_off = in_off if in_place else int(poff[j]) + at
            st, n = next_nonce(keys, ctr, int(sess[j]))
            if st == OK:
                p = oracle.decrypt(keys[int(sess[j])].tobytes(), n, b"", conns[j][pos + 2:pos + 2 + L])
                if p is None:
                    st = BAD_MAC
                    if not in_place:
                        want_out[out_off:out_off + L - 16] = 0
                else:
                    want_out[out_off:out_off + L - 16] = np.frombuffer(p, np.uint8)
                    skip[out_off + L - 16:out_off + L] = in_place  # the tag's bytes after an in-place decrypt are unspecified
                    plains[j] += p
            want_st[i] = st
            want[i] = (in_off, out_off, n, 0, L - 16, 0, int(sess[j]), 0)
            if st != OK and first_bad[j] == nframes[j]:
                first_bad[j] = k
            at += L - 16
            consumed[j] += 2 + L
        cstat[j] = F_FULL if nframes[j] < count[j] else F_BAD_LEN if walked[j][1] else F_OK

    d_wire, d_plain = _dev(wire), _fill(ptotal, CANARY)
    d_woff, d_wlen, d_poff = _dev(woff), _dev(np.array([len(b) for b in conns], np.uint32)), _dev(poff)
    d_recs, d_st, d_sess = _fill(48 * max_rec, 0x77), _fill(max_rec, 0x77), _dev(np.asarray(sess, np.uint32))
    d_first, d_nfr, d_fb = _fill(nconn, -1, torch.int64), _fill(nconn, -1, torch.int32), _fill(nconn, -1, torch.int32)
    d_cons, d_plen, d_cst = _fill(nconn, -1, torch.int64), _fill(nconn, -1, torch.int64), _fill(nconn, 0x77)
    d_total = _fill(1, -1, torch.int64)
    t.open_framed(d_sess, noise_amd.span(d_wire, off=d_woff, lens=d_wlen), d_recs, d_st, max_rec, d_nfr, d_cons,
                  d_cst, nconn, plain=None if in_place else noise_amd.span(d_plain, off=d_poff), d_first=d_first,
                  d_first_bad=d_fb, d_plain_len=d_plen, d_total=d_total, len_sum=len_sum)
    torch.cuda.synchronize()
    got_st, got = _host(d_st), _host(d_recs).view(REC)
    assert np.array_equal(got_st, want_st), (np.flatnonzero(got_st != want_st)[:5], got_st[:8], want_st[:8])
    for f in ("in_off", "out_off", "len", "ad_len", "key_idx", "reserved"):
        live = np.arange(max_rec) < taken if f in ("in_off", "out_off") else np.ones(max_rec, bool)
        assert np.array_equal(got[f][live], want[f][live]), (f, np.flatnonzero(got[f] != want[f])[:5])
    assigned = want_st <= BAD_MAC
    assert np.array_equal(got["nonce"][assigned], want["nonce"][assigned])
    assert np.array_equal(_host(d_first, np.uint64), np.array(first, np.uint64))
    assert np.array_equal(_host(d_nfr, np.uint32), np.array(nframes, np.uint32))
    assert np.array_equal(_host(d_fb, np.uint32), np.array(first_bad, np.uint32))
    assert np.array_equal(_host(d_cons, np.uint64), np.array(consumed, np.uint64))
    assert np.array_equal(_host(d_plen, np.uint64), np.array(plen, np.uint64))
    assert np.array_equal(_host(d_cst), np.array(cstat, np.uint8))
    assert int(_host(d_total, np.uint64)[0]) == total
    got_out = _host(d_wire if in_place else d_plain)
    assert np.array_equal(got_out[~skip], want_out[~skip]), np.flatnonzero((got_out != want_out) & ~skip)[:5]
    if not in_place:
        assert np.array_equal(_host(d_wire), wire)  # the received bytes are only read
    assert np.array_equal(counters(t), np.asarray(ctr, np.uint64))
    return want_st, plains, consumed, cstat


def edge_connections(nconn, rng, oracle, keys, ctr, sess, big_at):
    """The emulator's edge list over real frames: per connection 0 to about 40
    frames under the nonces the loop will give them (so the tags verify unless
    spoiled here), then one of the tails; some with a bad length in front of a
    frame; one 65535-byte frame."""
    ctr = [int(c) for c in ctr]
    conns = []
    for j in range(nconn):
        s = int(sess[j])
        live = s < len(keys) and keys[s].any()
        nf = int(rng.integers(30, 41)) if j % 11 == 3 else 0 if j % 5 == 4 else int(rng.integers(0, 5))
        bad_at = int(rng.integers(0, nf + 1)) if j % 13 == 2 else -1
        b = b""
        for k in range(nf + 1):
            if k == bad_at:
                b += struct.pack(">H", 15 if k % 2 else 0) + bytes(15 if k % 2 else 3)
            if k == nf:
                break
            L = 65535 if j == big_at and k == 1 else LS[int(rng.integers(5))]
            p = rng.integers(0, 256, L - 16, dtype=np.uint8).tobytes()
            n = ctr[s] if live else 0
            if live and k < (bad_at if bad_at >= 0 else nf) and ctr[s] < LIMIT:
                ctr[s] += 1  # only the frames the walk reaches take a nonce
            ct = oracle.encrypt(keys[s].tobytes() if live else bytes(32), n % (1 << 64), b"", p)
            if rng.integers(9) == 0:
                ct = ct[:-1] + bytes([ct[-1] ^ 0x40])  # a tag bit
            b += struct.pack(">H", L) + ct
        if bad_at < 0:
            tail = j % 6
            if tail == 1:
                b += b"\x00"
            elif tail == 2:
                b += struct.pack(">H", LS[j % 5])
            elif tail == 3:
                b += struct.pack(">H", LS[j % 5]) + bytes(LS[j % 5] - 1)
            elif tail == 4:
                b += b"\xff"
        conns.append(b)
    return conns


def edge_sessions(nconn, nsess, rng):
    sess = rng.integers(0, nsess, nconn).astype(np.uint32)
    sess[5::37] = nsess + 1
    sess[7::91] = 0xffffffff
    return sess


@pytest.mark.parametrize("cap", ["total", "total-1", "mid", "one", "total+70"])
@pytest.mark.parametrize("nconn", [65, 300])
def test_open_edges_against_the_loops(oracle, nconn, cap):
    rng = np.random.default_rng(1000 + nconn)
    nsess = 40
    keys = make_keys(nsess, rng, keyless=range(6, nsess, 7))
    ctr = np.array([0, (1 << 32) - 5, 12345678901, LIMIT - 3] * 10, np.uint64)
    sess = edge_sessions(nconn, nsess, rng)
    conns = edge_connections(nconn, rng, oracle, keys, ctr, sess, big_at=3)
    t = make_table(keys, ctr)
    in_place = cap in ("total-1", "total+70")
    st, _, _, cstat = run_open(t, keys, ctr.copy(), sess, conns, cap, in_place, oracle)
    if cap != "one":
        assert {OK, BAD_MAC, BAD_KEY, NONCE} <= set(st.tolist()), set(st.tolist())
        assert F_BAD_LEN in cstat
    assert (EMPTY in st) == (cap == "total+70") and (F_FULL in cstat) == (cap in ("total-1", "mid", "one"))
    t.close()


# ---- seal ----------------------------------------------------------------------------
def run_seal(t, keys, ctr, sess, msgs, mp, cap, oracle, len_sum=0):
    """msgs: the application bytes of each connection.  Checks everything the
    call writes against the loops and the oracle; ctr is moved.  Returns
    (statuses, the wire bytes written per connection, connection statuses)."""
    nconn = len(msgs)
    count = [(len(m) + mp - 1) // mp for m in msgs]
    max_rec = cap if isinstance(cap, int) else cap_of(cap, count)
    first, nframes, total = assign_slots(count, max_rec)
    taken = min(total, max_rec)
    moff, mtotal = place([len(m) for m in msgs])
    # a connection's room ends with its last frame: a write behind it lands in the canary
    woff, wtotal = place([(c - 1) * (mp + 18) + 18 + len(m) - (c - 1) * mp if c else 0 for c, m in zip(count, msgs)])
    msg = np.full(mtotal, CANARY, np.uint8)
    for j, m in enumerate(msgs):
        msg[int(moff[j]):int(moff[j]) + len(m)] = np.frombuffer(m, np.uint8)
    want_wire = np.full(wtotal, CANARY, np.uint8)
    want_st = np.full(max_rec, EMPTY, np.uint8)
    want = np.zeros(max_rec, REC)
    want["key_idx"][taken:], want["reserved"][taken:] = 0xffffffff, EMPTY
    used, wlen, cstat, sent = [0] * nconn, [0] * nconn, [F_OK] * nconn, [b""] * nconn
    for j in range(nconn):
        prefix = True
        for k in range(nframes[j]):
            i = first[j] + k
            p = msgs[j][k * mp:(k + 1) * mp]
            in_off, out_off = int(moff[j]) + k * mp, int(woff[j]) + k * (mp + 18) + 2
            st, n = next_nonce(keys, ctr, int(sess[j]))
            want_st[i] = st
            want[i] = (in_off, out_off, n, 0, len(p), 0, int(sess[j]), 0)
            if st != OK:
                prefix = False
                continue
            assert prefix  # refused records are a suffix
            f = struct.pack(">H", len(p) + 16) + oracle.encrypt(keys[int(sess[j])].tobytes(), n, b"", p)
            want_wire[out_off - 2:out_off - 2 + len(f)] = np.frombuffer(f, np.uint8)
            used[j] += len(p)
            wlen[j] += len(f)
            sent[j] += f
        cstat[j] = F_REFUSED if not prefix else F_FULL if nframes[j] < count[j] else F_OK

    d_msg, d_wire = _dev(msg), _fill(wtotal, CANARY)
    d_moff, d_mlen, d_woff = _dev(moff), _dev(np.array([len(m) for m in msgs], np.uint32)), _dev(woff)
    d_recs, d_st, d_sess = _fill(48 * max_rec, 0x77), _fill(max_rec, 0x77), _dev(np.asarray(sess, np.uint32))
    d_first, d_nfr = _fill(nconn, -1, torch.int64), _fill(nconn, -1, torch.int32)
    d_used, d_wlen, d_cst = _fill(nconn, -1, torch.int64), _fill(nconn, -1, torch.int64), _fill(nconn, 0x77)
    d_total = _fill(1, -1, torch.int64)
    t.seal_framed(d_sess, noise_amd.span(d_msg, off=d_moff, lens=d_mlen), noise_amd.span(d_wire, off=d_woff), mp,
                  d_recs, d_st, max_rec, d_nfr, d_used, d_wlen, d_cst, nconn, d_first=d_first, d_total=d_total,
                  len_sum=len_sum)
    torch.cuda.synchronize()
    got_st, got = _host(d_st), _host(d_recs).view(REC)
    assert np.array_equal(got_st, want_st), (np.flatnonzero(got_st != want_st)[:5], got_st[:8], want_st[:8])
    for f in ("in_off", "out_off", "len", "ad_len", "key_idx", "reserved"):
        live = np.arange(max_rec) < taken if f in ("in_off", "out_off") else np.ones(max_rec, bool)
        assert np.array_equal(got[f][live], want[f][live]), (f, np.flatnonzero(got[f] != want[f])[:5])
    assert np.array_equal(got["nonce"][want_st == OK], want["nonce"][want_st == OK])
    assert np.array_equal(_host(d_first, np.uint64), np.array(first, np.uint64))
    assert np.array_equal(_host(d_nfr, np.uint32), np.array(nframes, np.uint32))
    assert np.array_equal(_host(d_used, np.uint64), np.array(used, np.uint64))
    assert np.array_equal(_host(d_wlen, np.uint64), np.array(wlen, np.uint64))
    assert np.array_equal(_host(d_cst), np.array(cstat, np.uint8))
    assert int(_host(d_total, np.uint64)[0]) == total
    got_wire = _host(d_wire)
    assert np.array_equal(got_wire, want_wire), np.flatnonzero(got_wire != want_wire)[:5]
    assert np.array_equal(_host(d_msg), msg)
    assert np.array_equal(counters(t), np.asarray(ctr, np.uint64))
    return want_st, sent, cstat


def edge_messages(nconn, rng, mp, most):
    """Lengths 0, 1, multiples of max_payload and those +- 1, and anything."""
    msgs = []
    for j in range(nconn):
        m = int(rng.integers(1, most + 1))
        n = [0, 1, mp * m, mp * m + 1, mp * m - 1, int(rng.integers(0, mp * most // 4 + 2))][(j + 2) % 6]
        msgs.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    return msgs


@pytest.mark.parametrize("mp,cap", [(1, "total"), (1, "mid"), (64, "total-1"), (64, "total+70"), (64, "one"),
                                    (65519, "total")])
@pytest.mark.parametrize("nconn", [65, 300])
def test_seal_edges_against_the_oracle(oracle, nconn, mp, cap):
    rng = np.random.default_rng(2000 + nconn + mp)
    nsess = 40
    keys = make_keys(nsess, rng, keyless=range(6, nsess, 7))
    ctr = np.array([0, (1 << 32) - 5, 12345678901, LIMIT - 3] * 10, np.uint64)
    sess = edge_sessions(nconn, nsess, rng)
    if mp == 65519:  # two frames at the most, on a few connections: 131 KB each
        msgs = [b"" if j % 20 else m for j, m in enumerate(edge_messages(nconn, rng, mp, 1))]
    else:
        msgs = edge_messages(nconn, rng, mp, 40 if mp == 1 else 12)
    t = make_table(keys, ctr)
    st, _, cstat = run_seal(t, keys, ctr.copy(), sess, msgs, mp, cap, oracle)
    if cap != "one" and mp != 65519:  # (a handful of records there)
        assert {OK, BAD_KEY, NONCE} <= set(st.tolist()), set(st.tolist())
        assert F_REFUSED in cstat
    assert (EMPTY in st) == (cap == "total+70") and (F_FULL in cstat) == (cap in ("total-1", "mid", "one"))
    t.close()


# ---- the classified records path on unaligned records --------------------------------
def test_classified_path_seal_then_open(oracle):
    """2100 connections seal one record each of 1 to 3000 bytes, one of 65519;
    the receiver finds behind each a host-made empty frame: 4200 records of 0
    to 65519 bytes in one open, above the classifier's threshold."""
    rng = np.random.default_rng(31)
    nconn = 2100
    keys = make_keys(nconn, rng)
    ctr = np.zeros(nconn, np.uint64)
    sess = rng.permutation(nconn).astype(np.uint32)
    lens = rng.integers(1, 3001, nconn)
    lens[1234] = 65519
    msgs = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in lens]
    tx, rx = make_table(keys, ctr), make_table(keys, ctr)
    st, sent, _ = run_seal(tx, keys, ctr.copy(), sess, msgs, 65519, "total", oracle, len_sum=int(lens.sum()))
    assert (st == OK).all() and len(st) == nconn
    conns = [sent[j] + host_frames(oracle, keys[int(sess[j])].tobytes(), 1, [b""]) for j in range(nconn)]
    st, plains, _, _ = run_open(rx, keys, ctr.copy(), sess, conns, "total", False, oracle, len_sum=int(lens.sum()))
    assert (st == OK).all() and len(st) == 2 * nconn and plains == msgs
    tx.close()
    rx.close()


# ---- a stream cut anywhere: two calls that carry the tails over ------------------------
def test_stream_cut_anywhere_opens_in_two_calls(oracle):
    rng = np.random.default_rng(47)
    nconn, nsess, mp = 130, 50, 200
    keys = make_keys(nsess, rng)
    ctr = rng.integers(0, 1 << 40, nsess).astype(np.uint64)
    sess = rng.integers(0, nsess, nconn).astype(np.uint32)  # sessions on several connections
    msgs = [rng.integers(0, 256, int(rng.integers(0, 1500)), dtype=np.uint8).tobytes() for _ in range(nconn)]
    tx, rx = make_table(keys, ctr), make_table(keys, ctr)
    tx_ctr = ctr.copy()
    st, sent, _ = run_seal(tx, keys, tx_ctr, sess, msgs, mp, "total", oracle)
    assert (st == OK).all()
    # The receiver sees each connection's bytes in two reads.  A session on two
    # connections must meet its frames in the sender's order: connection by
    # connection.  So the first call gets whole streams for connections below a
    # boundary and nothing above it but for cuts of the boundary's own sessions.
    cuts = [int(rng.integers(0, len(b) + 1)) for b in sent]
    seen_sessions, first_read = set(), []
    for j in range(nconn):  # a later connection of a session waits for the earlier one to finish
        if int(sess[j]) in seen_sessions:
            cuts[j] = 0
        elif cuts[j] < len(sent[j]):
            seen_sessions.add(int(sess[j]))
        first_read.append(sent[j][:cuts[j]])
    rx_ctr = ctr.copy()
    _, plain1, consumed, _ = run_open(rx, keys, rx_ctr, sess, first_read, "total+70", False, oracle)
    second_read = [first_read[j][consumed[j]:] + sent[j][cuts[j]:] for j in range(nconn)]
    assert any(0 < len(first_read[j]) - consumed[j] for j in range(nconn))  # tails were carried over
    st2, plain2, consumed2, cstat = run_open(rx, keys, rx_ctr, sess, second_read, "total", True, oracle)
    assert (st2 == OK).all() and set(cstat) == {F_OK}
    assert [a + b for a, b in zip(plain1, plain2)] == msgs
    assert consumed2 == [len(b) for b in second_read]
    assert np.array_equal(counters(rx), counters(tx)) and np.array_equal(rx_ctr, tx_ctr)
    tx.close()
    rx.close()


# ---- tampering -------------------------------------------------------------------------
def test_flipped_tag_bit_in_a_middle_frame(oracle):
    rng = np.random.default_rng(5)
    nconn = 70
    keys = make_keys(nconn, rng)
    ctr = np.full(nconn, 9, np.uint64)
    sess = np.arange(nconn, dtype=np.uint32)
    plains = [[rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in (40, 0, 333, 64, 17)]
              for _ in range(nconn)]
    conns = [host_frames(oracle, keys[j].tobytes(), 9, plains[j]) for j in range(nconn)]
    j, k = 66, 2  # in the second wave; the frame of 333 bytes
    at = sum(2 + 16 + len(p) for p in plains[j][:k]) + 2 + len(plains[j][k]) + 5
    conns[j] = conns[j][:at] + bytes([conns[j][at] ^ 0x08]) + conns[j][at + 1:]
    t = make_table(keys, ctr)
    st, got, _, _ = run_open(t, keys, ctr.copy(), sess, conns, "total", False, oracle)
    # run_open checked the loop's answer: d_first_bad, the zeroed slot, the later nonces; here what that answer is
    assert st[5 * j + k] == BAD_MAC and (np.delete(st, 5 * j + k) == OK).all()
    assert got[j] == b"".join(plains[j][:k] + plains[j][k + 1:])
    assert (counters(t) == 14).all()
    t.close()


# ---- end to end ------------------------------------------------------------------------
def test_end_to_end_handshake_seal_open(oracle):
    """XX handshakes on the GPU -> split -> a sending and a receiving table ->
    framed seal -> framed open; one session's handshake corrupted on the wire:
    keyless on both sides."""
    n, bad = 96, 17
    rng = np.random.default_rng(51)
    I, R = noise_amd.HandshakeBatch("XX", True, n), noise_amd.HandshakeBatch("XX", False, n)
    for hs in (I, R):
        hs.set_key(noise_amd.HS_S, _dev(rng.integers(0, 256, 32 * n, dtype=np.uint8)))
        hs.start()
    hst = torch.zeros(n, dtype=torch.uint8, device="cuda")
    for m in range(3):
        w, r = (I, R) if m % 2 == 0 else (R, I)
        ov = w.info().overhead
        buf = torch.zeros(n * 128, dtype=torch.uint8, device="cuda")
        w.write_message(noise_amd.span(buf, stride=128))
        if m == 1:
            buf[bad * 128 + 40] ^= 1
        r.read_message(noise_amd.span(buf, stride=128, length=ov), d_status=hst)
    k = [torch.zeros(32 * n, dtype=torch.uint8, device="cuda") for _ in range(4)]
    I.split(k[0], k[1])
    R.split(k[2], k[3])
    torch.cuda.synchronize()
    keys = _host(k[0]).reshape(n, 32).copy()
    assert np.array_equal(keys, _host(k[2]).reshape(n, 32)) and not keys[bad].any() and keys[bad - 1].any()
    I.close()
    R.close()
    tx, rx = noise_amd.CipherStateTable(n), noise_amd.CipherStateTable(n)
    tx.set(0, n, k[0])
    rx.set(0, n, k[2])
    ctr = np.zeros(n, np.uint64)
    sess = rng.permutation(n).astype(np.uint32)
    msgs = [rng.integers(0, 256, int(rng.integers(1, 3000)), dtype=np.uint8).tobytes() for _ in range(n)]
    st, sent, cstat = run_seal(tx, keys, ctr.copy(), sess, msgs, 1024, "total", oracle)
    where = int(np.flatnonzero(sess == bad)[0])
    assert cstat[where] == F_REFUSED and sent[where] == b"" and cstat.count(F_REFUSED) == 1
    st, plains, _, _ = run_open(rx, keys, ctr.copy(), sess, sent, "total", True, oracle)
    assert (st == OK).all()
    assert [p for j, p in enumerate(plains) if j != where] == [m for j, m in enumerate(msgs) if j != where]
    tx.close()
    rx.close()


def test_cpp_device_framed():
    """noise::DeviceCipherStates::framed_seal / framed_open against
    noise::transport::append_frame / Deframer and noise::CipherState on the
    host, both ways: tests/cpp/device_framed_test.cpp."""
    exe = os.path.join(noise_amd.ROOT, "noise-cpp_amd", "bin", "device_framed_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
