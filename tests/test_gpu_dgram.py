"""GPU: the datagram wire format on CipherState tables -- noise_gpu_dgram_seal /
noise_gpu_dgram_open (csrc/dgram_kernels.hip, csrc/dgram_calls.hpp).

A packet is pack('<IIQ', type, receiver, counter) + ct || tag.  Expected
packets come from the CPU oracle and the plain assignment rule (n++ per record
of a session, refused at 2^64-2); expected statuses, outputs and window rows of
open from a plain Python loop over the well-formed packets in record order
(check before the tag, update only after it verified), with the oracle deciding
the tags.  Neither is the code under test.  A twin table fed host-built
descriptors through the calls that existed before (noise_gpu_cs_encrypt_records
/ noise_gpu_cswin_decrypt_records) must end in the same state.

Shapes: 1 packet, 63 / 64 (one wave, the one-workgroup window commit), 65 (two
waves, the sorted commit), 1500 (three sort chunks); packet offsets 0, 1, 4 and
8 mod 16 in every batch (the header's three load / store forms); packets of 31,
32 and 33 bytes; 2100 packets at aligned slots for the classified records path
(threshold 2048)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import noise_amd

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

OK, BAD_MAC, BAD_KEY, NONCE, REPLAY = (noise_amd.REC_OK, noise_amd.REC_BAD_MAC, noise_amd.REC_BAD_KEY,
                                       noise_amd.REC_NONCE, noise_amd.REC_REPLAY)
MALFORMED = getattr(noise_amd, "REC_MALFORMED", 5)
LIMIT = (1 << 64) - 2
W = 1024
TYPE = 4
MAXLEN = 65519
REC = noise_amd.record_dtype()
LENS = np.array([0, 1, 15, 16, 17, 64, 1000, 1024, 1040])
MISALIGN = np.array([0, 0, 1, 0, 4, 8])  # packet offsets mod 16, by packet index mod 6


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


# ---- the models ------------------------------------------------------------------
class Win:
    """check / update of include/noise_gpu.h, literally."""

    def __init__(self):
        self.next, self.bits = 0, 0

    def check(self, n):
        if n >= self.next:
            return True
        if self.next - n > W:
            return False
        return not (self.bits >> (n % W)) & 1

    def update(self, n):
        if n >= self.next:
            if n - self.next + 1 >= W:
                self.bits = 0
            else:
                for m in range(self.next, n + 1):
                    self.bits &= ~(1 << (m % W))
            self.next = n + 1
        self.bits |= 1 << (n % W)

    def copy(self):
        w = Win()
        w.next, w.bits = self.next, self.bits
        return w


def open_loop(keys, wins, pkts, oracle):
    """pkts: [(bytes on the wire, length the span reports)].  Malformed packets
    out, then the windowed loop -> statuses, kinds, plaintexts, parsed fields."""
    st, kind, plain, parsed = np.zeros(len(pkts), np.uint8), [], {}, []
    entry = {}
    for i, (raw, plen) in enumerate(pkts):
        typ, s, n = struct.unpack("<IIQ", raw[:16]) if len(raw) >= 16 else (None, None, None)
        if plen < 32 or plen > 32 + MAXLEN or typ != TYPE:
            st[i], k = MALFORMED, "malformed"
            parsed.append(None)
        else:
            parsed.append((s, n, plen - 32))
            if s >= len(keys) or not keys[s].any():
                st[i], k = BAD_KEY, "key"
            elif n >= LIMIT:
                st[i], k = NONCE, "nonce"
            else:
                w = wins.setdefault(s, Win())
                entry.setdefault(s, w.copy())
                if not w.check(n):
                    st[i], k = REPLAY, ("inbatch" if entry[s].check(n) else "entry")
                else:
                    plain[i] = oracle.decrypt(keys[s].tobytes(), n, b"", raw[16:plen])
                    if plain[i] is None:
                        st[i], k = BAD_MAC, "mac"
                    else:
                        w.update(n)
                        k = "ok"
        kind.append(k)
    return st, np.array(kind), plain, parsed


def seal_loop(keys, ctr, sess, lens):
    """The plain assignment rule, record by record; ctr is moved."""
    st, nonce = np.zeros(len(sess), np.uint8), np.zeros(len(sess), np.uint64)
    for i, (s, ln) in enumerate(zip(sess, lens)):
        s = int(s)
        if ln > MAXLEN:
            st[i] = MALFORMED
        elif s >= len(keys) or not keys[s].any():
            st[i] = BAD_KEY
        elif int(ctr[s]) == LIMIT:
            st[i] = NONCE
        else:
            nonce[i] = ctr[s]
            ctr[s] = (int(ctr[s]) + 1) % (1 << 64)
    return st, nonce


def make_table(nsess, keys, ctr):
    t = noise_amd.CipherStateTable(nsess)
    t.set(0, nsess, _dev(keys.reshape(-1)), 32, _dev(np.asarray(ctr, np.uint64)))
    return t


def make_keys(nsess, rng, keyless=()):
    keys = rng.integers(0, 256, (nsess, 32), dtype=np.uint8)
    keys[:, 0] |= 1
    for s in keyless:
        keys[s] = 0
    return keys


def counters(t):
    d = torch.zeros(t.nsess, dtype=torch.int64, device="cuda")
    t.get(0, t.nsess, d_n=d)
    torch.cuda.synchronize()
    return _host(d, np.uint64).copy()


def window_rows(t):
    d_next = _fill(t.nsess, -1, torch.int64)
    d_bits = _fill(t.nsess * 128, 0xEE)
    t.window_get(0, t.nsess, d_next, d_bits)
    torch.cuda.synchronize()
    return _host(d_next, np.uint64).copy(), _host(d_bits).reshape(t.nsess, 128).copy()


def check_rows(t, wins):
    got_next, got_bits = window_rows(t)
    want_next, want_bits = np.zeros(t.nsess, np.uint64), np.zeros((t.nsess, 128), np.uint8)
    for s, w in wins.items():
        want_next[s] = w.next
        want_bits[s] = np.frombuffer(w.bits.to_bytes(128, "little"), np.uint8)
    assert np.array_equal(got_next, want_next), np.flatnonzero(got_next != want_next)[:5]
    assert np.array_equal(got_bits, want_bits), np.flatnonzero((got_bits != want_bits).any(axis=1))[:5]
    return got_next, got_bits


def slots(sizes, misalign=True):
    """Offsets of records of `sizes` bytes: 16-byte aligned slots with at least
    16 canary bytes between them, some pushed to 1, 4 and 8 mod 16."""
    slot = (np.asarray(sizes) + 15) // 16 * 16 + 32
    off = np.cumsum(slot) - slot + 16
    if misalign:
        off = off + MISALIGN[np.arange(len(sizes)) % 6]
    return off.astype(np.uint64), int(slot.sum()) + 32


def header(receiver, counter):
    return struct.pack("<IIQ", TYPE, receiver, counter)


# ---- seal --------------------------------------------------------------------------
def run_seal(t, keys, ctr, sess, lens, peer, in_place, oracle, rng, twin=None, misalign=True):
    """One seal against the assignment rule and the oracle; returns the packets'
    bytes (None where refused) and the statuses.  twin: a table in the same
    state, given host-built descriptors through noise_gpu_cs_encrypt_records."""
    nrec = len(sess)
    want, nonce = seal_loop(keys, ctr, sess, lens)
    real = np.where(lens > MAXLEN, 0, lens)  # an over-length payload has no bytes and a bare slot
    off, total = slots(real + 32, misalign)
    img = np.full(total, 0xA5, np.uint8)
    pts = [rng.integers(0, 256, int(n), dtype=np.uint8) for n in real]
    if in_place:
        poff = off + 16
        for i, p in enumerate(pts):
            img[int(poff[i]):int(poff[i]) + len(p)] = p
        d_pkt = _dev(img)
        d_pay = d_pkt
    else:
        psize = real + np.arange(nrec) % 3  # packed, every alignment
        poff = (np.cumsum(psize) - psize).astype(np.uint64)
        pay = np.full(int(psize.sum()) + 1, 0x5A, np.uint8)
        for i, p in enumerate(pts):
            pay[int(poff[i]):int(poff[i]) + len(p)] = p
        d_pkt, d_pay = _dev(img), _dev(pay)
    d_off, d_poff, d_len = _dev(off), _dev(poff), _dev(lens.astype(np.uint32))
    d_sess = _dev(sess.astype(np.uint32))
    d_peer = None if peer is None else _dev(peer.astype(np.uint32))
    d_recs, d_st, d_plen = _fill(48 * nrec, 0x77), _fill(nrec, 0x77), _fill(nrec, -1, torch.int32)
    len_sum = int(real.sum())
    t.seal_datagrams(TYPE, d_sess, noise_amd.span(d_pay, off=d_poff, lens=d_len), noise_amd.span(d_pkt, off=d_off),
                     d_recs, d_st, nrec, d_peer=d_peer, d_pkt_len=d_plen, len_sum=len_sum)
    torch.cuda.synchronize()
    got, out, recs = _host(d_st).copy(), _host(d_pkt).copy(), _host(d_recs).view(REC).copy()
    assert np.array_equal(got, want), [(i, sess[i], lens[i], got[i], want[i]) for i in np.flatnonzero(got != want)[:8]]
    # every OK packet is the header plus the oracle's record; everything else is as it was
    want_out, packets = img.copy(), []
    for i in range(nrec):
        if want[i] != OK:
            packets.append(None)
            continue
        s, n = int(sess[i]), int(nonce[i])
        p = header(int(peer[s]) if peer is not None else s, n) + oracle.encrypt(keys[s].tobytes(), n, b"", pts[i].tobytes())
        want_out[int(off[i]):int(off[i]) + len(p)] = np.frombuffer(p, np.uint8)
        packets.append(p)
    bad = np.flatnonzero(out != want_out)
    assert bad.size == 0, (bad[:8], [i for i in range(nrec) if off[i] <= bad[0] < off[i] + 32 + real[i]])
    assert np.array_equal(_host(d_plen, np.uint32), np.where(want == OK, 32 + real, 0))
    okm = want == OK
    assert np.array_equal(recs["nonce"][okm], nonce[okm])
    mal = want == MALFORMED
    assert (recs["key_idx"][mal] == 0xFFFFFFFF).all() and (recs["len"][mal] == 0).all()
    assert np.array_equal(recs["key_idx"][~mal], sess[~mal]) and np.array_equal(recs["len"][~mal], real[~mal])
    assert np.array_equal(recs["in_off"][~mal], poff[~mal]) and np.array_equal(recs["out_off"][~mal], off[~mal] + 16)
    assert np.array_equal(counters(t), ctr)
    if twin is not None:
        assert not mal.any()
        r2 = np.zeros(nrec, REC)
        r2["in_off"], r2["out_off"], r2["len"], r2["key_idx"] = poff, off + 16, real, sess
        d_r2, d_st2 = _dev(r2.view(np.uint8)), _fill(nrec, 0x77)
        d_out2 = _dev(img)
        d_in2 = d_out2 if in_place else d_pay
        twin.encrypt_records(d_r2, nrec, d_in2, d_out2, d_status=d_st2, len_sum=len_sum)
        torch.cuda.synchronize()
        assert np.array_equal(_host(d_st2), got)
        out2, filled = _host(d_out2), _host(d_r2).view(REC)
        assert np.array_equal(filled["nonce"][okm], recs["nonce"][okm])
        for i in np.flatnonzero(okm):
            a, b = int(off[i]) + 16, int(off[i]) + 32 + int(real[i])
            assert np.array_equal(out2[a:b], out[a:b]), i
        assert np.array_equal(counters(twin), ctr)
    return packets, want


@pytest.mark.parametrize("in_place", [False, True], ids=["copy", "inplace"])
@pytest.mark.parametrize("nrec", [1, 63, 64, 65, 1500])
def test_seal_against_the_oracle_and_a_twin_table(oracle, nrec, in_place):
    rng = np.random.default_rng(1000 + nrec)
    nsess = 40
    keys = make_keys(nsess, rng, keyless=(7,))
    ctr = np.array([[0, (1 << 32) - 20, LIMIT - 2, 7][s % 4] for s in range(nsess)], np.uint64)
    t, twin = make_table(nsess, keys, ctr), make_table(nsess, keys, ctr)
    peer = rng.permutation(nsess).astype(np.uint32)
    seen = set()
    for batch in range(2):  # back to back: the second meets moved counters
        sess = rng.integers(0, nsess, nrec).astype(np.uint32)
        if nrec > 12:  # no session, the refused mark itself, a keyless row, and session 2 past its last nonce
            sess[3], sess[5], sess[4] = nsess, 0xFFFFFFFF, 7
            sess[6] = sess[8] = sess[10] = 2
        lens = rng.choice(LENS, nrec)
        _, st = run_seal(t, keys, ctr, sess, lens, peer, in_place, oracle, rng, twin=twin)
        seen |= set(st.tolist())
    assert seen >= ({OK, BAD_KEY, NONCE} if nrec >= 63 else {OK}), seen
    t.close()
    twin.close()


def test_seal_overlength_takes_no_nonce(oracle):
    """Per-record lengths over 65519 between good records of one session:
    MALFORMED, nothing written, and the neighbours' counters are consecutive."""
    rng = np.random.default_rng(7)
    keys = make_keys(4, rng)
    ctr = np.array([0, (1 << 32) - 1, 5, 5], np.uint64)
    t = make_table(4, keys, ctr)
    for pad in (0, 100):
        sess = np.array([1, 1, 1, 2, 1] + [int(x) for x in rng.integers(0, 4, pad)], np.uint32)
        lens = np.array([64, MAXLEN + 1, 33, 0xFFFFFFFF, 16] + [16] * pad, np.int64)
        before = int(ctr[1])
        packets, st = run_seal(t, keys, ctr, sess, lens, None, False, oracle, rng)
        assert list(st[:5]) == [OK, MALFORMED, OK, MALFORMED, OK]
        got = [struct.unpack("<IIQ", packets[i][:16])[2] for i in (0, 2, 4)]
        assert got == [before, before + 1, before + 2]
    t.close()


# ---- open --------------------------------------------------------------------------
def draw(rng, base, used, s):
    """A counter for session s: mostly moving up from base[s], with duplicates,
    late copies, the window's far edge, jumps past it, and a few never valid."""
    r, b = int(rng.integers(100)), int(base[s])
    if r < 45:
        n, b = b, b + 1
    elif r < 60 and used.get(s):
        n = used[s][int(rng.integers(len(used[s])))]
    elif r < 75:
        n = max(b - 1 - int(rng.integers(30)), 0)
    elif r < 83:
        n = max(b - 1000 - int(rng.integers(100)), 0)
    elif r < 90:
        b += 1000 + int(rng.integers(60))
        n, b = b, b + 1
    elif r < 97:
        n = b + 7
    else:
        n = LIMIT + int(rng.integers(2))
    base[s] = min(b, LIMIT + 1)
    n = min(n, (1 << 64) - 1)
    used.setdefault(s, []).append(n)
    return n


def run_open(t, keys, wins, pkts, in_place, oracle, twin=None, misalign=True, second_pass=False):
    """One open of pkts = [(bytes, reported length)] against the loop; returns kinds and statuses."""
    nrec = len(pkts)
    want, kind, plain, parsed = open_loop(keys, wins, pkts, oracle)
    plen = np.array([p[1] for p in pkts], np.int64)
    olen = np.array([0 if q is None else q[2] for q in parsed], np.int64)
    off, total = slots([len(p[0]) for p in pkts], misalign)
    img = np.full(total, 0xA5, np.uint8)
    for i, (raw, _) in enumerate(pkts):
        img[int(off[i]):int(off[i]) + len(raw)] = np.frombuffer(raw, np.uint8)
    d_pkt = _dev(img)
    if in_place:
        ooff, ototal, d_out, base_img = off + 16, total, d_pkt, img
    else:
        osize = olen + np.arange(nrec) % 4
        ooff, ototal = (np.cumsum(osize) - osize).astype(np.uint64), int(osize.sum()) + 1
        base_img = np.full(ototal, 0xA5, np.uint8)
        d_out = _dev(base_img)
    d_off, d_ooff, d_len = _dev(off), _dev(ooff), _dev(plen.astype(np.uint32))
    d_recs, d_st, d_olen = _fill(48 * nrec, 0x77), _fill(nrec, 0x77), _fill(nrec, -1, torch.int32)
    len_sum = int(olen.sum())

    def call():
        t.open_datagrams(TYPE, noise_amd.span(d_pkt, off=d_off, lens=d_len), noise_amd.span(d_out, off=d_ooff),
                         d_recs, d_st, nrec, d_payload_len=d_olen, len_sum=len_sum)
        torch.cuda.synchronize()

    call()
    got, out, recs = _host(d_st).copy(), _host(d_out).copy(), _host(d_recs).view(REC).copy()
    assert np.array_equal(got, want), [(i, kind[i], got[i], want[i]) for i in np.flatnonzero(got != want)[:8]]
    want_out, skip = base_img.copy(), np.zeros(ototal, bool)
    for i in range(nrec):
        o, ln = int(ooff[i]), int(olen[i])
        if kind[i] == "ok":
            want_out[o:o + ln] = np.frombuffer(plain[i], np.uint8)
            skip[o + ln:o + ln + 16] = in_place  # the tag's bytes after an in-place decrypt are unspecified
        elif kind[i] == "inbatch" or (kind[i] == "mac" and not in_place):
            want_out[o:o + ln] = 0  # a post-authentication replay is zeroed; so is a failed copy
    bad = np.flatnonzero((out != want_out) & ~skip)
    assert bad.size == 0, (bad[:8], [(i, kind[i]) for i in range(nrec) if ooff[i] <= bad[0] < ooff[i] + olen[i] + 16])
    if not in_place:
        assert np.array_equal(_host(d_pkt), img), "open wrote to the packets"
    assert np.array_equal(_host(d_olen, np.uint32), np.where(want == OK, olen, 0))
    mal = want == MALFORMED
    assert (recs["key_idx"][mal] == 0xFFFFFFFF).all() and (recs["len"][mal] == 0).all()
    good = np.flatnonzero(~mal)
    assert np.array_equal(recs["key_idx"][good], [parsed[i][0] for i in good])
    assert np.array_equal(recs["nonce"][good], np.array([parsed[i][1] for i in good], np.uint64))
    assert np.array_equal(recs["len"][good], olen[good])
    assert np.array_equal(recs["in_off"][good], off[good] + 16) and np.array_equal(recs["out_off"][good], ooff[good])
    rows = check_rows(t, wins)
    if twin is not None:  # the well-formed packets, as host-built descriptors, through the call that was there before
        r2 = np.zeros(len(good), REC)
        r2["key_idx"], r2["nonce"], r2["len"] = recs["key_idx"][good], recs["nonce"][good], olen[good]
        r2["in_off"], r2["out_off"] = off[good] + 16, ooff[good]
        d_in2 = _dev(img)
        d_out2 = d_in2 if in_place else _dev(base_img)
        d_st2 = _fill(max(len(good), 1), 0x77)
        d_r2 = _dev(r2.view(np.uint8)) if len(good) else None
        twin.decrypt_records_window(d_r2, len(good), d_in2, d_out2, d_st2, len_sum=len_sum)
        torch.cuda.synchronize()
        assert np.array_equal(_host(d_st2)[:len(good)], got[good])
        assert np.array_equal(_host(d_out2)[~skip], out[~skip])
        rows2 = window_rows(twin)
        assert np.array_equal(rows[0], rows2[0]) and np.array_equal(rows[1], rows2[1])
    if second_pass:
        # The identical wire again, against the loop: what was accepted is a replay
        # now, the rest is as before -- but for a packet whose tag failed the first
        # time and whose counter a later packet of the first pass took or slid past
        # (the loop looks at the window before the tag): that one is a replay too.
        assert not in_place
        want2, kind2, _, _ = open_loop(keys, wins, pkts, oracle)
        assert (want2[kind == "ok"] == REPLAY).all() and not (kind2 == "ok").any()
        same = (kind != "ok") & (kind != "mac")
        assert np.array_equal(want2[same], want[same])
        assert np.isin(want2[kind == "mac"], [BAD_MAC, REPLAY]).all() and (want2 == BAD_MAC).any()
        d_st.fill_(0x77)
        call()
        assert np.array_equal(_host(d_st), want2)
        assert np.array_equal(_host(d_out), out), "the second pass changed an output byte"
        check_rows(t, wins)
    return kind, want


def wire_packets(rng, oracle, keys, nsess, nrec, base, used, lens_choice):
    """nrec packets built in Python: genuine ones at drawn counters, with flipped
    tags, wrong types, truncations, receivers that are none, over-long claims."""
    pkts = []
    for i in range(nrec):
        s = int(rng.integers(nsess))
        n = draw(rng, base, used, s)
        pt = rng.integers(0, 256, int(rng.choice(lens_choice)), dtype=np.uint8).tobytes()
        body = bytearray(oracle.encrypt(keys[s].tobytes(), n, b"", pt))
        r = int(rng.integers(100))
        typ, recv = TYPE, s
        if r < 8:
            body[-1 - int(rng.integers(16))] ^= 0x40     # the tag
        elif r < 12:
            typ ^= 1 << int(rng.integers(32))
        elif r < 15:
            recv = nsess + int(rng.integers(3))
        elif r < 17:
            recv = 0xFFFFFFFF
        raw = struct.pack("<IIQ", typ, recv, n) + bytes(body)
        plen = len(raw)
        if 17 <= r < 21:
            plen = [0, 15, 16, 31][r - 17]               # truncated: nothing past plen exists
            raw = raw[:plen]
        elif r == 21:
            plen, raw = 32 + MAXLEN + 1 + int(rng.integers(2)) * 70000, raw[:16]  # a length no packet has
        pkts.append((raw, plen))
    return pkts


@pytest.mark.parametrize("in_place", [False, True], ids=["copy", "inplace"])
@pytest.mark.parametrize("nrec", [1, 63, 64, 65, 1500])
def test_open_against_the_loop_and_a_twin_table(oracle, nrec, in_place):
    rng = np.random.default_rng(2000 + nrec)
    nsess = 40
    keys = make_keys(nsess, rng, keyless=(7,))
    ctr = np.full(nsess, 7, np.uint64)
    t, twin = make_table(nsess, keys, ctr), make_table(nsess, keys, ctr)
    base = np.array([[0, (1 << 32) - 40, 5000, LIMIT - 1200][s % 4] for s in range(nsess)], object)
    used, wins, seen = {}, {}, set()
    for batch in range(3):  # back to back: the later ones meet windows that have seen traffic
        pkts = wire_packets(rng, oracle, keys, nsess, nrec, base, used, LENS)
        kind, _ = run_open(t, keys, wins, pkts, in_place, oracle, twin=twin)
        seen |= set(kind)
    want_seen = {"ok", "entry", "inbatch", "mac", "nonce", "key", "malformed"} if nrec >= 63 else set()
    assert seen >= want_seen, seen
    assert (counters(t) == 7).all() and (counters(twin) == 7).all()
    t.close()
    twin.close()


def test_open_packets_of_31_32_33_bytes(oracle):
    """The shortest packets, alone and as the last of a batch, at every offset
    alignment: 31 bytes is malformed, 32 an empty payload, 33 one byte."""
    rng = np.random.default_rng(5)
    keys = make_keys(3, rng)
    t = make_table(3, keys, np.full(3, 7, np.uint64))
    wins, n = {}, 0
    for count in (1, 2, 3, 6):
        for rot in range(3):
            pkts = []
            for i in range(count):
                ln = [0, 1, 0][(i + rot) % 3]
                raw = header(1, n) + oracle.encrypt(keys[1].tobytes(), n, b"", bytes([i] * ln))
                n += 1
                pkts.append((raw[:31], 31) if (i + rot) % 3 == 2 else (raw, len(raw)))
            kind, st = run_open(t, keys, wins, pkts, False, oracle)
            assert list(st) == [MALFORMED if (i + rot) % 3 == 2 else OK for i in range(count)]
    t.close()


# ---- the classified records path ----------------------------------------------------
@pytest.mark.parametrize("in_place", [False, True], ids=["copy", "inplace"])
def test_classified_path_seal_then_open(oracle, in_place):
    """2100 packets at 16-byte aligned slots: above the 2048-record threshold of
    the load-balanced records path, so the ciphertexts take the tile classes."""
    rng = np.random.default_rng(2100)
    nrec, nsess = 2100, 64
    cycle = np.array([0, 16, 64, 1000, 1024, 1040, 2048, 2049, 4096, 5000, 16384, 16385, 65519])
    lens = cycle[np.arange(nrec) % 13]
    sess = (np.arange(nrec) * 7 % nsess).astype(np.uint32)
    keys = make_keys(nsess, rng)
    ctr = np.zeros(nsess, np.uint64)
    tx, rx = make_table(nsess, keys, ctr), make_table(nsess, keys, ctr)
    packets, st = run_seal(tx, keys, ctr, sess, lens, None, in_place, oracle, rng, misalign=False)
    assert (st == OK).all()
    pkts = []
    for i, p in enumerate(packets):
        if i % 5 == 0:  # 5 and 13 are coprime: tags flipped in packets of every length
            p = p[:-3] + bytes([p[-3] ^ 0x10]) + p[-2:]
        pkts.append((p, len(p)))
    kind, st = run_open(rx, keys, {}, pkts, in_place, oracle, misalign=False)
    flipped = np.arange(nrec) % 5 == 0
    assert (st[flipped] == BAD_MAC).all() and (st[~flipped] == OK).all()
    for ln in cycle:
        assert (flipped & (lens == ln)).any() and (~flipped & (lens == ln)).any()
    tx.close()
    rx.close()


# ---- end to end ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def split_keys():
    """XX handshakes on the GPU -> split: the initiator -> responder key rows of
    both sides (equal); one session's handshake corrupted on the wire: keyless."""
    n, bad = 96, 17
    rng = np.random.default_rng(51)
    I, R = noise_amd.HandshakeBatch("XX", True, n), noise_amd.HandshakeBatch("XX", False, n)
    for hs in (I, R):
        hs.set_key(noise_amd.HS_S, _dev(rng.integers(0, 256, 32 * n, dtype=np.uint8)))
        hs.start()
    st = torch.zeros(n, dtype=torch.uint8, device="cuda")
    for m in range(3):
        w, r = (I, R) if m % 2 == 0 else (R, I)
        ov = w.info().overhead
        buf = torch.zeros(n * 128, dtype=torch.uint8, device="cuda")
        w.write_message(noise_amd.span(buf, stride=128))
        if m == 1:
            buf[bad * 128 + 40] ^= 1
        r.read_message(noise_amd.span(buf, stride=128, length=ov), d_status=st)
    k = [torch.zeros(32 * n, dtype=torch.uint8, device="cuda") for _ in range(4)]
    I.split(k[0], k[1])
    R.split(k[2], k[3])
    torch.cuda.synchronize()
    keys = _host(k[0]).reshape(n, 32).copy()
    assert np.array_equal(keys, _host(k[2]).reshape(n, 32)) and not keys[bad].any() and keys[bad - 1].any()
    I.close()
    R.close()
    return n, bad, k[0], k[2], keys


def test_end_to_end_handshake_seal_wire_open(split_keys, oracle):
    n, bad, k_tx, k_rx, keys = split_keys
    rng = np.random.default_rng(77)
    # the responder keeps its sessions in another order: initiator session s is its row perm[s]
    perm = rng.permutation(n).astype(np.uint32)
    rx_keys = np.zeros_like(keys)
    rx_keys[perm] = _host(k_rx).reshape(n, 32)
    tx, rx = noise_amd.CipherStateTable(n), noise_amd.CipherStateTable(n)
    tx.set(0, n, k_tx)
    rx.set(0, n, _dev(rx_keys.reshape(-1)))
    # ---- 16 packets per session, uniform 64-byte payloads: the stride / len_all span forms
    nrec, L = 16 * n, 64
    sess = rng.permutation(np.repeat(np.arange(n, dtype=np.uint32), 16))
    pt = rng.integers(0, 256, nrec * L, dtype=np.uint8)
    d_pkt, d_recs, d_st = _fill(nrec * (L + 32), 0xA5), _fill(48 * nrec, 0), _fill(nrec, 0x77)
    d_plen, d_sess, d_pt, d_perm = _fill(nrec, -1, torch.int32), _dev(sess), _dev(pt), _dev(perm)
    tx.seal_datagrams(TYPE, d_sess, noise_amd.span(d_pt, stride=L, length=L), noise_amd.span(d_pkt, stride=L + 32),
                      d_recs, d_st, nrec, d_peer=d_perm, d_pkt_len=d_plen, len_sum=nrec * L)
    torch.cuda.synchronize()
    st, out = _host(d_st), _host(d_pkt).reshape(nrec, L + 32)
    assert np.array_equal(st, np.where(sess == bad, BAD_KEY, OK))
    assert (out[sess == bad] == 0xA5).all()  # the failed handshake's session sends nothing
    assert np.array_equal(_host(d_plen, np.uint32), np.where(sess == bad, 0, L + 32))
    rank = {}
    sent = []
    for i in range(nrec):
        s = int(sess[i])
        if s == bad:
            continue
        c = rank.get(s, 0)
        rank[s] = c + 1
        p = out[i].tobytes()
        assert p == header(int(perm[s]), c) + oracle.encrypt(keys[s].tobytes(), c, b"", pt[i * L:(i + 1) * L].tobytes())
        sent.append(p)
    # ---- what a datagram network does to them
    wire = [sent[i] for i in rng.permutation(len(sent)) if rng.random() > 0.05]  # permuted, some dropped
    for _ in range(len(wire) // 12):
        wire.insert(int(rng.integers(len(wire) + 1)), wire[int(rng.integers(len(wire)))])  # duplicated
    pkts = []
    live = [int(perm[s]) for s in range(n) if s != bad]
    for j, p in enumerate(wire):
        r, plen = int(rng.integers(100)), len(p)
        if r < 5:
            p = p[:-2] + bytes([p[-2] ^ 1]) + p[-1:]     # tag flipped
        elif r < 8:
            p = bytes([p[0] ^ 2]) + p[1:]                # type flipped
        elif r < 11:
            p, plen = p[:31], 31                         # truncated
        elif r < 14:
            other = live[(live.index(struct.unpack("<I", p[4:8])[0]) + 1) % len(live)]
            p = p[:4] + struct.pack("<I", other) + p[8:]  # another live session
        elif r < 16:
            p = p[:4] + struct.pack("<I", n) + p[8:]     # no session
        pkts.append((p, plen))
    typ, recv, c = struct.unpack("<IIQ", wire[0][:16])
    pkts.insert(0, (struct.pack("<IIQ", typ, recv, c + 10 ** 6) + wire[0][16:], len(wire[0])))  # forged, far ahead
    pkts.insert(3, (header(int(perm[bad]), 0) + wire[0][16:], len(wire[0])))  # for the keyless row
    wins = {}
    kind, want = run_open(rx, rx_keys, wins, pkts, False, oracle, misalign=False, second_pass=True)
    assert kind[0] == "mac" and wins[recv].next <= 16  # the forged packet moved nothing
    assert {OK, BAD_MAC, BAD_KEY, REPLAY, MALFORMED} <= set(want.tolist()), set(want.tolist())
    assert (counters(rx) == 0).all()
    tx.close()
    rx.close()


def test_cpp_device_dgram():
    """noise::DeviceCipherStates::seal / open between two tables with a
    non-trivial d_peer, against noise::CipherState and noise::ReplayWindow on
    the host: tests/cpp/device_dgram_test.cpp."""
    exe = os.path.join(noise_amd.ROOT, "noise-cpp_amd", "bin", "device_dgram_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
