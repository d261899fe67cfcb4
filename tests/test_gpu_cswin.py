"""GPU: out-of-order receive on CipherState tables -- a replay window per
session (noise_gpu_cswin_*, csrc/cswin_kernels.hip).

Expected statuses and window rows come from a plain Python loop over the batch
in record order (the rule of include/noise_gpu.h: check before the tag, update
only after it verified); whether a tag verifies, and the plaintext, come from
the CPU oracle.  Neither is the code under test.  Every randomized case
asserts that the model alone produced each status it is about.

Shapes: batches of <= 64 records take the one-workgroup kernels, larger ones
the radix sort (1500 records: three chunks; 65537 sessions: three passes);
5000 records of one session are 79 steps of one wave."""
import os
import subprocess

import numpy as np
import pytest

import noise_amd

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

OK, BAD_MAC, BAD_KEY, NONCE = (noise_amd.REC_OK, noise_amd.REC_BAD_MAC, noise_amd.REC_BAD_KEY,
                               noise_amd.REC_NONCE)
REPLAY = getattr(noise_amd, "REC_REPLAY", 4)
LIMIT = (1 << 64) - 2
W = 1024
KOFF, NOFF = noise_amd.Record.key_idx.offset, noise_amd.Record.nonce.offset
ALL = {"ok", "entry", "inbatch", "mac", "nonce", "key"}


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


# ---- the model -------------------------------------------------------------------
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


def loop(keys, wins, sess, nonce, tag_ok):
    """The batch in record order -> (statuses, what each record was).  tag_ok(i)
    is asked only where the loop looks at the tag."""
    st, kind, entry = np.zeros(len(sess), np.uint8), [], {}
    for i, (s, n) in enumerate(zip(sess, nonce)):
        s, n = int(s), int(n)
        if s >= len(keys) or not keys[s].any():
            st[i], k = BAD_KEY, "key"
        elif n >= LIMIT:
            st[i], k = NONCE, "nonce"
        else:
            w = wins.setdefault(s, Win())
            entry.setdefault(s, w.copy())
            if not w.check(n):
                st[i], k = REPLAY, ("inbatch" if entry[s].check(n) else "entry")
            elif not tag_ok(i):
                st[i], k = BAD_MAC, "mac"
            else:
                w.update(n)
                k = "ok"
        kind.append(k)
    return st, np.array(kind)


def rows(t):
    d_next = torch.full((t.nsess,), -1, dtype=torch.int64, device="cuda")
    d_bits = torch.full((t.nsess * 128,), 0xEE, dtype=torch.uint8, device="cuda")
    t.window_get(0, t.nsess, d_next, d_bits)
    torch.cuda.synchronize()
    return _host(d_next, np.uint64), _host(d_bits).reshape(t.nsess, 128)


def check_rows(t, wins):
    got_next, got_bits = rows(t)
    want_next, want_bits = np.zeros(t.nsess, np.uint64), np.zeros((t.nsess, 128), np.uint8)
    for s, w in wins.items():
        want_next[s] = w.next
        want_bits[s] = np.frombuffer(w.bits.to_bytes(128, "little"), np.uint8)
    assert np.array_equal(got_next, want_next), np.flatnonzero(got_next != want_next)[:5]
    assert np.array_equal(got_bits, want_bits), np.flatnonzero((got_bits != want_bits).any(axis=1))[:5]
    return got_next, got_bits


def make_table(nsess, rng, keyless=()):
    keys = rng.integers(0, 256, (nsess, 32), dtype=np.uint8)
    keys[:, 0] |= 1
    for s in keyless:
        keys[s] = 0
    t = noise_amd.CipherStateTable(nsess)
    t.set(0, nsess, _dev(keys.reshape(-1)), 32, _dev(np.full(nsess, 7, np.uint64)))
    return t, keys


def counters_untouched(t):
    d = torch.zeros(t.nsess, dtype=torch.int64, device="cuda")
    t.get(0, t.nsess, d_n=d)
    torch.cuda.synchronize()
    return (_host(d, np.uint64) == 7).all()


# ---- the primitives ----------------------------------------------------------------
def draw(rng, base, used, s):
    """A nonce for session s: mostly moving up from base[s], with duplicates,
    reversals, the window's far edge, jumps past it, and a few never valid."""
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


def primitives(t, keys, wins, sess, nonce, verified, form):
    """filter, a stand-in verdict per candidate, commit -> statuses; all against the loop."""
    nrec = len(sess)
    want, kind = loop(keys, wins, sess, nonce, lambda i: verified[i])
    if form == "arrays":
        d_sess, d_nonce, kw = _dev(sess), _dev(nonce), {}
    else:
        recs = np.zeros(nrec, noise_amd.record_dtype())
        recs["key_idx"], recs["nonce"], recs["len"] = sess, nonce, 0x1234567
        d_sess = d_nonce = _dev(recs.view(np.uint8))
        kw = dict(sess_stride=48, nonce_stride=48, sess_offset=KOFF, nonce_offset=NOFF)
    st = torch.full((nrec,), 0xA5, dtype=torch.uint8, device="cuda")
    before = rows(t)
    t.window_filter(d_sess, d_nonce, st, nrec, **kw)
    after = rows(t)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])  # read-only
    pre = _host(st).copy()
    cand = np.isin(kind, ["ok", "mac", "inbatch"])
    assert np.array_equal(pre, np.where(cand, OK, want)), np.flatnonzero(pre != np.where(cand, OK, want))[:5]
    st2 = _dev(np.where(pre == OK, np.where(verified, OK, BAD_MAC), pre).astype(np.uint8))
    t.window_commit(d_sess, d_nonce, st2, nrec, **kw)
    torch.cuda.synchronize()
    got = _host(st2)
    assert np.array_equal(got, want), [(i, sess[i], nonce[i], got[i], want[i])
                                       for i in np.flatnonzero(got != want)[:5]]
    check_rows(t, wins)
    return set(kind), want


@pytest.mark.parametrize("form", ["arrays", "desc"])
@pytest.mark.parametrize("nrec", [1, 63, 64, 65, 1500])
def test_primitives_shuffled(nrec, form):
    rng = np.random.default_rng(nrec)
    nsess = 40
    t, keys = make_table(nsess, rng, keyless=(7,))
    base = np.array([[0, (1 << 32) - 40, 5000, LIMIT - 1200][s % 4] for s in range(nsess)], object)
    used, wins, seen = {}, {}, set()
    for batch in range(3):  # back to back: the later ones meet windows that have seen traffic
        sess = rng.integers(0, nsess, nrec).astype(np.uint32)
        if nrec > 8:
            sess[3], sess[5], sess[nrec - 1], sess[4] = nsess, nsess + 1, 0xFFFFFFFF, 7
        nonce = np.array([draw(rng, base, used, int(s) % nsess) for s in sess], np.uint64)
        seen |= primitives(t, keys, wins, sess, nonce, rng.random(nrec) < 0.9, form)[0]
    assert seen >= (ALL if nrec >= 63 else {"ok"}), seen
    assert counters_untouched(t)
    t.close()


def test_primitives_one_session_5000():
    """79 steps of one wave, three batches: duplicates, reversals, jumps past the window."""
    rng = np.random.default_rng(5000)
    t, keys = make_table(3, rng)
    base, used, wins, seen = np.array([0, (1 << 32) - 2000, 0], object), {}, {}, set()
    for batch in range(2):
        sess = np.ones(5000, np.uint32)
        nonce = np.array([draw(rng, base, used, 1) for _ in sess], np.uint64)
        seen |= primitives(t, keys, wins, sess, nonce, rng.random(5000) < 0.9, "arrays")[0]
    assert seen >= ALL - {"key"}, seen
    assert wins[1].next > 1 << 32  # crossed 2^32
    t.close()


def test_primitives_65537_sessions():
    """Three radix passes; indices that share low bytes and differ in high ones."""
    rng = np.random.default_rng(65537)
    nsess = 65537
    t, keys = make_table(nsess, rng)
    a, b = rng.integers(0, 5, 300), rng.integers(0, 5, 300)
    sess = (np.where(np.arange(300) % 2 == 1, a << 16 | b << 8 | 0x21, 0x010100 | a * 51) % nsess).astype(np.uint32)
    sess[17] = nsess - 1
    base, used, wins, seen = np.full(nsess, 3, object), {}, {}, set()
    for batch in range(2):
        nonce = np.array([draw(rng, base, used, int(s)) for s in sess], np.uint64)
        seen |= primitives(t, keys, wins, sess, nonce, rng.random(300) < 0.9, "arrays")[0]
    assert seen >= ALL - {"key"}, seen
    t.close()


def test_primitives_top_of_the_nonce_space():
    """2^64-3 is the last valid nonce; 2^64-2 and 2^64-1 are refused and move nothing."""
    rng = np.random.default_rng(3)
    t, keys = make_table(4, rng)
    wins = {}
    for nrec_pad in (0, 100):  # the one-workgroup path, then the sorted one
        s = 1 if nrec_pad == 0 else 2
        nonce = np.array([LIMIT - 1030, LIMIT - 3, LIMIT, LIMIT - 1, LIMIT + 1, LIMIT - 1, LIMIT - 2,
                          LIMIT - 1026, LIMIT - 1025, LIMIT - 3] + [LIMIT - 600 + i for i in range(nrec_pad)],
                         np.uint64)
        sess = np.full(len(nonce), s, np.uint32)
        seen = primitives(t, keys, wins, sess, nonce, np.ones(len(nonce), bool), "arrays")[0]
        assert seen >= {"ok", "inbatch", "nonce"}
        assert wins[s].next == LIMIT  # one past 2^64-3
    t.close()


def test_reset_set_and_rekey():
    """window_reset and set-with-keys start a fresh window; rekey and set-without-keys do not."""
    rng = np.random.default_rng(9)
    t, keys = make_table(6, rng)
    wins = {}
    sess = np.repeat(np.arange(6, dtype=np.uint32), 3)
    nonce = np.tile(np.array([5, 9, 5], np.uint64), 6)
    primitives(t, keys, wins, sess, nonce, np.ones(18, bool), "arrays")
    assert all(wins[s].next == 10 for s in range(6))
    t.window_reset(1, 2)                                             # sessions 1, 2
    t.set(4, 1, _dev(keys[4]), 32, _dev(np.full(1, 7, np.uint64)))   # session 4: a new key
    t.set(5, 1, None, 32, _dev(np.full(1, 7, np.uint64)))            # session 5: counter only
    t.rekey(_dev(np.array([0], np.uint32)), 1)                       # session 0
    for s in (1, 2, 4):
        wins[s] = Win()
    check_rows(t, wins)
    st = primitives(t, keys, wins, sess, nonce, np.ones(18, bool), "arrays")[1]
    assert list(st) == [REPLAY] * 3 + [OK, OK, REPLAY] * 2 + [REPLAY] * 3 + [OK, OK, REPLAY] + [REPLAY] * 3
    t.close()


def test_a_table_that_never_used_a_window_reads_fresh():
    t, _ = make_table(5, np.random.default_rng(1))
    check_rows(t, {})
    t.close()


# ---- end to end ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def split_keys():
    """XX handshakes on the GPU -> split: the sender's and the receiver's key
    rows (equal), one session's handshake corrupted on the wire: keyless rows."""
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


def send(tx, rng, n, nrec, lens):
    """nrec records through noise_gpu_cs_encrypt_records, which assigns the
    nonces and writes them into the descriptors -> [(session, nonce, wire bytes, plaintext)]."""
    recs = np.zeros(nrec, noise_amd.record_dtype())
    recs["len"], recs["key_idx"] = lens, rng.integers(0, n, nrec)
    slot = (lens + 16 + 15) // 16 * 16
    off = np.cumsum(slot) - slot
    recs["in_off"] = recs["out_off"] = off
    pt = rng.integers(0, 256, int(slot.sum()), dtype=np.uint8)
    d_recs, d_ct = _dev(recs.view(np.uint8)), torch.zeros(int(slot.sum()), dtype=torch.uint8, device="cuda")
    st = torch.zeros(nrec, dtype=torch.uint8, device="cuda")
    tx.encrypt_records(d_recs, nrec, _dev(pt), d_ct, d_status=st, len_sum=int(lens.sum()))
    torch.cuda.synchronize()
    filled, ct, st = _host(d_recs).view(noise_amd.record_dtype()), _host(d_ct), _host(st)
    return [(int(filled["key_idx"][i]), int(filled["nonce"][i]),
             ct[off[i]:off[i] + lens[i] + 16].copy(), pt[off[i]:off[i] + lens[i]].copy())
            for i in range(nrec) if st[i] == OK]


def scramble(rng, sent, late, n, nrec):
    """What a datagram network does to `sent`, cut or padded to nrec records:
    permuted, some dropped, some duplicated inside the batch, some tags flipped,
    late copies of an earlier batch, one forged record 10^6 ahead in front of its
    session's genuine ones, a nonce that is never valid, sessions that are none."""
    wire = [sent[i] for i in rng.permutation(len(sent))]
    wire = [r for r in wire if rng.random() > 0.05]
    out = []
    for s, nn, ct, pt in wire:
        if rng.random() < 0.05:
            ct = ct.copy()
            ct[-1 - int(rng.integers(16))] ^= 0x40
        out.append((s, nn, ct, pt))
    for _ in range(max(len(out) // 12, 3)):
        out.insert(int(rng.integers(len(out) + 1)), out[int(rng.integers(len(out)))])
    for r in late[:max(len(out) // 15, 3)]:
        out.insert(int(rng.integers(len(out) + 1)), r)
    # the session with the most records on the wire: genuine ones follow the forged one
    counts = np.bincount([r[0] for r in out])
    s, nn, ct, pt = next(r for r in out if r[0] == int(counts.argmax()))
    out.insert(0, (s, nn + 10 ** 6, ct, pt))          # forged: its tag cannot verify
    out.insert(5, (s, (1 << 64) - 1, ct, pt))         # never a valid nonce
    out.insert(9, (n + 3, nn, ct, pt))                # not a session
    out = out[:nrec]
    while len(out) < nrec:
        out.append(out[int(rng.integers(len(out)))])
    return out


def receive(rx, keys, wins, wire, oracle, form, in_place, need):
    """One windowed decrypt of `wire`, then the identical batch again."""
    nrec = len(wire)
    sess = np.array([w[0] for w in wire], np.uint32)
    nonce = np.array([w[1] for w in wire], np.uint64)
    lens = np.array([len(w[3]) for w in wire])
    plain = {}

    def tag_ok(i):
        plain[i] = oracle.decrypt(keys[sess[i]].tobytes(), int(nonce[i]), b"", wire[i][2].tobytes())
        return plain[i] is not None

    want, kind = loop(keys, wins, sess, nonce, tag_ok)
    assert set(kind) >= need, set(kind)
    forged = 0
    assert kind[forged] == "mac" and (kind[(sess == sess[forged]) & (np.arange(nrec) > 0)] == "ok").any()
    # buffers: 0xA5 canaries between and around the records; in place the output is the input
    slot = (lens + 16 + 15) // 16 * 16 + 16
    off = np.cumsum(slot) - slot + 16
    if form == "desc":
        off[::7] += 3  # unaligned records too
    total = int(slot.sum()) + 32
    img = np.full(total, 0xA5, np.uint8)
    for i, w in enumerate(wire):
        img[off[i]:off[i] + lens[i] + 16] = w[2]
    d_in = _dev(img)
    d_out = d_in if in_place else torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.full((nrec,), 0x77, dtype=torch.uint8, device="cuda")
    if form == "desc":
        recs = np.zeros(nrec, noise_amd.record_dtype())
        recs["len"], recs["key_idx"], recs["nonce"] = lens, sess, nonce
        recs["in_off"] = recs["out_off"] = off
        d_recs = _dev(recs.view(np.uint8))

        def run():
            rx.decrypt_records_window(d_recs, nrec, d_in, d_out, st, len_sum=int(lens.sum()))
    else:
        L = int(lens[0])
        assert (lens == L).all() and (np.diff(off) == slot[0]).all()
        d_sess, d_nonce = _dev(sess), _dev(nonce)

        def run():
            rx.decrypt_sessions_window(d_sess, d_nonce, d_in[16:], int(slot[0]), d_out[16:], int(slot[0]), L,
                                       st, nrec)
    run()
    torch.cuda.synchronize()
    got = _host(st).copy()
    assert np.array_equal(got, want), [(i, kind[i], got[i]) for i in np.flatnonzero(got != want)[:8]]
    out = _host(d_out).copy()
    want_out = img.copy() if in_place else np.full(total, 0xA5, np.uint8)
    skip = np.zeros(total, bool)
    for i in range(nrec):
        o, ln = int(off[i]), int(lens[i])
        if kind[i] == "ok":
            want_out[o:o + ln] = np.frombuffer(plain[i], np.uint8)
            assert plain[i] == wire[i][3].tobytes()
            skip[o + ln:o + ln + 16] = in_place  # the tag's bytes after an in-place decrypt are unspecified
        elif kind[i] == "inbatch" or (kind[i] == "mac" and not in_place):
            want_out[o:o + ln] = 0  # a post-authentication replay is zeroed; so is a failed copy
        # entry replays and refused records: untouched
    # a duplicate shares nothing with its twin here: every wire record has its own slot
    bad = np.flatnonzero((out != want_out) & ~skip)
    assert bad.size == 0, (bad[:8], [(i, kind[i]) for i in range(nrec) if off[i] <= bad[0] < off[i] + slot[i]])
    rows = check_rows(rx, wins)
    # ---- the identical batch again
    # (the loop looks at a tag only where the first pass saw it fail: those bytes are still the wire's)
    want2, kind2 = loop(keys, wins, sess, nonce, tag_ok)
    assert (want2[kind == "ok"] == REPLAY).all() and not (kind2 == "ok").any()
    st.fill_(0x77)
    run()
    torch.cuda.synchronize()
    assert np.array_equal(_host(st), want2)
    assert np.array_equal(_host(d_out), out), "the second pass changed an output byte"
    rows2 = check_rows(rx, wins)
    assert np.array_equal(rows[0], rows2[0]) and np.array_equal(rows[1], rows2[1])
    return kind


def end_to_end(split_keys, oracle, seed, form, in_place, nrec, len_choices):
    n, bad, k_tx, k_rx, keys = split_keys
    rng = np.random.default_rng(seed)
    tx, rx = noise_amd.CipherStateTable(n), noise_amd.CipherStateTable(n)
    tx.set(0, n, k_tx)
    rx.set(0, n, k_rx)
    wins = {}
    first = send(tx, rng, n, 120, rng.choice(len_choices, 120))
    assert first and all(s != bad for s, _, _, _ in first)  # the failed handshake's session sends nothing
    # an earlier batch arrives whole and in order ...
    k0 = receive_plain(rx, keys, wins, first, oracle, form)
    assert (k0 == "ok").all()
    # ... then the scrambled one, with late copies of the earlier batch
    sent = send(tx, rng, n, nrec, rng.choice(len_choices, nrec))
    wire = scramble(rng, sent, [first[i] for i in rng.permutation(len(first))], n, nrec)
    wire[20] = (bad, 3, wire[20][2], wire[20][3])  # a datagram for the keyless session
    receive(rx, keys, wins, wire, oracle, form, in_place, ALL)
    d = torch.zeros(n, dtype=torch.int64, device="cuda")
    rx.get(0, n, d_n=d)
    torch.cuda.synchronize()
    assert not _host(d, np.uint64).any()  # the receiver's in-order counters never moved
    tx.close()
    rx.close()


def receive_plain(rx, keys, wins, wire, oracle, form):
    """An undisturbed batch (copy form): everything is accepted."""
    nrec = len(wire)
    sess = np.array([w[0] for w in wire], np.uint32)
    nonce = np.array([w[1] for w in wire], np.uint64)
    lens = np.array([len(w[3]) for w in wire])
    want, kind = loop(keys, wins, sess, nonce, lambda i: True)
    slot = (lens + 16 + 15) // 16 * 16
    off = np.cumsum(slot) - slot
    img = np.zeros(int(slot.sum()), np.uint8)
    for i, w in enumerate(wire):
        img[off[i]:off[i] + lens[i] + 16] = w[2]
    d_in, d_out = _dev(img), torch.zeros(len(img), dtype=torch.uint8, device="cuda")
    st = torch.full((nrec,), 0x77, dtype=torch.uint8, device="cuda")
    if form == "desc":
        recs = np.zeros(nrec, noise_amd.record_dtype())
        recs["len"], recs["key_idx"], recs["nonce"] = lens, sess, nonce
        recs["in_off"] = recs["out_off"] = off
        rx.decrypt_records_window(_dev(recs.view(np.uint8)), nrec, d_in, d_out, st)
    else:
        rx.decrypt_sessions_window(_dev(sess), _dev(nonce), d_in, int(slot[0]), d_out, int(slot[0]),
                                   int(lens[0]), st, nrec)
    torch.cuda.synchronize()
    assert np.array_equal(_host(st), want)
    out = _host(d_out)
    for i, w in enumerate(wire):
        assert np.array_equal(out[off[i]:off[i] + lens[i]], w[3]), i
    check_rows(rx, wins)
    return kind


@pytest.mark.parametrize("in_place", [False, True], ids=["copy", "in-place"])
@pytest.mark.parametrize("L", [64, 1024])
def test_end_to_end_sessions(split_keys, oracle, L, in_place):
    end_to_end(split_keys, oracle, L + in_place, "sessions", in_place, 300, [L])


@pytest.mark.parametrize("in_place", [False, True], ids=["copy", "in-place"])
def test_end_to_end_records_mixed_lengths(split_keys, oracle, in_place):
    end_to_end(split_keys, oracle, 70 + in_place, "desc", in_place, 300, [1, 64, 100, 1024, 3000, 20000])


@pytest.mark.parametrize("in_place", [False, True], ids=["copy", "in-place"])
def test_end_to_end_records_classified(split_keys, oracle, in_place):
    """2100 records of <= 256 B: the classified path of the records kernels."""
    end_to_end(split_keys, oracle, 80 + in_place, "desc", in_place, 2100, [1, 16, 64, 100, 192, 255, 256])


def test_one_table_across_call_kinds(oracle):
    """One table (257 sessions: two radix passes) whose grow-only scratch is laid
    out four ways in turn (cs_scratch_layout, csrc/cstate_calls.hpp): in-order
    arrays, windowed descriptors (which grows it), a bare assign, windowed
    arrays.  Each call against the oracle and the host models."""
    n = 257
    rng = np.random.default_rng(n)
    t, keys = make_table(n, rng)
    tx = noise_amd.CipherStateTable(n)  # the peer that wrote what the windowed calls receive
    tx.set(0, n, _dev(keys.reshape(-1)), 32, _dev(np.full(n, 7, np.uint64)))
    ctr, wins = np.full(n, 7, np.uint64), {}
    # 1. noise_gpu_cs_encrypt_sessions, 65 records of 64 B
    L, nrec = 64, 65
    sess = rng.integers(0, n, nrec).astype(np.uint32)
    pt = rng.integers(0, 256, (nrec, L), dtype=np.uint8)
    ct = torch.full((nrec * (L + 16),), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.full((nrec,), 0x77, dtype=torch.uint8, device="cuda")
    t.encrypt_sessions(_dev(sess), _dev(pt.reshape(-1)), L, ct, L + 16, L, nrec, d_status=st)
    torch.cuda.synchronize()
    assert not _host(st).any()
    got = _host(ct).reshape(nrec, L + 16)
    for i, s in enumerate(sess):
        assert got[i].tobytes() == oracle.encrypt(keys[s].tobytes(), int(ctr[s]), b"", pt[i].tobytes()), i
        ctr[s] += 1
    # 2. noise_gpu_cswin_decrypt_records, 1500 records of mixed lengths
    sent = send(tx, rng, n, 1500, rng.choice([1, 64, 100, 1024, 3000], 1500))
    receive(t, keys, wins, scramble(rng, sent, [], n, 1500), oracle, "desc", False, ALL - {"entry"})
    # 3. noise_gpu_cs_assign, 1 record
    s = int(sess[0])
    d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = torch.full((1,), 0x77, dtype=torch.uint8, device="cuda")
    t.assign(_dev(np.array([s], np.uint32)), d_n, 1, st)
    torch.cuda.synchronize()
    assert int(_host(d_n, np.uint64)[0]) == int(ctr[s]) and int(_host(st)[0]) == OK
    ctr[s] += 1
    # 4. noise_gpu_cswin_decrypt_sessions, 65 records: new ones of 20 sessions and late copies from step 2
    sent4 = send(tx, rng, 20, 50, np.full(50, L))
    late = [r for r in sent if len(r[3]) == L]
    receive(t, keys, wins, scramble(rng, sent4, late, n, 65), oracle, "sessions", False, ALL)
    d = torch.zeros(n, dtype=torch.int64, device="cuda")
    t.get(0, n, d_n=d)
    torch.cuda.synchronize()
    assert np.array_equal(_host(d, np.uint64), ctr)  # the windowed calls never moved the in-order counters
    tx.close()
    t.close()


# ---- the C++ view ------------------------------------------------------------------
def test_cpp_device_windows():
    """noise::DeviceCipherStates' windowed calls against noise::ReplayWindow, and
    window(s) migration: tests/cpp/device_window_test.cpp."""
    exe = os.path.join(noise_amd.ROOT, "noise-cpp_amd", "bin", "device_window_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
