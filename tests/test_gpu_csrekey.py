"""GPU: the in-band rekey schedule of the CipherState tables
(noise_gpu_csrekey_set; csrc/cstate_kernels.hip k_csr_*, csrc/cstate_calls.hpp).

The model is the loop of include/noise_gpu.h written out in Python over a
(key, counter) pair per session, with the CPU oracle's REKEY:

    status = encrypt / decrypt(record)       # refused at n == 2^64-2, keyless does nothing
    if the call moved n and n % every == 0:  # n after the move, mod 2^64
        k = REKEY(k)

Expected ciphertexts come from the CPU oracle under the model's key and nonce
of every record.  Neither is the code under test.

Shapes: 300 sessions; batches of 65 records (sorted path, one chunk), 1500
(three chunks) and, in the framed and handshake tests, at most 64 (the
one-workgroup path); every in {1, 16, 1000}; three consecutive batches with
starts chosen so that boundaries fall inside and between them; sessions at
2^64-1 (the wrap and its rekey), next to the nonce limit, keyless, and indices
that name no session but would name a private key row."""
import os
import struct
import subprocess

import numpy as np
import pytest

import noise_amd

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

OK, BAD_MAC, BAD_KEY, NONCE = noise_amd.REC_OK, noise_amd.REC_BAD_MAC, noise_amd.REC_BAD_KEY, noise_amd.REC_NONCE
LIMIT = (1 << 64) - 2
M64 = 1 << 64
REC = noise_amd.record_dtype()
CANARY = 0xA5
NSESS = 300


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


class Model:
    """The loop, one (key, counter) per session."""

    def __init__(self, keys, ctr, every, oracle):
        self.k = [bytes(r) for r in np.asarray(keys, np.uint8)]
        self.n = [int(c) for c in ctr]
        self.every, self.oracle, self.rekeys = every, oracle, 0

    def step(self, s):
        """The next record of session s: (status, nonce, key)."""
        if s >= len(self.k) or not any(self.k[s]):
            return BAD_KEY, 0, None
        if self.n[s] == LIMIT:
            return NONCE, 0, None
        n, k = self.n[s], self.k[s]
        self.n[s] = (n + 1) % M64
        if self.n[s] % self.every == 0:
            self.k[s] = self.oracle.rekey(k)
            self.rekeys += 1
        return OK, n, k

    def batch(self, sess):
        st, nonce, key = np.zeros(len(sess), np.uint8), np.zeros(len(sess), np.uint64), np.zeros((len(sess), 32), np.uint8)
        for i, s in enumerate(sess):
            st[i], n, k = self.step(int(s))
            if k is not None:
                nonce[i], key[i] = n, np.frombuffer(k, np.uint8)
        return st, nonce, key


def make_keys(rng, keyless=()):
    keys = rng.integers(0, 256, (NSESS, 32), dtype=np.uint8)
    keys[:, 0] |= 1
    for s in keyless:
        keys[s] = 0
    return keys


def make_table(keys, ctr, every):
    t = noise_amd.CipherStateTable(len(keys))
    t.set(0, len(keys), _dev(keys.reshape(-1)), 32, _dev(np.asarray(ctr, np.uint64)))
    t.set_rekey_every(every)
    return t


def state(t):
    rows, ctr = _fill(32 * t.nsess, 0), _fill(t.nsess, 0, torch.int64)
    t.get(0, t.nsess, d_keys=rows, d_n=ctr)
    torch.cuda.synchronize()
    return _host(rows).reshape(t.nsess, 32).copy(), _host(ctr, np.uint64).copy()


def check_state(t, model):
    rows, ctr = state(t)
    assert np.array_equal(ctr, np.array(model.n, np.uint64))
    want = np.frombuffer(b"".join(model.k), np.uint8).reshape(-1, 32)
    assert np.array_equal(rows, want), np.flatnonzero((rows != want).any(axis=1))[:5]


def starts(rng, every):
    """Counters around the boundaries: 0, every-1, every, 3*every-1, a few below one, random; then the specials."""
    ctr = np.zeros(NSESS, np.uint64)
    for s in range(NSESS):
        base = int(rng.integers(0, 1 << 40)) // every * every
        ctr[s] = [0, every - 1, every, 3 * every - 1, base + max(every, 3) - 3, int(rng.integers(0, 1 << 60))][s % 6]
    ctr[4], ctr[5] = M64 - 1, LIMIT - 1  # the wrap and its rekey; room for one record
    last = LIMIT // every * every        # a boundary and the nonce limit within reach of one batch
    ctr[6] = last - 2
    return ctr


def records_batch(rng, nrec, lens):
    """Descriptors over 300 sessions: half of them sessions 1..8 (so that a session crosses several
    boundaries in a batch at every = 16), strays, a keyless session; 16-byte aligned slots."""
    recs = np.zeros(nrec, REC)
    sess = np.where(rng.random(nrec) < 0.5, rng.integers(1, 9, nrec), rng.integers(0, NSESS, nrec)).astype(np.uint32)
    if nrec > 40:
        sess[3], sess[11], sess[nrec - 1] = NSESS, NSESS + 7, 0xFFFFFFFF  # NSESS + 7 < nrec: a private row's index
        sess[9] = 13  # keyless
    recs["key_idx"], recs["len"], recs["nonce"] = sess, lens, 0xDEAD
    slot = (np.asarray(lens, np.int64) + 16 + 15) // 16 * 16 + 16
    off = np.cumsum(slot) - slot
    recs["in_off"] = recs["out_off"] = off
    return recs, int(slot.sum()) + 16


def run_records(oracle, tx, rx, mtx, mrx, recs, total, rng, tamper=()):
    """encrypt_records on tx, every ciphertext against the oracle under the model's key
    and nonce; then (with the tags at `tamper` spoiled) decrypt_records on rx."""
    nrec, sess = len(recs), recs["key_idx"].astype(np.uint32)
    lens, off = recs["len"].astype(np.int64), recs["out_off"].astype(np.int64)
    len_sum = int(lens.sum())
    pt = rng.integers(0, 256, total, dtype=np.uint8)
    d_recs, d_pt, d_ct, d_st = _dev(recs.view(np.uint8)), _dev(pt), _fill(total, CANARY), _fill(nrec, 0x77)
    tx.encrypt_records(d_recs, nrec, d_pt, d_ct, d_status=d_st, len_sum=len_sum)
    torch.cuda.synchronize()
    want_st, want_n, want_k = mtx.batch(sess)
    got_st, filled, ct = _host(d_st), _host(d_recs).view(REC), _host(d_ct).copy()
    assert np.array_equal(got_st, want_st), np.flatnonzero(got_st != want_st)[:5]
    ok = want_st == OK
    assert np.array_equal(filled["nonce"][ok], want_n[ok])
    for f in ("in_off", "out_off", "len", "key_idx", "ad_len", "reserved"):
        assert np.array_equal(filled[f], recs[f]), f
    # the accepted records under a key table of their own: row i is the model's key for record i
    acc = recs[ok].copy()
    acc["nonce"], acc["key_idx"] = want_n[ok], np.arange(int(ok.sum()))
    bad, first = oracle.check_records(False, np.ascontiguousarray(want_k[ok]).reshape(-1), int(ok.sum()), acc, pt, ct)
    assert bad == 0, ("ciphertext differs from the oracle's under the model's key", int(np.flatnonzero(ok)[first]))
    for i in np.flatnonzero(~ok):
        assert (ct[off[i]:off[i] + lens[i] + 16] == CANARY).all(), ("a record that was not accepted was written", i)
    check_state(tx, mtx)
    # the receiver
    for i in tamper:
        ct[off[i] + lens[i] + 5] ^= 0x04
    d_ct2, d_back, d_st2, d_recs2 = _dev(ct), _fill(total, CANARY), _fill(nrec, 0x77), _dev(recs.view(np.uint8))
    rx.decrypt_records(d_recs2, nrec, d_ct2, d_back, d_st2, len_sum=len_sum)
    torch.cuda.synchronize()
    want_st2, want_n2, _ = mrx.batch(sess)
    for i in tamper:
        assert want_st2[i] == OK
        want_st2[i] = BAD_MAC
    got_st2, back = _host(d_st2), _host(d_back)
    assert np.array_equal(got_st2, want_st2), np.flatnonzero(got_st2 != want_st2)[:5]
    assert np.array_equal(_host(d_recs2).view(REC)["nonce"][ok], want_n2[ok])
    for i in range(nrec):
        if want_st2[i] == OK:
            assert np.array_equal(back[off[i]:off[i] + lens[i]], pt[off[i]:off[i] + lens[i]]), i
        elif want_st2[i] != BAD_MAC:
            assert (back[off[i]:off[i] + lens[i] + 16] == CANARY).all(), i
    check_state(rx, mrx)
    return want_st, want_st2


def lengths(rng, nrec, L):
    return rng.choice([0, 1, 15, 64, 100, 255, 1000, 1024, 2000], nrec) if L == "ragged" else np.full(nrec, L)


# ---- sender and receiver tables, three consecutive batches ---------------------------
@pytest.mark.parametrize("L", [64, 1024, "ragged"])
@pytest.mark.parametrize("nrec", [65, 1500])
@pytest.mark.parametrize("every", [1, 16, 1000])
def test_records_three_batches(oracle, every, nrec, L):
    rng = np.random.default_rng(every * 7 + nrec)
    keys, ctr = make_keys(rng, keyless=(13,)), starts(rng, every)
    tx, rx = make_table(keys, ctr, every), make_table(keys, ctr, every)
    mtx, mrx = Model(keys, ctr, every, oracle), Model(keys, ctr, every, oracle)
    seen = set()
    for b in range(3):
        recs, total = records_batch(rng, nrec, lengths(rng, nrec, L))
        if b == 1:
            recs["key_idx"][::2] = 6  # the boundary below the limit, then the limit (every <= 16 at 65 records)
        st, _ = run_records(oracle, tx, rx, mtx, mrx, recs, total, rng)
        seen |= set(st.tolist())
    assert {OK, BAD_KEY} <= seen and mtx.rekeys > 0 and mtx.rekeys == mrx.rekeys
    if every <= 16 or nrec == 1500:
        assert NONCE in seen
    tx.close()
    rx.close()


def test_records_classified_path(oracle):
    """4200 records of 0 .. 65519 bytes: above the classifier's record count, unaligned
    lengths, every = 16, one batch and its continuation."""
    rng = np.random.default_rng(4200)
    every, nrec = 16, 4200
    keys, ctr = make_keys(rng, keyless=(13,)), starts(rng, every)
    tx, rx = make_table(keys, ctr, every), make_table(keys, ctr, every)
    mtx, mrx = Model(keys, ctr, every, oracle), Model(keys, ctr, every, oracle)
    for b in range(2):
        lens = rng.choice([0, 1, 63, 64, 65, 256, 1000, 1024, 1025, 2048, 4096], nrec)
        lens[rng.integers(0, nrec, 12)] = rng.integers(8000, 65520, 12)
        lens[77], lens[78] = 65519, 0
        recs, total = records_batch(rng, nrec, lens)
        st, _ = run_records(oracle, tx, rx, mtx, mrx, recs, total, rng)
        assert {OK, BAD_KEY, NONCE} <= set(st.tolist())
    assert mtx.rekeys > 200
    tx.close()
    rx.close()


# ---- the sessions form ------------------------------------------------------------------
@pytest.mark.parametrize("nrec", [65, 1500])
def test_sessions_form(oracle, nrec):
    rng = np.random.default_rng(nrec + 1)
    every, L = 16, 1024
    keys, ctr = make_keys(rng, keyless=(13,)), starts(rng, every)
    tx, rx = make_table(keys, ctr, every), make_table(keys, ctr, every)
    mtx, mrx = Model(keys, ctr, every, oracle), Model(keys, ctr, every, oracle)
    for b in range(3):
        recs, _ = records_batch(rng, nrec, np.full(nrec, L))
        sess = recs["key_idx"].astype(np.uint32)
        if b == 1:
            sess[::2] = 6
        pt = rng.integers(0, 256, (nrec, L), dtype=np.uint8)
        d_sess, d_pt = _dev(sess), _dev(pt.reshape(-1))
        d_ct, d_st = _fill(nrec * (L + 16), CANARY), _fill(nrec, 0x77)
        tx.encrypt_sessions(d_sess, d_pt, L, d_ct, L + 16, L, nrec, d_status=d_st)
        torch.cuda.synchronize()
        want_st, want_n, want_k = mtx.batch(sess)
        assert np.array_equal(_host(d_st), want_st)
        ct = _host(d_ct).reshape(nrec, L + 16)
        for i in range(nrec):
            if want_st[i] == OK:
                assert ct[i].tobytes() == oracle.encrypt(want_k[i].tobytes(), int(want_n[i]), b"", pt[i].tobytes()), i
            else:
                assert (ct[i] == CANARY).all(), i
        assert np.array_equal(_host(d_sess, np.uint32), sess)
        check_state(tx, mtx)
        d_back, d_st2 = _fill(nrec * L, CANARY), _fill(nrec, 0x77)
        rx.decrypt_sessions(d_sess, d_ct, L + 16, d_back, L, L, d_st2, nrec)
        torch.cuda.synchronize()
        want_st2, _, _ = mrx.batch(sess)
        # what was not encrypted is canary bytes on the wire: accepted by the counter, failed by the tag
        want_st2 = np.where((want_st2 == OK) & (want_st != OK), BAD_MAC, want_st2)
        assert np.array_equal(_host(d_st2), want_st2)
        back = _host(d_back).reshape(nrec, L)
        good = want_st2 == OK
        assert np.array_equal(back[good], pt[good])
        check_state(rx, mrx)
    assert mtx.rekeys > 3 and NONCE in want_st
    tx.close()
    rx.close()


# ---- stream framing ---------------------------------------------------------------------
def test_framed_seal_cut_anywhere_open_in_two_calls(oracle):
    """every = 16, 40 frames a connection: frames 17.. need the next key inside one call.
    The sealed wire is compared with append_frame over the loop (BE16(len + 16) || ct || tag),
    cut at an arbitrary byte per connection and opened in two calls, as Deframer would."""
    rng = np.random.default_rng(40)
    every, nconn, frames, mp = 16, 10, 40, 48
    keys = make_keys(rng)
    ctr = np.zeros(NSESS, np.uint64)
    sess = (np.arange(nconn) * 3 + 1).astype(np.uint32)
    ctr[sess] = np.array([0, 15, 16, 47, M64 - 1, 5, 31, 1000, 7, 8], dtype=np.uint64)
    tx, rx = make_table(keys, ctr, every), make_table(keys, ctr, every)
    mtx, mrx = Model(keys, ctr, every, oracle), Model(keys, ctr, every, oracle)
    mlen = frames * mp  # full frames: they lie back to back at the pitch mp + 18
    msgs = rng.integers(0, 256, (nconn, mlen), dtype=np.uint8)
    pitch, max_rec = frames * (mp + 18), nconn * frames
    d_msg, d_wire = _dev(msgs.reshape(-1)), _fill(nconn * pitch, CANARY)
    d_recs, d_st, d_sess = _fill(48 * max_rec, 0x77), _fill(max_rec, 0x77), _dev(sess)
    d_nfr, d_used, d_wlen, d_cst = (_fill(nconn, -1, torch.int32), _fill(nconn, -1, torch.int64),
                                    _fill(nconn, -1, torch.int64), _fill(nconn, 0x77))
    tx.seal_framed(d_sess, noise_amd.span(d_msg, stride=mlen, length=mlen), noise_amd.span(d_wire, stride=pitch), mp,
                   d_recs, d_st, max_rec, d_nfr, d_used, d_wlen, d_cst, nconn)
    torch.cuda.synchronize()
    want = []
    for j in range(nconn):
        b = b""
        for k in range(frames):
            st, n, key = mtx.step(int(sess[j]))
            assert st == OK
            ct = oracle.encrypt(key, n, b"", msgs[j, k * mp:(k + 1) * mp].tobytes())
            b += struct.pack(">H", len(ct)) + ct
        want.append(b)
    wire = _host(d_wire).reshape(nconn, pitch)
    assert (_host(d_st) == OK).all() and (_host(d_cst) == 0).all()
    assert (_host(d_nfr, np.uint32) == frames).all() and (_host(d_wlen, np.uint64) == pitch).all()
    for j in range(nconn):
        assert wire[j].tobytes() == want[j], j
    check_state(tx, mtx)
    assert mtx.rekeys >= 2 * nconn
    # the receiver: two reads, the unconsumed tail of the first carried into the second
    cut = rng.integers(0, pitch + 1, nconn)
    cut[0], cut[1], cut[2] = 0, pitch, 17 * (mp + 18) + 1
    carry, got = [b""] * nconn, [b""] * nconn
    for read in range(2):
        now = [carry[j] + (want[j][:cut[j]] if read == 0 else want[j][cut[j]:]) for j in range(nconn)]
        lens = np.array([len(b) for b in now], np.uint32)
        off = (np.arange(nconn, dtype=np.uint64) * (pitch + 32)) + np.arange(nconn, dtype=np.uint64) % 3
        buf = np.full(nconn * (pitch + 32) + 16, CANARY, np.uint8)
        for j, b in enumerate(now):
            buf[int(off[j]):int(off[j]) + len(b)] = np.frombuffer(b, np.uint8)
        d_buf, d_plain, d_off, d_lens = _dev(buf), _fill(nconn * mlen, CANARY), _dev(off), _dev(lens)
        d_st2, d_recs2 = _fill(max_rec, 0x77), _fill(48 * max_rec, 0x77)
        d_cons, d_plen = _fill(nconn, -1, torch.int64), _fill(nconn, -1, torch.int64)
        rx.open_framed(d_sess, noise_amd.span(d_buf, off=d_off, lens=d_lens), d_recs2, d_st2, max_rec, d_nfr,
                       d_cons, d_cst, nconn, plain=noise_amd.span(d_plain, stride=mlen), d_plain_len=d_plen)
        torch.cuda.synchronize()
        nfr, cons, plen = _host(d_nfr, np.uint32), _host(d_cons, np.uint64), _host(d_plen, np.uint64)
        plain = _host(d_plain).reshape(nconn, mlen)
        total = int(nfr.sum())
        assert (_host(d_st2)[:total] == OK).all() and (_host(d_cst) == 0).all()
        for j in range(nconn):
            assert nfr[j] == len(now[j]) // (mp + 18) and cons[j] == nfr[j] * (mp + 18) and plen[j] == nfr[j] * mp
            got[j] += plain[j, :int(plen[j])].tobytes()
            carry[j] = now[j][int(cons[j]):]
            for _ in range(int(nfr[j])):
                mrx.step(int(sess[j]))
        check_state(rx, mrx)
    for j in range(nconn):
        assert carry[j] == b"" and got[j] == msgs[j].tobytes(), j
    tx.close()
    rx.close()


# ---- the schedule is applied per record ---------------------------------------------------
def test_flipped_tag_bit_before_a_boundary(oracle):
    """The record that moves its session onto the boundary fails its tag: the counter and
    the generation move all the same, and every later record of the session verifies."""
    rng = np.random.default_rng(5)
    every, nrec = 16, 200
    keys = make_keys(rng)
    ctr = np.zeros(NSESS, np.uint64)
    ctr[2] = 10
    tx, rx = make_table(keys, ctr, every), make_table(keys, ctr, every)
    mtx, mrx = Model(keys, ctr, every, oracle), Model(keys, ctr, every, oracle)
    recs, total = records_batch(rng, nrec, np.full(nrec, 100))
    recs["key_idx"][::3] = 2
    mine = np.flatnonzero(recs["key_idx"] == 2)
    victim = int(mine[5])  # nonce 15: the move behind it lands on 16
    _, st2 = run_records(oracle, tx, rx, mtx, mrx, recs, total, rng, tamper=(victim,))
    assert st2[victim] == BAD_MAC and (st2[mine[6:]] == OK).all() and len(mine) > 40
    tx.close()
    rx.close()


@pytest.mark.parametrize("tx_every,rx_every", [(16, 17), (1, 2)])
def test_receiver_with_every_off_by_one(oracle, tx_every, rx_every):
    """A receiver whose schedule is one off the sender's: REC_OK up to the sender's first
    boundary and BAD_MAC from it on -- for as long as the two generation counts differ.  A
    key depends on the number of REKEYs alone, so at 16 against 17 the counts meet again
    (ranks 17 .. 31 run under REKEY^1 on both sides) and the expected pattern is the two
    loops': OK exactly where they hold the same key.  At 1 against 2 they never meet:
    everything behind record 0 fails."""
    rng = np.random.default_rng(6)
    nrec, L = 130, 64
    keys = make_keys(rng)
    ctr = np.zeros(NSESS, np.uint64)
    tx, rx = make_table(keys, ctr, tx_every), make_table(keys, ctr, rx_every)
    mtx, mrx = Model(keys, ctr, tx_every, oracle), Model(keys, ctr, rx_every, oracle)
    sess = np.where(np.arange(nrec) % 2 == 0, 3, 4).astype(np.uint32)  # 65 records each
    recs = np.zeros(nrec, REC)
    recs["key_idx"], recs["len"] = sess, L
    recs["in_off"] = recs["out_off"] = np.arange(nrec) * 96
    pt = rng.integers(0, 256, nrec * 96, dtype=np.uint8)
    d_pt, d_ct, d_back, d_st = _dev(pt), _fill(nrec * 96, 0), _fill(nrec * 96, 0), _fill(nrec, 0x77)
    d_recs, d_recs2 = _dev(recs.view(np.uint8)), _dev(recs.view(np.uint8))
    tx.encrypt_records(d_recs, nrec, d_pt, d_ct)
    rx.decrypt_records(d_recs2, nrec, d_ct, d_back, d_st)
    torch.cuda.synchronize()
    st = _host(d_st)
    _, _, k_tx = mtx.batch(sess)
    _, _, k_rx = mrx.batch(sess)
    same = (k_tx == k_rx).all(axis=1)
    assert np.array_equal(st, np.where(same, OK, BAD_MAC)), st
    for s in (3, 4):
        mine = np.flatnonzero(sess == s)
        first = tx_every  # the rank of the first record behind the sender's first boundary
        assert (st[mine[:first]] == OK).all() and st[mine[first]] == BAD_MAC
        if tx_every == 1:
            assert (st[mine[first:]] == BAD_MAC).all()
        else:
            assert (st[mine[first + 1:2 * tx_every]] == OK).all() and (st[mine] == BAD_MAC).sum() == sum(r // 16 != r // 17 for r in range(len(mine)))
    check_state(tx, mtx)
    check_state(rx, mrx)
    tx.close()
    rx.close()


# ---- handshake -> split -> two tables with a schedule -> traffic ----------------------------
def test_handshake_split_scheduled_tables(oracle):
    rng = np.random.default_rng(8)
    n, every, L = 48, 16, 64
    I, R = noise_amd.HandshakeBatch("XX", True, n), noise_amd.HandshakeBatch("XX", False, n)
    for hs, seed in ((I, 1), (R, 2)):
        for which in (noise_amd.HS_S, noise_amd.HS_E):
            hs.set_key(which, _dev(np.random.default_rng(seed * 10 + which).integers(0, 256, 32 * n, dtype=np.uint8)))
        hs.start()
    st = _fill(n, 0)
    for m in range(3):
        w, r = (I, R) if m % 2 == 0 else (R, I)
        buf, ov = _fill(n * 128, 0), w.info().overhead
        w.write_message(noise_amd.span(buf, stride=128))
        r.read_message(noise_amd.span(buf, stride=128, length=ov), d_status=st)
        torch.cuda.synchronize()
        assert int(st.sum()) == 0
    k = [_fill(32 * n, 0) for _ in range(4)]
    I.split(k[0], k[1])
    R.split(k[2], k[3])
    torch.cuda.synchronize()
    assert torch.equal(k[0], k[2])
    I.close()
    R.close()
    tx, rx = noise_amd.CipherStateTable(n), noise_amd.CipherStateTable(n)
    tx.set(0, n, k[0])  # initiator -> responder
    rx.set(0, n, k[2])
    tx.set_rekey_every(every)
    rx.set_rekey_every(every)
    keys = _host(k[0]).reshape(n, 32).copy()
    model = Model(keys, np.zeros(n, np.uint64), every, oracle)
    for nrec in (64, 500, 33):  # session 0 takes half of each batch
        sess = np.where(np.arange(nrec) % 2 == 0, 0, rng.integers(0, n, nrec)).astype(np.uint32)
        pt = rng.integers(0, 256, (nrec, L), dtype=np.uint8)
        d_sess, d_ct, d_back, d_st = _dev(sess), _fill(nrec * (L + 16), 0), _fill(nrec * L, 0), _fill(nrec, 0x77)
        tx.encrypt_sessions(d_sess, _dev(pt.reshape(-1)), L, d_ct, L + 16, L, nrec)
        rx.decrypt_sessions(d_sess, d_ct, L + 16, d_back, L, L, d_st, nrec)
        torch.cuda.synchronize()
        want_st, want_n, want_k = model.batch(sess)
        ct = _host(d_ct).reshape(nrec, L + 16)
        for i in range(nrec):
            assert ct[i].tobytes() == oracle.encrypt(want_k[i].tobytes(), int(want_n[i]), b"", pt[i].tobytes()), i
        assert (_host(d_st) == OK).all() and np.array_equal(_host(d_back).reshape(nrec, L), pt)
        check_state(tx, model)
        check_state(rx, model)
    assert model.rekeys >= (32 + 250 + 17) // every  # session 0 alone: half of 64 + 500 + 33 records
    tx.close()
    rx.close()


# ---- what a scheduled table refuses ---------------------------------------------------------
def test_refusals_and_recovery():
    rng = np.random.default_rng(9)
    keys = make_keys(rng)
    t = make_table(keys, np.zeros(NSESS, np.uint64), 16)
    E = noise_amd.NoiseGpuError
    nrec, L = 8, 64
    sess, nonce, st = _dev(np.arange(nrec, dtype=np.uint32)), _fill(nrec, 0, torch.int64), _fill(nrec, 0)
    recs = np.zeros(nrec, REC)
    recs["key_idx"], recs["len"] = np.arange(nrec), L
    recs["in_off"] = recs["out_off"] = np.arange(nrec) * 128
    d_recs, buf, out = _dev(recs.view(np.uint8)), _fill(nrec * 128, 0), _fill(nrec * 128, 0)
    nxt, bits, plen = _fill(nrec, 0, torch.int64), _fill(nrec * 128, 0), _fill(nrec, 0, torch.int32)
    calls = {
        "noise_gpu_cs_assign": lambda: t.assign(sess, nonce, nrec, st),
        "noise_gpu_cswin_reset": lambda: t.window_reset(0, nrec),
        "noise_gpu_cswin_get": lambda: t.window_get(0, nrec, d_next=nxt, d_bits=bits),
        "noise_gpu_cswin_filter": lambda: t.window_filter(sess, nonce, st, nrec),
        "noise_gpu_cswin_commit": lambda: t.window_commit(sess, nonce, st, nrec),
        "noise_gpu_cswin_decrypt_records": lambda: t.decrypt_records_window(d_recs, nrec, buf, out, st),
        "noise_gpu_cswin_decrypt_sessions": lambda: t.decrypt_sessions_window(sess, nonce, buf, L + 16, out, L, L, st,
                                                                              nrec),
        "noise_gpu_dgram_seal": lambda: t.seal_datagrams(4, sess, noise_amd.span(buf, stride=128, length=L),
                                                         noise_amd.span(out, stride=128), d_recs, st, nrec),
        "noise_gpu_dgram_open": lambda: t.open_datagrams(4, noise_amd.span(buf, stride=128, length=L + 32),
                                                         noise_amd.span(out, stride=128), d_recs, st, nrec,
                                                         d_payload_len=plen),
    }
    before = state(t)
    for name, call in calls.items():
        with pytest.raises(E) as e:
            call()
        assert e.value.code == noise_amd.E_ARG and "rekey schedule" in str(e.value) and name in str(e.value), name
    torch.cuda.synchronize()
    after = state(t)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])  # nothing moved
    t.set_rekey_every(0)
    for name, call in calls.items():
        call()  # they work again
    torch.cuda.synchronize()
    t.close()


def test_cpp_device_rekey():
    """noise::DeviceCipherStates::set_rekey_every against the loop over the host
    noise::CipherState: tests/cpp/device_rekey_test.cpp."""
    exe = os.path.join(noise_amd.ROOT, "noise-cpp_amd", "bin", "device_rekey_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
