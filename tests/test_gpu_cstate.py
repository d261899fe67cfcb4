"""GPU: device-resident CipherState tables (noise_gpu_cs_*, csrc/cstate_kernels.hip).

Expected nonces, counters and statuses come from a plain Python loop over the
batch (a dict of counters and the rule of include/noise_gpu.h: n++ per call,
refused at n == 2^64-2, a keyless state does nothing); expected bytes from the
CPU oracle under those nonces.  Neither is the code under test.

Shapes: batches of <= 64 records take the one-workgroup kernel, larger ones the
radix sort, whose waves own chunks of >= 512 records (1500 records: three
chunks); 1, 257 and 65537 sessions force 1, 2 and 3 radix passes."""
import numpy as np
import pytest

import noise_amd

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

OK, BAD_MAC, BAD_KEY, NONCE = (noise_amd.REC_OK, noise_amd.REC_BAD_MAC, noise_amd.REC_BAD_KEY,
                               getattr(noise_amd, "REC_NONCE", 3))
LIMIT = (1 << 64) - 2
KOFF, NOFF = noise_amd.Record.key_idx.offset, noise_amd.Record.nonce.offset


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


def make_table(nsess, rng, keyless=(), n0=None):
    """A table with random key rows (zero rows for `keyless`) and counters n0;
    returns (table, keys [nsess][32], model counters)."""
    keys = rng.integers(0, 256, (nsess, 32), dtype=np.uint8)
    keys[:, 0] |= 1
    for s in keyless:
        keys[s] = 0
    n = np.zeros(nsess, np.uint64) if n0 is None else np.array(n0, np.uint64)
    t = noise_amd.CipherStateTable(nsess)
    t.set(0, nsess, _dev(keys.reshape(-1)), 32, _dev(n))
    return t, keys, n.copy()


def expect(keys, n, sess):
    """The plain loop: per-record nonce and status; advances the model counters n."""
    nonces, st = np.zeros(len(sess), np.uint64), np.zeros(len(sess), np.uint8)
    cur = {}
    for i, s in enumerate(sess):
        s = int(s)
        if s >= len(keys) or not keys[s].any():
            st[i] = BAD_KEY
            continue
        v = cur.get(s, int(n[s]))
        if v == LIMIT:
            st[i] = NONCE
            continue
        nonces[i] = v
        cur[s] = (v + 1) % (1 << 64)
    for s, v in cur.items():
        n[s] = v
    return nonces, st


def counters(t):
    d = torch.zeros(t.nsess, dtype=torch.int64, device="cuda")
    t.get(0, t.nsess, d_n=d)
    torch.cuda.synchronize()
    return _host(d, np.uint64)


def assign(t, sess, form):
    """noise_gpu_cs_assign over plain arrays or a descriptor array -> (nonces, status)."""
    nrec = len(sess)
    st = torch.full((nrec,), 0xA5, dtype=torch.uint8, device="cuda")
    if form == "arrays":
        d_n = torch.full((nrec,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
        t.assign(_dev(sess), d_n, nrec, st)
        torch.cuda.synchronize()
        return _host(d_n, np.uint64), _host(st)
    recs = np.zeros(nrec, noise_amd.record_dtype())
    recs["key_idx"], recs["nonce"], recs["len"], recs["in_off"] = sess, 0x5A5A5A5A, 0x1234567, 99
    d_recs = _dev(recs.view(np.uint8))
    t.assign(d_recs, d_recs, nrec, st, sess_stride=48, nonce_stride=48, sess_offset=KOFF,
             nonce_offset=NOFF)
    torch.cuda.synchronize()
    back = _host(d_recs).view(noise_amd.record_dtype())
    for f in ("key_idx", "len", "in_off", "out_off", "ad_off", "ad_len", "reserved"):
        assert np.array_equal(back[f], recs[f]), f  # only the nonce field is written
    return back["nonce"].copy(), _host(st)


def check_assign(t, keys, n, sess, form):
    want_n, want_st = expect(keys, n, sess)
    got_n, got_st = assign(t, sess, form)
    assert np.array_equal(got_st, want_st)
    ok = want_st == OK
    assert np.array_equal(got_n[ok], want_n[ok])
    assert np.array_equal(counters(t), n)


# ---- assign alone -----------------------------------------------------------
@pytest.mark.parametrize("form", ["arrays", "desc"])
@pytest.mark.parametrize("nrec", [1, 63, 64, 65, 129, 1500])
def test_assign_shuffled(nrec, form):
    rng = np.random.default_rng(nrec)
    nsess = 40
    t, keys, n = make_table(nsess, rng, keyless=(7,), n0=rng.integers(0, 1 << 62, nsess, dtype=np.uint64))
    sess = rng.integers(0, nsess, nrec).astype(np.uint32)
    if nrec > 8:
        sess[3], sess[5], sess[nrec - 1] = nsess, nsess + 1, 0xFFFFFFFF
        sess[4] = 7
    check_assign(t, keys, n, sess, form)
    check_assign(t, keys, n, sess[::-1].copy(), form)  # the next batch continues
    t.close()


@pytest.mark.parametrize("nrec", [64, 1500])
def test_assign_one_session_and_own_session(nrec):
    rng = np.random.default_rng(11)
    t, keys, n = make_table(nrec, rng, n0=rng.integers(0, 1 << 40, nrec, dtype=np.uint64))
    check_assign(t, keys, n, np.full(nrec, 5, np.uint32), "arrays")  # ranks cross waves and chunks
    check_assign(t, keys, n, rng.permutation(nrec).astype(np.uint32), "arrays")
    check_assign(t, keys, n, np.arange(nrec - 1, -1, -1).astype(np.uint32), "desc")
    t.close()


@pytest.mark.parametrize("nsess", [1, 257, 65537])
def test_assign_radix_passes(nsess):
    """Indices whose high bytes differ while the low bytes are equal, and the
    other way round: a pass skipped or ordered wrongly merges or splits runs."""
    rng = np.random.default_rng(nsess)
    t, keys, n = make_table(nsess, rng, n0=rng.integers(0, 1 << 50, nsess, dtype=np.uint64))
    a, b = rng.integers(0, 5, 300), rng.integers(0, 5, 300)
    sess = np.where(np.arange(300) % 2 == 1, a << 16 | b << 8 | 0x21, 0x010100 | a * 51) % nsess
    sess = sess.astype(np.uint32)
    sess[17] = nsess - 1
    check_assign(t, keys, n, sess, "arrays")
    check_assign(t, keys, n, sess, "desc")
    t.close()


# ---- limits, keyless rows, bad indices --------------------------------------------
@pytest.mark.parametrize("nrec", [48, 400])
def test_nonce_limit_keyless_and_bad_indices(oracle, nrec):
    rng = np.random.default_rng(nrec)
    nsess, L = 20, 64
    n0 = rng.integers(0, 1 << 30, nsess, dtype=np.uint64)
    n0[5], n0[6] = LIMIT - 3, (1 << 64) - 1
    t, keys, n = make_table(nsess, rng, keyless=(9,), n0=n0)
    sess = rng.integers(10, nsess, nrec).astype(np.uint32)  # 9 is keyless, 10.. are neighbours
    at5 = np.arange(6) * (nrec // 7) + 2
    at6 = np.arange(3) * (nrec // 4) + 1
    sess[at5], sess[at6] = 5, 6
    sess[0], sess[nrec - 2], sess[nrec - 1], sess[4] = nsess, nsess + 1, 0xFFFFFFFF, 9
    pt = rng.integers(0, 256, (nrec, L), dtype=np.uint8)
    d_pt, d_sess = _dev(pt.reshape(-1)), _dev(sess)

    def run_encrypt():
        ct = torch.full((nrec * (L + 16),), 0xA5, dtype=torch.uint8, device="cuda")
        st = torch.full((nrec,), 0x77, dtype=torch.uint8, device="cuda")
        t.encrypt_sessions(d_sess, d_pt, L, ct, L + 16, L, nrec, d_status=st)
        torch.cuda.synchronize()
        return _host(ct).reshape(nrec, L + 16), _host(st)

    def check(ct, st, want_n, want_st):
        assert np.array_equal(st, want_st)
        for i in range(nrec):
            if want_st[i] == OK:
                want = oracle.encrypt(keys[sess[i]].tobytes(), int(want_n[i]), b"", pt[i].tobytes())
                assert ct[i].tobytes() == want, i
            else:
                assert (ct[i] == 0xA5).all(), ("a record that was not accepted was written", i)

    want_n, want_st = expect(keys, n, sess)
    assert [int(x) for x in want_n[at5][:3]] == [LIMIT - 3, LIMIT - 2, LIMIT - 1]
    assert list(want_st[at5]) == [OK, OK, OK, NONCE, NONCE, NONCE]
    assert [int(x) for x in want_n[at6]] == [(1 << 64) - 1, 0, 1] and n[5] == LIMIT and n[6] == 2
    check(*run_encrypt(), want_n, want_st)
    got = counters(t)
    assert np.array_equal(got, n) and got[9] == n0[9] and got[5] == LIMIT
    # the next batch: every record of session 5 is refused, the others go on
    want_n, want_st = expect(keys, n, sess)
    assert (want_st[at5] == NONCE).all()
    check(*run_encrypt(), want_n, want_st)
    assert np.array_equal(counters(t), n)
    # decrypt: refused records read NONCE, a caller's bad index BAD_KEY, nothing of either written
    ct = torch.full((nrec * (L + 16),), 0x11, dtype=torch.uint8, device="cuda")
    back = torch.full((nrec * L,), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.full((nrec,), 0x77, dtype=torch.uint8, device="cuda")
    t.decrypt_sessions(d_sess, ct, L + 16, back, L, L, st, nrec)
    torch.cuda.synchronize()
    _, want_st = expect(keys, n, sess)
    got_st, back = _host(st), _host(back).reshape(nrec, L)
    assert np.array_equal(got_st != OK, np.ones(nrec, bool))  # garbage never verifies
    for i in range(nrec):
        assert got_st[i] == (BAD_MAC if want_st[i] == OK else want_st[i]), i
        if want_st[i] != OK:
            assert (back[i] == 0xA5).all(), i
    assert np.array_equal(counters(t), n)  # n advanced past the failed tags
    t.close()


# ---- continuity ------------------------------------------------------------------
def test_back_to_back_batches_and_migration():
    rng = np.random.default_rng(21)
    nsess = 300
    n0 = rng.integers(0, 1 << 60, nsess, dtype=np.uint64)
    a, keys, n = make_table(nsess, rng, keyless=(3, 250), n0=n0)
    b = noise_amd.CipherStateTable(nsess)
    b.set(0, nsess, _dev(keys.reshape(-1)), 32, _dev(n0))
    s1 = rng.integers(0, nsess, 700).astype(np.uint32)
    s2 = rng.integers(0, nsess, 50).astype(np.uint32)   # the one-workgroup path in between
    s3 = rng.integers(0, nsess, 900).astype(np.uint32)
    both = np.concatenate([s1, s2, s3])
    d_both = _dev(both)
    n_a = torch.zeros(len(both), dtype=torch.int64, device="cuda")
    st_a = torch.zeros(len(both), dtype=torch.uint8, device="cuda")
    # three calls on one stream, no synchronisation between them
    a.assign(d_both[:700], n_a[:700], 700, st_a[:700])
    a.assign(d_both[700:750], n_a[700:750], 50, st_a[700:750])
    a.assign(d_both[750:], n_a[750:], 900, st_a[750:])
    n_b, st_b = assign(b, both, "arrays")
    torch.cuda.synchronize()
    want_n, want_st = expect(keys, n, both)
    ok = want_st == OK
    assert np.array_equal(_host(st_a), want_st) and np.array_equal(st_b, want_st)
    assert np.array_equal(_host(n_a, np.uint64)[ok], want_n[ok]) and np.array_equal(n_b[ok], want_n[ok])
    assert np.array_equal(counters(a), n) and np.array_equal(counters(b), n)
    # get -> set into a fresh table (shifted by one row): the next batch is the continuation
    rows = torch.zeros(32 * nsess, dtype=torch.uint8, device="cuda")
    ctr = torch.zeros(nsess, dtype=torch.int64, device="cuda")
    a.get(0, nsess, d_keys=rows, d_n=ctr)
    c = noise_amd.CipherStateTable(nsess + 1)
    c.set(1, nsess, rows, 32, ctr)
    torch.cuda.synchronize()
    assert np.array_equal(_host(rows).reshape(nsess, 32), keys)
    s4 = rng.integers(0, nsess, 400).astype(np.uint32)
    want_n, want_st = expect(keys, n, s4)
    got_n, got_st = assign(c, s4 + 1, "arrays")
    ok = want_st == OK
    assert np.array_equal(got_st, want_st) and np.array_equal(got_n[ok], want_n[ok])
    assert counters(c)[0] == 0 and np.array_equal(counters(c)[1:], n)
    for t in (a, b, c):
        t.close()


# ---- encrypt / decrypt -------------------------------------------------------------
def test_records_mixed_batch(oracle):
    """~2300 descriptors (above the classify threshold): tile, long and generic
    lengths, some with 64 B of AD, 40 sessions, shuffled."""
    rng = np.random.default_rng(31)
    nsess, nrec = 40, 2300
    n0 = rng.integers(0, 1 << 48, nsess, dtype=np.uint64)
    tx, keys, n = make_table(nsess, rng, keyless=(13,), n0=n0)
    rx = noise_amd.CipherStateTable(nsess)
    rx.set(0, nsess, _dev(keys.reshape(-1)), 32, _dev(n0))
    lens = rng.choice([64, 100, 192, 200, 256, 1000, 1024, 2048, 2500, 4096, 5000], nrec)
    recs = np.zeros(nrec, noise_amd.record_dtype())
    recs["len"], recs["key_idx"] = lens, rng.integers(0, nsess, nrec)
    recs["key_idx"][100], recs["key_idx"][200] = nsess, 13
    with_ad = rng.random(nrec) < 0.1
    recs["ad_len"] = np.where(with_ad, 64, 0)
    recs["ad_off"] = np.cumsum(recs["ad_len"]) - recs["ad_len"]
    slot = (lens + 16 + 15) // 16 * 16 + 16
    off = np.cumsum(slot) - slot
    off[::50] += 3  # unaligned records: the generic class (every slot has 16 spare bytes)
    slot_total = int(slot.sum()) + 16
    recs["in_off"] = recs["out_off"] = off
    recs["nonce"] = 0xDEAD
    pt = rng.integers(0, 256, slot_total, dtype=np.uint8)
    ad = rng.integers(0, 256, int(recs["ad_len"].sum()) + 16, dtype=np.uint8)
    d_recs, d_pt, d_ad = _dev(recs.view(np.uint8)), _dev(pt), _dev(ad)
    d_ct = torch.full((slot_total,), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.full((nrec,), 0x77, dtype=torch.uint8, device="cuda")
    tx.encrypt_records(d_recs, nrec, d_pt, d_ct, d_ad=d_ad, d_status=st, len_sum=int(lens.sum()))
    torch.cuda.synchronize()
    sess = recs["key_idx"].astype(np.uint32)
    want_n, want_st = expect(keys, n, sess)
    assert np.array_equal(_host(st), want_st)
    filled = _host(d_recs).view(noise_amd.record_dtype())
    ok = want_st == OK
    assert np.array_equal(filled["nonce"][ok], want_n[ok]) and np.array_equal(filled["key_idx"], sess)
    ct = _host(d_ct)
    for i in range(nrec):
        o, ln = int(off[i]), int(lens[i])
        if ok[i]:
            a = ad[int(recs["ad_off"][i]):int(recs["ad_off"][i]) + int(recs["ad_len"][i])].tobytes()
            want = oracle.encrypt(keys[sess[i]].tobytes(), int(want_n[i]), a, pt[o:o + ln].tobytes())
            assert ct[o:o + ln + 16].tobytes() == want, (i, ln)
        else:
            assert (ct[o:o + ln + 16] == 0xA5).all(), i
    assert np.array_equal(counters(tx), n)
    # the peer: same wire order, same nonces; one tampered record
    victim = int(np.flatnonzero(ok & (sess == 20))[2])
    d_ct[int(off[victim]) + 5] ^= 1
    d_recs2 = _dev(recs.view(np.uint8))
    back = torch.full((slot_total,), 0xA5, dtype=torch.uint8, device="cuda")
    st2 = torch.full((nrec,), 0x77, dtype=torch.uint8, device="cuda")
    rx.decrypt_records(d_recs2, nrec, d_ct, back, st2, d_ad=d_ad, len_sum=int(lens.sum()))
    torch.cuda.synchronize()
    want_st2 = want_st.copy()
    want_st2[victim] = BAD_MAC
    assert np.array_equal(_host(st2), want_st2)
    back = _host(back)
    for i in np.flatnonzero(want_st2 == OK):  # the victim's later records among them
        o, ln = int(off[i]), int(lens[i])
        assert np.array_equal(back[o:o + ln], pt[o:o + ln]), i
    assert np.array_equal(counters(rx), n)
    tx.close()
    rx.close()


@pytest.mark.parametrize("L", [64, 1024])
def test_sessions_form(oracle, L):
    rng = np.random.default_rng(L)
    nsess, nrec = 40, 1200
    n0 = rng.integers(0, 1 << 48, nsess, dtype=np.uint64)
    tx, keys, n = make_table(nsess, rng, n0=n0)
    rx = noise_amd.CipherStateTable(nsess)
    rx.set(0, nsess, _dev(keys.reshape(-1)), 32, _dev(n0))
    sess = rng.integers(0, nsess, nrec).astype(np.uint32)
    pt = rng.integers(0, 256, (nrec, L), dtype=np.uint8)
    d_sess, d_pt = _dev(sess), _dev(pt.reshape(-1))
    d_ct = torch.zeros(nrec * (L + 16), dtype=torch.uint8, device="cuda")
    tx.encrypt_sessions(d_sess, d_pt, L, d_ct, L + 16, L, nrec)  # no status
    torch.cuda.synchronize()
    want_n, want_st = expect(keys, n, sess)
    assert (want_st == OK).all()
    ct = _host(d_ct).reshape(nrec, L + 16)
    for i in range(nrec):
        assert ct[i].tobytes() == oracle.encrypt(keys[sess[i]].tobytes(), int(want_n[i]), b"",
                                                 pt[i].tobytes()), i
    victim = int(np.flatnonzero(sess == sess[10])[1])
    d_ct[victim * (L + 16) + L] ^= 0x80  # its tag
    back = torch.zeros(nrec * L, dtype=torch.uint8, device="cuda")
    st = torch.full((nrec,), 0x77, dtype=torch.uint8, device="cuda")
    rx.decrypt_sessions(d_sess, d_ct, L + 16, back, L, L, st, nrec)
    torch.cuda.synchronize()
    want_st[victim] = BAD_MAC
    assert np.array_equal(_host(st), want_st)
    keep = want_st == OK
    assert np.array_equal(_host(back).reshape(nrec, L)[keep], pt[keep])
    assert np.array_equal(counters(tx), n) and np.array_equal(counters(rx), n)
    tx.close()
    rx.close()


# ---- rekey -------------------------------------------------------------------------
def test_rekey_subset_and_all(oracle):
    rng = np.random.default_rng(41)
    nsess = 200
    n0 = rng.integers(0, 1 << 60, nsess, dtype=np.uint64)
    t, keys, n = make_table(nsess, rng, keyless=(8, 100), n0=n0)
    rows = torch.zeros(32 * nsess, dtype=torch.uint8, device="cuda")
    sub = np.array([3, 199, 8, nsess, 0xFFFFFFFF, 64], np.uint32)
    t.rekey(_dev(sub), len(sub))
    t.get(0, nsess, d_keys=rows)
    torch.cuda.synchronize()
    want = keys.copy()
    for s in (3, 199, 64):
        want[s] = np.frombuffer(oracle.rekey(keys[s].tobytes()), np.uint8)
    assert np.array_equal(_host(rows).reshape(nsess, 32), want)
    t.rekey()
    t.get(0, nsess, d_keys=rows)
    torch.cuda.synchronize()
    for s in range(nsess):
        if s not in (8, 100):
            want[s] = np.frombuffer(oracle.rekey(want[s].tobytes()), np.uint8)
    got = _host(rows).reshape(nsess, 32)
    assert np.array_equal(got, want) and not got[8].any() and not got[100].any()
    assert np.array_equal(counters(t), n0)
    t.close()


# ---- the C++ view ------------------------------------------------------------------
def test_cpp_device_cipher_states():
    """noise::DeviceCipherStates (host/noise_amd/device_states.hpp) against the
    host noise::CipherState: tests/cpp/device_states_test.cpp."""
    import os
    import subprocess
    exe = os.path.join(noise_amd.ROOT, "noise-cpp_amd", "bin", "device_states_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- end to end: handshake -> split -> tables -> transport ------------------------------
def test_handshake_split_tables_transport():
    n, L, bad = 96, 64, 17
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
            buf[bad * 128 + 40] ^= 1  # session 17's second message is corrupted on the wire
        r.read_message(noise_amd.span(buf, stride=128, length=ov), d_status=st)
    k = [torch.zeros(32 * n, dtype=torch.uint8, device="cuda") for _ in range(4)]
    I.split(k[0], k[1])
    R.split(k[2], k[3])
    # each side: a sending and a receiving CipherState per session, straight from the split rows
    tabs = [noise_amd.CipherStateTable(n) for _ in range(4)]
    for t, rows in zip(tabs, k):
        t.set(0, n, rows)
    i_send, i_recv, r_recv, r_send = tabs
    nrec = 3 * n
    for rnd in range(3):
        for send, recv in ((i_send, r_recv), (r_send, i_recv)):
            sess = _dev(rng.permutation(np.repeat(np.arange(n), 3)).astype(np.uint32))
            pt = _dev(rng.integers(0, 256, nrec * L, dtype=np.uint8))
            ct = torch.zeros(nrec * (L + 16), dtype=torch.uint8, device="cuda")
            back = torch.full((nrec * L,), 0xA5, dtype=torch.uint8, device="cuda")
            s1 = torch.zeros(nrec, dtype=torch.uint8, device="cuda")
            s2 = torch.zeros(nrec, dtype=torch.uint8, device="cuda")
            send.encrypt_sessions(sess, pt, L, ct, L + 16, L, nrec, d_status=s1)
            recv.decrypt_sessions(sess, ct, L + 16, back, L, L, s2, nrec)
            torch.cuda.synchronize()
            failed = _host(sess, np.uint32) == bad
            want = np.where(failed, BAD_KEY, OK).astype(np.uint8)
            assert np.array_equal(_host(s1), want) and np.array_equal(_host(s2), want)
            good = ~failed
            assert np.array_equal(_host(back).reshape(nrec, L)[good], _host(pt).reshape(nrec, L)[good])
            assert (_host(back).reshape(nrec, L)[failed] == 0xA5).all()
    want_ctr = np.full(n, 9, np.uint64)
    want_ctr[bad] = 0
    for t in tabs:
        assert np.array_equal(counters(t), want_ctr)
        t.close()
    I.close()
    R.close()
