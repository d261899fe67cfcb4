"""Every bit of the tag on every decrypt path of the GPU.

Every decrypt ends in (want.x ^ tag[0]) | (want.y ^ tag[1]) | (want.z ^ tag[2])
| (want.w ^ tag[3]); seven places hold that line, and a genuine record cannot
tell whether one of them skips a word, masks a bit or reads the received tag a
slot off.  tests/tag_sweep.py builds 384 records of which 128 carry one flipped
tag bit each; here that batch goes through every entry and shape that reaches
one of the seven (tests/test_tag_bits.py is the CPU twin).

Compare site -> entries and shapes, read from the dispatch (tile_classes.hpp
uniform_path / len_class, aead_kernels.hip, sessions_kernels.hip,
records_kernels.hip launch_classes, single_kernels.hip):

  tile_kernel.hpp:726   k_aead_tile, one instantiation per (DECRYPT, L, CONTIG,
      MODE): uniform batches, aligned, no AD, len in ExactLens (kTileUniform;
      CONTIG = packed strides; a batch whose nonces cross a multiple of 2^32
      is two launches), and the sessions entry (kTileSessions, both CONTIG).
      test_uniform_exact_tile, test_sessions, test_cipherstate_table[sessions].
      (The exact DESCRIPTOR classes do not come here: since the masked kernel
      took them over -- tile_kernel.hpp:95 -- launch_classes starts
      k_aead_mtile<kMTDesc> for the exact-size and the ragged records of a
      capacity alike.)
  mtile_kernel.hpp:716  k_aead_mtile: uniform, aligned, no AD, any other len up
      to 16 KiB at the smallest of the 21 MaskedCaps that holds it
      (kMTUniform); descriptor batches of >= 2048 records, aligned, no AD: len
      in ExactLens and every other len <= 2048 (kMTDesc, ten capacities); the
      staged uniform path (unaligned, >= 1024 records) runs the exact or the
      masked kernel on an aligned image and k_stage_out copies back by status.
      test_uniform_masked_tile, test_uniform_staged, test_records_classified
      [exact / ragged].
  records_kernels.hip:574  k_seg_finalize_w: classified descriptors with 2048 <
      len <= 65535 that are not 4, 8 or 16 KiB; the received tag comes through
      load16<true> (len % 16 == 0) or load16<false>, and R.ok gates the
      keystream passes.  test_records_classified[segmented], lengths with len
      % 16 in {0, 1, 15}.
  chachapoly_device.hpp:541  aead_record<VEC>: uniform batches with AD, or
      unaligned below 1024 records (k_aead_uniform); descriptor batches below
      2048 records, and the generic class of larger ones (AD, unaligned, len >
      65535: k_aead_records); the handshake's DecryptAndHash
      (handshake_kernels.hip:266).  test_uniform_lane_walk,
      test_records_classified[generic], test_records_unclassified,
      test_handshake_*, test_replay_window_* (256 records of len 100),
      test_cipherstate_table[records] (384 descriptors).
  single_kernels.hip:317 / :345  one_body, the launch per record of
      noise_gpu_decrypt_host: P = na + nl + 1 Poly1305 blocks, one wave for P
      <= 256, four above (:245); keystream by quads below 64 blocks (:176).
      len 1000: quads, one wave; 1001: an unaligned tag copy; 4064: 64 blocks,
      no quads, P = 255, one wave; 5000: four waves.  test_host_entry_launch.
  single_kernels.hip:697  one_body_fast, the resident workgroup serving a
      record whose (key, nonce) it speculated on.  test_host_entry_resident.

In place and out of place wherever the entry has both.  All lengths, layouts
and batch sizes are fixed; nothing is sampled."""
import ctypes
import random
import struct

import numpy as np
import pytest

import noise_amd
import tag_sweep as ts

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

OK, BAD_MAC, REPLAY = noise_amd.REC_OK, noise_amd.REC_BAD_MAC, noise_amd.REC_REPLAY
LIMIT = noise_amd.NONCE_LIMIT
N0 = 2**32 - 200  # the sweep crosses the nonce's word carry, where the host splits the exact tile launch
EXACT = [64, 128, 192, 256, 512, 1024, 2048, 4096, 8192, 16384]                      # tile_classes.hpp ExactLens
CAPS = [64, 128, 192, 256, 320, 384, 448, 512, 768, 1024, 1280, 1536, 1792, 2048,
        2304, 2560, 3072, 4096, 5120, 8192, 16384]                                   # tile_classes.hpp MaskedCaps
CLASSIFY_MIN = 2048  # records_kernels.hip kClassifyMin
STAGE_MIN = 1024     # tile_classes.hpp kStageMin
COPY_OR_IN_PLACE = pytest.mark.parametrize("in_place", [False, True], ids=["copy", "inplace"])


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    noise_amd.load()
    torch.cuda.set_device(0)


@pytest.fixture(scope="module")
def gpu():
    return ts.GpuBackend()


# ---- uniform batches ----------------------------------------------------------------
UNIFORM_EXACT = ([(L, "packed", False) for L in EXACT] + [(L, "padded", False) for L in (64, 1024, 16384)] +
                 [(L, "padded", True) for L in (64, 1024, 16384)])


@pytest.mark.parametrize("L,layout,in_place", UNIFORM_EXACT,
                         ids=["%d-%s-%s" % (L, lay, "inplace" if ip else "copy") for L, lay, ip in UNIFORM_EXACT])
def test_uniform_exact_tile(oracle, gpu, L, layout, in_place):
    rng = random.Random(0x7A60000 + L)
    ts.run_uniform(gpu, "uniform, exact tile", oracle, rng.randbytes(32), N0, L, b"", rng, layout, in_place)


UNIFORM_MASKED = [(cap - 1, False) for cap in CAPS] + [(L, True) for L in (300, 1000, 5000)]


@pytest.mark.parametrize("L,in_place", UNIFORM_MASKED,
                         ids=["%d-%s" % (L, "inplace" if ip else "copy") for L, ip in UNIFORM_MASKED])
def test_uniform_masked_tile(oracle, gpu, L, in_place):
    rng = random.Random(0x7A61000 + L)
    ts.run_uniform(gpu, "uniform, masked tile", oracle, rng.randbytes(32), N0, L, b"", rng, "padded", in_place)


@COPY_OR_IN_PLACE
def test_uniform_staged(oracle, gpu, in_place):
    """Base off by 3, 1024 genuine records and then the sweep: staged through an
    aligned image, the masked kernel at capacity 128, k_stage_out by status."""
    rng = random.Random(0x7A62000)
    ts.run_uniform(gpu, "uniform, staged", oracle, rng.randbytes(32), N0, 100, b"", rng, "misaligned", in_place,
                   nfill=STAGE_MIN)


@COPY_OR_IN_PLACE
@pytest.mark.parametrize("L,ad,layout", [(64, bytes(range(7)), "padded"), (77, bytes(range(7)), "padded"),
                                         (64, b"", "misaligned")], ids=["vector-ad7", "bytes-ad7", "misaligned"])
def test_uniform_lane_walk(oracle, gpu, L, ad, layout, in_place):
    """aead_record<VEC> (64 with AD, aligned) and aead_record<false> (77; a
    misaligned base below kStageMin records)."""
    rng = random.Random(0x7A63000 + L + len(ad))
    ts.run_uniform(gpu, "uniform, lane walk", oracle, rng.randbytes(32), N0, L, ad, rng, layout, in_place)


# ---- sessions -----------------------------------------------------------------------
@pytest.mark.parametrize("layout,in_place", [("packed", False), ("padded", False), ("padded", True)],
                         ids=["packed-copy", "padded-copy", "padded-inplace"])
@pytest.mark.parametrize("L", [256, 2048])
def test_sessions(oracle, gpu, L, layout, in_place):
    rng = random.Random(0x7A64000 + L)
    keys = [rng.randbytes(32) for _ in range(5)]
    ts.run_sessions(gpu, "sessions", oracle, keys, L, rng, layout, in_place)


# ---- descriptor batches ---------------------------------------------------------------
AD16 = bytes(range(0xD0, 0xE0))
CLASSIFIED = [  # (family, len, ad, input misalignment)
    ("exact", 64, b"", 0), ("exact", 1024, b"", 0), ("ragged", 100, b"", 0), ("ragged", 700, b"", 0),
    ("segmented", 2049, b"", 0), ("segmented", 3000, b"", 0), ("segmented", 5120 - 16, b"", 0),
    ("segmented", 65519, b"", 0),  # len % 16 = 1, 8, 0, 15
    ("generic-ad16", 81, AD16, 0), ("generic-off1", 79, b"", 1), ("generic-long", 70000, b"", 0),  # % 16 = 1, 15, 0
]


@COPY_OR_IN_PLACE
@pytest.mark.parametrize("family,L,ad,misalign", CLASSIFIED, ids=["%s-%d" % (c[0], c[1]) for c in CLASSIFIED])
def test_records_classified(oracle, gpu, family, L, ad, misalign, in_place):
    """>= 2048 descriptors: genuine 64-byte records up to the threshold, then
    the sweep of one family."""
    rng = random.Random(0x7A65000 + L + misalign)
    keys = [rng.randbytes(32) for _ in range(5)]
    ts.run_records(gpu, "records, classified, " + family, oracle, keys, lambda r: (r.randrange(5), ad, L), rng,
                   in_place, nfill=CLASSIFY_MIN - ts.NREC, misalign=misalign)


@COPY_OR_IN_PLACE
@pytest.mark.parametrize("L", [17, 1024])
def test_records_unclassified(oracle, gpu, L, in_place):
    rng = random.Random(0x7A66000 + L)
    keys = [rng.randbytes(32) for _ in range(5)]
    ts.run_records(gpu, "records, 384 descriptors", oracle, keys, lambda r: (r.randrange(5), b"", L), rng, in_place)


# ---- the host entry ---------------------------------------------------------------------
def _host_decrypt(lib, key, n, wire):
    buf = ctypes.create_string_buffer(wire, len(wire))
    rc = lib.noise_gpu_decrypt_host(key, n, None, 0, buf, len(wire))
    return rc, buf.raw


def _launch_path(oracle, lib, L, what):
    """128 tampered calls, one per bit, and the genuine record after each."""
    rng = random.Random(0x7A67000 + L)
    key, n, pt = rng.randbytes(32), rng.getrandbits(40), rng.randbytes(L)
    wire = oracle.encrypt(key, n, b"", pt)
    f = ts.Findings(what, "in place", "len %d" % L)
    for b in range(ts.NBITS):
        bad = ts.flip(wire, b)
        rc, raw = _host_decrypt(lib, key, n, bad)
        assert rc in (noise_amd.OK, noise_amd.E_MAC), (what, L, b, rc)
        f.bit(rc == noise_amd.E_MAC, b, "status %d" % rc)
        f.bit(rc != noise_amd.E_MAC or raw == bad, b, "a failed record's buffer was written")
        rc, raw = _host_decrypt(lib, key, n, wire)
        f.other(rc == noise_amd.OK and raw[:L] == pt, b, "the genuine record after the tampered one: %d" % rc)
    f.verdict()


@pytest.mark.parametrize("L", [1000, 1001, 4064, 5000])
def test_host_entry_launch(oracle, L):
    _launch_path(oracle, noise_amd.load(), L, "host entry, launch per record")


@pytest.mark.parametrize("L", [1000, 3040, 5000])
def test_host_entry_resident(oracle, L):
    """The resident workgroup: after the genuine record at n0 + 2j it holds the
    speculation for (key, n0 + 2j + 1), so by the hit condition of
    single_kernels.hip:921-931 (same key, that nonce, no more keystream and
    Poly1305 blocks than speculated: the same length) the record tampered in
    bit j at n0 + 2j + 1 is the one one_body_fast serves.  The test cannot see
    which body ran -- a missed speculation falls back to one_body, with the
    same verdict -- it can only put every bit where the fast body's compare
    is the one that has to reject it.  5000 bytes are over kResidentMaxLen and
    take the launch path with the resident mode on."""
    lib = noise_amd.load()
    noise_amd.set_resident(True, 50000)
    try:
        if L > 63 * 64:
            _launch_path(oracle, lib, L, "host entry, resident mode on, launch path")
            return
        rng = random.Random(0x7A68000 + L)
        key, n0 = rng.randbytes(32), rng.getrandbits(40)
        f = ts.Findings("host entry, resident", "in place", "len %d" % L)
        for j in range(ts.NBITS):
            pt = rng.randbytes(L)
            rc, raw = _host_decrypt(lib, key, n0 + 2 * j, oracle.encrypt(key, n0 + 2 * j, b"", pt))
            f.other(rc == noise_amd.OK and raw[:L] == pt, j, "the genuine record before the tampered one: %d" % rc)
            bad = ts.flip(oracle.encrypt(key, n0 + 2 * j + 1, b"", rng.randbytes(L)), j)
            rc, raw = _host_decrypt(lib, key, n0 + 2 * j + 1, bad)
            assert rc in (noise_amd.OK, noise_amd.E_MAC), ("host entry, resident", L, j, rc)
            f.bit(rc == noise_amd.E_MAC, j, "status %d" % rc)
            f.bit(rc != noise_amd.E_MAC or raw == bad, j, "a failed record's buffer was written")
        f.verdict()
    finally:
        noise_amd.set_resident(False)


# ---- batched handshake ------------------------------------------------------------------------
HS_N, HS_PAY = 384, 5


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def _np(t, dtype=np.uint8):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(dtype)


def _xx_sweep(message, tag_at):
    """XX, 384 sessions, 5-byte payloads; the sweep's bit flipped in the 16
    bytes at tag_at of `message` (0-based) before its reader sees it.
    -> (reader's statuses of that message, its payload rows, reader's key rows,
    peer's key rows, the payload sent)."""
    n = HS_N
    rng = np.random.default_rng(0x7A69 + 16 * message + tag_at)
    I, R = noise_amd.HandshakeBatch("XX", True, n), noise_amd.HandshakeBatch("XX", False, n)
    try:
        for hs in (I, R):
            hs.set_key(noise_amd.HS_S, _dev(rng.integers(0, 256, n * 32, dtype=np.uint8)))
            hs.set_key(noise_amd.HS_E, _dev(rng.integers(0, 256, n * 32, dtype=np.uint8)))
            hs.start()
        seen = None
        for m in range(3):
            w, r = (I, R) if m % 2 == 0 else (R, I)
            mlen = w.info().overhead + HS_PAY
            sent = rng.integers(1, 256, (n, 8), dtype=np.uint8)  # no zero byte: a zeroed payload is not the genuine one
            buf = torch.zeros(n * 128, dtype=torch.uint8, device="cuda")
            w.write_message(noise_amd.span(buf, stride=128), payload=noise_amd.span(_dev(sent.reshape(-1)), stride=8,
                                                                                   length=HS_PAY))
            if m == message:
                wire = _np(buf).copy().reshape(n, 128)
                assert tag_at + 16 <= mlen
                for i in range(n):
                    if ts.tampered(i):
                        b = i // 3
                        wire[i, tag_at + (b >> 3)] ^= 1 << (b & 7)
                buf = _dev(wire.reshape(-1))
            pay = torch.full((n * 16,), ts.FILL, dtype=torch.uint8, device="cuda")
            st = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
            r.read_message(noise_amd.span(buf, stride=128, length=mlen), payload=noise_amd.span(pay, stride=16),
                           d_status=st)
            if m == message:
                seen = (_np(st).copy(), _np(pay).copy().reshape(n, 16), sent[:, :HS_PAY], r is I)
            elif m < message:
                assert not _np(st).any()
        st, pay, sent, reader_is_initiator = seen
        rows = [torch.full((n * 32,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(4)]
        I.split(rows[0], rows[1])
        R.split(rows[2], rows[3])
        ki, kr = [np.stack([_np(rows[a]).reshape(n, 32), _np(rows[a + 1]).reshape(n, 32)]) for a in (0, 2)]
        return st, pay, sent, (ki, kr) if reader_is_initiator else (kr, ki)
    finally:
        I.close()
        R.close()


def _check_handshake(what, st, pay, sent, reader_keys, peer_keys, payload_written):
    """payload_written: the failing AEAD is the payload's own, whose failed copy
    is zeroed; otherwise the session failed before it and its row is untouched."""
    f = ts.Findings(what, "XX, %d sessions" % HS_N, "payload len %d" % HS_PAY)
    for i in range(HS_N):
        if ts.tampered(i):
            f.bit(st[i] == noise_amd.HS_BAD_MAC, i // 3, "status %d" % st[i])
            if payload_written:
                f.bit(not pay[i, :HS_PAY].any(), i // 3, "payload bytes of a failed session")
            else:
                f.bit((pay[i, :HS_PAY] == ts.FILL).all(), i // 3, "the payload of a session that failed before it was written")
            f.bit((pay[i, HS_PAY:] == ts.FILL).all(), i // 3, "wrote past the payload")
            f.bit(not reader_keys[:, i].any(), i // 3, "split gave a failed session a key")
        else:
            f.other(st[i] == noise_amd.HS_OK, i, "status %d" % st[i])
            f.other(np.array_equal(pay[i, :HS_PAY], sent[i]), i, "payload")
            f.other(reader_keys[:, i].any(axis=1).all(), i, "keyless")
            f.other(np.array_equal(reader_keys[:, i], peer_keys[:, i]), i, "split disagrees with the peer")
    f.verdict()


def test_handshake_message2_payload_tag():
    """XX message 2 read by the initiator, its last 16 bytes: the payload's
    tag.  The failed DecryptAndHash zeroes the payload (out of place)."""
    st, pay, sent, (rk, pk) = _xx_sweep(1, 96 + HS_PAY - 16)
    _check_handshake("handshake, message 2, payload tag", st, pay, sent, rk, pk, True)


def test_handshake_message2_static_key_tag():
    """XX message 2, bytes 64..79: the tag of the encrypted s.  A session that
    fails there is skipped by every later kernel (noise_gpu.h: a failed session
    stays failed, later calls skip it), the payload's included: its payload
    row is not written at all.  The row being untouched, not merely free of
    plaintext, is what pins this compare: MixHash(ct || tag) binds the flipped
    bit into h, so a session whose s tag were let through would still end in
    HS_BAD_MAC one step later, at the payload's AEAD -- which zeroes the row."""
    st, pay, sent, (rk, pk) = _xx_sweep(1, 64)
    _check_handshake("handshake, message 2, tag of s", st, pay, sent, rk, pk, False)


def test_handshake_message3_static_key_tag():
    """XX message 3 read by the responder, bytes 32..47: the tag of the
    encrypted s; the payload row as in message 2."""
    st, pay, sent, (rk, pk) = _xx_sweep(2, 32)
    _check_handshake("handshake, message 3, tag of s", st, pay, sent, rk, pk, False)


# ---- the replay window ---------------------------------------------------------------------------
WIN_L = 100
WIN_BASES = [0, (1 << 32) - 1, 5000, LIMIT - 1]  # as tests/test_gpu_cswin.py: 0, near 2^32, mid, the last valid nonce


def _window_table(rng):
    keys = rng.integers(0, 256, (ts.NBITS, 32), dtype=np.uint8)
    keys[:, 0] |= 1
    t = noise_amd.CipherStateTable(ts.NBITS)
    t.set(0, ts.NBITS, _dev(keys.reshape(-1)), 32, _dev(np.full(ts.NBITS, 7, np.uint64)))
    return t, keys


def _window_records(oracle, keys, rng):
    """Session b: the record at nonce n_b tampered in bit b, then the genuine one."""
    nonces = [WIN_BASES[b % 4] for b in range(ts.NBITS)]
    pts = [bytes(rng.integers(0, 256, WIN_L, dtype=np.uint8)) for _ in range(ts.NBITS)]
    wires = [oracle.encrypt(keys[b].tobytes(), nonces[b], b"", pts[b]) for b in range(ts.NBITS)]
    return nonces, pts, wires


def _check_window_rows(t, nonces, what):
    d_next = torch.full((ts.NBITS,), -1, dtype=torch.int64, device="cuda")
    d_bits = torch.full((ts.NBITS * 128,), 0xEE, dtype=torch.uint8, device="cuda")
    t.window_get(0, ts.NBITS, d_next, d_bits)
    nxt, bits = _np(d_next, np.uint64), _np(d_bits).reshape(ts.NBITS, 128)
    for b, n in enumerate(nonces):
        assert int(nxt[b]) == n + 1, (what, "session %d" % b, "next", int(nxt[b]), n + 1)
        want = np.frombuffer((1 << (n % 1024)).to_bytes(128, "little"), np.uint8)
        assert np.array_equal(bits[b], want), (what, "session %d" % b, "window bits")
    d_n = torch.zeros(ts.NBITS, dtype=torch.int64, device="cuda")
    t.get(0, ts.NBITS, d_n=d_n)
    assert (_np(d_n, np.uint64) == 7).all(), (what, "the in-order counters moved")


def _check_window_call(what, call, st, out, ranges, pts, first):
    """Record 2b is session b's tampered record, 2b + 1 the genuine one.  first:
    [BAD_MAC, OK], a zeroed copy and the plaintext; again: both REC_REPLAY,
    rejected against the window at entry, so nothing is written."""
    f = ts.Findings(what, call, "out of place", "len %d" % WIN_L)
    for b in range(ts.NBITS):
        (o0, o1) = ranges[2 * b], ranges[2 * b + 1]
        pair = "statuses %d, %d" % (st[2 * b], st[2 * b + 1])
        if first:
            f.bit((st[2 * b], st[2 * b + 1]) == (BAD_MAC, OK), b, pair)
            f.bit(out[o0:o0 + WIN_L] == bytes(WIN_L), b, "a failed copy is not zero")
            f.bit(out[o1:o1 + WIN_L] == pts[b], b, "plaintext of the genuine record")
        else:
            f.bit((st[2 * b], st[2 * b + 1]) == (REPLAY, REPLAY), b, pair)
            f.bit(out[o0:o0 + WIN_L] == out[o1:o1 + WIN_L] == bytes([ts.FILL]) * WIN_L, b, "a replay was written")
    f.verdict()


def test_replay_window_records(oracle, gpu):
    rng = np.random.default_rng(0x7A6A)
    t, keys = _window_table(rng)
    try:
        nonces, pts, wires = _window_records(oracle, keys, rng)
        items, inputs = [], []
        for b in range(ts.NBITS):
            it = ts.Item(b, nonces[b], b"", WIN_L, wires[b][:WIN_L], wires[b][WIN_L:])
            items += [it, it]
            inputs += [ts.flip(wires[b], b), wires[b]]
        desc, inbuf, adbuf, out_size = ts.records_layout(items, inputs, 0, False)
        ranges = [int(o) for o in desc["out_off"]]
        for first in (True, False):
            d_out, d_st = gpu.fill(out_size), gpu.fill(len(items), 9)
            t.decrypt_records_window(gpu.dev(desc.view(np.uint8)), len(items), gpu.dev(inbuf), d_out, d_st)
            out, st = gpu.host(d_out), gpu.host(d_st)
            call = "first call" if first else "the same records again"
            _check_window_call("replay window, records", call, st, out, ranges, pts, first)
            ts.records_outputs("replay window, records", desc, items, out, None)
            _check_window_rows(t, nonces, "replay window, records, " + call)
    finally:
        t.close()


def test_replay_window_datagrams(oracle, gpu):
    rng = np.random.default_rng(0x7A6B)
    t, keys = _window_table(rng)
    try:
        nonces, pts, wires = _window_records(oracle, keys, rng)
        TYPE, plen = 4, 16 + WIN_L + 16
        slot, oslot = ts.ceil16(plen) + 16, ts.ceil16(WIN_L) + 16
        img = bytearray([ts.FILL]) * (2 * ts.NBITS * slot)
        for b in range(ts.NBITS):
            hdr = struct.pack("<IIQ", TYPE, b, nonces[b])
            for k, w in enumerate((ts.flip(wires[b], b), wires[b])):
                img[(2 * b + k) * slot:(2 * b + k) * slot + plen] = hdr + w
        nrec = 2 * ts.NBITS
        off = _dev(np.arange(nrec, dtype=np.uint64) * slot)
        ooff = _dev(np.arange(nrec, dtype=np.uint64) * oslot)
        ranges = [i * oslot for i in range(nrec)]
        d_len = _dev(np.full(nrec, plen, np.uint32))
        for first in (True, False):
            d_pkt, d_out, d_st = gpu.dev(img), gpu.fill(nrec * oslot), gpu.fill(nrec, 9)
            d_recs = gpu.fill(48 * nrec, 0x77)
            t.open_datagrams(TYPE, noise_amd.span(d_pkt, off=off, lens=d_len), noise_amd.span(d_out, off=ooff),
                             d_recs, d_st, nrec)
            out, st = gpu.host(d_out), gpu.host(d_st)
            call = "first call" if first else "the same packets again"
            _check_window_call("replay window, datagrams", call, st, out, ranges, pts, first)
            for i in range(nrec):
                assert out[i * oslot + WIN_L:(i + 1) * oslot] == bytes([ts.FILL]) * (oslot - WIN_L), ("wrote past", i)
            assert gpu.host(d_pkt) == bytes(img), "open wrote to the packets"
            _check_window_rows(t, nonces, "replay window, datagrams, " + call)
    finally:
        t.close()


# ---- the in-order tables ---------------------------------------------------------------------------
class TableBackend(ts.GpuBackend):
    """CipherStateTable.decrypt_sessions / .decrypt_records in place of the
    plain entries: the key index is the session, and the nonces are the
    table's -- session s starts at START[s] and takes them in record order, so
    the sweep's records are made for exactly those."""
    START = [0, 7, (1 << 32) - 30, 1 << 40, LIMIT - 1000]

    def __init__(self, keys):
        super().__init__()
        self.t = noise_amd.CipherStateTable(len(keys))
        self.t.set(0, len(keys), self.dev(b"".join(keys)), 32, _dev(np.array(self.START, np.uint64)))
        self.count = [0] * len(keys)

    def specs(self, sessions, L):
        out = []
        for s in sessions:
            out.append((s, self.START[s] + self.count[s], b"", L))
            self.count[s] += 1
        return out

    def counters(self):
        d_n = torch.zeros(len(self.START), dtype=torch.int64, device="cuda")
        self.t.get(0, len(self.START), d_n=d_n)
        return [int(x) for x in _np(d_n, np.uint64)]

    def sessions(self, keys, idx, nonces, inbuf, in_stride, out_size, out_stride, L, nrec, in_place):
        d_in = self.dev(inbuf)
        d_out = d_in if in_place else self.fill(out_size)
        d_st = self.fill(nrec, 9)
        self.t.decrypt_sessions(_dev(np.array(idx, np.uint32)), d_in, in_stride, d_out, out_stride, L, d_st, nrec)
        return self.host(d_out)[:out_size], self.host(d_st)[:nrec]

    def records(self, keys, desc, inbuf, adbuf, out_size, in_place):
        desc = desc.copy()
        want = desc["nonce"].copy()
        desc["nonce"] = 0x5555555555555555  # the call fills them in
        d_desc, d_in = self.dev(desc.view(np.uint8)), self.dev(inbuf)
        d_out = d_in if in_place else self.fill(out_size)
        d_st = self.fill(len(desc), 9)
        self.t.decrypt_records(d_desc, len(desc), d_in, d_out, d_st, d_ad=self.dev(adbuf))
        got = np.frombuffer(self.host(d_desc), dtype=noise_amd.record_dtype())
        assert np.array_equal(got["nonce"], want), "the table assigned other nonces"
        return self.host(d_out)[:out_size], self.host(d_st)[:len(desc)]


@COPY_OR_IN_PLACE
@pytest.mark.parametrize("entry", ["sessions", "records"])
def test_cipherstate_table(oracle, entry, in_place):
    """One sweep through each in-order table call (they compose the kernels
    above: 256-byte records, the exact tile kernel keyed by session / 384
    descriptors, aead_record), and the counter rule of noise_gpu.h: decrypt
    advances the counter for accepted records whatever their tag does."""
    rng = random.Random(0x7A6C + (entry == "records"))
    keys = [rng.randbytes(32) for _ in range(5)]
    be = TableBackend(keys)
    try:
        L = 256
        specs = be.specs([rng.randrange(5) for _ in range(ts.NREC)], L)
        items, pts = ts.make_items(oracle, keys, specs, rng)
        wires = ts.sweep_inputs(items)
        what = "CipherStateTable.decrypt_" + entry
        if entry == "sessions":
            stride = L + 48
            inbuf = bytearray([ts.FILL]) * (ts.NREC * stride)
            for i, w in enumerate(wires):
                inbuf[i * stride:i * stride + L + 16] = w
            out, st = be.sessions(keys, [it.ki for it in items], None, bytes(inbuf), stride, ts.NREC * stride,
                                  stride, L, ts.NREC, in_place)
            lout = L + 16 if in_place else L
            outs = [out[i * stride:i * stride + lout] for i in range(ts.NREC)]
            for i in range(ts.NREC):
                assert out[i * stride + lout:(i + 1) * stride] == bytes([ts.FILL]) * (stride - lout), ("wrote past", i)
        else:
            desc, inbuf, adbuf, out_size = ts.records_layout(items, wires, 0, in_place)
            out, st = be.records(keys, desc, inbuf, adbuf, out_size, in_place)
            outs = ts.records_outputs(what, desc, items, out, inbuf if in_place else None)
        ts.check(what, "table nonces", items, 0, pts, wires, outs, list(st), in_place)
        assert be.counters() == [be.START[s] + be.count[s] for s in range(5)], (what, "counters")
        assert sum(be.count) == ts.NREC and min(be.count) > 0
    finally:
        be.t.close()
