"""Crafted Poly1305 edge states through every AEAD kernel path on the GPU.

Every other GPU test feeds random, synthetic or constant records, whose
Poly1305 accumulator is a random residue mod p = 2^130 - 5: the band
p <= h < 2^130 on entry to poly_final, a lane / segment partial sum held as
p + T on entry to to26 / mul26 / from26, the tag addition that carries through
all four words are never reached.  tests/poly_craft.py solves one ciphertext
block per record so that they are (tests/test_poly_edges.py is the CPU twin).

Every test, with crafted records ct || tag:
  * decrypts them: REC_OK and the plaintext the CPU oracle gives (and the
    reference's library where oracle/_ref is built);
  * encrypts that plaintext: ct || tag byte for byte -- the tag is the one the
    big-integer reference predicted;
  * flips the tag's low bit on every seventh record: REC_BAD_MAC and a zeroed
    copy (noise_gpu.h: out of place), E_MAC and an untouched buffer on the
    host entry points; every other record as before.

Final residues per shape: poly_craft.TARGETS and the two tag targets (tag all
zero with a carry out of every word, tag all ones).  Partial sums
{0, 4, p - 1, 2^130 - 7}: each 256-byte lane of a tile, each 1 KiB segment and
the tail unit of a segmented record; {0, 4, p - 1} after block 0, block 1 and
the last whole block of the one-lane walk.  A range with no whole ciphertext
block (the 1-byte tail of 2049) cannot be crafted and is no pair; neither is
"0 after block 0 without AD" ((c + 2^128) r = 0 has no 16-byte solution).
A (shape, target) pair is dropped only when no block came out after 64 redraws
of the other blocks and 40 of the nonce (uniform batches and a CipherState's
run fix the nonce by position: there a job waits for the next position), at
most 2 % per test and never a target in 0..4; the count is printed."""
import collections
import ctypes
import random

import numpy as np
import pytest

import noise_amd
import poly_craft as pc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

Item = collections.namedtuple("Item", "ki n ad L ct tag label")
FILL = 0xC3


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    noise_amd.load()
    torch.cuda.set_device(0)


def dev(b):
    a = np.frombuffer(bytes(b), dtype=np.uint8).copy()
    if a.size == 0:
        a = np.zeros(1, dtype=np.uint8)
    return torch.from_numpy(a).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().tobytes()


def nonce_stream(rng):
    while True:
        yield rng.getrandbits(64) % noise_amd.NONCE_LIMIT


# ---- the three steps ----------------------------------------------------------
def exercise(oracle, keys, items, run, what):
    """run(decrypt, items, inputs) -> (outputs, statuses)."""
    assert items
    wires = [it.ct + it.tag for it in items]
    pts = []
    for it, w in zip(items, wires):
        pt = oracle.decrypt(keys[it.ki], it.n, it.ad, w)
        assert pt is not None, (what, it.L, it.label)
        if oracle.ref is not None:
            assert oracle.decrypt(keys[it.ki], it.n, it.ad, w, lib=oracle.ref) == pt, (what, it.L, it.label)
        pts.append(pt)
    out, st = run(True, items, wires)
    for i, it in enumerate(items):
        assert st[i] == noise_amd.REC_OK, (what, "decrypt status", st[i], i, it.L, len(it.ad), it.label)
        assert out[i] == pts[i], (what, "plaintext", i, it.L, len(it.ad), it.label)
    out, _ = run(False, items, pts)
    for i, it in enumerate(items):
        assert out[i][:it.L] == it.ct, (what, "ciphertext", i, it.L, len(it.ad), it.label)
        assert out[i][it.L:] == it.tag, (what, "tag", out[i][it.L:].hex(), it.tag.hex(), i, it.L, len(it.ad),
                                          it.label)
    bad = []
    for i, w in enumerate(wires):
        if i % 7 == 3:
            w = bytearray(w)
            w[items[i].L] ^= 1
        bad.append(bytes(w))
    out, st = run(True, items, bad)
    for i, it in enumerate(items):
        if i % 7 == 3:
            assert st[i] == noise_amd.REC_BAD_MAC, (what, "tampered", st[i], i, it.L, it.label)
            # a failed copy is zeroed; the host entry points leave the caller's buffer as it was
            assert out[i] == (bad[i][:it.L] if run.in_place_on_failure else bytes(it.L)), (
                what, "output of a failed record", i, it.L, it.label)
        else:
            assert st[i] == noise_amd.REC_OK and out[i] == pts[i], (what, "beside a tampered one", i, it.L,
                                                                     it.label)


# ---- entry points --------------------------------------------------------------
def records_entry(keys):
    """noise_gpu_{en,de}crypt_records, every record at 16-byte aligned offsets, out of place."""
    d_keys = dev(b"".join(keys))

    def run(decrypt, items, inputs):
        n = len(items)
        desc = np.zeros(n, dtype=noise_amd.record_dtype())
        in_off = out_off = ad_off = 0
        for i, it in enumerate(items):
            lin, lout = (it.L + 16, it.L) if decrypt else (it.L, it.L + 16)
            desc[i] = (in_off, out_off, it.n, ad_off, it.L, len(it.ad), it.ki, 0)
            in_off += lin + 16 + (-lin % 16)
            out_off += lout + 16 + (-lout % 16)
            ad_off += len(it.ad) + (-len(it.ad) % 16)
        inb, adb = bytearray(in_off), bytearray(max(ad_off, 16))
        for i, it in enumerate(items):
            o = int(desc[i]["in_off"])
            inb[o:o + len(inputs[i])] = inputs[i]
            o = int(desc[i]["ad_off"])
            adb[o:o + len(it.ad)] = it.ad
        d_out = torch.full((out_off,), FILL, dtype=torch.uint8, device="cuda")
        d_desc, d_in, d_ad = dev(desc.view(np.uint8)), dev(inb), dev(adb)
        st = None
        if decrypt:
            d_st = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
            noise_amd.decrypt_records(d_keys, len(keys), d_desc, n, d_in, d_out, d_st, d_ad)
            st = list(host(d_st))
        else:
            noise_amd.encrypt_records(d_keys, len(keys), d_desc, n, d_in, d_out, d_ad)
        out = host(d_out)
        res = []
        for i, it in enumerate(items):
            o, lout = int(desc[i]["out_off"]), (it.L if decrypt else it.L + 16)
            res.append(out[o:o + lout])
            assert out[o + lout:o + lout + 16] == bytes([FILL]) * 16, ("wrote past the record", i, it.L)
        return res, st
    run.in_place_on_failure = False
    return run


def sessions_entry(keys, L):
    """noise_gpu_{en,de}crypt_sessions: per-record key index and nonce, padded strides."""
    d_keys = dev(b"".join(keys))
    stride = L + 48

    def run(decrypt, items, inputs):
        n = len(items)
        buf = np.zeros(n * stride, dtype=np.uint8)
        for i, b in enumerate(inputs):
            buf[i * stride:i * stride + len(b)] = np.frombuffer(b, dtype=np.uint8)
        d_idx = dev(np.array([it.ki for it in items], dtype=np.uint32).view(np.uint8))
        d_non = dev(np.array([it.n for it in items], dtype=np.uint64).view(np.uint8))
        d_in = torch.from_numpy(buf).cuda()
        d_out = torch.full((n * stride,), FILL, dtype=torch.uint8, device="cuda")
        st = None
        if decrypt:
            d_st = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
            noise_amd.decrypt_sessions(d_keys, len(keys), d_idx, d_non, d_in, stride, d_out, stride, L, d_st, n)
            st = list(host(d_st))
        else:
            noise_amd.encrypt_sessions(d_keys, len(keys), d_idx, d_non, d_in, stride, d_out, stride, L, n)
        out = host(d_out)
        lout = L if decrypt else L + 16
        for i in range(n):
            assert out[i * stride + lout:(i + 1) * stride] == bytes([FILL]) * (stride - lout), ("wrote past", i)
        return [out[i * stride:i * stride + lout] for i in range(n)], st
    run.in_place_on_failure = False
    return run


def uniform_entry(key, n0, L, ad):
    """noise_gpu_{en,de}crypt_uniform: record i at nonce n0 + i, one AD for all, padded strides."""
    stride = (L + 16 + 15) // 16 * 16 + 16

    def run(decrypt, items, inputs):
        n = len(items)
        assert [it.n for it in items] == [(n0 + i) % 2**64 for i in range(n)]
        buf = np.zeros(n * stride, dtype=np.uint8)
        for i, b in enumerate(inputs):
            buf[i * stride:i * stride + len(b)] = np.frombuffer(b, dtype=np.uint8)
        d_in = torch.from_numpy(buf).cuda()
        d_out = torch.full((n * stride,), FILL, dtype=torch.uint8, device="cuda")
        d_ad = dev(ad) if ad else None
        st = None
        if decrypt:
            d_st = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
            noise_amd.decrypt_uniform(key, n0, d_in, stride, d_out, stride, L, d_st, n, d_ad=d_ad, ad_stride=0,
                                      ad_len=len(ad))
            st = list(host(d_st))
        else:
            noise_amd.encrypt_uniform(key, n0, d_in, stride, d_out, stride, L, n, d_ad=d_ad, ad_stride=0,
                                      ad_len=len(ad))
        out = host(d_out)
        lout = L if decrypt else L + 16
        for i in range(n):
            assert out[i * stride + lout:(i + 1) * stride] == bytes([FILL]) * (stride - lout), ("wrote past", i)
        return [out[i * stride:i * stride + lout] for i in range(n)], st
    run.in_place_on_failure = False
    return run


def host_entry(key):
    """noise_gpu_{en,de}crypt_host, one record per call in nonce order."""
    lib = noise_amd.load()

    def run(decrypt, items, inputs):
        res, st = [], []
        for it, b in zip(items, inputs):
            if not decrypt:
                res.append(noise_amd.encrypt_host(key, it.n, it.ad, b))
                continue
            buf = ctypes.create_string_buffer(b, len(b))
            rc = lib.noise_gpu_decrypt_host(key, it.n, it.ad or None, len(it.ad), buf, len(b))
            assert rc in (noise_amd.OK, noise_amd.E_MAC), (rc, it.L, it.label)
            if rc == noise_amd.E_MAC:
                assert buf.raw == b, ("a failed record's buffer was written", it.L, it.label)
            res.append(buf.raw[:it.L])
            st.append(noise_amd.REC_OK if rc == noise_amd.OK else noise_amd.REC_BAD_MAC)
        return res, st
    run.in_place_on_failure = True
    return run


# ---- crafted sets ---------------------------------------------------------------
def finals(tally, key, ki, nonces, ad, L, rng, shape=None):
    """Every final-residue target at one shape, nonces redrawn."""
    out = []
    jobs = [(T, T) for T in pc.TARGETS] + [(("tag", i), lambda s, i=i: pc.TAG_TARGETS(s)[i]) for i in range(2)]
    for label, T in jobs:
        got = tally.add(shape or (L, len(ad)), label, pc.final_any_nonce(key, nonces, ad, L, T, rng))
        if got:
            n, ct, tag = got
            if isinstance(label, tuple):
                assert tag == (bytes(16), b"\xff" * 16)[label[1]]
            out.append(Item(ki, n, ad, L, ct, tag, ("final", label)))
    return out


def prefixes(tally, key, ki, nonces, L, groups, targets, rng, ad=b"", shape=None):
    """groups: lists of block ranges crafted into one record each, per target."""
    out = []
    for ranges in groups:
        ranges = [r for r in ranges if pc.has_whole_block(L, r)]
        if not ranges:
            continue
        for T in targets:
            if T == 0 and not ad and (0, 0) in ranges:
                continue  # no 16-byte c has (c + 2^128) r = 0
            got = tally.add(shape or (L, len(ad), tuple(ranges[:2])), T,
                            pc.prefix_any_nonce(key, nonces, L, ranges, T, rng, ad=ad))
            if got:
                n, ct, tag = got
                out.append(Item(ki, n, ad, L, ct, tag, ("prefix", ranges[0], len(ranges), T)))
    return out


def fillers(oracle, keys, nonces, L, count, rng):
    out = []
    for _ in range(count):
        ki, n = rng.randrange(len(keys)), next(nonces)
        w = oracle.encrypt(keys[ki], n, b"", rng.randbytes(L))
        out.append(Item(ki, n, b"", L, w[:L], w[L:], "filler"))
    return out


def sequence(tally, key, n0, ad, L, jobs, rng, shape):
    """Items at the nonces n0, n0 + 1, ...; the jobs never placed count as dropped."""
    placed, left = pc.craft_sequence(key, n0, ad, L, jobs, rng)
    for label, _ in jobs:
        tally.add(shape, label[-1] if label[0] != "tag" else label, None if label in left else True)
    return [Item(0, n, ad, L, w[:L], w[L:], label or "filler") for n, label, w in placed]


# ---- the paths --------------------------------------------------------------------
@pytest.mark.parametrize("L", [64, 256, 512, 1024, 2048])
def test_exact_tile_sessions(oracle, L):
    """Exact tile kernel, keyed: G = 1 (64, 256), one product (512), the log-tree
    (1024, 2048).  Final residues; every lane's 16-block sum."""
    rng = random.Random(0xE0 + L)
    keys = [rng.randbytes(32) for _ in range(3)]
    nonces = nonce_stream(rng)
    tally = pc.Tally("sessions L=%d" % L)
    items = finals(tally, keys[1], 1, nonces, b"", L, rng)
    lanes = pc.exact_lanes(L)
    items += prefixes(tally, keys[2], 2, nonces, L, [[r] for r in lanes], pc.PREFIX_TARGETS, rng)
    if len(lanes) > 1:  # all lanes at once
        items += prefixes(tally, keys[0], 0, nonces, L, [lanes], pc.PREFIX_TARGETS, rng)
    tally.check()
    rng.shuffle(items)
    exercise(oracle, keys, items, sessions_entry(keys, L), "sessions L=%d" % L)


MASKED = [(100, 128), (300, 512), (700, 1024), (1000, 1024), (2047, 2048)]  # (len, descriptor class capacity)
SEGMENTED = [3000, 2049, 5120 - 16, 65519]


def test_records_masked_tile_and_segments(oracle):
    """One classified batch (>= 2048 descriptors): the masked tile classes with a
    partial last lane, and long records as 1 KiB segments + tail + finalize."""
    rng = random.Random(0xE1)
    keys = [rng.randbytes(32) for _ in range(5)]
    nonces = nonce_stream(rng)
    tally = pc.Tally("records batch")
    items = []
    for L, cap in MASKED:
        ki = rng.randrange(5)
        items += finals(tally, keys[ki], ki, nonces, b"", L, rng)
        lanes = pc.masked_lanes(L, cap)
        items += prefixes(tally, keys[ki], ki, nonces, L, [[r] for r in lanes], pc.PREFIX_TARGETS, rng)
    for L in SEGMENTED:
        ki = rng.randrange(5)
        items += finals(tally, keys[ki], ki, nonces, b"", L, rng)
        segs, tail, lanes = pc.segment_units(L)
        units = segs + ([tail] if tail else [])
        if L <= 5120:  # one record per unit and target
            groups = [[r] for r in units + lanes]
        else:          # the 64 KiB records: every unit of a kind at once, one record per target
            groups = [units, lanes]
        items += prefixes(tally, keys[ki], ki, nonces, L, groups, pc.PREFIX_TARGETS, rng)
        if L <= 5120:
            items += prefixes(tally, keys[ki], ki, nonces, L, [units], pc.PREFIX_TARGETS, rng)
    tally.check()
    assert sum(it.L > 5120 for it in items) <= 32 and all(it.L == 65519 for it in items if it.L > 5120)
    items += fillers(oracle, keys, nonces, 64, max(0, 2100 - len(items)), rng)
    rng.shuffle(items)
    assert 2048 <= len(items) <= 4096
    exercise(oracle, keys, items, records_entry(keys), "records batch")


WALK = [16, 17, 100, 1024]
ADS = [b"", bytes(range(0xB0, 0xB7)), bytes(range(0xC0, 0xD0))]


def walk_ranges(L):
    """after block 0, after block 1, after the last whole block"""
    return sorted({(0, k) for k in (0, 1, L // 16 - 1) if k <= L // 16 - 1})


def test_lane_per_record_descriptors(oracle):
    """Below 2048 descriptors every record takes one lane (chachapoly_device.hpp
    aead_record, vector and byte-granular): final residues, and the walk's state
    p + T / p - 1 on entry to the next poly_block."""
    rng = random.Random(0xE2)
    keys = [rng.randbytes(32) for _ in range(2)]
    nonces = nonce_stream(rng)
    tally = pc.Tally("lane per record")
    items = []
    for L in WALK:
        for ad in ADS:
            ki = rng.randrange(2)
            items += finals(tally, keys[ki], ki, nonces, ad, L, rng)
            items += prefixes(tally, keys[ki], ki, nonces, L, [[r] for r in walk_ranges(L)], pc.WALK_TARGETS, rng,
                              ad=ad)
    tally.check()
    rng.shuffle(items)
    assert len(items) < 2048
    exercise(oracle, keys, items, records_entry(keys), "lane per record")


@pytest.mark.parametrize("adlen", [7, 16])
@pytest.mark.parametrize("L", WALK)
def test_lane_per_record_uniform_with_ad(oracle, L, adlen):
    """Uniform batches with AD run one lane per record; the nonce is the position."""
    rng = random.Random(0xE3 * 4096 + L * 32 + adlen)
    key, ad = rng.randbytes(32), rng.randbytes(adlen)
    n0 = 2**32 - 9  # crosses the nonce's word carry
    tally = pc.Tally("uniform with AD L=%d" % L)
    jobs = pc.final_jobs(key, ad, L, rng) + pc.prefix_jobs(key, ad, L, walk_ranges(L), pc.WALK_TARGETS, rng)
    items = sequence(tally, key, n0, ad, L, jobs, rng, (L, adlen))
    tally.check()
    exercise(oracle, [key], items, uniform_entry(key, n0, L, ad), "uniform with AD L=%d" % L)


@pytest.mark.parametrize("L,cap", [(1024, 0), (1000, 1024), (300, 320)])
def test_uniform_tile_kernels(oracle, L, cap):
    """Uniform batches without AD: the exact tile kernel (1024: G = 4, one
    product), the masked one (1000) and its one-lane capacity (300 in 320)."""
    rng = random.Random(0xE4 * 4096 + L)
    key = rng.randbytes(32)
    n0 = 2**64 - 20  # wraps inside the batch
    lanes = pc.masked_lanes(L, cap) if cap else pc.exact_lanes(L)
    tally = pc.Tally("uniform tile L=%d" % L)
    jobs = pc.final_jobs(key, b"", L, rng) + pc.prefix_jobs(key, b"", L, lanes, pc.PREFIX_TARGETS, rng)
    items = sequence(tally, key, n0, b"", L, jobs, rng, (L,))
    tally.check()
    exercise(oracle, [key], items, uniform_entry(key, n0, L, b""), "uniform tile L=%d" % L)


@pytest.mark.parametrize("resident", [False, True])
def test_single_record_host(oracle, resident):
    """noise_gpu_{en,de}crypt_host: a launch per record, and the resident
    workgroup, whose speculation on (key, n + 1) serves the run of nonces."""
    rng = random.Random(0xE5)
    key = rng.randbytes(32)
    tally = pc.Tally("single record")
    sets = []
    for L, ad in [(64, b""), (1000, b""), (1000, bytes(range(7))), (4032, b"")]:
        n0 = rng.getrandbits(40)
        sets.append((L, ad, sequence(tally, key, n0, ad, L, pc.final_jobs(key, ad, L, rng), rng, (L, len(ad)))))
    tally.check()
    if resident:
        noise_amd.set_resident(True, 50000)
    try:
        for L, ad, items in sets:
            exercise(oracle, [key], items, host_entry(key), "host L=%d resident=%s" % (L, resident))
    finally:
        if resident:
            noise_amd.set_resident(False)
