"""GPU parity of the uniform / sessions tile kernel (tile_kernel.hpp) where its
arithmetic around the ChaCha20 rounds was trimmed: one recombination product
per lane for G = 2 and 4 (L = 512, 1024) beside the kept log-tree (G = 8, 64:
L = 2048, 16384, the latter with the mid-butterfly carry), no carry before
from26, and -- uniform batches -- round-1 columns computed once per launch on
the host for the launch's high nonce word, with the batch split in two
launches where its nonces cross a multiple of 2^32.

Every case compares byte for byte with the CPU oracle (oracle_check_uniform /
oracle_check_records): partial tiles, tile and super-tile boundaries, nonce
ranges at 2^32 and 2^64, tampered tags and ciphertext (status 1 for those
records alone; zeros out of place, the buffer untouched in place), sessions
with a key index past the table and an all-zero key row (status 2, nothing
written), and records of all-0xFF / all-0x00 bytes (the largest and smallest
limbs the carry-free recombination meets).
Reference: crypto_aead_write / crypto_aead_read, monocypher.c:2899-2929;
nonce framing noise.cpp:207-215."""
import random

import numpy as np
import pytest

import noise_amd

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FILL = 0xEE
SEED = 0x7472696D


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    noise_amd.load()
    torch.cuda.set_device(0)


@pytest.fixture(scope="module")
def stream(oracle):
    """the synthetic plaintext stream, once: 130 records of 16 KiB at the most"""
    return np.frombuffer(oracle.synthetic(130 * 16384, SEED), dtype=np.uint8)


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _roundtrip(oracle, key, n0, pt, L, nrec):
    """packed encrypt, then decrypt, both exact against the oracle"""
    d_pt = torch.from_numpy(pt.copy()).cuda()
    d_ct = torch.full(((L + 16) * nrec,), FILL, dtype=torch.uint8, device="cuda")
    noise_amd.encrypt_uniform(key, n0, d_pt, L, d_ct, L + 16, L, nrec)
    ct = _np(d_ct)
    assert oracle.check_uniform(0, key, n0, pt, L, ct, L + 16, L, nrec) == (0, -1)
    d_back = torch.full((L * nrec,), FILL, dtype=torch.uint8, device="cuda")
    d_st = torch.full((nrec,), 9, dtype=torch.uint8, device="cuda")
    noise_amd.decrypt_uniform(key, n0, d_ct, L + 16, d_back, L, L, d_st, nrec)
    st, back = _np(d_st), _np(d_back)
    assert not st.any()
    assert oracle.check_uniform(1, key, n0, ct, L + 16, back, L, L, nrec, status=st) == (0, -1)
    assert np.array_equal(back, pt)
    return ct


@pytest.mark.parametrize("nrec", [1, 15, 17, 65, 130])
@pytest.mark.parametrize("L", [512, 1024, 2048, 16384])
def test_uniform_both_directions(oracle, stream, L, nrec):
    key = random.Random(L + nrec).randbytes(32)
    _roundtrip(oracle, key, 5 + nrec, stream[:L * nrec], L, nrec)


@pytest.mark.parametrize("n0", [2**32 - 70, 2**32 - 64, 2**64 - 130, 0],
                         ids=["cross_in_supertile", "cross_at_supertile", "end_2^64", "zero"])
def test_uniform_nonce_edges(oracle, stream, n0):
    """2^32 - 70: the range crosses 2^32 inside the second super-tile (the host
    splits the batch there); 2^32 - 64: at a super-tile boundary; 2^64 - 130:
    the last nonce is 2^64 - 1."""
    L, nrec = 1024, 130
    key = random.Random(n0 % 1000003).randbytes(32)
    _roundtrip(oracle, key, n0, stream[:L * nrec], L, nrec)


TAMPER = {"tag_rec0": (0, 1024 + 5), "tag_rec16": (16, 1024 + 15), "tag_rec64": (64, 1024),
          "ct_rec63": (63, 700)}


@pytest.mark.parametrize("in_place", [False, True], ids=["copy", "in_place"])
@pytest.mark.parametrize("what", sorted(TAMPER))
def test_uniform_tampered(oracle, stream, what, in_place):
    L, nrec, n0 = 1024, 65, 2**32 - 3
    key = random.Random(len(what)).randbytes(32)
    pt = stream[:L * nrec]
    ct = oracle.encrypt_uniform_np(key, n0, pt, L, L, L + 16, nrec).copy()
    bad, off = TAMPER[what]
    ct[bad * (L + 16) + off] ^= 0x04  # one bit
    d_ct = torch.from_numpy(ct.copy()).cuda()
    d_st = torch.full((nrec,), 9, dtype=torch.uint8, device="cuda")
    if in_place:
        d_out, os_ = d_ct, L + 16
    else:
        d_out, os_ = torch.full((L * nrec,), FILL, dtype=torch.uint8, device="cuda"), L
    noise_amd.decrypt_uniform(key, n0, d_ct, L + 16, d_out, os_, L, d_st, nrec)
    st, back = _np(d_st), _np(d_out)
    want_st = np.zeros(nrec, dtype=np.uint8)
    want_st[bad] = noise_amd.REC_BAD_MAC
    assert np.array_equal(st, want_st)
    assert oracle.check_uniform(1, key, n0, ct, L + 16, back, os_, L, nrec, status=st) == (0, -1)
    rows = back.reshape(nrec, os_)
    ok = np.ones(nrec, dtype=bool)
    ok[bad] = False
    assert np.array_equal(rows[ok, :L], pt.reshape(nrec, L)[ok])
    if in_place:
        want = ct.reshape(nrec, L + 16)
        assert np.array_equal(rows[bad], want[bad])           # the failed record: untouched
        assert np.array_equal(rows[:, L:], want[:, L:])       # every tag stays
    else:
        assert not rows[bad].any()                            # no unauthenticated plaintext


@pytest.mark.parametrize("L", [512, 1024])
def test_sessions(oracle, stream, L):
    nrec, nkeys = 65, 9
    rng = random.Random(L * 31)
    keys = [rng.randbytes(32) for _ in range(8)] + [bytes(32)]  # row 8: "no key"
    kidx = np.array([r % 8 for r in range(nrec)], dtype=np.uint32)
    kidx[21], kidx[64] = nkeys + 3, 8  # past the table; the all-zero row
    bad_key = [21, 64]
    nonces = np.array([(2**32 - 9 + r + (int(kidx[r]) << 36)) % 2**64 for r in range(nrec)],
                      dtype=np.uint64)
    pt = stream[:L * nrec]
    ktab = np.frombuffer(b"".join(keys), dtype=np.uint8).copy()
    d_keys = torch.from_numpy(ktab).cuda()
    d_idx = torch.from_numpy(kidx.view(np.uint8).copy()).cuda()
    d_non = torch.from_numpy(nonces.view(np.uint8).copy()).cuda()
    d_pt = torch.from_numpy(pt.copy()).cuda()
    cs = L + 16
    d_ct = torch.full((cs * nrec,), FILL, dtype=torch.uint8, device="cuda")
    noise_amd.encrypt_sessions(d_keys, nkeys, d_idx, d_non, d_pt, L, d_ct, cs, L, nrec)
    ct = _np(d_ct).copy()
    desc = np.zeros(nrec, dtype=noise_amd.record_dtype())
    r = np.arange(nrec, dtype=np.uint64)
    desc["in_off"], desc["out_off"] = r * np.uint64(L), r * np.uint64(cs)
    desc["nonce"], desc["len"], desc["key_idx"] = nonces, L, kidx
    assert oracle.check_records(0, ktab, nkeys, desc, pt, ct) == (0, -1)
    for b in bad_key:  # nothing written
        assert (ct[b * cs:(b + 1) * cs] == FILL).all(), b
    ct[5 * cs + L + 2] ^= 0x80  # and one failed tag
    d_c2 = torch.from_numpy(ct.copy()).cuda()
    d_back = torch.full((L * nrec,), FILL, dtype=torch.uint8, device="cuda")
    d_st = torch.full((nrec,), 9, dtype=torch.uint8, device="cuda")
    noise_amd.decrypt_sessions(d_keys, nkeys, d_idx, d_non, d_c2, cs, d_back, L, L, d_st, nrec)
    st, back = _np(d_st), _np(d_back)
    want_st = np.zeros(nrec, dtype=np.uint8)
    want_st[5] = noise_amd.REC_BAD_MAC
    want_st[bad_key] = noise_amd.REC_BAD_KEY
    assert np.array_equal(st, want_st)
    ddesc = desc.copy()
    ddesc["in_off"], ddesc["out_off"] = desc["out_off"], desc["in_off"]
    assert oracle.check_records(1, ktab, nkeys, ddesc, ct, back, status=st) == (0, -1)
    rows = back.reshape(nrec, L)
    ok = np.ones(nrec, dtype=bool)
    ok[[5] + bad_key] = False
    assert np.array_equal(rows[ok], pt.reshape(nrec, L)[ok])
    assert not rows[5].any()
    for b in bad_key:
        assert (rows[b] == FILL).all(), b


@pytest.mark.parametrize("byte", [0xFF, 0x00])
@pytest.mark.parametrize("L,nrec", [(1024, 65), (16384, 3)])
def test_uniform_constant_records(oracle, L, nrec, byte):
    key = random.Random(L + byte).randbytes(32)
    pt = np.full(L * nrec, byte, dtype=np.uint8)
    _roundtrip(oracle, key, 2**32 - 2, pt, L, nrec)
