"""Every tag bit on the CPU (the twin of tests/test_gpu_tag_bits.py).

* The references themselves: the C oracle, and the reference's library where
  oracle/_ref is built, reject a flip of each of the 128 tag bits and accept
  the genuine record, at len 0, 1, 16, 1024, with and without AD.
* The kernels in the emulation: tools/emu/emu_tagbits (the unmodified kernels
  compiled for the host under AddressSanitizer, a stand-alone program run as
  a subprocess; it only runs the decrypt and hands back statuses and output
  bytes) on the 384-record sweep of tests/tag_sweep.py, with that module's
  assertions against the oracle, out of place and in place, through
    the exact tile kernel (uniform 64 and 1024; the nonces cross 2^32),
    the masked tile kernel (uniform 300 and 1000),
    the lane walk (uniform with a 7-byte AD, vector 64 and byte-granular 77),
    classified descriptor batches (the emulation classifies from 64 records):
      exact classes 64 and 1024 and ragged classes 100 and 700 (the masked
      tile kernel, kMTDesc), segmented 2049 and 3000 (k_seg_finalize_w; len
      % 16 = 1 and 8: both load16 variants read the tag), generic records
      (16 bytes of AD; input off by 1),
    unclassified descriptors (calls of 48 < 64 records: aead_record).
  The latency kernel (noise_gpu_decrypt_host) is left to the GPU test: one
  emulated launch of its 256 threads costs 0.2-0.6 s (tests/test_emu_kernels.py),
  so 128 tampered calls and their genuine twins would be the longest job of
  that module's pool.
Test infrastructure only: the product runs these kernels on the GPU."""
import os
import random
import struct
import subprocess

import pytest

import tag_sweep as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tools", "emu")
JOBS = "-j%d" % max(1, min(8, os.cpu_count() or 1))


# ---- the references -------------------------------------------------------------
def _reference_sweep(oracle, lib):
    rng = random.Random(0x7A6B)
    for L in (0, 1, 16, 1024):
        for ad in (b"", bytes(range(0xA0, 0xA7))):
            key, n, pt = rng.randbytes(32), rng.getrandbits(64) % (2**64 - 2), rng.randbytes(L)
            w = oracle.encrypt(key, n, ad, pt, lib=lib)
            assert len(w) == L + 16
            assert oracle.decrypt(key, n, ad, w, lib=lib) == pt, (L, len(ad), "genuine")
            for b in range(ts.NBITS):
                assert oracle.decrypt(key, n, ad, ts.flip(w, b), lib=lib) is None, (L, len(ad), "tag bit %d" % b)


def test_oracle_rejects_every_tag_bit(oracle):
    _reference_sweep(oracle, None)


def test_reference_library_rejects_every_tag_bit(oracle):
    if oracle.ref is None:
        pytest.skip("oracle/_ref not built")
    _reference_sweep(oracle, oracle.ref)
    # and the two agree on the bytes the sweeps are built from
    key = bytes(range(32))
    assert oracle.encrypt(key, 5, b"ad", b"x" * 100, lib=oracle.ref) == oracle.encrypt(key, 5, b"ad", b"x" * 100)


def test_sweep_construction():
    """384 records, record j tampered iff j % 3 == 1 in tag bit j // 3: each
    bit once, nothing but that bit."""
    wire = bytes(range(40)) + bytes(16)
    seen = set()
    for j in range(ts.NREC):
        if ts.tampered(j):
            t = ts.flip(wire, j // 3)
            diff = int.from_bytes(bytes(x ^ y for x, y in zip(t, wire)), "little")
            assert diff >> (8 * 40) == 1 << (j // 3) and diff & ((1 << 320) - 1) == 0
            seen.add(j // 3)
    assert seen == set(range(128)) and sum(ts.tampered(j) for j in range(ts.NREC)) == 128
    assert not ts.tampered(-2) and not ts.tampered(0) and ts.tampered(1) and not ts.tampered(2)


# ---- the kernels in the emulation -------------------------------------------------
class EmuBackend:
    """One emu_tagbits process; a job goes down its stdin, the statuses and the
    output image come back on its stdout."""

    def __init__(self, binary):
        self.p = subprocess.Popen([binary], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                  env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))

    def _job(self, blob, nrec, out_size):
        try:
            self.p.stdin.write(blob)
            self.p.stdin.flush()
            head = self.p.stdout.read(16)
        except BrokenPipeError:
            head = b""
        if len(head) != 16:
            self.p.stdin.close()
            err = self.p.stderr.read().decode(errors="replace")
            pytest.fail("emu_tagbits ended (exit %s):\n%s" % (self.p.wait(), err[-6000:]))
        assert struct.unpack("<QQ", head) == (nrec, out_size)
        st, out = self.p.stdout.read(nrec), self.p.stdout.read(out_size)
        assert len(st) == nrec and len(out) == out_size
        return out, st

    def uniform(self, key, n0, inbuf, in_off, in_stride, out_size, out_off, out_stride, L, ad, nrec, in_place):
        blob = struct.pack("<IIQQ", 0, int(in_place), len(inbuf), out_size) + key + struct.pack(
            "<QQQQQIIQ", n0 % 2**64, in_off, in_stride, out_off, out_stride, L, len(ad), nrec) + ad + inbuf
        return self._job(blob, nrec, out_size)

    def records(self, keys, desc, inbuf, adbuf, out_size, in_place):
        adbuf = adbuf + bytes(-len(adbuf) % 16)
        blob = struct.pack("<IIQQ", 1, int(in_place), len(inbuf), out_size) + struct.pack(
            "<IIQQ", len(keys), 0, len(desc), len(adbuf)) + b"".join(keys) + desc.tobytes() + adbuf + inbuf
        return self._job(blob, len(desc), out_size)

    def close(self):
        self.p.stdin.close()
        err = self.p.stderr.read().decode(errors="replace")
        rc = self.p.wait(timeout=120)
        assert rc == 0, err[-6000:]


@pytest.fixture(scope="module")
def emu():
    r = subprocess.run(["make", JOBS, "-C", EMU, "GRID_CAP=3u", "tagbits"], capture_output=True, text=True,
                       timeout=1200)
    if r.returncode != 0:
        pytest.fail("emulation build failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])
    be = EmuBackend(os.path.join(EMU, "build", "emu_tagbits"))
    yield be
    be.close()


N0 = 2**32 - 200  # the sweep crosses the nonce's word carry: the host splits the exact tile launch
UNIFORM = [  # (path, len, ad, layout)
    ("exact tile", 64, b"", "packed"), ("exact tile", 1024, b"", "packed"), ("exact tile", 64, b"", "padded"),
    ("masked tile", 300, b"", "padded"), ("masked tile", 1000, b"", "padded"),
    ("lane walk, vector", 64, bytes(range(7)), "padded"), ("lane walk, bytes", 77, bytes(range(7)), "padded"),
]


@pytest.mark.parametrize("in_place", [False, True], ids=["copy", "inplace"])
@pytest.mark.parametrize("path,L,ad,layout", UNIFORM, ids=["%s-%d-%s" % (c[0].replace(" ", "_").replace(",", ""), c[1], c[3])
                                                          for c in UNIFORM])
def test_uniform_emulated(oracle, emu, path, L, ad, layout, in_place):
    rng = random.Random(0xB175 + L + len(ad))
    ts.run_uniform(emu, "emulated uniform, " + path, oracle, rng.randbytes(32), N0, L, ad, rng, layout, in_place)


AD16 = bytes(range(0xD0, 0xE0))
RECORDS = [  # (family, len, ad, input misalignment, descriptors per call)
    ("exact class", 64, b"", 0, None), ("exact class", 1024, b"", 0, None),
    ("ragged class", 100, b"", 0, None), ("ragged class", 700, b"", 0, None),
    ("segmented", 2049, b"", 0, None), ("segmented", 3000, b"", 0, None),
    ("generic, AD", 65, AD16, 0, None), ("generic, input off by 1", 79, b"", 1, None),
    ("unclassified", 17, b"", 0, 48), ("unclassified", 1024, b"", 0, 48),
]


@pytest.mark.parametrize("in_place", [False, True], ids=["copy", "inplace"])
@pytest.mark.parametrize("family,L,ad,misalign,per_call", RECORDS,
                         ids=["%s-%d" % (c[0].split(",")[-1].strip().replace(" ", "_"), c[1]) for c in RECORDS])
def test_records_emulated(oracle, emu, family, L, ad, misalign, per_call, in_place):
    rng = random.Random(0xB176 + L + misalign)
    keys = [rng.randbytes(32) for _ in range(5)]
    ts.run_records(emu, "emulated records, " + family, oracle, keys, lambda r: (r.randrange(5), ad, L), rng,
                   in_place, misalign=misalign, per_call=per_call)
