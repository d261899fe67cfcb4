"""Poly1305 edge states on the CPU (the twin of tests/test_gpu_poly_edges.py).

Random records leave the Poly1305 accumulator a random residue mod
p = 2^130 - 5, so they never make h >= p on entry to the final reduction
(probability ~2^-125), never hold a partial sum as p + T, never make the tag
addition carry through all four words.  tests/poly_craft.py solves one
ciphertext block so that a record's residue, or the sum of a run of blocks, is
a chosen target.  Here:

* RFC 8439 appendix A.3 Poly1305 vectors #1-#11
  (tests/golden/poly1305_edge_vectors.tsv) through the big-integer
  make_fixtures.poly1305: the reference everything else leans on.
* The crafter against the C oracle (and the reference's library where
  oracle/_ref is built): every crafted record decrypts, and re-encrypting the
  plaintext returns ct || tag with the tag the crafter predicted.
* tools/emu/emu_poly_edges: the kernels' own poly_block / poly_final / to26 /
  carry26 / from26 / mul26 compiled for the host (ASan + UBSan, a stand-alone
  program fed over stdin) against the Python tags: the block chain and
  poly_final; the chain, to26, two carries, from26, poly_final; the G-lane
  recombination, G = 2..64; one product per block summed limb-wise, two
  carries, from26, poly_final.  The program reports how many vectors had
  h >= p on entry to poly_final, and how many of those p <= h < 2^130; every
  count must be non-zero.
Test infrastructure only: the product runs these kernels on the GPU."""
import os
import random
import subprocess

import pytest

import poly_craft as pc
from make_fixtures import poly1305
from oracle_lib import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tools", "emu")
JOBS = "-j%d" % max(1, min(8, os.cpu_count() or 1))

LENGTHS = [16, 17, 64, 100, 256, 1000, 1024]
ADS = [b"", bytes(range(0xA0, 0xA7))]


def edge_vectors():
    rows = []
    for line in open(os.path.join(GOLDEN, "poly1305_edge_vectors.tsv")):
        if line.strip() and not line.startswith("#"):
            name, key, msg, tag = line.rstrip("\n").split("\t")
            rows.append((name, bytes.fromhex(key), bytes.fromhex(msg), bytes.fromhex(tag)))
    return rows


def test_rfc8439_a3_vectors():
    rows = edge_vectors()
    assert [r[0] for r in rows[:11]] == ["rfc8439_a3_%d" % i for i in range(1, 12)]
    for name, key, msg, tag in rows:
        assert len(key) == 32 and len(tag) == 16
        assert poly1305(key, msg) == tag, name


def crafted_records():
    """(L, ad, target label, key, n, ct, tag) over LENGTHS x ADS x every target;
    fixed seed.  Short records have one free block, so the nonce is redrawn."""
    rng = random.Random(0x706F6C79)
    key = rng.randbytes(32)
    tally = pc.Tally("crafter")
    out = []
    nonces = iter(range(1 << 20, 1 << 40))
    for L in LENGTHS:
        for ad in ADS:
            targets = [(T, T) for T in pc.TARGETS] + [(("tag", i), lambda s, i=i: pc.TAG_TARGETS(s)[i])
                                                      for i in range(2)]
            for label, T in targets:
                got = tally.add((L, len(ad)), label, pc.final_any_nonce(key, nonces, ad, L, T, rng))
                if got:
                    out.append((L, ad, label, key) + got)
    tally.check()
    return out


@pytest.fixture(scope="module")
def crafted():
    return crafted_records()


def test_crafted_records_have_their_residue(crafted):
    zero = ones = 0
    for L, ad, label, key, n, ct, tag in crafted:
        assert len(ct) == L
        r, s = pc.otk(key, n)
        T = pc.residue(key, n, ad, ct)
        assert tag == pc.tag_of(T, s)
        if isinstance(label, int):
            assert T == label
        else:
            assert tag == (bytes(16), b"\xff" * 16)[label[1]]
            zero += label[1] == 0
            ones += label[1] == 1
        # the same tag from the plain reference over the AEAD's MAC input
        otk = r.to_bytes(16, "little") + s.to_bytes(16, "little")
        data = ad + bytes(-len(ad) % 16) + ct + bytes(-L % 16) + len(ad).to_bytes(8, "little") + L.to_bytes(8, "little")
        assert poly1305(otk, data) == tag
    assert zero and ones  # the all-zero and the all-ones tag both occur


def _roundtrip(oracle, crafted, lib):
    for L, ad, label, key, n, ct, tag in crafted:
        pt = oracle.decrypt(key, n, ad, ct + tag, lib=lib)
        assert pt is not None, (L, len(ad), label)
        assert oracle.encrypt(key, n, ad, pt, lib=lib) == ct + tag, (L, len(ad), label)
        bad = bytearray(ct + tag)
        bad[L] ^= 1
        assert oracle.decrypt(key, n, ad, bytes(bad), lib=lib) is None


def test_crafted_records_against_oracle(oracle, crafted):
    _roundtrip(oracle, crafted, None)


def test_crafted_records_against_reference(oracle, crafted):
    if oracle.ref is None:
        pytest.skip("oracle/_ref not built")
    _roundtrip(oracle, crafted, oracle.ref)


# ---- the device functions on the host ----------------------------------------
def _line(r, s, blocks, tag):
    return " ".join([r.to_bytes(16, "little").hex(), s.to_bytes(16, "little").hex(), str(len(blocks))] +
                    [b.hex() for b in blocks] + [tag.hex()])


def _tag(r, s, blocks):
    msg = b"".join(blocks)
    return poly1305((r & pc.CLAMP).to_bytes(16, "little") + s.to_bytes(16, "little"), msg)


def _solve_blocks(r, blocks, first, last, T, rng):
    """Redraw blocks first..last (whole 16-byte blocks) until their Horner sum
    from a zero accumulator is T: poly_craft's method on a bare block list."""
    for _ in range(pc.RETRIES * 4):
        for i in range(first, last + 1):
            blocks[i] = rng.randbytes(16)
        j = rng.randrange(first, last + 1)
        blocks[j] = bytes(16)
        ints = [int.from_bytes(b, "little") | pc.HIBIT for b in blocks[first:last + 1]]
        c = pc._solve(r, T, pc._horner(r, ints), last - j + 1)
        if c is not None:
            blocks[j] = c.to_bytes(16, "little")
            ints = [int.from_bytes(b, "little") | pc.HIBIT for b in blocks[first:last + 1]]
            assert pc._horner(r, ints) == T
            return True
        if first == last:
            break
    return False


def emu_vectors():
    """Lines for emu_poly_edges, with what each is for."""
    rng = random.Random(0x65646765)
    lines = []
    ALL = pc.CLAMP  # every clamped bit of r set
    # the A.3 vectors
    for name, key, msg, tag in edge_vectors():
        blocks = [msg[i:i + 16] for i in range(0, len(msg), 16)]
        lines.append(_line(int.from_bytes(key[:16], "little"), int.from_bytes(key[16:], "little"), blocks, tag))
    # the largest r over all-ones blocks, every length the lanes take and a few odd ones
    for nb in [1, 2, 5, 16, 63, 64, 65] + [16 * G + 1 for G in (2, 4, 8, 16, 32, 64)]:
        for s in (0, pc.M128, rng.getrandbits(128)):
            blocks = [b"\xff" * 16] * nb
            lines.append(_line(ALL, s, blocks, _tag(ALL, s, blocks)))
    tally = pc.Tally("emu vectors")
    rs = [ALL] + [rng.getrandbits(128) & pc.CLAMP for _ in range(3)]
    # chosen final residues
    for r in rs:
        for nb in (1, 2, 4, 17, 64, 65):
            s = rng.getrandbits(128)
            for T in pc.TARGETS + pc.TAG_TARGETS(s):
                if nb == 1 and T == 0:
                    continue  # (c + 2^128) r = 0 has no solution c < 2^128: not a pair
                blocks = [rng.randbytes(16) for _ in range(nb)]
                ok = _solve_blocks(r, blocks, 0, nb - 1, T, rng)
                for _ in range(pc.NONCE_REDRAWS if nb == 1 else 0):
                    if ok:  # a single block has one solution per r: redraw r (free here) instead
                        break
                    r = rng.getrandbits(128) & pc.CLAMP
                    ok = _solve_blocks(r, blocks, 0, 0, T, rng)
                if tally.add(("final", nb), T, ok or None):
                    tag = _tag(r, s, blocks)
                    assert tag == pc.tag_of(T, s)
                    lines.append(_line(r, s, blocks, tag))
    # chosen lane sums: every lane's 16 blocks sum to T, and the record ends in one more block
    for r in rs:
        for G in (2, 4, 8, 16, 32, 64):
            for T in pc.PREFIX_TARGETS:
                s = rng.getrandbits(128)
                blocks = [rng.randbytes(16) for _ in range(16 * G + 1)]
                ok = all(_solve_blocks(r, blocks, 16 * j, 16 * j + 15, T, rng) for j in range(G))
                if tally.add(("lanes", G), T, ok or None):
                    lines.append(_line(r, s, blocks, _tag(r, s, blocks)))
    # both at once: lane sums T and a chosen final residue through the last block
    for r in rs:
        for G in (2, 4, 64):
            for T in pc.MUST_HAVE:
                s = rng.getrandbits(128)
                blocks = [rng.randbytes(16) for _ in range(16 * G + 1)]
                ok = all(_solve_blocks(r, blocks, 16 * j, 16 * j + 15, 4 - T, rng) for j in range(G))
                if ok:
                    # the last block alone decides the final residue: H = (H_lanes + m) r
                    ints = [int.from_bytes(b, "little") | pc.HIBIT for b in blocks[:-1]]
                    c = pc._solve(r, T, (pc._horner(r, ints) + pc.HIBIT) * r % pc.P, 1)
                    ok = c is not None
                    if ok:
                        blocks[-1] = c.to_bytes(16, "little")
                if ok:  # one solution per (r, lanes): an extra, not counted when it gives no block
                    tag = _tag(r, s, blocks)
                    assert tag == pc.tag_of(T, s)
                    lines.append(_line(r, s, blocks, tag))
    tally.check()
    return lines


def _counts(stdout):
    import re
    m = re.search(r"h >= p on entry to poly_final: chain (\d+), ending (\d+), products (\d+)", stdout)
    b = re.search(r"of these p <= h < 2\^130: chain (\d+), ending (\d+), products (\d+)", stdout)
    k = re.search(r"lane sums h >= p on entry to to26: (\d+) of (\d+)", stdout)
    assert m and b and k, stdout[-2000:]
    return [int(x) for x in m.groups()], [int(x) for x in b.groups()], int(k.group(1))


def run_emu(lines, binary=None):
    binary = binary or os.path.join(EMU, "build", "emu_poly_edges")
    return subprocess.run([binary], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600,
                          env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))


def test_device_functions_on_chosen_residues():
    r = subprocess.run(["make", JOBS, "-C", EMU, "polyedges"], capture_output=True, text=True, timeout=1200)
    if r.returncode != 0:
        pytest.fail("emulation build failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])
    lines = emu_vectors()
    r = run_emu(lines)
    print(r.stdout[-600:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert "vectors %d\n" % len(lines) in r.stdout
    assert "ok (0 failures)" in r.stdout
    ge, band, lanes = _counts(r.stdout)
    # without these the test could silently stop reaching the final subtraction:
    # h >= p in every ending, and in each also the band p <= h < 2^130 that only
    # the carry of h + 5 through all four words detects (random records reach
    # h >= 2^130 now and then, that band never)
    assert min(ge) > 0 and min(band) > 0 and lanes > 0
