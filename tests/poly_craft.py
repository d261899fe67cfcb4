"""Crafted ChaChaPoly records whose Poly1305 state is a chosen residue.

Under a random one-time key the Poly1305 accumulator is a random residue mod
p = 2^130 - 5, so random records never reach the places where limb arithmetic
goes wrong: h >= p on entry to the final reduction, a lane or segment partial
sum held as p + T, a tag addition whose carry ripples through all four words.
The one-time key (r, s) is fixed by (key, nonce), but the MAC runs over the
ciphertext, and a ciphertext block can be solved for: with every other block
fixed, the residue is affine in one 16-byte block c_j,
    residue = H0 + c_j r^e  (mod p),    c_j = (T - H0) r^(-e)  (mod p),
and the solution is a block when it is below 2^128 (about one try in four).

Everything here is Python big integers over the ChaCha20 block function and
the layout helpers of tests/golden/make_fixtures.py; nothing comes from the
code under test.  Every crafted record is recomputed and asserted before it is
returned.  Test infrastructure only."""
import functools
import os
import struct
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_fixtures import _pad16, chacha20_block, noise_nonce  # noqa: E402

P = (1 << 130) - 5
M128 = (1 << 128) - 1
CLAMP = 0x0ffffffc0ffffffc0ffffffc0fffffff
HIBIT = 1 << 128
RETRIES = 64          # fresh random blocks per (key, nonce)
NONCE_REDRAWS = 40    # at least the 8 a (shape, target) pair is owed before it may be dropped
MAX_DROPPED = 0.02    # share of a test's (shape, target) pairs that may be left out

# final or partial residues every path is fed
TARGETS = [0, 1, 2, 3, 4, 5, P - 1, P - 2, P - 5, P - 6,
           (1 << 128) - 1, 1 << 128, 1 << 129, (1 << 130) - 7]
MUST_HAVE = (0, 1, 2, 3, 4)   # held as p + T: the final subtraction must happen
PREFIX_TARGETS = [0, 4, P - 1, (1 << 130) - 7]
WALK_TARGETS = [0, 4, P - 1]


def TAG_TARGETS(s):
    """Residues whose tag is all zero with a carry out of every word, and all ones."""
    return [(HIBIT - s) % P, (HIBIT - s - 1) % P]


@functools.lru_cache(maxsize=1 << 14)
def otk(key, n):
    """One-time Poly1305 key of (key, nonce): ChaCha20 block 0, r clamped."""
    blk = chacha20_block(key, 0, noise_nonce(n))
    return int.from_bytes(blk[:16], "little") & CLAMP, int.from_bytes(blk[16:32], "little")


def _blocks(data):
    """16-byte blocks of zero-padded data as integers with the 2^128 bit."""
    data = data + _pad16(data)
    return [int.from_bytes(data[i:i + 16], "little") | HIBIT for i in range(0, len(data), 16)]


def _horner(r, blocks, h=0):
    for m in blocks:
        h = (h + m) * r % P
    return h


def mac_blocks(ad, ct):
    return _blocks(ad) + _blocks(ct) + [int.from_bytes(struct.pack("<QQ", len(ad), len(ct)), "little") | HIBIT]


def residue(key, n, ad, ct):
    """Whole-record Poly1305 residue (before + s) of pad16(ad) | pad16(ct) | lengths."""
    r, _ = otk(key, n)
    return _horner(r, mac_blocks(ad, ct))


def prefix_sum(key, n, ct, first, last, ad=b""):
    """Horner sum over ciphertext blocks first..last from a zero accumulator
    (first == 0 with AD: from the accumulator the AD blocks leave)."""
    r, _ = otk(key, n)
    h = _horner(r, _blocks(ad)) if first == 0 and ad else 0
    return _horner(r, _blocks(ct[16 * first:16 * last + 16]), h)


def tag_of(T, s):
    return ((T + s) & M128).to_bytes(16, "little")


def _solve(r, T, H0, e):
    """c with H0 + c r^e == T (mod p), or None when it is no 16-byte block."""
    if r == 0:
        return None
    c = (T - H0) * pow(pow(r, e, P), P - 2, P) % P
    return c if c <= M128 else None


def craft_final(key, n, ad, L, T, rng):
    """(ct, tag): L ciphertext bytes whose whole-record residue under (key, n, ad)
    is T, tag = (T + s) mod 2^128; None when no try gave a block."""
    nfull = L // 16
    if nfull == 0:
        return None
    r, s = otk(key, n)
    nad, nct = (len(ad) + 15) // 16, (L + 15) // 16
    for _ in range(RETRIES):
        ct = bytearray(rng.randbytes(L))
        j = rng.randrange(nfull)
        ct[16 * j:16 * j + 16] = bytes(16)
        H0 = _horner(r, mac_blocks(ad, bytes(ct)))
        e = nad + nct + 1 - (nad + j)  # blocks from block j to the end of the MAC input
        c = _solve(r, T, H0, e)
        if c is not None:
            ct[16 * j:16 * j + 16] = c.to_bytes(16, "little")
            ct = bytes(ct)
            assert residue(key, n, ad, ct) == T
            return ct, tag_of(T, s)
        if L == 16:
            break  # a single free block and nothing else to redraw: one solution per (key, nonce)
    return None


def craft_prefix(key, n, L, first, last, T, rng, ct=None, ad=b""):
    """ct of L bytes whose sum over ciphertext blocks first..last, started from a
    zero accumulator, is T: a tile lane's or a 1 KiB segment's partial sum, or
    (first == 0) the state of the one-lane walk after block `last` -- then the
    AD blocks, if any, come first.  With `ct` given only blocks first..last of
    it are redrawn, so one record can hold several crafted ranges."""
    nct = (L + 15) // 16
    assert 0 <= first <= last < nct
    hi = min(last, L // 16 - 1)  # the free block is a whole one
    if hi < first:
        return None
    r, _ = otk(key, n)
    h_in = _horner(r, _blocks(ad)) if first == 0 and ad else 0
    base = bytearray(ct if ct is not None else rng.randbytes(L))
    lo_b, hi_b = 16 * first, min(16 * last + 16, L)
    for _ in range(RETRIES):
        base[lo_b:hi_b] = rng.randbytes(hi_b - lo_b)
        j = rng.randrange(first, hi + 1)
        base[16 * j:16 * j + 16] = bytes(16)
        H0 = _horner(r, _blocks(bytes(base[lo_b:hi_b])), h_in)
        c = _solve(r, T, H0, last - j + 1)
        if c is not None:
            base[16 * j:16 * j + 16] = c.to_bytes(16, "little")
            out = bytes(base)
            assert prefix_sum(key, n, out, first, last, ad) == T
            return out
        if first == last:
            break  # one solution per (key, nonce)
    return None


def seal(key, n, ad, ct):
    """ct || tag of a ciphertext (the tag from the big-integer reference)."""
    _, s = otk(key, n)
    return ct + tag_of(residue(key, n, ad, ct), s)


class Tally:
    """The (shape, target) pairs a test asked for and the ones it had to drop."""

    def __init__(self, what):
        self.what, self.asked, self.dropped = what, 0, []

    def add(self, shape, T, got):
        self.asked += 1
        if got is None:
            self.dropped.append((shape, T))
        return got

    def check(self):
        print("%s: %d of %d (shape, target) pairs dropped" % (self.what, len(self.dropped), self.asked))
        assert len(self.dropped) <= MAX_DROPPED * self.asked, self.dropped
        must = [d for d in self.dropped if d[1] in MUST_HAVE]
        assert not must, must


def final_any_nonce(key, nonces, ad, L, T, rng):
    """craft_final with the nonce redrawn from `nonces` (an iterator): (n, ct, tag) or None."""
    for _ in range(NONCE_REDRAWS + 1):
        n = next(nonces)
        got = craft_final(key, n, ad, L, T(otk(key, n)[1]) if callable(T) else T, rng)
        if got is not None:
            return (n,) + got
    return None


def prefix_any_nonce(key, nonces, L, ranges, T, rng, ad=b""):
    """A sealed record whose block ranges [(first, last), ...] all sum to T, the
    nonce redrawn when a range gives no block: (n, ct, tag) or None."""
    for _ in range(NONCE_REDRAWS + 1):
        n = next(nonces)
        ct = rng.randbytes(L)
        for first, last in ranges:
            ct = craft_prefix(key, n, L, first, last, T, rng, ct=ct, ad=ad)
            if ct is None:
                break
        if ct is not None:
            for first, last in ranges:
                assert prefix_sum(key, n, ct, first, last, ad) == T
            sealed = seal(key, n, ad, ct)
            return n, ct, sealed[L:]
    return None


def craft_sequence(key, n0, ad, L, jobs, rng, spare=3):
    """Records at the fixed nonces n0, n0 + 1, ... (a uniform batch, or a
    CipherState's run): position by position the next pending job is tried, a
    job that gives no block there waits for the next position and the one after
    it is tried instead.  jobs: [(label, fn(n) -> ct | None)].  Returns
    ([(n, label or None, ct || tag)], labels never placed); a position that took
    no job holds a random sealed record."""
    pending, out = list(jobs), []
    limit = spare * len(jobs) + 8
    n = n0
    while pending and len(out) < limit:
        placed = None
        for k, (label, fn) in enumerate(pending):
            ct = fn(n)
            if ct is not None:
                placed = label
                del pending[k]
                break
        if placed is None:
            ct = rng.randbytes(L)
        out.append((n, placed, seal(key, n, ad, ct)))
        n = (n + 1) % (1 << 64)
    return out, [label for label, _ in pending]


def final_jobs(key, ad, L, rng, targets=None):
    """craft_sequence jobs: every target (and the two tag targets) as the final residue."""
    jobs = []
    for T in (TARGETS if targets is None else targets):
        jobs.append((("final", T), lambda n, T=T: (craft_final(key, n, ad, L, T, rng) or (None,))[0]))
    for i in range(2):
        jobs.append((("tag", i), lambda n, i=i: (craft_final(key, n, ad, L, TAG_TARGETS(otk(key, n)[1])[i], rng)
                                                  or (None,))[0]))
    return jobs


def prefix_jobs(key, ad, L, ranges, targets, rng):
    """craft_sequence jobs: each block range summing to each target."""
    return [(("prefix", first, last, T),
             lambda n, first=first, last=last, T=T: craft_prefix(key, n, L, first, last, T, rng, ad=ad))
            for first, last in ranges for T in targets]


# ---- which blocks a lane, a segment or a tail unit sums (the kernels' layouts,
# restated from their headers: tile_kernel.hpp, mtile_kernel.hpp, records_kernels.hip)
def exact_lanes(L):
    """Exact tile kernel: lanes of 256 B (16 blocks); one lane below 256 B."""
    g = max(1, L // 256)
    bpl = L // 16 // g
    return [(bpl * j, bpl * j + bpl - 1) for j in range(g)]


def masked_lanes(L, cap, block0=0):
    """Masked tile of capacity cap: up to 7 chunks one lane; above, lanes of 4
    chunks with the record right-aligned by whole chunks (the absent chunks lead)."""
    nch = cap // 64
    g = 1 if nch <= 7 else nch // 4
    cpl = nch // g
    cc, nblk = (L + 63) // 64, (L + 15) // 16
    dc = nch - cc
    out = []
    for j in range(g):
        c_hi = cpl * j - dc + cpl - 1
        if c_hi < 0:
            continue
        c_lo = max(0, cpl * j - dc)
        out.append((block0 + 4 * c_lo, block0 + min(4 * c_hi + 3, nblk - 1)))
    return out


def segment_units(L):
    """Segmented long record: (segments, tail unit or None, 16-block lanes of the
    segments and the tail's masked 1 KiB lanes)."""
    nf, rest = L // 1024, L % 1024
    segs = [(64 * s, 64 * s + 63) for s in range(nf)]
    lanes = [(64 * s + 16 * j, 64 * s + 16 * j + 15) for s in range(nf) for j in range(4)]
    tail = None
    if rest:
        tail = (64 * nf, 64 * nf + (rest + 15) // 16 - 1)
        lanes += masked_lanes(rest, 1024, 64 * nf)
    return segs, tail, lanes


def has_whole_block(L, rng_):
    """A range can be crafted when it holds a whole ciphertext block."""
    return rng_[0] <= L // 16 - 1
