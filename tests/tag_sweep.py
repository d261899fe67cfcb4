"""One sweep over the 128 bits of a record's tag, for every decrypt path.

A decrypt ends in a comparison of the computed tag with the received one.
Genuine records cannot test it: a comparison that skips a word, masks a bit or
reads the tag one slot off still accepts them.  The sweep is a batch of
NREC = 384 genuine records ct || tag from the CPU oracle in which record j is
tampered iff j % 3 == 1, by flipping exactly tag bit b = j // 3 (byte b >> 3
of the tag, mask 1 << (b & 7)): each of the 128 bits once, in 128 different
records, between 256 genuine ones.

The layouts below (plain Python: offsets, strides, buffer images) are handed
to a backend that only runs the decrypt: GpuBackend here (the C ABI through
noise_amd; tests/test_gpu_tag_bits.py) and the emulated kernels in
tests/test_tag_bits.py.  After the decrypt, for every record:
  status   tampered: REC_BAD_MAC, the others REC_OK;
  output   genuine: the oracle's plaintext; tampered, out of place: len zero
           bytes; tampered, in place: the tampered input unchanged, tag
           included;
  gaps     the bytes after each record up to its stride (or its slot): still
           the fill value.
Plain module, no fixtures: test infrastructure only."""
import collections

import numpy as np

import noise_amd

NREC, NBITS, FILL = 384, 128, 0xC3
assert NREC == 3 * NBITS

Item = collections.namedtuple("Item", "ki n ad L ct tag")


def tampered(j):
    """Record j of the sweep (j < 0: a filler before it) is a tampered one."""
    return j >= 0 and j % 3 == 1


def flip(wire, b):
    """wire = ct || tag with tag bit b flipped."""
    w = bytearray(wire)
    w[len(w) - 16 + (b >> 3)] ^= 1 << (b & 7)
    return bytes(w)


def make_items(oracle, keys, specs, rng):
    """specs: (key index, nonce, ad, len) -> genuine Items and their plaintexts."""
    items, pts = [], []
    for ki, n, ad, L in specs:
        pt = rng.randbytes(L)
        w = oracle.encrypt(keys[ki], n, ad, pt)
        items.append(Item(ki, n, ad, L, w[:L], w[L:]))
        pts.append(pt)
    return items, pts


def sweep_inputs(items, first=0):
    """The wire images of a batch whose sweep starts at record `first` (the
    records before it are genuine fillers)."""
    assert len(items) - first == NREC
    wires = []
    for i, it in enumerate(items):
        w = it.ct + it.tag
        wires.append(flip(w, (i - first) // 3) if tampered(i - first) else w)
    assert sum(w != it.ct + it.tag for w, it in zip(wires, items)) == NBITS
    return wires


class Findings:
    """What a sweep got wrong: every record is looked at before the verdict, so
    the failure names the entry, layout and length once, and all the tag bits
    (and genuine records) concerned."""

    def __init__(self, *where):
        self.where, self.bits, self.genuine = where, {}, []

    def bit(self, ok, b, reason):
        if not ok:
            self.bits.setdefault(b, reason)

    def other(self, ok, i, reason):
        if not ok:
            self.genuine.append((i, reason))

    @staticmethod
    def spans(bits):
        out, bits = [], sorted(bits)
        for b in bits:
            if out and out[-1][1] == b - 1:
                out[-1][1] = b
            else:
                out.append([b, b])
        return ",".join("%d" % a if a == b else "%d-%d" % (a, b) for a, b in out)

    def verdict(self):
        assert not self.bits and not self.genuine, self.where + (
            "tag bits " + (self.spans(self.bits) or "none"), sorted(set(self.bits.values())),
            "%d genuine records" % len(self.genuine), self.genuine[:4])


def check(what, layout, items, first, pts, wires, outs, st, in_place, ok=noise_amd.REC_OK,
          bad_mac=noise_amd.REC_BAD_MAC):
    """outs[i]: record i's output range (len bytes; in place len + 16: the whole record)."""
    assert len(outs) == len(st) == len(items)
    lens = sorted({it.L for it in items[first:]})
    f = Findings(what, layout, "in place" if in_place else "out of place", "len %s" % ",".join(map(str, lens)))
    for i, it in enumerate(items):
        j = i - first
        if tampered(j):
            f.bit(st[i] == bad_mac, j // 3, "status %d" % st[i])
            if in_place:
                f.bit(outs[i] == wires[i], j // 3, "a failed record was written in place")
            else:
                f.bit(outs[i] == bytes(it.L), j // 3, "a failed copy is not zero")
        else:
            f.other(st[i] == ok, i, "status %d" % st[i])
            f.other(outs[i][:it.L] == pts[i], i, "plaintext")
    f.verdict()


def _gap(what, buf, lo, hi, i):
    assert buf[lo:hi] == bytes([FILL]) * (hi - lo), (what, "wrote past record %d" % i, lo, hi)


def ceil16(x):
    return (x + 15) // 16 * 16


# ---- layouts ----------------------------------------------------------------------
def run_uniform(backend, what, oracle, key, n0, L, ad, rng, layout, in_place, nfill=0):
    """noise_gpu_decrypt_uniform: record i at nonce n0 + i, nfill genuine records
    before the sweep.  layout: "packed" (strides len + 16 / len), "padded"
    (16-byte aligned strides with a gap), "misaligned" (base off by 3, strides
    off 16)."""
    nrec = nfill + NREC
    items, pts = make_items(oracle, [key], [(0, (n0 + i) % 2**64, ad, L) for i in range(nrec)], rng)
    wires = sweep_inputs(items, nfill)
    base = 3 if layout == "misaligned" else 0
    if layout == "packed":
        in_stride, out_stride = L + 16, L
    elif layout == "padded":
        in_stride, out_stride = ceil16(L + 16) + 16, ceil16(L) + 32
    else:
        in_stride, out_stride = L + 16 + 5, L + 7
    if in_place:
        out_stride = in_stride
    inbuf = bytearray([FILL]) * ceil16(base + nrec * in_stride + 32)
    for i, w in enumerate(wires):
        inbuf[base + i * in_stride:base + i * in_stride + L + 16] = w
    out_size = len(inbuf) if in_place else ceil16(base + nrec * out_stride + 32)
    out, st = backend.uniform(key, n0, bytes(inbuf), base, in_stride, out_size, base, out_stride, L, ad, nrec,
                              in_place)
    lout = L + 16 if in_place else L
    outs = [out[base + i * out_stride:base + i * out_stride + lout] for i in range(nrec)]
    for i in range(nrec):
        _gap(what, out, base + i * out_stride + lout, base + (i + 1) * out_stride, i)
    _gap(what, out, 0, base, -1)
    _gap(what, out, base + nrec * out_stride, out_size, nrec)
    check(what, layout, items, nfill, pts, wires, outs, list(st), in_place)


def run_sessions(backend, what, oracle, keys, L, rng, layout, in_place):
    """noise_gpu_decrypt_sessions: a key index and a nonce per record."""
    specs = [(rng.randrange(len(keys)), rng.getrandbits(64) % noise_amd.NONCE_LIMIT, b"", L) for _ in range(NREC)]
    items, pts = make_items(oracle, keys, specs, rng)
    wires = sweep_inputs(items)
    in_stride, out_stride = (L + 16, L) if layout == "packed" else (L + 48, L + 48)
    if in_place:
        out_stride = in_stride
    inbuf = bytearray([FILL]) * (NREC * in_stride)
    for i, w in enumerate(wires):
        inbuf[i * in_stride:i * in_stride + L + 16] = w
    out_size = NREC * out_stride
    out, st = backend.sessions(keys, [it.ki for it in items], [it.n for it in items], bytes(inbuf), in_stride,
                               out_size, out_stride, L, NREC, in_place)
    lout = L + 16 if in_place else L
    outs = [out[i * out_stride:i * out_stride + lout] for i in range(NREC)]
    for i in range(NREC):
        _gap(what, out, i * out_stride + lout, (i + 1) * out_stride, i)
    check(what, layout, items, 0, pts, wires, outs, list(st), in_place)


def records_layout(items, wires, first, in_place, misalign=0):
    """Descriptors and images of a batch: every record in a 16-byte aligned
    slot with at least 16 fill bytes after it; the sweep's records (from
    `first`) pushed `misalign` bytes into their input slot.  An in-place
    record has in_off == out_off."""
    n = len(items)
    desc = np.zeros(n, dtype=noise_amd.record_dtype())
    in_off = out_off = ad_off = 0
    for i, it in enumerate(items):
        m = misalign if i >= first else 0
        desc[i] = (in_off + m, in_off + m if in_place else out_off, it.n, ad_off, it.L, len(it.ad), it.ki, 0)
        in_off += ceil16(it.L + 16 + m) + 16
        out_off += ceil16(it.L) + 16
        ad_off += ceil16(len(it.ad))
    inbuf, adbuf = bytearray([FILL]) * in_off, bytearray(max(ad_off, 16))
    for i, it in enumerate(items):
        o = int(desc[i]["in_off"])
        inbuf[o:o + it.L + 16] = wires[i]
        o = int(desc[i]["ad_off"])
        adbuf[o:o + len(it.ad)] = it.ad
    return desc, bytes(inbuf), bytes(adbuf), (in_off if in_place else out_off)


def records_outputs(what, desc, items, out, initial):
    """Every record's output range of the image `out`; every byte outside
    them is what it was (initial: the input image in place, None: the fill)."""
    outs, own = [], np.zeros(len(out), dtype=bool)
    for i, it in enumerate(items):
        o, lout = int(desc[i]["out_off"]), it.L + 16 if initial is not None else it.L
        outs.append(out[o:o + lout])
        own[o:o + lout] = True
    got = np.frombuffer(out, dtype=np.uint8)
    was = np.frombuffer(initial, dtype=np.uint8) if initial is not None else np.uint8(FILL)
    wrong = np.flatnonzero((got != was) & ~own)
    assert wrong.size == 0, (what, "wrote outside the records' outputs", wrong[:8].tolist())
    return outs


def run_records(backend, what, oracle, keys, spec, rng, in_place, nfill=0, misalign=0, per_call=None):
    """noise_gpu_decrypt_records: nfill genuine 64-byte records, then the sweep of
    records spec(rng) -> (key index, ad, len).  per_call: the batch goes in
    calls of that many descriptors over the same images (each call judged on
    an image of its own)."""
    draw = lambda: rng.getrandbits(64) % noise_amd.NONCE_LIMIT
    specs = [(rng.randrange(len(keys)), draw(), b"", 64) for _ in range(nfill)]
    for _ in range(NREC):
        ki, ad, L = spec(rng)
        specs.append((ki, draw(), ad, L))
    items, pts = make_items(oracle, keys, specs, rng)
    wires = sweep_inputs(items, nfill)
    desc, inbuf, adbuf, out_size = records_layout(items, wires, nfill, in_place, misalign)
    outs, st = [], []
    for lo in range(0, len(items), per_call or len(items)):
        hi = min(len(items), lo + (per_call or len(items)))
        out, s = backend.records(keys, desc[lo:hi], inbuf, adbuf, out_size, in_place)
        outs += records_outputs(what, desc[lo:hi], items[lo:hi], out, inbuf if in_place else None)
        st += list(s)
    layout = "slots" if not misalign else "input off by %d" % misalign
    check(what, layout, items, nfill, pts, wires, outs, st, in_place)


# ---- the GPU backend ---------------------------------------------------------------
class GpuBackend:
    """The device entry points of the C ABI; torch tensors are the HBM buffers."""

    def __init__(self):
        import torch
        self.torch = torch

    def dev(self, b):
        a = np.frombuffer(bytes(b), dtype=np.uint8).copy()
        if a.size == 0:
            a = np.zeros(1, dtype=np.uint8)
        return self.torch.from_numpy(a).cuda()

    def host(self, t):
        self.torch.cuda.synchronize()
        return t.cpu().numpy().tobytes()

    def fill(self, n, value=FILL):
        return self.torch.full((max(n, 1),), value, dtype=self.torch.uint8, device="cuda")

    def uniform(self, key, n0, inbuf, in_off, in_stride, out_size, out_off, out_stride, L, ad, nrec, in_place):
        d_in = self.dev(inbuf)
        d_out = d_in if in_place else self.fill(out_size)
        d_st = self.fill(nrec, 9)
        noise_amd.decrypt_uniform(key, n0, d_in, in_stride, d_out, out_stride, L, d_st, nrec,
                                  d_ad=self.dev(ad) if ad else None, ad_stride=0, ad_len=len(ad),
                                  in_offset=in_off, out_offset=out_off)
        out = self.host(d_out)
        if not in_place:
            assert self.host(d_in) == inbuf, "the decrypt wrote to its input"
        return out[:out_size], self.host(d_st)[:nrec]

    def sessions(self, keys, idx, nonces, inbuf, in_stride, out_size, out_stride, L, nrec, in_place):
        d_keys = self.dev(b"".join(keys))
        d_idx = self.dev(np.array(idx, dtype=np.uint32).view(np.uint8))
        d_non = self.dev(np.array(nonces, dtype=np.uint64).view(np.uint8))
        d_in = self.dev(inbuf)
        d_out = d_in if in_place else self.fill(out_size)
        d_st = self.fill(nrec, 9)
        noise_amd.decrypt_sessions(d_keys, len(keys), d_idx, d_non, d_in, in_stride, d_out, out_stride, L, d_st, nrec)
        return self.host(d_out)[:out_size], self.host(d_st)[:nrec]

    def records(self, keys, desc, inbuf, adbuf, out_size, in_place):
        n = len(desc)
        d_keys, d_desc = self.dev(b"".join(keys)), self.dev(desc.view(np.uint8))
        d_in, d_ad = self.dev(inbuf), self.dev(adbuf)
        d_out = d_in if in_place else self.fill(out_size)
        d_st = self.fill(n, 9)
        noise_amd.decrypt_records(d_keys, len(keys), d_desc, n, d_in, d_out, d_st, d_ad)
        if not in_place:
            assert self.host(d_in) == inbuf, "the decrypt wrote to its input"
        return self.host(d_out)[:out_size], self.host(d_st)[:n]
