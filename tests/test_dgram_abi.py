"""CPU: the datagram entry points of the CipherState tables (noise_gpu_dgram_seal
/ noise_gpu_dgram_open) are declared, exported and bound, their constants have
the values of include/noise_gpu.h, and every argument rule is refused with its
own noise_gpu_last_error() text before any device call: with no table behind
the call and pointers that are never dereferenced, on a machine without a GPU."""
import ctypes
import subprocess

import pytest

import noise_amd

E_ARG = noise_amd.E_ARG
BUF = 0x10000  # never dereferenced: every call below is refused first
NAMES = ["noise_gpu_dgram_seal", "noise_gpu_dgram_open"]
MAX = 65519


@pytest.fixture(scope="module")
def lib():
    return noise_amd.load()


def _err(lib):
    return lib.noise_gpu_last_error().decode()


def _span(base=BUF, off=None, stride=64, lens=None, len_all=64):
    return noise_amd.Span(base, off, stride, lens, len_all, 0)


def _seal(lib, cs=None, sess=BUF, peer=None, payload="default", pkt="default", recs=BUF, pkt_len=BUF,
          status=BUF, nrec=5):
    payload = _span() if payload == "default" else payload
    pkt = _span() if pkt == "default" else pkt
    return lib.noise_gpu_dgram_seal(cs, 4, sess, peer, ctypes.byref(payload) if payload else None,
                                    ctypes.byref(pkt) if pkt else None, recs, pkt_len, status, 0, nrec, None)


def _open(lib, cs=None, pkt="default", payload="default", recs=BUF, payload_len=BUF, status=BUF, nrec=5):
    payload = _span() if payload == "default" else payload
    pkt = _span() if pkt == "default" else pkt
    return lib.noise_gpu_dgram_open(cs, 4, ctypes.byref(pkt) if pkt else None,
                                    ctypes.byref(payload) if payload else None, recs, payload_len, status, 0,
                                    nrec, None)


def test_constants_and_symbols(lib):
    assert noise_amd.REC_MALFORMED == 5 and noise_amd.DGRAM_HDR == 16 and noise_amd.DGRAM_MAX_LEN == MAX
    header = open(noise_amd.HEADER).read()
    for line in ("#define NOISE_GPU_DGRAM_HDR 16u", "#define NOISE_GPU_DGRAM_MAX_LEN 65519u",
                 "#define NOISE_GPU_REC_MALFORMED 5u"):
        assert line in header, line
    declared = [n for n in noise_amd.declared_symbols() if n.startswith("noise_gpu_dgram_")]
    assert sorted(declared) == sorted(NAMES)
    nm = subprocess.run(["nm", "-D", "--defined-only", noise_amd.LIB_PATH], capture_output=True,
                        text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if " T " in line}
    for n in NAMES:
        assert n in exported, n
        assert getattr(lib, n).argtypes is not None, n  # the binding declares a signature
    for m in ("seal_datagrams", "open_datagrams"):
        assert callable(getattr(noise_amd.CipherStateTable, m)), m


def test_null_table(lib):
    """Everything else in order and no table: that is what the text says."""
    assert _seal(lib) == E_ARG and "null table" in _err(lib)
    assert _open(lib) == E_ARG and "null table" in _err(lib)
    assert _seal(lib, nrec=0) == E_ARG and "null table" in _err(lib)  # an empty batch on no table
    assert _open(lib, nrec=0) == E_ARG and "null table" in _err(lib)


def test_batch_size(lib):
    assert _seal(lib, nrec=(1 << 31) + 1) == E_ARG and "2^31" in _err(lib)
    assert _open(lib, nrec=(1 << 31) + 1) == E_ARG and "2^31" in _err(lib)
    assert _seal(lib, nrec=1 << 31) == E_ARG and "null table" in _err(lib)  # 2^31 itself passes that rule
    assert _open(lib, nrec=1 << 31) == E_ARG and "null table" in _err(lib)


def test_null_spans_bases_and_outputs(lib):
    for call in (_seal, _open):
        assert call(lib, payload=None) == E_ARG and "null span" in _err(lib)
        assert call(lib, pkt=None) == E_ARG and "null span" in _err(lib)
        assert call(lib, payload=_span(base=None)) == E_ARG and "null span" in _err(lib)
        assert call(lib, pkt=_span(base=None)) == E_ARG and "null span" in _err(lib)
        assert call(lib, recs=None) == E_ARG and "null descriptors / status" in _err(lib)
        assert call(lib, status=None) == E_ARG and "null descriptors / status" in _err(lib)
    assert _seal(lib, sess=None) == E_ARG and "null session array" in _err(lib)
    # the optional arrays may be null: the refusal is the missing table's
    assert _seal(lib, peer=None, pkt_len=None) == E_ARG and "null table" in _err(lib)
    assert _open(lib, payload_len=None) == E_ARG and "null table" in _err(lib)


def test_alignment(lib):
    for call in (_seal, _open):
        for which in ("payload", "pkt"):
            assert call(lib, **{which: _span(off=BUF + 4)}) == E_ARG and "offsets must be 8-byte aligned" in _err(lib)
        assert call(lib, recs=BUF + 4) == E_ARG and "descriptors must be 8-byte aligned" in _err(lib)
        assert call(lib, recs=BUF + 8) == E_ARG and "null table" in _err(lib)  # 8 is enough
    # the lengths that are read: seal's payload, open's packets
    assert _seal(lib, payload=_span(lens=BUF + 2)) == E_ARG and "lengths must be 4-byte aligned" in _err(lib)
    assert _open(lib, pkt=_span(lens=BUF + 2)) == E_ARG and "lengths must be 4-byte aligned" in _err(lib)
    for kw in ({"sess": BUF + 2}, {"peer": BUF + 1}, {"pkt_len": BUF + 2}):
        assert _seal(lib, **kw) == E_ARG and "must be 4-byte aligned" in _err(lib), kw
    assert _open(lib, payload_len=BUF + 3) == E_ARG and "must be 4-byte aligned" in _err(lib)


def test_uniform_lengths(lib):
    assert _seal(lib, payload=_span(len_all=MAX + 1)) == E_ARG and "NOISE_GPU_DGRAM_MAX_LEN" in _err(lib)
    assert _seal(lib, payload=_span(len_all=MAX)) == E_ARG and "null table" in _err(lib)
    assert _seal(lib, payload=_span(len_all=0)) == E_ARG and "null table" in _err(lib)
    # with per-record lengths len_all means nothing
    assert _seal(lib, payload=_span(lens=BUF, len_all=MAX + 1)) == E_ARG and "null table" in _err(lib)
    for bad in (0, 31, 32 + MAX + 1, 0xffffffff):
        assert _open(lib, pkt=_span(len_all=bad)) == E_ARG and "packet length outside" in _err(lib), bad
    for good in (32, 33, 32 + MAX):
        assert _open(lib, pkt=_span(len_all=good)) == E_ARG and "null table" in _err(lib), good
    assert _open(lib, pkt=_span(lens=BUF, len_all=5)) == E_ARG and "null table" in _err(lib)
    # a slot span's lengths are not read: nothing about them is checked
    assert _open(lib, payload=_span(lens=BUF + 1, len_all=0)) == E_ARG and "null table" in _err(lib)
    assert _seal(lib, pkt=_span(lens=BUF + 1, len_all=0)) == E_ARG and "null table" in _err(lib)
