"""CPU: the stream-framing entry points of the CipherState tables
(noise_gpu_framed_open / noise_gpu_framed_seal) are declared, exported and
bound, their constants have the values of include/noise_gpu.h, and every
argument rule is refused with its own noise_gpu_last_error() text before any
device call: with no table behind the call and pointers that are never
dereferenced, on a machine without a GPU."""
import ctypes
import subprocess

import pytest

import noise_amd

E_ARG = noise_amd.E_ARG
BUF = 0x10000  # never dereferenced: every call below is refused first
NAMES = ["noise_gpu_framed_open", "noise_gpu_framed_seal"]
MAX = 65519


@pytest.fixture(scope="module")
def lib():
    return noise_amd.load()


def _err(lib):
    return lib.noise_gpu_last_error().decode()


def _span(base=BUF, off=None, stride=64, lens=None, len_all=64):
    return noise_amd.Span(base, off, stride, lens, len_all, 0)


def _ref(s):
    return ctypes.byref(s) if s else None


def _open(lib, cs=None, sess=BUF, wire="default", plain="default", recs=BUF, status=BUF, max_rec=9, first=BUF,
          nframes=BUF, first_bad=BUF, consumed=BUF, plain_len=BUF, conn_status=BUF, total=BUF, nconn=5):
    wire = _span() if wire == "default" else wire
    plain = _span() if plain == "default" else plain
    return lib.noise_gpu_framed_open(cs, sess, _ref(wire), _ref(plain), recs, status, max_rec, first, nframes,
                                     first_bad, consumed, plain_len, conn_status, total, 0, nconn, None)


def _seal(lib, cs=None, sess=BUF, msg="default", wire="default", max_payload=1024, recs=BUF, status=BUF,
          max_rec=9, first=BUF, nframes=BUF, msg_used=BUF, wire_len=BUF, conn_status=BUF, total=BUF, nconn=5):
    msg = _span() if msg == "default" else msg
    wire = _span() if wire == "default" else wire
    return lib.noise_gpu_framed_seal(cs, sess, _ref(msg), _ref(wire), max_payload, recs, status, max_rec, first,
                                     nframes, msg_used, wire_len, conn_status, total, 0, nconn, None)


def test_constants_and_symbols(lib):
    assert noise_amd.REC_EMPTY == 6
    assert (noise_amd.FRAMED_OK, noise_amd.FRAMED_BAD_LEN, noise_amd.FRAMED_FULL,
            noise_amd.FRAMED_REFUSED) == (0, 1, 2, 3)
    assert noise_amd.FRAMED_MAX_PAYLOAD == MAX
    header = " ".join(open(noise_amd.HEADER).read().split())
    for line in ("#define NOISE_GPU_REC_EMPTY 6u", "#define NOISE_GPU_FRAMED_OK 0u",
                 "#define NOISE_GPU_FRAMED_BAD_LEN 1u", "#define NOISE_GPU_FRAMED_FULL 2u",
                 "#define NOISE_GPU_FRAMED_REFUSED 3u"):
        assert line in header, line
    declared = [n for n in noise_amd.declared_symbols() if n.startswith("noise_gpu_framed_")]
    assert sorted(declared) == sorted(NAMES)
    nm = subprocess.run(["nm", "-D", "--defined-only", noise_amd.LIB_PATH], capture_output=True,
                        text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if " T " in line}
    for n in NAMES:
        assert n in exported, n
        assert getattr(lib, n).argtypes is not None and len(getattr(lib, n).argtypes) == 17, n
    for m in ("seal_framed", "open_framed"):
        assert callable(getattr(noise_amd.CipherStateTable, m)), m


def test_null_table(lib):
    """Everything else in order and no table: that is what the text says."""
    for call in (_open, _seal):
        assert call(lib) == E_ARG and "null table" in _err(lib)
        assert call(lib, nconn=0) == E_ARG and "null table" in _err(lib)  # an empty batch on no table
        assert call(lib, nconn=0, max_rec=0) == E_ARG and "null table" in _err(lib)


def test_batch_sizes(lib):
    for call in (_open, _seal):
        assert call(lib, nconn=(1 << 31) + 1) == E_ARG and "2^31 connections" in _err(lib)
        assert call(lib, max_rec=(1 << 31) + 1) == E_ARG and "2^31 record slots" in _err(lib)
        assert call(lib, nconn=1 << 31, max_rec=1 << 31) == E_ARG and "null table" in _err(lib)  # 2^31 passes
        assert call(lib, max_rec=0) == E_ARG and "max_rec is 0" in _err(lib)
        assert call(lib, max_rec=1) == E_ARG and "null table" in _err(lib)


def test_max_payload(lib):
    for bad in (0, MAX + 1, 65535, 0xffffffff):
        assert _seal(lib, max_payload=bad) == E_ARG and "max_payload outside 1 .. 65519" in _err(lib), bad
        assert _seal(lib, max_payload=bad, nconn=0) == E_ARG and "max_payload" in _err(lib), bad
    for good in (1, 64, MAX):
        assert _seal(lib, max_payload=good) == E_ARG and "null table" in _err(lib), good


def test_null_spans_bases_and_arrays(lib):
    assert _open(lib, wire=None) == E_ARG and "null span" in _err(lib)
    assert _open(lib, wire=_span(base=None)) == E_ARG and "null span" in _err(lib)
    assert _open(lib, plain=_span(base=None)) == E_ARG and "null span" in _err(lib)
    assert _open(lib, plain=None) == E_ARG and "null table" in _err(lib)  # in place
    for which in ("msg", "wire"):
        assert _seal(lib, **{which: None}) == E_ARG and "null span" in _err(lib)
        assert _seal(lib, **{which: _span(base=None)}) == E_ARG and "null span" in _err(lib)
    for call in (_open, _seal):
        assert call(lib, recs=None) == E_ARG and "null descriptors / status" in _err(lib)
        assert call(lib, status=None) == E_ARG and "null descriptors / status" in _err(lib)
        assert call(lib, sess=None) == E_ARG and "null session array" in _err(lib)
        for req in ("nframes", "conn_status"):
            assert call(lib, **{req: None}) == E_ARG and "null per-connection output array" in _err(lib), req
        # the optional arrays may be null: the refusal is the missing table's
        assert call(lib, first=None, total=None) == E_ARG and "null table" in _err(lib)
    assert _open(lib, consumed=None) == E_ARG and "null per-connection output array" in _err(lib)
    assert _open(lib, first_bad=None, plain_len=None) == E_ARG and "null table" in _err(lib)
    for req in ("msg_used", "wire_len"):
        assert _seal(lib, **{req: None}) == E_ARG and "null per-connection output array" in _err(lib), req


def test_alignment(lib):
    assert _open(lib, wire=_span(off=BUF + 4)) == E_ARG and "offsets must be 8-byte aligned" in _err(lib)
    assert _open(lib, plain=_span(off=BUF + 4)) == E_ARG and "offsets must be 8-byte aligned" in _err(lib)
    assert _seal(lib, msg=_span(off=BUF + 4)) == E_ARG and "offsets must be 8-byte aligned" in _err(lib)
    assert _seal(lib, wire=_span(off=BUF + 4)) == E_ARG and "offsets must be 8-byte aligned" in _err(lib)
    # the lengths that are read: open's wire, seal's msg
    assert _open(lib, wire=_span(lens=BUF + 2)) == E_ARG and "lengths must be 4-byte aligned" in _err(lib)
    assert _seal(lib, msg=_span(lens=BUF + 2)) == E_ARG and "lengths must be 4-byte aligned" in _err(lib)
    # a slot span's lengths are not read; len_all applies to a wire without lengths, whatever it is
    assert _open(lib, plain=_span(lens=BUF + 1, len_all=0)) == E_ARG and "null table" in _err(lib)
    assert _seal(lib, wire=_span(lens=BUF + 1, len_all=0)) == E_ARG and "null table" in _err(lib)
    for n in (0, 1, 0xffffffff):
        assert _open(lib, wire=_span(len_all=n)) == E_ARG and "null table" in _err(lib)
        assert _seal(lib, msg=_span(len_all=n)) == E_ARG and "null table" in _err(lib)
    for call in (_open, _seal):
        assert call(lib, recs=BUF + 4) == E_ARG and "descriptors must be 8-byte aligned" in _err(lib)
        assert call(lib, recs=BUF + 8) == E_ARG and "null table" in _err(lib)  # 8 is enough
        for kw in ({"sess": BUF + 2}, {"nframes": BUF + 2}):
            assert call(lib, **kw) == E_ARG and "must be 4-byte aligned" in _err(lib), kw
        for kw in ({"first": BUF + 4}, {"total": BUF + 4}):
            assert call(lib, **kw) == E_ARG and "must be 8-byte aligned" in _err(lib), kw
        assert call(lib, conn_status=BUF + 1, status=BUF + 3) == E_ARG and "null table" in _err(lib)  # bytes
    assert _open(lib, first_bad=BUF + 1) == E_ARG and "must be 4-byte aligned" in _err(lib)
    for kw in ({"consumed": BUF + 4}, {"plain_len": BUF + 4}):
        assert _open(lib, **kw) == E_ARG and "must be 8-byte aligned" in _err(lib), kw
    for kw in ({"msg_used": BUF + 4}, {"wire_len": BUF + 4}):
        assert _seal(lib, **kw) == E_ARG and "must be 8-byte aligned" in _err(lib), kw
