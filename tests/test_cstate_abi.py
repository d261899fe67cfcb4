"""CPU: the CipherState-table entry points (noise_gpu_cs_*) validate their
arguments before any device call, and without a gfx950 device create fails
with E_NODEV (no CPU fallback).  Each refusal is told apart from the others by
the text noise_gpu_last_error() keeps: a NULL handle would otherwise hide
whether the range / stride check ran at all."""
import ctypes

import pytest

import noise_amd

E_ARG, E_NODEV, OK = noise_amd.E_ARG, noise_amd.E_NODEV, noise_amd.OK
BUF = ctypes.c_void_p(0x10000)  # never dereferenced: every call below is refused first


@pytest.fixture(scope="module")
def lib():
    return noise_amd.load()


def _err(lib):
    return lib.noise_gpu_last_error().decode()


def _have_device(lib):
    n = ctypes.c_int(0)
    lib.noise_gpu_device_count(ctypes.byref(n))
    return n.value > 0


def test_constants_and_symbols(lib):
    assert noise_amd.REC_NONCE == 3
    header = open(noise_amd.HEADER).read()
    assert "#define NOISE_GPU_REC_NONCE 3u" in header
    names = [n for n in noise_amd.declared_symbols() if n.startswith("noise_gpu_cs_")]
    assert sorted(names) == sorted("noise_gpu_cs_" + s for s in (
        "create", "destroy", "set", "get", "rekey", "assign", "encrypt_records", "decrypt_records",
        "encrypt_sessions", "decrypt_sessions"))
    for n in names:
        assert getattr(lib, n).argtypes is not None, n  # the binding declares a signature


def test_create_and_destroy(lib):
    h = ctypes.c_void_p(1)
    assert lib.noise_gpu_cs_create(0, ctypes.byref(h)) == E_ARG and h.value is None
    assert lib.noise_gpu_cs_create((1 << 32) - 1, ctypes.byref(h)) == E_ARG
    assert lib.noise_gpu_cs_create(1 << 40, ctypes.byref(h)) == E_ARG
    assert lib.noise_gpu_cs_create(4, None) == E_ARG
    assert lib.noise_gpu_cs_destroy(None) == OK
    if not _have_device(lib):
        assert lib.noise_gpu_cs_create(4, ctypes.byref(h)) == E_NODEV and h.value is None
        assert lib.noise_gpu_cs_create((1 << 32) - 2, ctypes.byref(h)) == E_NODEV


def test_null_handle(lib):
    assert lib.noise_gpu_cs_set(None, 0, 1, BUF, 32, None, None) == E_ARG and "null table" in _err(lib)
    assert lib.noise_gpu_cs_get(None, 0, 1, BUF, None, None) == E_ARG and "null table" in _err(lib)
    assert lib.noise_gpu_cs_rekey(None, None, 0, None) == E_ARG and "null table" in _err(lib)
    assert lib.noise_gpu_cs_assign(None, BUF, 4, BUF, 8, None, 5, None) == E_ARG
    assert "null table" in _err(lib)
    for fn in (lib.noise_gpu_cs_encrypt_records, lib.noise_gpu_cs_decrypt_records):
        assert fn(None, BUF, 5, BUF, BUF, None, BUF, 0, None) == E_ARG and "null table" in _err(lib)
    for fn in (lib.noise_gpu_cs_encrypt_sessions, lib.noise_gpu_cs_decrypt_sessions):
        assert fn(None, BUF, BUF, 64, BUF, 80, 64, BUF, 5, None) == E_ARG and "null table" in _err(lib)
    # an empty batch on no table is still a bad call
    assert lib.noise_gpu_cs_assign(None, BUF, 4, BUF, 8, None, 0, None) == E_ARG


def test_range_and_stride_checks(lib):
    top = (1 << 64) - 1
    assert lib.noise_gpu_cs_set(None, top, 2, BUF, 32, None, None) == E_ARG and "overflows" in _err(lib)
    assert lib.noise_gpu_cs_get(None, 5, top - 3, BUF, None, None) == E_ARG and "overflows" in _err(lib)
    assert lib.noise_gpu_cs_set(None, 0, 1, BUF, 16, None, None) == E_ARG and "key_stride" in _err(lib)
    assert lib.noise_gpu_cs_assign(None, BUF, 4, BUF, 0, None, 5, None) == E_ARG
    assert "nonce stride" in _err(lib)
    assert lib.noise_gpu_cs_assign(None, BUF, 4, BUF, 12, None, 5, None) == E_ARG
    assert "nonce stride" in _err(lib)
    assert lib.noise_gpu_cs_assign(None, BUF, 0, BUF, 8, None, 5, None) == E_ARG
    assert "session stride" in _err(lib)
    assert lib.noise_gpu_cs_assign(None, BUF, 4, BUF, 8, None, (1 << 31) + 1, None) == E_ARG
    assert "2^31" in _err(lib)


@pytest.mark.gpu
def test_checks_on_a_live_table(lib):
    """The same checks with a table behind them, and nrec 0 -> OK."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    t = noise_amd.CipherStateTable(10)
    E = noise_amd.NoiseGpuError
    keys = torch.zeros(32 * 16, dtype=torch.uint8, device="cuda")
    n = torch.zeros(16, dtype=torch.int64, device="cuda")
    sess = torch.zeros(16, dtype=torch.int32, device="cuda")
    for first, count in ((0, 11), (10, 1), (5, (1 << 64) - 3)):
        with pytest.raises(E):
            t.set(first, count, keys)
        with pytest.raises(E):
            t.get(first, count, d_keys=keys)
    t.set(10, 0, keys)  # empty range at the end
    with pytest.raises(E):
        t.assign(sess, n, 5, nonce_stride=0)
    with pytest.raises(E):
        t.encrypt_sessions(sess, keys, 65, keys, 80, 65, 2)  # no such sessions shape
    with pytest.raises(E):
        t.decrypt_sessions(sess, keys, 80, keys, 64, 64, None, 2)  # status required
    t.assign(sess, n, 0)
    t.encrypt_records(None, 0, None, None)
    t.decrypt_sessions(None, None, 0, None, 0, 64, None, 0)
    torch.cuda.synchronize()
    t.close()
    t.close()
