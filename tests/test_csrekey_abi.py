"""CPU: the in-band rekey schedule of the CipherState tables
(noise_gpu_csrekey_set / noise_gpu_csrekey_get) is declared, exported and
bound, the noise_gpu_csrekey_* set is exactly these two, and a null table or a
null output is refused with its own noise_gpu_last_error() text -- with no
table behind the call, on a machine without a GPU."""
import ctypes
import subprocess

import pytest

import noise_amd

E_ARG = noise_amd.E_ARG
NAMES = ["noise_gpu_csrekey_get", "noise_gpu_csrekey_set"]


@pytest.fixture(scope="module")
def lib():
    return noise_amd.load()


def _err(lib):
    return lib.noise_gpu_last_error().decode()


def test_declared_and_bound(lib):
    declared = [n for n in noise_amd.declared_symbols() if n.startswith("noise_gpu_csrekey_")]
    assert declared == NAMES
    for n in NAMES:
        assert getattr(lib, n).argtypes is not None and getattr(lib, n).restype is ctypes.c_int, n
    assert lib.noise_gpu_csrekey_set.argtypes == [ctypes.c_void_p, ctypes.c_uint64]
    assert lib.noise_gpu_csrekey_get.argtypes == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    header = " ".join(open(noise_amd.HEADER).read().split())
    assert "int noise_gpu_csrekey_set(noise_gpu_cs *cs, uint64_t every);" in header
    assert "int noise_gpu_csrekey_get(const noise_gpu_cs *cs, uint64_t *every);" in header


def test_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", noise_amd.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = sorted(line.split()[-1] for line in out.splitlines() if "noise_gpu_csrekey_" in line)
    assert exported == NAMES


def test_null_table_and_null_output(lib):
    every = ctypes.c_uint64(77)
    assert lib.noise_gpu_csrekey_set(None, 16) == E_ARG and "null table" in _err(lib)
    assert lib.noise_gpu_csrekey_set(None, 0) == E_ARG and "null table" in _err(lib)
    assert lib.noise_gpu_csrekey_get(None, ctypes.byref(every)) == E_ARG and "null table" in _err(lib)
    assert every.value == 77  # untouched
    assert lib.noise_gpu_csrekey_get(None, None) == E_ARG and "null output" in _err(lib)
    fake = ctypes.c_void_p(0x10000)  # never dereferenced: the output is checked first
    assert lib.noise_gpu_csrekey_get(fake, None) == E_ARG and "null output" in _err(lib)


@pytest.mark.gpu
def test_set_and_get_on_a_live_table(lib):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    t = noise_amd.CipherStateTable(4)
    assert t.rekey_every() == 0  # off after create
    for every in (1, 16, 1 << 32, (1 << 64) - 1, 0):
        t.set_rekey_every(every)
        assert t.rekey_every() == every
    assert lib.noise_gpu_csrekey_get(t.h, None) == E_ARG and "null output" in _err(lib)
    t.close()
