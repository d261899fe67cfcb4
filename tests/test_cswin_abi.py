"""CPU: the windowed entry points of the CipherState tables (noise_gpu_cswin_*)
are declared, exported and bound, validate their arguments before any device
call, and without a gfx950 device fail with E_NODEV (no CPU fallback).  Each
refusal is told apart by the text noise_gpu_last_error() keeps.  Also the host
rule itself: noise::ReplayWindow against a brute-force model
(tests/cpp/replay_window_test.cpp)."""
import ctypes
import os
import subprocess

import pytest

import noise_amd

E_ARG, E_NODEV, OK = noise_amd.E_ARG, noise_amd.E_NODEV, noise_amd.OK
BUF = ctypes.c_void_p(0x10000)  # never dereferenced: every call below is refused first
ODD = ctypes.c_void_p(0x10002)
NAMES = ["noise_gpu_cswin_" + s for s in ("reset", "get", "filter", "commit", "decrypt_records",
                                          "decrypt_sessions")]


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
    assert noise_amd.REC_REPLAY == 4 and noise_amd.CS_WINDOW == 1024
    header = open(noise_amd.HEADER).read()
    assert "#define NOISE_GPU_REC_REPLAY 4u" in header and "#define NOISE_GPU_CS_WINDOW 1024u" in header
    declared = [n for n in noise_amd.declared_symbols() if n.startswith("noise_gpu_cswin_")]
    assert sorted(declared) == sorted(NAMES)
    nm = subprocess.run(["nm", "-D", "--defined-only", noise_amd.LIB_PATH], capture_output=True,
                        text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if " T " in line}
    for n in NAMES:
        assert n in exported, n
        assert getattr(lib, n).argtypes is not None, n  # the binding declares a signature
    for m in ("window_reset", "window_get", "window_filter", "window_commit", "decrypt_records_window",
              "decrypt_sessions_window"):
        assert callable(getattr(noise_amd.CipherStateTable, m)), m


def test_null_handle(lib):
    assert lib.noise_gpu_cswin_reset(None, 0, 1, None) == E_ARG and "null table" in _err(lib)
    assert lib.noise_gpu_cswin_get(None, 0, 1, BUF, BUF, None) == E_ARG and "null table" in _err(lib)
    for fn in (lib.noise_gpu_cswin_filter, lib.noise_gpu_cswin_commit):
        assert fn(None, BUF, 4, BUF, 8, BUF, 5, None) == E_ARG and "null table" in _err(lib)
        assert fn(None, BUF, 4, BUF, 8, BUF, 0, None) == E_ARG  # an empty batch on no table
    assert lib.noise_gpu_cswin_decrypt_records(None, BUF, 5, BUF, BUF, None, BUF, 0, None) == E_ARG
    assert "null table" in _err(lib)
    assert lib.noise_gpu_cswin_decrypt_sessions(None, BUF, BUF, BUF, 80, BUF, 80, 64, BUF, 5, None) == E_ARG
    assert "null table" in _err(lib)


def test_range_stride_and_size_checks(lib):
    top = (1 << 64) - 1
    assert lib.noise_gpu_cswin_reset(None, top, 2, None) == E_ARG and "overflows" in _err(lib)
    assert lib.noise_gpu_cswin_get(None, 5, top - 3, BUF, BUF, None) == E_ARG and "overflows" in _err(lib)
    assert lib.noise_gpu_cswin_get(None, 0, 1, ODD, BUF, None) == E_ARG and "8-byte aligned" in _err(lib)
    for fn in (lib.noise_gpu_cswin_filter, lib.noise_gpu_cswin_commit):
        assert fn(None, BUF, 4, BUF, 0, BUF, 5, None) == E_ARG and "nonce stride" in _err(lib)
        assert fn(None, BUF, 4, BUF, 12, BUF, 5, None) == E_ARG and "nonce stride" in _err(lib)
        assert fn(None, BUF, 0, BUF, 8, BUF, 5, None) == E_ARG and "session stride" in _err(lib)
        assert fn(None, BUF, 6, BUF, 8, BUF, 5, None) == E_ARG and "session stride" in _err(lib)
        assert fn(None, BUF, 4, BUF, 8, BUF, (1 << 31) + 1, None) == E_ARG and "2^31" in _err(lib)
    assert lib.noise_gpu_cswin_decrypt_records(None, BUF, (1 << 31) + 1, BUF, BUF, None, BUF, 0,
                                               None) == E_ARG and "2^31" in _err(lib)
    assert lib.noise_gpu_cswin_decrypt_sessions(None, BUF, BUF, BUF, 80, BUF, 80, 64, BUF, (1 << 31) + 1,
                                                None) == E_ARG and "2^31" in _err(lib)


def test_no_device_no_table(lib):
    """Without a device there is no table to call these on: create is what fails."""
    if not _have_device(lib):
        h = ctypes.c_void_p(1)
        assert lib.noise_gpu_cs_create(4, ctypes.byref(h)) == E_NODEV and h.value is None


def test_replay_window_against_brute_force(tmp_path):
    """noise::ReplayWindow (host/noise_amd/replay_window.hpp, plain C++) against
    a set of accepted nonces plus their maximum: the window's edges (1024 behind
    next accepted if unseen, 1025 too old), jumps of exactly 1023 / 1024 / 1025,
    nonces around 2^32 and up to 2^64-3 (tests/cpp/replay_window_test.cpp)."""
    exe = str(tmp_path / "replay_window_test")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I",
                    os.path.join(noise_amd.ROOT, "noise-cpp_amd", "host"),
                    os.path.join(noise_amd.ROOT, "tests", "cpp", "replay_window_test.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " 0 wrong" in r.stdout and "never exercised" not in r.stdout


@pytest.mark.gpu
def test_checks_on_a_live_table(lib):
    """The same checks with a table behind them, and nrec 0 -> OK."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    t = noise_amd.CipherStateTable(10)
    E = noise_amd.NoiseGpuError
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    n = torch.zeros(16, dtype=torch.int64, device="cuda")
    sess = torch.zeros(16, dtype=torch.int32, device="cuda")
    st = torch.zeros(16, dtype=torch.uint8, device="cuda")
    for first, count in ((0, 11), (10, 1), (5, (1 << 64) - 3)):
        with pytest.raises(E):
            t.window_reset(first, count)
        with pytest.raises(E):
            t.window_get(first, count, d_next=n)
    t.window_reset(10, 0)  # empty range at the end
    with pytest.raises(E):
        t.window_filter(sess, n, st, 5, nonce_stride=0)
    with pytest.raises(E):
        t.window_filter(sess, n, None, 5)  # status required
    with pytest.raises(E):
        t.window_commit(sess, n, None, 5)
    with pytest.raises(E):
        t.decrypt_sessions_window(sess, n, buf, 81, buf[2048:], 65, 65, st, 2)  # no such sessions shape
    with pytest.raises(E):
        t.decrypt_sessions_window(sess, n, buf, 80, buf[2048:], 64, 64, None, 2)  # status required
    with pytest.raises(E):
        t.decrypt_sessions_window(sess, None, buf, 80, buf[2048:], 64, 64, st, 2)  # nonces required
    with pytest.raises(E):
        t.decrypt_records_window(buf, 2, buf, buf, None)
    t.window_filter(sess, n, st, 0)
    t.window_commit(sess, n, st, 0)
    t.decrypt_records_window(None, 0, None, None, None)
    t.decrypt_sessions_window(None, None, None, 0, None, 0, 64, None, 0)
    torch.cuda.synchronize()
    t.close()
    t.close()
