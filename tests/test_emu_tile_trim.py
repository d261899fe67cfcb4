"""CPU-side checks of the exact tile kernel's trimmed arithmetic
(tile_kernel.hpp), the twin of tests/test_gpu_tile_trim.py:

* tools/emu/emu_uniform `tile`: the unmodified kernel and its host launcher
  compiled as host C++ (tools/emu) under AddressSanitizer, uniform batches at
  L = 512, 1024 (one recombination product per lane), 2048 and 16384 (the
  log-tree), 1..130 records, packed, padded and in place, nonce ranges that
  cross 2^32 (the host's split into two launches) or end at 2^64 - 1,
  all-0xFF / all-0x00 records, every fifth record tampered -- against the
  oracle, with every store watched: none outside a record's output, none of
  unverified plaintext.
* tools/emu/emu_poly_recombine: the Poly1305 recombination without the carries
  before from26, with the device functions alone under ASan + UBSan: r with
  every clamped bit set over all-ones blocks, and 10,000 random (r, message)
  pairs, against a straight Horner chain; no limb reaches 2^31.
  What it does not prove: the chain it compares with is the kernel's own
  poly_block / poly_final, so an error in those two cancels, and under random
  (r, message) the accumulator never lies in p <= h < 2^130 on entry to
  poly_final nor is a lane sum ever held as p + T.  tests/test_poly_edges.py
  (tools/emu/emu_poly_edges) feeds chosen residues and compares with tags
  computed in Python.
Test infrastructure only: the product runs these kernels on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tools", "emu")
BUILD = os.path.join(EMU, "build")
JOBS = "-j%d" % max(1, min(8, os.cpu_count() or 1))


def _make(*args):
    r = subprocess.run(["make", JOBS, "-C", EMU, *args], capture_output=True, text=True, timeout=1200)
    if r.returncode != 0:
        pytest.fail("emulation build failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])


def _run(name, *args):
    return subprocess.run([os.path.join(BUILD, name), *args], capture_output=True, text=True, timeout=900,
                          env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))


def test_exact_tile_kernel_emulated():
    _make("GRID_CAP=3u", "uniform")
    r = _run("emu_uniform", "tile")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert "uniform tile: 0 stores outside, 0 stores of unverified plaintext" in r.stdout
    assert "ok (0 failures)" in r.stdout


def test_poly_recombination_without_carries():
    _make("poly")
    r = _run("emu_poly_recombine")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert "ok (0 failures)" in r.stdout
