"""CPU-side check of the replay-window kernels: the unmodified
csrc/cswin_kernels.hip and the sort it shares with nonce assignment
(csrc/cstate_kernels.hip) compiled as host C++ against the HIP stand-in in
tools/emu and run as a stand-alone program (tools/emu/emu_cswin.cpp) under
AddressSanitizer.  Every batch goes through cs_window_call
(csrc/cstate_calls.hpp), the composition the C ABI runs: scratch carve, private
copy, prefilter, commit, finish.  The build caps the grid at 3 workgroups and
cuts the sort into 640-record chunks; tables, window rows, batches and outputs
are allocated at their exact sizes and the scratch at cs_scratch_layout's
total, so an index past any of them or past a scratch region is an ASan report.
Every case runs two batches in sequence on windows that have seen traffic
(bases at 0, across 2^32, and running into the 2^64-2 limit) and is checked
inside the program against the plain loop of include/noise_gpu.h over
noise::ReplayWindow: pre-statuses and refused marks of the prefilter (which
must not write to the table), final statuses, next and bitmap rows, and every
output byte (accepted: kept; post-authentication replay: zeroed; everything
else and every gap: untouched).  A case fails if the model never produced a
status it is about.  Only the AEAD launch between prefilter and commit is a
stand-in there; it is also where the prefilter's results are checked.  Test
infrastructure only: the product runs these kernels on the GPU
(tests/test_gpu_cswin.py)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tools", "emu")
BIN = os.path.join(EMU, "build", "emu_cswin")


@pytest.fixture(scope="module")
def run():
    r = subprocess.run(["make", "-j4", "-C", EMU, "GRID_CAP=3u", "cswin"], capture_output=True,
                       text=True, timeout=900)
    if r.returncode != 0:
        pytest.fail("emulation build failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    return subprocess.run([BIN], capture_output=True, text=True, timeout=900, env=env)


def test_emulated_window_kernels_match_the_loop(run):
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "emu_cswin: all ok" in run.stdout and "FAIL" not in run.stdout
    assert "AddressSanitizer" not in run.stderr


@pytest.mark.parametrize("case", [
    "mixed-1:", "mixed-63:", "mixed-64:", "mixed-65:", "mixed-129:", "mixed-1500:",
    "own-session-1500:", "one-session-1500:", "one-session-5000: 5000 records", "nsess-1:", "nsess-257:",
    "nsess-65537:", "aliases-14:", "aliases-114:", "forged-ahead-40:", "forged-ahead-700:"])
def test_case_ran(run, case):
    # each case prints one line per batch: arrays first, descriptors second
    assert run.stdout.count("ok " + case) == 2, run.stdout[-3000:]
