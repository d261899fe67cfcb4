"""CPU-side check of the CipherState-table kernels' indexing and of the
in-order call around them: the unmodified csrc/cstate_kernels.hip and
csrc/cstate_calls.hpp compiled as host C++ against the HIP stand-in in
tools/emu and run as a stand-alone program (tools/emu/emu_cstate.cpp) under
AddressSanitizer.  Every batch goes through cs_inorder_call, the composition
the C ABI runs (scratch carve, private copy, assignment, k_cs_fix); only the
AEAD launch inside it is a stand-in.  The build caps the grid at 3 workgroups
and cuts the sort into 640-record chunks (a full batch of 8 steps and a
partial one), so at 5000 records every workgroup loops over several chunks;
tables and batches are allocated at their exact sizes and the scratch at
cs_scratch_layout's total, so an index past any of them, or a scratch region
that overlaps the next, is an ASan report or a failed check.  Cases: 1 .. 1500
records shuffled over 40 sessions with bad indices, all in one session, each
in its own; 1 / 257 / 65537 sessions (1, 2, 3 radix passes) with indices that
share low bytes and differ in high ones and the reverse; 5000 records over
70000 sessions; the nonce limit (2^64-5 and 2^64-1) on both paths; the decrypt
direction (refused records read NONCE again after the stand-in's BAD_KEY, the
caller's columns stay as they were); the scratch layout against the four
layouts the calls used to write out; set and rekey.  Every result is checked
inside the program against a plain loop (a map of counters) and the oracle's
rekey.  Test infrastructure only: the product runs these kernels on the GPU
(tests/test_gpu_cstate.py)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tools", "emu")
BIN = os.path.join(EMU, "build", "emu_cstate")


@pytest.fixture(scope="module")
def run():
    r = subprocess.run(["make", "-j4", "-C", EMU, "GRID_CAP=3u", "cstate"], capture_output=True,
                       text=True, timeout=900)
    if r.returncode != 0:
        pytest.fail("emulation build failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    return subprocess.run([BIN], capture_output=True, text=True, timeout=900, env=env)


def test_emulated_cstate_kernels_match_the_loop(run):
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "emu_cstate: all ok" in run.stdout and "FAIL" not in run.stdout
    assert "AddressSanitizer" not in run.stderr


@pytest.mark.parametrize("case", [
    "mixed-1:", "mixed-63:", "mixed-64:", "mixed-65:", "mixed-129:", "mixed-1500:",
    "one-session-1500:", "own-session-1500:", "nsess-1:", "nsess-257:", "nsess-65537:",
    "nsess-70000: 5000 records", "limit-small:", "limit-sorted:", "rekey",
    "decrypt-1:", "decrypt-63:", "decrypt-64:", "decrypt-65:", "decrypt-129:", "decrypt-1500:", "layout"])
def test_case_ran(run, case):
    assert "ok " + case in run.stdout, run.stdout[-3000:]
