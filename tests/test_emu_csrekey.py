"""CPU-side check of the in-band rekey schedule of the CipherState tables
(noise_gpu_csrekey_*): the unmodified csrc/cstate_kernels.hip and
csrc/cstate_calls.hpp compiled as host C++ against the HIP stand-in in
tools/emu and run as a stand-alone program (tools/emu/emu_csrekey.cpp) under
AddressSanitizer; nothing is loaded into Python.  The build caps the grid at 3
workgroups and cuts the sort into 640-record chunks, as emu_cstate's.  Every
batch goes through cs_inorder_call; only the AEAD launch inside it is a
stand-in, which records the 32 key bytes and the nonce each record was handed.
The program compares those, the statuses, the final key rows (chains of the
oracle's REKEY) and the counters with the loop of include/noise_gpu.h
    status = encrypt / decrypt(record); if n moved and n % every == 0: rekey()
and checks after every call that the private key rows of the scratch are zero.
The scratch and all arrays have their exact sizes.  A case fails if the loop
never produced the status or the crossing it is about.  Test infrastructure
only: the product runs these kernels on the GPU (tests/test_gpu_csrekey.py)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tools", "emu")
BIN = os.path.join(EMU, "build", "emu_csrekey")
EVERY = [1, 2, 3, 64, 1000, 1 << 32, 1 << 63, (1 << 64) - 1]
COUNTS = [1, 63, 64, 65, 129, 1500]


@pytest.fixture(scope="module")
def run():
    r = subprocess.run(["make", "-j4", "-C", EMU, "GRID_CAP=3u", "csrekey"], capture_output=True,
                       text=True, timeout=900)
    if r.returncode != 0:
        pytest.fail("emulation build failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    return subprocess.run([BIN], capture_output=True, text=True, timeout=900, env=env)


def test_emulated_schedule_matches_the_loop(run):
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "emu_csrekey: all ok" in run.stdout and "FAIL" not in run.stdout
    assert "AddressSanitizer" not in run.stderr


@pytest.mark.parametrize("every", EVERY)
def test_grid_ran(run, every):
    """Every batch size at this `every`, two back-to-back batches each; over them 1, 5 and 300 sessions."""
    nsess = set()
    for nrec in COUNTS:
        lines = [ln for ln in run.stdout.splitlines()
                 if ln.startswith("ok grid-e%d-r%d-s" % (every, nrec)) and "every %d," % every in ln]
        assert len(lines) == 2, (nrec, run.stdout[-2000:])
        nsess.add(lines[0].split("-s")[1].split(":")[0])
    assert nsess == {"1", "5", "300"}


@pytest.mark.parametrize("nrec", COUNTS)
def test_grid_covers_every_session_count_at_every_batch_size(run, nrec):
    got = {ln.split("-s")[1].split(":")[0] for ln in run.stdout.splitlines()
           if ln.startswith("ok grid-e") and "-r%d-s" % nrec in ln}
    assert got == {"1", "5", "300"}


@pytest.mark.parametrize("case", [
    "arith", "cross3-small:", "cross3-sorted:", "cross3-chunks:", "every1-1500:", "last-hit-1:", "last-hit-64:",
    "last-hit-129:", "last-hit-1500:", "last-hit-limit:", "wrap-small:", "wrap-sorted:", "wrap-max:", "room-1:",
    "traps-5:", "traps-64:", "traps-65:", "traps-1500:", "traps-1500-e1:"])
def test_case_ran_in_every_form(run, case):
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("ok " + case)]
    if case == "arith":
        assert len(lines) == 1
        return
    forms = {(("descriptors" in ln), ("decrypt" in ln)) for ln in lines}
    assert len(lines) == 4 and len(forms) == 4, lines


@pytest.mark.parametrize("nrec", [1, 64, 65, 1500])
def test_schedule_switched_off_is_the_existing_path(run, nrec):
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("ok off-%d:" % nrec)]
    assert len(lines) == 4, run.stdout[-2000:]
