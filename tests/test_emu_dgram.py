"""CPU-side check of the datagram kernels and calls: the unmodified
csrc/dgram_kernels.hip and csrc/dgram_calls.hpp compiled as host C++ against
the HIP stand-in in tools/emu, over the unmodified table kernels
(csrc/cstate_kernels.hip, csrc/cswin_kernels.hip) and compositions
(csrc/cstate_calls.hpp), run as a stand-alone program (tools/emu/emu_dgram.cpp)
under AddressSanitizer.  The build caps the grid at 3 workgroups and cuts the
sort into 640-record chunks.  Packet buffers, outputs, d_recs, status and length
arrays are allocated at their exact sizes and the scratch at cs_scratch_layout's
total; a malformed packet is stored only as far as it may be read (its header,
or nothing where its length alone refuses it), so a read past a short packet or
a store past a slot is an ASan report.  Every case is checked inside the
program against the plain loops of include/noise_gpu.h -- open: malformed
packets out, then the windowed loop over noise::ReplayWindow; seal:
CipherState's n++ -- statuses, d_recs, lengths, every output and gap byte,
counters, next and the bitmap rows.  A case fails if the model never produced a
status it is about.  Only the AEAD launch is a stand-in.  Test infrastructure
only: the product runs these kernels on the GPU (tests/test_gpu_dgram.py)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tools", "emu")
BIN = os.path.join(EMU, "build", "emu_dgram")


@pytest.fixture(scope="module")
def run():
    r = subprocess.run(["make", "-j4", "-C", EMU, "GRID_CAP=3u", "dgram"], capture_output=True,
                       text=True, timeout=900)
    if r.returncode != 0:
        pytest.fail("emulation build failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    return subprocess.run([BIN], capture_output=True, text=True, timeout=900, env=env)


def test_emulated_datagram_calls_match_the_loops(run):
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "emu_dgram: all ok" in run.stdout and "FAIL" not in run.stdout
    assert "AddressSanitizer" not in run.stderr


FORMS = ["form-%s-%s-%s:" % (a, b, c) for a in ("stride", "off") for b in ("lenall", "len")
         for c in ("copy", "inplace")]
ALIGNS = ["align-%d-%s:" % (a, c) for a in (0, 1, 4, 8) for c in ("copy", "inplace")]


@pytest.mark.parametrize("case", ["mixed-1:", "mixed-63:", "mixed-64:", "mixed-65:", "mixed-129:",
                                  "mixed-1500:"] + FORMS + ALIGNS)
def test_case_ran_both_ways(run, case):
    # each of these prints one line per batch, two batches, for open and for seal
    assert run.stdout.count("ok open " + case) == 2, run.stdout[-3000:]
    assert run.stdout.count("ok seal " + case) == 2, run.stdout[-3000:]


@pytest.mark.parametrize("case,count", [("ok open limits-1500:", 2), ("ok seal overlength-3:", 1),
                                        ("ok seal overlength-203:", 1), ("ok seal overlength-stride:", 1)] +
                         [("ok open lengths-%d-%s:" % (a, c), 8) for a in (0, 1, 4, 8)
                          for c in ("copy", "inplace")])
def test_edge_case_ran(run, case, count):
    assert run.stdout.count(case) == count, run.stdout[-3000:]
