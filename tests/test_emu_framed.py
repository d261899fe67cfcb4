"""CPU-side check of the stream-framing kernels and calls: the unmodified
csrc/framed_kernels.hip and csrc/framed_calls.hpp compiled as host C++ against
the HIP stand-in in tools/emu, over the unmodified table kernels
(csrc/cstate_kernels.hip) and composition (csrc/cstate_calls.hpp), run as a
stand-alone program (tools/emu/emu_framed.cpp) under AddressSanitizer.  The
build caps the grid at 3 workgroups and cuts the sort into 640-record chunks.
d_recs, status, the per-connection arrays and the outputs are allocated at their
exact sizes and the scratch at framed_scratch_layout's total; while a call runs,
the received bytes are addressable for exactly len[j] bytes per connection, so a
read past a partial tail is an ASan report.  Every case is checked inside the
program against the plain loops of include/noise_gpu.h plus CipherState's n++:
statuses, d_recs, all per-connection outputs, every output and gap byte, the
counters.  A case fails if the model never produced a status it is about.  Only
the AEAD launch is a stand-in.  Test infrastructure only: the product runs these
kernels on the GPU (tests/test_gpu_framed.py)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tools", "emu")
BIN = os.path.join(EMU, "build", "emu_framed")


@pytest.fixture(scope="module")
def run():
    r = subprocess.run(["make", "-j4", "-C", EMU, "GRID_CAP=3u", "framed"], capture_output=True,
                       text=True, timeout=900)
    if r.returncode != 0:
        pytest.fail("emulation build failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    return subprocess.run([BIN], capture_output=True, text=True, timeout=900, env=env)


def test_emulated_framed_calls_match_the_loops(run):
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "emu_framed: all ok" in run.stdout and "FAIL" not in run.stdout
    assert "AddressSanitizer" not in run.stderr


@pytest.mark.parametrize("case", ["mixed-1:", "mixed-63:", "mixed-64:", "mixed-65:", "mixed-129:", "mixed-1500:",
                                  "limit:"])
def test_case_ran_both_ways(run, case):
    # two batches each, a copy and in place for open
    assert run.stdout.count("ok open " + case) == 2, run.stdout[-3000:]
    assert run.stdout.count("ok seal " + case) == 2, run.stdout[-3000:]


FORMS = ["form-%s-%s" % (a, b) for a in ("stride", "off") for b in ("lenall", "len")]
CAPS = ["total", "total-1", "mid", "one", "total+70"]


@pytest.mark.parametrize("case,count",
                         [("ok open %s-%s:" % (f, c), 1) for f in FORMS for c in ("copy", "inplace")] +
                         [("ok seal %s-copy:" % f, 1) for f in FORMS] +
                         [("ok %s align-%d-%s:" % (w, a, c), 1) for w in ("open", "seal") for a in (0, 1, 2, 14)
                          for c in CAPS] +
                         [("ok open tail-%d-%s:" % (t, c), 1) for t in range(4) for c in ("copy", "inplace")] +
                         [("ok open badlen-%d-at-%d:" % (L, at), 1) for L in (0, 15) for at in range(3)] +
                         [("ok open longest:", 2), ("ok seal largest:", 2)])
def test_edge_case_ran(run, case, count):
    assert run.stdout.count(case) == count, run.stdout[-3000:]
