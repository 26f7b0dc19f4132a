"""The owning types of fredholm_amd/csrc/fh_memory.h (DeviceBuffer, PinnedBuffer, Event, Stream) as a stand-alone program: no GPU, no library.

tools/fh_memory_check.cpp replaces the header's seam with a counting fake that can refuse an allocation, and checks the 16-byte floor, grow-only ensure, what a failure
leaves behind, moves, release, the destructors, a vector of buffers that reallocates, and that nothing is live at the end."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fh_memory_check_program_passes(tmp_path):
    exe = tmp_path / "fh_memory_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tools", "fh_memory_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "fh_memory_check: ok" in run.stdout, run.stdout
