"""What the dark-sky-pixel rule rests on (fredholm_amd/csrc/fh_dark_sky.h, render_plan_host.h: dark_sky_verdict), as a stand-alone program: no GPU, no library.

tools/dark_sky_check.cpp goes through every float in [-1, -2^-11] to show that the Hosek sky's `zenith` is NaN there (the device's bits: include/fh_elementary.h),
through the verdict's truth table, and through 12800 pixels of 200 random cameras on which the rule is compared with a brute-force, double-precision thin lens."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dark_sky_check_program_passes(tmp_path):
    exe = tmp_path / "dark_sky_check"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", os.path.join(ROOT, "tools", "dark_sky_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0 and "dark_sky_check: ok" in run.stdout and "FAILED" not in run.stdout, run.stdout
    # (a) is exhaustive: every float from -1 to -2^-11, i.e. the bit patterns 0xba000000 ... 0xbf800000
    assert "(a) %d floats in [-1, -2^-11]: zenith is NaN for all but 0" % (0xbf800000 - 0xba000000 + 1) in run.stdout
    assert "(b) dark_sky_verdict: 128 cases" in run.stdout
    m = re.search(r"\(c\) 12800 pixels, (\d+) called dark, (\d+) truly dark", run.stdout)
    assert m and 0 < int(m.group(1)) <= int(m.group(2))  # the rule is conservative: it calls no more pixels dark than are
