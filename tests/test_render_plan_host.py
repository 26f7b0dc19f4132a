"""The host-only decisions of fh_render's submit path (fredholm_amd/csrc/render_plan_host.h) as a stand-alone program: no GPU, no library.

tools/render_plan_check.cpp holds the cases the code's own comments state, derived by hand, and replays tests/golden/render_plan_cases.json: the inputs and the outputs
of the same lines while they were still inside render_submit (tools/README.md), equal to the last bit."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_render_plan_check_program_passes(tmp_path):
    exe = tmp_path / "render_plan_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", os.path.join(ROOT, "tools", "render_plan_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cases = os.path.join(ROOT, "tests", "golden", "render_plan_cases.json")
    run = subprocess.run([str(exe), cases], capture_output=True, text=True)
    assert run.returncode == 0 and "render_plan_check: ok" in run.stdout, run.stdout
    # the program replayed every row of the table, and the table has rows for every function of the header
    rows = json.load(open(cases))
    assert "(%d cases)" % len(rows) in run.stdout, run.stdout
    assert {r["fn"] for r in rows} == {"pool_target_cap", "samples_per_pass", "stream_lds_entries", "stream_wgs", "stream_chunk", "tail_wave_depth", "fold_survival", "fold_probe_cost",
                                      "bottom_up_verdict", "lens_values"}
    # a table it cannot read, or one whose expected value is off by one bit, fails
    assert subprocess.run([str(exe), str(tmp_path / "missing.json")], capture_output=True, text=True).returncode != 0
    k = next(i for i, r in enumerate(rows) if r["fn"] == "lens_values")
    rows[k]["out"][0] ^= 1
    bad = tmp_path / "bad.json"
    bad.write_text(json.dumps(rows))
    run = subprocess.run([str(exe), str(bad)], capture_output=True, text=True)
    assert run.returncode != 0 and "render_plan_check: 1 failures" in run.stdout and "FAILED case %d (lens_values)" % k in run.stdout, run.stdout
