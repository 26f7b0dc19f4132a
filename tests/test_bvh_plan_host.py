"""The host-only decisions of the BVH build (fredholm_amd/csrc/bvh_plan_host.h) as a stand-alone program: no GPU, no library.

tools/bvh_plan_check.cpp holds the cases the code's own comments state, derived by hand, and replays tests/golden/bvh_plan_cases.json: the inputs and the outputs
of the same lines while they were still inside bvh_build_device (tools/README.md), equal to the last bit."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bvh_plan_check_program_passes(tmp_path):
    exe = tmp_path / "bvh_plan_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", os.path.join(ROOT, "tools", "bvh_plan_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cases = os.path.join(ROOT, "tests", "golden", "bvh_plan_cases.json")
    run = subprocess.run([str(exe), cases], capture_output=True, text=True)
    assert run.returncode == 0 and "bvh_plan_check: ok" in run.stdout, run.stdout
    # the program replayed every row of the table, and the table has rows for every function of the header
    rows = json.load(open(cases))
    assert "(%d cases)" % len(rows) in run.stdout, run.stdout
    assert {r["fn"] for r in rows} == {"build_switches", "scene_padding", "split_cells", "refit_eligible", "refit_accepted", "tree_shape", "split_enabled", "split_search", "builder",
                                       "collapse_plan", "collapse_limits", "tree_refittable", "tree_stats"}
    # a table it cannot read, or one whose expected value is off by one bit, fails
    assert subprocess.run([str(exe), str(tmp_path / "missing.json")], capture_output=True, text=True).returncode != 0
    for fn in ("scene_padding", "split_search", "builder", "tree_stats"):
        k = next(i for i, r in enumerate(rows) if r["fn"] == fn)
        flipped = json.loads(json.dumps(rows))
        flipped[k]["out"][1] ^= 1
        bad = tmp_path / "bad.json"
        bad.write_text(json.dumps(flipped))
        run = subprocess.run([str(exe), str(bad)], capture_output=True, text=True)
        assert run.returncode != 0 and "bvh_plan_check: 1 failures" in run.stdout and "FAILED case %d (%s)" % (k, fn) in run.stdout, run.stdout
