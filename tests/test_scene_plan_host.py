"""The host-only decisions of a scene upload (fredholm_amd/csrc/scene_plan_host.h) as a stand-alone program: no GPU, no library.

tools/scene_plan_check.cpp holds the cases the code's own comments state, derived by hand, and replays tests/golden/scene_plan_cases.json: the inputs and the outputs
of the same lines while they were still inside capi.hip's rebuild_device_scene and upload_textures (tools/README.md), equal to the last bit."""
import json
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# functions of the header whose rows are those of plan_scene, which is made of them: a plan_scene row holds one hash or counter per part of the plan
PARTS_OF_PLAN_SCENE = {"scene_arguments_error", "plan_textures", "plan_materials", "plan_faces", "plan_alpha_records", "face_texcoords", "srgb_decode_table", "plan_lum"}


def test_scene_plan_check_program_passes(tmp_path):
    exe = tmp_path / "scene_plan_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", os.path.join(ROOT, "tools", "scene_plan_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cases = os.path.join(ROOT, "tests", "golden", "scene_plan_cases.json")
    run = subprocess.run([str(exe), cases], capture_output=True, text=True)
    assert run.returncode == 0 and "scene_plan_check: ok" in run.stdout, run.stdout
    # the program replayed every row of the table, and the table has rows for every function of the header
    rows = json.load(open(cases))
    assert "(%d cases)" % len(rows) in run.stdout, run.stdout
    header = open(os.path.join(ROOT, "fredholm_amd", "csrc", "scene_plan_host.h")).read()
    functions = set(re.findall(r"^inline [\w:<>*& ]*?[ *&](\w+)\(", header, flags=re.M))
    assert len(functions) >= 19 and "footprint_class" in functions and "plan_scene" in functions, functions
    assert {r["fn"] for r in rows} == functions - PARTS_OF_PLAN_SCENE
    assert PARTS_OF_PLAN_SCENE < functions
    # whole scenes: refused ones with every message, and accepted ones with any-hit records, with and without each switch
    scenes = [r for r in rows if r["fn"] == "plan_scene"]
    assert {r["out"][0] for r in scenes} == set(range(8))
    assert sum(1 for r in scenes if r["out"][0] == 0 and r["out"][15] > 1) >= 100
    assert {(r["in"][2] != 0, r["in"][3] != 0) for r in scenes} == {(False, False), (True, False), (False, True), (True, True)}
    # a table it cannot read, or one whose expected value is off by one bit, fails
    assert subprocess.run([str(exe), str(tmp_path / "missing.json")], capture_output=True, text=True).returncode != 0
    for fn, word in (("material_lobes", 0), ("shading_classes", 0), ("texel_span", 1), ("footprint_class", 0), ("cell_corners", 5), ("micromap_words", 3), ("plan_scene", 7), ("plan_scene", 16)):
        k = next(i for i, r in enumerate(rows) if r["fn"] == fn and (fn != "plan_scene" or (r["out"][0] == 0 and r["out"][15] > 1)))
        flipped = json.loads(json.dumps(rows))
        flipped[k]["out"][word] ^= 1
        bad = tmp_path / "bad.json"
        bad.write_text(json.dumps(flipped))
        run = subprocess.run([str(exe), str(bad)], capture_output=True, text=True)
        assert run.returncode != 0 and "scene_plan_check: 1 failures" in run.stdout and "FAILED case %d (%s)" % (k, fn) in run.stdout, run.stdout
