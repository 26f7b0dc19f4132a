"""Evidence that the operand ranges the short divisions claim hold (-m gpu): renders with the library variant built with -DFH_CHECK_DIV_RANGES, in which every
converted site (fredholm_amd/csrc/fh_vec.h: div_r, div_r_nofix, normalize_r) counts the calls whose operands leave the range written at the site.  The count must be 0.

The variant is a second library (fredholm_amd/libfredholm_hip_divranges.so, built by fredholm_amd/csrc/Makefile next to the default one) and a process loads one
library, so the renders run in ONE child process -- this file, run as a script with FH_LIB set -- which prints one JSON line.  The counter belongs to the device code, not
to a context: the child reads it at the end from a context of its own (fh_stats.div_range_violations).  Last of all the child renders with a camera OUTSIDE the claims
(a field of view of 1e-7 rad: 1 / tan(fov / 2) = 2e7 > 2^21), which must count: the check that the library in use is the counting one.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANT = os.path.join(ROOT, "fredholm_amd", "libfredholm_hip_divranges.so")
SEEDS = range(101, 141)  # 40 seeds of tests/test_gpu_parity.py: test_random_materials_textures_and_lights_match_checker, as tools/fuzz_more.py runs them


def _child():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import fredholm_amd as F
    from fredholm_amd import scenes
    from oracle import pyoracle as O
    import test_gpu_parity as T
    O.lib()
    W, H, SPP, DEPTH = 96, 64, 8, 5

    def total():
        r = F.Renderer(0)
        r.wait_for_completion()
        n = r.stats()["div_range_violations"]
        r.close()
        return int(n)

    def render(sc, cam, setup=None, bg=(0.1, 0.2, 0.4)):
        r = F.Renderer(0)
        r.load_scene(sc)
        r.build_ias()
        if setup:
            setup(r)
        r.set_resolution(W, H)
        L = F.RenderLayer(r, W, H)
        r.render(cam, bg, L, SPP, DEPTH)
        r.wait_for_completion()
        finite = bool(np.isfinite(L.download("beauty")).all())
        paths = r.stats()["paths"]
        r.close()
        return finite, int(paths)

    def sky(x):
        x.set_directional_light((0, 0, 0), scenes.SOUP_SUN, 0.0)
        x.load_arhosek_sky(3.0, 0.3)

    soup = scenes.triangle_soup(500, 0.3)
    lo, hi = soup["vertices"].min(axis=0), soup["vertices"].max(axis=0)
    size = float(np.linalg.norm(hi - lo))
    out = {"renders": {}}
    cases = {
        "soup_500_hosek": (soup, F.Camera(**scenes.SOUP_CAMERA), sky),
        "cornell_area_light": (scenes.cornell_box(), F.Camera(**scenes.CORNELL_CAMERA), None),
        "textured_cornell": (scenes.textured_cornell_box(), F.Camera(**scenes.CORNELL_CAMERA), None),
        "soup_wide_open_lens": (soup, F.Camera(**dict(scenes.SOUP_CAMERA, F=1.0, focus=3.0)), sky),
        "cornell_wide_open_lens": (scenes.cornell_box(), F.Camera(**dict(scenes.CORNELL_CAMERA, F=1.0, focus=2.0)), None),
        "soup_camera_1000_sizes_away": (soup, F.Camera(**dict(scenes.SOUP_CAMERA, origin=(0.0, 0.0, 1000.0 * size), fov=0.002)), sky),
        "soup_camera_1000_sizes_away_wide": (soup, F.Camera(**dict(scenes.SOUP_CAMERA, origin=(0.0, 0.3 * size, 1000.0 * size))), sky),
    }
    for name, (sc, cam, setup) in cases.items():
        finite, paths = render(sc, cam, setup)
        out["renders"][name] = {"finite": finite, "paths": paths, "violations_so_far": total()}
    failed = []
    for seed in SEEDS:
        try:
            T.test_random_materials_textures_and_lights_match_checker(O, seed)
        except AssertionError as e:  # (parity with the checker is that test's business; it is reported, and the counter is read all the same)
            failed.append([seed, str(e)[:120]])
    out["random_material_seeds"] = len(SEEDS)
    out["random_material_parity_failures"] = failed
    out["violations"] = total()
    render(scenes.cornell_box(), F.Camera(**dict(scenes.CORNELL_CAMERA, fov=1e-7)))
    out["violations_after_a_camera_outside_the_claims"] = total()
    print(json.dumps(out), flush=True)


@pytest.fixture(scope="module")
def variant_library():
    if not os.path.exists(VARIANT):
        p = subprocess.run(["make", "-C", os.path.join(ROOT, "fredholm_amd", "csrc"), "-j", "6", "../libfredholm_hip_divranges.so"], capture_output=True, text=True)
        if p.returncode != 0 or not os.path.exists(VARIANT):
            pytest.skip("the -DFH_CHECK_DIV_RANGES variant of the library cannot be built here: " + (p.stderr.strip().splitlines() or ["make failed"])[-1][:200])
    return VARIANT


@pytest.fixture(scope="module")
def record(variant_library):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, FH_LIB=variant_library), capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(rec, indent=1))
    return rec


@pytest.mark.gpu
def test_no_operand_leaves_its_claimed_range_in_the_scenes_and_cameras(record):
    r = record["renders"]
    assert set(r) >= {"soup_500_hosek", "cornell_area_light", "textured_cornell", "soup_wide_open_lens", "soup_camera_1000_sizes_away"}
    for name, v in r.items():
        assert v["paths"] == 96 * 64 * 8 and v["finite"], (name, v)
        assert v["violations_so_far"] == 0, (name, v)


@pytest.mark.gpu
def test_no_operand_leaves_its_claimed_range_in_forty_random_material_scenes(record):
    assert record["random_material_seeds"] >= 40
    assert record["random_material_parity_failures"] == []
    assert record["violations"] == 0


@pytest.mark.gpu
def test_the_library_that_rendered_them_counts(record):
    assert record["violations"] == 0 and record["violations_after_a_camera_outside_the_claims"] > 0


if __name__ == "__main__":
    _child()
