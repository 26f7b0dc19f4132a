"""Dark sky pixels (render.hip: k_split_pixels, k_dark_pixels; fh_dark_sky.h: dark_sky_pixel; render_plan_host.h: dark_sky_verdict).

Under the Hosek sky every sample of a sky pixel whose rays all point below the horizon is NaN, which the guard counts as zero.  Such pixels skip k_sky_pixels: k_dark_pixels
applies the updates of the running means that samples of value zero make.  FH_DARK_SKY=1 against =0 therefore has to match bit for bit: the six layers, sample_count
and the issued count (fh_kat_sample_counts), for every camera and call pattern below.

The switch is read when a context is created, so each side runs in a fresh child process: this file, run as a program, renders every case of CASES under the
FH_DARK_SKY it finds and writes the results to an .npz; the two children run once per session (fixture `sides`).  FH_DEBUG_TAIL=1 makes every call that split off sky
pixels print "[dark-sky] <dark> of <sky> sky pixels are dark" to stderr, which is where the dark counts come from: a comparison of a path with itself cannot pass for one of the two.

Scene and frame: a 500-face soup under the Hosek sky, 96 x 64, depth 5, the split forced on for small calls (FH_SKY_SPLIT_MIN_LOG2=0)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

W, H, DEPTH = 96, 64, 5
BG = (0.0, 0.0, 0.0)
FOV = float(np.radians(60.0))


def _pitched(deg):
    a = np.radians(deg)
    return dict(origin=(0.0, 0.0, 3.0), forward=(0.0, float(np.sin(a)), float(-np.cos(a))), fov=FOV, F=100.0, focus=10000.0)


LEVEL, UP, DOWN = _pitched(0.0), _pitched(40.0), _pitched(-40.0)
WIDE = dict(LEVEL, F=2.0, origin=(0.0, 0.0, 12.0))  # (lens radius 2 f / F = 1.73: from three units away every pixel of the frame has a ray that reaches the soup, and nothing splits)

# name -> list of (camera, roll in degrees, samples) calls into one set of layers, and whether the context renders adaptively
CASES = {
    "level_17_16": ([(LEVEL, 0.0, 17), (LEVEL, 0.0, 16)], False),   # 33 spp: crosses a CMJ block of sixteen and resumes the means
    "up_17_16": ([(UP, 0.0, 17), (UP, 0.0, 16)], False),            # no dark pixel
    "down_17_16": ([(DOWN, 0.0, 17), (DOWN, 0.0, 16)], False),      # nearly every sky pixel dark
    "rolled_17_16": ([(LEVEL, 30.0, 17), (LEVEL, 30.0, 16)], False),  # the horizon crosses the groups of 64 pixels
    "wide_17_16": ([(WIDE, 0.0, 17), (WIDE, 0.0, 16)], False),      # F = 2: large footprints
    # pitched up, then down without init_render_states: the dark pixels of the second call carry non-zero beauty (and, where the soup was seen, AOV) means, so the
    # recurrences run; the third call renders them again from the issued count the second left
    "up_8_down_9_up_4": ([(UP, 0.0, 8), (DOWN, 0.0, 9), (UP, 0.0, 4)], False),
    "level_4x1": ([(LEVEL, 0.0, 1)] * 4, False),                    # against the CPU checker, rows around the horizon
    "adaptive_level_24": ([(LEVEL, 0.0, 24)], True),                # keeps the old path
}
DARK_EXPECTED = {"level_17_16": True, "up_17_16": False, "down_17_16": True, "rolled_17_16": True}


def _camera(F, cam, roll):
    c = F.Camera(**cam)
    if roll:
        a = np.radians(roll)
        m = np.array(c.m_transform, dtype=np.float64)
        r, u = m[:, 0].copy(), m[:, 1].copy()
        m[:, 0] = np.cos(a) * r + np.sin(a) * u
        m[:, 1] = -np.sin(a) * r + np.cos(a) * u
        c.m_transform = m.astype(np.float32)
    return c


def _worker(out_path):
    import ctypes as C

    import fredholm_amd as F
    from fredholm_amd import native as N
    from fredholm_amd import scenes

    r = F.Renderer(0)
    r.load_scene(scenes.triangle_soup(500, 0.1))
    r.build_ias()
    r.load_arhosek_sky(3.0, 0.3)
    r.set_resolution(W, H)
    out = {}
    for name, (calls, adaptive) in CASES.items():
        print(f"[case] {name}", file=sys.stderr, flush=True)
        r.init_render_states()
        if adaptive:
            r.set_adaptive_sampling(0.05, min_samples=8, step=4)
        L = F.RenderLayer(r, W, H)
        for cam, roll, n in calls:
            r.render(_camera(F, cam, roll), BG, L, n, DEPTH)
        r.wait_for_completion()  # (raises on a bounds-test violation)
        for layer in F.RenderLayer.NAMES:
            out[f"{name}/{layer}"] = L.download(layer)
        sc, iss = np.empty((H, W), np.uint32), np.empty((H, W), np.uint32)
        N.check(r._ctx, N.lib().fh_kat_sample_counts(r._ctx, N.ptr(sc), N.ptr(iss), C.c_uint32(W * H)), "fh_kat_sample_counts")
        out[f"{name}/sample_count"], out[f"{name}/issued"] = sc, iss
        L.free()
    r.close()
    np.savez(out_path, **out)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def sides(tmp_path_factory):
    """{switch: (arrays, {case: [(dark, sky) per call that split off sky pixels]})}"""
    d = tmp_path_factory.mktemp("dark_sky")
    got = {}
    for switch in ("0", "1"):
        path = str(d / f"side{switch}.npz")
        env = dict(os.environ, FH_DARK_SKY=switch, FH_SKY_SPLIT_MIN_LOG2="0", FH_DEBUG_TAIL="1")
        env.pop("FH_SKY_SPLIT", None)
        run = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stderr[-4000:]
        dark, case = {}, None
        for line in run.stderr.splitlines():
            if line.startswith("[case] "):
                case = line[7:].strip()
                dark[case] = []
            m = re.match(r"\[dark-sky\] (\d+) of (\d+) sky pixels are dark", line)
            if m:
                dark[case].append((int(m.group(1)), int(m.group(2))))
        got[switch] = (dict(np.load(path)), dark)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_dark_sky_pixels_keep_every_bit(sides, case):
    (off, dark_off), (on, dark_on) = sides["0"], sides["1"]
    import fredholm_amd as F
    assert len(F.RenderLayer.NAMES) == 6
    for key in list(F.RenderLayer.NAMES) + ["sample_count", "issued"]:
        a, b = off[f"{case}/{key}"], on[f"{case}/{key}"]
        same = _bits(a) == _bits(b)
        assert same.all(), f"{case}, {key}: {int((~same).sum())} values differ"
    calls, adaptive = CASES[case]
    total = sum(n for _, _, n in calls)
    if not adaptive:
        assert (on[f"{case}/sample_count"] == total).all() and (on[f"{case}/issued"] == total).all()
    assert len(dark_on[case]) == len(dark_off[case]) == len(calls)  # every call split off sky pixels, on both sides
    assert all(d == 0 for d, _ in dark_off[case])
    assert [s for _, s in dark_on[case]] == [s for _, s in dark_off[case]]  # the sky list and the dark list together are the sky list of before
    print(case, "dark / sky pixels per call:", dark_on[case])
    if adaptive:
        assert all(d == 0 for d, _ in dark_on[case])  # (dark_sky_verdict: an adaptive call keeps the old path)
        assert on[f"{case}/sample_count"].min() < total  # ... and it did stop pixels
    if case in DARK_EXPECTED:
        for d, _ in dark_on[case]:
            assert (d > 0) == DARK_EXPECTED[case], dark_on[case]
    if case == "up_8_down_9_up_4":
        (d0, _), (d1, s1), (d2, _) = dark_on[case]
        assert d0 == 0 and d1 > 0 and d2 == 0
        assert np.abs(on[f"{case}/beauty"][..., :3]).max() > 0.0
    if case == "down_17_16":
        d, s = dark_on[case][0]
        assert d >= 0.9 * s, (d, s)


@pytest.mark.gpu
def test_level_camera_matches_the_checker_around_the_horizon(sides, oracle):
    """4 spp of the level camera, rows 24..40 of 64 (the horizon runs between rows 31 and 32; the rule's margin keeps the two or three rows next to it on the dark side ordinary sky
    pixels, the rows beyond them are dark): the beauty layer equals the CPU checker's bit for bit, by the rule of bench.py's parity_block (99.9 % of the pixels; here: all of them, or
    RMSE <= 1e-5 of the crop's mean)."""
    import fredholm_amd as F
    from fredholm_amd import scenes
    on, dark_on = sides["1"]
    assert all(d > 0 for d, _ in dark_on["level_4x1"])
    rows = (24, 40)
    S = oracle.Scene(scenes.triangle_soup(500, 0.1))
    S.load_arhosek_sky(3.0, 0.3)
    Lo = S.new_layers(W, H)
    for _ in range(4):
        S.render(F.Camera(**LEVEL).params(), W, H, Lo, 1, DEPTH, bg=BG, n_threads=8, rows=rows)
    gpu, ref = on["level_4x1/beauty"][rows[0]:rows[1]], Lo["beauty"][rows[0]:rows[1]]
    same = float((_bits(gpu) == _bits(ref)).all(axis=2).mean())
    a, b = np.nan_to_num(gpu[..., :3].astype(np.float64)), np.nan_to_num(ref[..., :3].astype(np.float64))
    rmse = float(np.sqrt(((a - b) ** 2).mean()))
    print(f"bit-identical pixels {same:.5f}, rmse {rmse:.3e}, crop mean {b.mean():.5f}")
    assert same >= 0.999 and rmse <= 1e-5 * max(float(b.mean()), 1e-6)


if __name__ == "__main__":
    _worker(sys.argv[1])
