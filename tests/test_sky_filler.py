"""GPU tests (-m gpu): the sky pixels of a call rendered by a filler launch beside the passes and a drain launch behind them, over one cursor (render.hip: k_sky_pixels).

Which of the two launches renders a group of 64 sky pixels is a race by design; what a pixel holds afterwards is not: one lane runs all samples of the call for it, with
the operations k_generate / k_accumulate apply.  So every comparison here is bit for bit -- all six layers and the sample counts, any two NaNs counting as equal --
against the CPU checker, under three settings of the filler: off (the drain renders everything), one workgroup in total (the drain renders most groups) and one
workgroup per CU (the default).  The AOV means of a sky pixel are brought up to date after its sample loop, and not at all where they hold +0: pixels that carry AOV
state, -0 and NaN included, are compared too.  Small frames with the sky split forced (FH_SKY_SPLIT_MIN_LOG2=0); the checker renders each case once, one sample per call.
"""
import numpy as np
import pytest

import fredholm_amd as F
from fredholm_amd import scenes

pytestmark = pytest.mark.gpu

W, H = 128, 96
NAMES = F.RenderLayer.NAMES
BG = (0.05, 0.1, 0.2)
DEPTH = 5
FILLER = {"off": {"FH_SKY_BLOCKS": "0"}, "one_workgroup": {"FH_SKY_FILLER_GRID": "1"}, "one_per_cu": {"FH_SKY_BLOCKS": "1"}}
SWITCHES = ("FH_SKY_SPLIT", "FH_PIPELINE", "FH_SKY_SPLIT_MIN_LOG2", "FH_SKY_BLOCKS", "FH_SKY_FILLER_GRID")

# the 1000-triangle soup from far enough away that more than half of the frame is sky
CAM_FAR = dict(origin=(0.4, 0.2, 6.0), fov=1.2, F=16.0, focus=6.0, forward=(-0.15, -0.05, -1.0))
# a camera that sees the soup in the middle of the frame, and the same camera turned until those pixels see the sky
CAM_NEAR = dict(origin=(0.4, 0.2, 4.0), fov=1.2, F=16.0, focus=4.0, forward=(-0.15, -0.05, -1.0))
CAM_TURNED = dict(origin=(0.4, 0.2, 4.0), fov=1.2, F=16.0, focus=4.0, forward=(-1.0, -0.05, -0.6))

_CACHE = {}


def _soup():
    if "soup" not in _CACHE:
        _CACHE["soup"] = scenes.triangle_soup(1000, 0.1)
    return _CACHE["soup"]


def _context(monkeypatch, env, w=W, h=H, scene=None):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    e = {"FH_SKY_SPLIT_MIN_LOG2": "0"}
    e.update(env)
    for k, v in e.items():
        monkeypatch.setenv(k, v)
    r = F.Renderer(0)  # (the environment is read here)
    for k in e:
        monkeypatch.delenv(k)
    r.load_scene(_soup() if scene is None else scene)
    r.build_ias()
    r.set_directional_light((0.0, 0.0, 0.0), scenes.SOUP_SUN, 0.0)
    r.clear_directional_light()
    r.load_arhosek_sky(3.0, 0.3)
    r.set_resolution(w, h)
    return r, F.RenderLayer(r, w, h)


def _checker(oracle):
    import ctypes as C
    S = oracle.Scene(_soup())
    S.set_directional_light((0.0, 0.0, 0.0), scenes.SOUP_SUN, 0.0)
    oracle.lib().orc_set_directional_light(S.h, 0, None, None, C.c_float(0))
    S.load_arhosek_sky(3.0, 0.3)
    return S


def _state(r, L):
    r.wait_for_completion()
    s = {n: L.download(n) for n in NAMES}
    s["sample_count"] = r.sample_counts()
    return s


def _assert_same(got, want, what, keys=NAMES + ("sample_count",)):
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if a.dtype == np.float32:
            eq = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
        else:
            eq = a == b
        eq = eq.reshape(a.shape[0] * a.shape[1], -1).all(axis=1)
        bad = np.flatnonzero(~eq)
        print(f"{what}: {k}: {bad.size} of {eq.size} pixels differ")
        assert bad.size == 0, f"{what}: {k} differs in {bad.size} pixels, the first at pixel {bad[0]}"


# ------------------------------------------------------------------ a frame that is mostly sky, 40 samples in three calls
def _frame_reference(oracle):
    if "frame" not in _CACHE:
        S = _checker(oracle)
        Lo = S.new_layers(W, H)
        cam = F.Camera(**CAM_FAR)
        for _ in range(16 + 8 + 16):  # (one sample per call: a checker call of several samples carries the reference's first-hit state through the launch)
            S.render(cam.params(), W, H, Lo, 1, DEPTH, bg=BG, n_threads=8)
        _CACHE["frame"] = Lo
    return _CACHE["frame"]


@pytest.mark.parametrize("filler", list(FILLER))
def test_frame_matches_checker_under_every_filler_setting(oracle, monkeypatch, filler):
    """128 x 96, more than half of it sky, Hosek sky, 16 + 8 + 16 samples from a cleared state: layers and counts equal the checker's bit for bit, every sky sample
    is counted, and fh_sync reports no bounds-test violation (it would raise)."""
    r, L = _context(monkeypatch, FILLER[filler])
    cam = F.Camera(**CAM_FAR)
    r.reset_stats()
    for n in (16, 8, 16):
        r.render(cam, BG, L, n, DEPTH)
    got = _state(r, L)
    st = r.stats()
    L.free()
    r.close()
    sky_pixels, rem = divmod(st["sky_pixel_samples"], 40)
    print(f"{filler}: {sky_pixels} of {W * H} pixels are sky")
    assert rem == 0 and sky_pixels > W * H // 2 and st["paths"] == 40 * W * H
    _assert_same(got, _frame_reference(oracle), filler)


# ------------------------------------------------------------------ sky pixels that carry AOV state
def _prefill():
    """AOV layers with -0.0 and NaN in single channels of single pixels (and an ordinary value), everything else +0"""
    f = {n: np.zeros((H, W) if n == "depth" else (H, W, 4), np.float32) for n in NAMES}
    neg0, nan = np.float32(-0.0), np.float32(np.nan)
    yy, xx = np.mgrid[0:H, 0:W]
    k = (yy * W + xx) % 29
    f["position"][..., 0][k == 1] = neg0
    f["position"][..., 2][k == 2] = nan
    f["normal"][..., 1][k == 3] = neg0
    f["normal"][..., 0][k == 4] = nan
    f["albedo"][..., 2][k == 5] = neg0
    f["albedo"][..., 1][k == 6] = nan
    f["depth"][k == 7] = neg0
    f["depth"][k == 8] = nan
    f["texcoord"][..., 0][k == 9] = neg0
    f["texcoord"][..., 1][k == 10] = nan
    f["texcoord"][..., 1][k == 11] = neg0
    f["position"][..., 1][k == 12] = np.float32(1.5)
    return f


def _aov_reference(oracle, case):
    key = "aov_" + case
    if key not in _CACHE:
        S = _checker(oracle)
        Lo = S.new_layers(W, H)
        if case == "rendered":
            for _ in range(4):  # (one sample per call, as in _frame_reference)
                S.render(F.Camera(**CAM_NEAR).params(), W, H, Lo, 1, DEPTH, bg=BG, n_threads=8)
        else:
            for n, a in _prefill().items():
                Lo[n][...] = a
        for _ in range(3 + 5):
            S.render(F.Camera(**CAM_TURNED).params(), W, H, Lo, 1, DEPTH, bg=BG, n_threads=8)
        _CACHE[key] = Lo
    return _CACHE[key]


@pytest.mark.parametrize("filler", ["off", "one_per_cu"])
@pytest.mark.parametrize("case", ["rendered", "prefilled"])
def test_sky_pixels_with_aov_state_match_checker(oracle, monkeypatch, case, filler):
    """`rendered`: 4 samples with a camera that sees the soup, then -- without init_render_states -- the camera turns and 8 more samples fall on pixels that are now sky
    and still hold the AOV means of the hits.  `prefilled`: the layers hold -0.0 and NaN in single channels before the first sample; the skip of all-+0 pixels must not
    apply to them (0 * -0 + 0 is +0, NaN stays NaN).  Both equal the checker doing the same."""
    r, L = _context(monkeypatch, FILLER[filler])
    r.reset_stats()
    if case == "rendered":
        r.render(F.Camera(**CAM_NEAR), BG, L, 4, DEPTH)
        r.wait_for_completion()
        hit = L.download("depth") != 0
        before = r.stats()["sky_pixel_samples"]
    else:
        for n, a in _prefill().items():
            L._bufs[n].upload(a)
        hit, before = None, 0
    for n in (3, 5):
        r.render(F.Camera(**CAM_TURNED), BG, L, n, DEPTH)
    got = _state(r, L)
    st = r.stats()
    L.free()
    r.close()
    assert st["sky_pixel_samples"] - before > 8 * W * H // 2  # the turned camera sees mostly sky ...
    if hit is not None:  # ... also where the first camera saw the soup
        n_hit = int(hit.sum())
        print(f"{n_hit} pixels carry AOV state")
        assert n_hit > 200
    _assert_same(got, _aov_reference(oracle, case), f"{case} / {filler}")


# ------------------------------------------------------------------ adaptive sampling: the per-pixel rule and guard blocks
@pytest.mark.parametrize("block", [1, 4])
def test_adaptive_results_do_not_depend_on_the_filler(monkeypatch, block):
    """the adaptive scene of test_gpu_adaptive_sampling.py (Hosek-sky soup, 64 x 48, sky split forced): the per-pixel rule (one sky launch pair per call) and guard
    blocks (one per round), filler off / one workgroup / one per CU: identical layers, counts, moments and `paths`."""
    w, h = 64, 48
    sc = scenes.triangle_soup(3000, 0.1)
    out = {}
    for filler, env in FILLER.items():
        r, L = _context(monkeypatch, env, w, h, sc)
        r.set_adaptive_policy(block, 1)
        r.set_adaptive_sampling(0.05, 16, 8)
        r.reset_stats()
        for n in (24, 40):
            r.render(F.Camera(**CAM_NEAR), BG, L, n, DEPTH)
        s = _state(r, L)
        s["moments"] = r.luminance_moments()
        st = r.stats()
        L.free()
        r.close()
        out[filler] = (s, st)
        print(f"block {block}, filler {filler}: paths {st['paths']}, sky-pixel samples {st['sky_pixel_samples']}, counts {s['sample_count'].min()}..{s['sample_count'].max()}")
    ref, ref_st = out["off"]
    assert ref_st["sky_pixel_samples"] > 0 and ref["sample_count"].min() < 64  # the sky split was active and some pixels stopped early
    for filler in ("one_workgroup", "one_per_cu"):
        s, st = out[filler]
        _assert_same(s, ref, f"block {block}: {filler} against off", NAMES + ("sample_count", "moments"))
        assert st["paths"] == ref_st["paths"] and st["sky_pixel_samples"] == ref_st["sky_pixel_samples"]
