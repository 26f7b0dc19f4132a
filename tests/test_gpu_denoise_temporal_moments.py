"""Tests of the temporal moments of the temporal stage (include/fredholm_hip.h: fh_set_denoise_temporal_moments; fredholm_amd/csrc/denoise.hip: k_temporal<., ., true>).
The restatement is tests/test_denoise_temporal_moments_host.py's: the response suite's look-up, clip and blend with the moments looked up like the colour, blended
with the same weights and, in a call without sample moments, their variance in place of the 7 x 7 estimate where the history is min_history long.  The device is held to
the float32 restatement's bits and to the temporal suite's bound against the float64 one (_compare: 4 x the float32 restatement's own distance), and to bits wherever the
header promises bits.  The tests marked gpu need the device; that every 37 x 29 case holds pixels of every kind is checked on the CPU as well.

One thing the cases cannot hold: with the clip off and min_history 2 a pixel WITH a history always has h = min(h_h + 1, max_history) >= 2 (h_h >= 1: a stored length is 1
or more, and so is a weighted mean of them), so "a history shorter than min_history" does not exist there; those cases are asserted to have none, and the other two kinds.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import fredholm_amd as F
from fredholm_amd import native as N
from fredholm_amd import scenes
from fredholm_amd.renderer import DeviceBuffer

import test_denoise_temporal_moments_host as H
from test_denoise_temporal_moments_host import MIN_HISTORY, R
from test_gpu_denoise_response import M, T, SIZES, Dev, _bits, _compare, _hit, _relmse

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOKS = ("own", "reproject", "motion")
KAPPA = 6.0
# the pixels made misses in the second frame (B: no history in the third call, a history of 2 in the fourth) and in the third (A: no history in the fourth call)
BLOCKS = {"37x29": dict(A=(5, 10, 4, 9), B=(22, 28, 15, 21)), "5x3": dict(A=(1, 2, 1, 2), B=(3, 4, 1, 2))}


# ------------------------------------------------------------------ the cases
def _missed(layers, x0, x1, y0, y1):
    lay = {k: v.copy() for k, v in layers.items()}
    lay["normal"][y0:y1, x0:x1] = 0.0
    lay["position"][y0:y1, x0:x1] = 0.0
    return lay


def moments_case(size, look, seed=401):
    """[(camera, layers, ids, table)] of four consecutive calls: "own": a still camera; "reproject": cameras A, B, A, B (the step between the two planes leaves 2 x 2
    taps invalid in every call); "motion": A, B, A, B with the near plane an instance that turns a little further in every frame.  Every frame is lit anew (the response
    suite's _relit, with its NaN, its Inf and its counts of 0 and 1), block B is missed in the second frame and block A in the third"""
    w, h = SIZES[size]
    a, b = T._cameras(w, h, T.SHIFT[size])
    calls = []
    for k in range(4):
        cam = a if look == "own" or k % 2 == 0 else b
        ids = table = None
        if look == "motion":
            pivot = (-0.4, 0.0, T.NEAR)
            lay, ids, _ = M.planes_moved(w, h, cam, seed + k, *M.rot_y(0.12 * k, pivot))
            if k:
                prev, cur = M.affine(*M.rot_y(0.12 * (k - 1), pivot)), M.affine(*M.rot_y(0.12 * k, pivot))
                table = N.motion_from_transforms([M.IDENT, prev[0]], [M.IDENT, prev[1]], [M.IDENT, cur[0]], [M.IDENT, cur[1]])
        else:
            lay, _ = T._two_planes(w, h, cam, seed + k)
        lay = R._relit(lay, seed + 10 + k, k % 3)
        if k == 1:
            lay = _missed(lay, *BLOCKS[size]["B"])
        if k == 2:
            lay = _missed(lay, *BLOCKS[size]["A"])
        if ids is not None:
            ids = np.where(_hit(lay["normal"]), ids, M.MISS).astype(np.uint32)
        calls.append((cam, lay, ids, table))
    return calls


def _check_kinds(st, lay, gamma, min_history, what):
    long, short, none = H.kinds(st, lay["normal"])
    print(f"temporal moments {what}: h >= min_history: {long}, shorter history: {short}, no history: {none}")
    assert long > 0 and none > 0, (what, long, short, none)
    if gamma is None and min_history <= 2.0:
        assert short == 0, (what, short)  # (the module's docstring: h = h_h + 1 >= 2)
    else:
        assert short > 0, (what, long, short, none)


def test_cases_hold_pixels_of_every_kind(oracle):
    """no GPU: by the float32 restatement's own count, the last call of every 37 x 29 case of the restatement test has pixels whose history is min_history long, pixels
    with a shorter history (where one can exist) and hit pixels without a history; the motion cases carry; and the variance that replaces the spatial estimate differs"""
    for look in LOOKS:
        for gamma in (None, R.GAMMA):
            for min_history in (2.0, 4.0):
                st, off = H.moments_restatements(oracle, gamma, min_history)[1], H.moments_restatements(oracle, gamma, None)[1]
                for k, call in enumerate(moments_case("37x29", look)):
                    R._restate(st, call, use_moments=False, passes=1)
                    R._restate(off, call, use_moments=False, passes=1)
                    if k and look == "motion":
                        assert st.carried.any()
                _check_kinds(st, call[1], gamma, min_history, f"37x29 {look} gamma={gamma} min_history={min_history}")
                assert not _bits(st.hist["v"][st.long], off.hist["v"][st.long])


# ------------------------------------------------------------------ device side
class switched:
    """the context's switches for a block -- min_history (None: off), gamma (None: off), kappa (None: off) -- and all three off again after it: the session's renderer is
    shared with the other suites.  Entering with the moments switch on or leaving with it on drops the history"""

    def __init__(self, r, min_history, gamma=None, kappa=None):
        self.r, self.min_history, self.gamma, self.kappa = r, min_history, gamma, kappa

    def __enter__(self):
        r = self.r
        r.clear_denoise_response() if self.gamma is None else r.set_denoise_response(self.gamma)
        r.clear_denoise_response_noise() if self.kappa is None else r.set_denoise_response_noise(self.kappa)
        r.clear_denoise_temporal_moments() if self.min_history is None else r.set_denoise_temporal_moments(self.min_history)
        return r

    def __exit__(self, *exc):
        self.r.clear_denoise_response()
        self.r.clear_denoise_response_noise()
        self.r.set_denoise_temporal_moments(MIN_HISTORY)  # (the min_history a later get reports: back to the default)
        self.r.clear_denoise_temporal_moments()


def run_calls(r, calls, min_history, gamma=None, kappa=None, **kw):
    """the outputs of consecutive calls from an empty history under the given switches"""
    with switched(r, min_history, gamma, kappa):
        r.reset_denoise_history()
        return [R.dev_call(r, c, **kw) for c in calls]


# ------------------------------------------------------------------ 1: the first call
@gpu
@pytest.mark.parametrize("use_moments,upscale", [(True, False), (False, False), (True, True), (False, True)])
def test_first_call_with_the_switch_on_is_the_guided_filter(renderer, use_moments, upscale):
    cam = F.Camera(origin=(0.0, 0.0, 1.0))
    devs = {k: Dev(renderer, T._random_layers(*wh, seed)) for (k, wh), seed in zip(SIZES.items(), (5, 6))}
    try:
        with switched(renderer, MIN_HISTORY):
            want = {k: d.guided(use_moments, upscale) for k, d in devs.items()}
            assert renderer.denoise_history_info() == (0, 0, 0)
            assert _bits(devs["37x29"].temporal(cam, use_moments, upscale), want["37x29"])
            assert _bits(devs["5x3"].temporal(cam, use_moments, upscale), want["5x3"])  # a change of width x height drops the history
            assert renderer.denoise_history_info() == (5, 3, 1)
            renderer.reset_denoise_history()
            assert _bits(devs["5x3"].temporal(cam, use_moments, upscale), want["5x3"])
    finally:
        for d in devs.values():
            d.free()


# ------------------------------------------------------------------ 2, 3: the calls that keep the switched-off bits
@gpu
@pytest.mark.parametrize("gamma", [None, R.GAMMA])
@pytest.mark.parametrize("look", LOOKS)
def test_a_min_history_no_history_reaches_gives_the_switched_off_bits(renderer, look, gamma):
    """min_history 1e30, no sample moments: the moments are kept and never used, so all four calls have the bits of the context with the switch off"""
    calls = moments_case("37x29", look, seed=411)
    want = run_calls(renderer, calls, None, gamma, use_moments=False)
    got = run_calls(renderer, calls, 1e30, gamma, use_moments=False)
    assert all(_bits(x, y) for x, y in zip(want, got))
    assert not _bits(run_calls(renderer, calls, 2.0, gamma, use_moments=False)[3], want[3])  # (the switch does something)


@gpu
@pytest.mark.parametrize("gamma,kappa", [(None, None), (R.GAMMA, None), (R.GAMMA, KAPPA)])
@pytest.mark.parametrize("look", ["reproject", "motion"])
def test_calls_with_sample_moments_keep_the_switched_off_bits(renderer, look, gamma, kappa):
    """with moments and counts v is untouched, and the noise box (gamma 1, kappa 6) acts as it does with the switch off"""
    calls = moments_case("37x29", look, seed=421)
    want = run_calls(renderer, calls, None, gamma, kappa, use_moments=True)
    got = run_calls(renderer, calls, 2.0, gamma, kappa, use_moments=True)
    assert all(_bits(x, y) for x, y in zip(want, got))
    if kappa is not None:
        assert not _bits(want[3], run_calls(renderer, calls, None, gamma, None, use_moments=True)[3])  # (the noise box does something in these calls)


# ------------------------------------------------------------------ 4: the stage against the restatement
@gpu
@pytest.mark.parametrize("min_history", [2.0, 4.0])
@pytest.mark.parametrize("gamma", [None, R.GAMMA])
@pytest.mark.parametrize("look", LOOKS)
@pytest.mark.parametrize("size", list(SIZES))
def test_stage_with_moments_matches_the_restatement(renderer, oracle, size, look, gamma, min_history):
    """four consecutive calls without sample moments, so that blended moments are themselves looked up and blended again, through all three look-ups with the clip off and
    on.  The device must have the float32 restatement's bits and lie within the temporal suite's bound of the float64 one."""
    r64, r32 = H.moments_restatements(oracle, gamma, min_history)
    with switched(renderer, min_history, gamma):
        renderer.reset_denoise_history()
        for k, call in enumerate(moments_case(size, look)):
            got = R.dev_call(renderer, call, use_moments=False)
            o64, o32 = R._restate(r64, call, use_moments=False), R._restate(r32, call, use_moments=False)
            same = _compare(f"moments {size} {look} gamma={gamma} min_history={min_history} call {k + 1}", got, o64, o32)
            assert _bits(got, o32), (k, same)
        assert renderer.denoise_history_info() == SIZES[size] + (4,)
    if size == "37x29":
        _check_kinds(r32, call[1], gamma, min_history, f"{size} {look} gamma={gamma} min_history={min_history}")
        if look == "motion":
            assert r32.carried.any()


# ------------------------------------------------------------------ 5, 6: the switch and the history
@gpu
def test_turning_the_switch_on_or_off_drops_the_history_and_min_history_alone_does_not(renderer):
    calls = moments_case("37x29", "reproject", seed=431)
    d = Dev(renderer, calls[2][1])
    try:
        with switched(renderer, None):
            guided = d.guided(False)
            renderer.reset_denoise_history()
            outs = [R.dev_call(renderer, c, use_moments=False) for c in calls[:2]]
            assert renderer.denoise_history_info() == (37, 29, 2)
            renderer.set_denoise_temporal_moments(2.0)  # off -> on
            assert renderer.get_denoise_temporal_moments() == (True, 2.0) and renderer.denoise_history_info() == (0, 0, 0)
            assert _bits(R.dev_call(renderer, calls[2], use_moments=False), guided) and renderer.denoise_history_info() == (37, 29, 1)
            renderer.set_denoise_temporal_moments(3.0)  # min_history alone
            assert renderer.get_denoise_temporal_moments() == (True, 3.0) and renderer.denoise_history_info() == (37, 29, 1)
            assert not _bits(R.dev_call(renderer, calls[2], use_moments=False), guided) and renderer.denoise_history_info() == (37, 29, 2)
            renderer.clear_denoise_temporal_moments()  # on -> off
            assert renderer.get_denoise_temporal_moments() == (False, 3.0) and renderer.denoise_history_info() == (0, 0, 0)
            assert _bits(R.dev_call(renderer, calls[2], use_moments=False), guided) and renderer.denoise_history_info() == (37, 29, 1)
            renderer.clear_denoise_temporal_moments()  # off -> off: nothing
            assert renderer.denoise_history_info() == (37, 29, 1)
            # and what the sequence gives from here is what it gives with the switch never touched
            renderer.reset_denoise_history()
            assert all(_bits(x, R.dev_call(renderer, c, use_moments=False)) for x, c in zip(outs, calls[:2]))
    finally:
        d.free()


@gpu
def test_a_refused_setter_leaves_switch_history_and_output_alone(renderer):
    calls = moments_case("37x29", "reproject", seed=441)
    want = run_calls(renderer, calls, 3.0, use_moments=False)
    L, ctx = N.lib(), renderer._ctx
    with switched(renderer, 3.0):
        renderer.reset_denoise_history()
        outs = []
        for k, call in enumerate(calls):
            for bad in (float("nan"), float("inf"), 0.5, -1.0):
                assert L.fh_set_denoise_temporal_moments(ctx, C.byref(N.TemporalMomentsParamsC(bad))) == -1
                assert b"fh_set_denoise_temporal_moments" in L.fh_last_error(ctx) and b"min_history" in L.fh_last_error(ctx)
                assert renderer.get_denoise_temporal_moments() == (True, 3.0)
            assert renderer.denoise_history_info() == ((37, 29, k) if k else (0, 0, 0))
            outs.append(R.dev_call(renderer, call, use_moments=False))
        assert all(_bits(x, y) for x, y in zip(want, outs))
        renderer.clear_denoise_temporal_moments()
        R.dev_call(renderer, calls[0], use_moments=False)
        assert L.fh_set_denoise_temporal_moments(ctx, C.byref(N.TemporalMomentsParamsC(float("nan")))) == -1  # refused while off: still off, the history kept
        assert renderer.get_denoise_temporal_moments() == (False, 3.0) and renderer.denoise_history_info() == (37, 29, 1)
        on = C.c_int(7)
        assert L.fh_get_denoise_temporal_moments(ctx, C.byref(on), None) == 0 and on.value == 0


# ------------------------------------------------------------------ 7, 8: groups and neighbours
@gpu
@pytest.mark.parametrize("look", ["own", "reproject"])
def test_a_group_gives_the_plain_contexts_bits(renderer, look):
    calls = moments_case("37x29", look, seed=451)
    want = run_calls(renderer, calls, 2.0, use_moments=False)
    g = F.Renderer(devices=[0, 0])
    try:
        assert g.get_denoise_temporal_moments() == (False, MIN_HISTORY)
        assert all(_bits(x, y) for x, y in zip(want, run_calls(g, calls, 2.0, use_moments=False)))
        g.set_denoise_temporal_moments(6.0)
        assert g.get_denoise_temporal_moments() == (True, 6.0) and g.denoise_history_info() == (0, 0, 0)
        with pytest.raises(N.FredholmError, match="min_history"):
            g.set_denoise_temporal_moments(0.5)
        assert g.get_denoise_temporal_moments() == (True, 6.0)
    finally:
        g.close()


@gpu
def test_other_calls_keep_their_bits_beside_a_switched_on_context(renderer, oracle):
    """fh_denoise, fh_denoise_guided and switch-off temporal calls on the session's context, interleaved with switch-on calls on a second context"""
    calls = moments_case("37x29", "reproject", seed=461)
    d = Dev(renderer, calls[0][1])
    out = DeviceBuffer(renderer, d.w * d.h * 16)
    other = F.Renderer(0)

    def atrous():
        renderer.denoise(d.w, d.h, d.bufs["beauty"].ptr, d.bufs["normal"].ptr, d.bufs["albedo"].ptr, out.ptr)
        renderer.wait_for_completion()
        return out.download(np.float32, (d.h, d.w, 4))
    try:
        before = [atrous(), d.guided(True), d.guided(False, upscale=True)] + run_calls(renderer, calls, None, use_moments=False)
        other.set_denoise_temporal_moments(2.0)
        renderer.reset_denoise_history()
        after = []
        for call in calls:
            switched_on = R.dev_call(other, call, use_moments=False)
            after.append(R.dev_call(renderer, call, use_moments=False))
        assert not _bits(switched_on, after[-1]) and renderer.get_denoise_temporal_moments()[0] is False
        after = [atrous(), d.guided(True), d.guided(False, upscale=True)] + after
        assert all(_bits(x, y) for x, y in zip(before, after))
        lay = calls[0][1]
        assert _bits(before[0], oracle.denoise(lay["beauty"], lay["normal"], lay["albedo"]))
    finally:
        other.close()
        out.free()
        d.free()


# ------------------------------------------------------------------ 9: quality on the device
def replay_record():
    with open(os.path.join(ROOT, "profiles", "denoise_temporal_moments_replay.json")) as f:
        return json.loads(f.readline())


def device_sequence(cams, spp, min_history):
    """the frames rendered by fh_render -- frame k with `spp` one-sample calls and seed 1 + k from cams[k] -- and denoised at once by fh_denoise_temporal WITHOUT
    moments and counts, the clip off, the moments switch at min_history (None: off); the last frame's output"""
    q = T.QUALITY
    w, h = q["w"], q["h"]
    r = F.Renderer(0)
    try:
        r.load_scene(scenes.cornell_box())
        r.build_ias()
        r.set_resolution(w, h)
        L, out = F.RenderLayer(r, w, h), DeviceBuffer(r, 16 * w * h)
        if min_history is not None:
            r.set_denoise_temporal_moments(min_history)
        p = L.ptrs
        for k, cam in enumerate(cams):
            L.clear()
            r.init_render_states()
            r.seed = 1 + k
            for _ in range(spp):
                r.render(cam, (0.0, 0.0, 0.0), L, 1, q["depth"])
            r.denoise_temporal(w, h, p["beauty"], p["normal"], p["albedo"], out.ptr, p["position"], p["depth"], cam)
            r.wait_for_completion()
        assert r.denoise_history_info() == (w, h, len(cams))
        return out.download(np.float32, (h, w, 4))
    finally:
        r.close()


@gpu
@pytest.mark.parametrize("name", ["moving_16spp", "still_1spp"])
def test_quality_without_sample_moments(name):
    """Cornell box, 96 x 72, depth 5, 8 frames with seeds 1 .. 8, no sample moments, the clip off: the temporal suite's QUALITY sequence (16 spp, a moving camera) and a
    still camera at 1 spp, truths of 1024 spp.  With R the float64 replay's ratio of the sequence (profiles/denoise_temporal_moments_replay.json), the call with the
    switch on is at most (R + 1) / 2 x the call with it off -- the margin rule of the temporal and motion suites."""
    q = T.QUALITY
    assert (q["w"], q["h"], q["depth"], q["truth_spp"]) == tuple(R.RESPONSE_QUALITY[k] for k in ("w", "h", "depth", "truth_spp"))
    if name == "moving_16spp":
        cams, spp = [T.quality_camera(k) for k in range(q["frames"])], q["spp"]
        truth = R.device_truth(scenes.cornell_box(), cams[-1])
    else:
        cams, spp = [F.Camera(**scenes.CORNELL_CAMERA)] * 8, 1
        truth = R.truth_before()
    ratio = replay_record()["R"][name]
    off, on = _relmse(device_sequence(cams, spp, None), truth), _relmse(device_sequence(cams, spp, MIN_HISTORY), truth)
    print(f"temporal moments quality ({name}): spatial estimate {off:.5f}, temporal moments {on:.5f} ({on / off:.4f} x; replay {ratio:.4f}, asserted {(ratio + 1.0) / 2.0:.4f} x)")
    assert ratio < 1.0 and on <= (ratio + 1.0) / 2.0 * off, (name, on, off, ratio)
