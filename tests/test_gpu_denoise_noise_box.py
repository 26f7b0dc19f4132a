"""Tests of the noise box of the clipped temporal stage (include/fredholm_hip.h: fh_set_denoise_response_noise, step 4b; fredholm_amd/csrc/denoise.hip:
k_temporal<., kClipColourNoise>).  The restatement of test_denoise_noise_box_host.py -- the response suite's with step 4b -- in float64 and in float32; the device is held
to the suite's bound, 4 x the largest float32-versus-float64 difference of the same case, and to the float32 restatement's bits.  Where the header promises bits the
comparison is bit for bit.  The tests marked gpu need the device; that every case has pixels the noise box clips and pixels it leaves alone is checked on the CPU too.
Quality: the sequences of the response suite, with the replay's record (profiles/denoise_noise_box_replay.json) for the margins."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import fredholm_amd as F
from fredholm_amd import native as N
from fredholm_amd import scenes
from fredholm_amd.renderer import DeviceBuffer

import test_denoise_noise_box_host as H
import test_gpu_denoise_response as R
from test_denoise_noise_box_host import KAPPA
from test_gpu_denoise_response import GAMMA, KINDS, M, T, _restate, dev_call, response_case
from test_gpu_denoise_temporal import SIZES, Dev, _bits, _compare, _relmse

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class switched:
    """the context's two switches for a block -- gamma None: the response switch off, kappa None: the noise switch off -- and both off again after it: the session's
    renderer is shared with the other suites"""

    def __init__(self, r, gamma, kappa):
        self.r, self.gamma, self.kappa = r, gamma, kappa

    def __enter__(self):
        if self.gamma is None:
            self.r.clear_denoise_response()
        else:
            self.r.set_denoise_response(self.gamma)
        if self.kappa is None:
            self.r.clear_denoise_response_noise()
        else:
            self.r.set_denoise_response_noise(self.kappa)
        return self.r

    def __exit__(self, *exc):
        self.r.clear_denoise_response()
        self.r.clear_denoise_response_noise()


def run_calls(r, calls, gamma, kappa, **kw):
    """the outputs of consecutive calls from an empty history, the switches at (gamma, kappa)"""
    with switched(r, gamma, kappa):
        r.reset_denoise_history()
        return [dev_call(r, c, **kw) for c in calls]


def test_cases_have_pixels_the_noise_box_clips_and_pixels_it_leaves_alone(oracle):
    """no GPU: by the float32 restatement's own count, every case of the restatement test has, over its second and third call, pixels with a history whose noise
    excess w is > 0 and pixels where it is 0, and among the former pixels where the noise box's excess is the larger of the two and so decides u"""
    for size in SIZES:
        for kind in KINDS:
            st = H.noise_restatements(oracle, GAMMA, KAPPA)[1]
            total = np.zeros(4, int)
            for call in response_case(size, kind):
                _restate(st, call, passes=1)
                if st.w is not None:
                    total += H.noise_counts(st) + (int((st.w[st.have] > st.u_s[st.have]).sum()), int((st.u_s[st.have] > st.w[st.have]).sum()))
            print(f"noise box case {size} {kind}: w > 0: {total[0]}, w = 0: {total[1]}, w > u_s: {total[2]}, u_s > w: {total[3]}")
            assert (total[:3] > 0).all(), (size, kind, total)


# ------------------------------------------------------------------ 1: the stage against the restatement
@gpu
@pytest.mark.parametrize("upscale", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", list(SIZES))
def test_noise_box_stage_matches_the_restatement(renderer, oracle, size, kind, upscale):
    """three consecutive calls with moments, so that a history the noise box clamped is itself looked up (and clamped) again.  The device must lie within 4 x the
    float32 restatement's own distance from the float64 one (_compare) and have the float32 restatement's bits.
    Observed on an MI355X: ratio 1.000 and every value bit-identical in all 48 comparisons; float32 error 2.2e-7 ... 2.9e-6."""
    r64, r32 = H.noise_restatements(oracle, GAMMA, KAPPA)
    total = np.zeros(2, int)
    with switched(renderer, GAMMA, KAPPA):
        renderer.reset_denoise_history()
        for k, call in enumerate(response_case(size, kind)):
            got = dev_call(renderer, call, upscale=upscale)
            o64, o32 = _restate(r64, call, upscale=upscale), _restate(r32, call, upscale=upscale)
            same = _compare(f"noise box {size} {kind} up={upscale} call {k + 1}", got, o64, o32)
            assert _bits(got, o32), (k, same)
            total += H.noise_counts(r32)
        assert renderer.denoise_history_info() == SIZES[size] + (3,)
    assert (total > 0).all(), total  # (w > 0, w = 0: a case in which the noise box clips nothing, or everything, proves nothing)


@gpu
@pytest.mark.parametrize("size", list(SIZES))
def test_a_window_of_the_pixel_alone_still_meets_the_noise_box(renderer, oracle, size):
    """step 3 with step 4b on the device: the second frame's radiance (and moments) x 8, so that the pixel the response suite leaves alone in its window -- n = 1,
    cc = c_h, u_s = 0 -- has a history outside its noise box: w > 0 there by the float32 restatement (asserted), and the device has that restatement's bits"""
    calls = response_case(size, "still", seed=481)[:2]
    cam, lay, ids, table = calls[1]
    calls[1] = (cam, dict(lay, beauty=lay["beauty"] * np.float32(8), moments=lay["moments"] * np.asarray([8, 64], np.float32)), ids, table)
    r32 = H.noise_restatements(oracle, GAMMA, KAPPA)[1]
    want = [_restate(r32, c) for c in calls]
    x, y = R.ALONE[size][1]
    assert r32.have[y, x] and r32.n[y, x] == 1 and r32.u_s[y, x] == 0 and r32.w[y, x] > 0 and r32.u[y, x] == r32.w[y, x]
    got = run_calls(renderer, calls, GAMMA, KAPPA)
    assert _bits(got[0], want[0]) and _bits(got[1], want[1])
    assert not _bits(got[1], run_calls(renderer, calls, GAMMA, None)[1])


# ------------------------------------------------------------------ 2: identities, bit for bit
@gpu
def test_set_then_cleared_is_the_response_call(renderer):
    calls = response_case("37x29", "moved", seed=401) + response_case("37x29", "still", seed=402)[2:]
    want = run_calls(renderer, calls, GAMMA, None)
    with switched(renderer, GAMMA, None):
        renderer.set_denoise_response_noise(4.5)
        assert renderer.get_denoise_response_noise() == (True, 4.5)
        renderer.clear_denoise_response_noise()
        assert renderer.get_denoise_response_noise() == (False, 4.5)
        renderer.reset_denoise_history()
        got = [dev_call(renderer, c) for c in calls]
    assert all(_bits(x, y) for x, y in zip(want, got))
    on = run_calls(renderer, calls, GAMMA, KAPPA)
    assert _bits(on[0], want[0]) and not _bits(on[1], want[1]) and not _bits(on[3], want[3])  # (the switch does something, in the moved and in the still kernel)
    renderer.set_denoise_response_noise(KAPPA)  # (the kappa a later get reports: back to the default)
    renderer.clear_denoise_response_noise()


@gpu
def test_a_huge_kappa_clips_nothing_and_gives_the_response_call(renderer, oracle):
    """kappa = 1e30: s is 1e30 standard deviations (or + infinity), the float32 restatement reports no pixel with w > 0 (asserted first; every pixel of these frames
    has v + v_h > 0), so cd = cc, u = u_s, and every pixel has the response call's bits in the still, the moved and the motion kernel"""
    calls = response_case("37x29", "moved", seed=411) + response_case("37x29", "still", seed=412)[2:] + response_case("37x29", "carried-still", seed=413)[2:]
    r32 = H.noise_restatements(oracle, GAMMA, 1e30)[1]
    clipped = []
    for call in calls:
        _restate(r32, call, passes=1)
        if r32.w is not None:
            assert r32.have.any()
            clipped.append(int((r32.w[r32.have] > 0).sum()))
    assert clipped == [0, 0, 0, 0], clipped
    want = run_calls(renderer, calls, GAMMA, None)
    got = run_calls(renderer, calls, GAMMA, 1e30)
    assert all(_bits(x, y) for x, y in zip(want, got))


@gpu
@pytest.mark.parametrize("upscale", [False, True])
def test_a_call_without_moments_is_the_response_call(renderer, upscale):
    calls = response_case("37x29", "moved", seed=421) + response_case("37x29", "carried-still", seed=422)[2:]
    want = run_calls(renderer, calls, GAMMA, None, use_moments=False, upscale=upscale)
    got = run_calls(renderer, calls, GAMMA, KAPPA, use_moments=False, upscale=upscale)
    assert all(_bits(x, y) for x, y in zip(want, got))


@gpu
def test_noise_on_with_response_off_is_the_plain_call(renderer):
    calls = response_case("37x29", "moved", seed=431) + response_case("37x29", "carried-still", seed=432)[2:]
    want = run_calls(renderer, calls, None, None)
    got = run_calls(renderer, calls, None, KAPPA)
    assert all(_bits(x, y) for x, y in zip(want, got))
    assert not _bits(run_calls(renderer, calls, GAMMA, KAPPA)[1], want[1])


@gpu
@pytest.mark.parametrize("upscale", [False, True])
def test_first_call_with_both_switches_on_is_the_guided_filter(renderer, upscale):
    cam = F.Camera(origin=(0.0, 0.0, 1.0))
    devs = {k: Dev(renderer, T._random_layers(*wh, seed)) for (k, wh), seed in zip(SIZES.items(), (7, 8))}
    try:
        with switched(renderer, GAMMA, KAPPA):
            renderer.reset_denoise_history()
            want = {k: d.guided(True, upscale) for k, d in devs.items()}
            assert _bits(devs["37x29"].temporal(cam, True, upscale), want["37x29"])
            assert _bits(devs["5x3"].temporal(cam, True, upscale), want["5x3"])  # a change of width x height drops the history
            assert not _bits(devs["5x3"].temporal(cam, True, upscale, temporal=dict(normal_cos_min=0.5, plane_tol=0.5)), want["5x3"])  # (now there is one)
            renderer.reset_denoise_history()
            assert _bits(devs["5x3"].temporal(cam, True, upscale), want["5x3"])
    finally:
        for d in devs.values():
            d.free()


@gpu
def test_identity_maps_under_a_moved_camera_give_the_plain_table_call(renderer):
    """the motion form of the noise kernel with every pixel carried by identity maps must equal its moved-camera form: both go through the one look-up, td_reproject,
    with a carried (P, N) that has the pixel's own bits"""
    frames = T._abc("37x29", 441)
    table = (N.MotionC * 1)()
    for k in range(12):
        table[0].point[k] = float(M.IDENT[k])
    for k in range(9):
        table[0].normal[k] = 1.0 if k % 4 == 0 else 0.0
    table[0].moved = 1
    ids = np.zeros((29, 37), np.uint32)
    want = run_calls(renderer, [(c, l, None, None) for c, l in frames], GAMMA, KAPPA)
    got = run_calls(renderer, [(c, l, ids, table) for c, l in frames], GAMMA, KAPPA)
    assert all(_bits(x, y) for x, y in zip(want, got))
    assert not _bits(want[1], run_calls(renderer, [(c, l, None, None) for c, l in frames], GAMMA, None)[1])


@gpu
def test_a_group_gives_the_plain_contexts_bits(renderer):
    calls = response_case("37x29", "moved", seed=451) + response_case("37x29", "still", seed=452)[2:]
    want = run_calls(renderer, calls, GAMMA, KAPPA)
    g = F.Renderer(devices=[0, 0])
    try:
        assert g.get_denoise_response_noise() == (False, KAPPA)
        assert all(_bits(x, y) for x, y in zip(want, run_calls(g, calls, GAMMA, KAPPA)))
        g.set_denoise_response_noise(3.0)
        assert g.get_denoise_response_noise() == (True, 3.0) and g.get_denoise_response() == (False, GAMMA)
        with pytest.raises(N.FredholmError, match="kappa"):
            g.set_denoise_response_noise(0.0)
        assert g.get_denoise_response_noise() == (True, 3.0)
        assert g.denoise_history_info() == (37, 29, 4)
    finally:
        g.close()


@gpu
def test_other_calls_keep_their_bits_beside_a_switched_on_context(renderer, oracle):
    """fh_denoise, fh_denoise_guided and plain temporal calls on the session's context, interleaved with calls on a second context that has both switches on"""
    frames = [(cam, lay, None, None) for cam, lay in T._abc("37x29", 461)]
    d = Dev(renderer, frames[0][1])
    out = DeviceBuffer(renderer, d.w * d.h * 16)
    other = F.Renderer(0)

    def atrous():
        renderer.denoise(d.w, d.h, d.bufs["beauty"].ptr, d.bufs["normal"].ptr, d.bufs["albedo"].ptr, out.ptr)
        renderer.wait_for_completion()
        return out.download(np.float32, (d.h, d.w, 4))
    try:
        before = [atrous(), d.guided(True), d.guided(False, upscale=True)] + run_calls(renderer, frames, None, None)
        other.set_denoise_response(GAMMA)
        other.set_denoise_response_noise(KAPPA)
        other.reset_denoise_history()
        renderer.reset_denoise_history()
        after = []
        for call in frames:
            switched_on = dev_call(other, call)
            after.append(dev_call(renderer, call))
        assert not _bits(switched_on, after[-1])
        after = [atrous(), d.guided(True), d.guided(False, upscale=True)] + after
        assert all(_bits(x, y) for x, y in zip(before, after))
        lay = frames[0][1]
        assert _bits(before[0], oracle.denoise(lay["beauty"], lay["normal"], lay["albedo"]))
    finally:
        other.close()
        out.free()
        d.free()


# ------------------------------------------------------------------ 3: refusals
@gpu
def test_a_bad_kappa_leaves_switch_history_and_output_alone(renderer):
    calls = response_case("37x29", "moved", seed=471)
    want = run_calls(renderer, calls, GAMMA, 4.5)
    L, ctx = N.lib(), renderer._ctx
    try:
        renderer.reset_denoise_history()
        renderer.set_denoise_response(GAMMA)
        renderer.set_denoise_response_noise(4.5)
        outs = []
        for k, call in enumerate(calls):
            for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
                assert L.fh_set_denoise_response_noise(ctx, C.byref(N.ResponseNoiseParamsC(bad))) == -1
                assert b"fh_set_denoise_response_noise" in L.fh_last_error(ctx) and b"kappa" in L.fh_last_error(ctx)
                assert renderer.get_denoise_response_noise() == (True, 4.5) and renderer.get_denoise_response() == (True, GAMMA)
            assert renderer.denoise_history_info() == ((37, 29, k) if k else (0, 0, 0))
            outs.append(dev_call(renderer, call))
        assert all(_bits(x, y) for x, y in zip(want, outs))
        renderer.clear_denoise_response_noise()
        assert L.fh_set_denoise_response_noise(ctx, C.byref(N.ResponseNoiseParamsC(float("nan")))) == -1
        assert renderer.get_denoise_response_noise() == (False, 4.5)
        on = C.c_int(7)
        assert L.fh_get_denoise_response_noise(ctx, C.byref(on), None) == 0 and on.value == 0
    finally:
        renderer.clear_denoise_response()
        renderer.set_denoise_response_noise(KAPPA)  # (the kappa a later get reports: back to the default)
        renderer.clear_denoise_response_noise()


# ------------------------------------------------------------------ 4: quality on the device
def replay_record():
    with open(os.path.join(ROOT, "profiles", "denoise_noise_box_replay.json")) as f:
        return json.loads(f.readline())


def replay_relmse(rec, tag, call, frame, field="relmse"):
    return {f["frame"]: f[field] for f in rec["sequences"][tag][call]}[frame]


def device_sequence(plan, gamma, kappa, score_from, with_guided=False, motion=False):
    """the response suite's device_sequence with the second switch and, motion, the moving-block sequence: plan = [(scene or None, camera, transforms or None)] per
    frame -- a scene is loaded (load_scene + build_ias) before that frame is rendered, transforms are set (set_transforms + build_ias) with fh_set_denoise_motion on,
    so that fh_denoise_temporal carries the block itself.  16 one-sample calls per frame with seed 1 + k, denoised at once with moments on the same context.
    Returns the outputs of the frames from `score_from` on (1-based), fh_denoise_guided's of the same layers (with_guided), and the last frame's id plane (motion)."""
    q = R.RESPONSE_QUALITY
    w, h = q["w"], q["h"]
    r = F.Renderer(0)
    outs, guided, ids = {}, {}, None
    try:
        L = None
        for k, (scene, cam, transforms) in enumerate(plan):
            if scene is not None:
                r.load_scene(scene)
                r.build_ias()
                if L is None:
                    r.set_resolution(w, h)
                    L = F.RenderLayer(r, w, h)
                    moments, counts, out = DeviceBuffer(r, 8 * w * h), DeviceBuffer(r, 4 * w * h), DeviceBuffer(r, 16 * w * h)
                    if gamma is not None:
                        r.set_denoise_response(gamma)
                    if kappa is not None:
                        r.set_denoise_response_noise(kappa)
                    if motion:
                        r.set_denoise_motion(True)
                    r.reset_denoise_history()
            if transforms is not None:
                r.set_transforms(*transforms)
                r.build_ias()
            r.set_adaptive_sampling(0.0)  # (threshold 0: the moments exist and nothing stops)
            R._render_frame(r, L, cam, 1 + k, q["spp"], q["depth"], moments, counts)
            p = L.ptrs
            r.denoise_temporal(w, h, p["beauty"], p["normal"], p["albedo"], out.ptr, p["position"], p["depth"], cam, moments.ptr, counts.ptr)
            r.wait_for_completion()
            if k + 1 >= score_from:
                outs[k + 1] = out.download(np.float32, (h, w, 4))
                if with_guided:
                    r.denoise_guided(w, h, p["beauty"], p["normal"], p["albedo"], out.ptr, p["position"], p["depth"], moments.ptr, counts.ptr)
                    r.wait_for_completion()
                    guided[k + 1] = out.download(np.float32, (h, w, 4))
        assert r.denoise_history_info() == (w, h, len(plan))
        if motion:
            idb = DeviceBuffer(r, 4 * w * h)
            r.primary_instances(plan[-1][1], w, h, idb.ptr)
            r.wait_for_completion()
            ids = idb.download(np.uint32, (h, w))
    finally:
        r.close()
    return outs, guided, ids


@gpu
@pytest.mark.parametrize("tag", ["L", "S"])
def test_quality_after_a_change_of_lighting(tag):
    """the response suite's sequences: Cornell box, 96 x 72, depth 5, 16 spp per frame with seeds 1 + k, a still camera, 8 frames, then the light's emission x 0.25
    (L) or the light quad moved by + 0.5 in x (S), then 4 more; truths of 1024 spp.  gamma = 1 and the default kappa.
    (S): first the premise -- the clipped call's frame 9 is more than 5 x the guided filter's (replay: 12 x) -- then the noise box at frames 9 and 12 is at most
    (rho + 1) / 2 x the clipped call, rho the replay's ratio of that frame (0.155 and 0.238).
    (L): the noise box at frames 9 and 12 is at most 1.05 x the clipped call (replay: 0.96 x), and at frame 8 -- nothing has changed yet -- at most 1.05 x the plain call.
    Replay (float64, checker-rendered frames), guided / clipped / noise box at frames 9 and 12:
      (L) 0.00651 / 0.02774 / 0.02662;  0.00655 / 0.00820 / 0.00779      (S) 0.03113 / 0.38772 / 0.05994;  0.03393 / 0.10950 / 0.02609
    Observed on an MI355X: the same figures to the digits shown (the device renders the checker's samples); (L) frame 8 plain 0.01510, noise box 0.01439 (0.953 x)."""
    q = R.RESPONSE_QUALITY
    cam = F.Camera(**scenes.CORNELL_CAMERA)
    nb, na = q["frames_before"], q["frames_after"]
    plan = [(scenes.cornell_box() if k == 0 else R.changed_scene(tag) if k == nb else None, cam, None) for k in range(nb + na)]
    clipped, guided, _ = device_sequence(plan, GAMMA, None, nb, with_guided=True)
    noise, _, _ = device_sequence(plan, GAMMA, KAPPA, nb)
    after = R.device_truth(R.changed_scene(tag), cam)
    rec = replay_record()
    err = {}
    for k in sorted(clipped):
        t = R.truth_before() if k <= nb else after
        err[k] = (_relmse(guided[k], t), _relmse(clipped[k], t), _relmse(noise[k], t))
        rho = replay_relmse(rec, tag, f"kappa={KAPPA}", k) / replay_relmse(rec, tag, "clipped", k)
        print(f"noise box quality ({tag}) frame {k}: guided {err[k][0]:.5f}, clipped {err[k][1]:.5f}, noise box {err[k][2]:.5f} ({err[k][2] / err[k][1]:.4f} x clipped; replay rho {rho:.4f})")
    if tag == "S":
        assert err[nb + 1][1] > 5.0 * err[nb + 1][0], err[nb + 1]
        for k in (nb + 1, nb + na):
            rho = replay_relmse(rec, tag, f"kappa={KAPPA}", k) / replay_relmse(rec, tag, "clipped", k)
            assert err[k][2] <= (rho + 1.0) / 2.0 * err[k][1], (k, err[k])
    else:
        for k in (nb + 1, nb + na):
            assert err[k][2] <= 1.05 * err[k][1], (k, err[k])
        plain, _, _ = device_sequence(plan[:nb], None, None, nb)
        ep = _relmse(plain[nb], R.truth_before())
        print(f"noise box quality (L) frame {nb}: plain temporal {ep:.5f}, noise box {err[nb][2]:.5f} ({err[nb][2] / ep:.4f} x)")
        assert err[nb][2] <= 1.05 * ep, (err[nb], ep)


@gpu
def test_quality_of_the_steady_moving_camera_sequence_is_kept():
    """(M), the temporal suite's QUALITY sequence (a moving camera, nothing else changes): the noise box's last frame is at most 1.05 x the plain call's (replay: 0.886 x).
    Observed on an MI355X: plain 0.01445, noise box 0.01279 (0.886 x)."""
    q = T.QUALITY
    plan = [(scenes.cornell_box() if k == 0 else None, T.quality_camera(k), None) for k in range(q["frames"])]
    plain, _, _ = device_sequence(plan, None, None, q["frames"])
    noise, _, _ = device_sequence(plan, GAMMA, KAPPA, q["frames"])
    truth = R.device_truth(scenes.cornell_box(), T.quality_camera(q["frames"] - 1))
    ep, en = _relmse(plain[q["frames"]], truth), _relmse(noise[q["frames"]], truth)
    print(f"noise box quality (M) frame {q['frames']}: plain temporal {ep:.5f}, noise box {en:.5f} ({en / ep:.4f} x)")
    assert en <= 1.05 * ep, (en, ep)


@gpu
def test_quality_of_the_steady_moving_block_sequence_is_kept():
    """(B), the motion suite's MOTION_QUALITY sequence (a still camera, the short block moving 0.05 per frame, carried by fh_set_denoise_motion): over the last frame
    and over the block's own pixels -- dim, indirectly lit, heavy-tailed: the constraint that binds kappa -- the noise box is at most 1.05 x the motion call without
    clipping (replay: 0.672 x and 1.038 x).
    Observed on an MI355X: frame 0.02533 -> 0.01701 (0.672 x), the block's 282 pixels 0.00482 -> 0.00501 (1.038 x)."""
    q = M.MOTION_QUALITY
    assert (q["w"], q["h"], q["spp"], q["depth"], q["truth_spp"]) == tuple(R.RESPONSE_QUALITY[k] for k in ("w", "h", "spp", "depth", "truth_spp"))
    cam = F.Camera(**scenes.CORNELL_CAMERA)
    plan = [(scenes.cornell_box_instanced() if k == 0 else None, cam, scenes.instanced_transforms(M.motion_quality_offset(k))) for k in range(q["frames"])]
    plain, _, ids = device_sequence(plan, None, None, q["frames"], motion=True)
    noise, _, _ = device_sequence(plan, GAMMA, KAPPA, q["frames"], motion=True)
    r = F.Renderer(0)
    try:
        r.load_scene(scenes.cornell_box_instanced())
        r.build_ias()
        r.set_transforms(*scenes.instanced_transforms(M.motion_quality_offset(q["frames"] - 1)))
        r.build_ias()
        r.set_resolution(q["w"], q["h"])
        truth = R._truth(r, F.RenderLayer(r, q["w"], q["h"]), cam, q["truth_spp"], q["depth"])
    finally:
        r.close()
    box = ids == 1
    n = q["frames"]
    fp, fn = _relmse(plain[n], truth), _relmse(noise[n], truth)
    bp, bn = _relmse(plain[n][box][None], truth[box][None]), _relmse(noise[n][box][None], truth[box][None])
    print(f"noise box quality (B) frame {n}: plain motion {fp:.5f}, noise box {fn:.5f} ({fn / fp:.4f} x); the block's {int(box.sum())} pixels: {bp:.5f}, {bn:.5f} ({bn / bp:.4f} x)")
    assert box.sum() > 200
    assert fn <= 1.05 * fp, (fn, fp)
    assert bn <= 1.05 * bp, (bn, bp)
