"""Auto-exposure of the post chain on the device (include/fredholm_hip.h: fh_set_auto_exposure ... fh_get_luminance_histogram; post.hip: k_meter_histogram,
k_meter_resolve, k_tone_map_metered, k_bloom_threshold_metered) against the numpy restatement of the header's arithmetic below, which
tests/test_auto_exposure_host.py pins, bit for bit, to csrc/fh_meter.h compiled for the host.  The restatement takes its log2, exp and pow from the checker
(oracle.elementary); the rank cuts and the sum S are numpy float64 in the header's order.  The histogram is compared as integers, the state as bits.

The float64 restatement (resolve64) runs the same resolve on the same integer histogram with every float in double.  STATE_BOUND, its distance from the float32 one,
is measured on the pair on the CPU (test_auto_exposure_host.py::test_the_float32_and_float64_restatements_agree_within_the_bound asserts it on the sequences used here).
Source of the bound: per metering call the float32 resolve rounds eight times (bin centre: /, +; mean: one conversion; target: -, +; ev: -, *, +) at magnitudes below
32, half an ulp of which is 1.9e-6; the smoothing passes a share 1 - a <= 1 of the earlier error on, so after k calls the distance is at most 8 * 1.9e-6 * k.  For
the six calls of the sequence: 9.2e-5.  Measured on the pair: 3.7e-7 at the most."""
import ctypes as C
import math

import numpy as np
import pytest

f32 = np.float32
DEFAULTS = dict(key=0.18, compensation_ev=0.0, min_ev=-16.0, max_ev=16.0, low=0.10, high=0.90, speed_up=3.0, speed_down=1.0, frame_time=1.0 / 30.0, log2_lo=-16.0,
                log2_hi=16.0)
STATE_BOUND = 8 * 1.9e-6 * 6


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ the restatement
def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def histogram(oracle, img, p):
    """the 257 counts of an image (any shape ending in 4 channels): the header's metering in float32, one rounding per operation"""
    px = np.ascontiguousarray(img, dtype=np.float32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        r, g, b = (np.where(np.isnan(px[:, k]) | (np.abs(px[:, k]) > f32(3.0e38)), f32(0), px[:, k]) for k in range(3))
        l = (r * f32(0.2126729) + g * f32(0.7151522)) + b * f32(0.0721750)
        metered = l > 0
        scale = f32(256.0) / (f32(p["log2_hi"]) - f32(p["log2_lo"]))
        t = np.floor((oracle.elementary("log2", np.where(metered, l, f32(1))) - f32(p["log2_lo"])) * scale)
    bins = np.where(metered, np.clip(t, 0, 255), 256).astype(np.int64)
    return np.bincount(bins, minlength=257).astype(np.uint32)


def consts(oracle, p):
    """what the host hands the resolve: scale, log2key, a_up, a_down (float32)"""
    scale = f32(256.0) / (f32(p["log2_hi"]) - f32(p["log2_lo"]))
    log2key = oracle.elementary("log2", [p["key"]])[0]
    if math.isinf(p["frame_time"]):
        a_up = a_down = f32(1)
    else:
        a_up, a_down = (f32(1) - oracle.elementary("exp", [-f32(p["frame_time"]) * f32(s)])[0] for s in (p["speed_up"], p["speed_down"]))
    return scale, log2key, a_up, a_down


def rank_cuts(n, low, high):
    cut, end = int(np.float64(n) * np.float64(f32(low))), int(np.float64(n) * np.float64(f32(high)))
    if end <= cut:
        end = min(cut + 1, n)
        cut = end - 1
    return cut, end


def kept_counts(hist, cut, end):
    c1 = np.cumsum(hist[:256].astype(np.int64))
    c0 = c1 - hist[:256]
    return np.maximum(0, np.minimum(c1, end) - np.maximum(c0, cut))


def resolve(oracle, hist, p, state):
    """one resolve in float32 (S and the cuts in float64): state is None before any, or the dict this returns.  Unchanged when nothing was metered"""
    n = int(hist[:256].astype(np.int64).sum())
    state = dict(state) if state else dict(ev=f32(0), target_ev=f32(0), mean_log2=f32(0), metered=0, unmetered=0, frames=0)
    if n == 0:
        return state
    scale, log2key, a_up, a_down = consts(oracle, p)
    cut, end = rank_cuts(n, p["low"], p["high"])
    kept = kept_counts(hist, cut, end)
    centre = (np.arange(256, dtype=np.float32) + f32(0.5)) / scale + f32(p["log2_lo"])
    s = np.float64(0)
    for b in range(256):
        s = s + np.float64(kept[b]) * np.float64(centre[b])
    mean = f32(s / np.float64(end - cut))
    target = np.fmax(f32(p["min_ev"]), np.fmin((log2key - mean) + f32(p["compensation_ev"]), f32(p["max_ev"])))
    if state["frames"] == 0:
        ev = target
    else:
        a = a_up if target > state["ev"] else a_down
        ev = state["ev"] + (target - state["ev"]) * a
    return dict(ev=f32(ev), target_ev=f32(target), mean_log2=mean, metered=n, unmetered=int(hist[256]), frames=state["frames"] + 1)


def resolve64(hist, p, state):
    """the same resolve with every float a double and numpy's log2 / exp"""
    n = int(hist[:256].astype(np.int64).sum())
    state = dict(state) if state else dict(ev=0.0, target_ev=0.0, mean_log2=0.0, metered=0, unmetered=0, frames=0)
    if n == 0:
        return state
    scale = 256.0 / (p["log2_hi"] - p["log2_lo"])
    cut, end = rank_cuts(n, p["low"], p["high"])
    kept = kept_counts(hist, cut, end)
    centre = (np.arange(256, dtype=np.float64) + 0.5) / scale + p["log2_lo"]
    mean = float((kept * centre).sum() / (end - cut))
    target = max(p["min_ev"], min(math.log2(p["key"]) - mean + p["compensation_ev"], p["max_ev"]))
    if state["frames"] == 0:
        ev = target
    else:
        speed = p["speed_up"] if target > state["ev"] else p["speed_down"]
        a = 1.0 if math.isinf(p["frame_time"]) else 1.0 - math.exp(-p["frame_time"] * speed)
        ev = state["ev"] + (target - state["ev"]) * a
    return dict(ev=ev, target_ev=target, mean_log2=mean, metered=n, unmetered=int(hist[256]), frames=state["frames"] + 1)


def exposure_of(oracle, ev):
    return oracle.elementary("pow", [2.0], [ev])[0]


# ------------------------------------------------------------------ images
SIZES = [(1, 1), (3, 5), (16, 16), (67, 35), (256, 1), (257, 1), (1024, 640)]
SPECIALS = [np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0, 1e-45, 1e-40, -1e-40, 3.2e38, -3.2e38, 3.0e38]


def image(kind, w, h, seed=0, level=1.0):
    """"mixed": log-uniform luminances over 2^-20 .. 2^20 with tinted colours, every 7th pixel an exact grey power of two, every 5th with one channel special (NaN,
    +-inf, negative, +-0, denormal, beyond 3e38); "noise": log-uniform over 2^-2 .. 2^2 times level; "constant"; "black": nothing metered (zeros, negatives, NaN)"""
    rng = np.random.default_rng(1000 * w + h + seed)
    n = w * h
    if kind == "constant":
        img = np.tile(np.array([0.8, 0.5, 0.3, 1.0], np.float32) * f32(level), (n, 1))
    elif kind == "black":
        img = np.zeros((n, 4), np.float32)
        img[1::3, :3] = -1.0
        img[2::3, 0] = np.nan
    else:
        span = 20.0 if kind == "mixed" else 2.0
        lum = np.exp2(rng.uniform(-span, span, n)) * level
        img = np.ones((n, 4), np.float32)
        img[:, :3] = (lum[:, None] * rng.uniform(0.2, 1.8, (n, 3))).astype(np.float32)
        if kind == "mixed":
            k = rng.integers(-30, 31, n)
            img[::7, :3] = np.exp2(k[::7]).astype(np.float32)[:, None]
            idx = np.arange(0, n, 5)
            img[idx, rng.integers(0, 3, idx.size)] = np.array(SPECIALS, np.float32)[rng.integers(0, len(SPECIALS), idx.size)]
    return img.reshape(h, w, 4)


# ------------------------------------------------------------------ device plumbing
@pytest.fixture()
def ae(renderer):
    """the session's renderer, handed back with the switch off"""
    yield renderer
    renderer.clear_auto_exposure()


def _upload(r, img):
    from fredholm_amd.renderer import DeviceBuffer
    b = DeviceBuffer(r, img.nbytes)
    b.upload(img)
    return b


def _same_state(got, want):
    return (all(_bits(got[k]).tolist() == _bits(want[k]).tolist() for k in ("ev", "target_ev", "mean_log2"))
            and all(int(got[k]) == int(want[k]) for k in ("metered", "unmetered", "frames")))


def _post(r, img, pp, bufs=None):
    """fh_post_process on cleared buffers: the output, never-written border included"""
    from fredholm_amd.renderer import DeviceBuffer
    h, w = img.shape[:2]
    own = bufs is None
    bufs = bufs or [DeviceBuffer(r, w * h * 16) for _ in range(4)]
    bufs[0].upload(img)
    for b in bufs[1:]:
        b.clear()
    r.post_process(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, w, h, pp, bufs[3].ptr)
    r.wait_for_completion()
    out = bufs[3].download(np.float32, (h, w, 4))
    if own:
        for b in bufs:
            b.free()
    return out


# ------------------------------------------------------------------ histogram
@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_histogram_equals_the_restatement_as_integers(ae, oracle, w, h):
    p = params(frame_time=math.inf)
    ae.set_auto_exposure(**p)
    for kind in ("mixed", "constant", "black"):
        img = image(kind, w, h)
        buf = _upload(ae, img)
        ae.auto_exposure_reset()
        before = ae.auto_exposure_state()
        ae.meter_exposure(buf.ptr, w, h)
        got, state = ae.luminance_histogram(), ae.auto_exposure_state()
        buf.free()
        want = histogram(oracle, img, p)
        assert int(want.sum()) == w * h and np.array_equal(got, want), (kind, np.flatnonzero(got != want)[:8])
        if kind == "black":
            assert want[256] == w * h and state == before  # nothing metered: the state is left alone
        else:
            assert _same_state(state, resolve(oracle, want, p, None)), (kind, state)
    if (w, h) == (16, 16):
        assert histogram(oracle, image("constant", w, h), p).max() == 256  # (one bin holds the whole constant image)


# ------------------------------------------------------------------ state
def sequence_images(w=67, h=35):
    """luminance falls (the target rises), then rises (the target falls); a black frame after the second"""
    levels = [1.0, 0.25, None, 0.25, 4.0, 4.0, 4.0]
    return [image("black", w, h) if lv is None else image("noise", w, h, seed=k, level=lv) for k, lv in enumerate(levels)]


@pytest.mark.gpu
def test_state_follows_the_restatement_through_a_rise_a_black_frame_and_a_fall(ae, oracle):
    w, h = 67, 35
    p = params(speed_up=6.0, speed_down=2.0)
    ae.set_auto_exposure(**p)
    want, want64, calls, checked = None, None, 0, []
    for img in sequence_images(w, h):
        buf = _upload(ae, img)
        ae.meter_exposure(buf.ptr, w, h)
        got = ae.auto_exposure_state()
        buf.free()
        hist = histogram(oracle, img, p)
        black = hist[:256].sum() == 0
        before = want
        want, want64 = resolve(oracle, hist, p, want), resolve64(hist, p, want64)
        calls += 0 if black else 1
        if black:
            assert _same_state(got, before) and got["frames"] == calls  # the black frame changed nothing
        if black or calls in (1, 2, 6):
            checked.append(calls)
            assert _same_state(got, want), (calls, got, want)
            assert abs(float(got["ev"]) - want64["ev"]) <= STATE_BOUND and abs(float(got["target_ev"]) - want64["target_ev"]) <= STATE_BOUND, (calls, got, want64)
    assert checked == [1, 2, 2, 6]
    assert want["target_ev"] < want["ev"]  # the sequence ends while the exposure is still falling: the smoothing is what was compared
    ae.auto_exposure_reset()
    img = image("noise", w, h, seed=9, level=0.5)
    buf = _upload(ae, img)
    ae.meter_exposure(buf.ptr, w, h)
    got = ae.auto_exposure_state()
    buf.free()
    assert got["frames"] == 1 and _bits(got["ev"]) == _bits(got["target_ev"]) and _same_state(got, resolve(oracle, histogram(oracle, img, p), p, None))


# ------------------------------------------------------------------ the whole chain, without a restatement
def _chain_image(w, h):
    rng = np.random.default_rng(12)
    return (rng.uniform(0, 1, (h, w, 4)) ** 3 * 8).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(67, 35), (96, 72)])
@pytest.mark.parametrize("mode", ["plain", "bloom", "bloom-relative"])
def test_pinned_exposure_is_the_switched_off_call_at_that_iso_in_every_bit(ae, w, h, mode):
    """ISO = 120 * 2^k is an exposure of exactly 2^k, and fhe_pow(2, k) is exact: with min_ev = max_ev = k the metered chain must be the plain one"""
    import fredholm_amd as F
    img = _chain_image(w, h)
    for k in (-3, 0, 2):
        thr = 2.0
        ae.clear_auto_exposure()
        off = _post(ae, img, F.PostProcessParams(use_bloom=mode != "plain", bloom_threshold=thr * (2.0 ** -k if mode == "bloom-relative" else 1.0), bloom_sigma=5.0,
                                                 ISO=120.0 * 2.0 ** k, chromatic_aberration=1.0))
        ae.set_auto_exposure(min_ev=float(k), max_ev=float(k), bloom_relative=mode == "bloom-relative")
        on = _post(ae, img, F.PostProcessParams(use_bloom=mode != "plain", bloom_threshold=thr, bloom_sigma=5.0, ISO=80.0, chromatic_aberration=1.0))
        assert ae.auto_exposure_state()["ev"] == k
        assert np.array_equal(_bits(on), _bits(off)), (k, mode)
        assert (on[(h // 16) * 16:] == 0).all() and (on[:, (w // 16) * 16:] == 0).all() and on[0, 0, 3] == 1


@pytest.mark.gpu
def test_free_exposure_is_the_checkers_tone_map_of_the_scaled_pixels(ae, oracle):
    import fredholm_amd as F
    w, h = 64, 48
    img = image("noise", w, h, seed=3, level=3.0)
    p = params(frame_time=math.inf)
    ae.set_auto_exposure(**p)
    got = _post(ae, img, F.PostProcessParams(use_bloom=False, ISO=80.0, chromatic_aberration=0.0))
    state = ae.auto_exposure_state()
    assert _same_state(state, resolve(oracle, histogram(oracle, img, p), p, None)) and abs(state["ev"]) > 0.5  # (free: not the ISO exposure, not 1)
    # the tone map's float pixel addressing with ca = 0, as the kernel computes it (tests/test_oracle_anchors.py restates the same for the checker)
    i, j = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    uvx, uvy = i / f32(w), j / f32(h)
    idx = (uvx * f32(w) + f32(w) * (uvy * f32(h))).astype(np.int32)
    x = img.reshape(-1, 4)[idx.reshape(-1), :3] * exposure_of(oracle, state["ev"])
    want = oracle.math("linear_to_srgb", oracle.math("uchimura", x)).reshape(h, w, 3)
    assert np.array_equal(_bits(got[..., :3]), _bits(want)) and (got[..., 3] == 1).all()


# ------------------------------------------------------------------ switched off, and neighbours
@pytest.mark.gpu
@pytest.mark.parametrize("use_bloom", [False, True])
def test_off_cleared_and_beside_a_switched_on_context_the_chain_has_the_parents_bits(ae, oracle, use_bloom):
    import fredholm_amd as F
    w, h = 70, 50  # the images of test_post_process_identical_including_unwritten_border
    img = _chain_image(w, h)
    pp = F.PostProcessParams(use_bloom=use_bloom, bloom_threshold=2.0, bloom_sigma=5.0, ISO=80.0, chromatic_aberration=1.0)
    want = _bits(oracle.post_process(img, use_bloom, 2.0, 5.0, 80.0, 1.0))
    assert ae.get_auto_exposure()[0] is False
    assert np.array_equal(_bits(_post(ae, img, pp)), want)
    ae.set_auto_exposure()
    assert not np.array_equal(_bits(_post(ae, img, pp)), want)  # (the switch does something on this image)
    other = F.Renderer(0)
    try:
        assert other.get_auto_exposure()[0] is False
        assert np.array_equal(_bits(_post(other, img, pp)), want)  # beside the switched-on one
    finally:
        other.close()
    ae.clear_auto_exposure()
    assert np.array_equal(_bits(_post(ae, img, pp)), want)
    with pytest.raises(F.native.FredholmError):
        ae.auto_exposure_state()  # off: the state is gone


@pytest.mark.gpu
def test_a_refused_set_leaves_parameters_state_and_output_alone(ae):
    import fredholm_amd as F
    w, h = 67, 35
    img = _chain_image(w, h)
    pp = F.PostProcessParams(use_bloom=False, ISO=80.0, chromatic_aberration=1.0)
    ae.set_auto_exposure(key=0.3, speed_up=0.0, speed_down=0.0)  # (speeds 0: after the first frame ev stays, so two calls give the same output)
    first, state, par = _post(ae, img, pp), ae.auto_exposure_state(), ae.get_auto_exposure()
    for bad in (dict(key=0.0), dict(low=0.9, high=0.1), dict(frame_time=float("nan")), dict(min_ev=1.0, max_ev=0.0)):
        with pytest.raises(F.native.FredholmError):
            ae.set_auto_exposure(**bad)
    assert ae.get_auto_exposure() == par and par[0] is True and abs(par[1]["key"] - 0.3) < 1e-7
    after = ae.auto_exposure_state()
    assert after == state
    again = _post(ae, img, pp)
    assert np.array_equal(_bits(again), _bits(first)) and ae.auto_exposure_state()["frames"] == state["frames"] + 1


@pytest.mark.gpu
def test_a_group_of_two_members_on_one_device_gives_the_plain_contexts_state_and_output(ae):
    import fredholm_amd as F
    w, h = 67, 35
    img = _chain_image(w, h)
    pp = F.PostProcessParams(use_bloom=True, bloom_threshold=2.0, bloom_sigma=5.0, ISO=80.0, chromatic_aberration=1.0)
    ae.set_auto_exposure(bloom_relative=True)
    plain, plain_state, plain_hist = _post(ae, img, pp), ae.auto_exposure_state(), ae.luminance_histogram()
    g = F.Renderer(devices=[0, 0])
    try:
        assert g.group_size == 2
        g.set_auto_exposure(bloom_relative=True)
        out = _post(g, img, pp)
        assert g.auto_exposure_state() == plain_state and np.array_equal(g.luminance_histogram(), plain_hist)
        assert np.array_equal(_bits(out), _bits(plain))
    finally:
        g.close()


# ------------------------------------------------------------------ end to end
E2E = dict(w=96, h=72, spp=16, depth=5, frames_before=4, frames_after=4)


@pytest.fixture(scope="module")
def cornell_frames():
    """the beauty of 4 frames of the Cornell box and 4 after its light's emission x 0.25 (the sequence of the response tests), rendered once"""
    import fredholm_amd as F
    from fredholm_amd import scenes
    from test_gpu_denoise_response import changed_scene
    q = E2E
    r = F.Renderer(0)
    frames = []
    try:
        cam = F.Camera(**scenes.CORNELL_CAMERA)
        L = None
        for k in range(q["frames_before"] + q["frames_after"]):
            if k in (0, q["frames_before"]):
                r.load_scene(scenes.cornell_box() if k == 0 else changed_scene("L"))
                r.build_ias()
                if L is None:
                    r.set_resolution(q["w"], q["h"])
                    L = F.RenderLayer(r, q["w"], q["h"])
            L.clear()
            r.init_render_states()
            r.seed = 1 + k
            r.render(cam, (0.0, 0.0, 0.0), L, q["spp"], q["depth"])
            r.wait_for_completion()
            frames.append(L.download("beauty").reshape(q["h"], q["w"], 4).copy())
        L.free()
    finally:
        r.close()
    return frames


def _tone_mapped_means(r, frames, pp):
    """mean luminance of the written pixels of every frame's post output, and the state after each"""
    from fredholm_amd.renderer import DeviceBuffer
    h, w = frames[0].shape[:2]
    bufs = [DeviceBuffer(r, w * h * 16) for _ in range(4)]
    means, states = [], []
    on = r.get_auto_exposure()[0]
    for f in frames:
        out = _post(r, f, pp, bufs)[:(h // 16) * 16, :(w // 16) * 16, :3].astype(np.float64)
        means.append(float((out @ np.array([0.2126729, 0.7151522, 0.0721750])).mean()))
        states.append(r.auto_exposure_state() if on else None)
    for b in bufs:
        b.free()
    return means, states


@pytest.mark.gpu
def test_cornell_box_with_a_dimmed_light_end_to_end(ae, oracle, cornell_frames):
    import fredholm_amd as F
    frames, nb = cornell_frames, E2E["frames_before"]
    pp = F.PostProcessParams(use_bloom=False, ISO=80.0, chromatic_aberration=1.0)
    off, _ = _tone_mapped_means(ae, frames, pp)
    # no adaptation: the exposure follows the light at once, and the picture changes by less than it does without the switch
    p = params(frame_time=math.inf)
    ae.set_auto_exposure(**p)
    held, states = _tone_mapped_means(ae, frames, pp)
    step = lambda m: abs(np.mean(m[nb:]) - np.mean(m[:nb]))
    assert step(off) > 0.02 and step(held) < step(off), (off, held)
    want = None
    for f, s in zip(frames, states):
        want = resolve(oracle, histogram(oracle, f, p), p, want)
        assert _same_state(s, want), (s, want)
    # finite speeds: ev moves monotonically towards the new target, each frame the restatement's
    ae.clear_auto_exposure()
    p = params(frame_time=1.0 / 24.0, speed_up=3.0, speed_down=1.0)
    ae.set_auto_exposure(**p)
    _, states = _tone_mapped_means(ae, frames, pp)
    want = None
    for f, s in zip(frames, states):
        want = resolve(oracle, histogram(oracle, f, p), p, want)
        assert _same_state(s, want), (s, want)
    evs = [float(s["ev"]) for s in states]
    assert states[nb]["target_ev"] > states[nb - 1]["target_ev"] + 1.0  # a quarter of the light: about two stops up
    assert all(evs[k] < evs[k + 1] < float(states[k + 1]["target_ev"]) for k in range(nb - 1, len(frames) - 1)), (evs, [float(s["target_ev"]) for s in states])
