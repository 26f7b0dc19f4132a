"""GPU tests (-m gpu): adaptive sampling (fh_set_adaptive_sampling) against plain renders, a float32 replay of its moments and a restatement of its stop rule.

Sampler keys are (pixel, per-pixel sample index, slot, seed) and the running means are updated sample by sample in a fixed order, so a pixel that stops after s
samples holds exactly the bits a plain render holds after s samples.  Every comparison below is therefore bit for bit: all six layers and the sample counts, in
every pixel, any two NaNs counting as equal.  Small frames (64 x 48) of three scenes: the Cornell box (NEE + MIS), the Hosek-sky soup with the sky-pixel split
forced (FH_SKY_SPLIT_MIN_LOG2=0: k_sky_pixels and the passes both run) and the textured box with cut-outs.
"""
import ctypes as C

import numpy as np
import pytest

import fredholm_amd as F
from fredholm_amd import native as N
from fredholm_amd import scenes
from fredholm_amd.renderer import DeviceBuffer

pytestmark = pytest.mark.gpu

W, H = 64, 48
P = W * H
NAMES = F.RenderLayer.NAMES
SCENES = ("cornell", "soup_sky", "textured")
FLAG_SERIAL_PASSES = 8
FLAG_REFERENCE_FIRSTHIT = 4


def _scene(name):
    """(scene, camera, background, max_depth, Hosek sky, environment of the context)"""
    if name == "cornell":
        return scenes.cornell_box(), F.Camera(**scenes.CORNELL_CAMERA), (0.0, 0.0, 0.0), 5, False, {}
    if name == "soup_sky":
        cam = F.Camera(origin=(0.4, 0.2, 4.0), fov=1.2, F=16.0, focus=4.0, forward=(-0.15, -0.05, -1.0))
        return scenes.triangle_soup(3000, 0.1), cam, (0.05, 0.1, 0.2), 5, True, {"FH_SKY_SPLIT_MIN_LOG2": "0"}
    if name == "textured":
        return scenes.textured_cornell_box(), F.Camera(**scenes.CORNELL_CAMERA), (0.1, 0.2, 0.4), 4, False, {}
    raise KeyError(name)


_SC = {}


def _sc(name):
    if name not in _SC:
        _SC[name] = _scene(name)
    return _SC[name]


def _context(monkeypatch, name, env=None, pool=None, shard=None):
    sc, cam, bg, depth, sky, scene_env = _sc(name)
    e = dict(scene_env)
    e.update(env or {})
    for k in ("FH_SKY_SPLIT", "FH_PIPELINE", "FH_SKY_SPLIT_MIN_LOG2"):
        monkeypatch.delenv(k, raising=False)
    for k, v in e.items():
        monkeypatch.setenv(k, v)
    r = F.Renderer(0)  # (the environment is read here)
    for k in e:
        monkeypatch.delenv(k)
    if pool:
        r.set_path_pool(pool)
    r.load_scene(sc)
    r.build_ias()
    if sky:
        r.set_directional_light((0.0, 0.0, 0.0), scenes.SOUP_SUN, 0.0)
        r.clear_directional_light()
        r.load_arhosek_sky(3.0, 0.3)
    if shard:
        r.set_tile_shard(shard[0], shard[1], 8, 8)
    r.set_resolution(W, H)
    return r, F.RenderLayer(r, W, H)


def _params(threshold, min_samples, step, floor=0.01):
    return N.AdaptiveParamsC(float(threshold), float(floor), int(min_samples), int(step))


def _set(r, p):
    return N.lib().fh_set_adaptive_sampling(r._ctx, None if p is None else C.byref(p))


def _render(r, L, name, calls):
    _, cam, bg, depth, _, _ = _sc(name)
    for n in calls:
        r.render(cam, bg, L, n, depth)
    r.wait_for_completion()


def _state(r, L, moments=False):
    s = {n: L.download(n) for n in NAMES}
    s["count"] = r.sample_counts()
    if moments:
        s["m"] = r.luminance_moments()
    return s


def _bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != np.float32:
        return a == b
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _assert_same(got, want, what, keys=NAMES + ("count",)):
    for k in keys:
        eq = _bits_equal(got[k], want[k])
        eq = eq.reshape(H, W, -1).all(axis=2)
        bad = np.flatnonzero(~eq)
        assert bad.size == 0, f"{what}: {k} differs in {bad.size} pixels, the first at pixel {bad[0]}"


def _fresh(r, L, p):
    r.wait_for_completion()
    r.init_render_states()
    L.clear()
    if p is not None:
        assert _set(r, p) == 0, N.lib().fh_last_error(r._ctx)
    else:
        assert _set(r, None) == 0


# ------------------------------------------------------------------ the test's own statement of the stop rule (include/fredholm_hip.h)
def _converged(n, m1, m2, threshold, floor, min_samples, step):
    """float32, in the contract's order; n an int, m1 / m2 float32 arrays"""
    f = np.float32
    if n < min_samples or n % step:
        return np.zeros(m1.shape, bool)
    with np.errstate(all="ignore"):
        d = (m2 - m1 * m1).astype(f)
        d = np.where(d < f(0), f(0), d).astype(f)  # (NaN stays NaN)
        var = (d * f(f(n) / f(n - 1))).astype(f)
        e2 = (var / f(n)).astype(f)
        ref = np.where(m1 > f(floor), m1, f(floor)).astype(f)
        t = (f(threshold) * ref).astype(f)
        return (f(threshold) > f(0)) & (e2 <= (t * t).astype(f))


def _boundary_snapshots(monkeypatch, name, step, cap):
    """threshold-0 run (every pixel to the cap) in calls of `step`: the state at every boundary"""
    r, L = _context(monkeypatch, name)
    _fresh(r, L, _params(0.0, 2, step))
    snaps = {0: _state(r, L, moments=True)}
    for n in range(step, cap + 1, step):
        _render(r, L, name, [step])
        snaps[n] = _state(r, L, moments=True)
    r.close()
    return snaps


def _expected_stops(snaps, threshold, floor, min_samples, step, cap):
    stop = np.full((H, W), cap, np.int64)
    done = np.zeros((H, W), bool)
    for n in range(0, cap + 1, step):
        c = _converged(n, snaps[n]["m"][..., 0], snaps[n]["m"][..., 1], threshold, floor, min_samples, step) & ~done
        stop[c] = n
        done |= c
    return stop


def _state_at(snaps, stop):
    out = {}
    for k in NAMES + ("count",):
        a = np.array(snaps[0][k])
        for n in np.unique(stop):
            sel = stop == n
            a[sel] = snaps[int(n)][k][sel]
        out[k] = a
    return out


def _error_quantiles(snaps, n, floor, qs):
    m = snaps[n]["m"].astype(np.float64)
    e2 = np.maximum(m[..., 1] - m[..., 0] ** 2, 0.0) / (n - 1)
    rel = np.sqrt(e2) / np.maximum(m[..., 0], floor)
    rel = rel[np.isfinite(rel) & (rel > 0.0)]  # (pixels of zero variance -- the sky, emitters -- stop at any threshold: quantiles of the others)
    return [float(np.quantile(rel, q)) for q in qs]


# ------------------------------------------------------------------ 1. threshold 0 is a plain render
@pytest.mark.parametrize("name", SCENES)
def test_threshold_zero_equals_plain_render(monkeypatch, name):
    rp, Lp = _context(monkeypatch, name)
    ra, La = _context(monkeypatch, name)
    _fresh(rp, Lp, None)
    _fresh(ra, La, _params(0.0, 64, 16))
    for pattern in ([1], [3], [17], [1] * 40):
        _render(rp, Lp, name, pattern)
        _render(ra, La, name, pattern)
        _assert_same(_state(ra, La), _state(rp, Lp), f"{name}, threshold 0 after calls {pattern[:3]}{'...' if len(pattern) > 3 else ''}")
    assert ra.active_pixel_count() == P
    rp.close()
    ra.close()


# ------------------------------------------------------------------ 2. the moments are a float32 replay of the contract
@pytest.mark.parametrize("name", SCENES)
def test_moments_equal_float32_replay(monkeypatch, name):
    S = 24
    r, L = _context(monkeypatch, name)
    rad = []
    for n in range(S):  # sample n's NaN-guarded radiance: issued = n, sample_count = 0, cleared layers, one sample
        _fresh(r, L, None)
        iss = np.full(P, n, np.uint32)
        N.check(r._ctx, N.lib().fh_kat_set_issued(r._ctx, N.ptr(iss), C.c_uint32(P)), "fh_kat_set_issued")
        _render(r, L, name, [1])
        rad.append(L.download("beauty")[..., :3].copy())
    f = np.float32
    m1 = np.zeros((H, W), f)
    m2 = np.zeros((H, W), f)
    for n in range(S):
        x = rad[n]
        y = ((x[..., 0] * f(0.2126729)).astype(f) + (x[..., 1] * f(0.7151522)).astype(f)).astype(f)
        y = (y + (x[..., 2] * f(0.0721750)).astype(f)).astype(f)
        coef = f(f(1.0) / (f(n) + f(1.0)))
        fn = f(n)
        m1 = (coef * ((fn * m1).astype(f) + y).astype(f)).astype(f)
        m2 = (coef * ((fn * m2).astype(f) + (y * y).astype(f)).astype(f)).astype(f)
    _fresh(r, L, _params(0.0, 2, 4))
    _render(r, L, name, [5, 1, 18])
    m = r.luminance_moments()
    assert np.array_equal(r.sample_counts(), np.full((H, W), S, np.uint32))
    for k, want in ((0, m1), (1, m2)):
        eq = _bits_equal(m[..., k], want)
        assert eq.all(), f"{name}: m{k + 1} differs from the float32 replay in {int((~eq).sum())} pixels"
    r.close()


# ------------------------------------------------------------------ 3. the stop rule
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("step,min_samples,cap", [(4, 8, 48), (16, 32, 96)])
def test_each_pixel_stops_at_its_first_converged_boundary(monkeypatch, oracle, name, step, min_samples, cap):
    floor = 0.01
    snaps = _boundary_snapshots(monkeypatch, name, step, cap)
    thresholds = _error_quantiles(snaps, min_samples, floor, (0.3, 0.7))
    r, L = _context(monkeypatch, name)
    for t in thresholds:
        stop = _expected_stops(snaps, t, floor, min_samples, step, cap)
        assert (stop < cap).any(), f"{name}: threshold {t} stops no pixel early"
        _fresh(r, L, _params(t, min_samples, step, floor))
        _render(r, L, name, [cap])
        got = _state(r, L)
        assert np.array_equal(got["count"], stop.astype(np.uint32)), f"{name}, threshold {t:.4g}: {int((got['count'] != stop).sum())} pixels stop elsewhere"
        _assert_same(got, _state_at(snaps, stop), f"{name}, threshold {t:.4g}, step {step}")
    r.close()
    if name == "cornell":  # the checker in rounds of `step` samples: its snapshot at each pixel's count
        sc, cam, bg, depth, _, _ = _sc(name)
        S = oracle.Scene(sc)
        Lo = S.new_layers(W, H)
        ref = {0: {k: np.array(Lo[k]) for k in NAMES}}
        for n in range(step, cap + 1, step):
            for _ in range(step):
                S.render(cam.params(), W, H, Lo, 1, depth, bg=bg, n_threads=8)
            ref[n] = {k: np.array(Lo[k]) for k in NAMES}
        for n in ref:
            ref[n]["count"] = np.full((H, W), n, np.uint32)
        stop = _expected_stops(snaps, thresholds[0], floor, min_samples, step, cap)
        _assert_same(_state_at(snaps, stop), _state_at(ref, stop), f"checker, step {step}")


# ------------------------------------------------------------------ 4. how the samples are submitted changes no bit
def _invariance_params(monkeypatch, name):
    snaps = _boundary_snapshots(monkeypatch, name, 4, 8)
    return _params(_error_quantiles(snaps, 8, 0.01, (0.5,))[0], 8, 4)


@pytest.mark.parametrize("name", SCENES)
def test_splitting_and_pipeline_change_no_bit(monkeypatch, name):
    p = _invariance_params(monkeypatch, name)
    cap = 48

    def run(calls=(cap,), env=None, pool=None, flags=0):
        r, L = _context(monkeypatch, name, env=env, pool=pool)
        if flags:
            r.set_flags(flags)
        _fresh(r, L, p)
        _render(r, L, name, calls)
        s = _state(r, L, moments=True)
        r.close()
        return s

    ref = run()
    assert 0 < int((ref["count"] < cap).sum()) < P, "the invariance run should stop some pixels early and not all"
    keys = NAMES + ("count", "m")
    _assert_same(run(calls=(5, 7, 13, 23)), ref, f"{name}: calls ending off a boundary", keys)
    _assert_same(run(calls=(1,) * cap), ref, f"{name}: 1-spp calls", keys)
    _assert_same(run(pool=2 * P), ref, f"{name}: small path pool", keys)
    _assert_same(run(flags=FLAG_SERIAL_PASSES), ref, f"{name}: FH_FLAG_SERIAL_PASSES", keys)
    _assert_same(run(env={"FH_PIPELINE": "0"}), ref, f"{name}: FH_PIPELINE=0", keys)
    _assert_same(run(env={"FH_PIPELINE": "2"}), ref, f"{name}: FH_PIPELINE=2", keys)
    _assert_same(run(env={"FH_SKY_SPLIT": "0"}), ref, f"{name}: FH_SKY_SPLIT=0", keys)
    for world in (2, 3):
        ctxs = [_context(monkeypatch, name, shard=(k, world)) for k in range(world)]
        counts = np.zeros((H, W), np.uint32)
        for r, L in ctxs:
            _fresh(r, L, p)
            _render(r, L, name, [cap])
            counts += r.sample_counts()
        got = {"count": counts}
        r0 = ctxs[0][0]
        for layer in NAMES:
            fpp = 1 if layer == "depth" else 4
            packed = []
            for r, L in ctxs:
                b = DeviceBuffer(r, max(1, r.owned_pixel_count()) * fpp * 4)
                r.pack_owned(L.ptrs[layer], fpp, b.ptr)
                r.wait_for_completion()
                packed.append(b)
            out = DeviceBuffer(r0, P * fpp * 4)
            r0.unpack_shards([b.ptr for b in packed], fpp, out.ptr)
            got[layer] = out.download(np.float32, (H, W) if fpp == 1 else (H, W, 4))
            for b in packed + [out]:
                b.free()
        _assert_same(got, ref, f"{name}: tile shards of world {world}")
        for r, _ in ctxs:
            r.close()


# ------------------------------------------------------------------ 5. counters
@pytest.mark.parametrize("name", SCENES)
def test_paths_and_active_count_follow_the_stops(monkeypatch, name):
    floor, step, min_samples, cap = 0.01, 4, 8, 32
    snaps = _boundary_snapshots(monkeypatch, name, step, cap)
    t = _error_quantiles(snaps, min_samples, floor, (0.5,))[0]
    r, L = _context(monkeypatch, name)
    _fresh(r, L, _params(t, min_samples, step, floor))
    before = np.zeros((H, W), np.int64)
    for calls in ([3], [9], [1, 1], [18]):
        r.reset_stats()
        _render(r, L, name, calls)
        now = r.sample_counts().astype(np.int64)
        assert r.stats()["paths"] == int((now - before).sum()), f"{name}: fh_stats.paths is not the sum of the count increments after {calls}"
        before = now
    stop = _expected_stops(snaps, t, floor, min_samples, step, cap)
    assert np.array_equal(before, np.minimum(stop, 32))
    # at the cap every pixel sits on a boundary: the active ones are those the restated predicate does not stop
    assert r.active_pixel_count() == int((~_converged(32, snaps[32]["m"][..., 0], snaps[32]["m"][..., 1], t, floor, min_samples, step) & (stop == cap)).sum())
    # a fully converged frame: FH_OK, no bit changes, no path
    _fresh(r, L, _params(1e10, 2, 2, floor))
    _render(r, L, name, [6])
    assert r.active_pixel_count() == 0
    a = _state(r, L, moments=True)
    r.reset_stats()
    _render(r, L, name, [5, 16])
    assert r.stats()["paths"] == 0
    _assert_same(_state(r, L, moments=True), a, f"{name}: a converged frame", NAMES + ("count", "m"))
    assert np.array_equal(a["count"], np.full((H, W), 2, np.uint32))
    r.close()


# ------------------------------------------------------------------ 6. errors
def test_bad_parameters_and_states_are_refused(monkeypatch):
    r, L = _context(monkeypatch, "cornell")
    for bad in (_params(-0.1, 8, 4), _params(float("nan"), 8, 4), _params(float("inf"), 8, 4), _params(0.1, 8, 4, floor=0.0), _params(0.1, 8, 4, floor=-1.0),
                _params(0.1, 8, 4, floor=float("nan")), _params(0.1, 1, 4), _params(0.1, 8, 0)):
        assert _set(r, bad) == -1
    assert r.adaptive_sampling() is None
    m = DeviceBuffer(r, 8 * P)
    assert N.lib().fh_get_luminance_moments(r._ctx, C.c_void_p(m.ptr)) == -1  # while off
    _render(r, L, "cornell", [2])
    assert _set(r, _params(0.1, 8, 4)) == -1  # samples accumulated since the init
    assert _set(r, None) == 0  # turning it off is always accepted
    r.init_render_states()
    assert _set(r, _params(0.1, 8, 4)) == 0
    assert r.adaptive_sampling() == {"threshold": pytest.approx(0.1), "floor": pytest.approx(0.01), "min_samples": 8, "step": 4}
    assert N.lib().fh_get_luminance_moments(r._ctx, C.c_void_p(m.ptr)) == 0
    r.set_flags(FLAG_REFERENCE_FIRSTHIT)
    _, cam, bg, depth, _, _ = _sc("cornell")
    with pytest.raises(N.FredholmError):
        r.render(cam, bg, L, 2, depth)
    r.render(cam, bg, L, 1, depth)  # (one sample per launch has no first-hit state)
    r.set_flags(0)
    _render(r, L, "cornell", [3])
    assert _set(r, _params(0.2, 8, 4)) == -1
    # fh_set_resolution keeps the mode and resets its state
    r.set_resolution(W, H)
    assert r.adaptive_sampling() is not None
    assert np.array_equal(r.sample_counts(), np.zeros((H, W), np.uint32))
    assert np.array_equal(r.luminance_moments(), np.zeros((H, W, 2), np.float32))
    assert _set(r, _params(0.2, 8, 4)) == 0
    m.free()
    r.close()


# ------------------------------------------------------------------ 7. it helps
def test_adaptive_beats_uniform_at_equal_samples_on_the_cornell_box(monkeypatch):
    """Cornell box, 64 x 48: truth = 8192 spp plain.  Adaptive: threshold 0.05, floor 0.01, min_samples 64, step 16, cap 1024.  Uniform: the adaptive run's
    mean spp, rounded.  Error = mean over pixels of ((y - y_truth) / max(y_truth, floor))^2 of the beauty luminance.  Sampling is deterministic, so the numbers
    are fixed; first measured on an MI355X: mean spp 633.8, 1728 of 3072 pixels stopped before the cap, error 4.939e-3 adaptive against 6.949e-3 uniform
    (ratio 0.71), 98.55 % of the early pixels within 3 thresholds of the truth.  The bounds below leave slack: ratio < 0.85, >= 95 %."""
    name, thr, floor = "cornell", 0.05, 0.01
    r, L = _context(monkeypatch, name)

    def lum(b):
        b = b.astype(np.float64)
        return b[..., 0] * 0.2126729 + b[..., 1] * 0.7151522 + b[..., 2] * 0.0721750

    _fresh(r, L, None)
    _render(r, L, name, [8192])
    truth = lum(L.download("beauty"))
    _fresh(r, L, _params(thr, 64, 16, floor))
    _render(r, L, name, [1024])
    ya = lum(L.download("beauty"))
    counts = r.sample_counts()
    mean_spp = float(counts.mean())
    _fresh(r, L, None)
    _render(r, L, name, [max(1, int(round(mean_spp)))])
    yu = lum(L.download("beauty"))
    ref = np.maximum(truth, floor)
    err_a = float(np.mean(((ya - truth) / ref) ** 2))
    err_u = float(np.mean(((yu - truth) / ref) ** 2))
    early = counts < 1024
    within = float(np.mean(np.abs(ya - truth)[early] <= 3.0 * thr * ref[early])) if early.any() else 1.0
    print(f"adaptive mean spp {mean_spp:.1f}, stopped early {int(early.sum())} of {P}; relative squared error adaptive {err_a:.3e}, uniform {err_u:.3e}; "
          f"early pixels within 3 thr: {within:.4f}")
    assert early.any() and not early.all()
    assert err_a < 0.85 * err_u
    assert within >= 0.95
    r.close()
