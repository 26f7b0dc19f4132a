"""GPU tests (-m gpu): the adaptive-sampling policy (fh_set_adaptive_policy): guard blocks that stop together and boundaries on a doubling schedule.

The method is that of test_gpu_adaptive_sampling.py.  A threshold-0 run in calls of `step` gives the state of every pixel at every multiple of `step`; the
test's own numpy restatement of the rule (the per-pixel predicate in float32, in the contract's order; AND over the aligned block; boundaries b0 * 2^k) gives
each pixel's stop; and a pixel that stops after s samples must hold exactly the bits of the snapshot at s: all six layers and the sample counts, in every pixel,
any two NaNs counting as equal.  Scenes: the Cornell box, the Hosek-sky soup with the sky-pixel split forced (k_sky_pixels and the passes both run, and guard
blocks at the silhouette hold pixels of both) and the textured box with cut-outs; frames of 64 x 48 and of 61 x 43 (no multiple of 8 in either direction).
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fredholm_amd as F
from fredholm_amd import native as N
from fredholm_amd import scenes
from fredholm_amd.renderer import DeviceBuffer

pytestmark = pytest.mark.gpu

SIZES = ((64, 48), (61, 43))
NAMES = F.RenderLayer.NAMES
SCENES = ("cornell", "soup_sky", "textured")
FLAG_SERIAL_PASSES = 8
FH_E_INVALID = -1
STEP, CAP_SNAP = 4, 80  # the snapshots every test shares: the state at 0, 4, 8 ... 80 samples


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


def _context(monkeypatch, name, size=SIZES[0], env=None, pool=None, shard=None, devices=None):
    sc, cam, bg, depth, sky, scene_env = _sc(name)
    e = dict(scene_env)
    e.update(env or {})
    for k in ("FH_SKY_SPLIT", "FH_PIPELINE", "FH_SKY_SPLIT_MIN_LOG2"):
        monkeypatch.delenv(k, raising=False)
    for k, v in e.items():
        monkeypatch.setenv(k, v)
    r = F.Renderer(0) if devices is None else F.Renderer(devices=devices)  # (the environment is read here)
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
    r.set_resolution(*size)
    return r, F.RenderLayer(r, *size)


def _params(threshold, min_samples, step, floor=0.01):
    return N.AdaptiveParamsC(float(threshold), float(floor), int(min_samples), int(step))


def _set(r, p):
    return N.lib().fh_set_adaptive_sampling(r._ctx, None if p is None else C.byref(p))


def _policy(r, block, growth):
    return N.lib().fh_set_adaptive_policy(r._ctx, C.c_uint32(block), C.c_uint32(growth))


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
        h, w = np.asarray(want[k]).shape[:2]
        eq = _bits_equal(got[k], want[k]).reshape(h, w, -1).all(axis=2)
        bad = np.flatnonzero(~eq)
        assert bad.size == 0, f"{what}: {k} differs in {bad.size} pixels, the first at pixel {bad[0]}"


def _fresh(r, L, p, policy=None):
    """init_render_states, cleared layers, then the policy (None: left as it is) and the mode (None: off)"""
    r.wait_for_completion()
    r.init_render_states()
    L.clear()
    if policy is not None:
        assert _policy(r, *policy) == 0, N.lib().fh_last_error(r._ctx)
    if p is not None:
        assert _set(r, p) == 0, N.lib().fh_last_error(r._ctx)
    else:
        assert _set(r, None) == 0


# ------------------------------------------------------------------ the test's own statement of the rule (include/fredholm_hip.h)
def _b0(min_samples, step):
    return -(-min_samples // step) * step


def _is_boundary(n, min_samples, step, growth):
    if growth == 1:
        return n >= min_samples and n % step == 0
    b0 = _b0(min_samples, step)
    if n < b0 or n % b0:
        return False
    q = n // b0
    return q & (q - 1) == 0


def _pixel_predicate(n, m1, m2, threshold, floor):
    """e2 <= (threshold * max(m1, floor))^2 in float32, in the contract's order, at a count n that is a boundary; m1 / m2 float32 arrays"""
    f = np.float32
    with np.errstate(all="ignore"):
        d = (m2 - m1 * m1).astype(f)
        d = np.where(d < f(0), f(0), d).astype(f)  # (NaN stays NaN)
        var = (d * f(f(n) / f(n - 1))).astype(f)
        e2 = (var / f(n)).astype(f)
        ref = np.where(m1 > f(floor), m1, f(floor)).astype(f)
        t = (f(threshold) * ref).astype(f)
        return (f(threshold) > f(0)) & (e2 <= (t * t).astype(f))


def _block_all(c, block):
    """every pixel: do all pixels of its guard block (aligned, cut off by the frame) hold True"""
    out = np.empty_like(c)
    h, w = c.shape
    for y in range(0, h, block):
        for x in range(0, w, block):
            out[y:y + block, x:x + block] = c[y:y + block, x:x + block].all()
    return out


def _block_max(v, block):
    h, w = v.shape
    return np.array([v[y:y + block, x:x + block].max() for y in range(0, h, block) for x in range(0, w, block)])


def _converged(snaps, n, threshold, floor, min_samples, step, block, growth):
    if n == 0 or not _is_boundary(n, min_samples, step, growth):
        return np.zeros(snaps[0]["count"].shape, bool)
    return _block_all(_pixel_predicate(n, snaps[n]["m"][..., 0], snaps[n]["m"][..., 1], threshold, floor), block)


def _expected_stops(snaps, threshold, floor, min_samples, step, cap, block, growth):
    stop = np.full(snaps[0]["count"].shape, cap, np.int64)
    done = np.zeros(stop.shape, bool)
    for n in range(0, cap + 1, STEP):
        c = _converged(snaps, n, threshold, floor, min_samples, step, block, growth) & ~done
        stop[c] = n
        done |= c
    return stop


def _state_at(snaps, stop, keys=NAMES + ("count",)):
    out = {}
    for k in keys:
        a = np.array(snaps[0][k])
        for n in np.unique(stop):
            sel = stop == n
            a[sel] = snaps[int(n)][k][sel]
        out[k] = a
    return out


_SNAPS = {}


def _snapshots(monkeypatch, name, size=SIZES[0]):
    """threshold-0 run with the default policy (every pixel to CAP_SNAP) in calls of STEP: the state at every multiple of STEP"""
    if (name, size) not in _SNAPS:
        r, L = _context(monkeypatch, name, size)
        _fresh(r, L, _params(0.0, 2, STEP))
        snaps = {0: _state(r, L, moments=True)}
        for n in range(STEP, CAP_SNAP + 1, STEP):
            _render(r, L, name, [STEP])
            snaps[n] = _state(r, L, moments=True)
            assert (snaps[n]["count"] == n).all()
        r.close()
        _SNAPS[(name, size)] = snaps
    return _SNAPS[(name, size)]


def _block_threshold(snaps, n, floor, block, q):
    """a quantile of the per-block maximum of the relative error estimate at n samples, over the blocks where it is finite and not zero (blocks of zero variance
    -- the sky, emitters -- stop at any threshold): about a share q of those blocks is converged at n, the others are not"""
    m = snaps[n]["m"].astype(np.float64)
    with np.errstate(all="ignore"):
        rel = np.sqrt(np.maximum(m[..., 1] - m[..., 0] ** 2, 0.0) / (n - 1)) / np.maximum(m[..., 0], floor)
    rel = np.where(np.isfinite(rel), rel, np.inf)
    b = _block_max(rel, block)
    b = b[np.isfinite(b) & (b > 0.0)]
    return float(np.quantile(b, q))


def _splitting_threshold(snaps, floor, min_samples, cap, block, growth, also=None):
    """(threshold, expected stops): the largest of a few quantiles of the per-block maximum error at the first boundary for which the restated rule stops some blocks
    before the cap and leaves some running to it (at few samples the estimates fall fast, so a median can let every block stop before the cap)"""
    for q in (0.5, 0.35, 0.25, 0.15, 0.08, 0.04, 0.02):
        t = _block_threshold(snaps, _b0(min_samples, STEP), floor, block, q)
        stop = _expected_stops(snaps, t, floor, min_samples, STEP, cap, block, growth)
        if (stop < cap).any() and (stop == cap).any() and (also is None or also(stop)):
            return t, stop
    raise AssertionError("no quantile of the block errors splits the frame into blocks that stop early and blocks that do not")


def _assert_blocks_share_counts(count, block, what):
    lo = -_block_max(-count.astype(np.int64), block)
    hi = _block_max(count.astype(np.int64), block)
    assert np.array_equal(lo, hi), f"{what}: {int((lo != hi).sum())} guard blocks hold pixels of different counts"


# ------------------------------------------------------------------ 1. the defaults are the per-pixel rule
@pytest.mark.parametrize("name", SCENES)
def test_policy_one_one_is_the_mode_without_the_call(monkeypatch, name):
    floor, min_samples, cap = 0.01, 8, 48
    snaps = _snapshots(monkeypatch, name)
    p = _params(_block_threshold(snaps, min_samples, floor, 1, 0.5), min_samples, STEP, floor)
    ra, La = _context(monkeypatch, name)
    rb, Lb = _context(monkeypatch, name)
    _fresh(ra, La, p)
    _fresh(rb, Lb, p, policy=(1, 1))
    assert rb.adaptive_policy() == (1, 1) == ra.adaptive_policy()
    for calls in ([cap], [7, 9]):
        _render(ra, La, name, calls)
        _render(rb, Lb, name, calls)
        a, b = _state(ra, La, moments=True), _state(rb, Lb, moments=True)
        _assert_same(b, a, f"{name}: policy (1, 1) after {calls}", NAMES + ("count", "m"))
        assert ra.active_pixel_count() == rb.active_pixel_count()
    assert 0 < int((a["count"] < cap + 16).sum()) < a["count"].size
    stop = _expected_stops(snaps, p.threshold, floor, min_samples, STEP, cap + 16, 1, 1)
    assert np.array_equal(a["count"], stop.astype(np.uint32))
    ra.close()
    rb.close()


# ------------------------------------------------------------------ 2. the block rule
_CHECKER = {}


def _checker_snapshots(oracle, cap):
    """the CPU checker's state of the Cornell box at every multiple of STEP up to cap (64 x 48)"""
    if cap not in _CHECKER:
        W, H = SIZES[0]
        sc, cam, bg, depth, _, _ = _sc("cornell")
        S = oracle.Scene(sc)
        Lo = S.new_layers(W, H)
        ref = {0: {k: np.array(Lo[k]) for k in NAMES}}
        for n in range(STEP, cap + 1, STEP):
            for _ in range(STEP):
                S.render(cam.params(), W, H, Lo, 1, depth, bg=bg, n_threads=8)
            ref[n] = {k: np.array(Lo[k]) for k in NAMES}
        for n in ref:
            ref[n]["count"] = np.full((H, W), n, np.uint32)
        _CHECKER[cap] = ref
    return _CHECKER[cap]


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("block", (2, 4, 8))
def test_each_block_stops_at_the_first_boundary_where_all_of_it_is_converged(monkeypatch, oracle, name, size, block):
    floor, min_samples, cap = 0.01, 8, 48
    snaps = _snapshots(monkeypatch, name, size)
    t, stop = _splitting_threshold(snaps, floor, min_samples, cap, block, 1)
    assert (stop < cap).any(), f"{name}: threshold {t} stops no block before the cap"
    assert (stop == cap).any(), f"{name}: threshold {t} stops every block before the cap"
    r, L = _context(monkeypatch, name, size)
    _fresh(r, L, _params(t, min_samples, STEP, floor), policy=(block, 1))
    _render(r, L, name, [cap])
    got = _state(r, L)
    _assert_blocks_share_counts(got["count"], block, f"{name}, block {block}")
    assert np.array_equal(got["count"], stop.astype(np.uint32)), f"{name}, block {block}, threshold {t:.4g}: {int((got['count'] != stop).sum())} pixels stop elsewhere"
    _assert_same(got, _state_at(snaps, stop), f"{name}, block {block}, threshold {t:.4g}")
    # the rule is not the per-pixel one: some pixel that was converged alone went on sampling
    alone = _expected_stops(snaps, t, floor, min_samples, STEP, cap, 1, 1)
    assert (alone < stop).any()
    r.close()
    if name == "cornell" and size == SIZES[0]:  # the checker in rounds of STEP samples: its snapshot at each pixel's count
        _assert_same(_state_at(snaps, stop), _state_at(_checker_snapshots(oracle, cap), stop), f"checker, block {block}")


# ------------------------------------------------------------------ 3. growth 2
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("block", (1, 4))
@pytest.mark.parametrize("min_samples", (8, 10))  # (10: no multiple of the step; b0 = 12)
def test_growth_two_stops_on_the_doubling_schedule_only(monkeypatch, name, block, min_samples):
    floor, cap = 0.01, CAP_SNAP
    b0 = _b0(min_samples, STEP)
    schedule = [b0 << k for k in range(8) if b0 << k <= cap]
    snaps = _snapshots(monkeypatch, name)
    t, stop = _splitting_threshold(snaps, floor, min_samples, cap, block, 2, also=lambda s: len(set(np.unique(s).tolist()) & set(schedule)) >= 2)
    assert set(np.unique(stop).tolist()) <= set(schedule) | {cap}
    assert (stop < cap).any() and (stop == cap).any()
    assert len(set(np.unique(stop).tolist()) & set(schedule)) >= 2, "the threshold should stop blocks at more than one boundary of the schedule"
    # (growth 1 would have stopped some of them earlier, between two boundaries of the schedule)
    assert (_expected_stops(snaps, t, floor, min_samples, STEP, cap, block, 1) < stop).any()
    r, L = _context(monkeypatch, name)
    for calls in ([cap], [b0, b0, cap - 2 * b0], [3, 30, 47]):
        _fresh(r, L, _params(t, min_samples, STEP, floor), policy=(block, 2))
        _render(r, L, name, calls)
        got = _state(r, L)
        assert np.array_equal(got["count"], stop.astype(np.uint32)), f"{name}, block {block}, calls {calls}: {int((got['count'] != stop).sum())} pixels stop elsewhere"
        _assert_same(got, _state_at(snaps, stop), f"{name}, block {block}, growth 2, calls {calls}")
    r.close()


def test_next_boundary_walks_the_schedule(monkeypatch):
    r, L = _context(monkeypatch, "cornell")
    out = C.c_uint32(0)
    assert N.lib().fh_adaptive_next_boundary(r._ctx, C.byref(out)) == FH_E_INVALID  # while the mode is off
    _fresh(r, L, _params(0.0, 10, 4), policy=(1, 2))  # b0 = 12
    walked = []
    for _ in range(4):  # calls that end on boundaries: 12, 24, 48, 96
        n = r.adaptive_next_boundary()
        walked.append(n)
        _render(r, L, "cornell", [n])
    assert walked == [12, 12, 24, 48]
    assert r.adaptive_next_boundary() == 96
    _render(r, L, "cornell", [5])  # a call that ends between two boundaries: the remainder
    assert r.adaptive_next_boundary() == 91
    assert (r.sample_counts() == 101).all()
    _fresh(r, L, _params(0.0, 10, 4), policy=(4, 2))
    _render(r, L, "cornell", [13])
    assert r.adaptive_next_boundary() == 11
    _fresh(r, L, _params(0.0, 10, 4), policy=(1, 1))  # growth 1: every multiple of step >= min_samples
    assert r.adaptive_next_boundary() == 12
    _render(r, L, "cornell", [12])
    assert r.adaptive_next_boundary() == 4
    _render(r, L, "cornell", [1])
    assert r.adaptive_next_boundary() == 3
    r.close()


# ------------------------------------------------------------------ 4. how the samples are submitted changes no bit
def _sum_states(states):
    out = dict(states[0])
    for s in states[1:]:
        out["count"] = out["count"] + s["count"]
    return out


class _Environ:
    """monkeypatch's two calls on os.environ, for the child process below"""

    @staticmethod
    def setenv(k, v):
        os.environ[k] = v

    @staticmethod
    def delenv(k, raising=True):
        if raising or k in os.environ:
            del os.environ[k]


def _child_run(out, name, block, growth, threshold_hex, floor_hex, min_samples, step, cap):
    """what the child process of _run_with_pixel_block_zero runs: one frame, its state into an .npz"""
    p = _params(float.fromhex(threshold_hex), min_samples, step, float.fromhex(floor_hex))
    r, L = _context(_Environ, name)
    _fresh(r, L, p, policy=(block, growth))
    _render(r, L, name, [cap])
    np.savez(out, **_state(r, L, moments=True))
    r.close()


def _run_with_pixel_block_zero(tmp_path, name, block, growth, p, cap):
    """FH_PIXEL_BLOCK is read once per process (the order of the ownership list: rows of a tile instead of 8 x 8 blocks), so the frame is rendered by a child"""
    out = str(tmp_path / "pixel_block_zero.npz")
    here, root = os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (f"import sys; sys.path[:0] = [{root!r}, {here!r}]; import test_gpu_adaptive_policy as T; "
            f"T._child_run({out!r}, {name!r}, {block}, {growth}, {float(p.threshold).hex()!r}, {float(p.floor).hex()!r}, {p.min_samples}, {p.step}, {cap})")
    env = dict(os.environ, FH_PIXEL_BLOCK="0")
    for k in ("FH_SKY_SPLIT", "FH_PIPELINE", "FH_SKY_SPLIT_MIN_LOG2"):
        env.pop(k, None)
    run = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("block,growth", ((4, 2), (8, 1)))
def test_splitting_pipeline_lists_shards_and_groups_change_no_bit(monkeypatch, tmp_path, name, block, growth):
    floor, min_samples, cap = 0.01, 8, 48
    W, H = SIZES[0]
    snaps = _snapshots(monkeypatch, name)
    p = _params(_splitting_threshold(snaps, floor, min_samples, cap, block, growth)[0], min_samples, STEP, floor)

    def run(calls=(cap,), env=None, pool=None, flags=0, devices=None):
        r, L = _context(monkeypatch, name, env=env, pool=pool, devices=devices)
        if flags:
            r.set_flags(flags)
        _fresh(r, L, p, policy=(block, growth))
        _render(r, L, name, calls)
        s = _state(r, L, moments=True)
        r.close()
        return s

    ref = run()
    assert 0 < int((ref["count"] < cap).sum()) < W * H, "the invariance run should stop some blocks early and not all"
    assert np.array_equal(ref["count"], _expected_stops(snaps, p.threshold, floor, min_samples, STEP, cap, block, growth).astype(np.uint32))
    keys = NAMES + ("count", "m")
    _assert_same(run(calls=(5, 7, 13, 23)), ref, f"{name}: calls ending off a boundary", keys)
    _assert_same(run(calls=(1,) * cap), ref, f"{name}: 1-spp calls", keys)
    _assert_same(run(pool=2 * W * H), ref, f"{name}: small path pool", keys)
    _assert_same(run(flags=FLAG_SERIAL_PASSES), ref, f"{name}: FH_FLAG_SERIAL_PASSES", keys)
    _assert_same(run(env={"FH_PIPELINE": "0"}), ref, f"{name}: FH_PIPELINE=0", keys)
    _assert_same(run(env={"FH_PIPELINE": "2"}), ref, f"{name}: FH_PIPELINE=2", keys)
    _assert_same(run(env={"FH_SKY_SPLIT": "0"}), ref, f"{name}: FH_SKY_SPLIT=0", keys)
    _assert_same(run(env={"FH_SKY_SPLIT_MIN_LOG2": "0"}), ref, f"{name}: the sky split forced", keys)
    _assert_same(_run_with_pixel_block_zero(tmp_path, name, block, growth, p, cap), ref, f"{name}: FH_PIXEL_BLOCK=0", keys)
    for devices in ([0, 0], [0, 0, 0]):
        _assert_same(run(devices=devices), ref, f"{name}: group {devices}", keys)
    for world in (2, 3):
        ctxs = [_context(monkeypatch, name, shard=(k, world)) for k in range(world)]
        counts = np.zeros((H, W), np.uint32)
        for r, L in ctxs:
            _fresh(r, L, p, policy=(block, growth))
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
            out = DeviceBuffer(r0, W * H * fpp * 4)
            r0.unpack_shards([b.ptr for b in packed], fpp, out.ptr)
            got[layer] = out.download(np.float32, (H, W) if fpp == 1 else (H, W, 4))
            for b in packed + [out]:
                b.free()
        _assert_same(got, ref, f"{name}: tile shards of world {world}")
        for r, _ in ctxs:
            r.close()


# ------------------------------------------------------------------ 5. counters
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("block,growth", ((4, 1), (4, 2)))
def test_paths_and_active_count_follow_the_blocks(monkeypatch, name, block, growth):
    floor, min_samples, cap = 0.01, 8, 32
    W, H = SIZES[0]
    snaps = _snapshots(monkeypatch, name)
    for q in (0.5, 0.35, 0.25, 0.15, 0.08, 0.04, 0.02):  # (as _splitting_threshold, and some block must still be unconverged AT the cap: the active count below is not 0)
        t = _block_threshold(snaps, min_samples, floor, block, q)
        s = _expected_stops(snaps, t, floor, min_samples, STEP, cap, block, growth)
        if (s < cap).any() and not _converged(snaps, cap, t, floor, min_samples, STEP, block, growth)[s == cap].all():
            break
    r, L = _context(monkeypatch, name)
    _fresh(r, L, _params(t, min_samples, STEP, floor), policy=(block, growth))
    assert r.active_pixel_count() == W * H
    before = np.zeros((H, W), np.int64)
    for calls in ([3], [9], [1, 1], [18]):
        r.reset_stats()
        _render(r, L, name, calls)
        now = r.sample_counts().astype(np.int64)
        assert r.stats()["paths"] == int((now - before).sum()), f"{name}: fh_stats.paths is not the sum of the count increments after {calls}"
        before = now
    stop = _expected_stops(snaps, t, floor, min_samples, STEP, cap, block, growth)
    assert np.array_equal(before, stop)
    # at the cap every pixel sits on a boundary: the active ones are the pixels of the blocks the restated rule leaves unconverged
    want_active = int((~_converged(snaps, cap, t, floor, min_samples, STEP, block, growth) & (stop == cap)).sum())
    assert 0 < want_active < W * H
    assert r.active_pixel_count() == want_active
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


# ------------------------------------------------------------------ 6. refusals
def test_bad_policies_and_states_are_refused(monkeypatch):
    r, L = _context(monkeypatch, "cornell")
    assert r.adaptive_policy() == (1, 1)
    assert _policy(r, 4, 2) == 0  # accepted while the mode is off
    assert r.adaptive_policy() == (4, 2)
    for block, growth in ((0, 1), (3, 1), (16, 1), (5, 2), (4, 0), (4, 3), (0, 0)):
        assert _policy(r, block, growth) == FH_E_INVALID, (block, growth)
        assert r.adaptive_policy() == (4, 2)
    # it survives the mode going on and off and a change of resolution
    assert _set(r, _params(0.1, 8, 4)) == 0
    assert _set(r, None) == 0
    r.set_resolution(*SIZES[0])
    assert r.adaptive_policy() == (4, 2)
    assert _set(r, _params(0.1, 8, 4)) == 0
    assert r.adaptive_policy() == (4, 2)
    _render(r, L, "cornell", [2])
    assert _policy(r, 2, 2) == FH_E_INVALID and _policy(r, 4, 1) == FH_E_INVALID  # samples accumulated since the init
    assert r.adaptive_policy() == (4, 2)
    assert _policy(r, 4, 2) == 0  # the values it has
    r.init_render_states()
    assert _policy(r, 2, 1) == 0
    assert r.adaptive_policy() == (2, 1)
    # tiles and blocks: whichever call would let a block span two owners is the one refused
    assert N.lib().fh_set_tile_shard(r._ctx, C.c_uint32(0), C.c_uint32(1), C.c_uint32(4), C.c_uint32(4)) == 0
    assert _policy(r, 8, 1) == FH_E_INVALID
    assert r.adaptive_policy() == (2, 1)
    assert _policy(r, 4, 1) == 0
    assert N.lib().fh_set_tile_shard(r._ctx, C.c_uint32(0), C.c_uint32(1), C.c_uint32(32), C.c_uint32(32)) == 0
    assert _policy(r, 8, 1) == 0
    n_owned = r.owned_pixel_count()
    assert N.lib().fh_set_tile_shard(r._ctx, C.c_uint32(0), C.c_uint32(2), C.c_uint32(4), C.c_uint32(4)) == FH_E_INVALID
    assert N.lib().fh_set_tile_shard(r._ctx, C.c_uint32(0), C.c_uint32(1), C.c_uint32(16), C.c_uint32(12)) == FH_E_INVALID
    assert r.owned_pixel_count() == n_owned and r.adaptive_policy() == (8, 1)
    assert N.lib().fh_set_tile_shard(r._ctx, C.c_uint32(0), C.c_uint32(2), C.c_uint32(16), C.c_uint32(8)) == 0
    r.close()


def test_a_group_takes_the_policy_and_reports_a_member_that_refuses(monkeypatch):
    name, cap = "cornell", 48
    r, L = _context(monkeypatch, name, devices=[0, 0])
    try:
        assert _policy(r, 4, 2) == 0
        assert r.adaptive_policy() == (4, 2)
        for k in range(2):  # every member holds it
            m, b, g = C.c_void_p(0), C.c_uint32(0), C.c_uint32(0)
            assert N.lib().fh_ctx_member(r._ctx, C.c_uint32(k), C.byref(m)) == 0
            assert N.lib().fh_get_adaptive_policy(m, C.byref(b), C.byref(g)) == 0 and (b.value, g.value) == (4, 2)
        assert _policy(r, 3, 1) == FH_E_INVALID
        assert N.lib().fh_last_error(r._ctx).startswith(b"member 0: fh_set_adaptive_policy")
        assert r.adaptive_policy() == (4, 2)
        assert N.lib().fh_set_tile_shard(r._ctx, C.c_uint32(0), C.c_uint32(1), C.c_uint32(4), C.c_uint32(4)) == 0
        assert _policy(r, 8, 1) == FH_E_INVALID
        assert N.lib().fh_last_error(r._ctx).startswith(b"member 0: fh_set_adaptive_policy")
        assert N.lib().fh_set_tile_shard(r._ctx, C.c_uint32(0), C.c_uint32(1), C.c_uint32(32), C.c_uint32(32)) == 0
        # and the group still renders, by the policy it kept
        _fresh(r, L, _params(0.0, 8, 4))
        assert r.adaptive_next_boundary() == 8
        _render(r, L, name, [cap])
        assert (r.sample_counts() == cap).all()
    finally:
        L.free()
        r.close()


# ------------------------------------------------------------------ 7. it fixes the interior
def test_guard_blocks_fix_the_interior(monkeypatch, tmp_path):
    """The Sponza-class interior (write_sponza_gltf(detail=0.35) through the glTF loader, SPONZA_CAMERA, sun (12, 11, 9) along SPONZA_SUN with angle 1.0, Hosek
    sky 3.0 / 0.3, black background, depth 8) at 128 x 72.  Truth = 4096 spp plain.  Adaptive: threshold 0.05, floor 0.01, min_samples 64, step 16, cap 1024,
    (block, growth) = (1, 1), (4, 1), (4, 2).  Uniform: a plain frame of the adaptive run's mean spp, rounded.  Error = mean over pixels of
    ((y - y_truth) / max(y_truth, floor))^2 of the beauty luminance.  A float64 replay of the rules on the CPU checker's samples gave error(4, 1) / error(1, 1) =
    0.42, error(4, 1) / uniform = 0.95, error(4, 2) / error(1, 1) = 0.42, error(4, 2) / uniform = 0.97 and error(1, 1) / uniform = 1.98.  The bounds: <= 0.6
    against the per-pixel rule, <= 1.10 against the uniform frame.  Sampling is deterministic, so the numbers are fixed; measured on an MI355X:
    (1, 1): mean spp 828.5, 30.6 % of the pixels stopped before the cap, error 2.5371e-2 against 1.2836e-2 uniform (ratio 1.977);
    (4, 1): mean spp 935.7, 14.2 %, error 1.0758e-2 against 1.1302e-2 uniform (ratio 0.952), 0.424 of the per-pixel rule's;
    (4, 2): mean spp 948.7, 8.3 %, error 1.0742e-2 against 1.1112e-2 uniform (ratio 0.967), 0.423 of the per-pixel rule's."""
    from fredholm_amd import scenes_sponza as SS
    W, H, depth, thr, floor, cap = 128, 72, 8, 0.05, 0.01, 1024
    path = tmp_path / "interior.gltf"
    SS.write_sponza_gltf(str(path), detail=0.35)
    for k in ("FH_SKY_SPLIT", "FH_PIPELINE", "FH_SKY_SPLIT_MIN_LOG2"):
        monkeypatch.delenv(k, raising=False)
    r = F.Renderer(0)
    r.load_scene(str(path))
    r.build_ias()
    r.set_directional_light((12.0, 11.0, 9.0), SS.SPONZA_SUN, 1.0)
    r.load_arhosek_sky(3.0, 0.3)
    r.set_resolution(W, H)
    L = F.RenderLayer(r, W, H)
    cam, bg = F.Camera(**SS.SPONZA_CAMERA), (0.0, 0.0, 0.0)

    def lum(b):
        b = b.astype(np.float64)
        return b[..., 0] * 0.2126729 + b[..., 1] * 0.7151522 + b[..., 2] * 0.0721750

    def frame(n, p=None, policy=(1, 1)):
        _fresh(r, L, p, policy=policy)
        r.render(cam, bg, L, n, depth)
        r.wait_for_completion()
        return lum(L.download("beauty"))

    truth = frame(4096)
    ref = np.maximum(truth, floor)
    err, uni, spp = {}, {}, {}
    for policy in ((1, 1), (4, 1), (4, 2)):
        y = frame(cap, _params(thr, 64, 16, floor), policy)
        counts = r.sample_counts()
        early = counts < cap
        assert early.any() and not early.all(), policy
        spp[policy] = float(counts.mean())
        err[policy] = float(np.mean(((y - truth) / ref) ** 2))
        yu = frame(max(1, int(round(spp[policy]))))
        uni[policy] = float(np.mean(((yu - truth) / ref) ** 2))
        print(f"policy {policy}: mean spp {spp[policy]:.1f}, stopped early {float(early.mean()):.3f}, relative squared error {err[policy]:.4e}, "
              f"uniform at equal samples {uni[policy]:.4e}, ratio {err[policy] / uni[policy]:.3f}, against the per-pixel rule {err[policy] / err[(1, 1)]:.3f}")
    r.close()
    for policy in ((4, 1), (4, 2)):
        assert err[policy] <= 0.6 * err[(1, 1)], (policy, err[policy], err[(1, 1)])
        assert err[policy] <= 1.10 * uni[policy], (policy, err[policy], uni[policy])
