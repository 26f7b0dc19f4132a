"""GPU tests (-m gpu): rendered pixels against the CPU checker at high and wrapping sample indices.

The reference keys every sample's Sobol' draws by the 32-bit value image_idx + n_spp * width * height (pt.cu:386), which wraps 2^32: at 1080p from
sample 2071 on, at 4K from sample 517 on, so every frame of the benchmark's 4096- and 8192-spp configurations renders in that regime.  The other image
tests start at sample 0 and render a few samples.  Here both per-pixel counters (the running-mean count and the issued count) start wherever a test
puts them (fh_kat_set_sample_counts), from nonzero running means in all six layers, and the result has to be bit-identical to the checker's in EVERY
pixel of every layer (any two NaNs count as equal): a wrap bug changes only the pixels past the crossing, which the image tolerance of the other files
(99.9 %) would let through.  The counters read back afterwards have to equal the checker's sample_count.

The start indices: CMJ block edges (k_sky_pixels caches its draws per block of 16 samples), the benchmark's regime, the crossing inside the frame,
the second wrap, 2^24 (where (float)n stops being exact: the running means' weights) and the counter's own wrap (the reference's uint wraps too).
"""
import ctypes as C

import numpy as np
import pytest

import fredholm_amd as F
from fredholm_amd import native as N
from fredholm_amd import scenes

pytestmark = pytest.mark.gpu

W, H = 64, 48
P = W * H
WRAP = (1 << 32) // P  # 1398101: image_idx + WRAP * P crosses 2^32 at image_idx 1024
STARTS = [15, 16, 17, 517, 518, 2071, 2072, 8190, WRAP - 1, WRAP, WRAP + 1, 2 * WRAP + 1, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, 0xFFFFFFFE]
CALLS = (1, 3, 17)  # from a start of 15 the calls cross a block of sixteen samples inside a call
NAMES = F.RenderLayer.NAMES


@pytest.fixture(params=["auto", "stream"])
def traversal(request, monkeypatch):
    """the library's own choice of traversal kernels, and the streaming kernels forced (FH_STREAM=1, read when a context is created)"""
    if request.param == "stream":
        monkeypatch.setenv("FH_STREAM", "1")
    else:
        monkeypatch.delenv("FH_STREAM", raising=False)
    return request.param


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_every_pixel(gpu, ref, name, what):
    """every pixel of layer `name` bit-identical (any two NaNs equal); the first differing pixel is reported by its index in the flattened arrays"""
    gpu, ref = np.asarray(gpu, np.float32), np.asarray(ref, np.float32)
    eq = (_bits(gpu) == _bits(ref)) | (np.isnan(gpu) & np.isnan(ref))
    bad = np.flatnonzero(~eq.reshape(-1, 1 if name == "depth" else 4).all(axis=1))
    assert bad.size == 0, f"{what}, {name}: {bad.size} pixels differ, the first at pixel {bad[0]}"


def _set_counts(r, counts):
    c = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
    N.check(r._ctx, N.lib().fh_kat_set_sample_counts(r._ctx, N.ptr(c), C.c_uint32(c.size)), "fh_kat_set_sample_counts")


def _counts(r, w, h):
    sc, iss = np.empty((h, w), np.uint32), np.empty((h, w), np.uint32)
    N.check(r._ctx, N.lib().fh_kat_sample_counts(r._ctx, N.ptr(sc), N.ptr(iss), C.c_uint32(w * h)), "fh_kat_sample_counts")
    return sc, iss


def _preload(seed, w, h):
    """nonzero, finite running means for the six layers (the same arrays go to both sides)"""
    rng = np.random.default_rng(seed)
    out = {}
    for name in NAMES:
        shape = (h, w) if name == "depth" else (h, w, 4)
        out[name] = rng.random(shape, dtype=np.float32) * np.float32(2.95) + np.float32(0.05)
    return out


def _upload(r, L, layers):
    r.wait_for_completion()
    for name in NAMES:
        L._bufs[name].upload(layers[name])


def _download(L):
    return {name: L.download(name) for name in NAMES}


def _hosek(x, oracle):
    x.set_directional_light((0.0, 0.0, 0.0), scenes.SOUP_SUN, 0.0)
    if isinstance(x, F.Renderer):
        x.clear_directional_light()
    else:
        oracle.lib().orc_set_directional_light(x.h, 0, None, None, C.c_float(0))
    x.load_arhosek_sky(3.0, 0.3)


# the small-frame scenes: (scene, camera, background, depth, sky + sun setup, environment of the context)
def _small_scene(name):
    if name == "cornell":  # NEE + MIS: every path goes k_generate -> k_shade -> k_accumulate
        return scenes.cornell_box(), F.Camera(**scenes.CORNELL_CAMERA), (0.0, 0.0, 0.0), 5, False, {}
    if name == "soup_sky":  # thin lens + Hosek sky; the sky-pixel split forced for small calls, so k_sky_pixels and the passes both run
        cam = F.Camera(origin=(0.4, 0.2, 4.0), fov=1.2, F=16.0, focus=4.0, forward=(-0.15, -0.05, -1.0))
        return scenes.triangle_soup(3000, 0.1), cam, (0.05, 0.1, 0.2), 5, True, {"FH_SKY_SPLIT_MIN_LOG2": "0"}
    if name == "textured":  # cut-outs
        return scenes.textured_cornell_box(), F.Camera(**scenes.CORNELL_CAMERA), (0.1, 0.2, 0.4), 4, False, {}
    if name == "cornell_towards_light":  # the bug-compat mode's scene: directly visible emitters
        cam = F.Camera(origin=(0.0, 1.2, 0.0), fov=0.5 * np.pi, F=100.0, focus=1e4, forward=(0.0, 1.0, -0.001))
        return scenes.cornell_box(), cam, (0.1, 0.2, 0.4), 4, False, {}
    raise KeyError(name)


_SCENES = {}
_REF = {}


def _scene(name):
    if name not in _SCENES:
        _SCENES[name] = _small_scene(name)
    return _SCENES[name]


def _checker(oracle, name):
    if ("scene", name) not in _REF:
        sc, _, _, _, sky, _ = _scene(name)
        S = oracle.Scene(sc)
        if sky:
            _hosek(S, oracle)
        _REF[("scene", name)] = S
    return _REF[("scene", name)]


def _reference(oracle, name, start, seed, w=W, h=H, calls=CALLS, one_launch=False):
    """the checker from the preload of `seed` at per-pixel start indices `start` (an int or an (h, w) array); k one-sample launches per call of k samples
    (the library's definition of n_samples = k), or one launch of k samples (one_launch: the bug-compat mode)"""
    key = (name, start if np.isscalar(start) else start.tobytes(), seed, w, h, calls, one_launch)
    if key not in _REF:
        _, cam, bg, depth, _, _ = _scene(name)
        S = _checker(oracle, name)
        Lo = S.new_layers(w, h)
        for k, v in _preload(seed, w, h).items():
            Lo[k][...] = v
        Lo["sample_count"][...] = start
        for n in calls:
            for _ in range(1 if one_launch else n):
                S.render(cam.params(), w, h, Lo, n if one_launch else 1, depth, bg=bg, n_threads=8)
        _REF[key] = Lo
    return _REF[key]


def _context(monkeypatch, name, pool=None, w=W, h=H):
    sc, cam, bg, depth, sky, env = _scene(name)
    monkeypatch.delenv("FH_SKY_SPLIT", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = F.Renderer(0)
    for k in env:
        monkeypatch.delenv(k)
    if pool:
        r.set_path_pool(pool)
    r.load_scene(sc)
    r.build_ias()
    if sky:
        _hosek(r, None)
    r.set_resolution(w, h)
    return r, F.RenderLayer(r, w, h)


def _render_from(r, L, name, start, seed, w=W, h=H, check_issued_per_call=False):
    _, cam, bg, depth, _, _ = _scene(name)
    _upload(r, L, _preload(seed, w, h))
    counts = np.broadcast_to(np.asarray(start, np.uint32), (h, w))
    _set_counts(r, counts)
    done = counts.copy()
    for n in CALLS:
        r.render(cam, bg, L, n, depth)
        if check_issued_per_call:
            sc, iss = _counts(r, w, h)
            done = done + np.uint32(n)
            assert np.array_equal(iss, sc) and np.array_equal(sc, done), f"start {start}: the counters drift apart after a call of {n}"
    r.wait_for_completion()
    return _download(L), _counts(r, w, h)


def _compare(gpu, counts, ref, what):
    for name in NAMES:
        _assert_every_pixel(gpu[name], ref[name], name, what)
    sc, iss = counts
    assert np.array_equal(sc, ref["sample_count"]), f"{what}: sample_count differs from the checker's"
    assert np.array_equal(iss, ref["sample_count"]), f"{what}: the issued count differs from the checker's sample_count"


# ------------------------------------------------------------------ the hook itself
def test_sample_count_hook_checks_its_arguments_and_is_reset_by_the_library():
    r = F.Renderer(0)
    r.load_scene(scenes.cornell_box())
    r.build_ias()
    c = np.arange(12, dtype=np.uint32)
    assert N.lib().fh_kat_set_sample_counts(r._ctx, N.ptr(c), C.c_uint32(12)) == N.lib().fh_kat_sample_counts(r._ctx, None, None, C.c_uint32(12)) == -1  # before fh_set_resolution
    r.set_resolution(4, 3)
    assert N.lib().fh_kat_set_sample_counts(r._ctx, N.ptr(c), C.c_uint32(11)) == -1
    assert N.lib().fh_kat_set_sample_counts(r._ctx, None, C.c_uint32(12)) == -1
    assert N.lib().fh_kat_sample_counts(r._ctx, None, None, C.c_uint32(13)) == -1
    _set_counts(r, c + np.uint32(0xFFFFFFF0))
    sc, iss = _counts(r, 4, 3)
    assert np.array_equal(sc, (c + np.uint32(0xFFFFFFF0)).reshape(3, 4)) and np.array_equal(iss, sc)
    only = np.zeros(12, np.uint32)
    N.check(r._ctx, N.lib().fh_kat_sample_counts(r._ctx, None, N.ptr(only), C.c_uint32(12)), "fh_kat_sample_counts")
    assert np.array_equal(only, c + np.uint32(0xFFFFFFF0))
    r.init_render_states()
    assert all((a == 0).all() for a in _counts(r, 4, 3))
    _set_counts(r, c + 1)
    r.set_resolution(3, 4)
    assert all((a == 0).all() for a in _counts(r, 3, 4))
    r.close()


# ------------------------------------------------------------------ a. one start index for the whole frame
@pytest.mark.parametrize("name", ["cornell", "soup_sky", "textured"])
def test_uniform_start_index_matches_checker(oracle, monkeypatch, traversal, name):
    r, L = _context(monkeypatch, name)
    r.reset_stats()
    for i, s in enumerate(STARTS):
        gpu, counts = _render_from(r, L, name, s, seed=i)
        _compare(gpu, counts, _reference(oracle, name, s, seed=i), f"{name}, start {s}")
    if name == "soup_sky":
        assert r.stats()["sky_pixel_samples"] > 0  # k_sky_pixels did render some of these pixels
    r.close()


# ------------------------------------------------------------------ b. a start index of its own per pixel
@pytest.mark.parametrize("name", ["cornell", "soup_sky", "textured"])
def test_per_pixel_start_indices_match_checker(oracle, monkeypatch, traversal, name):
    """lanes of one wave and pixels of one 8 x 8 block hold different indices and different numbers of wraps"""
    start = np.random.default_rng(5).choice(np.asarray(STARTS, np.uint32), size=(H, W)).astype(np.uint32)
    r, L = _context(monkeypatch, name)
    gpu, counts = _render_from(r, L, name, start, seed=99)
    _compare(gpu, counts, _reference(oracle, name, start, seed=99), f"{name}, per-pixel starts")
    r.close()


# ------------------------------------------------------------------ c. calls of many passes
@pytest.mark.parametrize("poison", [False, True])
def test_many_passes_per_call_at_high_start_indices(oracle, monkeypatch, traversal, poison):
    """a pool of one path per pixel: a call of 17 samples is 17 passes, with k_bump_issued between them; both counters agree after every call"""
    if poison:
        monkeypatch.setenv("FH_POISON", "1")
    else:
        monkeypatch.delenv("FH_POISON", raising=False)
    r, L = _context(monkeypatch, "cornell", pool=P)
    for i, s in enumerate(STARTS):
        gpu, counts = _render_from(r, L, "cornell", s, seed=i, check_issued_per_call=True)
        _compare(gpu, counts, _reference(oracle, "cornell", s, seed=i), f"small pool, start {s}")
    assert r.stats()["n_passes"] >= len(STARTS) * sum(CALLS)
    r.close()


# ------------------------------------------------------------------ d. one rank of a tile split
def test_tile_shard_at_a_wrapping_start_index(oracle, monkeypatch, traversal):
    rank, world, tw, th = 1, 3, 16, 16
    r, L = _context(monkeypatch, "cornell")
    r.set_tile_shard(rank, world, tw, th)
    s = WRAP
    gpu, (sc, iss) = _render_from(r, L, "cornell", s, seed=7)
    ref = _reference(oracle, "cornell", s, seed=7)
    ys, xs = np.mgrid[0:H, 0:W]
    own = ((xs // tw + (W // tw) * (ys // th)) % world == rank)
    assert own.sum() == r.owned_pixel_count() and own.reshape(-1)[1024:].any() and own.reshape(-1)[:1024].any()  # owned pixels on both sides of the crossing
    pre = _preload(7, W, H)
    for name in NAMES:
        _assert_every_pixel(gpu[name][own], ref[name][own], name, "owned pixels")
        assert np.array_equal(_bits(gpu[name][~own]), _bits(pre[name][~own])), f"unowned pixels, {name}"
    assert np.array_equal(sc[own], ref["sample_count"][own]) and np.array_equal(iss[own], ref["sample_count"][own])
    assert (sc[~own] == s).all() and (iss[~own] == s).all()
    r.close()


# ------------------------------------------------------------------ e. the bug-compat mode
def test_reference_firsthit_mode_at_a_wrapping_start_index(oracle, monkeypatch, traversal):
    """FH_FLAG_REFERENCE_FIRSTHIT: a call of k samples is ONE reference launch of k samples; a pool of 4 samples per pixel, so that the carried state crosses passes
    (as test_gpu_parity.py: test_reference_firsthit_bug_compat_mode)"""
    name = "cornell_towards_light"
    r, L = _context(monkeypatch, name, pool=P * 4)
    r.set_flags(N.FLAG_REFERENCE_FIRSTHIT)
    for i, s in enumerate((WRAP, 0xFFFFFFFE)):
        gpu, counts = _render_from(r, L, name, s, seed=20 + i)
        _compare(gpu, counts, _reference(oracle, name, s, seed=20 + i, one_launch=True), f"bug-compat mode, start {s}")
    r.close()


# ------------------------------------------------------------------ f. the benchmark's frame sizes
def _crossing_row(w, h, start, n):
    """the row of the first pixel whose sample index crosses 2^32 within samples start .. start + n - 1, or None"""
    for k in range(n):
        base = ((start + k) * w * h) % (1 << 32)
        if base + w * h > (1 << 32):
            return ((1 << 32) - base) // w
    return None


@pytest.mark.parametrize("w,h,depth,start", [(3840, 2160, 16, 517), (3840, 2160, 16, 8190), (1920, 1080, 8, 2071), (1920, 1080, 8, 4095)],
                         ids=["4k-517", "4k-8190", "1080p-2071", "1080p-4095"])
def test_benchmark_frame_sizes_at_their_sample_indices(oracle, w, h, depth, start):
    """configs[4] (4K, depth 16) and configs[3] (1080p, depth 8) frame sizes with an emitter soup under the Hosek sky, two samples from `start`; the checker on
    a crop of rows that holds the 2^32 crossing where one falls inside the frame (517 at 4K: row 1761; 2071 at 1080p: row 282)"""
    sc = scenes.soup_with_emitters(20000, 0.08)
    cam = F.Camera(**dict(scenes.SOUP_CAMERA, origin=(0.0, 0.0, 1.5)))  # (closer than configs[4]'s camera: the soup fills rows 282 of 1080 and 1761 of 2160, which the crops hold)
    row = _crossing_row(w, h, start, 2)
    assert row == {(3840, 517): 1761, (1920, 2071): 282}.get((w, start))
    rows = (row - 1, row + 2) if row is not None else (h // 2 - 1, h // 2 + 1)
    r = F.Renderer(0)
    r.load_scene(sc)
    r.build_ias()
    _hosek(r, oracle)
    r.set_resolution(w, h)
    L = F.RenderLayer(r, w, h)
    pre = _preload(start, w, h)
    _upload(r, L, pre)
    _set_counts(r, np.full((h, w), start, np.uint32))
    r.render(cam, (0.0, 0.0, 0.0), L, 2, depth)
    r.wait_for_completion()
    gpu = _download(L)
    sc_, iss = _counts(r, w, h)
    r.close()
    assert (sc_ == start + 2).all() and (iss == start + 2).all()
    S = oracle.Scene(sc)
    _hosek(S, oracle)
    Lo = S.new_layers(w, h)
    for k, v in pre.items():
        Lo[k][...] = v
    Lo["sample_count"][...] = start
    for _ in range(2):
        S.render(cam.params(), w, h, Lo, 1, depth, n_threads=oracle.hardware_threads(), rows=rows)
    y0, y1 = rows
    for name in NAMES:
        _assert_every_pixel(gpu[name][y0:y1], Lo[name][y0:y1], name, f"{w}x{h} from {start}, rows {rows}")
    assert (Lo["sample_count"][y0:y1] == start + 2).all()
    first = S.new_layers(w, h)  # (one sample from empty layers: the crop's camera rays do hit the soup)
    S.render(cam.params(), w, h, first, 1, 1, n_threads=oracle.hardware_threads(), rows=rows)
    assert (first["depth"][y0:y1] > 0).mean() > 0.2


# ------------------------------------------------------------------ g. the regime reached by rendering, without the hook
def test_sample_2071_of_config2_reached_by_rendering(oracle):
    """configs[2] (1M-triangle soup, Hosek sky, 1080p, depth 8): 2071 samples in calls of 16 and a remainder, as the rtcamp8 driver renders, then two more,
    whose first crosses 2^32 at image_idx 541696 (row 282).  A second context started from the downloaded state through the hook gives the same bits, and so
    does the checker on rows 280 - 284."""
    w, h, depth, n0 = 1920, 1080, 8, 2071
    sc = scenes.triangle_soup(1_000_000)
    cam = F.Camera(**scenes.SOUP_CAMERA)
    bg = (0.0, 0.0, 0.0)
    assert _crossing_row(w, h, n0, 1) == 282

    def context():
        r = F.Renderer(0)
        r.load_scene(sc)
        r.build_ias()
        _hosek(r, oracle)
        r.set_resolution(w, h)
        return r, F.RenderLayer(r, w, h)

    r, L = context()
    for n in [16] * (n0 // 16) + [n0 % 16]:
        r.render(cam, bg, L, n, depth)
    r.wait_for_completion()
    sc_, iss = _counts(r, w, h)
    assert (sc_ == n0).all() and (iss == n0).all()
    state = _download(L)
    r.render(cam, bg, L, 2, depth)
    r.wait_for_completion()
    a = _download(L)
    sc_, iss = _counts(r, w, h)
    assert (sc_ == n0 + 2).all() and (iss == n0 + 2).all()
    r.close()
    r2, L2 = context()
    _upload(r2, L2, state)
    _set_counts(r2, np.full((h, w), n0, np.uint32))
    r2.render(cam, bg, L2, 2, depth)
    r2.wait_for_completion()
    b = _download(L2)
    r2.close()
    for name in NAMES:
        _assert_every_pixel(b[name], a[name], name, "state set through the hook")
    S = oracle.Scene(sc)
    _hosek(S, oracle)
    Lo = S.new_layers(w, h)
    for k, v in state.items():
        Lo[k][...] = v
    Lo["sample_count"][...] = n0
    rows = (280, 285)
    for _ in range(2):
        S.render(cam.params(), w, h, Lo, 1, depth, bg=bg, n_threads=oracle.hardware_threads(), rows=rows)
    for name in NAMES:
        _assert_every_pixel(a[name][rows[0]:rows[1]], Lo[name][rows[0]:rows[1]], name, f"rows {rows}")
