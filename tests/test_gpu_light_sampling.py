"""Sampling of area lights by power on the device (fh_set_light_sampling), against the numpy restatement and float64 expectations (light_sampling_model.py) -- the CPU
checker has no counterpart of this mode, so it is not the yardstick here; its camera and its texture unit (each pinned bit for bit to the device's by the parity suite)
are what the expectations and the textured emitter's mean are made of.
  A  table and pick   the device's table and picks equal the restatement bit for bit through the two hooks; the table follows set_transforms and load_scene; chi-square
  B  unbiased         converged frames, on and off, against Lambert's polygon formula; with environment sampling on as well; a rough-conductor floor on against off
  C  variance         the measured on / off variance ratio against the predicted one
  D  nothing else     on then off is never-on in every layer; without emitters nothing changes; with the mode on, how the work is cut and traced changes no bit
The lifecycle test (E) is tests/test_gpu_light_sampling_lifecycle.py."""
import ctypes as C
from statistics import NormalDist

import numpy as np
import pytest

import env_sampling_model as EM
import expectation_model as E
import fredholm_amd as F
import light_sampling_model as M
import light_sampling_scenes as S
from fredholm_amd import native as N
from fredholm_amd import scenes
from test_bsdf_sampling_density import DENSITY_CASES, P_FAIL
from test_estimator_expectation import FLOOR_HALF, REL_BIAS, assert_unbiased, floor_hits, lens_at, pixel_means

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H, DEPTH1 = 32, 24, 1
LAYERS = ("beauty", "position", "depth", "normal", "texcoord", "albedo")
CASES = {c[0]: c[1] for c in DENSITY_CASES}
UP = (0.0, 1.0, 0.0)
K_BLOCK = 256  # lights.hip: lanes of a workgroup = emitters of a chunk of the scan.  1, 2: one partial chunk; 257: two; 1025: five; 65 537: 257 chunks, two rounds of the chunk-sum scan
STRIPS = (1, 2, K_BLOCK + 1, 4 * K_BLOCK + 1, K_BLOCK * K_BLOCK + 1)
FH_E_INVALID = -1


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def kat_table(r, n):
    q, cdf, p, total = np.zeros(n, np.uint32), np.zeros(n + 1, f32), np.zeros(n, f32), C.c_uint64(0)
    N.check(r._ctx, N.lib().fh_kat_light_table(r._ctx, N.ptr(q), N.ptr(cdf), N.ptr(p), C.byref(total)), "fh_kat_light_table")
    return q, cdf, p, int(total.value)


def kat_pick(r, u1):
    u1 = np.ascontiguousarray(u1, f32)
    k, p = np.zeros(len(u1), np.uint32), np.zeros(len(u1), f32)
    N.check(r._ctx, N.lib().fh_kat_light_pick(r._ctx, len(u1), N.ptr(u1), N.ptr(k), N.ptr(p)), "fh_kat_light_pick")
    return k, p


def _draws(t, rng, n=20000):
    U = t.uniform
    below = lambda x: np.nextafter(f32(x), f32(-1))
    on_cdf = (U + (f32(1) - U) * t.cdf[rng.integers(0, t.n + 1, 64)]).astype(f32)
    u1 = np.concatenate([np.array([0.0, below(U), U, below(1.0), 0.5], f32), on_cdf, below(on_cdf), rng.random(n).astype(f32)])
    return u1[(u1 >= 0) & (u1 < 1)]


def _check_table(r, t, rng):
    q, cdf, p, total = kat_table(r, t.n)
    assert (q == t.q).all() and q.min() >= 1 and total == t.total
    assert (_bits(cdf) == _bits(t.cdf)).all() and (_bits(p) == _bits(t.p)).all()
    u1 = _draws(t, rng)
    k, pk = kat_pick(r, u1)
    wk, wp = t.pick(u1)
    assert (k == wk).all() and (_bits(pk) == _bits(wp)).all()


def _strip_table(corners, mat_of, colours, U):
    return M.Table(M.weight(M.area(corners[:, 0], corners[:, 1], corners[:, 2]), colours[mat_of]), U)


# ---------------------------------------------------------------------------------------------------------------- A. table and pick
@pytest.mark.parametrize("n", STRIPS)
def test_table_and_pick_equal_the_restatement(n):
    """strips of n emissive triangles, areas 2^-10 .. 2^4, two emissive materials; the 257-strip has a zero-area emitter"""
    U = 0.125
    sc, corners, mat_of, colours = S.strip(n, seed=n, zero_area_at=100 if n == K_BLOCK + 1 else None)
    r = F.Renderer(0)
    try:
        r.load_scene(sc)
        r.build_ias()
        for hook in (lambda: kat_table(r, n), lambda: kat_pick(r, [0.5])):  # off: refused
            with pytest.raises(Exception):
                hook()
        r.set_light_sampling(U)
        assert r.get_light_sampling() == (True, U)
        t = _strip_table(corners, mat_of, colours, U)
        if n == K_BLOCK + 1:
            assert t.q[100] == 1
        _check_table(r, t, np.random.default_rng(n))
        r.set_light_sampling(0.5)  # the share alone: everything is rebuilt
        _check_table(r, _strip_table(corners, mat_of, colours, 0.5), np.random.default_rng(n + 1))
    finally:
        r.close()


def test_the_table_follows_set_transforms_and_load_scene():
    n, U = 300, 0.25
    sc, corners, mat_of, colours = S.strip(n, seed=5)
    inst = np.zeros(sc["indices"].shape[0], np.uint32)
    inst[:n // 2] = 1
    sc["instance_ids"] = inst
    ident = np.asarray([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], f32)
    sc["object_to_world"], sc["world_to_object"] = np.tile(ident, (2, 1)), np.tile(ident, (2, 1))
    r = F.Renderer(0)
    try:
        r.load_scene(sc)
        r.build_ias()
        r.set_light_sampling(U)
        rng = np.random.default_rng(1)
        _check_table(r, _strip_table(corners, mat_of, colours, U), rng)
        o2w, w2o = np.tile(ident, (2, 1)), np.tile(ident, (2, 1))
        o2w[1, [0, 5, 10]] = 2.0   # instance 1 twice as large (a power of two: the world-space corners stay exact): its emitters' areas x 4
        w2o[1, [0, 5, 10]] = 0.5
        r.set_transforms(o2w, w2o)
        r.build_ias()
        moved = corners.copy()
        moved[:n // 2] *= f32(2.0)
        t = _strip_table(moved, mat_of, colours, U)
        assert not (t.q == _strip_table(corners, mat_of, colours, U).q).all()
        _check_table(r, t, rng)
        sc2, corners2, mat2, colours2 = S.strip(77, seed=9)  # another scene: other counts of emitters and faces
        r.load_scene(sc2)
        r.build_ias()
        _check_table(r, _strip_table(corners2, mat2, colours2, U), rng)
    finally:
        r.close()


def test_a_textured_emitter_weighs_the_mean_over_the_stated_points(oracle):
    """scenes.textured_cornell_box(): the light's emission is an sRGB checker; the mean over the 16 barycentric points through the checker's texture unit"""
    sc = scenes.textured_cornell_box()
    U = 0.25
    lights = [f for f in range(sc["indices"].shape[0]) if sc["materials"]["emission_texture_id"][sc["material_ids"][f]] >= 0 or np.any(sc["materials"]["emission_color"][sc["material_ids"][f]] > 0)]
    r = F.Renderer(0)
    try:
        r.load_scene(sc)
        r.build_ias()
        assert r.n_lights() == len(lights) == 2
        r.set_light_sampling(U)
        cols, corners = [], []
        for f in lights:
            m = sc["materials"][sc["material_ids"][f]]
            tex = sc["textures"][int(m["emission_texture_id"])]
            idx = sc["indices"][f]
            uv = sc["texcoords"][idx]
            fetch = lambda tu, tv: oracle.tex2d(tex["rgba8"], tex["srgb"], np.array([[tu, tv]], f32))[0, :3]
            cols.append(M.mean_emission(fetch, uv[0], uv[1], uv[2]))
            corners.append(sc["vertices"][idx])
        corners = np.array(corners, f32)
        t = M.Table(M.weight(M.area(corners[:, 0], corners[:, 1], corners[:, 2]), np.array(cols, f32)), U)
        _check_table(r, t, np.random.default_rng(2))
    finally:
        r.close()


def test_picks_follow_pick_p():
    """2^20 picks on the 1025-light strip against pick_p: pooled chi-square at P_FAIL"""
    n, U = 4 * K_BLOCK + 1, 0.25
    sc, corners, mat_of, colours = S.strip(n, seed=n)
    r = F.Renderer(0)
    try:
        r.load_scene(sc)
        r.build_ias()
        r.set_light_sampling(U)
        t = _strip_table(corners, mat_of, colours, U)
        m = 1 << 20
        k, p = kat_pick(r, np.random.default_rng(4).random(m).astype(f32))
    finally:
        r.close()
    assert abs(float(t.p.astype(np.float64).sum()) - 1.0) < 1e-4
    x, dof = E.chi2_pooled(np.bincount(k, minlength=n), t.p.astype(np.float64) * m)
    assert E.chi2_sf(x, dof) > P_FAIL, (x, dof)


def test_the_hooks_refuse_a_scene_without_emitters():
    r = F.Renderer(0)
    try:
        sc = scenes.cornell_box()
        sc["materials"]["emission_color"][:] = 0.0
        r.load_scene(sc)
        r.build_ias()
        r.set_light_sampling()
        assert r.get_light_sampling() == (True, N.LIGHT_UNIFORM_FRACTION_DEFAULT) and r.n_lights() == 0
        q = np.zeros(4, np.uint32)
        assert N.lib().fh_kat_light_table(r._ctx, N.ptr(q), None, None, None) == FH_E_INVALID
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------------------------- B. unbiased
def _new(sc, setup=None, w=W, h=H, **kw):
    r = F.Renderer(0, **kw) if kw else F.Renderer(0)
    r.load_scene(sc)
    r.build_ias()
    if setup:
        setup(r)
    r.set_resolution(w, h)
    return r, F.RenderLayer(r, w, h)


def _render(sc, cam, w, h, spp, depth, setup, bg=(0.0, 0.0, 0.0)):
    r, L = _new(sc, setup, w, h)
    r.render(cam, bg, L, spp, depth)
    r.wait_for_completion()
    img = L.download("beauty")[..., :3].astype(np.float64)
    r.close()
    return img


ASIDE = 15.0  # B's scene: the bright lamp 15 to the side (light_sampling_scenes.model_quads)


def _model_expectation(oracle, cam, w, h, spp, quads):
    def fn(o, d):
        x = floor_hits(o, d, FLOOR_HALF)
        e = sum(E.polygon_irradiance(x, UP, q)[:, None] * le[None, :] for q, le in quads)
        return S.MODEL_RHO / np.pi * e
    return pixel_means(oracle, cam, w, h, spp, fn)


def _missed_bias(points, quads=None):
    """the mistake these tests must catch: resolve_light_ray left on 1 / (n * area) while shade uses P_k.  The light ray's weight is then pdf / (pdf + p_uniform), the two
    MIS weights no longer add up to 1, and the frame gains  integral of (w_b(uniform) - w_b(P)) f L cos  over the emitters: from the model, the BSDF draw's mean under the
    uniform pick minus its mean under the table's, per point and channel"""
    tris, les = S.model_lights(quads)
    n = len(tris)
    P = S.model_table(N.LIGHT_UNIFORM_FRACTION_DEFAULT, quads).p.astype(np.float64)
    out = []
    for x in points:
        on = M.lambert_floor_moments(x, UP, S.MODEL_RHO, tris, les, P, 4)[1][0]
        off = M.lambert_floor_moments(x, UP, S.MODEL_RHO, tris, les, np.full(n, 1.0 / n), 4)[1][0]
        out.append(off - on)
    return np.array(out)


def test_the_model_scene_has_a_small_bright_and_a_large_dim_emitter():
    assert S.model_power_ratio() >= 50.0
    qs = S.model_quads()
    area = lambda q: 0.5 * (np.linalg.norm(np.cross(q[1] - q[0], q[2] - q[0])) + np.linalg.norm(np.cross(q[2] - q[0], q[3] - q[0])))
    assert area(qs[0][0]) > 4.0 * area(qs[1][0])


@pytest.mark.parametrize("mode", ["on", "off"])
def test_lambert_floor_under_the_model_lights_is_unbiased(oracle, mode):
    """depth 1: Lambert's polygon formula whatever the pick distribution (on a Lambertian floor with rho <= 1 the clamp never binds: the model asserts it).  The test
    provably fails on a resolve_light_ray left on the uniform density: that bias, from the model, is far above what the frame resolves.  (With the lamp at the panel's
    side the panel carries 2 % of the frame and the lamp's light rays weigh next to nothing either way: the term is 1 % of E there.  Hence the lamp moved aside)"""
    cam = lens_at((0.0, 4.0, 0.0))
    w, h, spp = 64, 48, 4096
    quads = S.model_quads(ASIDE)
    expect = _model_expectation(oracle, cam, w, h, 64, quads)  # (smooth in the floor point: 64 camera rays per pixel stand for the frame's)
    e = expect.reshape(-1, 3).mean(axis=0)
    missed = _missed_bias(S.MODEL_GRID, quads).mean(axis=0)
    assert (np.abs(missed) > 10.0 * REL_BIAS * e).all(), (missed, e)
    setup = (lambda r: r.set_light_sampling()) if mode == "on" else None
    assert_unbiased(_render(S.model_scene(quads=quads), cam, w, h, spp, DEPTH1, setup), expect, "model lights, switch " + mode)


def test_both_switches_together_are_unbiased(oracle):
    """environment sampling on as well, under the SUN image of the environment tests: the emitters' part is Lambert's formula, the sky's part the integral of f L cos
    over the directions the quads leave free, both as tests/test_gpu_env_sampling.py has them for its one quad"""
    SUN = EM.sun_image()
    cam = lens_at((0.0, 4.0, 0.0))
    w, h, spp = 64, 48, 8192
    r = F.Renderer(0)
    try:
        r.load_ibl(SUN)
        dirs, wq = EM.cell_quadrature(range(EM.H // 2))
        d32 = np.ascontiguousarray(dirs, f32).reshape(-1, 3)
        Lq = np.zeros_like(d32)
        N.check(r._ctx, N.lib().fh_kat_env_radiance(r._ctx, len(d32), N.ptr(d32), N.ptr(Lq)), "fh_kat_env_radiance")

        def rad(d):
            d = np.ascontiguousarray(d, f32).reshape(-1, 3)
            out = np.zeros_like(d)
            N.check(r._ctx, N.lib().fh_kat_env_radiance(r._ctx, len(d), N.ptr(d), N.ptr(out)), "fh_kat_env_radiance")
            return out.astype(np.float64)
        rho = S.MODEL_RHO
        whole = (wq * dirs[:, 1]) @ (rho / np.pi * Lq.astype(np.float64))

        def covered(x):
            total = np.zeros((len(x), 3))
            for tri, _ in zip(*S.model_lights()):
                y, dA = M.triangle_quadrature(tri, 3)
                v = y[None, :, :] - x[:, None, :]
                r2 = (v * v).sum(axis=2)
                d = v / np.sqrt(r2)[:, :, None]
                geom = d[:, :, 1] * d[:, :, 1] / r2
                total += (rho / np.pi)[None, :] * ((geom * dA[None, :])[:, :, None] * rad(d).reshape(len(x), len(y), 3)).sum(axis=1)
            return total

        def fn(o, d):
            x = floor_hits(o, d, FLOOR_HALF)
            e = sum(E.polygon_irradiance(x, UP, q)[:, None] * le[None, :] for q, le in S.model_quads())
            return whole[None, :] - covered(x) + rho / np.pi * e
        expect = pixel_means(oracle, cam, w, h, 16, fn)
    finally:
        r.close()
    img = _render(S.model_scene(), cam, w, h, spp, DEPTH1, lambda r: (r.load_ibl(SUN), r.set_env_sampling(0.5), r.set_light_sampling()))
    assert_unbiased(img, expect, "model lights under the sun image, both switches on")


CONDUCTOR = "anisotropy-free rough metal"


def _conductor_expectation(oracle, cam, w, h, pick_p, n_rays=4):
    """per pixel, the mean over its first n_rays camera rays of light_sampling_model.first_vertex_emitters at the floor point and the direction it is seen from
    (the expectation is smooth in both: four rays stand for the frame's)"""
    tris, les = S.model_lights()
    pix = np.arange(w * h, dtype=np.uint32)
    acc = np.zeros((w * h, 3))
    for s in range(n_rays):
        rays = oracle.camera_rays(cam.params(), w, h, 1, pix, np.full(w * h, s, np.uint32)).astype(np.float64)
        x = floor_hits(rays[:, 0:3], rays[:, 3:6], FLOOR_HALF)
        acc += np.array([M.first_vertex_emitters(oracle.bsdf_lobes, CASES[CONDUCTOR], -rays[k, 3:6], x[k], tris, les, pick_p, 3) for k in range(w * h)])
    return (acc / n_rays).reshape(h, w, 3)


@pytest.mark.parametrize("mode", ["on", "off"])
def test_rough_conductor_floor_is_held_to_its_own_expectation(oracle, mode, capsys):
    """a rough-conductor floor (roughness 0.6) under the model lights, depth 1: the frame against the float64 first-vertex quadrature of both draws over the emitters,
    with the clamp inside the integral and the pick probabilities of the mode -- the table's with the switch on, 1 / n with it off.  Where the clamp binds the
    expectation depends on the pick (include/fredholm_hip.h states the limit), so each mode is held to its own; the two expectations are printed"""
    cam = lens_at((0.0, 4.0, 0.0))
    n = len(S.model_lights()[0])
    P = S.model_table(N.LIGHT_UNIFORM_FRACTION_DEFAULT).p.astype(np.float64) if mode == "on" else np.full(n, 1.0 / n)
    expect = _conductor_expectation(oracle, cam, W, H, P)
    setup = (lambda r: r.set_light_sampling()) if mode == "on" else None
    img = _render(S.model_scene(CASES[CONDUCTOR]), cam, W, H, 65536, DEPTH1, setup)
    with capsys.disabled():
        print(f"\n[light sampling] rough-conductor floor under the model lights, switch {mode}: expected frame mean {expect.reshape(-1, 3).mean(axis=0)}, rendered {img.reshape(-1, 3).mean(axis=0)}")
    assert_unbiased(img, expect, "rough-conductor floor, switch " + mode)


# ---------------------------------------------------------------------------------------------------------------- C. variance against its prediction
N_SEEDS = 64


def test_the_variance_ratio_is_the_predicted_one(oracle, capsys):
    """the model scene, depth 1, one sample per pixel: the variance over N_SEEDS frames, summed over pixels and channels, on and off, against
    light_sampling_model.lambert_floor_variance at every pixel's floor point.  Margin: the sample variance of n values has the variance (mu4 - var^2) / n; the sum over
    the pixels of a channel adds those, and the three channels share their draws, so their standard errors are added (full correlation assumed); the log of the ratio of
    two such sums has the standard error sqrt of the sum of the two relative squares.  The test allows Z(P_FAIL) of those plus 2 % for the (n - 1) / n of the per-pixel
    means, the pixel footprint and the model's quadrature.  Nothing of it comes from the device"""
    cam = lens_at((0.0, 4.0, 0.0))
    pix = np.arange(W * H, dtype=np.uint32)
    rays = oracle.camera_rays(cam.params(), W, H, 1, pix, np.zeros(W * H, np.uint32)).astype(np.float64)
    points = floor_hits(rays[:, 0:3], rays[:, 3:6], FLOOR_HALF)
    pred = S.model_prediction(N.LIGHT_UNIFORM_FRACTION_DEFAULT, points=list(points), level=3)
    want = pred["variance_on"] / pred["variance_off"]
    se_log = np.sqrt((pred["se_term_on"] ** 2 + pred["se_term_off"] ** 2) / N_SEEDS)
    margin = NormalDist().inv_cdf(1.0 - P_FAIL / 2) * se_log + 0.02
    assert margin < 0.5 * abs(np.log(want)), "the test could not tell the two samplers apart"
    measured = {}
    for mode in ("on", "off"):
        r, L = _new(S.model_scene(), (lambda r: r.set_light_sampling()) if mode == "on" else None)
        frames = []
        cam_c, bg = cam.as_c(), np.zeros(3, f32)
        for seed in range(N_SEEDS):
            r.init_render_states()
            N.check(r._ctx, N.lib().fh_render(r._ctx, C.byref(cam_c), N.ptr(bg), C.byref(L.as_c()), 1, DEPTH1, C.c_uint32(1000 + seed)), "fh_render")
            r.wait_for_completion()
            frames.append(L.download("beauty")[..., :3].astype(np.float64))
        r.close()
        measured[mode] = float(np.var(np.stack(frames), axis=0, ddof=1).mean(axis=(0, 1)).sum())
    got = measured["on"] / measured["off"]
    with capsys.disabled():
        print(f"\n[light sampling] first-vertex variance on / off, Lambert floor under the model lights: predicted {pred['variance_on']:.5f} / {pred['variance_off']:.5f} = {want:.5f}, "
              f"measured over {N_SEEDS} frames {measured['on']:.5f} / {measured['off']:.5f} = {got:.5f}; margin on the log ratio {margin:.3f}")
    assert abs(np.log(got / want)) <= margin


# ---------------------------------------------------------------------------------------------------------------- D. nothing else moves
def _frame(r, L, cam, calls, depth, bg=(0.1, 0.2, 0.3)):
    r.init_render_states()
    for n in calls:
        r.render(cam, bg, L, n, depth)
    r.wait_for_completion()
    return {k: L.download(k) for k in LAYERS}


def _same(a, b, layers=LAYERS):
    return all((np.ascontiguousarray(a[k]).view(np.uint32) == np.ascontiguousarray(b[k]).view(np.uint32)).all() for k in layers)


def _cornell(setup=None, monkeypatch=None, env=None, **kw):
    if env:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    r, L = _new(scenes.cornell_box(), setup, **kw)
    if env:
        for k in env:
            monkeypatch.delenv(k)
    return r, L


def test_on_then_off_is_never_on_in_all_six_layers():
    cam = F.Camera(**scenes.CORNELL_CAMERA)
    r, L = _cornell()
    never = _frame(r, L, cam, [2, 3], 4)
    r.set_light_sampling(0.25)
    on = _frame(r, L, cam, [2, 3], 4)
    r.clear_light_sampling()
    assert r.get_light_sampling() == (False, 0.25)
    after = _frame(r, L, cam, [2, 3], 4)
    r.close()
    assert _same(never, after) and not _same(never, on)
    assert _same(never, on, ("position", "depth", "normal", "texcoord", "albedo"))  # the mode touches radiance only


def test_without_emitters_the_switch_changes_neither_bits_nor_launches():
    """two fresh contexts (what a pass launches depends on what earlier passes of its context measured), one with the switch on"""
    sc = scenes.cornell_box()
    sc["materials"]["emission_color"][:] = 0.0
    cam = F.Camera(**scenes.CORNELL_CAMERA)
    frames, stats = {}, {}
    for mode, setup in (("off", None), ("on", lambda r: r.set_light_sampling())):
        r, L = _new(sc, setup)
        r.reset_stats()
        frames[mode] = [_frame(r, L, cam, [4], 4), _frame(r, L, cam, [1, 3], 4)]
        stats[mode] = r.stats()
        r.close()
    assert _same(frames["off"][0], frames["on"][0]) and _same(frames["off"][1], frames["on"][1])
    for k in ("n_closest_launches", "n_shadow_launches", "n_tail_launches", "n_shade_launches"):
        assert stats["on"][k] == stats["off"][k], k


def test_with_the_mode_on_how_the_work_is_cut_and_traced_changes_no_bit(monkeypatch):
    """the Cornell box (two emitters, depth 5) with the mode on: one call of 8 samples against the samples split into calls (a one-pass call takes the merged launch where
    the streaming kernels trace), a small path pool (several passes), one pass in flight, a pinned tail depth low and high (shade and the fused tail both shade), forced
    streaming against the cooperative fixed-batch kernels, the binary-BVH fallback, two tile shards, a two-member group on one device, adaptive sampling at threshold 0.
    A secondary-ray family whose twin was forgotten keeps the uniform density while shade uses the table: its frame differs from the others here"""
    cam = F.Camera(**scenes.CORNELL_CAMERA)

    def on(r):
        r.set_light_sampling(0.25)
    r, L = _cornell(on)
    want = _frame(r, L, cam, [8], 5)
    assert _same(_frame(r, L, cam, [1, 3, 4], 5), want), "split into calls"
    r.set_path_pool(W * H * 2)
    assert _same(_frame(r, L, cam, [8], 5), want), "pool size: four passes"
    r.close()
    r, L = _cornell()
    assert not _same(_frame(r, L, cam, [8], 5), want)
    r.close()
    for env in ({"FH_PIPELINE": "0"}, {"FH_TAIL_DEPTH": "1"}, {"FH_TAIL_DEPTH": "8"}, {"FH_STREAM": "1"}, {"FH_STREAM": "1", "FH_MERGE": "0"}, {"FH_STREAM": "0"}, {"FH_COOP": "0"}, {"FH_BVH2": "1"},
                {"FH_STREAM": "1", "FH_TAIL_DEPTH": "8"}):
        r, L = _cornell(on, monkeypatch, env)
        assert _same(_frame(r, L, cam, [8], 5), want), env
        assert _same(_frame(r, L, cam, [1, 3, 4], 5), want), (env, "split into calls")
        r.close()
    parts = []
    for rank in range(2):
        r, L = _cornell(lambda r: (on(r), r.set_tile_shard(rank, 2, 8, 8)))
        parts.append(_frame(r, L, cam, [8], 5))
        r.close()
    from fredholm_amd import distributed as D
    for k in LAYERS:
        got = np.zeros_like(want[k]).reshape(W * H, -1)
        for rank in range(2):
            own = D.tile_ownership(W, H, rank, 2, 8, 8)
            got[own] = parts[rank][k].reshape(W * H, -1)[own]
        assert (got.view(np.uint32) == want[k].reshape(W * H, -1).view(np.uint32)).all(), f"tile shards: {k}"
    r = F.Renderer(devices=[0, 0])
    r.load_scene(scenes.cornell_box())
    r.build_ias()
    on(r)
    r.set_resolution(W, H)
    L = F.RenderLayer(r, W, H)
    assert r.get_light_sampling() == (True, 0.25)
    assert _same(_frame(r, L, cam, [8], 5), want), "a two-member group on one device"
    r.close()
    r, L = _cornell(on)
    r.init_render_states()
    r.set_adaptive_sampling(0.0, min_samples=4, step=4)
    r.render(cam, (0.1, 0.2, 0.3), L, 8, 5)
    r.wait_for_completion()
    got = {k: L.download(k) for k in LAYERS}
    r.close()
    assert _same(got, want), "adaptive sampling at threshold 0"
