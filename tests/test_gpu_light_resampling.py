"""Resampling of the light table's picks on the device (fh_set_light_resampling), against the numpy restatement and the float64 model (light_resampling_model.py).
  A  bits          proxies and choices equal the restatement through the hooks, on the model scene, on strips of 1 .. 1025 emitters and after set_transforms; M = 1
  B  distribution  chi-square of 2^18 choices at three points of the lamp-aside scene against the exact marginal
  C  unbiased      converged frames against Lambert's polygon formula, lamp overhead and lamp aside, M = 2 and the default; with environment sampling on as well
  D  variance      the measured first-vertex variance ratios resampled / table and resampled / off against the predicted ones
  E  nothing else  M = 1 and the switch off keep today's bits with and without light sampling; how the work is cut and traced changes no bit
The lifecycle test is tests/test_gpu_light_resampling_lifecycle.py."""
import ctypes as C
from statistics import NormalDist

import numpy as np
import pytest

import env_sampling_model as EM
import expectation_model as E
import fredholm_amd as F
import light_resampling_model as R
import light_resampling_scenes as RS
import light_sampling_model as M
import light_sampling_scenes as S
from fredholm_amd import native as N
from fredholm_amd import scenes
from test_bsdf_sampling_density import P_FAIL
from test_estimator_expectation import FLOOR_HALF, REL_BIAS, assert_unbiased, floor_hits, lens_at, pixel_means
from test_gpu_light_sampling import CASES, CONDUCTOR, LAYERS, _cornell, _frame, _model_expectation, _new, _render, _same, _strip_table, kat_pick

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H, DEPTH1 = 32, 24, 1
UP = RS.UP
U = N.LIGHT_UNIFORM_FRACTION_DEFAULT
M_DEFAULT = N.LIGHT_CANDIDATES_DEFAULT


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def kat_proxies(r, n):
    out = np.zeros((n, 8), f32)
    N.check(r._ctx, N.lib().fh_kat_light_proxies(r._ctx, N.ptr(out)), "fh_kat_light_proxies")
    return out


def kat_resample(r, so, ns, u1, u_sel):
    so, ns, u1, u_sel = (np.ascontiguousarray(a, f32) for a in (so, ns, u1, u_sel))
    idx, ratio = np.zeros(len(u1), np.uint32), np.zeros(len(u1), f32)
    N.check(r._ctx, N.lib().fh_kat_light_resample(r._ctx, len(u1), N.ptr(so), N.ptr(ns), N.ptr(u1), N.ptr(u_sel), N.ptr(idx), N.ptr(ratio)), "fh_kat_light_resample")
    return idx, ratio


def device_usel(n, dim=7, seed=0x5EED):
    px, spp, out = np.arange(n, dtype=np.uint32), (np.arange(n, dtype=np.uint32) * np.uint32(2654435761)) >> np.uint32(20), np.zeros(n, f32)
    assert N.lib().fh_kat_light_usel(n, N.ptr(px), N.ptr(np.ascontiguousarray(spp)), dim, seed, N.ptr(out)) == 0
    return out


def _points(prox, m, rng):
    from test_light_resampling_host import shaded_points
    return shaded_points(prox, m, rng, 2000)


def _check(r, table, prox, rng, ms=R.CANDIDATES):
    """proxies by value (a zero component's sign is the transform's, and G does not read it), choices and ratios bit for bit, for every M"""
    got = kat_proxies(r, table.n)
    assert got.shape == prox.shape and (got == prox).all()
    for m in ms:
        r.set_light_resampling(m)
        assert r.get_light_resampling() == (True, m)
        pts = _points(prox, m, rng)
        idx, ratio = kat_resample(r, pts[:, 0:3], pts[:, 3:6], pts[:, 6], pts[:, 7])
        _, _, want_idx, want_ratio, _ = R.resample(table, prox, pts[:, 0:3], pts[:, 3:6], pts[:, 6], pts[:, 7], m)
        assert (idx == want_idx).all() and (_bits(ratio) == _bits(want_ratio)).all(), m
        if m == 1:
            assert (ratio == 1).all() and (idx == kat_pick(r, pts[:, 6])[0]).all()
    r.clear_light_resampling()  # off: the function runs with M = 1
    pts = _points(prox, 1, rng)
    idx, ratio = kat_resample(r, pts[:, 0:3], pts[:, 3:6], pts[:, 6], pts[:, 7])
    assert (ratio == 1).all() and (idx == kat_pick(r, pts[:, 6])[0]).all()


# ---------------------------------------------------------------------------------------------------------------- A. bits
@pytest.mark.parametrize("aside", [0.0, RS.ASIDE])
def test_model_scene_proxies_and_choices_equal_the_restatement(aside):
    quads = S.model_quads(aside)
    r = F.Renderer(0)
    try:
        r.load_scene(S.model_scene(quads=quads))
        r.build_ias()
        with pytest.raises(Exception):  # light sampling off: refused
            kat_proxies(r, 4)
        r.set_light_sampling()
        assert r.get_light_resampling() == (False, M_DEFAULT)
        _check(r, S.model_table(U, quads), RS.model_proxies(quads), np.random.default_rng(1))
    finally:
        r.close()


@pytest.mark.parametrize("n", (1, 2, 257, 1025))
def test_strip_proxies_and_choices_equal_the_restatement(n):
    """strips of n emissive triangles (light_sampling_scenes.strip); the 257-strip has a zero-area emitter"""
    sc, corners, mat_of, colours = S.strip(n, seed=n, zero_area_at=100 if n == 257 else None)
    r = F.Renderer(0)
    try:
        r.load_scene(sc)
        r.build_ias()
        r.set_light_sampling(0.125)
        prox = RS.proxies_of(corners)
        if n == 257:
            prox[100, 4:7] = kat_proxies(r, n)[100, 4:7]  # (a face without area has no normal of its own: whatever unit or zero vector the upload gave it)
            assert prox[100, 3] == 0 and (np.abs(prox[100, 4:7]) <= 1).all()
        _check(r, _strip_table(corners, mat_of, colours, 0.125), prox, np.random.default_rng(n))
    finally:
        r.close()


def test_the_proxies_follow_set_transforms():
    n = 300
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
        r.set_light_sampling(0.25)
        r.set_light_resampling(8)
        rng = np.random.default_rng(1)
        _check(r, _strip_table(corners, mat_of, colours, 0.25), RS.proxies_of(corners), rng, ms=(8,))
        o2w, w2o = np.tile(ident, (2, 1)), np.tile(ident, (2, 1))
        o2w[1, [0, 5, 10]] = 2.0   # instance 1 twice as large (a power of two: the world-space corners stay exact)
        w2o[1, [0, 5, 10]] = 0.5
        r.set_transforms(o2w, w2o)
        r.build_ias()
        moved = corners.copy()
        moved[:n // 2] *= f32(2.0)
        assert not (RS.proxies_of(moved) == RS.proxies_of(corners)).all()
        _check(r, _strip_table(moved, mat_of, colours, 0.25), RS.proxies_of(moved), rng, ms=(8,))
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------------------------- B. distribution
CHI_POINTS = (np.array([-40.0, 0.0, 30.0]), np.array([-1.75, 0.0, -3.0]), S.MODEL_X)  # far from everything; under the panel; the model's point


@pytest.mark.parametrize("m", sorted({M_DEFAULT, 16}))
def test_choices_follow_the_exact_marginal(m):
    """2^18 choices per point on the lamp-aside scene, u1 uniform from numpy, u_sel the device's own light_usel: pooled chi-square at P_FAIL against the marginal"""
    quads = S.model_quads(RS.ASIDE)
    table, prox = S.model_table(U, quads), RS.model_proxies(quads)
    k = 1 << 18
    r = F.Renderer(0)
    try:
        r.load_scene(S.model_scene(quads=quads))
        r.build_ias()
        r.set_light_sampling()
        r.set_light_resampling(m)
        us = device_usel(k)
        assert (us.view(np.uint32) == R.usel(np.arange(k), (np.arange(k, dtype=np.uint32) * np.uint32(2654435761)) >> np.uint32(20), 7, 0x5EED).view(np.uint32)).all()
        for j, x in enumerate(CHI_POINTS):
            u1 = np.random.default_rng(10 + j).random(k).astype(f32)
            idx, _ = kat_resample(r, np.tile(x.astype(f32), (k, 1)), np.tile(np.array(UP, f32), (k, 1)), u1, us)
            q = R.marginal(table, R.geom64(prox, x, np.array(UP)), m)
            assert abs(q.sum() - 1.0) < 1e-12
            stat, dof = E.chi2_pooled(np.bincount(idx, minlength=table.n), q * k)
            assert E.chi2_sf(stat, dof) > P_FAIL, (x, stat, dof)
            if j == 2:
                assert np.abs(q - table.p).max() > 0.05  # (a marginal that equalled the table's would make this test blind)
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------------------------- C. unbiased
def _mistakes(quads, m):
    """from the model, per mistake: the bias of the frame mean (rgb) over the model's floor points -- dividing by pdf_area instead of pdf_area_ris, and the resampled
    density in the shade site's MIS weight only"""
    tris, les = S.model_lights(quads)
    table, prox = S.model_table(U, quads), RS.model_proxies(quads)
    good = np.array([R.floor_moments(x, UP, S.MODEL_RHO, tris, les, table, prox, m)[0][0] for x in S.MODEL_GRID]).mean(axis=0)
    return {k: np.array([R.floor_moments(x, UP, S.MODEL_RHO, tris, les, table, prox, m, mistake=k)[0][0] for x in S.MODEL_GRID]).mean(axis=0) - good for k in ("pdf_area", "one_site")}


@pytest.mark.parametrize("m", sorted({2, M_DEFAULT}))
@pytest.mark.parametrize("aside", [0.0, RS.ASIDE])
def test_lambert_floor_with_resampling_is_unbiased(oracle, aside, m, capsys):
    """depth 1, the Lambertian floor under the model lights: Lambert's polygon formula whatever M (the model shows the clamp binds nowhere: its largest unclamped
    term is 0.59).  What the frame can see of the two mistakes, from the model, as multiples of REL_BIAS x E (printed):
      lamp 15 aside, default M:  pdf_area 57 .. 156, one_site 11 .. 25  -- both at least 10 x, asserted;
      lamp 15 aside, M = 2:      pdf_area 20 .. 55 (asserted), one_site 6.7 .. 15: the blue channel stays under 10 x, red and green are over it (asserted for those);
      lamp overhead, either M:   both under 0.6 x.  The lamp carries that frame and every candidate set holds it, so G / (S / M) is nearly 1 whenever it matters and
                                 neither mistake moves the mean.  The frame is held to the formula all the same; it cannot tell the mistakes apart there."""
    cam = lens_at((0.0, 4.0, 0.0))
    w, h, spp = 64, 48, 4096
    quads = S.model_quads(aside)
    expect = _model_expectation(oracle, cam, w, h, 64, quads)
    e = expect.reshape(-1, 3).mean(axis=0)
    power = {k: np.abs(v) / (REL_BIAS * e) for k, v in _mistakes(quads, m).items()}
    with capsys.disabled():
        print(f"\n[light resampling] lamp aside {aside}, M = {m}: the mistakes as multiples of REL_BIAS x E: " + ", ".join(f"{k} {np.round(v, 2)}" for k, v in power.items()))
    if aside:
        assert (power["pdf_area"] >= 10.0).all(), power
        assert (power["one_site"] >= 10.0).all() if m == M_DEFAULT else (power["one_site"][:2] >= 10.0).all(), power
    img = _render(S.model_scene(quads=quads), cam, w, h, spp, DEPTH1, lambda r: (r.set_light_sampling(), r.set_light_resampling(m)))
    assert_unbiased(img, expect, f"model lights, lamp aside {aside}, resampling among {m}")


def test_both_sampling_switches_and_resampling_together_are_unbiased(oracle):
    """environment sampling on as well, under the SUN image of the environment tests: the expectation of tests/test_gpu_light_sampling.py's test of both switches"""
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
    img = _render(S.model_scene(), cam, w, h, spp, DEPTH1, lambda r: (r.load_ibl(SUN), r.set_env_sampling(0.5), r.set_light_sampling(), r.set_light_resampling()))
    assert_unbiased(img, expect, "model lights under the sun image, both switches and resampling on")


def test_rough_conductor_floor_with_resampling_is_held_to_its_own_expectation(oracle, capsys):
    """a rough-conductor floor (roughness 0.6) under the model lights with the lamp 15 aside, depth 1, default M: the frame against the float64 first-vertex quadrature
    of both draws over the emitters with the clamp inside and the resampled density in the area draw's division (light_resampling_model.
    first_vertex_emitters_resampled).  Whether the clamp binds anywhere in that quadrature is printed; the frame is held to the quadrature with the clamp either way"""
    cam = lens_at((0.0, 4.0, 0.0))
    quads = S.model_quads(RS.ASIDE)
    tris, les = S.model_lights(quads)
    table, prox = S.model_table(U, quads), RS.model_proxies(quads)
    pix = np.arange(W * H, dtype=np.uint32)
    acc, info, n_rays = np.zeros((W * H, 3)), {}, 4
    for s in range(n_rays):
        rays = oracle.camera_rays(cam.params(), W, H, 1, pix, np.full(W * H, s, np.uint32)).astype(np.float64)
        x = floor_hits(rays[:, 0:3], rays[:, 3:6], FLOOR_HALF)
        acc += np.array([R.first_vertex_emitters_resampled(oracle.bsdf_lobes, CASES[CONDUCTOR], -rays[k, 3:6], x[k], tris, les, table, prox, M_DEFAULT, 3, info) for k in range(W * H)])
    expect = (acc / n_rays).reshape(H, W, 3)
    img = _render(S.model_scene(CASES[CONDUCTOR], quads=quads), cam, W, H, 65536, DEPTH1, lambda r: (r.set_light_sampling(), r.set_light_resampling()))
    with capsys.disabled():
        print(f"\n[light resampling] rough-conductor floor, lamp 15 aside, M = {M_DEFAULT}: largest unclamped term of the area draw {info['clamp_max']:.4f} "
              f"(the clamp {'binds' if info['clamp_max'] > 1.0 else 'binds nowhere'}); expected frame mean {expect.reshape(-1, 3).mean(axis=0)}, rendered {img.reshape(-1, 3).mean(axis=0)}")
    assert_unbiased(img, expect, "rough-conductor floor with resampling")


# ---------------------------------------------------------------------------------------------------------------- D. variance against its prediction
N_SEEDS = 128


def test_the_variance_ratios_are_the_predicted_ones(oracle, capsys):
    """the lamp-aside scene, depth 1, one sample per pixel: the variance over N_SEEDS frames, summed over pixels and channels, of resampling (default M), the table
    alone and the switch off, against the models at every pixel's floor point.  The margin is the existing variance test's rule (tests/test_gpu_light_sampling.py):
    Z(P_FAIL) standard errors of the log ratio plus 2 %, all from the model and nothing from the device"""
    cam = lens_at((0.0, 4.0, 0.0))
    quads = S.model_quads(RS.ASIDE)
    pix = np.arange(W * H, dtype=np.uint32)
    rays = oracle.camera_rays(cam.params(), W, H, 1, pix, np.zeros(W * H, np.uint32)).astype(np.float64)
    points = list(floor_hits(rays[:, 0:3], rays[:, 3:6], FLOOR_HALF))
    base = S.model_prediction(U, points=points, level=3, quads=quads)
    ris = RS.model_prediction(M_DEFAULT, points=points, level=3, quads=quads)
    pred = {"resampled": (ris["variance"], ris["se_term"]), "table": (base["variance_on"], base["se_term_on"]), "off": (base["variance_off"], base["se_term_off"])}
    z = NormalDist().inv_cdf(1.0 - P_FAIL / 2)
    want, margin = {}, {}
    for other in ("table", "off"):
        want[other] = pred["resampled"][0] / pred[other][0]
        margin[other] = z * np.sqrt((pred["resampled"][1] ** 2 + pred[other][1] ** 2) / N_SEEDS) + 0.02
        assert margin[other] < 0.5 * abs(np.log(want[other])), f"the test could not tell resampling and {other} apart"
    setups = {"resampled": lambda r: (r.set_light_sampling(), r.set_light_resampling()), "table": lambda r: r.set_light_sampling(), "off": None}
    measured = {}
    for mode, setup in setups.items():
        r, L = _new(S.model_scene(quads=quads), setup)
        frames = []
        cam_c, bg = cam.as_c(), np.zeros(3, f32)
        for seed in range(N_SEEDS):
            r.init_render_states()
            N.check(r._ctx, N.lib().fh_render(r._ctx, C.byref(cam_c), N.ptr(bg), C.byref(L.as_c()), 1, DEPTH1, C.c_uint32(1000 + seed)), "fh_render")
            r.wait_for_completion()
            frames.append(L.download("beauty")[..., :3].astype(np.float64))
        r.close()
        measured[mode] = float(np.var(np.stack(frames), axis=0, ddof=1).mean(axis=(0, 1)).sum())
    with capsys.disabled():
        print(f"\n[light resampling] first-vertex variance, lamp 15 aside, M = {M_DEFAULT}, {N_SEEDS} frames: predicted resampled / table / off "
              f"{pred['resampled'][0]:.6f} / {pred['table'][0]:.6f} / {pred['off'][0]:.6f}, measured {measured['resampled']:.6f} / {measured['table']:.6f} / {measured['off']:.6f}; "
              f"margins on the log ratios {margin['table']:.3f}, {margin['off']:.3f}")
    for other in ("table", "off"):
        assert abs(np.log(measured["resampled"] / measured[other] / want[other])) <= margin[other], other


# ---------------------------------------------------------------------------------------------------------------- E. nothing else moves
def test_one_candidate_and_the_switch_off_keep_todays_bits():
    """all six layers: with light sampling on, M = 1 and on-then-off are the table's frame; M > 1 is not, and touches radiance only; without light sampling the
    switch changes nothing at all"""
    cam = F.Camera(**scenes.CORNELL_CAMERA)
    r, L = _cornell()
    plain = _frame(r, L, cam, [2, 3], 4)
    r.set_light_resampling(16)
    assert _same(_frame(r, L, cam, [2, 3], 4), plain), "resampling without light sampling"
    r.clear_light_resampling()
    r.set_light_sampling(0.25)
    table = _frame(r, L, cam, [2, 3], 4)
    assert not _same(table, plain)
    r.set_light_resampling(1)
    assert _same(_frame(r, L, cam, [2, 3], 4), table), "M = 1"
    r.set_light_resampling(8)
    on = _frame(r, L, cam, [2, 3], 4)
    assert not _same(on, table) and _same(on, table, ("position", "depth", "normal", "texcoord", "albedo"))
    r.clear_light_resampling()
    assert r.get_light_resampling() == (False, 8)
    assert _same(_frame(r, L, cam, [2, 3], 4), table), "on then off"
    r.clear_light_sampling()
    assert _same(_frame(r, L, cam, [2, 3], 4), plain)
    r.close()


def test_without_emitters_the_switch_changes_neither_bits_nor_launches():
    sc = scenes.cornell_box()
    sc["materials"]["emission_color"][:] = 0.0
    cam = F.Camera(**scenes.CORNELL_CAMERA)
    frames, stats = {}, {}
    for mode, setup in (("off", None), ("on", lambda r: (r.set_light_sampling(), r.set_light_resampling(16)))):
        r, L = _new(sc, setup)
        r.reset_stats()
        frames[mode] = [_frame(r, L, cam, [4], 4), _frame(r, L, cam, [1, 3], 4)]
        stats[mode] = r.stats()
        r.close()
    assert _same(frames["off"][0], frames["on"][0]) and _same(frames["off"][1], frames["on"][1])
    for k in ("n_closest_launches", "n_shadow_launches", "n_tail_launches", "n_shade_launches"):
        assert stats["on"][k] == stats["off"][k], k


def test_with_resampling_on_how_the_work_is_cut_and_traced_changes_no_bit(monkeypatch):
    """the Cornell box (two emitters, depth 5) with resampling among 8: one call of 8 samples against the samples split into calls, a small path pool, one pass in
    flight, a pinned tail depth low and high (shade and the fused tail both resample), forced streaming against the cooperative fixed-batch kernels, the binary-BVH
    fallback, two tile shards, a two-member group on one device, adaptive sampling at threshold 0"""
    cam = F.Camera(**scenes.CORNELL_CAMERA)

    def on(r):
        r.set_light_sampling(0.25)
        r.set_light_resampling(8)
    r, L = _cornell(on)
    want = _frame(r, L, cam, [8], 5)
    assert _same(_frame(r, L, cam, [1, 3, 4], 5), want), "split into calls"
    r.set_path_pool(W * H * 2)
    assert _same(_frame(r, L, cam, [8], 5), want), "pool size: four passes"
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
    assert r.get_light_resampling() == (True, 8)
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
