"""Importance sampling of the environment on the device (fh_set_env_sampling), against numpy restatements and float64 integrals -- the CPU checker cannot learn
this mode, so it is not the yardstick here; its elementary functions, texture unit, Hosek dome and BSDF lobes (each pinned bit for bit to the device's by the parity
suite) are what the restatement (env_sampling_model.py) and the integrals are made of.
  table and hooks   the device's table, draws and densities equal the restatement bit for bit: both test images, the Hosek dome, a constant
  sampler           2^20 draws against the quadrature of the density (chi-square), report == evaluator, the cap on draws that map back to a neighbouring cell
  unbiased          converged frames against the float64 expectation of the estimator, with and without an emitter (the light_pending route)
  variance          the measured on / off variance ratio against the predicted one
  nothing else      on then off is never-on in every layer; with the mode on, how the work is cut changes no bit"""
import ctypes as C
from statistics import NormalDist

import numpy as np
import pytest

import env_sampling_model as M
import expectation_model as E
import fredholm_amd as F
from fredholm_amd import native as N
from fredholm_amd import scenes
from test_bsdf_sampling_density import DENSITY_CASES, P_FAIL
from test_estimator_expectation import (FLOOR_HALF, REL_BIAS, TILE, _lambert, _materials, _plane, _scene, assert_unbiased, floor_hits, lens_at, pixel_means)

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H, DEPTH1 = 32, 24, 1
LAYERS = ("beauty", "position", "depth", "normal", "texcoord", "albedo")
CASES = {c[0]: c[1] for c in DENSITY_CASES}
SUN = M.sun_image()
UP = np.array([0.0, 1.0, 0.0])


def _kat(r, fn, *args):
    N.check(r._ctx, getattr(N.lib(), fn)(r._ctx, *args), fn)


def kat_table(r):
    q, cr, cm, cp = np.zeros((M.H, M.W), np.uint32), np.zeros((M.H, M.W + 1), f32), np.zeros(M.H + 1, f32), np.zeros((M.H, M.W), f32)
    _kat(r, "fh_kat_env_table", N.ptr(q), N.ptr(cr), N.ptr(cm), N.ptr(cp))
    return q, cr, cm, cp


def kat_sample(r, u, n):
    u, n = np.ascontiguousarray(u, f32), np.ascontiguousarray(n, f32)
    d, p, c = np.zeros((len(u), 3), f32), np.zeros(len(u), f32), np.zeros(len(u), np.uint32)
    _kat(r, "fh_kat_env_sample", len(u), N.ptr(u), N.ptr(n), N.ptr(d), N.ptr(p), N.ptr(c))
    return d, p, c


def kat_pdf(r, d, n):
    d, n = np.ascontiguousarray(d, f32), np.ascontiguousarray(n, f32)
    p, c = np.zeros(len(d), f32), np.zeros(len(d), np.uint32)
    _kat(r, "fh_kat_env_pdf", len(d), N.ptr(d), N.ptr(n), N.ptr(p), N.ptr(c))
    return p, c


def kat_radiance(r, d):
    d = np.ascontiguousarray(d, f32).reshape(-1, 3)
    out = np.zeros_like(d)
    _kat(r, "fh_kat_env_radiance", len(d), N.ptr(d), N.ptr(out))
    return out


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _one_texel_image():
    """1024 x 512 with a one-texel patch: by the header's formula K = ceil(1024 / 512) = 2 still; the wider images below are the ones with more sub-samples"""
    return M.sun_image(1024, 512, patch=1, elevation_deg=35.0, phi_deg=200.0)


# wider than 1024: K = 3, 4 and 5 sub-samples per cell and axis -- positions (a + 0.5) / K that are no binary fractions, and serial sums of 9, 16 and 25 terms.  A few rows suffice:
# the build evaluates the image at all 512 x 256 x K x K points whatever its height
WIDE = {"1100 x 8 (K = 3)": (1100, 8, 3), "2048 x 6 (K = 4)": (2048, 6, 4), "2300 x 5 (K = 5)": (2300, 5, 5)}


def _wide_image(name):
    w, h, k = WIDE[name]
    assert M.subsamples(w) == k
    img = M.sun_image(w, h, patch=1, elevation_deg=45.0, phi_deg=77.0)
    img[..., :3] *= (1.0 + 0.37 * np.sin(np.arange(w) * 0.731))[None, :, None].astype(f32)  # texel-to-texel variation: every sub-sample of a cell sees another value
    return img


def _environments(oracle):
    sun_dir = np.array([0.0, 1.0, 0.0], f32)  # the context's default sun
    return {"sun image": (lambda r: r.load_ibl(SUN), ("ibl", SUN)),
            "one texel of 1024 x 512": (lambda r: r.load_ibl(_one_texel_image()), ("ibl", _one_texel_image())),
            **{name: ((lambda r, name=name: r.load_ibl(_wide_image(name))), ("ibl", _wide_image(name))) for name in WIDE},
            "hosek dome": (lambda r: r.load_arhosek_sky(3.0, 0.3), ("hosek", oracle.hosek_cook(3.0, 0.3, sun_dir), sun_dir)),
            "constant": (lambda r: None, ("constant",))}


@pytest.fixture(scope="module")
def ctx():
    r = F.Renderer(0)
    yield r
    r.close()


def _reset(r):
    r.clear_ibl()
    r.clear_arhosek_sky()
    r.clear_env_sampling()
    r.set_sky_intensity(1.0)


# ---------------------------------------------------------------------------------------------------------------- table and hooks
@pytest.mark.parametrize("name", ["sun image", "one texel of 1024 x 512", *WIDE, "hosek dome", "constant"])
def test_table_and_hooks_equal_the_restatement(ctx, oracle, name):
    setup, env = _environments(oracle)[name]
    beta = 0.25
    _reset(ctx)
    setup(ctx)
    ctx.set_sky_intensity(3.0)  # (the table does not see it)
    ctx.set_env_sampling(beta)
    assert ctx.get_env_sampling() == (True, beta)
    k = M.subsamples(env[1].shape[1]) if env[0] == "ibl" else 2
    d, st = M.subsample_dirs(k, oracle)
    if env[0] != "constant":  # what the build evaluates, point by point
        assert (_bits(kat_radiance(ctx, d)) == _bits(M.radiance(env, d, oracle).reshape(-1, 3))).all()
    t = M.Table(M.weights_of(env, oracle))
    q, cr, cm, cp = kat_table(ctx)
    assert (q == t.q).all() and q.min() >= 1
    assert (_bits(cr) == _bits(t.cdf_row)).all() and (_bits(cm) == _bits(t.cdf_m)).all() and (_bits(cp) == _bits(t.cell_p)).all()
    rng = np.random.default_rng(21)
    n = 1 << 16
    u = rng.random((n, 2)).astype(f32)
    nrm = _unit(rng.normal(size=(n, 3))).astype(f32)
    nrm[: n // 4] = [0.0, 1.0, 0.0]
    ds, ps, cs, cosine = M.sample(t, beta, u, nrm, oracle)
    gd, gp, gc = kat_sample(ctx, u, nrm)
    assert 0.2 < cosine.mean() < 0.3
    assert (_bits(gd) == _bits(ds)).all() and (_bits(gp) == _bits(ps)).all() and (gc == cs).all()
    dirs = _unit(rng.normal(size=(n, 3))).astype(f32)
    pe, ce = M.pdf(t, beta, dirs, nrm, oracle)
    gp, gc = kat_pdf(ctx, dirs, nrm)
    assert (_bits(gp) == _bits(pe)).all() and (gc == ce).all()
    ctx.set_env_sampling(0.5)  # the fraction alone: the same table, the new mixture
    q2 = kat_table(ctx)[0]
    assert (q2 == q).all() and (_bits(kat_pdf(ctx, dirs, nrm)[0]) == _bits(M.pdf(t, 0.5, dirs, nrm, oracle)[0])).all()
    _reset(ctx)
    with pytest.raises(N.FredholmError):
        kat_table(ctx)


def _floor_scene(mat):
    return _scene([(_plane(0.0, FLOOR_HALF, TILE, True), 0)], _materials(mat))


def _new(sc, setup=None, w=W, h=H, **kw):
    r = F.Renderer(0, **kw) if kw else F.Renderer(0)
    r.load_scene(sc)
    r.build_ias()
    if setup:
        setup(r)
    r.set_resolution(w, h)
    return r, F.RenderLayer(r, w, h)


def _frame(r, L, cam, calls, depth, bg=(0.1, 0.2, 0.3)):
    r.init_render_states()
    for n in calls:
        r.render(cam, bg, L, n, depth)
    r.wait_for_completion()
    return {k: L.download(k) for k in LAYERS}


def _same(a, b):
    return all((np.ascontiguousarray(a[k]).view(np.uint32) == np.ascontiguousarray(b[k]).view(np.uint32)).all() for k in LAYERS)


def test_the_table_follows_load_ibl_and_clear_ibl(oracle):
    """the table a frame uses is the one of the environment it renders: after fh_load_ibl and after fh_clear_ibl a context gives the bits of a fresh context in that state"""
    sc, cam = _floor_scene(CASES["diffuse only"]), lens_at((0.0, 4.0, 0.0))
    fresh = {}
    for state, setup in (("constant", lambda r: r.set_env_sampling(0.5)), ("sun", lambda r: (r.load_ibl(SUN), r.set_env_sampling(0.5)))):
        r, L = _new(sc, setup)
        fresh[state] = _frame(r, L, cam, [4], 2)
        r.close()
    assert not _same(fresh["constant"], fresh["sun"])
    r, L = _new(sc, lambda r: r.set_env_sampling(0.5))
    assert _same(_frame(r, L, cam, [4], 2), fresh["constant"])
    r.load_ibl(SUN)
    assert _same(_frame(r, L, cam, [4], 2), fresh["sun"])
    assert (kat_table(r)[0] == M.Table(M.weights_of(("ibl", SUN), oracle)).q).all()
    r.clear_ibl()
    assert _same(_frame(r, L, cam, [4], 2), fresh["constant"])
    r.load_arhosek_sky(3.0, 0.3)
    dome = _frame(r, L, cam, [4], 2)
    r.clear_arhosek_sky()
    assert not _same(dome, fresh["constant"]) and _same(_frame(r, L, cam, [4], 2), fresh["constant"])
    r.close()


# ---------------------------------------------------------------------------------------------------------------- the sampler against its own density
def _histogram_quadrature():
    """Gauss-Legendre panels between the table's cell boundaries AND the boundaries of expectation_model.cell_of's 24 x 24 histogram (uniform in cos theta and phi): every
    panel lies in one table cell and one histogram cell, so the table density is smooth on it"""
    tb = np.concatenate([np.arange(M.H + 1) * np.pi / M.H, np.arccos(np.linspace(1.0, -1.0, 25))])
    pb = np.concatenate([np.arange(M.W + 1) * 2 * np.pi / M.W, np.linspace(0.0, 2 * np.pi, 25)])
    t, wt, _ = E._gl_panels(tb, 2)
    p, wp, _ = E._gl_panels(pb, 2)
    T, P = np.meshgrid(t, p, indexing="ij")
    dirs = np.stack([np.sin(T) * np.cos(P), np.cos(T), np.sin(T) * np.sin(P)], axis=-1).reshape(-1, 3)
    return dirs, ((wt * np.sin(t))[:, None] * wp[None, :]).ravel()


@pytest.mark.parametrize("normal", [(0.0, 1.0, 0.0), (0.6, 0.64, 0.48)], ids=["up", "tilted"])
def test_the_sampler_draws_its_density(ctx, oracle, normal, capsys):
    _reset(ctx)
    ctx.load_ibl(SUN)
    ctx.set_env_sampling(0.5)
    n = 1 << 20
    u = np.random.default_rng(31).random((n, 2)).astype(f32)
    nrm = np.tile(np.asarray(normal, f32), (n, 1))
    d, p, c = kat_sample(ctx, u, nrm)
    assert np.isfinite(d).all() and np.isfinite(p).all() and (p > 0).all() and np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0).max() < 1e-5
    # chi-square on the 24 x 24 grid against the quadrature of the evaluator, at the significance the BSDF samplers are held to
    dirs, wq = _histogram_quadrature()
    dens = kat_pdf(ctx, dirs, np.tile(np.asarray(normal, f32), (len(dirs), 1)))[0].astype(np.float64)
    expected = np.bincount(E.cell_of(dirs), weights=wq * dens, minlength=576)
    assert abs(expected.sum() - 1.0) < 1e-4
    stat, dof = E.chi2_pooled(np.bincount(E.cell_of(d), minlength=576), n * expected)
    assert E.chi2_sf(stat, dof) > P_FAIL, f"chi2 {stat:.1f} on {dof} dof"
    # the report is the evaluator's value, in every bit, wherever the direction maps back to the cell it was reported from
    pe, ce = kat_pdf(ctx, d, nrm)
    same = ce == c
    assert (_bits(pe[same]) == _bits(p[same])).all()
    table = u[:, 0] >= f32(0.5)
    share = float((~same)[table].mean())
    with capsys.disabled():
        print(f"\n[env sampling] device: {(~same).sum()} of {table.sum()} table draws map back to a neighbouring cell ({share:.2e}; cap 1e-3)")
    assert same[~table].all() and share <= 1e-3
    _reset(ctx)


# ---------------------------------------------------------------------------------------------------------------- unbiased
def _sun_radiance(r):
    return lambda world: kat_radiance(r, world).astype(np.float64)


def _render(sc, cam, w, h, spp, depth, beta, bg=(0.0, 0.0, 0.0)):
    r, L = _new(sc, lambda r: r.load_ibl(SUN), w, h)
    if beta is not None:
        r.set_env_sampling(beta)
    r.render(cam, bg, L, spp, depth)
    r.wait_for_completion()
    img = L.download("beauty")[..., :3].astype(np.float64)
    r.close()
    return img


def test_lambert_floor_under_the_sun_image_is_unbiased(ctx, oracle):
    """depth 1, mode on: the frame's mean against the float64 expectation of the estimator (env_sampling_model.first_vertex_env: both draws, their MIS weights,
    regularize_weight, L from the device at the quadrature nodes).  For a Lambertian the two weights add up to 1 wherever the sky ray can escape, so the
    expectation is the integral of f L |cos| over the upper hemisphere, which the test also asserts of the model"""
    _reset(ctx)
    ctx.load_ibl(SUN)
    ctx.set_env_sampling(0.5)
    t = M.Table(M.weights_of(("ibl", SUN), oracle))
    mat = CASES["diffuse only"]
    e, lost = M.first_vertex_env(oracle.bsdf_lobes, mat, E.wo_at(0.8), t, 0.5, _sun_radiance(ctx))
    dirs, wq = M.cell_quadrature(range(M.H // 2))
    rho = np.asarray(mat["base_color"][0], np.float64)[:3]
    direct = (wq * dirs[:, 1]) @ (rho / np.pi * kat_radiance(ctx, dirs).astype(np.float64))
    assert lost < 1e-6 and np.abs(e / direct - 1.0).max() < 1e-4
    _reset(ctx)
    cam = lens_at((0.0, 4.0, 0.0))
    expect = pixel_means(oracle, cam, W, H, 4096, lambda o, d: np.broadcast_to(e, (len(o), 3)) + 0.0 * floor_hits(o, d, FLOOR_HALF))
    assert_unbiased(_render(_floor_scene(mat), cam, W, H, 4096, DEPTH1, 0.5), expect, "diffuse only, mode on")


def test_a_sun_below_the_shading_horizon_adds_nothing(ctx, oracle):
    """The Lambertian floor with its shading normals tilted 70 degrees away from the sun patch: the patch stays above the floor's plane and falls below the shading
    horizon.  The table draws it all the same; the BSDF's evaluation is not defined down there (it answers rho / pi on both sides, other lobes NaN, which
    regularize_weight turns into a full weight), so the mode must add nothing for such a draw -- interiors with normal maps rendered the sun's whole radiance before
    it did.  Expected, by quadrature (the cosine's kink crosses cells: < 1e-4 of E): above both horizons the two draws' weights add up to 1, so the integral of
    rho / pi * L * cos there; above the shading horizon and below the floor's plane the sky ray is stopped by the floor, and the BSDF-sampled ray, which the
    reference starts on the far side of a surface it leaves downwards (pt.cu:893-925), escapes with its weight pdf / (pdf + pdf_light) alone -- pdf_light being
    |cos| / pi with the switch off and the mixture's p with it on"""
    _reset(ctx)
    ctx.load_ibl(SUN)
    t = M.Table(M.weights_of(("ibl", SUN), oracle))
    mat = CASES["diffuse only"]
    rho = np.asarray(mat["base_color"][0], np.float64)[:3]
    tilt, az = np.radians(70.0), np.radians(120.0 + 180.0)
    ns = np.array([np.sin(tilt) * np.cos(az), np.cos(tilt), np.sin(tilt) * np.sin(az)])
    dirs, wq = M.cell_quadrature(range(M.H))
    Lq = kat_radiance(ctx, dirs).astype(np.float64)
    _reset(ctx)
    cos_s = np.maximum(dirs @ ns, 0.0)
    above = dirs[:, 1] > 0
    sun = Lq[:, 1] > 0.25  # the patch and its bilinear ramp
    assert sun.any() and (dirs[sun] @ ns < 0).all() and (dirs[sun, 1] > 0.5).all()
    leak = (wq * sun * np.abs(dirs @ ns)) @ (rho / np.pi * Lq)  # what the patch would add through |cos|
    sc = _floor_scene(mat)
    sc["normals"][:] = ns.astype(f32)
    cam = lens_at((0.0, 4.0, 0.0))
    for beta in (0.5, None):
        p_b = cos_s / np.pi
        p_light = p_b if beta is None else M.mixture_density64(t, beta, dirs, ns)
        weight = np.where(above, 1.0, p_b / np.maximum(p_b + p_light, 1e-300))
        e = (wq * cos_s * weight) @ (rho / np.pi * Lq)
        assert (leak > 20.0 * REL_BIAS * e).all()
        expect = pixel_means(oracle, cam, W, H, 64, lambda o, d: np.broadcast_to(e, (len(o), 3)) + 0.0 * floor_hits(o, d, FLOOR_HALF))
        assert_unbiased(_render(sc, cam, W, H, 4096, DEPTH1, beta), expect, f"tilted shading normals, cosine fraction {beta}")


def test_a_sky_ray_whose_weight_is_not_finite_adds_nothing(ctx, oracle):
    """The Lambertian floor seen from BELOW, under the sun image turned upside down (the patch at -50 degrees).  For a hit on the back side of an opaque surface every
    lobe weight of the reference's BSDF is 0: eval is 0, the lobe pmf is 0 / 0 and eval_pdf is NaN (oracle.bsdf(mat, entering=False); asserted below), so the sky ray's
    weight is NaN, which regularize_weight (clamp01) turns into 1.  With the switch off that is a glow, 1 * L(d) for the cosine-distributed sky ray and the same for the
    BSDF-sampled ray (f = 0, pdf NaN, its direction cosine-distributed round the flipped normal).  Under the table a sky ray weighed 1 has the expectation integral of
    p * L, the patch's radiance times its share of the draws: the mode drops a sky ray whose weight is not finite and keeps the clamp for the BSDF-sampled ray, whose
    direction does not depend on the table.  This is what made the textured interior 500 x too bright (its curtains and cards are seen from both sides).
    Expected with the mode on: the light ray alone, the integral of |cos| / pi * L over the lower hemisphere, by quadrature on the table's cells.
    Bound: the frame's mean against its empirical standard error at P_FAIL over the three channels, plus 5e-4 of E for the quadrature.  Power: what an undropped sky ray
    would add, the integral of p * L over the lower hemisphere, must be above 20 of those bounds"""
    mat = CASES["diffuse only"]
    back = oracle.bsdf(mat, False, np.array([[0.6, 0.8, 0.0]], f32), np.array([[0.0, 0.8, 0.6]], f32), np.array([0.3], f32), np.array([[0.2, 0.7]], f32))[0]
    assert (back[0:3] == 0).all() and np.isnan(back[3]) and (back[7:10] == 0).all() and np.isnan(back[10]) and back[5] > 0
    flipped = np.ascontiguousarray(SUN[::-1])
    _reset(ctx)
    ctx.load_ibl(flipped)
    t = M.Table(M.weights_of(("ibl", flipped), oracle))
    dirs, wq = M.cell_quadrature(range(M.H // 2, M.H))
    Lq = kat_radiance(ctx, dirs).astype(np.float64)
    _reset(ctx)
    down = np.array([0.0, -1.0, 0.0])
    e = (wq * (-dirs[:, 1]) / np.pi) @ Lq
    undropped = (wq * M.mixture_density64(t, 0.5, dirs, down)) @ Lq
    fw = np.array([0.0, 1.0, -0.7])
    fw /= np.linalg.norm(fw)
    cam = F.Camera(origin=tuple(np.array([0.0, -4.0, 0.0]) + fw / np.tan(0.3)), forward=(0.0, 1.0, -0.7), fov=0.6, F=100.0)
    r, L = _new(_floor_scene(mat), lambda r: (r.load_ibl(flipped), r.set_env_sampling(0.5)))
    r.render(cam, (0.0, 0.0, 0.0), L, 8192, DEPTH1)
    r.wait_for_completion()
    img, normal = L.download("beauty")[..., :3].astype(np.float64).reshape(-1, 3), L.download("normal")[..., :3]
    r.close()
    assert np.isfinite(img).all() and (normal[..., 1] < -0.99).all()  # every pixel sees the floor's back: its shading normal is flipped towards the camera
    mean, se = img.mean(axis=0), img.std(axis=0, ddof=1) / np.sqrt(len(img))
    bound = NormalDist().inv_cdf(1.0 - P_FAIL / 6) * se + 5e-4 * e
    assert (undropped > 20.0 * bound).all(), (undropped, bound)
    assert (np.abs(mean - e) <= bound).all(), f"mean {mean}, expected {e}, bound {bound}"


def _narrow_camera(cos_o=0.8, azimuth=2.3, fov=0.004, dist=40.0):
    """a camera far from the floor with a field of view so narrow that wo is one direction but for a linear term over the frame; it looks at the origin"""
    s = np.sqrt(1.0 - cos_o * cos_o)
    wo_world = np.array([s * np.cos(azimuth), cos_o, s * np.sin(azimuth)])
    f = 1.0 / np.tan(0.5 * fov)
    lens = dist * wo_world
    return F.Camera(origin=tuple(lens + f * (-wo_world)), forward=tuple(-wo_world), fov=fov, F=1e6), wo_world


@pytest.mark.parametrize("name", ["anisotropy-free rough metal", "glass"])
def test_conductor_and_glass_floors_under_the_sun_image_are_unbiased(ctx, oracle, name):
    """as above for a rough conductor and the transmissive case.  Their expectation depends on wo, so the camera is far away with a field of view of 0.004: over the
    frame wo moves by 2e-3, the expectation is evaluated at the frame's corners and centre and interpolated bilinearly per camera ray, and the centre measures what
    the interpolation leaves out.  The yardstick is the estimator's expectation, not the integral of f L |cos|: for a transmissive floor the reference's
    estimator does not add up to that with the switch off either (its sky ray starts on the outer side and never reaches the lower hemisphere)"""
    _reset(ctx)
    ctx.load_ibl(SUN)
    t = M.Table(M.weights_of(("ibl", SUN), oracle))
    mat = CASES[name]
    cam, wo_c = _narrow_camera()
    spp = 8192
    pix = np.arange(W * H, dtype=np.uint32)
    rays = oracle.camera_rays(cam.params(), W, H, 1, pix, np.zeros(W * H, np.uint32)).astype(np.float64)
    wo_all = -_unit(rays[:, 3:6])
    # a basis of the wo spread about the centre: wo = wo_c + a e1 + b e2 to first order
    e1 = _unit(np.cross(UP, wo_c))
    e2 = np.cross(wo_c, e1)
    a_all, b_all = wo_all @ e1, wo_all @ e2
    a_m, b_m = 1.05 * np.abs(a_all).max(), 1.05 * np.abs(b_all).max()

    def local(wo_world):
        return _unit(wo_world) * np.array([1.0, 1.0, -1.0])  # the local frame of the +y normal: the world's with z negated

    def at(a, b):
        v, lost = M.first_vertex_env(oracle.bsdf_lobes, mat, local(wo_c + a * e1 + b * e2), t, 0.5, _sun_radiance(ctx))
        assert lost < 2e-3
        return v
    corner = {(sa, sb): at(sa * a_m, sb * b_m) for sa in (-1, 1) for sb in (-1, 1)}
    centre = at(0.0, 0.0)
    interp_centre = sum(corner.values()) / 4.0
    assert np.abs(interp_centre / centre - 1.0).max() < 2e-4, "the expectation is not bilinear over the frame"
    _reset(ctx)

    def fn(o, d):
        wo = -_unit(d)
        x, y = (wo @ e1) / a_m, (wo @ e2) / b_m
        assert (np.abs(x) <= 1.0).all() and (np.abs(y) <= 1.0).all()
        floor_hits(o, d, FLOOR_HALF)
        return sum(((1 + sa * x) * (1 + sb * y) / 4.0)[:, None] * v[None, :] for (sa, sb), v in corner.items())
    expect = pixel_means(oracle, cam, W, H, spp, fn)
    assert_unbiased(_render(_floor_scene(mat), cam, W, H, spp, DEPTH1, 0.5), expect, f"{name}, mode on")


QUAD = np.array([[-0.5, 5.0, -1.5], [0.5, 5.0, -1.5], [0.5, 5.0, -0.5], [-0.5, 5.0, -0.5]])  # a small emitter above the floor, facing down, away from the sun patch
QUAD_LE = np.array([30.0, 20.0, 10.0])


def _quad_scene(mat):
    n = np.cross(QUAD[1] - QUAD[0], QUAD[2] - QUAD[0])
    pts = [tuple(p) for p in (QUAD if n[1] < 0 else QUAD[::-1])]
    return _scene([(_plane(0.0, FLOOR_HALF, TILE, True), 0), (scenes._quad(*pts), 1)], _materials(mat, _lambert((0.0, 0.0, 0.0), tuple(QUAD_LE))))


def _covered_by_quad(x, rho, radiance_of, n_panel=8):
    """per floor point x (N, 3): the integral of f L cos over the directions the quad covers, as an area integral over the quad (2 x 2 Gauss-Legendre on n_panel^2 panels)"""
    g, wg = np.polynomial.legendre.leggauss(2)
    s = ((np.arange(n_panel)[:, None] + 0.5 * (g[None, :] + 1.0)) / n_panel).ravel()
    ws = np.tile(0.5 * wg / n_panel, n_panel)
    S, T = np.meshgrid(s, s, indexing="ij")
    y = (QUAD[0][None, :] + S.ravel()[:, None] * (QUAD[1] - QUAD[0])[None, :] + T.ravel()[:, None] * (QUAD[3] - QUAD[0])[None, :])
    area = np.linalg.norm(np.cross(QUAD[1] - QUAD[0], QUAD[3] - QUAD[0]))
    wy = (ws[:, None] * ws[None, :]).ravel() * area
    v = y[None, :, :] - x[:, None, :]
    r2 = (v * v).sum(axis=2)
    d = v / np.sqrt(r2)[:, :, None]
    geom = d[:, :, 1] * d[:, :, 1] / r2  # cos at the floor (normal +y) * cos at the quad (normal -y) / r^2
    L = radiance_of(d.reshape(-1, 3)).reshape(len(x), len(y), 3)
    return (rho / np.pi)[None, :] * ((geom * wy[None, :])[:, :, None] * L).sum(axis=1)


def test_lambert_floor_with_an_emitter_runs_the_pending_light_ray(ctx, oracle):
    """The same floor with a small emissive quad above it: the scene has emitters, so the BSDF-sampled light ray is finished by resolve_light_ray from what
    light_pending handed over (cos' = pi p(ld), f' = f |cos| / cos').  Expected: Lambert's polygon formula for the quad, plus the integral of f L cos over the
    upper hemisphere less the directions the quad covers (there the sky ray is stopped and the light ray finds the emitter; its two weights, area and BSDF, add up
    to 1 whatever the mode).
    With a wrong cos' -- say the plain |cos|, i.e. the switch's hand-over forgotten -- the miss branch would weigh the light ray by pdf / (pdf + |cos| / pi) = 1 / 2
    while the sky ray keeps p / (p + pdf): the test would see the term  integral of (1 / 2 - pdf / (pdf + p)) f L cos  over the escaping directions.  The test
    computes that term from the model and asserts that it is far above what the frame resolves, so it does fail on that mistake"""
    _reset(ctx)
    ctx.load_ibl(SUN)
    t = M.Table(M.weights_of(("ibl", SUN), oracle))
    mat = CASES["diffuse only"]
    rho = np.asarray(mat["base_color"][0], np.float64)[:3]
    rad = _sun_radiance(ctx)
    dirs, wq = M.cell_quadrature(range(M.H // 2))
    Lq = rad(dirs)
    whole = (wq * dirs[:, 1]) @ (rho / np.pi * Lq)
    p, pb = M.mixture_density64(t, 0.5, dirs, UP), dirs[:, 1] / np.pi
    missed = (wq * dirs[:, 1] * (0.5 - pb / (pb + p))) @ (rho / np.pi * Lq)  # what a light ray weighed with cos' = |cos| would add
    cam = lens_at((0.0, 4.0, 0.0))

    def fn(o, d):
        x = floor_hits(o, d, FLOOR_HALF)
        return whole[None, :] - _covered_by_quad(x, rho, rad) + (rho / np.pi)[None, :] * E.polygon_irradiance(x, UP, QUAD)[:, None] * QUAD_LE[None, :]
    expect = pixel_means(oracle, cam, W, H, 64, fn)  # (the expectation is smooth in the floor point: 64 camera rays per pixel stand for the frame's 8192)
    _reset(ctx)
    e = expect.reshape(-1, 3).mean(axis=0)
    assert (np.abs(missed) > 10.0 * REL_BIAS * e).all(), (missed, e)
    assert_unbiased(_render(_quad_scene(mat), cam, W, H, 8192, DEPTH1, 0.5), expect, "diffuse only with an emitter, mode on")


# ---------------------------------------------------------------------------------------------------------------- lower variance, against a prediction
N_SEEDS = 96


def test_the_variance_ratio_is_the_predicted_one(ctx, oracle, capsys):
    """Lambertian floor (albedo 0.8) under the sun image, depth 1, one sample per pixel: the variance over N_SEEDS frames, summed over pixels and channels, with the mode
    on and off, against env_sampling_model.lambert_floor_variance (float64 quadrature of  sum over the two draws of  integral c^2 / p - (integral c)^2).
    Margin: a sample variance over n = W * H * N_SEEDS independent values has the relative standard error sqrt((kappa - 1) / n), kappa = mu4 / var^2 the kurtosis, which
    the model gives too (per channel; the largest is used); the log of the ratio of two such variances has the standard error sqrt of the sum of the two squares.  The
    test allows Z_FAIL of those (P_FAIL, two-sided) plus 2 % for the (n - 1) / n of the per-pixel means and the model's quadrature.  Nothing of it comes from the device"""
    _reset(ctx)
    ctx.load_ibl(SUN)
    rho = (0.8, 0.8, 0.8)
    t = M.Table(M.weights_of(("ibl", SUN), oracle))
    dirs, wq = M.cell_quadrature(range(M.H // 2))
    Lq = kat_radiance(ctx, dirs).astype(np.float64)
    _reset(ctx)
    pred, kappa = {}, {}
    for mode, beta in (("on", 0.5), ("off", None)):
        mean, var, mu4 = M.lambert_floor_variance(t, beta, dirs, wq, Lq, rho)
        pred[mode], kappa[mode] = float(var.sum()), float((mu4 / var ** 2).max())
    n = W * H * N_SEEDS
    se_log = np.sqrt((kappa["on"] - 1.0) / n + (kappa["off"] - 1.0) / n)
    margin = NormalDist().inv_cdf(1.0 - P_FAIL / 2) * se_log + 0.02
    assert margin < 0.5 * abs(np.log(pred["on"] / pred["off"])), "the test could not tell the two samplers apart"
    sc, cam = _floor_scene(_lambert(rho)), lens_at((0.0, 4.0, 0.0))
    measured = {}
    for mode, beta in (("on", 0.5), ("off", None)):
        r, L = _new(sc, lambda r: r.load_ibl(SUN))
        if beta is not None:
            r.set_env_sampling(beta)
        frames = []
        cam_c, bg = cam.as_c(), np.zeros(3, f32)
        for seed in range(N_SEEDS):
            r.init_render_states()
            N.check(r._ctx, N.lib().fh_render(r._ctx, C.byref(cam_c), N.ptr(bg), C.byref(L.as_c()), 1, DEPTH1, C.c_uint32(1000 + seed)), "fh_render")
            r.wait_for_completion()
            frames.append(L.download("beauty")[..., :3].astype(np.float64))
        r.close()
        measured[mode] = float(np.var(np.stack(frames), axis=0, ddof=1).mean(axis=(0, 1)).sum())
    got, want = measured["on"] / measured["off"], pred["on"] / pred["off"]
    with capsys.disabled():
        print(f"\n[env sampling] first-vertex variance on / off, Lambert floor under the sun image: predicted {pred['on']:.3f} / {pred['off']:.1f} = {want:.5f}, "
              f"measured over {N_SEEDS} frames {measured['on']:.3f} / {measured['off']:.1f} = {got:.5f}; margin on the log ratio {margin:.3f} (kurtosis {kappa['on']:.0f} / {kappa['off']:.0f})")
    assert abs(np.log(got / want)) <= margin


# ---------------------------------------------------------------------------------------------------------------- nothing else moves
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
    r, L = _cornell(lambda r: r.load_ibl(SUN))
    never = _frame(r, L, cam, [2, 3], 4)
    r.set_env_sampling(0.5)
    on = _frame(r, L, cam, [2, 3], 4)
    r.clear_env_sampling()
    assert r.get_env_sampling() == (False, 0.5)
    after = _frame(r, L, cam, [2, 3], 4)
    r.close()
    assert _same(never, after) and not _same(never, on)
    for k in ("position", "depth", "normal", "texcoord", "albedo"):  # the mode touches radiance only
        assert (never[k].view(np.uint32) == on[k].view(np.uint32)).all(), k


def test_with_the_mode_on_how_the_work_is_cut_changes_no_bit(monkeypatch):
    """the Cornell box (emitters: light_pending; depth 5: the fused tail) under the sun image with the mode on: one call of 8 samples against the samples split into
    calls, a small path pool, one pass in flight, two tile shards put together, a two-member group on one device, and adaptive sampling at threshold 0"""
    cam = F.Camera(**scenes.CORNELL_CAMERA)

    def on(r):
        r.load_ibl(SUN)
        r.set_env_sampling(0.5)
    r, L = _cornell(on)
    want = _frame(r, L, cam, [8], 5)
    assert _same(_frame(r, L, cam, [1, 3, 4], 5), want), "split into calls"
    r.set_path_pool(W * H * 2)
    assert _same(_frame(r, L, cam, [8], 5), want), "pool size"
    r.close()
    r, L = _cornell(on, monkeypatch, {"FH_PIPELINE": "0"})
    assert _same(_frame(r, L, cam, [8], 5), want), "FH_PIPELINE=0"
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
    assert r.get_env_sampling() == (True, 0.5)
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
