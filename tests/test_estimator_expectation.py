"""Converged renders against float64 expectations of the estimator pt.cu defines (pt.cu:418-502, 680-944).

Every image test elsewhere compares the device with the checker bit for bit, and the checker is our own restatement of pt.cu, so a
misreading of the integrator made the same way on both sides passes them.  Here the rendered pixels are held to what pt.cu's
estimator adds up to in expectation, computed in float64 by tests/expectation_model.py (written from pt.cu, citing its lines):
1. a tiled floor under a constant background or a directional light along its normal, every DENSITY_CASES material: the
   first-vertex expectation by quadrature over the sphere (sky NEE, BSDF-sampled light ray, directional NEE, regularize_weight);
2. a Lambertian floor under two emissive quads, each split into two triangles of unequal area: Lambert's polygon formula (light
   pick, pdf_area, r^2 / |cos|, both MIS directions, the light ray's emissive-hit branch);
3. a grey floor under a grey emissive ceiling at several max_depth: the depth-truncated series of pt.cu's loop (roulette, throughput).
Each test compares the frame's mean residual (pixel - E) with its empirical standard error at P_FAIL, and first asserts that its
5 sigma bound is within REL_BIAS of E, so that no test passes by having no power.

The model's lobes (f_i, pmf_i * pdf_i) come from the checker's orc_bsdf_lobes, which the GPU parity suite pins bit for bit to the
device's.  Large surfaces are built from tiles of <= 20 units: on triangles of 1e3-1e4 units the error of the watertight test exceeds
ray_origin_offset's epsilon (pt.cu:405-416), the floor's own shadow, light and continuation rays hit it again, and a Lambertian
floor under a constant background renders 0.79 rho (depth 1) / 1.12 rho (depth 8) instead of rho, on both sides alike.  Where
that starts is measured by test_where_surfaces_start_to_shadow_themselves (test_trace_exact_host.py, test_gpu_trace_exact.py): no
leaving ray hits its own surface again up to a half-extent of 20 units, 0.4 % do at 100 (tilted), 11-23 % at 1e3, 28-34 % at 1e4.
"""
from statistics import NormalDist

import numpy as np
import pytest

import expectation_model as M
import fredholm_amd as F
from fredholm_amd import scenes
from fredholm_amd.native import default_materials
from test_bsdf_sampling_density import DENSITY_CASES, P_FAIL

N_CHANNELS = 3
Z_FAIL = NormalDist().inv_cdf(1.0 - P_FAIL / (2 * N_CHANNELS))  # two-sided, over the three channels
REL_BIAS = 0.005  # each test must be able to see a relative bias of 0.5 % of E at 5 sigma
REL_SLACK = 5e-4  # the model's own error: quadrature, tabulation in cos theta_o, float32 accumulation of the running mean
TILE = 10.0

# the camera's rays start at the lens, origin - f forward with f = 1 / tan(fov / 2) = 3.2 for fov = 0.6 (camera.cu:28-45): lens_at()
FOV = 0.6
FORWARD = np.array([0.0, -1.0, -0.7])


def lens_at(p):
    """a Camera whose lens centre is p, looking down at 35 degrees from the vertical"""
    f = 1.0 / np.tan(0.5 * FOV)
    fw = FORWARD / np.linalg.norm(FORWARD)
    return F.Camera(origin=tuple(np.asarray(p, np.float64) + f * fw), forward=tuple(FORWARD), fov=FOV, F=100.0)


def _plane(y, half, tile, facing_up):
    tris = []
    ks = np.arange(-half, half, tile)
    for x in ks:
        for z in ks:
            q = [(x, y, z), (x, y, z + tile), (x + tile, y, z + tile), (x + tile, y, z)]
            tris += scenes._quad(*(q if facing_up else q[::-1]))
    return tris


def _scene(parts, materials):
    tris, ids = [], []
    for t, m in parts:
        tris += t
        ids += [m] * (len(t) // 3)
    return scenes._finish(tris, ids, materials)


def _materials(*mats):
    out = default_materials(len(mats))
    for k, m in enumerate(mats):
        out[k] = m[0] if m.shape else m
    return out


def _lambert(rho, le=(0.0, 0.0, 0.0)):
    m = default_materials(1)
    m["specular"] = 0.0
    m["diffuse_roughness"] = 0.0
    m["base_color"] = rho
    m["emission_color"] = le
    return m


# ---------------------------------------------------------------------------------------------------------------- rendering
def render_checker(oracle, sc, cam, w, h, spp, depth, bg=(0.0, 0.0, 0.0), setup=None):
    S = oracle.Scene(sc)
    if setup:
        setup(S)
    L = S.new_layers(w, h)
    S.render(cam.params(), w, h, L, spp, depth, bg=bg, n_threads=8)
    return L["beauty"][..., :3].astype(np.float64)


def render_device(sc, cam, w, h, spp, depth, bg=(0.0, 0.0, 0.0), setup=None):
    r = F.Renderer(0)
    try:
        r.load_scene(sc)
        r.build_ias()
        if setup:
            setup(r)
        r.set_resolution(w, h)
        L = F.RenderLayer(r, w, h)
        r.render(cam, bg, L, spp, depth)
        r.wait_for_completion()
        return L.download("beauty")[..., :3].astype(np.float64)
    finally:
        r.close()


def pixel_means(oracle, cam, w, h, spp, fn, chunk=256):
    """per pixel: the mean of fn(origins, directions) (float64, (n, 3)) over the pixel's actual camera rays, samples 0 .. spp - 1
    (orc_camera_rays, pinned bit for bit to the device's camera)"""
    pix = np.arange(w * h, dtype=np.uint32)
    acc = np.zeros((w * h, 3))
    for s0 in range(0, spp, chunk):
        k = min(chunk, spp - s0)
        ns = np.repeat(np.arange(s0, s0 + k, dtype=np.uint32), w * h)
        r = oracle.camera_rays(cam.params(), w, h, 1, np.tile(pix, k), ns).astype(np.float64)
        acc += fn(r[:, 0:3], r[:, 3:6]).reshape(k, w * h, 3).sum(axis=0)
    return (acc / spp).reshape(h, w, 3)


def floor_hits(o, d, half):
    """hit points of camera rays on the floor y = 0; all of them must land well inside the tiled square"""
    t = -o[:, 1] / d[:, 1]
    x = o + t[:, None] * d
    assert (t > 0).all() and (np.abs(x[:, [0, 2]]) < half - TILE).all(), "a camera ray misses the floor"
    return x


def assert_unbiased(img, expect, what):
    """the frame's mean residual against its empirical standard error (P_FAIL, Bonferroni over the channels), and the test's power"""
    r = (img - expect).reshape(-1, 3)
    e = expect.reshape(-1, 3).mean(axis=0)
    n = r.shape[0]
    mean, se = r.mean(axis=0), r.std(axis=0, ddof=1) / np.sqrt(n)
    slack = REL_SLACK * e
    assert (5.0 * se + slack <= REL_BIAS * e).all(), f"{what}: no power, 5 se = {5 * se / e} of E"
    z = np.abs(mean) / np.maximum(se, 1e-300)
    assert (np.abs(mean) <= Z_FAIL * se + slack).all(), f"{what}: mean residual {mean / e} of E = {z} se (E = {e})"


# ------------------------------------------------------------------------------------------- 1. first vertex, floor, isotropic
FLOOR_HALF = 30.0
BG = np.array([0.9, 0.6, 0.3])
LE_DIR = np.array([2.0, 3.0, 4.0])
# degrees (DirectionalLight::angle, the full cone).  Both stay narrower than 2 x the smallest view angle (18 degrees), so no mirror
# direction enters the cone and the directional expectation stays smooth in cos theta_o for the tabulation
DIR_CONES = (4.0, 24.0)


class Tabulated:
    """g(cos theta_o) at Chebyshev nodes over the camera's range, interpolated by the Chebyshev polynomial through them; the
    interpolation error is measured against direct evaluations at points between the nodes"""

    def __init__(self, g, lo, hi, n, n_check=4):
        k = np.arange(n)
        self.lo, self.hi = lo, hi
        x = np.cos((2 * k + 1) * np.pi / (2 * n))
        self.c = np.stack([np.polynomial.chebyshev.chebfit(x, col, n - 1) for col in np.array([g(self._c(v)) for v in x]).T])
        t = np.cos(np.pi * (np.arange(n_check) + 0.5) / n_check * (1 - 1e-3))
        mid = 0.5 * (t[:-1] + t[1:]) if n_check > 1 else t
        self.err = max(float(np.abs(self(np.array([self._c(v)])) - g(self._c(v))).max()) for v in mid)

    def _c(self, x):
        return self.lo + 0.5 * (x + 1.0) * (self.hi - self.lo)

    def __call__(self, cos_o):
        x = 2.0 * (np.asarray(cos_o) - self.lo) / (self.hi - self.lo) - 1.0
        return np.stack([np.polynomial.chebyshev.chebval(x, c) for c in self.c], axis=-1)


def _cos_range(oracle, cam, w, h, spp):
    pix = np.arange(w * h, dtype=np.uint32)
    r = oracle.camera_rays(cam.params(), w, h, 1, np.tile(pix, 16), np.repeat(np.arange(0, spp, max(spp // 16, 1))[:16].astype(np.uint32), w * h))
    c = -r[:, 4] / np.linalg.norm(r[:, 3:6], axis=1)
    return float(c.min()) - 0.005, float(c.max()) + 0.005


def _floor_case(oracle, mat, w, h, spp, light):
    """(scene, camera, bg, setup, per-pixel expectation, clamp binds) for one material under light = "bg" or a cone angle"""
    cam = lens_at((0.0, 4.0, 0.0))
    sc = _scene([(_plane(0.0, FLOOR_HALF, TILE, True), 0)], _materials(mat))
    lo, hi = _cos_range(oracle, cam, w, h, spp)
    peaks = []
    if light == "bg":
        def g(c):
            v, peak, _ = M.first_vertex_constant_background(oracle.bsdf_lobes, mat, c)
            peaks.append(peak)
            return v * BG
        bg, setup = tuple(BG), None
    else:
        def g(c):
            v, peak = M.first_vertex_directional(oracle.bsdf_lobes, mat, c, light)
            peaks.append(peak)
            return v * LE_DIR
        bg = (0.0, 0.0, 0.0)

        def setup(x):
            x.set_directional_light(tuple(LE_DIR), (0.0, 1.0, 0.0), light)
    tab = Tabulated(g, lo, hi, 9 if light == "bg" else 33)  # the directional expectation is cheap but steep for sharp lobes

    def fn(o, d):
        floor_hits(o, d, FLOOR_HALF)
        return tab(-d[:, 1] / np.linalg.norm(d, axis=1))
    expect = pixel_means(oracle, cam, w, h, spp, fn)
    assert tab.err <= 0.5 * REL_SLACK * expect.reshape(-1, 3).mean(axis=0).min(), f"tabulation error {tab.err}"
    return sc, cam, bg, setup, expect, max(peaks) > 1.0


CLAMP_FREE = {"diffuse only", "rough diffuse", "full metal", "anisotropy-free rough metal"}  # the others' weights exceed 1 somewhere


def _ids(cases):
    return [c[0] for c in cases]


@pytest.mark.parametrize("name,mat,lobes", DENSITY_CASES, ids=_ids(DENSITY_CASES))
def test_checker_floor_under_constant_background(oracle, name, mat, lobes):
    sc, cam, bg, setup, expect, binds = _floor_case(oracle, mat, 32, 24, 512, "bg")
    assert binds == (name not in CLAMP_FREE)
    for depth in (1, 8):  # identical in expectation: the floor is convex, every continuation ray escapes and a miss adds nothing
        assert_unbiased(render_checker(oracle, sc, cam, 32, 24, 512, depth, bg=bg, setup=setup), expect, f"{name} depth {depth}")


@pytest.mark.parametrize("angle", DIR_CONES)
@pytest.mark.parametrize("name,mat,lobes", DENSITY_CASES, ids=_ids(DENSITY_CASES))
def test_checker_floor_under_directional_light(oracle, name, mat, lobes, angle):
    sc, cam, bg, setup, expect, _ = _floor_case(oracle, mat, 32, 24, 4096, angle)
    assert_unbiased(render_checker(oracle, sc, cam, 32, 24, 4096, 1, bg=bg, setup=setup), expect, f"{name} cone {angle}")


@pytest.mark.gpu
@pytest.mark.parametrize("name,mat,lobes", DENSITY_CASES, ids=_ids(DENSITY_CASES))
def test_device_floor_under_constant_background_and_directional_light(oracle, name, mat, lobes):
    sc, cam, bg, setup, expect, binds = _floor_case(oracle, mat, 64, 48, 2048, "bg")
    assert binds == (name not in CLAMP_FREE)
    for depth in (1, 8):
        assert_unbiased(render_device(sc, cam, 64, 48, 2048, depth, bg=bg, setup=setup), expect, f"{name} depth {depth}")
    for angle in DIR_CONES:
        sc, cam, bg, setup, expect, _ = _floor_case(oracle, mat, 64, 48, 4096, angle)
        assert_unbiased(render_device(sc, cam, 64, 48, 4096, 1, bg=bg, setup=setup), expect, f"{name} cone {angle}")


# --------------------------------------------------------------------------------------------------- 2. area lights, closed form
RHO_AREA = np.array([0.8, 0.6, 0.4])
# two convex quads facing down (-y), each split by the diagonal p0-p2 into triangles of unequal area
LIGHT_QUADS = [
    (np.array([[-3.0, 6.0, -4.0], [-1.0, 6.0, -4.5], [-0.5, 6.0, -1.0], [-2.5, 6.0, -2.5]]), np.array([6.0, 4.0, 3.0])),
    (np.array([[1.0, 7.0, -2.0], [2.5, 7.0, -2.2], [2.0, 7.0, -0.5], [1.2, 7.0, -1.5]]), np.array([10.0, 14.0, 20.0])),
]


def _area_scene():
    parts = [(_plane(0.0, FLOOR_HALF, TILE, True), 0)]
    mats = [_lambert(tuple(RHO_AREA))]
    for k, (q, le) in enumerate(LIGHT_QUADS):
        n = np.cross(q[1] - q[0], q[2] - q[0])
        pts = [tuple(p) for p in (q if n[1] < 0 else q[::-1])]
        parts.append((scenes._quad(*pts), k + 1))
        mats.append(_lambert((0.0, 0.0, 0.0), tuple(le)))
    return _scene(parts, _materials(*mats))


def _area_expectation(oracle, cam, w, h, spp):
    def fn(o, d):
        x = floor_hits(o, d, FLOOR_HALF)
        e = sum(M.polygon_irradiance(x, (0.0, 1.0, 0.0), q)[:, None] * le[None, :] for q, le in LIGHT_QUADS)
        return RHO_AREA / np.pi * e
    return pixel_means(oracle, cam, w, h, spp, fn)


def test_area_light_quads_are_split_unequally():
    for q, _ in LIGHT_QUADS:
        a = 0.5 * np.linalg.norm(np.cross(q[1] - q[0], q[2] - q[0]))
        b = 0.5 * np.linalg.norm(np.cross(q[2] - q[0], q[3] - q[0]))
        assert abs(a - b) > 0.2 * (a + b)


def test_checker_area_lights_against_lamberts_formula(oracle):
    sc = _area_scene()
    S = oracle.Scene(sc)
    assert S.n_lights() == 4
    cam = lens_at((0.0, 4.0, 0.0))
    expect = _area_expectation(oracle, cam, 32, 24, 2048)
    assert_unbiased(render_checker(oracle, sc, cam, 32, 24, 2048, 1), expect, "area lights")


@pytest.mark.gpu
def test_device_area_lights_against_lamberts_formula(oracle):
    cam = lens_at((0.0, 4.0, 0.0))
    expect = _area_expectation(oracle, cam, 64, 48, 4096)
    assert_unbiased(render_device(_area_scene(), cam, 64, 48, 4096, 1), expect, "area lights")


# --------------------------------------------------------------------------------------------------- 3. multiple bounces
RHO_FLOOR, RHO_CEIL, LE_CEIL = 0.7, 0.8, np.array([1.0, 2.0, 3.0])
PLANES_HALF, PLANES_GAP = 100.0, 1.0  # leak at the edges ~ (gap / half)^2 = 1e-4 per bounce, < REL_BIAS / 10
DEPTHS = (1, 2, 3, 8)


def _two_planes():
    return _scene([(_plane(0.0, PLANES_HALF, 20.0, True), 0), (_plane(PLANES_GAP, PLANES_HALF, 20.0, False), 1)],
                  _materials(_lambert((RHO_FLOOR,) * 3), _lambert((RHO_CEIL,) * 3, tuple(LE_CEIL))))


def _two_plane_expectation(oracle, cam, w, h, spp, depth):
    e = M.two_plane_radiance(RHO_FLOOR, RHO_CEIL, LE_CEIL, depth)

    def fn(o, d):
        assert (np.abs(o[:, 1] - 0.6) < 0.1).all()  # the lens lies between the planes
        floor_hits(o, d, PLANES_HALF)
        return np.broadcast_to(e, (o.shape[0], 3))
    return pixel_means(oracle, cam, w, h, spp, fn)


def test_two_plane_series_needs_every_term():
    # at max_depth 8 the floor is visited 4 times; roulette runs at depths 1 .. 7
    e = [M.two_plane_radiance(RHO_FLOOR, RHO_CEIL, 1.0, d) for d in DEPTHS]
    assert e[0] == e[1] == RHO_FLOOR and e[2] > e[1] * (1 + 10 * REL_BIAS) and e[3] > e[2] * (1 + 10 * REL_BIAS)


@pytest.mark.parametrize("depth", DEPTHS)
def test_checker_two_planes_bounce_series(oracle, depth):
    sc = _two_planes()
    cam = lens_at((0.0, 0.6, 0.0))
    expect = _two_plane_expectation(oracle, cam, 32, 24, 1024, depth)
    assert_unbiased(render_checker(oracle, sc, cam, 32, 24, 1024, depth), expect, f"two planes depth {depth}")


@pytest.mark.gpu
def test_device_two_planes_bounce_series(oracle):
    sc = _two_planes()
    cam = lens_at((0.0, 0.6, 0.0))
    for depth in DEPTHS:
        expect = _two_plane_expectation(oracle, cam, 64, 48, 4096, depth)
        assert_unbiased(render_device(sc, cam, 64, 48, 4096, depth), expect, f"two planes depth {depth}")
