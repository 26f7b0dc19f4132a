"""Scenes and predictions the light-sampling tests share (CPU only): the model scene -- the Lambertian floor of test_estimator_expectation.py under its two unequally split
quads, rescaled into a large dim panel and a small bright lamp whose powers differ by more than 50 x --, the strips of emissive triangles the table tests upload, and
the float64 prediction of the first-vertex variance with the switch on and off (light_sampling_model.py)."""
import numpy as np

import light_sampling_model as M
from fredholm_amd import scenes
from test_estimator_expectation import FLOOR_HALF, LIGHT_QUADS, RHO_AREA, TILE, _lambert, _materials, _plane, _scene

f32 = np.float32
MODEL_RHO = RHO_AREA
MODEL_X = np.array([0.5, 0.0, -1.5])
# floor points the default's rule is evaluated on: the part of the floor the tests' camera sees
MODEL_GRID = [np.array([x, 0.0, z]) for x in (-3.0, -1.5, 0.0, 1.5, 3.0) for z in (-5.0, -3.5, -2.0, -0.5)]
DIM, BRIGHT, SHRINK = 0.1, 25.0, 0.5  # the first quad's radiance x DIM; the second shrunk about its centroid by SHRINK, its radiance x BRIGHT


def model_quads(aside=0.0):
    """aside: the bright lamp moved that far along +x, at its height (above it the panel would shadow the floor the camera sees).  Its power stays, its share of the
    floor's irradiance falls: the dim panel, whose pick probability the table changes most, then carries enough of the frame for a wrong density on the BSDF-sampled ray
    to show (test_gpu_light_sampling.py, B)"""
    (q0, le0), (q1, le1) = LIGHT_QUADS
    c = q1.mean(axis=0)
    return [(q0, le0 * DIM), (c + SHRINK * (q1 - c) + np.array([aside, 0.0, 0.0]), le1 * BRIGHT)]


def _facing_down(q):
    n = np.cross(q[1] - q[0], q[2] - q[0])
    return q if n[1] < 0 else q[::-1]


def model_lights(quads=None):
    """the four emissive triangles in face order (each quad split by the diagonal p0-p2, as scenes._quad does) and their radiances"""
    tris, les = [], []
    for q, le in (model_quads() if quads is None else quads):
        p = _facing_down(q)
        tris += [np.array([p[0], p[1], p[2]]), np.array([p[0], p[2], p[3]])]
        les += [le, le]
    return tris, les


def model_scene(floor=None, quads=None):
    parts = [(_plane(0.0, FLOOR_HALF, TILE, True), 0)]
    mats = [floor if floor is not None else _lambert(tuple(MODEL_RHO))]
    for k, (q, le) in enumerate(model_quads() if quads is None else quads):
        parts.append((scenes._quad(*[tuple(p) for p in _facing_down(q)]), k + 1))
        mats.append(_lambert((0.0, 0.0, 0.0), tuple(le)))
    return _scene(parts, _materials(*mats))


def model_table(uniform, quads=None, misjudge=None):
    """misjudge: per-emitter factors on the weights, for a textured emitter whose 16 points misjudge its mean"""
    tris, les = model_lights(quads)
    t = np.array(tris, f32)
    w = M.weight(M.area(t[:, 0], t[:, 1], t[:, 2]), np.array(les, f32))
    return M.Table(w if misjudge is None else (w * np.asarray(misjudge, f32)).astype(f32), uniform)


def model_power_ratio():
    tris, les = model_lights()
    t = np.array(tris, f32)
    w = M.weight(M.area(t[:, 0], t[:, 1], t[:, 2]), np.array(les, f32)).astype(np.float64)
    return (w[2] + w[3]) / (w[0] + w[1])


def model_moments(pick_p, points, level=4, quads=None):
    """per point and channel: (mean, variance, fourth central moment), arrays (n_points, 3)"""
    tris, les = model_lights(quads)
    out = [M.lambert_floor_variance(x, (0.0, 1.0, 0.0), MODEL_RHO, tris, les, pick_p, level) for x in points]
    return tuple(np.array([o[k] for o in out]) for k in range(3))


def model_prediction(uniform, points=None, level=4, quads=None, misjudge=None):
    """variance summed over the channels and averaged over the points, on (share `uniform`) and off, and for each the term  sum over channels of
    sqrt(sum over points of (mu4 - var^2))  that bounds the standard error of that sum's estimate (the channels share their draws: full correlation assumed)"""
    points = MODEL_GRID if points is None else points
    n = len(model_lights(quads)[0])
    out = {}
    for mode, p in (("on", model_table(uniform, quads, misjudge).p.astype(np.float64)), ("off", np.full(n, 1.0 / n))):
        mean, var, mu4 = model_moments(p, points, level, quads)
        out["variance_" + mode] = float(var.sum(axis=1).mean())
        out["se_term_" + mode] = float(np.sqrt((mu4 - var ** 2).sum(axis=0)).sum() / var.sum())  # times 1 / sqrt(frames): the relative standard error
        out["mean_" + mode] = mean
    return out


# ------------------------------------------------------------------------------------------------ strips of emissive triangles
def strip(n, seed=3, zero_area_at=None):
    """n emissive triangles in a row under y = 5, facing down, areas 2^-10 .. 2^4 (corner coordinates are small dyadic numbers, so the float32 area of the header is what
    the restatement computes from them too), two emissive materials, and one Lambertian floor quad.  -> (scene, corners [n, 3, 3] float32, material index per light)"""
    rng = np.random.default_rng(seed)
    e = rng.integers(-10, 5, n)             # area = 2^e = 0.5 * base * height
    base = 2.0 ** np.ceil((e + 1) / 2.0)
    height = 2.0 ** (e + 1) / base
    x0 = np.arange(n) * 0.0078125 - 8.0       # overlapping is fine: nothing here traces a ray
    tris, ids, corners = [], [], []
    mat_of = rng.integers(1, 3, n)
    for k in range(n):
        b, h = (0.0, 0.0) if k == zero_area_at else (base[k], height[k])
        p = [(x0[k], 5.0, 0.0), (x0[k] + b, 5.0, 0.0), (x0[k], 5.0, h)]  # cross(p1 - p0, p2 - p0) points down
        tris += p
        ids.append(int(mat_of[k]))
        corners.append(p)
    fl = scenes._quad((-20.0, 0.0, -20.0), (-20.0, 0.0, 20.0), (20.0, 0.0, 20.0), (20.0, 0.0, -20.0))
    mats = [_lambert((0.5, 0.5, 0.5)), _lambert((0.0, 0.0, 0.0), (3.0, 2.0, 1.0)), _lambert((0.0, 0.0, 0.0), (0.25, 40.0, 7.0))]
    all_tris, all_ids = tris + fl, ids + [0] * (len(fl) // 3)
    sc = scenes._finish(all_tris, all_ids, _materials(*mats))
    return sc, np.array(corners, f32), mat_of, np.array([[0, 0, 0], [3.0, 2.0, 1.0], [0.25, 40.0, 7.0]], f32)
