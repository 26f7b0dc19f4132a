"""Sampling of area lights by power (fh_set_light_sampling), restated in numpy from the paragraph of include/fredholm_hip.h -- not from csrc/fh_lights.h, with which it
shares no code -- bit for bit in float32: weights, quantisation, CDF, pick probabilities and the pick.  And a float64 model of what the mode is for: the first-vertex
variance of a Lambertian floor under emissive triangles for a given pick distribution, with the kurtosis a variance-ratio test sizes its margin by."""
import numpy as np

f32 = np.float32
QUANT = f32(1048576.0)
BELOW_ONE = f32(0.99999994)
N_POINTS = 16


# ------------------------------------------------------------------------------------------------ the arithmetic of the header, float32
def points():
    """the 16 barycentric points (bu, bv), in the header's order"""
    out = []
    for j in range(4):
        for i in range(4 - j):
            out.append((f32(3 * i + 1) / f32(12.0), f32(3 * j + 1) / f32(12.0)))
    for j in range(3):
        for i in range(3 - j):
            out.append((f32(3 * i + 2) / f32(12.0), f32(3 * j + 2) / f32(12.0)))
    assert len(out) == N_POINTS
    return out


def point_coordinate(t0, t1, t2, bu, bv):
    """(bw * t0 + bu * t1) + bv * t2 with bw = 1 - bu - bv, float32 throughout"""
    t0, t1, t2 = f32(t0), f32(t1), f32(t2)
    bw = f32(f32(f32(1.0) - bu) - bv)
    return f32(f32(f32(bw * t0) + f32(bu * t1)) + f32(bv * t2))


def mean_emission(fetch, uv0, uv1, uv2):
    """per channel the serial sum of fetch(tu, tv) -> (r, g, b) float32 over the 16 points, divided by 16"""
    s = np.zeros(3, f32)
    for bu, bv in points():
        s = (s + np.asarray(fetch(point_coordinate(uv0[0], uv1[0], uv2[0], bu, bv), point_coordinate(uv0[1], uv1[1], uv2[1], bu, bv)), f32)).astype(f32)
    return (s / f32(N_POINTS)).astype(f32)


def area(p0, p1, p2):
    """0.5f * length(cross(p1 - p0, p2 - p0)), arrays of shape (n, 3), every product and sum rounded to float32 in the order written"""
    p0, p1, p2 = (np.asarray(p, f32) for p in (p0, p1, p2))
    a, b = (p1 - p0).astype(f32), (p2 - p0).astype(f32)

    def m(x, y):
        return (x * y).astype(f32)
    c = np.stack([(m(a[:, 1], b[:, 2]) - m(a[:, 2], b[:, 1])).astype(f32), (m(a[:, 2], b[:, 0]) - m(a[:, 0], b[:, 2])).astype(f32),
                  (m(a[:, 0], b[:, 1]) - m(a[:, 1], b[:, 0])).astype(f32)], axis=1)
    d = ((m(c[:, 0], c[:, 0]) + m(c[:, 1], c[:, 1])).astype(f32) + m(c[:, 2], c[:, 2])).astype(f32)
    with np.errstate(invalid="ignore"):
        return (f32(0.5) * np.sqrt(d).astype(f32)).astype(f32)


def finite(x):
    x = np.asarray(x, f32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x) | (np.abs(x) > f32(3.0e38)), f32(0.0), x).astype(f32)


def weight(a, e):
    """a: (n,) areas; e: (n, 3) emission colours -> (n,) weights"""
    a, e = np.asarray(a, f32), np.asarray(e, f32)
    r, g, b = finite(e[:, 0]), finite(e[:, 1]), finite(e[:, 2])
    with np.errstate(invalid="ignore", over="ignore"):
        l = ((r * f32(0.2126729)).astype(f32) + (g * f32(0.7151522)).astype(f32)).astype(f32)
        l = (l + (b * f32(0.0721750)).astype(f32)).astype(f32)
        l = np.fmax(l, f32(0.0)).astype(f32)
        return np.fmin((a * l).astype(f32), f32(3.0e38)).astype(f32)


class Table:
    def __init__(self, w, uniform):
        w = np.asarray(w, f32)
        self.n = n = int(w.size)
        self.uniform = U = f32(uniform)
        w_max = f32(0.0)
        for x in (w.max(initial=f32(0.0)),):
            w_max = np.fmax(w_max, x)
        if w_max > 0:
            with np.errstate(invalid="ignore"):
                q = ((w / w_max).astype(f32) * QUANT).astype(f32)
            q = np.maximum(q.astype(np.int64), 1).astype(np.uint32)
        else:
            q = np.ones(n, np.uint32)
        self.q = q
        self.total = T = int(q.astype(np.uint64).sum())
        run = np.concatenate([[0], np.cumsum(q.astype(np.uint64))]).astype(np.uint64)
        self.cdf = (run.astype(np.float64) / np.float64(T)).astype(f32)
        assert self.cdf[0] == 0 and self.cdf[n] == 1
        share = (q.astype(np.float64) / np.float64(T)).astype(f32)
        self.p = (((f32(1.0) - U) * share).astype(f32) + U / f32(n)).astype(f32)

    def pick(self, u1):
        """u1: (m,) float32 draws -> (index, reported probability)"""
        u1 = np.asarray(u1, f32)
        n, U = self.n, self.uniform
        with np.errstate(invalid="ignore", divide="ignore"):
            uu = (u1 / U).astype(f32)
            k_uni = np.minimum((uu * f32(n)).astype(f32).astype(np.int64), n - 1)
            ut = np.fmin(((u1 - U).astype(f32) / (f32(1.0) - U)).astype(f32), BELOW_ONE).astype(f32)
        lo, hi = np.zeros(u1.size, np.int64), np.full(u1.size, n, np.int64)
        while True:
            go = hi - lo > 1
            if not go.any():
                break
            mid = (lo + hi) >> 1
            le = self.cdf[mid] <= ut
            lo = np.where(go & le, mid, lo)
            hi = np.where(go & ~le, mid, hi)
        k = np.where(u1 < U, k_uni, lo)
        return k.astype(np.uint32), self.p[k]


def refused(uniform):
    u = f32(uniform)
    return not (u > 0 and u <= 1)


# ------------------------------------------------------------------------------------------------ the float64 model
def triangle_quadrature(tri, level=5):
    """centroids and areas of the 4^level congruent pieces of a triangle (3, 3)"""
    tri = np.asarray(tri, np.float64)
    n = 2 ** level
    pts, k = [], 0
    for j in range(n):
        for i in range(n - j):
            pts.append(((i + 1 / 3) / n, (j + 1 / 3) / n))
            if i + j < n - 1:
                pts.append(((i + 2 / 3) / n, (j + 2 / 3) / n))
    b = np.array(pts)
    x = tri[0] + b[:, :1] * (tri[1] - tri[0]) + b[:, 1:] * (tri[2] - tri[0])
    a = 0.5 * np.linalg.norm(np.cross(tri[1] - tri[0], tri[2] - tri[0]))
    return x, np.full(len(x), a / len(x))


def lambert_floor_moments(x, normal, rho, tris, les, pick_p, level=5):
    """raw moments 1 .. 4 of the two first-vertex draws at floor point x (Lambertian, albedo rho (3,)) under emissive triangles tris [(3, 3)] facing the floor with
    radiance les [(3,)], the emitter picked with probability pick_p[k]: ((m1..m4 of the area draw), (m1..m4 of the BSDF-sampled light ray)), each (4, 3).
    Both draws are integrals over the emitters' area: the area draw has density P_k / area_k there, the BSDF draw cos / pi * |cos_l| / r^2."""
    x, normal, rho = np.asarray(x, np.float64), np.asarray(normal, np.float64), np.asarray(rho, np.float64)
    ma, mb = np.zeros((4, 3)), np.zeros((4, 3))
    for tri, le, P in zip(tris, les, pick_p):
        tri = np.asarray(tri, np.float64)
        y, dA = triangle_quadrature(tri, level)
        A = dA.sum()
        nl = np.cross(tri[1] - tri[0], tri[2] - tri[0])
        nl /= np.linalg.norm(nl)
        d = y - x
        r2 = (d * d).sum(axis=1)
        w = d / np.sqrt(r2)[:, None]
        cos = np.maximum(w @ normal, 0.0)
        cosl = np.abs(w @ nl)
        p_area = r2 / cosl * (P / A)       # solid-angle density of the area draw
        p_bsdf = cos / np.pi
        live = cos > 0
        wa = np.where(live, p_area / (p_area + p_bsdf), 0.0)
        wb = np.where(live, p_bsdf / (p_area + p_bsdf), 0.0)
        # contributions (per channel): clamp01(w f cos / p) * Le with f = rho / pi; on a Lambertian surface w f cos / p <= rho <= 1, asserted
        ca = (wa * cos / np.pi / p_area)[:, None] * rho[None, :]
        cb = wb[:, None] * rho[None, :]
        assert (ca <= 1.0 + 1e-12).all() and (cb <= 1.0 + 1e-12).all(), "clamp01 would bind"
        ca = ca * np.asarray(le)[None, :]
        cb = cb * np.asarray(le)[None, :]
        da = (P / A) * dA                  # probability of the piece under the area draw
        db = p_bsdf * cosl / r2 * dA       # ... under the BSDF draw
        for m in range(4):
            ma[m] += (da[:, None] * ca ** (m + 1)).sum(axis=0)
            mb[m] += (db[:, None] * cb ** (m + 1)).sum(axis=0)
    return ma, mb


def central(raw):
    """(mean, variance, fourth central moment) from raw moments m1..m4 of a variable that is 0 with the remaining probability"""
    m1, m2, m3, m4 = raw
    return m1, m2 - m1 ** 2, m4 - 4 * m1 * m3 + 6 * m1 ** 2 * m2 - 3 * m1 ** 4


def lambert_floor_variance(x, normal, rho, tris, les, pick_p, level=5):
    """(mean, variance, fourth central moment) per channel of the sum of the two independent draws"""
    ma, mb = lambert_floor_moments(x, normal, rho, tris, les, pick_p, level)
    e1, v1, k1 = central(ma)
    e2, v2, k2 = central(mb)
    var = v1 + v2
    mu4 = k1 + k2 + 6 * v1 * v2
    return e1 + e2, var, mu4


def lambert_polygon(x, normal, rho, tris, les):
    """Lambert's polygon formula for the same floor point: what the mean must be whatever the pick distribution is"""
    import expectation_model as E
    x = np.asarray(x, np.float64)[None, :]
    return sum(E.polygon_irradiance(x, tuple(normal), np.asarray(t, np.float64))[0] * np.asarray(le) for t, le in zip(tris, les)) * np.asarray(rho) / np.pi


def first_vertex_emitters(bsdf_lobes, mat, wo_world, x, tris, les, pick_p, level=4):
    """Expected radiance (rgb) that one visit of the closest-hit program adds at floor point x (normal +y, throughput 1, black background) under emissive triangles
    facing the floor, for ANY material -- expectation_model.first_vertex_constant_background with the emitters inside the integral, both draws as integrals over the
    emitters' area (pieces y, dA; wi the direction to y, r its distance, cos_l the cosine at the emitter, p_k = r^2 / cos_l * P_k / area_k):
      area draw:  y ~ P_k / area_k,  w = p_k / (p_k + pdf_b(wi)),  c = regularize(w f |cos| / p_k) Le;
      light ray, lobe i:  wi ~ lobe i's real density d_i (per solid angle: d_i cos_l / r^2 per area),  w = r_i / (r_i + p_k),  c = regularize(w f_i |cos| / r_i) Le,
      (f_i, r_i) what Bsdf::sample reports for the lobe; a ray that finds no emitter adds nothing.
    wo_world: unit vector from x towards the viewer.  The floor's local frame is the world's with z negated (env_sampling_model.local_grid)."""
    import expectation_model as E
    flip = np.array([1.0, 1.0, -1.0])
    wo = np.asarray(wo_world, np.float64) * flip
    x = np.asarray(x, np.float64)
    total = np.zeros(3)
    for tri, le, P in zip(tris, les, pick_p):
        tri = np.asarray(tri, np.float64)
        y, dA = triangle_quadrature(tri, level)
        A = dA.sum()
        nl = np.cross(tri[1] - tri[0], tri[2] - tri[0])
        nl /= np.linalg.norm(nl)
        d = y - x
        r2 = (d * d).sum(axis=1)
        wi_w = d / np.sqrt(r2)[:, None]
        cosl = np.abs(wi_w @ nl)
        dirs = wi_w * flip
        c = np.abs(dirs[:, 1])
        pk = r2 / cosl * (P / A)
        n = len(dirs)
        r_all = bsdf_lobes(mat, True, 127, np.repeat(wo[None, :].astype(f32), n, 0), dirs.astype(f32), np.zeros(n, f32), np.full((n, 2), 0.5, f32)).astype(np.float64)
        wa, _ = E._weight(pk, r_all[:, 3], r_all[:, 0:3], c, pk)
        total += ((P / A) * dA) @ (wa * np.asarray(le)[None, :])
        per_lobe = E.lobes(bsdf_lobes, mat, True, wo, dirs)
        for bit, dens in E.lobe_densities(mat, True, wo, dirs, per_lobe).items():
            f_i, r_i = per_lobe[0][bit]
            wb, _ = E._weight(r_i, pk, f_i, c, r_i)
            on = dens > 0
            total += (dens * cosl / r2 * dA) @ np.where(on[:, None], wb * np.asarray(le)[None, :], 0.0)
    return total
