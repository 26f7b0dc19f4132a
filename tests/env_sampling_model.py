"""numpy restatement of fh_set_env_sampling (include/fredholm_hip.h) for test_env_sampling_host.py, test_gpu_env_sampling.py and tools/env_sampling_model.py
(a plain helper module, not a conftest).

Every fp32 step is a numpy float32 operation in the header's order; the elementary functions are the CPU checker's (oracle.elementary, its own implementation of
the specification include/fh_elementary.h follows), the image fetch is the checker's texture unit (oracle.tex2d_f32) and the Hosek dome the checker's
(oracle.hosek_radiance): nothing of the product's code is used to state what the product must compute.  Integers are numpy uint64, the CDF quotients float64
divisions rounded once."""
import numpy as np

W, H = 512, 256
CELLS = W * H
f32 = np.float32
PI = f32(3.14159265358979323846)
TWO_PI = f32(2.0) * PI
BELOW_ONE = f32(0.99999994)
SIN_FLOOR = f32(2.0 ** -20)
BIG = f32(3.0e38)
LUM = (f32(0.2126729), f32(0.7151522), f32(0.0721750))


def subsamples(ibl_w):
    return int(min(max(-(-int(ibl_w) // W), 2), 16))


# ---------------------------------------------------------------------------------------------------------------- the test environments
def sun_image(w=64, h=32, patch=2, radiance=400.0, elevation_deg=50.0, phi_deg=120.0):
    """a w x h float4 lat-long image: a smooth dim gradient 0.05 .. 0.2 and one patch x patch texel block of `radiance` at about `elevation_deg`"""
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    g = 0.05 + 0.15 * (0.5 + 0.5 * np.cos(2 * np.pi * x / w)) * (1.0 - y / (h - 1.0))
    img = np.zeros((h, w, 4), np.float32)
    img[..., 0], img[..., 1], img[..., 2], img[..., 3] = g, 0.9 * g, 0.8 * g, 1.0
    ty = int(round((90.0 - elevation_deg) / 180.0 * h)) - patch // 2
    tx = int(round(phi_deg / 360.0 * w)) - patch // 2
    img[ty:ty + patch, tx:tx + patch, 0:3] = radiance
    return img


def direction(u, v, oracle):
    """(u, v) in [0, 1)^2 -> d, sin theta (float32 arrays)"""
    u, v = np.asarray(u, f32), np.asarray(v, f32)
    t, p = v * PI, u * TWO_PI
    st, ct = oracle.elementary("sin", t).reshape(t.shape), oracle.elementary("cos", t).reshape(t.shape)
    sp, cp = oracle.elementary("sin", p).reshape(p.shape), oracle.elementary("cos", p).reshape(p.shape)
    return np.stack([st * cp, ct, st * sp], axis=-1), st


def subsample_uv(k):
    """u [W, k] (cell i, sub-sample a), v [H, k] (cell j, sub-sample b)"""
    a = (np.arange(k, dtype=f32) + f32(0.5)) / f32(k)
    u = (np.arange(W, dtype=f32)[:, None] + a[None, :]) / f32(W)
    v = (np.arange(H, dtype=f32)[:, None] + a[None, :]) / f32(H)
    return u.astype(f32), v.astype(f32)


def subsample_dirs(k, oracle):
    """directions [H, k(b), W, k(a), 3] and sin theta [H, k(b)] of every sub-sample"""
    u, v = subsample_uv(k)
    U = np.broadcast_to(u[None, None, :, :], (H, k, W, k))
    V = np.broadcast_to(v[:, :, None, None], (H, k, W, k))
    d, st = direction(U, V, oracle)
    return d.astype(f32), st[:, :, 0, 0]


def uv_of(d, oracle):
    """the environment look-up's mapping: direction -> (phi / 2 pi, theta / pi)"""
    d = np.asarray(d, f32)
    theta = oracle.elementary("acos", np.fmax(f32(-1), np.fmin(d[..., 1], f32(1)))).reshape(d.shape[:-1])
    phi = oracle.elementary("atan2", d[..., 2], d[..., 0]).reshape(d.shape[:-1])
    phi = np.where(phi < 0, phi + TWO_PI, phi).astype(f32)
    return phi / TWO_PI, theta / PI


def radiance(env, d, oracle):
    """what the context shows along d at sky intensity 1.  env: ("ibl", image) | ("hosek", state30, sun_dir) | ("constant",)"""
    d = np.ascontiguousarray(d, f32)
    if env[0] == "ibl":
        u, v = uv_of(d, oracle)
        return oracle.tex2d_f32(env[1], np.stack([u, v], axis=-1).reshape(-1, 2))[:, :3].reshape(d.shape)
    if env[0] == "hosek":
        return oracle.hosek_radiance(env[1], env[2], 1.0, d.reshape(-1, 3)).reshape(d.shape)
    return np.ones(d.shape, f32)


def finite(x):
    x = np.asarray(x, f32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x) | (np.abs(x) > BIG), f32(0), x).astype(f32)


def lum(rgb):
    r, g, b = finite(rgb[..., 0]), finite(rgb[..., 1]), finite(rgb[..., 2])
    with np.errstate(over="ignore", invalid="ignore"):
        return ((r * LUM[0] + g * LUM[1]) + b * LUM[2]).astype(f32)


def cell_means(l, st):
    """l [H, k, W, k]: the luminance at the sub-samples (None: a constant background); st [H, k].  The serial sum b outer, a inner, then the mean"""
    k = st.shape[1]
    s = np.zeros((H, W), f32)
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(k):
            sb = np.fmax(st[:, b], f32(0))[:, None]
            for a in range(k):
                la = f32(1) if l is None else l[:, b, :, a]
                s = (s + np.fmin(np.fmax(la, f32(0)), BIG) * sb).astype(f32)
        return np.fmin(s / f32(k * k), BIG).astype(f32)


def weights_of(env, oracle):
    k = subsamples(env[1].shape[1]) if env[0] == "ibl" else 2
    d, st = subsample_dirs(k, oracle)
    return cell_means(None if env[0] == "constant" else lum(radiance(env, d, oracle)), st)


class Table:
    """quantised weights, CDFs and cell probabilities from the cell means w [H, W]"""

    def __init__(self, w):
        w = np.asarray(w, f32)
        w_max = w.max()
        if w_max > 0:
            q = np.maximum(((w / w_max) * f32(1048576.0)).astype(f32).astype(np.uint64), 1)
        else:
            q = np.ones((H, W), np.uint64)
        self.q = q
        self.row_sum = q.sum(axis=1)
        self.total = int(self.row_sum.sum())
        pre = np.concatenate([np.zeros((H, 1), np.uint64), np.cumsum(q, axis=1)], axis=1)
        self.cdf_row = (pre.astype(np.float64) / self.row_sum[:, None].astype(np.float64)).astype(f32)
        prm = np.concatenate([np.zeros(1, np.uint64), np.cumsum(self.row_sum)])
        self.cdf_m = (prm.astype(np.float64) / np.float64(self.total)).astype(f32)
        self.cell_p = (q.astype(np.float64) / np.float64(self.total)).astype(f32)
        assert self.cdf_row[:, -1].view(np.uint32).tolist() == [0x3F800000] * H and self.cdf_m[-1] == f32(1)


def search(cdf, u):
    """per element: the largest k with cdf[k] <= u, by the header's bisection.  cdf [n + 1] or [N, n + 1] (one row per element)"""
    n = cdf.shape[-1] - 1
    lo, hi = np.zeros(u.shape, np.int64), np.full(u.shape, n, np.int64)
    rows = np.arange(u.shape[0]) if cdf.ndim == 2 else None
    while (hi - lo > 1).any():
        go = hi - lo > 1
        mid = (lo + hi) >> 1
        c = cdf[rows, mid] if cdf.ndim == 2 else cdf[mid]
        left = go & (c <= u)
        right = go & ~(c <= u)
        lo = np.where(left, mid, lo)
        hi = np.where(right, mid, hi)
    return lo


def remap(c0, c1, u):
    return np.fmin((u - c0) / (c1 - c0), BELOW_ONE).astype(f32)


def mixture_pdf(t, beta, cell, d, n):
    d, n, beta = np.asarray(d, f32), np.asarray(n, f32), f32(beta)
    st = np.fmax(np.sqrt(d[:, 0] * d[:, 0] + d[:, 2] * d[:, 2]), SIN_FLOOR).astype(f32)
    cosn = ((d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]).astype(f32)
    pt = (t.cell_p.reshape(-1)[cell] * f32(CELLS)) / ((f32(2) * (PI * PI)) * st)
    return ((f32(1) - beta) * pt + beta * (np.fmax(cosn, f32(0)) / PI)).astype(f32)


def cell_of(d, oracle):
    u, v = uv_of(d, oracle)
    fi, fj = u * f32(W), v * f32(H)
    i = np.where(fi >= W - 1, W - 1, np.where(fi > 0, fi, 0).astype(np.int64))
    j = np.where(fj >= H - 1, H - 1, np.where(fj > 0, fj, 0).astype(np.int64))
    return (j * W + i).astype(np.int64)


def pdf(t, beta, d, n, oracle):
    c = cell_of(d, oracle)
    return mixture_pdf(t, beta, c, d, n), c


def sample_table(t, beta, ux, uy, n, oracle):
    """the table branch on the rescaled (ux, uy): direction, density, drawn cell"""
    ux, uy = np.asarray(ux, f32), np.asarray(uy, f32)
    j = search(t.cdf_m, ux)
    rows = t.cdf_row[j]
    i = search(rows, uy)
    k = np.arange(len(ux))
    v = ((j.astype(f32) + remap(t.cdf_m[j], t.cdf_m[j + 1], ux)) / f32(H)).astype(f32)
    u = ((i.astype(f32) + remap(rows[k, i], rows[k, i + 1], uy)) / f32(W)).astype(f32)
    d, _ = direction(u, v, oracle)
    cell = j * W + i
    return d.astype(f32), mixture_pdf(t, beta, cell, d, n), cell


def onb(n):
    n = np.asarray(n, f32)
    sign = np.copysign(f32(1), n[:, 2]).astype(f32)
    a = (f32(-1) / (sign + n[:, 2])).astype(f32)
    bb = (n[:, 0] * n[:, 1] * a).astype(f32)
    t = np.stack([f32(1) + sign * n[:, 0] * n[:, 0] * a, sign * bb, -sign * n[:, 0]], axis=-1).astype(f32)
    b = np.stack([bb, sign + n[:, 1] * n[:, 1] * a, -n[:, 1]], axis=-1).astype(f32)
    return t, b


def to_world(v, t, n, b):
    return np.stack([(v[:, 0] * t[:, k] + v[:, 1] * n[:, k]) + v[:, 2] * b[:, k] for k in range(3)], axis=-1).astype(f32)


def sample(t, beta, u, n, oracle):
    """the sky slot's draw: (direction, density, cell, took the cosine branch)"""
    u, n, beta = np.asarray(u, f32), np.asarray(n, f32), f32(beta)
    cosine = u[:, 0] < beta
    with np.errstate(divide="ignore", invalid="ignore"):
        ux = np.where(cosine, u[:, 0] / beta, np.fmin((u[:, 0] - beta) / (f32(1) - beta), BELOW_ONE)).astype(f32)
    tg, bt = onb(n)
    dc = to_world(oracle.warp(1, np.stack([ux, u[:, 1]], axis=-1)), tg, n, bt)
    pc, cc = pdf(t, beta, dc, n, oracle)
    dt, ptab, ct = sample_table(t, beta, np.where(cosine, f32(0), ux), u[:, 1], n, oracle)
    m = cosine[:, None]
    return np.where(m, dc, dt).astype(f32), np.where(cosine, pc, ptab).astype(f32), np.where(cosine, cc, ct), cosine


# ---------------------------------------------------------------------------------------------------------------- float64 side
def table_density64(t, dirs):
    """float64 table density P_cell * W * H / (2 pi^2 sin theta) of unit directions (N, 3), cells by the exact mapping"""
    d = np.asarray(dirs, np.float64)
    theta = np.arccos(np.clip(d[:, 1], -1.0, 1.0))
    phi = np.mod(np.arctan2(d[:, 2], d[:, 0]), 2 * np.pi)
    i = np.clip((phi / (2 * np.pi) * W).astype(int), 0, W - 1)
    j = np.clip((theta / np.pi * H).astype(int), 0, H - 1)
    p = t.q[j, i].astype(np.float64) / float(t.total)
    return p * CELLS / (2 * np.pi ** 2 * np.maximum(np.sin(theta), 1e-300))


def mixture_density64(t, beta, dirs, normal):
    d = np.asarray(dirs, np.float64)
    return (1.0 - beta) * table_density64(t, d) + beta * np.maximum(d @ np.asarray(normal, np.float64), 0.0) / np.pi


def cell_quadrature(rows=range(H), n_gl=2):
    """Gauss-Legendre nodes inside every table cell of the given rows: unit directions (N, 3) and weights d omega (N,).  The table density is constant times
    1 / sin theta inside a cell and a bilinear image has its kinks on cell boundaries wherever 512 x 256 is a multiple of its size, so the panels hold smooth pieces only"""
    x, wx = np.polynomial.legendre.leggauss(n_gl)
    rows = np.asarray(list(rows))
    th = ((rows[:, None] + 0.5 * (x[None, :] + 1.0)) * np.pi / H).ravel()
    ph = ((np.arange(W)[:, None] + 0.5 * (x[None, :] + 1.0)) * 2 * np.pi / W).ravel()
    wt, wp = np.tile(0.5 * wx * np.pi / H, len(rows)), np.tile(0.5 * wx * 2 * np.pi / W, W)
    T, P = np.meshgrid(th, ph, indexing="ij")
    wq = ((wt * np.sin(th))[:, None] * wp[None, :]).ravel()
    return np.stack([np.sin(T) * np.cos(P), np.cos(T), np.sin(T) * np.sin(P)], axis=-1).reshape(-1, 3), wq


def lambert_floor_moments(t, beta, dirs, wq, L, rho):
    """Raw moments 1 .. 4, per channel (4, 3), of the two independent first-vertex draws at a Lambertian floor (normal +y, albedo rho) that sees the whole upper
    hemisphere: the sky ray and the BSDF-sampled light ray, as ((sky), (bsdf)).  beta None: today's estimator (sky ray cosine-distributed, pdf_light = |cos| / pi);
    otherwise the mixture of table t.  dirs, wq: a quadrature of the UPPER hemisphere; L (N, 3): the environment at the nodes.
    c = clamp01(w f cos / p) L with w = p / (p + q): the clamp never binds for a Lambertian (w f cos / p = f cos / (p + q) <= rho / (1 + beta) < 1)"""
    d = np.asarray(dirs, np.float64)
    cos = np.maximum(d[:, 1], 0.0)
    p_b = cos / np.pi                                       # the diffuse lobe's density, which is also today's sky density
    p_s = p_b if beta is None else mixture_density64(t, beta, d, (0.0, 1.0, 0.0))
    f = np.asarray(rho, np.float64)[None, :] / np.pi
    g = (f * cos[:, None] / (p_s + p_b)[:, None]) * np.asarray(L, np.float64)  # the contribution of either draw at a direction: w f cos / p = f cos / (p_s + p_b)
    assert (f * cos[:, None] / (p_s + p_b)[:, None] <= 1.0).all()
    sky = np.stack([(wq * p_s) @ g ** k for k in (1, 2, 3, 4)])
    bsdf = np.stack([(wq * p_b) @ g ** k for k in (1, 2, 3, 4)])
    return sky, bsdf


def central_of_sum(*raw):
    """(mean, variance, fourth central moment), per channel, of the sum of independent variables given by their raw moments 1 .. 4"""
    mean, var, mu4, pair = 0.0, 0.0, 0.0, 0.0
    for m in raw:
        m1, m2, m3, m4 = m
        v = m2 - m1 * m1
        c4 = m4 - 4 * m3 * m1 + 6 * m2 * m1 * m1 - 3 * m1 ** 4
        mu4 = mu4 + c4 + 6 * var * v
        mean, var = mean + m1, var + v
    return mean, var, mu4


def lambert_floor_variance(t, beta, dirs, wq, L, rho):
    """(expectation, variance, fourth central moment) per channel of one first-vertex sample: the sum of the two independent draws"""
    return central_of_sum(*lambert_floor_moments(t, beta, dirs, wq, L, rho))


# ---------------------------------------------------------------------------------------------------------------- the estimator's expectation, any material
def local_grid(wo, entering, n_gl=2):
    """Quadrature over the sphere in the floor's local frame (y the normal; the local frame of a +y normal is the world's with z negated, so the table's cell
    boundaries are the same set of angles in both): Gauss-Legendre panels between the table's cell boundaries, refined round the polar and azimuthal angles where the
    microfacet lobes of wo peak (expectation_model.peaks; the azimuth opposite wo's).  Returns local dirs (N, 3) and weights d omega"""
    import expectation_model as E
    az = float(np.arctan2(wo[2], wo[0])) + np.pi
    tb = np.concatenate([np.arange(H + 1) * np.pi / H] + [E._peak_breaks(p, 0.0, np.pi) for p in E.peaks(wo, entering)] + [[np.arccos(-np.clip(wo[1], -1.0, 1.0))]])
    pb = np.concatenate([np.arange(W + 1) * 2 * np.pi / W] + [E._peak_breaks(np.mod(az, 2 * np.pi) + k * 2 * np.pi, 0.0, 2 * np.pi) for k in (-1, 0, 1)])
    t, wt, _ = E._gl_panels(tb, n_gl)
    p, wp, _ = E._gl_panels(pb, n_gl)
    T, P = np.meshgrid(t, p, indexing="ij")
    wq = ((wt * np.sin(t))[:, None] * wp[None, :]).ravel()
    st = np.sin(T)
    return np.stack([st * np.cos(P), np.cos(T), st * np.sin(P)], axis=-1).reshape(-1, 3), wq


def first_vertex_env(bsdf_lobes, mat, wo, t, beta, radiance_of):
    """Expected radiance (rgb) that one visit of the closest-hit program adds at a point of an open floor (normal +y, throughput 1) under an environment, every ray
    that does not start into the floor escaping -- expectation_model.first_vertex_constant_background with the environment inside the integral and, for beta not None, the mixture of table t as the sky
    ray's density and as pdf_light of the BSDF-sampled ray:
      sky ray: d ~ p, w = p / (p + pdf_b), c = regularize(w f |cos| / p) L(d);   light ray, lobe i: d ~ its density, w = r_i / (r_i + p), c = regularize(w f_i |cos| / r_i) L(d).
    wo: local unit vector (any azimuth); radiance_of(world dirs (N, 3) float64) -> (N, 3).  Returns (expectation (3,), lost mass of the lobes' samplers)"""
    import expectation_model as E
    wo = np.asarray(wo, np.float64)
    dirs, wq = local_grid(wo, True)
    world = dirs * np.array([1.0, 1.0, -1.0])
    L = np.asarray(radiance_of(world), np.float64)
    c = np.abs(dirs[:, 1])
    p = np.maximum(dirs[:, 1], 0.0) / np.pi if beta is None else mixture_density64(t, beta, world, (0.0, 1.0, 0.0))
    p_light = c / np.pi if beta is None else p              # (today's pdf_light is |cos| / pi on both hemispheres)
    n = len(dirs)
    r_all = bsdf_lobes(mat, True, 127, np.repeat(wo[None, :].astype(f32), n, 0), dirs.astype(f32), np.zeros(n, f32), np.full((n, 2), 0.5, f32)).astype(np.float64)
    live = (p > 0) & (dirs[:, 1] > 0)  # a sky ray at or below the shading horizon adds nothing (the header), and the floor itself would stop it: it leaves from the outer side
    wsky, _ = E._weight(np.where(live, p, 1.0), r_all[:, 3], r_all[:, 0:3], c, np.where(live, p, 1.0))
    total = (wq * p * live) @ (wsky * L)
    per_lobe = E.lobes(bsdf_lobes, mat, True, wo, dirs)
    mass = 0.0
    for bit, dens in E.lobe_densities(mat, True, wo, dirs, per_lobe).items():
        f_i, r_i = per_lobe[0][bit]
        wb, _ = E._weight(r_i, p_light, f_i, c, r_i)
        on = dens > 0
        total = total + (wq * dens) @ np.where(on[:, None], wb * L, 0.0)
        mass += float(wq @ dens)
    return total, max(1.0 - mass, 0.0)
