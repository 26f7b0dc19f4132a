"""Float64 model of the BSDF samplers for test_bsdf_sampling_density.py (a plain helper module, not a conftest).

The lobes themselves are not restated here: f_i and pmf_i * pdf_i come from the checker's orc_bsdf_lobes (one lobe bit), which
the GPU parity suite pins bit for bit to the device's fh_kat_bsdf_lobes.  What this module adds is everything around the lobes:
quadrature over the sphere, the density each sampler really draws and the chi-square bookkeeping.

Local shading frame: y is the normal, wo lies in the x-y plane with x >= 0.
"""
import numpy as np

LOBE_BITS = (1, 2, 4, 8, 16, 32, 64)  # coat, metal, specular, transmission, sheen, diffuse transmission, diffuse
L_TRANS, L_SHEEN = 8, 16


def wo_at(cos_theta):
    c = float(cos_theta)
    return np.array([np.sqrt(max(1.0 - c * c, 0.0)), c, 0.0])


def _gl_panels(breaks, n):
    """Gauss-Legendre nodes and weights on every panel between consecutive breakpoints; also the panel index of each node"""
    x, w = np.polynomial.legendre.leggauss(n)
    b = np.unique(np.asarray(breaks, np.float64))
    lo, hi = b[:-1], b[1:]
    nodes = (0.5 * (hi - lo))[:, None] * x[None, :] + (0.5 * (hi + lo))[:, None]
    weights = (0.5 * (hi - lo))[:, None] * w[None, :]
    return nodes.ravel(), weights.ravel(), b


def _peak_breaks(center, lo, hi):
    steps = np.array([1e-3, 3e-3, 1e-2, 3e-2, 0.1, 0.3, 1.0])
    b = np.concatenate([center - steps, center + steps])
    return b[(b > lo) & (b < hi)]


def peaks(wo, entering, eta=1.5):
    """polar angles where the microfacet lobes of wo peak: the mirror direction and the refracted one (theta measured from +y)"""
    ct = float(np.clip(wo[1], -1.0, 1.0))
    th = [float(np.arccos(ct))]
    ni, nt = (1.0, eta) if entering else (eta, 1.0)
    s = ni / nt * np.sqrt(max(1.0 - ct * ct, 0.0))
    if s < 1.0:
        th.append(float(np.pi - np.arcsin(s)))
    return th


def sphere_grid(wo, entering, n_cos=24, n_phi=24, n_gl=6):
    """Quadrature over the whole sphere in (theta, phi).  Breakpoints: the cells of the chi-square histogram (uniform in cos theta
    and in phi), the horizons below, and geometric refinements around the lobes' peaks (phi = pi for wo in the x-y plane), so that every
    GL panel lies inside one cell and sharp GGX lobes (alpha = roughness^2 down to 1e-4) are resolved.
    Returns dirs (N, 3), weights (N,) for d(omega), and the histogram cell of every node."""
    cell_t = np.arccos(np.linspace(1.0, -1.0, n_cos + 1))
    # the horizon, and cos theta = -wo.y where normalize(wo + wi) crosses the horizon (the GGX reflection lobes end there)
    tb = np.concatenate([cell_t, [0.5 * np.pi, np.arccos(-np.clip(wo[1], -1.0, 1.0))]] + [_peak_breaks(p, 0.0, np.pi) for p in peaks(wo, entering)] + [_peak_breaks(0.0, 0.0, np.pi)])
    pb = np.concatenate([np.linspace(0.0, 2 * np.pi, n_phi + 1), _peak_breaks(np.pi, 0.0, 2 * np.pi), _peak_breaks(0.0, 0.0, 2 * np.pi),
                         _peak_breaks(2 * np.pi, 0.0, 2 * np.pi)])
    t, wt, _ = _gl_panels(tb, n_gl)
    p, wp, _ = _gl_panels(pb, n_gl)
    T, P = np.meshgrid(t, p, indexing="ij")
    W = (wt * np.sin(t))[:, None] * wp[None, :]
    st = np.sin(T)
    dirs = np.stack([st * np.cos(P), np.cos(T), st * np.sin(P)], axis=-1).reshape(-1, 3)
    ci = np.clip(((1.0 - np.cos(T)) / 2.0 * n_cos).astype(int), 0, n_cos - 1)
    pi_ = np.clip((P / (2 * np.pi) * n_phi).astype(int), 0, n_phi - 1)
    return dirs, W.ravel(), (ci * n_phi + pi_).ravel()


def cell_of(wi, n_cos=24, n_phi=24):
    wi = np.asarray(wi, np.float64)
    c = np.clip(wi[:, 1], -1.0, 1.0)
    phi = np.mod(np.arctan2(wi[:, 2], wi[:, 0]), 2 * np.pi)
    ci = np.clip(((1.0 - c) / 2.0 * n_cos).astype(int), 0, n_cos - 1)
    pi_ = np.clip((phi / (2 * np.pi) * n_phi).astype(int), 0, n_phi - 1)
    return ci * n_phi + pi_


def lobes(bsdf_lobes, mat, entering, wo, dirs):
    """per lobe bit: (weighted f_i rgb (N,3), pmf_i * pdf_i (N,)) at wi = dirs, and the material's pmf (7,).
    bsdf_lobes(mat, entering, only, wo, wi, u1, u2) -> 18 columns (oracle.bsdf_lobes or the device's fh_kat_bsdf_lobes)."""
    n = dirs.shape[0]
    wo32 = np.repeat(np.asarray(wo, np.float32)[None, :], n, axis=0)
    wi32 = dirs.astype(np.float32)
    u1 = np.zeros(n, np.float32)
    u2 = np.full((n, 2), 0.5, np.float32)
    out, pmf = {}, None
    for bit in LOBE_BITS:
        r = bsdf_lobes(mat, entering, bit, wo32, wi32, u1, u2)
        pmf = r[0, 11:18].astype(np.float64)
        out[bit] = (r[:, 0:3].astype(np.float64), r[:, 3].astype(np.float64))
    return out, pmf


def sampled_density(bit, wo, entering, dirs, reported, eta=1.5):
    """The density (per unit solid angle, before the lobe's pmf) with which lobe `bit`'s sampler really draws wi = dirs, in terms of
    the lobe's own reported pdf where the two agree:
    - GGX reflection (coat, metal, specular): wi = reflect(wo, h) with h ~ VNDF; the reported 0.25 Dvis / |wo.h| is the density of
      the h with h.y > 0 only (the VNDF never draws the others), so it is zeroed where normalize(wo + wi).y <= 0.
    - sheen: the reference draws the HALF vector h cosine-distributed and reflects wo about it (bxdf.cu:758-772), yet reports
      |cos wi| / pi (bxdf.cu:774-777).  The drawn density is |h.y| / pi / (4 |wo.h|) with h = normalize(wo + wi).
    - transmission: only where wi is on the other side from wo, from a half vector with h.y > 0 (refraction); the total-internal-
      reflection branch (bxdf.cu:660-679) draws reflections instead, modelled below.
    - cosine lobes (diffuse, diffuse transmission): the reported |cos wi| / pi, on their own hemisphere (the report covers both).
    `reported` is pmf_i * pdf_i at dirs from `lobes`; returns pmf_i * (true density)."""
    wo = np.asarray(wo, np.float64)
    d = np.asarray(dirs, np.float64)
    h = wo[None, :] + d
    h /= np.maximum(np.linalg.norm(h, axis=1, keepdims=True), 1e-300)
    if bit in (1, 2, 4):
        return np.where(h[:, 1] > 0, reported, 0.0)
    if bit == 64:
        return np.where(d[:, 1] > 0, reported, 0.0)
    if bit == 32:
        return np.where(d[:, 1] < 0, reported, 0.0)
    raise ValueError("sampled_density models the reflection and cosine lobes; sheen and transmission need sheen_density / the TIR model")


def sheen_density(wo, dirs):
    wo = np.asarray(wo, np.float64)
    h = wo[None, :] + np.asarray(dirs, np.float64)
    h /= np.maximum(np.linalg.norm(h, axis=1, keepdims=True), 1e-300)
    return np.abs(h[:, 1]) / np.pi / (4.0 * np.maximum(np.abs(h @ wo), 1e-300))


def chi2_sf(x, k):
    """upper tail of the chi-square distribution (Wilson-Hilferty; accurate to a few per cent in p at k >= 10, ample at p = 1e-5)"""
    if k <= 0:
        return 1.0
    from math import erfc, sqrt
    z = ((x / k) ** (1.0 / 3.0) - (1.0 - 2.0 / (9.0 * k))) / sqrt(2.0 / (9.0 * k))
    return 0.5 * erfc(z / sqrt(2.0))


def chi2_pooled(observed, expected, min_expected=5.0):
    """chi-square statistic and degrees of freedom after pooling all cells whose expected count is below min_expected into one"""
    observed, expected = np.asarray(observed, np.float64), np.asarray(expected, np.float64)
    small = expected < min_expected
    o = np.append(observed[~small], observed[small].sum())
    e = np.append(expected[~small], expected[small].sum())
    keep = e > 0
    if (o[~keep] > 0).any():
        return np.inf, max(int(keep.sum()) - 1, 1)
    o, e = o[keep], e[keep]
    return float(((o - e) ** 2 / e).sum()), len(e) - 1


# ---------------------------------------------------------------------------------------------------------------------------------
# The mixture's sampled density, lobe by lobe (used by test_bsdf_sampling_density.py and the estimator expectations below)
def alpha_of(mat):
    r = float(np.clip(mat["specular_roughness"][0], 0.01, 1.0))
    return r * r


def ggx_dvis(a, wo, h):
    """float64 GGX visible-normal density of h (isotropic alpha a), for the total-internal-reflection branch only"""
    lam = 0.5 * (-1.0 + np.sqrt(1.0 + a * a * (wo[0] ** 2 + wo[2] ** 2) / wo[1] ** 2))
    t = (h[:, 0] ** 2 + h[:, 2] ** 2) / (a * a) + h[:, 1] ** 2
    d = 1.0 / (np.pi * a * a * t * t)
    return np.abs(h @ wo) * d / (abs(wo[1]) * (1.0 + lam))


def tir(wo, h, entering, eta=1.5):
    ni, nt = (1.0, eta) if entering else (eta, 1.0)
    c = h @ wo
    return (ni / nt) ** 2 * (1.0 - c * c) > 1.0


def lobe_densities(mat, entering, wo, dirs, per_lobe, eta=1.5):
    """per lobe bit: pmf_i * (the density lobe i's sampler really draws at dirs), see sampled_density; the transmission lobe's
    total-internal-reflection branch (bxdf.cu:660-679) draws the reflection density of its half vector instead"""
    wo64 = np.asarray(wo, np.float64)
    lobe_vals, pmf = per_lobe
    out = {}
    for bit, (f, pp) in lobe_vals.items():
        k = LOBE_BITS.index(bit)
        if pmf[k] == 0 or not np.isfinite(pmf[k]):
            continue
        if bit == L_SHEEN:
            out[bit] = pmf[k] * sheen_density(wo64, dirs)
        elif bit == L_TRANS:
            ni, nt = (1.0, eta) if entering else (eta, 1.0)
            h = -(ni * wo64[None, :] + nt * dirs)
            h /= np.linalg.norm(h, axis=1, keepdims=True)
            h = np.where(h[:, 1:2] < 0, -h, h)
            refr = (h @ wo64 > 0) & (np.einsum("ij,ij->i", dirs, h) < 0) & ~tir(wo64, h, entering, eta)
            dens = np.where(refr, pp, 0.0)
            hr = wo64[None, :] + dirs
            hr /= np.linalg.norm(hr, axis=1, keepdims=True)
            refl = (hr[:, 1] > 0) & tir(wo64, hr, entering, eta)
            out[bit] = dens + np.where(refl, pmf[k] * ggx_dvis(alpha_of(mat), wo64, hr) / (4.0 * np.abs(hr @ wo64)), 0.0)
        else:
            out[bit] = sampled_density(bit, wo64, entering, dirs, pp, eta)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# Expectations of what pt.cu's closest-hit program adds at a surface point (pt.cu:680-944), in float64.
# Every weight goes through regularize_weight (pt.cu:372-375): clamp(w, 0, 1) per channel, i.e. fmaxf(0, fminf(w, 1)), so NaN -> 1.
def regularize(w):
    return np.fmax(0.0, np.fmin(w, 1.0))


def _weight(mis_pdf, other_pdf, f, cos_i, pdf):
    """pt.cu:786-790, :817-821, :881-885, :919-921: regularize_weight(throughput * mis_weight * f * |cos wi| / pdf) at throughput 1,
    mis_weight = pdf0 / (pdf0 + pdf1) (compute_mis_weight, pt.cu:365-369); returns (clamped, unclamped) (N, 3)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        w = (mis_pdf / (mis_pdf + other_pdf))[:, None] * f * (cos_i / pdf)[:, None]
    return regularize(w), w


def first_vertex_constant_background(bsdf_lobes, mat, cos_o, entering=True, n_gl=6):
    """Expected regularized weight (rgb, per unit background radiance) that one visit of pt.cu's closest-hit program adds at a point
    of an open convex surface under a constant background, seen at cos theta_o, throughput 1.  Both rays escape, so each carries
    the background (miss programs, pt.cu:531-543); nothing else is lit.
    - sky NEE (pt.cu:842-857): wi cosine-distributed on the hemisphere above the shading normal only, pdf = |cos wi| / pi, MIS
      against the whole mixture's eval_pdf, f = the whole mixture's eval;
    - the BSDF-sampled light ray (pt.cu:893-925): lobe i chosen with pmf_i, wi drawn with lobe i's real density anywhere on the
      sphere, (f, pdf) = (f_i, pmf_i * pdf_i) of the chosen lobe (Bsdf::sample), and on a miss pdf_light = |cos wi| / pi (:911-913).
    Lost draws (the density's missing mass) come back with a NaN or zero pdf, whose weight the clamp turns into 1 (NaN -> 1).
    Returns (expected weight (3,), largest unclamped weight with nonzero density, lost mass)."""
    wo = wo_at(cos_o)
    dirs, w, _ = sphere_grid(wo, entering, n_gl=n_gl)
    per_lobe = lobes(bsdf_lobes, mat, entering, wo, dirs)
    c = np.abs(dirs[:, 1])
    p_cos = c / np.pi
    r_all = bsdf_lobes(mat, entering, 127, np.repeat(wo[None, :].astype(np.float32), len(dirs), 0), dirs.astype(np.float32),
                       np.zeros(len(dirs), np.float32), np.full((len(dirs), 2), 0.5, np.float32)).astype(np.float64)
    up = dirs[:, 1] > 0
    wsky, raw = _weight(p_cos, r_all[:, 3], r_all[:, 0:3], c, p_cos)
    total = ((w * p_cos * up) @ wsky)
    peak = float(np.nanmax(np.where(up[:, None], raw, -np.inf)))
    mass = 0.0
    for bit, dens in lobe_densities(mat, entering, wo, dirs, per_lobe).items():
        f_i, r_i = per_lobe[0][bit]
        wb, raw = _weight(r_i, p_cos, f_i, c, r_i)
        live = dens > 0
        total = total + (w * dens) @ np.where(live[:, None], wb, 0.0)
        if live.any():
            peak = max(peak, float(np.nanmax(raw[live])))
        mass += float(w @ dens)
    lost = max(1.0 - mass, 0.0)
    return total + lost, peak, lost


def first_vertex_directional(bsdf_lobes, mat, cos_o, angle_deg, entering=True, n_r=24, n_phi=48):
    """Expected regularized weight (rgb, per unit Le) of pt.cu's directional-light NEE (pt.cu:772-793) at a point whose shading
    normal is the light's direction, seen at cos theta_o.  The shadow ray aims at a point drawn uniformly on a disk of radius
    1e9 tan(angle / 2) at distance 1e9 (sample_position_on_directional_light, pt.cu:324-342), so wi = normalize(n + tan(angle / 2) d)
    with d uniform on the unit disk of the plane; pdf = 1, MIS against eval_pdf.  Returns (expected weight (3,), largest unclamped)."""
    x, wx = np.polynomial.legendre.leggauss(n_r)
    rr, wr = 0.5 * (x + 1.0), 0.5 * wx
    ph, wp = np.polynomial.legendre.leggauss(n_phi)
    ph, wp = np.pi * (ph + 1.0), np.pi * wp
    R, P = np.meshgrid(rr, ph, indexing="ij")
    W = ((wr * rr)[:, None] * wp[None, :] / np.pi).ravel()  # uniform on the unit disk: r dr dphi / pi
    t = np.tan(np.radians(0.5 * angle_deg))
    d = np.stack([t * R * np.cos(P), np.ones_like(R), t * R * np.sin(P)], axis=-1).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    wo = wo_at(cos_o)
    n = len(d)
    r = bsdf_lobes(mat, entering, 127, np.repeat(wo[None, :].astype(np.float32), n, 0), d.astype(np.float32), np.zeros(n, np.float32),
                   np.full((n, 2), 0.5, np.float32)).astype(np.float64)
    wc, raw = _weight(np.ones(n), r[:, 3], r[:, 0:3], np.abs(d[:, 1]), np.ones(n))
    return W @ wc, float(raw.max())


# ---------------------------------------------------------------------------------------------------------------------------------
def polygon_irradiance(x, normal, poly):
    """Lambert's formula: the irradiance at x (normal `normal`) from a uniform polygon of unit radiance, fully above x's tangent
    plane: (1/2) sum_k angle(v_k, v_k+1) * dot(normal, normalize(v_k x v_k+1)), v_k = poly_k - x.  x (N, 3), poly (K, 3)."""
    x = np.asarray(x, np.float64)
    v = np.asarray(poly, np.float64)[None, :, :] - x[:, None, :]
    v /= np.linalg.norm(v, axis=2, keepdims=True)
    a, b = v, np.roll(v, -1, axis=1)
    cr = np.cross(a, b)
    ang = np.arctan2(np.linalg.norm(cr, axis=2), np.einsum("nkj,nkj->nk", a, b))
    g = cr / np.maximum(np.linalg.norm(cr, axis=2, keepdims=True), 1e-300)
    return np.abs(0.5 * (ang * (g @ np.asarray(normal, np.float64))).sum(axis=1))


def two_plane_radiance(rho_floor, rho_ceiling, le, max_depth):
    """Expected radiance of pt.cu's loop (pt.cu:455-472) at a grey Lambertian floor under a parallel, infinite, grey Lambertian
    ceiling that emits le downwards, constant background 0.  At the floor (depths 0, 2, 4, ...) NEE and the BSDF-sampled light ray
    together add rho_floor * le (their MIS weights sum to 1); at the ceiling (depths 1, 3, ...) nothing is added: its emission
    counts only at a first hit (pt.cu:752-759), its own plane lies on its horizon and its light ray finds the floor, le = 0.  Each
    continuation multiplies the throughput by the albedo, and roulette divides it back to 1 (prr = luminance(throughput) = albedo,
    the throughput / prr of pt.cu:457-462), so the floor's k-th visit adds (rho_floor rho_ceiling)^k rho_floor le."""
    n_floor = (int(max_depth) + 1) // 2
    q = rho_floor * rho_ceiling
    return rho_floor * le * sum(q ** k for k in range(n_floor))
