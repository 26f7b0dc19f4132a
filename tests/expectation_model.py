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
