"""Resampling of the light table's picks by distance and facing (fh_set_light_resampling), restated in numpy from the paragraph of include/fredholm_hip.h -- not from
csrc/fh_lights.h, with which it shares no code -- bit for bit in float32: proxies, geometric weight, candidates, u_sel, choice and ratio.  And a float64 model on top
of light_sampling_model.py: the exact marginal of the chosen emitter at a point, and the first-vertex moments of a Lambertian floor with the resampled density in
the division and the table's in the MIS weight."""
import numpy as np

import light_sampling_model as LM

f32 = np.float32
u32 = np.uint32
FLOOR = f32(0.0625)
G_MIN, G_MAX = f32(1e-30), f32(1e30)
SALT = 0x9E3779B9
CANDIDATES = (1, 2, 4, 8, 16)


def refused(m):
    return m not in CANDIDATES


# ------------------------------------------------------------------------------------------------ the arithmetic of the header, float32
def proxies(corners, normals, area):
    """corners, normals: (n, 3, 3) float32 (corner, component); area (n,) -> (n, 8) float32: (c.x, c.y, c.z, a), (m.x, m.y, m.z, 0)"""
    p, nn, a = np.asarray(corners, f32), np.asarray(normals, f32), np.asarray(area, f32)
    out = np.zeros((len(p), 8), f32)
    with np.errstate(all="ignore"):
        out[:, 0:3] = (((p[:, 0] + p[:, 1]).astype(f32) + p[:, 2]).astype(f32) / f32(3.0)).astype(f32)
        out[:, 3] = a
        s = ((nn[:, 0] + nn[:, 1]).astype(f32) + nn[:, 2]).astype(f32)
        sq = (((s[:, 0] * s[:, 0]).astype(f32) + (s[:, 1] * s[:, 1]).astype(f32)).astype(f32) + (s[:, 2] * s[:, 2]).astype(f32)).astype(f32)
        ln = np.sqrt(sq).astype(f32)
        ok = (ln > 0) & (ln <= f32(3.0e38))
        out[:, 4:7] = np.where(ok[:, None], (s / ln[:, None]).astype(f32), f32(0.0))
    return out


def _dot(ax, ay, az, bx, by, bz):
    return (((ax * bx).astype(f32) + (ay * by).astype(f32)).astype(f32) + (az * bz).astype(f32)).astype(f32)


def geom(prox, so, ns):
    """prox (m, 8): the proxy of each row's emitter; so, ns (m, 3) -> G (m,) float32"""
    prox, so, ns = np.asarray(prox, f32), np.asarray(so, f32), np.asarray(ns, f32)
    with np.errstate(all="ignore"):
        v = (prox[:, 0:3] - so).astype(f32)
        r2 = _dot(v[:, 0], v[:, 1], v[:, 2], v[:, 0], v[:, 1], v[:, 2])
        r = np.sqrt(r2).astype(f32)
        d = (v / r[:, None]).astype(f32)
        cs = (np.fmax(_dot(ns[:, 0], ns[:, 1], ns[:, 2], d[:, 0], d[:, 1], d[:, 2]), f32(0.0)) + FLOOR).astype(f32)
        cl = (np.fmax(-_dot(prox[:, 4], prox[:, 5], prox[:, 6], d[:, 0], d[:, 1], d[:, 2]), f32(0.0)) + FLOOR).astype(f32)
        g = ((cs * cl).astype(f32) / (r2 + prox[:, 3]).astype(f32)).astype(f32)
        return np.fmin(np.fmax(g, G_MIN), G_MAX).astype(f32)


def candidate_draws(u1, m):
    """u1 (k,) -> u (k, m) float32: the stratified copies of the one draw"""
    u1 = np.asarray(u1, f32)
    t = (u1 * f32(m)).astype(f32)
    j = np.minimum(t.astype(np.int64), m - 1)
    v = (t - j.astype(f32)).astype(f32)
    k = np.arange(m, dtype=f32)[None, :]
    return np.fmin(((k + v[:, None]).astype(f32) / f32(m)).astype(f32), LM.BELOW_ONE).astype(f32)


def _rotl17(h):
    return ((h << u32(17)) | (h >> u32(15))).astype(u32)


def xxhash32_4(x, y, z, w):
    with np.errstate(over="ignore"):
        x, y, z, w = (np.asarray(a, u32) for a in (x, y, z, w))
        h = (w + u32(374761393) + x * u32(3266489917)).astype(u32)
        h = (u32(668265263) * _rotl17(h)).astype(u32)
        h = (h + y * u32(3266489917)).astype(u32)
        h = (u32(668265263) * _rotl17(h)).astype(u32)
        h = (h + z * u32(3266489917)).astype(u32)
        h = (u32(668265263) * _rotl17(h)).astype(u32)
        h = (u32(2246822519) * (h ^ (h >> u32(15)))).astype(u32)
        h = (u32(3266489917) * (h ^ (h >> u32(13)))).astype(u32)
        return (h ^ (h >> u32(16))).astype(u32)


def usel(image_idx, n_spp, dim_area, seed_hash):
    h = xxhash32_4(image_idx, n_spp, u32(dim_area), u32(seed_hash) ^ u32(SALT))
    return ((h >> u32(8)).astype(f32) * f32(2.0 ** -24)).astype(f32)


def resample(table, prox, so, ns, u1, u_sel, m):
    """table: light_sampling_model.Table; prox (n, 8); so, ns (k, 3); u1, u_sel (k,) -> (candidates (k, m), G (k, m), chosen index (k,), ratio (k,), S (k,))"""
    so, ns, u_sel = np.asarray(so, f32), np.asarray(ns, f32), np.asarray(u_sel, f32)
    u = candidate_draws(u1, m)
    k = len(u)
    idx = np.stack([table.pick(u[:, c])[0] for c in range(m)], axis=1).astype(np.int64)
    g = np.stack([geom(prox[idx[:, c]], so, ns) for c in range(m)], axis=1)
    run = np.zeros((k, m), f32)
    s = np.zeros(k, f32)
    for c in range(m):
        s = (s + g[:, c]).astype(f32)
        run[:, c] = s
    thr = (u_sel * s).astype(f32)
    over = run > thr[:, None]
    first = np.where(over.any(axis=1), over.argmax(axis=1), m - 1)
    rows = np.arange(k)
    with np.errstate(all="ignore"):
        ratio = (g[rows, first] / (s / f32(m)).astype(f32)).astype(f32)
    return idx.astype(u32), g, idx[rows, first].astype(u32), ratio, s


# ------------------------------------------------------------------------------------------------ the float64 model
def geom64(prox, x, ns):
    """G of every emitter (n,) seen from one point, float64 (the clamp never binds on the scenes this is used for: asserted)"""
    prox, x, ns = np.asarray(prox, np.float64), np.asarray(x, np.float64), np.asarray(ns, np.float64)
    v = prox[:, 0:3] - x
    r2 = (v * v).sum(axis=1)
    d = v / np.sqrt(r2)[:, None]
    g = (np.maximum(d @ ns, 0.0) + 0.0625) * (np.maximum(-(prox[:, 4:7] * d).sum(axis=1), 0.0) + 0.0625) / (r2 + prox[:, 3])
    assert ((g > 1e-30) & (g < 1e30)).all()
    return g


def _pick64(table, u):
    """light_pick as a function of a real u in [0, 1): the emitter of every entry of u"""
    n, U, cdf = table.n, float(table.uniform), table.cdf.astype(np.float64)
    uni = np.minimum((u / U * n).astype(np.int64), n - 1)
    tab = np.clip(np.searchsorted(cdf, (u - U) / (1.0 - U), side="right") - 1, 0, n - 1) if U < 1.0 else uni
    return np.where(u < U, uni, tab)


def pieces(table, m):
    """The candidate sets as v runs over [0, 1): light_pick is piecewise constant in its draw, with breakpoints at U * i / n (the uniform part) and at
    U + (1 - U) * cdf[i] (the table's part); candidate k reads it at (k + v) / m, so in v the breakpoints are m * b - k.  -> (length (p,), candidates (p, m))"""
    n, U = table.n, float(table.uniform)
    b = np.concatenate([U * np.arange(n + 1) / n, U + (1.0 - U) * table.cdf.astype(np.float64)])
    cuts = [np.array([0.0, 1.0])]
    for k in range(m):
        v = m * b - k
        cuts.append(v[(v > 0.0) & (v < 1.0)])
    edges = np.unique(np.concatenate(cuts))
    lo, hi = edges[:-1], edges[1:]
    keep = hi - lo > 0
    lo, hi = lo[keep], hi[keep]
    mid = 0.5 * (lo + hi)
    cand = np.stack([_pick64(table, (k + mid) / m) for k in range(m)], axis=1)
    return hi - lo, cand


def marginal(table, g, m):
    """exact probability of every emitter being the chosen one at a point whose geometric weights are g (n,)"""
    length, cand = pieces(table, m)
    gc = g[cand]
    share = gc / gc.sum(axis=1, keepdims=True)
    out = np.zeros(table.n)
    np.add.at(out, cand.ravel(), (length[:, None] * share).ravel())
    return out


def _emitter_terms(x, normal, rho, tri, le, level):
    """per quadrature piece of one emitter: density of the area draw per unit pick probability, the BSDF density, cos, dA / A, dA cos_l / r2; and rho * le"""
    tri = np.asarray(tri, np.float64)
    y, dA = LM.triangle_quadrature(tri, level)
    A = dA.sum()
    nl = np.cross(tri[1] - tri[0], tri[2] - tri[0])
    nl /= np.linalg.norm(nl)
    d = y - x
    r2 = (d * d).sum(axis=1)
    w = d / np.sqrt(r2)[:, None]
    cos = np.maximum(w @ normal, 0.0)
    cosl = np.abs(w @ nl)
    return r2 / cosl / A, cos / np.pi, cos, dA / A, dA * cosl / r2


def floor_moments(x, normal, rho, tris, les, table, prox, m, level=4, mistake=None, info=None):
    """raw moments 1 .. 4, (4, 3) each, of the area draw with resampling among m candidates and of the BSDF-sampled light ray (light_sampling_model.
    lambert_floor_moments with the table's pick: that draw does not change).  For every piece of v and every candidate k chosen with G_k / S: the emitter's area
    quadrature of  clamp01(w f cos / (p ratio)) Le,  p the TABLE's solid-angle density (it makes w), ratio = G_k / (S / m).
    mistake = "pdf_area": the division is by p, the resampled density forgotten; mistake = "one_site": the resampled density also makes the shade site's w while the
    BSDF-sampled ray keeps the table's -- the two mistakes the unbiasedness tests must be able to see.
    The clamp is inside the quadrature: unlike under the table alone (w f cos / p <= rho), a chosen candidate whose ratio is small can lift a Lambertian floor's
    term above 1.  info (a dict) receives clamp_max, the largest unclamped term, and clamped_probability, the probability of a draw that the clamp cuts"""
    x, normal, rho = np.asarray(x, np.float64), np.asarray(normal, np.float64), np.asarray(rho, np.float64)
    P = table.p.astype(np.float64)
    _, mb = LM.lambert_floor_moments(x, normal, rho, tris, les, P, level)
    g = geom64(prox, x, normal)
    length, cand = pieces(table, m)
    gc = g[cand]
    S = gc.sum(axis=1, keepdims=True)
    share, ratio = gc / S, gc / (S / m)
    prob = length[:, None] * share                                     # of (piece, chosen candidate)
    ma = np.zeros((4, 3))
    for e in range(table.n):
        on = cand == e
        if not on.any():
            continue
        p_unit, p_bsdf, cos, da, _ = _emitter_terms(x, normal, rho, tris[e], les[e], level)
        live = cos > 0
        p = p_unit * P[e]
        # the candidate sets repeat from piece to piece: one row per distinct ratio, with the probability of all (piece, candidate) pairs that have it
        rt, inv = np.unique(np.round(ratio[on], 13), return_inverse=True)
        pr = np.bincount(inv.ravel(), weights=prob[on].ravel(), minlength=len(rt))
        if mistake == "one_site":
            pd = p[None, :] * rt[:, None]
            c = pd / (pd + p_bsdf[None, :]) * cos[None, :] / np.pi / pd
        elif mistake == "pdf_area":
            c = np.repeat((p / (p + p_bsdf) * cos / np.pi / p)[None, :], len(rt), axis=0)
        else:
            c = (p / (p + p_bsdf) * cos / np.pi / p)[None, :] / rt[:, None]
        c = np.where(live[None, :], c, 0.0)[:, :, None] * rho[None, None, :]
        if info is not None:
            info["clamp_max"] = max(info.get("clamp_max", 0.0), float(c.max()))
            info["clamped_probability"] = info.get("clamped_probability", 0.0) + float(((pr[:, None] * da[None, :]) * (c.max(axis=2) > 1.0)).sum())
        val = np.minimum(c, 1.0) * np.asarray(les[e], np.float64)[None, None, :]   # clamp01 per channel, then the emission
        wgt = pr[:, None] * da[None, :]
        for k in range(4):
            ma[k] += np.einsum("ij,ijc->c", wgt, val ** (k + 1))
    return ma, mb


def floor_variance(x, normal, rho, tris, les, table, prox, m, level=4):
    """(mean, variance, fourth central moment) per channel of the sum of the two independent draws"""
    ma, mb = floor_moments(x, normal, rho, tris, les, table, prox, m, level)
    e1, v1, k1 = LM.central(ma)
    e2, v2, k2 = LM.central(mb)
    return e1 + e2, v1 + v2, k1 + k2 + 6 * v1 * v2


def first_vertex_emitters_resampled(bsdf_lobes, mat, wo_world, x, tris, les, table, prox, m, level=4, info=None):
    """light_sampling_model.first_vertex_emitters (any material, both draws as integrals over the emitters' area, the clamp inside) with resampling among m candidates:
    the BSDF-sampled light ray's part is that function's, with the table's pick probabilities; the area draw's part is replaced -- emitter e is chosen with ratio rt
    with the probability the pieces of v give, the point is uniform on it, w comes from the TABLE's density p_k and the division is by p_k rt.
    info (a dict) receives clamp_max: the largest unclamped term of the area draw, over the channels"""
    import expectation_model as E
    flip = np.array([1.0, 1.0, -1.0])
    wo = np.asarray(wo_world, np.float64) * flip
    x = np.asarray(x, np.float64)
    P = table.p.astype(np.float64)
    total = LM.first_vertex_emitters(bsdf_lobes, mat, wo_world, x, tris, les, P, level)
    g = geom64(prox, x, np.array([0.0, 1.0, 0.0]))
    length, cand = pieces(table, m)
    gc = g[cand]
    S = gc.sum(axis=1, keepdims=True)
    prob, ratio = length[:, None] * gc / S, gc / (S / m)
    for e, (tri, le) in enumerate(zip(tris, les)):
        tri = np.asarray(tri, np.float64)
        y, dA = LM.triangle_quadrature(tri, level)
        A = dA.sum()
        nl = np.cross(tri[1] - tri[0], tri[2] - tri[0])
        nl /= np.linalg.norm(nl)
        d = y - x
        r2 = (d * d).sum(axis=1)
        wi_w = d / np.sqrt(r2)[:, None]
        cosl = np.abs(wi_w @ nl)
        dirs = wi_w * flip
        c = np.abs(dirs[:, 1])
        pk = r2 / cosl * (P[e] / A)
        n = len(dirs)
        r_all = bsdf_lobes(mat, True, 127, np.repeat(wo[None, :].astype(f32), n, 0), dirs.astype(f32), np.zeros(n, f32), np.full((n, 2), 0.5, f32)).astype(np.float64)
        le = np.asarray(le, np.float64)
        wa, _ = E._weight(pk, r_all[:, 3], r_all[:, 0:3], c, pk)
        total -= ((P[e] / A) * dA) @ (wa * le[None, :])          # the table's area draw, as first_vertex_emitters added it
        on = cand == e
        if not on.any():
            continue
        rt, inv = np.unique(np.round(ratio[on], 13), return_inverse=True)
        pr = np.bincount(inv.ravel(), weights=prob[on].ravel(), minlength=len(rt))
        for q, t in zip(pr, rt):
            wa, raw = E._weight(pk, r_all[:, 3], r_all[:, 0:3], c, pk * t)
            total += (q * dA / A) @ (wa * le[None, :])
            if info is not None:
                info["clamp_max"] = max(info.get("clamp_max", 0.0), float(np.nanmax(raw)))
    return total
