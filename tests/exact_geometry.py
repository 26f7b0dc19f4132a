"""Exact float64 ray / triangle geometry for test_trace_exact_host.py and test_gpu_trace_exact.py (a plain helper module, not a conftest).

The device's tri_test (fredholm_amd/csrc/fh_trace.h) and the checker's (oracle/oracle.cpp) are the same lines, so the parity suite cannot see a
misreading made in both.  Nothing here is taken from either: no shear, no dominant axis, no fallback.  A ray is the float32 origin and direction exactly
as given, a triangle its three float32 vertices, and everything else is numpy float64:

    U = d . (C x B)    V = d . (A x C)    W = d . (B x A)        with A, B, C the vertices minus the origin

are the signed edge functions (scalar triple products).  The ray's line passes through the closed triangle iff they do not have mixed signs; U, V, W over
their sum are the barycentric weights of p0, p1, p2 (the hit attributes u, v are those of p1 and p2); t comes from the plane equation
n . (p0 - o) = t n . d with n = (p1 - p0) x (p2 - p0), which uses none of the three.

Meshes are built in float64, placed (scaled, then shifted) in float64 and only then cast to float32; faces index ONE float32 point table, so shared edges
and vertices are shared to the last bit -- which is all "watertight" promises anything about.  Everything is seeded: the host suite and the GPU suite see
identical scenes and rays.
"""
import functools

import numpy as np

from fredholm_amd import scenes
from fredholm_amd.native import default_materials

MISS = 0xFFFFFFFF
PLACEMENTS = ((1.0, (0.0, 0.0, 0.0)), (1.0, (3.0, 5.0, -2.0)), (16.0, (40.0, -20.0, 10.0)), (1.0 / 64.0, (0.0, 0.0, 0.0)))
IDENTITY = PLACEMENTS[0]


# ------------------------------------------------------------------ meshes
def _place(p64, placement):
    scale, shift = placement
    return (np.asarray(p64, np.float64) * scale + np.asarray(shift, np.float64)).astype(np.float32)


def _mesh(points32, faces):
    """(scene, float32 vertex array [3 * faces, 3]) of faces that index one table of float32 points"""
    faces = np.asarray(faces, np.int64)
    sc = scenes._finish(points32[faces.reshape(-1)], np.zeros(faces.shape[0], np.uint32), default_materials(1))
    return sc, sc["vertices"]


def _grid(n, axis, height, jitter_rng=None):
    """(n+1)^2 points over [-1,1]^2 at `height` along `axis` and 2 n^2 faces whose normal is +axis; the diagonal alternates from column to column, so an
    interior vertex belongs to six faces.  In-plane axes: (axis + 1) % 3 carries the column index i, (axis + 2) % 3 the row index j."""
    p, q = (axis + 1) % 3, (axis + 2) % 3
    k = np.arange(n + 1)
    i, j = np.meshgrid(k, k, indexing="xy")  # point id = j * (n + 1) + i
    uv = np.stack([-1.0 + 2.0 * i / n, -1.0 + 2.0 * j / n], axis=-1).reshape(-1, 2)
    if jitter_rng is not None:
        inner = ((i > 0) & (i < n) & (j > 0) & (j < n)).reshape(-1)
        uv[inner] += jitter_rng.uniform(-0.3, 0.3, (int(inner.sum()), 2)) * (2.0 / n)
    pts = np.zeros((uv.shape[0], 3))
    pts[:, p], pts[:, q], pts[:, axis] = uv[:, 0], uv[:, 1], height
    faces = []
    for cj in range(n):
        for ci in range(n):
            a, b, c, d = cj * (n + 1) + ci, cj * (n + 1) + ci + 1, (cj + 1) * (n + 1) + ci + 1, (cj + 1) * (n + 1) + ci  # counterclockwise seen from +axis
            faces += [(a, b, c), (a, c, d)] if ci % 2 == 0 else [(a, b, d), (b, c, d)]
    return pts, np.asarray(faces)


def jittered_plane(n=12, placement=IDENTITY, seed=101):
    """All faces coplanar (y = 0 before the placement, one float32 y after it): every ray into the footprint has to hit."""
    pts, faces = _grid(n, 1, 0.0, np.random.default_rng(seed))
    return _mesh(_place(pts, placement), faces)


def dyadic_plane(n=8, axis=1, placement=IDENTITY):
    """Every coordinate a multiple of 1 / n: vertices, edge midpoints and the edge functions of axis-parallel rays through them are exact in float32."""
    pts, faces = _grid(n, axis, 0.25)
    return _mesh(_place(pts, placement), faces)


def star_sphere(nu=24, nv=12, placement=IDENTITY, seed=202):
    """A closed UV sphere about the origin, every vertex at its own radius 1 +- 0.2: a ray from anywhere inside has to hit."""
    rng = np.random.default_rng(seed)
    pts = [(0.0, 1.0, 0.0)]
    for k in range(1, nv):
        th = np.pi * k / nv
        for i in range(nu):
            ph = 2.0 * np.pi * i / nu
            pts.append((np.sin(th) * np.cos(ph), np.cos(th), np.sin(th) * np.sin(ph)))
    pts.append((0.0, -1.0, 0.0))
    pts = np.asarray(pts) * rng.uniform(0.8, 1.2, (len(pts), 1))
    ring = lambda k, i: 1 + (k - 1) * nu + i % nu
    south = len(pts) - 1
    faces = []
    for i in range(nu):
        faces.append((0, ring(1, i), ring(1, i + 1)))
        faces.append((south, ring(nv - 1, i + 1), ring(nv - 1, i)))
        for k in range(1, nv - 1):
            a, b, c, d = ring(k, i), ring(k + 1, i), ring(k + 1, i + 1), ring(k, i + 1)
            faces += [(a, b, c), (a, c, d)] if (i + k) % 2 == 0 else [(a, b, d), (b, c, d)]
    faces = np.asarray(faces)
    tri = pts[faces]
    inward = (np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]) * tri.mean(axis=1)).sum(axis=1) < 0.0
    faces[inward] = faces[inward][:, ::-1]  # normals point away from the centre
    return _mesh(_place(pts, placement), faces)


FLOOR_TILT = (0.37, 0.21)  # radians about z, then about x


def floor_rotation(tilted):
    if not tilted:
        return np.eye(3)
    (cz, sz), (cx, sx) = [(np.cos(a), np.sin(a)) for a in FLOOR_TILT]
    return np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])


def floor_quad(S, tilted=False, placement=IDENTITY):
    """Two triangles of half-extent S through the origin, normal +y before the tilt."""
    pts = np.array([(-S, 0, S), (S, 0, S), (S, 0, -S), (-S, 0, -S)], np.float64) @ floor_rotation(tilted).T
    return _mesh(_place(pts, placement), [(0, 1, 2), (0, 2, 3)])


# ------------------------------------------------------------------ rays
def _pack(o32, d, tmax=1e9):
    n = o32.shape[0]
    return np.ascontiguousarray(np.concatenate([o32, np.asarray(d, np.float32), np.broadcast_to(np.asarray(tmax, np.float32), (n,)).reshape(n, 1)], axis=1), dtype=np.float32)


def random_dirs(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def aimed(rng, targets, n, lo, hi, tmax=1e9):
    """n rays from float32 origins uniform in the box [lo, hi], each towards a target picked at random: normalize(target - origin) in float64, cast to float32"""
    o = rng.uniform(np.asarray(lo, np.float64), np.asarray(hi, np.float64), (n, 3)).astype(np.float32)
    d = np.asarray(targets, np.float64)[rng.integers(0, len(targets), n)] - o.astype(np.float64)
    return _pack(o, d / np.linalg.norm(d, axis=1, keepdims=True), tmax)


def edge_points(scene, rng, n):
    """n random points on random edges of the mesh (float64 combinations of the float32 end points)"""
    v = scene["vertices"].astype(np.float64).reshape(-1, 3, 3)
    f, k, s = rng.integers(0, v.shape[0], n), rng.integers(0, 3, n), rng.uniform(0.0, 1.0, (n, 1))
    return (1.0 - s) * v[f, k] + s * v[f, (k + 1) % 3]


def seam_targets(scene, rng):
    """where a test that is not watertight leaks: every vertex of the mesh and 4000 points on its edges"""
    return np.concatenate([scene["vertices"].astype(np.float64), edge_points(scene, rng, 4000)])


# ------------------------------------------------------------------ the float64 reference
def _geometry(o, d, p0, p1, p2):
    A, B, C = p0 - o, p1 - o, p2 - o
    U, V, W = (d * np.cross(C, B)).sum(-1), (d * np.cross(A, C)).sum(-1), (d * np.cross(B, A)).sum(-1)
    det = U + V + W
    nrm = np.cross(p1 - p0, p2 - p0)
    nd = (nrm * d).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (nrm * A).sum(-1) / nd
        bw, bu, bv = U / det, V / det, W / det
    mixed = ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))
    inside = ~mixed & (det != 0.0)
    margin = np.where(det != 0.0, np.minimum(bw, np.minimum(bu, bv)), -np.inf)
    return dict(U=U, V=V, W=W, det=det, t=t, bu=bu, bv=bv, inside=inside, margin=margin, normal=nrm, n_dot_d=nd)


def exact_hit(rays, V):
    """every ray against every triangle: arrays [rays, faces]"""
    r = np.asarray(rays, np.float64)
    tri = np.asarray(V, np.float64).reshape(1, -1, 3, 3)
    return _geometry(r[:, None, 0:3], r[:, None, 3:6], tri[:, :, 0], tri[:, :, 1], tri[:, :, 2])


def on_face(rays, prim, V):
    """every ray against the one face `prim` names for it: arrays [rays], plus the intersection point X, cos of the angle between ray and normal, and
    L, the largest |coordinate| of a vertex of the face seen from the origin"""
    r = np.asarray(rays, np.float64)
    tri = np.asarray(V, np.float64).reshape(-1, 3, 3)[np.asarray(prim, np.int64)]
    o, d = r[:, 0:3], r[:, 3:6]
    g = _geometry(o, d, tri[:, 0], tri[:, 1], tri[:, 2])
    g["X"] = o + g["t"][:, None] * d
    g["cos"] = np.abs(g["n_dot_d"]) / (np.linalg.norm(g["normal"], axis=1) * np.linalg.norm(d, axis=1))
    g["L"] = np.abs(tri - o[:, None, :]).max(axis=(1, 2))
    g["tri"] = tri
    return g


def hit_errors(rays, tuv, prim, V):
    """(error of t along the ray, distance of the reported point from the exact one), both in units of 2^-24 L / cos theta, for the rays that hit"""
    hit = prim != MISS
    r, tuv = np.asarray(rays, np.float64)[hit], np.asarray(tuv, np.float64)[hit]
    g = on_face(r, prim[hit], V)
    unit = 2.0 ** -24 * g["L"] / g["cos"]
    et = np.abs(tuv[:, 0] - g["t"]) * np.linalg.norm(r[:, 3:6], axis=1) / unit
    u, v = tuv[:, 1:2], tuv[:, 2:3]
    point = (1.0 - u - v) * g["tri"][:, 0] + u * g["tri"][:, 1] + v * g["tri"][:, 2]
    return et, np.linalg.norm(point - g["X"], axis=1) / unit, g


AMBIGUITY = 1e-5


def decide(rays, V):
    """What exact geometry says about every ray against ALL faces, and for which rays it says so by less than AMBIGUITY: a face whose smallest barycentric
    weight is within AMBIGUITY of 0 at a distance the ray reaches, two nearest hits closer than AMBIGUITY relative, a hit within AMBIGUITY relative of tmax."""
    g = exact_hit(rays, V)
    tmax = np.asarray(rays, np.float64)[:, 6:7]
    t = g["t"]
    valid = g["inside"] & (t >= 0.0) & (t <= tmax)
    tv = np.where(valid, t, np.inf)
    order = np.sort(tv, axis=1)
    t1, t2 = order[:, 0], (order[:, 1] if tv.shape[1] > 1 else np.full(tv.shape[0], np.inf))
    near_edge = ((np.abs(g["margin"]) < AMBIGUITY) & (t >= 0.0) & (t <= tmax * (1.0 + AMBIGUITY))).any(axis=1)
    with np.errstate(invalid="ignore"):
        near_tie = np.isfinite(t2) & (t2 - t1 < AMBIGUITY * t2)
    near_end = ((g["margin"] > -AMBIGUITY) & (np.abs(t - tmax) <= AMBIGUITY * tmax)).any(axis=1)
    hit = valid.any(axis=1)
    return dict(hit=hit, prim=np.where(hit, tv.argmin(axis=1), MISS).astype(np.uint32), t=t1, ambiguous=near_edge | near_tie | near_end)


# ------------------------------------------------------------------ the cases of the two suites (cached: scenes and rays are read-only)
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def seam_case(kind, placement_index):
    """(scene, V, 40 000 rays) of test 1 and 2.  plane: origins 0.05 .. 2 scene units above the footprint, aimed at vertices and edge points within 0.95 of
    it.  sphere: origins within 0.3 scene units of the centre, 35 000 aimed at vertices and edge points, 5000 in random directions."""
    placement = PLACEMENTS[placement_index]
    scale, shift = placement[0], np.asarray(placement[1], np.float64)
    rng = np.random.default_rng(1000 + 10 * placement_index + (kind == "sphere"))
    if kind == "plane":
        sc, V = jittered_plane(12, placement)
        targets = seam_targets(sc, rng)
        local = (targets - shift) / scale
        targets = targets[(np.abs(local[:, 0]) <= 0.95) & (np.abs(local[:, 2]) <= 0.95)]
        rays = aimed(rng, targets, 40000, shift + scale * np.array([-1.0, 0.05, -1.0]), shift + scale * np.array([1.0, 2.0, 1.0]))
    else:
        sc, V = star_sphere(24, 12, placement)
        rays = aimed(rng, seam_targets(sc, rng), 40000, shift - 0.3 * scale, shift + 0.3 * scale)
        rays[35000:, 3:6] = random_dirs(rng, 5000).astype(np.float32)
    _frozen(V, rays)
    return sc, V, rays


SEAM_CASES = [(kind, k) for kind in ("plane", "sphere") for k in range(len(PLACEMENTS))]
SEAM_IDS = [f"{kind}-{k}" for kind, k in SEAM_CASES]


@functools.lru_cache(maxsize=None)
def decided_case(name):
    """(scene, V, 2000 rays, decide(rays, V)) of test 3: 500 rays in random directions from a box around the scene, 1200 aimed at face centroids, 300 aimed
    likewise that end after 0.05 .. 1.0.  The Cornell box's origins stay above its floor plane: the blocks stand ON the floor, so from below the floor and a
    block's bottom are hit at exactly the same distance, which geometry does not decide."""
    sc = scenes.triangle_soup(500, 0.3) if name == "soup" else scenes.cornell_box()
    V = sc["vertices"]
    rng = np.random.default_rng(31 if name == "soup" else 32)
    lo, hi = V.min(axis=0).astype(np.float64) - 0.3, V.max(axis=0).astype(np.float64) + 0.3
    if name == "cornell":
        lo[1] = 0.01
    centroids = V.astype(np.float64).reshape(-1, 3, 3).mean(axis=1)
    rays = np.concatenate([aimed(rng, centroids, 500, lo, hi), aimed(rng, centroids, 1200, lo, hi), aimed(rng, centroids, 300, lo, hi, rng.uniform(0.05, 1.0, 300))])
    rays[:500, 3:6] = random_dirs(rng, 500).astype(np.float32)
    _frozen(V, rays)
    return sc, V, rays, decide(rays, V)


DECIDED_CASES = ["soup", "cornell"]


@functools.lru_cache(maxsize=None)
def tie_case(axis, side):
    """(scene, rays, expected face ids) of test 4: rays exactly along -+axis from 1.5 away onto every interior vertex of dyadic_plane(8, axis), every midpoint
    of an interior edge along either in-plane axis and every diagonal midpoint.  Such a ray lies exactly on an edge of two faces or on a vertex of six."""
    n = 8
    sc, V = dyadic_plane(n, axis)
    p, q = (axis + 1) % 3, (axis + 2) % 3
    h = 2.0 / n
    inner, cells = -1.0 + h * np.arange(1, n), -1.0 + h * (np.arange(n) + 0.5)
    uv = [(a, b) for a in inner for b in inner] + [(a, b) for a in cells for b in inner] + [(a, b) for a in inner for b in cells] + [(a, b) for a in cells for b in cells]
    uv = np.asarray(uv, np.float64)
    target = np.zeros((uv.shape[0], 3))
    target[:, p], target[:, q], target[:, axis] = uv[:, 0], uv[:, 1], 0.25
    e = np.zeros(3)
    e[axis] = float(side)
    rays = _pack((target + 1.5 * e).astype(np.float32), np.broadcast_to(-e, target.shape))
    assert np.array_equal(rays[:, 0:3].astype(np.float64), target + 1.5 * e)  # dyadic: nothing was rounded
    # the closed triangles that hold the target, in exact (dyadic) float64 arithmetic on the two in-plane coordinates
    tri = V.astype(np.float64).reshape(-1, 3, 3)[:, :, [p, q]]
    a, b, c, x = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2], uv[:, None, :]
    cross = lambda s, t: s[..., 0] * t[..., 1] - s[..., 1] * t[..., 0]
    e0, e1, e2 = cross(b - a, x - a), cross(c - b, x - b), cross(a - c, x - c)
    holds = ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))
    assert (holds.sum(axis=1) >= 2).all() and (holds.sum(axis=1) <= 6).all()
    want = holds.argmax(axis=1).astype(np.uint32)  # the lowest id
    _frozen(rays, want)
    return sc, rays, want


TIE_CASES = [(axis, side) for axis in (0, 1, 2) for side in (1, -1)]
TIE_IDS = [f"{'xyz'[axis]}{'+' if side > 0 else '-'}" for axis, side in TIE_CASES]


def _bezout(a, b):
    """(x, y) with a x + b y = gcd(a, b)"""
    x0, y0, x1, y1 = 1, 0, 0, 1
    while b:
        k = a // b
        a, b, x0, y0, x1, y1 = b, a - k * b, x1, y1, x0 - k * x1, y0 - k * y1
    return x0, y0


@functools.lru_cache(maxsize=None)
def cancel_case(axis, side):
    """(scene, V, rays, exact hit flags) of the second half of test 4: 64 lone triangles and one ray along -+axis for each, which passes an edge B C of its
    triangle at a distance float32 does not resolve.  Seen from the ray, B = (bx, by) 2^-13 and C = (cx, cy) 2^-13 are integer points of opposite directions
    with cx by - cy bx = +-1: the edge function is +-2^-26 exactly, while both float32 products round to one number and their difference is 0 -- the case
    tri_test redoes in fp64.  Every edge is used twice, with the third vertex on either side: the ray is inside one triangle and outside the other by that
    2^-26.  All coordinates keep under 24 bits (triangles sit at multiples of 8, the rays' origins on them), so vertex - origin is exact, float64 evaluates
    the edge functions without any rounding, and the reference's flags are the truth, not an estimate."""
    rng = np.random.default_rng(600 + axis)
    p, q = (axis + 1) % 3, (axis + 2) % 3
    unit = 2.0 ** -13
    pts, origins = [], []
    while len(origins) < 64:
        bx, by = (int(v) for v in rng.integers(2 ** 12, 2 ** 13, 2))
        x, y = _bezout(by, bx)
        if by * x + bx * y != 1:
            continue  # not coprime
        m = int(rng.choice([-1, 1]))
        k = int(round(rng.uniform(0.5, 1.0) + m * x / bx))
        cx, cy = m * x - k * bx, -m * y - k * by  # cx by - cy bx = m, and C close to -s B with s in 0.5 .. 1
        assert cx * by - cy * bx == m
        f = lambda v: np.float32(v * unit)
        if np.float32(f(cx) * f(by)) - np.float32(f(cy) * f(bx)) != 0.0 or cx >= 0 or cy >= 0:
            continue  # (the products did not round to the same float32)
        nrm = np.array([by - cy, cx - bx], np.float64)
        nrm *= 0.75 / (unit * np.linalg.norm(nrm))
        for far in (1, -1):
            ax, ay = (int(v) for v in np.round(far * nrm))
            o = np.array([8.0 * (len(origins) % 8) - 28.0, 8.0 * (len(origins) // 8) - 28.0])
            for vx, vy in ((ax, ay), (bx, by), (cx, cy)):
                point = np.zeros(3)
                point[p], point[q], point[axis] = o[0] + vx * unit, o[1] + vy * unit, 0.25
                pts.append(point)
            start = np.zeros(3)
            start[p], start[q], start[axis] = o[0], o[1], 0.25 + 1.5 * side
            origins.append(start)
    pts, origins = np.asarray(pts), np.asarray(origins)
    assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)  # nothing is rounded
    e = np.zeros(3)
    e[axis] = float(side)
    sc, V = _mesh(pts.astype(np.float32), np.arange(len(pts)).reshape(-1, 3))
    rays = _pack(origins.astype(np.float32), np.broadcast_to(-e, origins.shape))
    g = on_face(rays, np.arange(64), V)
    assert (np.abs(g["bu"] * g["bv"] * (1.0 - g["bu"] - g["bv"])) > 0).all()  # no edge function is 0: every ray is strictly inside or strictly outside
    assert np.array_equal(g["inside"][0::2], ~g["inside"][1::2])           # ... and each edge has the ray inside one of its two triangles
    others = exact_hit(rays, V)["inside"]
    assert np.array_equal(others, np.eye(64, dtype=bool) & g["inside"][:, None])  # no ray reaches a neighbour's triangle
    _frozen(V, rays)
    return sc, V, rays, g["inside"].copy()


@functools.lru_cache(maxsize=None)
def floor_case(S, tilted):
    """(scene, V, 4000 first-hit rays) of test 5: origins 2.5 .. 3.5 units off the surface, aimed at points within 0.95 min(S, 5) of the centre"""
    sc, V = floor_quad(float(S), tilted)
    rng = np.random.default_rng(5000 + int(S) + int(tilted))
    m = 0.95 * min(float(S), 5.0)
    n = 4000
    target = np.stack([rng.uniform(-m, m, n), np.zeros(n), rng.uniform(-m, m, n)], axis=1)
    origin = target + np.stack([rng.uniform(-3.0, 3.0, n), rng.uniform(2.5, 3.5, n), rng.uniform(-3.0, 3.0, n)], axis=1)
    R = floor_rotation(tilted)
    o = (origin @ R.T).astype(np.float32)
    d = target @ R.T - o.astype(np.float64)
    rays = _pack(o, d / np.linalg.norm(d, axis=1, keepdims=True))
    _frozen(V, rays)
    return sc, V, rays


FLOOR_SIZES = [1, 10, 20, 100, 1000, 10000]
FLOOR_CASES = [(S, tilted) for S in FLOOR_SIZES for tilted in (False, True)]
FLOOR_IDS = [f"{S}-{'tilted' if tilted else 'flat'}" for S, tilted in FLOOR_CASES]
FLOOR_CLEAN_UP_TO = 20  # no surface of half-extent <= 20 may shadow itself: the estimator suite's 10-unit tiles depend on it


def leaving_rays(scene, rays, tuv, prim, offset_origin, seed):
    """For every first hit: the point rebuilt in float32 from (u, v) the way the integrator does it, (1 - u - v) p0 + u p1 + v p2, moved off the surface by
    `offset_origin` (arrays [n, 3] of points and normals -> [n, 3]) along the face normal on the ray's side, and from there a ray in a random direction of
    that side's hemisphere.  Returns (rays, their normals)."""
    rng = np.random.default_rng(seed)
    v = random_dirs(rng, rays.shape[0])  # drawn for every ray, so that the directions do not depend on which rays hit
    hit = prim != MISS
    f = prim[hit].astype(np.int64)
    tri = scene["vertices"].reshape(-1, 3, 3)[f]
    u, w = tuv[hit, 1:2].astype(np.float32), tuv[hit, 2:3].astype(np.float32)
    x = (np.float32(1.0) - u - w) * tri[:, 0] + u * tri[:, 1] + w * tri[:, 2]
    assert x.dtype == np.float32
    nrm = scene["normals"][3 * f].astype(np.float32)
    nrm = np.where((nrm.astype(np.float64) * rays[hit, 3:6]).sum(axis=1, keepdims=True) > 0.0, -nrm, nrm)
    v = v[hit]
    v = np.where((v * nrm).sum(axis=1, keepdims=True) < 0.0, -v, v)
    start = np.ascontiguousarray(offset_origin(np.ascontiguousarray(x), np.ascontiguousarray(nrm)), dtype=np.float32)
    return _pack(start, v), nrm
