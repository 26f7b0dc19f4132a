"""The checker's ray / triangle hits against exact float64 geometry (tests/exact_geometry.py); the same five tests run on the device in test_gpu_trace_exact.py.

Every traversal test elsewhere compares the device with the checker bit for bit, and the checker's tri_test restates the device's line by line: an axis
permutation, a shear sign, the operands of the fp64 fallback or the barycentric order, misread on both sides, passes all of them.  Here the hits are held to
geometry that shares no code with either:
1. no ray aimed at the shared vertices and edges of a coplanar jittered mesh or from inside a closed star-shaped one gets through ("watertight");
2. a reported hit lies where the ray meets the reported face, to 16 units of 2^-24 L / cos theta in t and in the point rebuilt from (u, v)
   (L: largest |coordinate| of the face seen from the origin; theta: angle between ray and normal).  The form is what the algorithm predicts -- the sheared
   coordinates round in proportion to L, the division by det divides by cos theta; the constant is measured, not derived: on these rays the checker reaches
   the maxima printed by the test (recorded in DESIGN.md 4), and test_checker_stays_well_inside_the_cap fails above 8 rather than let 16 creep;
3. hit or miss, the closest face and occlusion equal exact geometry on every ray that geometry decides by more than 1e-5;
4. a ray exactly on an edge or a vertex -- edge functions exactly 0, the fp64 fallback -- hits at exactly t = 1.5 the lowest face id of those that hold the
   point (equal t resolves to the lower face id); and a ray that passes an edge at a distance float32 products do not resolve -- the
   fallback's other entrance -- is inside or outside as exact arithmetic says;
5. rays leaving a surface from offset_origin's point do not hit it again while the surface's half-extent is <= 20; beyond that they do, and the shares are
   printed (and recorded in DESIGN.md 4) as a stated limit of the reference's fixed offset.
Each test runs on the checker's tree and on its test of every face (brute=True), which have to agree in every bit.

What the suite sees, tried on scratch copies of oracle.cpp's tri_test: bu = W * rcp fails tests 2 and 5 and the second half of 4; leaving the float products
in place of the fp64 fallback fails the second half of 4 (the first half cannot: on dyadic coordinates float and fp64 agree).  Dropping the swap of kx and
ky for a negative d[kz] fails nothing and cannot: without culling it negates U, V, W, det and T together, so t, u, v and the accepted set keep every bit but
the sign of a zero barycentric.
"""
import numpy as np
import pytest

import exact_geometry as G

CAP = 16.0          # units of 2^-24 L / cos theta a reported t and point may be off by
CAP_CHECKER = 8.0   # above this on the checker: investigate, do not raise CAP

_traced = {}
_measured = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _trace(oracle, scene, rays):
    """closest hits by the tree, asserted bit-identical to the test of every face; and the scene for further queries"""
    S = oracle.Scene(scene)
    tuv, prim = S.trace(rays)
    tuv_b, prim_b = S.trace(rays, brute=True)
    assert np.array_equal(prim, prim_b) and np.array_equal(_bits(tuv), _bits(tuv_b))
    return S, tuv, prim


def _seam(oracle, case):
    if case not in _traced:
        sc, V, rays = G.seam_case(*case)
        S, tuv, prim = _trace(oracle, sc, rays)
        occ = S.trace(rays, any_hit=True)[1] != G.MISS
        occ_b = S.trace(rays, any_hit=True, brute=True)[1] != G.MISS
        _traced[case] = (tuv, prim, occ, occ_b)
    return _traced[case]


def _say(capsys, text):
    with capsys.disabled():
        print("\n  " + text, end="")


def test_the_meshes_are_what_the_tests_assume():
    """closed or coplanar, shared vertices shared to the bit, no face folded over by the jitter, the float64 reference consistent with itself"""
    for k, placement in enumerate(G.PLACEMENTS):
        sc, V = G.jittered_plane(12, placement)
        assert V.shape == (3 * 288, 3) and np.unique(V[:, 1]).size == 1 and np.unique(V, axis=0).shape[0] == 169
        assert (sc["normals"][:, 1] > 0.999).all()
        sc, V = G.star_sphere(24, 12, placement)
        assert V.shape == (3 * 528, 3) and np.unique(V, axis=0).shape[0] == 24 * 11 + 2
        tri = V.astype(np.float64).reshape(-1, 3, 3)
        # closed: every directed edge has its opposite exactly once
        key = lambda a, b: [(tuple(x), tuple(y)) for x, y in zip(a, b)]
        edges = sum((key(tri[:, i], tri[:, (i + 1) % 3]) for i in range(3)), [])
        assert len(set(edges)) == len(edges) and set(edges) == {(b, a) for a, b in edges}
        # star-shaped about its centre: every face's plane has the centre behind it
        centre = np.asarray(placement[1], np.float64)
        assert ((np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]) * (tri[:, 0] - centre)).sum(axis=1) > 0).all()
    for axis in range(3):
        V = G.dyadic_plane(8, axis)[1]
        assert np.array_equal(V * 8, np.round(V * 8)) and (V[:, axis] == 0.25).all()
    sc, V, rays = G.seam_case("sphere", 1)
    g = G.on_face(rays[:2000], np.arange(2000) % 528, V)
    assert np.allclose(g["det"], -g["n_dot_d"], rtol=1e-9, atol=1e-12)  # the edge functions and the plane equation are two routes to one number
    inside = g["inside"]
    rebuilt = (1 - g["bu"] - g["bv"])[:, None] * g["tri"][:, 0] + g["bu"][:, None] * g["tri"][:, 1] + g["bv"][:, None] * g["tri"][:, 2]
    assert inside.any() and np.abs(rebuilt - g["X"])[inside].max() < 1e-9


@pytest.mark.parametrize("case", G.SEAM_CASES, ids=G.SEAM_IDS)
def test_no_ray_gets_through_a_mesh(oracle, case):
    tuv, prim, occ, occ_b = _seam(oracle, case)
    assert prim.shape == (40000,)
    assert int((prim == G.MISS).sum()) == 0
    assert int((~occ).sum()) == 0 and int((~occ_b).sum()) == 0


@pytest.mark.parametrize("case", G.SEAM_CASES, ids=G.SEAM_IDS)
def test_a_hit_lies_where_the_ray_meets_the_face(oracle, capsys, case):
    tuv, prim, _, _ = _seam(oracle, case)
    sc, V, rays = G.seam_case(*case)
    et, ex, g = G.hit_errors(rays, tuv, prim, V)
    _measured[case] = (et.max(), ex.max())
    _say(capsys, f"checker {G.SEAM_IDS[G.SEAM_CASES.index(case)]}: t off by at most {et.max():.2f} units (99.9 %: {np.quantile(et, 0.999):.2f}), the point by {ex.max():.2f} "
                 f"(99.9 %: {np.quantile(ex, 0.999):.2f}); smallest cos theta {g['cos'].min():.1e}")
    assert et.size > 0 and g["inside"].mean() > 0.5  # (the reported face is one the exact ray passes through, or a neighbour by a rounding)
    assert et.max() <= CAP, et.max()
    assert ex.max() <= CAP, ex.max()


def test_checker_stays_well_inside_the_cap(oracle):
    for case in G.SEAM_CASES:
        if case not in _measured:
            tuv, prim, _, _ = _seam(oracle, case)
            sc, V, rays = G.seam_case(*case)
            et, ex, _ = G.hit_errors(rays, tuv, prim, V)
            _measured[case] = (et.max(), ex.max())
    worst = max(max(v) for v in _measured.values())
    assert worst <= CAP_CHECKER, _measured


@pytest.mark.parametrize("name", G.DECIDED_CASES)
def test_hits_agree_with_exact_geometry_where_geometry_decides(oracle, capsys, name):
    sc, V, rays, want = G.decided_case(name)
    S, tuv, prim = _trace(oracle, sc, rays)
    clear = ~want["ambiguous"]
    _say(capsys, f"checker {name}: {want['ambiguous'].mean():.2%} of the rays ambiguous, {want['hit'].mean():.1%} hit")
    assert want["ambiguous"].mean() <= 0.01
    assert 0.2 <= want["hit"].mean() <= 0.95
    assert np.array_equal((prim != G.MISS)[clear], want["hit"][clear])
    assert np.array_equal(prim[clear], want["prim"][clear])
    for brute in (False, True):
        occ = S.trace(rays, any_hit=True, brute=brute)[1] != G.MISS
        assert np.array_equal(occ[clear], want["hit"][clear])


@pytest.mark.parametrize("case", G.TIE_CASES, ids=G.TIE_IDS)
def test_exact_ties_take_the_lowest_face_id(oracle, case):
    sc, rays, want = G.tie_case(*case)
    S, tuv, prim = _trace(oracle, sc, rays)
    assert rays.shape[0] == 49 + 56 + 56 + 64
    assert (prim != G.MISS).all()
    assert (tuv[:, 0] == np.float32(1.5)).all()
    assert np.array_equal(prim, want), np.flatnonzero(prim != want)
    assert (S.trace(rays, any_hit=True)[1] != G.MISS).all()


@pytest.mark.parametrize("case", G.TIE_CASES, ids=G.TIE_IDS)
def test_edge_functions_that_cancel_in_float32_take_their_exact_sign(oracle, case):
    """the other way into the fp64 fallback: the float32 products of an edge function round to the same number while the exact value is +-2^-26 -- outside the
    triangle on 32 of the 64 rays, inside on the other 32 (exact_geometry.cancel_case).  Taking the float 0 for "on the edge" would hit all 64."""
    sc, V, rays, inside = G.cancel_case(*case)
    S, tuv, prim = _trace(oracle, sc, rays)
    assert inside.sum() == 32
    assert np.array_equal(prim != G.MISS, inside), np.flatnonzero((prim != G.MISS) != inside)
    assert np.array_equal(prim[inside], np.arange(64, dtype=np.uint32)[inside])
    assert max(x.max() for x in G.hit_errors(rays, tuv, prim, V)[:2]) <= CAP
    for brute in (False, True):
        assert np.array_equal(S.trace(rays, any_hit=True, brute=brute)[1] != G.MISS, inside)


def _host_offset(oracle):
    return lambda p, n: np.array([oracle.offset_origin(a, b) for a, b in zip(p, n)], np.float32).reshape(-1, 3)


@pytest.mark.parametrize("case", G.FLOOR_CASES, ids=G.FLOOR_IDS)
def test_where_surfaces_start_to_shadow_themselves(oracle, capsys, case):
    S_half, tilted = case
    sc, V, rays = G.floor_case(S_half, tilted)
    S, tuv, prim = _trace(oracle, sc, rays)
    assert (prim != G.MISS).mean() > 0.99
    assert max(x.max() for x in G.hit_errors(rays, tuv, prim, V)[:2]) <= CAP
    leaving, nrm = G.leaving_rays(sc, rays, tuv, prim, _host_offset(oracle), seed=77)
    assert ((leaving[:, 3:6] * nrm).sum(axis=1) >= 0).all()
    _, _, again = _trace(oracle, sc, leaving)
    share = (again != G.MISS).mean()
    _say(capsys, f"checker floor {G.FLOOR_IDS[G.FLOOR_CASES.index(case)]}: {share:.2%} of {leaving.shape[0]} leaving rays hit the floor again")
    if S_half <= G.FLOOR_CLEAN_UP_TO:
        assert share == 0.0
