"""The device's ray / triangle hits against exact float64 geometry (-m gpu): the five tests of test_trace_exact_host.py, on the same scenes and rays
(tests/exact_geometry.py, fixed seeds), through Renderer.trace_rays.

Every test also asserts bit equality with the checker's test of every face on the same rays.  That tells a device bug from a shared one: where only the exact
check fails, device and checker are wrong together; where parity fails and the checker still passes the exact check, the bug is in fh_trace.h, bvh_build.hip
or the kernels that inline them.  The caps and what they rest on are described in test_trace_exact_host.py.
"""
import numpy as np
import pytest

import exact_geometry as G
import fredholm_amd as F
from fredholm_amd import native as N

pytestmark = pytest.mark.gpu

CAP = 16.0  # units of 2^-24 L / cos theta (test_trace_exact_host.py)

_checker = {}
_traced = {}


@pytest.fixture(autouse=True, params=["auto", "stream"])
def traversal_kernels(request, monkeypatch):
    """Every test of this file runs twice: with the library's own choice of traversal kernels (fixed 64-ray batches for trees under 4096 nodes, which is
    what these small scenes build) and with the streaming kernels forced (FH_STREAM=1, read when a context is created) -- the kernels every big scene uses."""
    if request.param == "stream":
        monkeypatch.setenv("FH_STREAM", "1")
    else:
        monkeypatch.delenv("FH_STREAM", raising=False)
    yield request.param


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _renderer(scene):
    r = F.Renderer(0)  # (its own context: FH_STREAM is read when one is created)
    r.load_scene(scene)
    r.build_ias()
    return r


def _trace(r, oracle, scene, rays, key=None):
    """closest hits and occlusion on the device; the closest hits asserted bit-identical to the checker's test of every face"""
    tuv, prim = r.trace_rays(rays)
    occ = r.trace_rays(rays, any_hit=True)[1] != G.MISS
    if key is None or key not in _checker:
        ref = oracle.Scene(scene).trace(rays, brute=True)
        if key is not None:
            _checker[key] = ref
    else:
        ref = _checker[key]
    assert np.array_equal(prim, ref[1]), f"{int((prim != ref[1]).sum())} faces differ from the checker's"
    assert np.array_equal(_bits(tuv), _bits(ref[0]))
    assert np.array_equal(occ, ref[1] != G.MISS)
    return tuv, prim, occ


def _seam(oracle, case, kernels):
    if (case, kernels) not in _traced:
        sc, V, rays = G.seam_case(*case)
        r = _renderer(sc)
        try:
            tuv, prim = r.trace_rays(rays)
            occ = r.trace_rays(rays, any_hit=True)[1] != G.MISS
        finally:
            r.close()
        if case not in _checker:
            _checker[case] = oracle.Scene(sc).trace(rays, brute=True)
        _traced[(case, kernels)] = (tuv, prim, occ)
    return _traced[(case, kernels)] + (_checker[case],)


@pytest.mark.parametrize("case", G.SEAM_CASES, ids=G.SEAM_IDS)
def test_no_ray_gets_through_a_mesh(oracle, traversal_kernels, case):
    tuv, prim, occ, ref = _seam(oracle, case, traversal_kernels)
    assert prim.shape == (40000,)
    assert int((prim == G.MISS).sum()) == 0
    assert int((~occ).sum()) == 0
    assert np.array_equal(prim, ref[1]) and np.array_equal(_bits(tuv), _bits(ref[0]))


@pytest.mark.parametrize("case", G.SEAM_CASES, ids=G.SEAM_IDS)
def test_a_hit_lies_where_the_ray_meets_the_face(oracle, traversal_kernels, case):
    tuv, prim, occ, ref = _seam(oracle, case, traversal_kernels)
    sc, V, rays = G.seam_case(*case)
    et, ex, g = G.hit_errors(rays, tuv, prim, V)
    ct, cx, _ = G.hit_errors(rays, ref[0], ref[1], V)
    print(f"{G.SEAM_IDS[G.SEAM_CASES.index(case)]} ({traversal_kernels}): device t off by at most {et.max():.2f} units, the point by {ex.max():.2f}; checker {ct.max():.2f} and {cx.max():.2f}")
    assert et.size > 0
    assert et.max() <= CAP, et.max()
    assert ex.max() <= CAP, ex.max()
    assert np.array_equal(prim, ref[1]) and np.array_equal(_bits(tuv), _bits(ref[0]))


@pytest.mark.parametrize("name", G.DECIDED_CASES)
def test_hits_agree_with_exact_geometry_where_geometry_decides(oracle, name):
    sc, V, rays, want = G.decided_case(name)
    r = _renderer(sc)
    try:
        tuv, prim, occ = _trace(r, oracle, sc, rays, key=("decided", name))
    finally:
        r.close()
    clear = ~want["ambiguous"]
    assert want["ambiguous"].mean() <= 0.01
    assert np.array_equal((prim != G.MISS)[clear], want["hit"][clear])
    assert np.array_equal(prim[clear], want["prim"][clear])
    assert np.array_equal(occ[clear], want["hit"][clear])


@pytest.mark.parametrize("case", G.TIE_CASES, ids=G.TIE_IDS)
def test_exact_ties_take_the_lowest_face_id(oracle, case):
    sc, rays, want = G.tie_case(*case)
    r = _renderer(sc)
    try:
        tuv, prim, occ = _trace(r, oracle, sc, rays, key=("tie", case))
    finally:
        r.close()
    assert (prim != G.MISS).all() and occ.all()
    assert (tuv[:, 0] == np.float32(1.5)).all()
    assert np.array_equal(prim, want), np.flatnonzero(prim != want)


@pytest.mark.parametrize("case", G.TIE_CASES, ids=G.TIE_IDS)
def test_edge_functions_that_cancel_in_float32_take_their_exact_sign(oracle, case):
    sc, V, rays, inside = G.cancel_case(*case)
    r = _renderer(sc)
    try:
        tuv, prim, occ = _trace(r, oracle, sc, rays, key=("cancel", case))
    finally:
        r.close()
    assert np.array_equal(prim != G.MISS, inside), np.flatnonzero((prim != G.MISS) != inside)
    assert np.array_equal(occ, inside)
    assert np.array_equal(prim[inside], np.arange(64, dtype=np.uint32)[inside])
    assert max(x.max() for x in G.hit_errors(rays, tuv, prim, V)[:2]) <= CAP


@pytest.mark.parametrize("case", G.FLOOR_CASES, ids=G.FLOOR_IDS)
def test_where_surfaces_start_to_shadow_themselves(oracle, traversal_kernels, case):
    S_half, tilted = case
    sc, V, rays = G.floor_case(S_half, tilted)
    r = _renderer(sc)
    try:
        tuv, prim, _ = _trace(r, oracle, sc, rays, key=("floor", case))

        def offset(p, n):
            out = np.zeros_like(p)
            N.check(r._ctx, N.lib().fh_kat_offset_origin(r._ctx, p.shape[0], N.ptr(p), N.ptr(n), N.ptr(out)), "fh_kat_offset_origin")
            return out

        leaving, nrm = G.leaving_rays(sc, rays, tuv, prim, offset, seed=77)
        # (from here on the device's hits equal the checker's ray for ray: all that is asserted beyond the half-extent of 20)
        _, again, _ = _trace(r, oracle, sc, leaving)
    finally:
        r.close()
    assert (prim != G.MISS).mean() > 0.99
    share = (again != G.MISS).mean()
    print(f"floor {G.FLOOR_IDS[G.FLOOR_CASES.index(case)]} ({traversal_kernels}): {share:.2%} of {leaving.shape[0]} leaving rays hit the floor again")
    if S_half <= G.FLOOR_CLEAN_UP_TO:
        assert share == 0.0
