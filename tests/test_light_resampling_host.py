"""Resampling of the light table's picks (fh_set_light_resampling), the parts that need no GPU: the ABI (symbols, struct, header), the refusals decided before the
context, the facades and rtcamp's flag, and csrc/fh_lights.h compiled for the host (with -fsanitize=address,undefined) into a stand-alone program that is given
emitters and shaded points and must reproduce, bit for bit, the proxies, geometric weights, candidates, choice and ratio of the numpy restatement
(light_resampling_model.py).  Then what the float64 model must satisfy: its exact marginal sums to 1, M = 1 is the table's model, its mean does not depend on M, and
the rule that chose the default M."""
import ctypes as C
import inspect
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from fredholm_amd import native as N

import light_resampling_model as R
import light_resampling_scenes as RS
import light_sampling_model as M
import light_sampling_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINK = ["-L" + os.path.join(ROOT, "fredholm_amd"), "-lfredholm_hip", "-Wl,-rpath," + os.path.join(ROOT, "fredholm_amd"), "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
FH_E_INVALID = -1
f32 = np.float32
BAD_M = (0, -1, 3, 5, 6, 7, 12, 17, 32, 2 ** 31 - 1, -2 ** 31)


def test_symbols_struct_and_header_agree(tmp_path):
    L = N.load_library()
    want = {"fh_set_light_resampling": [C.c_void_p, C.POINTER(N.LightResamplingParamsC)],
            "fh_get_light_resampling": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(N.LightResamplingParamsC)],
            "fh_kat_light_proxies": [C.c_void_p, C.c_void_p],
            "fh_kat_light_resample": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
            "fh_kat_light_usel": [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]}
    for name, sig in want.items():
        assert name in N.EXPORTS
        fn = getattr(L, name)
        assert fn.restype is C.c_int and fn.argtypes == N.SIGNATURES[name] == sig, name
    hdr = " ".join(open(os.path.join(ROOT, "include", "fredholm_hip.h")).read().split())
    hdr_test = " ".join(open(os.path.join(ROOT, "include", "fredholm_hip_test.h")).read().split())
    for decl in ("int fh_set_light_resampling(fh_ctx* ctx, const fh_light_resampling_params* params);", "int fh_get_light_resampling(fh_ctx* ctx, int* on, fh_light_resampling_params* params);",
                 "#define FH_LIGHT_CANDIDATES_DEFAULT %d" % N.LIGHT_CANDIDATES_DEFAULT, "seed_hash ^ 0x%08x" % R.SALT):
        assert decl in hdr, decl
    assert "any pick that depends on the shaded point, " not in hdr and "Not covered: a light hierarchy, product sampling with the BSDF." in hdr
    for decl in ("int fh_kat_light_proxies(fh_ctx* ctx, float* proxies8);",
                 "int fh_kat_light_resample(fh_ctx* ctx, uint32_t n, const float* so3, const float* ns3, const float* u1, const float* u_sel, uint32_t* index, float* ratio);",
                 "int fh_kat_light_usel(uint32_t n, const uint32_t* image_idx, const uint32_t* n_spp, uint32_t dim_area, uint32_t seed_hash, float* u_sel);"):
        assert decl in hdr_test, decl
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fredholm_hip.h"\nint main(void) { printf("%zu %zu %d\\n", sizeof(fh_light_resampling_params), '
                   'offsetof(fh_light_resampling_params, candidates), FH_LIGHT_CANDIDATES_DEFAULT); return 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(N.LightResamplingParamsC), N.LightResamplingParamsC.candidates.offset, N.LIGHT_CANDIDATES_DEFAULT] == [4, 0, N.LIGHT_CANDIDATES_DEFAULT]


def test_the_refusal_is_decided_before_the_context_is_looked_at():
    """with a NULL context: an M outside {1, 2, 4, 8, 16} is refused with its message; good counts and NULL (off) get as far as the context check"""
    L = N.lib()
    for bad in BAD_M:
        assert R.refused(bad)
        assert L.fh_set_light_resampling(None, C.byref(N.LightResamplingParamsC(bad))) == FH_E_INVALID
        assert L.fh_last_error(None).decode() == "fh_set_light_resampling: candidates must be 1, 2, 4, 8 or 16", bad
    L.fh_denoise_history_reset(None)
    marker = L.fh_last_error(None)
    for good in N.LIGHT_CANDIDATES:
        assert not R.refused(good)
        assert L.fh_set_light_resampling(None, C.byref(N.LightResamplingParamsC(good))) == FH_E_INVALID and L.fh_last_error(None) == marker, good
    assert L.fh_set_light_resampling(None, None) == FH_E_INVALID and L.fh_last_error(None) == marker
    on = C.c_int(0)
    assert L.fh_get_light_resampling(None, C.byref(on), None) == FH_E_INVALID
    for hook in ("fh_kat_light_proxies", "fh_kat_light_resample"):
        assert getattr(L, hook)(*[0 if a is C.c_uint32 else None for a in N.SIGNATURES[hook]]) == FH_E_INVALID
    assert L.fh_kat_light_usel(0, None, None, 0, 0, None) == FH_E_INVALID


def test_usel_on_the_host_equals_the_restatement_and_is_uniform():
    """fh_kat_light_usel runs the function the kernels call on the host: bit for bit the restatement's, in [0, 1), multiples of 2^-24, and flat over 16 bins"""
    rng = np.random.default_rng(3)
    n = 1 << 16
    px, spp = rng.integers(0, 1 << 22, n).astype(np.uint32), rng.integers(0, 1 << 16, n).astype(np.uint32)
    for dim, seed in ((0, 0), (5, 0x12345678), (47, 0xFFFFFFFF)):
        got = np.zeros(n, f32)
        assert N.lib().fh_kat_light_usel(n, N.ptr(px), N.ptr(spp), dim, seed, N.ptr(got)) == 0
        want = R.usel(px, spp, dim, seed)
        assert (got.view(np.uint32) == want.view(np.uint32)).all()
        assert (got >= 0).all() and (got < 1).all() and (got * 2.0 ** 24 == np.round(got * 2.0 ** 24)).all()
        counts = np.bincount((got * 16).astype(int), minlength=16)
        assert ((counts - n / 16) ** 2 / (n / 16)).sum() < 60.0  # chi-square, 15 degrees of freedom: 60 is beyond 1e-6


def test_python_facade_has_the_methods_with_the_library_default():
    from fredholm_amd.renderer import Renderer
    assert inspect.signature(Renderer.set_light_resampling).parameters["candidates"].default == N.LIGHT_CANDIDATES_DEFAULT
    assert N.LIGHT_CANDIDATES_DEFAULT in (2, 4, 8, 16) and N.LIGHT_CANDIDATES == R.CANDIDATES
    for name in ("clear_light_resampling", "get_light_resampling"):
        assert callable(getattr(Renderer, name))


# ------------------------------------------------------------------ the C++ facade over stubbed entry points
FACADE = r"""
#include "fredholm/renderer.h"
#include <cstdio>
#include <cstring>
static int g_on = 0;
extern "C" int fh_ctx_create(int, fh_ctx** out) { *out = reinterpret_cast<fh_ctx*>(0x10); return FH_OK; }  // never dereferenced: the entries are the ones below
extern "C" int fh_ctx_create_group(const int*, uint32_t, fh_ctx** out) { *out = reinterpret_cast<fh_ctx*>(0x10); return FH_OK; }
extern "C" int fh_ctx_destroy(fh_ctx*) { return FH_OK; }
extern "C" const char* fh_last_error(fh_ctx*) { return "candidates must be 1, 2, 4, 8 or 16"; }
extern "C" int fh_set_light_sampling(fh_ctx*, const fh_light_sampling_params* p)
{
  g_on = p != nullptr;
  if (p) std::printf("fh_set_light_sampling %g\n", (double)p->uniform_fraction);
  else std::printf("fh_set_light_sampling off\n");
  return FH_OK;
}
extern "C" int fh_get_light_sampling(fh_ctx*, int* on, fh_light_sampling_params*) { *on = g_on; return FH_OK; }
extern "C" int fh_set_light_resampling(fh_ctx*, const fh_light_resampling_params* p)
{
  if (p) std::printf("fh_set_light_resampling %d\n", p->candidates);
  else std::printf("fh_set_light_resampling off\n");
  const int m = p ? p->candidates : 1;
  return m == 1 || m == 2 || m == 4 || m == 8 || m == 16 ? FH_OK : FH_E_INVALID;
}
int main(int argc, char** argv)
{
  const char* what = argc > 1 ? argv[1] : "default";
  try {
    optwl::Context context;
    fredholm::Renderer renderer(context.get_context());
    if (std::strcmp(what, "set") == 0) renderer.set_light_resampling(16);
    if (std::strcmp(what, "on") == 0) renderer.set_light_resampling();
    if (std::strcmp(what, "off") == 0) renderer.clear_light_resampling();
    std::printf("ready\n");
  } catch (const std::exception& e) { std::printf("error %s\n", e.what()); return 3; }
  return 0;
}
"""


@pytest.fixture(scope="module")
def facade(tmp_path_factory):
    d = tmp_path_factory.mktemp("light_resampling_facade")
    (d / "facade.cpp").write_text(FACADE)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(d / "facade.cpp"), *LINK, "-lpthread", "-o", str(d / "facade")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(d / "facade")


def _run(exe, *args, env=None, rc=0):
    e = {k: v for k, v in os.environ.items() if k not in ("FH_LIGHT_SAMPLING", "FH_LIGHT_RESAMPLING", "FH_ENV_SAMPLING", "FH_DEVICES")}
    e.update(env or {})
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=e)
    assert r.returncode == rc, (r.stdout, r.stderr)
    return r.stdout.splitlines()


def test_the_environment_variable_and_the_facade_reach_the_entry_point(facade):
    table = "fh_set_light_sampling %g" % N.LIGHT_UNIFORM_FRACTION_DEFAULT
    default = "fh_set_light_resampling %d" % N.LIGHT_CANDIDATES_DEFAULT
    assert _run(facade) == ["ready"]  # (unset: the switch is not touched)
    assert _run(facade, env={"FH_LIGHT_RESAMPLING": "0"}) == ["ready"]
    assert _run(facade, env={"FH_LIGHT_RESAMPLING": "1"}) == [table, default, "ready"]  # (it implies light sampling at the library's share)
    assert _run(facade, env={"FH_LIGHT_RESAMPLING": "16"}) == [table, "fh_set_light_resampling 16", "ready"]
    assert _run(facade, env={"FH_LIGHT_RESAMPLING": "8", "FH_LIGHT_SAMPLING": "0.25"}) == ["fh_set_light_sampling 0.25", "fh_set_light_resampling 8", "ready"]  # (... or at that variable's)
    assert _run(facade, env={"FH_LIGHT_RESAMPLING": "many"}, rc=3)[0].startswith("error FH_LIGHT_RESAMPLING")
    assert _run(facade, env={"FH_LIGHT_RESAMPLING": "3"}, rc=3)[-1].startswith("error ")  # (the library's refusal is thrown)
    assert _run(facade, "on") == [default, "ready"]  # (the method alone does not touch light sampling)
    assert _run(facade, "set", env={"FH_LIGHT_RESAMPLING": "1"}) == [table, default, "fh_set_light_resampling 16", "ready"]  # (what the application sets afterwards wins)
    assert _run(facade, "off", env={"FH_LIGHT_RESAMPLING": "1"}) == [table, default, "fh_set_light_resampling off", "ready"]


def test_rtcamp_refuses_the_flag_without_light_sampling_and_bad_counts(tmp_path):
    rt = tmp_path / "rtcamp"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "rtcamp.cpp"), *LINK, "-lpthread", "-o", str(rt)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(rt), "--scene", "x.obj", "--light-resampling"], capture_output=True, text=True)
    assert run.returncode == 2 and "--light-resampling goes with --light-sampling" in run.stderr, run.stderr
    for bad in ("0", "3", "17", "4x"):
        run = subprocess.run([str(rt), "--scene", "x.obj", "--light-sampling", "--light-resampling", bad], capture_output=True, text=True)
        assert run.returncode == 2 and "--light-resampling takes 1, 2, 4, 8 or 16" in run.stderr, (bad, run.stderr)
    run = subprocess.run([str(rt)], capture_output=True, text=True)
    assert run.returncode == 2 and "--light-resampling [M]" in run.stderr


# ------------------------------------------------------------------ fh_lights.h on the host against the restatement
PROGRAM = r"""
// reads: U, n; n x (area, r, g, b); n x 18 floats (p0, p1, p2, n0, n1, n2); M, m; m x (so, ns, u1, u_sel).
// writes: the proxies (8 floats each); per point: the M candidates, their G, then (chosen index, ratio, S)
#include <cstdio>
#include <vector>
#include "fh_lights.h"
using namespace fh;
int main(int argc, char** argv)
{
  if (argc != 3) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) return 2;
  float U = 0.0f;
  uint32_t n = 0, m = 0;
  int M = 0;
  if (std::fread(&U, 4, 1, in) != 1 || std::fread(&n, 4, 1, in) != 1 || n == 0) return 2;
  std::vector<float> rec((size_t)n * 4), geo((size_t)n * 18), w(n), cdf((size_t)n + 1), p(n);
  std::vector<uint32_t> q(n);
  if (std::fread(rec.data(), 4, rec.size(), in) != rec.size() || std::fread(geo.data(), 4, geo.size(), in) != geo.size()) return 2;
  for (uint32_t k = 0; k < n; ++k) w[k] = light_weight(rec[4 * k], rec[4 * k + 1], rec[4 * k + 2], rec[4 * k + 3]);
  uint64_t total = 0;
  light_build_host(w.data(), n, U, q.data(), cdf.data(), p.data(), &total);
  std::vector<LightProxy> prox(n);
  for (uint32_t k = 0; k < n; ++k) {
    const float* g = &geo[18 * (size_t)k];
    prox[k] = light_proxy(g, g + 3, g + 6, g + 9, g + 12, g + 15, rec[4 * k]);
  }
  std::fwrite(prox.data(), sizeof(LightProxy), n, out);
  if (std::fread(&M, 4, 1, in) != 1 || std::fread(&m, 4, 1, in) != 1) return 2;
  const fh_light_resampling_params prm = {M};
  if (const char* why = light_resampling_refusal(&prm)) { std::fprintf(stderr, "%s\n", why); return 3; }
  const LightTable t = {cdf.data(), nullptr, U, prox.data(), (uint32_t)M};
  for (uint32_t s = 0; s < m; ++s) {
    float a[8];
    if (std::fread(a, 4, 8, in) != 8) return 2;
    const float v = light_candidate_v(a[6], (uint32_t)M);
    std::vector<uint32_t> idx(M);
    std::vector<float> g(M);
    for (int k = 0; k < M; ++k) {
      idx[k] = light_pick(t.cdf, n, U, light_candidate_u((uint32_t)k, v, (uint32_t)M));
      g[k] = light_geom(prox[idx[k]], a[0], a[1], a[2], a[3], a[4], a[5]);
    }
    std::fwrite(idx.data(), 4, M, out); std::fwrite(g.data(), 4, M, out);
    const LightChoice ch = light_resample(t, n, a[6], a[7], a[0], a[1], a[2], a[3], a[4], a[5]);
    std::fwrite(&ch.index, 4, 1, out); std::fwrite(&ch.ratio, 4, 1, out); std::fwrite(&ch.sum, 4, 1, out);
  }
  std::fclose(in);
  std::fclose(out);
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """csrc/fh_lights.h compiled for the host, with the address and undefined-behaviour sanitizers, into a stand-alone program"""
    d = tmp_path_factory.mktemp("light_resampling_host")
    (d / "resample.cpp").write_text(PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-I" + os.path.join(ROOT, "fredholm_amd", "csrc"), str(d / "resample.cpp"), "-o", str(d / "resample")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(U, rec, corners, normals, m_cand, points, rc=0):
        """rec [n, 4] (area, r, g, b); corners, normals [n, 3, 3]; points [m, 8] (so, ns, u1, u_sel)"""
        n = len(rec)
        geo = np.concatenate([np.asarray(corners, f32).reshape(n, 9), np.asarray(normals, f32).reshape(n, 9)], axis=1)
        blob = (struct.pack("<fI", U, n) + np.ascontiguousarray(rec, f32).tobytes() + np.ascontiguousarray(geo, f32).tobytes() + struct.pack("<iI", m_cand, len(points))
                + np.ascontiguousarray(points, f32).tobytes())
        (d / "in.bin").write_bytes(blob)
        r = subprocess.run([str(d / "resample"), str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
        assert r.returncode == rc, r.stderr
        if rc:
            return r.stderr
        raw = np.frombuffer((d / "out.bin").read_bytes(), dtype=np.uint32)
        assert raw.size == 8 * n + len(points) * (2 * m_cand + 3)
        per = raw[8 * n:].reshape(len(points), 2 * m_cand + 3)
        return dict(proxies=raw[:8 * n].reshape(n, 8), cand=per[:, :m_cand], g=per[:, m_cand:2 * m_cand], index=per[:, -3], ratio=per[:, -2], sum=per[:, -1])
    return run


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def shaded_points(prox, m_cand, rng, n_random=300):
    """[k, 8] (so, ns, u1, u_sel): random points under and over the emitters with normals up, down and anywhere; so exactly at two centroids; every combination of
    u1 in {0, the last float below 1, the stratum edges k / M and the floats just below them} with u_sel in {0, the last float below 1}"""
    below = lambda x: np.nextafter(f32(x), f32(-1))
    so = np.stack([rng.uniform(-9.0, 1.0, n_random), rng.uniform(0.0, 6.5, n_random), rng.uniform(-1.0, 5.0, n_random)], axis=1).astype(f32)
    ns = rng.normal(size=(n_random, 3))
    ns = (ns / np.linalg.norm(ns, axis=1, keepdims=True)).astype(f32)
    ns[0::3] = (0.0, 1.0, 0.0)
    ns[1::3] = (0.0, -1.0, 0.0)   # facing away from emitters overhead
    so[:2] = prox[[0, len(prox) // 2], 0:3]   # exactly at a centroid: r2 = 0, d = NaN, both cosines fall to their floors
    u1 = rng.random(n_random).astype(f32)
    us = rng.random(n_random).astype(f32)
    edges = [f32(0.0), below(1.0)]
    for k in range(1, m_cand):
        edges += [f32(k) / f32(m_cand), below(f32(k) / f32(m_cand))]
    extra = [(so[3 + i % 7], ns[3 + i % 5], e, s) for i, e in enumerate(edges) for s in (f32(0.0), below(1.0))]
    pts = np.concatenate([so, ns, u1[:, None], us[:, None]], axis=1)
    return np.concatenate([pts, np.array([np.concatenate([a, b, [e, s]]) for a, b, e, s in extra], f32)]).astype(f32)


def strip_inputs(n, U):
    sc, corners, mat_of, colours = S.strip(n, seed=n, zero_area_at=100 if n == 257 else None)
    area = M.area(corners[:, 0], corners[:, 1], corners[:, 2])
    normals = np.tile(np.array([0.0, -1.0, 0.0], f32), (n, 3, 1))  # (a zero-area face has no normal of its own: the strip's)
    rec = np.concatenate([area[:, None], colours[mat_of]], axis=1).astype(f32)
    return rec, corners, normals, M.Table(M.weight(area, colours[mat_of]), U)


@pytest.mark.parametrize("n", (1, 2, 257))
def test_the_header_on_the_host_equals_the_restatement_bit_for_bit(program, n):
    """strips of 1, 2 and 257 emitters (the last with a zero-area emitter, one emitter's normals summing to zero and one's not finite), every M"""
    U = 0.125
    rec, corners, normals, table = strip_inputs(n, U)
    if n == 257:
        normals[7] = [(1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 0.0)]
        normals[9, 1] = (np.inf, 0.0, 0.0)
        assert rec[100, 0] == 0.0
    prox = R.proxies(corners, normals, rec[:, 0])
    if n == 257:
        assert (prox[7, 4:7] == 0).all() and (prox[9, 4:7] == 0).all() and prox[100, 3] == 0
    rng = np.random.default_rng(n)
    for m_cand in R.CANDIDATES:
        pts = shaded_points(prox, m_cand, rng)
        if n == 257:
            pts[2, 0:3] = prox[100, 0:3]   # at the centroid of the zero-area emitter: G = (1/256) / 0, clamped to 1e30 when it is a candidate
        got = program(U, rec, corners, normals, m_cand, pts)
        assert (got["proxies"] == _bits(prox)).all()
        cand, g, idx, ratio, s = R.resample(table, prox, pts[:, 0:3], pts[:, 3:6], pts[:, 6], pts[:, 7], m_cand)
        assert (got["cand"] == cand).all() and (got["g"] == _bits(g)).all(), m_cand
        assert (got["index"] == idx).all() and (got["ratio"] == _bits(ratio)).all() and (got["sum"] == _bits(s)).all(), m_cand
        assert np.isfinite(g).all() and (g >= R.G_MIN).all() and (g <= R.G_MAX).all() and (ratio > 0).all() and np.isfinite(ratio).all()
        if m_cand == 1:
            assert (ratio == 1).all() and (idx == table.pick(pts[:, 6])[0]).all()
        # u_sel = 0 chooses the first candidate, the last float below 1 one whose running sum reaches S
        first = pts[:, 7] == 0
        assert first.any() and (idx[first] == cand[first, 0]).all()


def test_the_program_refuses_what_the_library_refuses(program):
    rec, corners, normals, _ = strip_inputs(2, 0.125)
    for bad in BAD_M:
        assert "candidates must be 1, 2, 4, 8 or 16" in program(0.125, rec, corners, normals, bad, np.zeros((0, 8), f32), rc=3)


# ------------------------------------------------------------------ the float64 model
def test_the_exact_marginal_sums_to_one_and_follows_the_restatement():
    """at three points of the lamp-aside scene, for every M: the marginal sums to 1, M = 1 gives the table's pick probabilities, and 2^17 choices of the float32
    restatement follow it (chi-square)"""
    import expectation_model as E
    quads = S.model_quads(RS.ASIDE)
    table, prox = S.model_table(N.LIGHT_UNIFORM_FRACTION_DEFAULT, quads), RS.model_proxies(quads)
    rng = np.random.default_rng(5)
    for x in (np.array([-40.0, 0.0, 30.0]), np.array([-1.75, 0.0, -3.0]), S.MODEL_X):
        g = R.geom64(prox, x, np.array(RS.UP))
        for m in R.CANDIDATES:
            q = R.marginal(table, g, m)
            assert abs(q.sum() - 1.0) < 1e-12 and (q > 0).all()
            if m == 1:
                assert np.allclose(q, table.p.astype(np.float64), rtol=0, atol=2e-7)
            k = 1 << 17
            so, ns = np.tile(x.astype(f32), (k, 1)), np.tile(np.array(RS.UP, f32), (k, 1))
            idx = R.resample(table, prox, so, ns, rng.random(k).astype(f32), rng.random(k).astype(f32), m)[2]
            stat, dof = E.chi2_pooled(np.bincount(idx, minlength=table.n), q * k)
            assert E.chi2_sf(stat, dof) > 1e-6, (x, m, stat, dof)


def test_one_candidate_is_the_tables_model_and_the_mean_does_not_depend_on_m():
    """M = 1 reproduces light_sampling_model.lambert_floor_moments to rounding (the exact marginal of the float32 CDF against the rounded pick probabilities); for
    every M the mean is Lambert's polygon formula; the clamp binds nowhere in the quadrature of either model scene"""
    for aside in (0.0, RS.ASIDE):
        quads = S.model_quads(aside)
        tris, les = S.model_lights(quads)
        table, prox = S.model_table(N.LIGHT_UNIFORM_FRACTION_DEFAULT, quads), RS.model_proxies(quads)
        want = M.lambert_polygon(S.MODEL_X, RS.UP, S.MODEL_RHO, tris, les)
        ma1, mb1 = M.lambert_floor_moments(S.MODEL_X, RS.UP, S.MODEL_RHO, tris, les, table.p.astype(np.float64), 4)
        info = {}
        for m in R.CANDIDATES:
            ma, mb = R.floor_moments(S.MODEL_X, RS.UP, S.MODEL_RHO, tris, les, table, prox, m, 4, info=info)
            assert np.allclose(ma[0] + mb[0], want, rtol=1e-3), (aside, m)
            assert np.allclose(ma[0] + mb[0], ma1[0] + mb1[0], rtol=1e-6), (aside, m)
            if m == 1:
                assert np.allclose(ma, ma1, rtol=1e-5) and np.allclose(mb, mb1, rtol=0, atol=0)
        assert info["clamp_max"] < 1.0 and info["clamped_probability"] == 0.0


def test_the_default_follows_its_rule_and_the_record_says_where_it_stands():
    """profiles/light_resampling_model.json: the smallest M among 2, 4, 8, 16 whose predicted variance on the lamp-aside scene is within 1.25 x the best of the four;
    resampling beats the table alone there, and the record says for which M, if any, it ends below the uniform pick"""
    rec = json.load(open(os.path.join(ROOT, "profiles", "light_resampling_model.json")))
    quads = S.model_quads(RS.ASIDE)
    var = {m: RS.model_prediction(m, quads=quads)["variance"] for m in (2, 4, 8, 16)}
    assert RS.default_candidates(var) == N.LIGHT_CANDIDATES_DEFAULT == rec["default_candidates"]
    base = S.model_prediction(N.LIGHT_UNIFORM_FRACTION_DEFAULT, quads=quads)
    for m in (2, 4, 8, 16):
        assert np.isclose(var[m], rec["lamp_aside"]["variance_resampled"][str(m)], rtol=1e-9)
        assert var[m] < base["variance_on"]
        assert rec["lamp_aside_below_uniform"][str(m)] == bool(var[m] < base["variance_off"])
    assert np.isclose(base["variance_on"] / base["variance_off"], rec["lamp_aside"]["table_to_uniform"], rtol=1e-9)
