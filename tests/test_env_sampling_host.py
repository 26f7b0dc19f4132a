"""Importance sampling of the environment, the parts that need no GPU: the ABI (symbols, struct, header), the refusals decided before the context, the facades and
rtcamp's flags, and csrc/fh_envmap.h compiled for the host (with -fsanitize=address,undefined) into a stand-alone program that is given the point-sampled radiances
and must reproduce, bit for bit, the integer weights, CDFs, drawn directions and densities of the numpy restatement (env_sampling_model.py).  Then what the
restatement itself must satisfy: no cell of probability zero, the density's integral, and the share of draws that map back to a neighbouring cell."""
import ctypes as C
import inspect
import os
import struct
import subprocess

import numpy as np
import pytest

from fredholm_amd import native as N

import env_sampling_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINK = ["-L" + os.path.join(ROOT, "fredholm_amd"), "-lfredholm_hip", "-Wl,-rpath," + os.path.join(ROOT, "fredholm_amd"), "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
FH_E_INVALID = -1
f32 = np.float32


def test_symbols_struct_and_header_agree(tmp_path):
    L = N.load_library()
    want = {"fh_set_env_sampling": [C.c_void_p, C.POINTER(N.EnvSamplingParamsC)],
            "fh_get_env_sampling": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(N.EnvSamplingParamsC)],
            "fh_kat_env_table": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
            "fh_kat_env_sample": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
            "fh_kat_env_pdf": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
            "fh_kat_env_radiance": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]}
    for name, sig in want.items():
        assert name in N.EXPORTS
        fn = getattr(L, name)
        assert fn.restype is C.c_int and fn.argtypes == N.SIGNATURES[name] == sig, name
    hdr = " ".join(open(os.path.join(ROOT, "include", "fredholm_hip.h")).read().split())
    hdr_test = " ".join(open(os.path.join(ROOT, "include", "fredholm_hip_test.h")).read().split())
    for decl in ("int fh_set_env_sampling(fh_ctx* ctx, const fh_env_sampling_params* params);", "int fh_get_env_sampling(fh_ctx* ctx, int* on, fh_env_sampling_params* params);",
                 "#define FH_ENV_COSINE_FRACTION_DEFAULT %sf" % repr(N.ENV_COSINE_FRACTION_DEFAULT)):
        assert decl in hdr, decl
    for decl in ("int fh_kat_env_table(fh_ctx* ctx, uint32_t* weights, float* cdf_row, float* cdf_marginal, float* cell_p);",
                 "int fh_kat_env_sample(fh_ctx* ctx, uint32_t n, const float* u2, const float* normal3, float* dir3, float* pdf, uint32_t* cell);",
                 "int fh_kat_env_pdf(fh_ctx* ctx, uint32_t n, const float* dirs3, const float* normal3, float* pdf, uint32_t* cell);",
                 "int fh_kat_env_radiance(fh_ctx* ctx, uint32_t n, const float* dirs3, float* out3);"):
        assert decl in hdr_test, decl
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fredholm_hip.h"\nint main(void) { printf("%zu %zu %.9g\\n", sizeof(fh_env_sampling_params), '
                   'offsetof(fh_env_sampling_params, cosine_fraction), (double)FH_ENV_COSINE_FRACTION_DEFAULT); return 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(got[0]), int(got[1])] == [C.sizeof(N.EnvSamplingParamsC), N.EnvSamplingParamsC.cosine_fraction.offset] == [4, 0]
    assert float(got[2]) == float(f32(N.ENV_COSINE_FRACTION_DEFAULT))
    # the table's shape as the header, the kernels' header and the restatement state it
    env_h = open(os.path.join(ROOT, "fredholm_amd", "csrc", "fh_envmap.h")).read()
    assert "kEnvW = 512, kEnvH = 256" in env_h and (M.W, M.H) == (512, 256) and "512 x 256 cells" in hdr


def test_the_refusal_is_decided_before_the_context_is_looked_at():
    """with a NULL context: a fraction outside [0, 1) is refused with its message; good fractions and NULL (off) get as far as the context check"""
    L = N.lib()
    for bad in (1.0, -0.01, 1.5, float("nan"), float("inf"), -float("inf")):
        assert L.fh_set_env_sampling(None, C.byref(N.EnvSamplingParamsC(bad))) == FH_E_INVALID
        assert L.fh_last_error(None).decode() == "fh_set_env_sampling: cosine_fraction must be in [0, 1)", bad
    L.fh_denoise_history_reset(None)
    marker = L.fh_last_error(None)
    for good in (0.0, 0.125, 0.25, 0.5, float(np.nextafter(f32(1), f32(0)))):
        assert L.fh_set_env_sampling(None, C.byref(N.EnvSamplingParamsC(good))) == FH_E_INVALID and L.fh_last_error(None) == marker, good
    assert L.fh_set_env_sampling(None, None) == FH_E_INVALID and L.fh_last_error(None) == marker
    on = C.c_int(0)
    assert L.fh_get_env_sampling(None, C.byref(on), None) == FH_E_INVALID
    for hook in ("fh_kat_env_table", "fh_kat_env_sample", "fh_kat_env_pdf", "fh_kat_env_radiance"):
        assert getattr(L, hook)(*[0 if a is C.c_uint32 else None for a in N.SIGNATURES[hook]]) == FH_E_INVALID


def test_python_facade_has_the_methods_with_the_library_default():
    from fredholm_amd.renderer import Renderer
    assert inspect.signature(Renderer.set_env_sampling).parameters["cosine_fraction"].default == N.ENV_COSINE_FRACTION_DEFAULT
    assert N.ENV_COSINE_FRACTION_DEFAULT in (0.125, 0.25, 0.5)
    for name in ("clear_env_sampling", "get_env_sampling"):
        assert callable(getattr(Renderer, name))


# ------------------------------------------------------------------ the C++ facade over stubbed entry points
FACADE = r"""
#include "fredholm/renderer.h"
#include <cstdio>
#include <cstring>
extern "C" int fh_ctx_create(int, fh_ctx** out) { *out = reinterpret_cast<fh_ctx*>(0x10); return FH_OK; }  // never dereferenced: the entries are the ones below
extern "C" int fh_ctx_create_group(const int*, uint32_t, fh_ctx** out) { *out = reinterpret_cast<fh_ctx*>(0x10); return FH_OK; }
extern "C" int fh_ctx_destroy(fh_ctx*) { return FH_OK; }
extern "C" const char* fh_last_error(fh_ctx*) { return "cosine_fraction must be in [0, 1)"; }
extern "C" int fh_set_env_sampling(fh_ctx*, const fh_env_sampling_params* p)
{
  if (p) std::printf("fh_set_env_sampling %g\n", (double)p->cosine_fraction);
  else std::printf("fh_set_env_sampling off\n");
  return p && !(p->cosine_fraction >= 0.0f && p->cosine_fraction < 1.0f) ? FH_E_INVALID : FH_OK;
}
int main(int argc, char** argv)
{
  const char* what = argc > 1 ? argv[1] : "default";
  try {
    optwl::Context context;
    fredholm::Renderer renderer(context.get_context());
    if (std::strcmp(what, "set") == 0) renderer.set_env_sampling(0.5f);
    if (std::strcmp(what, "on") == 0) renderer.set_env_sampling();
    if (std::strcmp(what, "off") == 0) renderer.clear_env_sampling();
    std::printf("ready\n");
  } catch (const std::exception& e) { std::printf("error %s\n", e.what()); return 3; }
  return 0;
}
"""


@pytest.fixture(scope="module")
def facade(tmp_path_factory):
    d = tmp_path_factory.mktemp("env_sampling_facade")
    (d / "facade.cpp").write_text(FACADE)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(d / "facade.cpp"), *LINK, "-lpthread", "-o", str(d / "facade")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(d / "facade")


def _run(exe, *args, env=None, rc=0):
    e = {k: v for k, v in os.environ.items() if k not in ("FH_ENV_SAMPLING", "FH_DEVICES")}
    e.update(env or {})
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=e)
    assert r.returncode == rc, (r.stdout, r.stderr)
    return r.stdout.splitlines()


def test_the_environment_variable_and_the_facade_reach_the_entry_point(facade):
    default = "fh_set_env_sampling %g" % N.ENV_COSINE_FRACTION_DEFAULT
    assert _run(facade) == ["ready"]  # (unset: the switch is not touched)
    assert _run(facade, env={"FH_ENV_SAMPLING": "0"}) == ["ready"]
    assert _run(facade, env={"FH_ENV_SAMPLING": "1"}) == [default, "ready"]
    assert _run(facade, env={"FH_ENV_SAMPLING": "0.125"}) == ["fh_set_env_sampling 0.125", "ready"]
    assert _run(facade, env={"FH_ENV_SAMPLING": "sunny"}, rc=3)[0].startswith("error FH_ENV_SAMPLING")
    assert _run(facade, env={"FH_ENV_SAMPLING": "1.5"}, rc=3)[-1].startswith("error ")  # (the library's refusal is thrown)
    assert _run(facade, "on") == [default, "ready"]
    assert _run(facade, "set", env={"FH_ENV_SAMPLING": "1"}) == [default, "fh_set_env_sampling 0.5", "ready"]  # (what the application sets afterwards wins)
    assert _run(facade, "off", env={"FH_ENV_SAMPLING": "1"}) == [default, "fh_set_env_sampling off", "ready"]


def test_rtcamp_refuses_the_fraction_without_the_switch_and_bad_values(tmp_path):
    rt = tmp_path / "rtcamp"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "rtcamp.cpp"), *LINK, "-lpthread", "-o", str(rt)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(rt), "--scene", "x.obj", "--env-cosine-fraction", "0.25"], capture_output=True, text=True)
    assert run.returncode == 2 and "--env-cosine-fraction goes with --env-sampling" in run.stderr, run.stderr
    for bad in ("1", "-0.1", "nan"):
        run = subprocess.run([str(rt), "--scene", "x.obj", "--env-sampling", "--env-cosine-fraction", bad], capture_output=True, text=True)
        assert run.returncode == 2 and "--env-cosine-fraction must be in [0, 1)" in run.stderr, (bad, run.stderr)
    run = subprocess.run([str(rt), "--scene", "x.obj", "--env-sampling", "--env-cosine-fraction"], capture_output=True, text=True)
    assert run.returncode == 2 and "missing value" in run.stderr
    run = subprocess.run([str(rt)], capture_output=True, text=True)
    assert run.returncode == 2 and "--env-sampling" in run.stderr and "--env-cosine-fraction" in run.stderr


# ------------------------------------------------------------------ fh_envmap.h on the host against the restatement
ENVMAP = r"""
// reads: k (0: a constant background, no radiances follow), then for k > 0 the radiances [256][k (b)][512][k (a)][3]; beta; n and n x (ux, uy, normal);
// m and m x (direction, normal).  writes: q, cdf_row, cdf_m, cell_p; per draw (cosine branch?, rescaled ux, direction, density, cell); per evaluation (density, cell)
#include <cstdio>
#include <vector>
#include "fh_envmap.h"
using namespace fh;
int main(int argc, char** argv)
{
  if (argc != 3) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) return 2;
  uint32_t kk = 0;
  if (std::fread(&kk, 4, 1, in) != 1 || kk > 16) return 2;
  const int k = kk ? (int)kk : 2;
  std::vector<float> rad;
  if (kk) { rad.resize((size_t)kEnvCells * k * k * 3); if (std::fread(rad.data(), 4, rad.size(), in) != rad.size()) return 2; }
  std::vector<float> w(kEnvCells);
  for (int j = 0; j < kEnvH; ++j)
    for (int i = 0; i < kEnvW; ++i) {
      float sum = 0.0f;
      for (int b = 0; b < k; ++b)
        for (int a = 0; a < k; ++a) {
          float u, v, st;
          env_subsample_uv(i, j, a, b, k, &u, &v);
          env_direction(u, v, &st);
          const float* c = kk ? &rad[((((size_t)j * k + b) * kEnvW + i) * k + a) * 3] : nullptr;
          sum += env_sample_weight(c ? env_lum(c[0], c[1], c[2]) : 1.0f, st);
        }
      w[j * kEnvW + i] = env_cell_mean(sum, k);
    }
  std::vector<uint32_t> q(kEnvCells);
  std::vector<float> cdf_row((size_t)kEnvH * kEnvRowCdf), cdf_m(kEnvH + 1), cell_p(kEnvCells);
  env_build_host(w.data(), q.data(), cdf_row.data(), cdf_m.data(), cell_p.data());
  std::fwrite(q.data(), 4, q.size(), out); std::fwrite(cdf_row.data(), 4, cdf_row.size(), out);
  std::fwrite(cdf_m.data(), 4, cdf_m.size(), out); std::fwrite(cell_p.data(), 4, cell_p.size(), out);
  EnvTable t{cdf_row.data(), cdf_m.data(), cell_p.data(), 0.0f};
  uint32_t n = 0, m = 0;
  if (std::fread(&t.beta, 4, 1, in) != 1 || std::fread(&n, 4, 1, in) != 1) return 2;
  const fh_env_sampling_params p = {t.beta};
  if (const char* why = env_sampling_refusal(&p)) { std::fprintf(stderr, "%s\n", why); return 3; }
  for (uint32_t s = 0; s < n; ++s) {
    float x[5];
    if (std::fread(x, 4, 5, in) != 5) return 2;
    float ux = x[0], rec[6] = {0, 0, 0, 0, 0, 0};
    uint32_t cell = 0;
    const bool cosine = env_select_cosine(t.beta, &ux);
    rec[0] = cosine ? 1.0f : 0.0f; rec[1] = ux;
    if (!cosine) { const EnvDir d = env_sample_table(t, ux, x[1], EnvDir{x[2], x[3], x[4]}, &rec[5], &cell); rec[2] = d.x; rec[3] = d.y; rec[4] = d.z; }
    std::fwrite(rec, 4, 6, out); std::fwrite(&cell, 4, 1, out);
  }
  if (std::fread(&m, 4, 1, in) != 1) return 2;
  for (uint32_t s = 0; s < m; ++s) {
    float x[6];
    if (std::fread(x, 4, 6, in) != 6) return 2;
    uint32_t cell = 0;
    const float pdf = env_pdf(t, EnvDir{x[0], x[1], x[2]}, EnvDir{x[3], x[4], x[5]}, &cell);
    std::fwrite(&pdf, 4, 1, out); std::fwrite(&cell, 4, 1, out);
  }
  std::fclose(in);
  std::fclose(out);
  return 0;
}
"""


@pytest.fixture(scope="module")
def envmap(tmp_path_factory):
    """csrc/fh_envmap.h compiled for the host, with the address and undefined-behaviour sanitizers, into a stand-alone program"""
    d = tmp_path_factory.mktemp("envmap_host")
    (d / "envmap.cpp").write_text(ENVMAP)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-I" + os.path.join(ROOT, "fredholm_amd", "csrc"), str(d / "envmap.cpp"), "-o", str(d / "envmap")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(rad, beta, draws, evals):
        """rad: [256, k, 512, k, 3] or None (constant); draws [n, 5]; evals [m, 6]"""
        k = 0 if rad is None else rad.shape[1]
        blob = struct.pack("<I", k) + (b"" if rad is None else np.ascontiguousarray(rad, f32).tobytes())
        blob += struct.pack("<fI", beta, len(draws)) + np.ascontiguousarray(draws, f32).tobytes() + struct.pack("<I", len(evals)) + np.ascontiguousarray(evals, f32).tobytes()
        (d / "in.bin").write_bytes(blob)
        r = subprocess.run([str(d / "envmap"), str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        raw = np.frombuffer((d / "out.bin").read_bytes(), dtype=np.uint32)
        sizes = [M.CELLS, M.H * (M.W + 1), M.H + 1, M.CELLS, 7 * len(draws), 2 * len(evals)]
        assert raw.size == sum(sizes)
        parts = np.split(raw, np.cumsum(sizes)[:-1])
        return dict(q=parts[0].reshape(M.H, M.W), cdf_row=parts[1].reshape(M.H, M.W + 1), cdf_m=parts[2], cell_p=parts[3].reshape(M.H, M.W),
                    draws=parts[4].reshape(-1, 7), evals=parts[5].reshape(-1, 2))
    return run


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _normals(rng, n):
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v[: n // 4] = [0.0, 1.0, 0.0]
    return v.astype(f32)


def _check_against_restatement(envmap, oracle, env, beta, seed):
    rng = np.random.default_rng(seed)
    k = M.subsamples(env[1].shape[1]) if env[0] == "ibl" else 2
    rad = None
    if env[0] != "constant":
        d, _ = M.subsample_dirs(k, oracle)
        rad = M.radiance(env, d, oracle)
    t = M.Table(M.weights_of(env, oracle))
    n = 20000
    u = rng.random((n, 2)).astype(f32)
    u[:8, 0] = [0.0, beta, np.nextafter(f32(beta), f32(0)), np.nextafter(f32(1), f32(0)), 0.5, 0.5, 0.999, 0.75]
    u[:8, 1] = [0.0, 0.0, 0.5, np.nextafter(f32(1), f32(0)), 0.0, np.nextafter(f32(1), f32(0)), 0.999, 0.25]
    nrm = _normals(rng, n)
    dirs = _normals(rng, n)
    dirs[:6] = [[0, 1, 0], [0, -1, 0], [1, 0, 0], [-1, 0, -0.0], [0, 0, 1], [1e-8, 1, 0]]
    got = envmap(rad, beta, np.concatenate([u, nrm], axis=1), np.concatenate([dirs, nrm], axis=1))
    assert (got["q"] == t.q.astype(np.uint32)).all()
    assert (got["cdf_row"] == _bits(t.cdf_row)).all() and (got["cdf_m"] == _bits(t.cdf_m)).all() and (got["cell_p"] == _bits(t.cell_p)).all()
    ds, ps, cs, cosine = M.sample(t, beta, u, nrm, oracle)
    assert (got["draws"][:, 0].view(f32) == cosine.astype(f32)).all()
    tb = ~cosine
    assert tb.sum() > n // 4
    assert (got["draws"][tb, 2:5] == _bits(ds[tb])).all() and (got["draws"][tb, 5] == _bits(ps[tb])).all() and (got["draws"][tb, 6] == cs[tb].astype(np.uint32)).all()
    pe, ce = M.pdf(t, beta, dirs, nrm, oracle)
    assert (got["evals"][:, 0] == _bits(pe)).all() and (got["evals"][:, 1] == ce.astype(np.uint32)).all()
    # the sampler's report and the evaluator's value are the same bits wherever the direction maps back to the drawn cell
    back_p, back_c = M.pdf(t, beta, ds, nrm, oracle)
    same = back_c == cs
    assert (_bits(back_p[same]) == _bits(ps[same])).all()
    return t


@pytest.mark.parametrize("beta", [0.25, 0.0])
def test_the_header_on_the_host_equals_the_restatement_on_the_sun_image(envmap, oracle, beta):
    t = _check_against_restatement(envmap, oracle, ("ibl", M.sun_image()), beta, 11)
    assert t.q.max() == 1 << 20 and t.q.min() >= 1


def test_the_header_on_the_host_equals_the_restatement_on_a_constant_and_on_the_dome(envmap, oracle):
    t = _check_against_restatement(envmap, oracle, ("constant",), 0.5, 12)
    # every weight is sin theta: rows mirror about the equator and every row is flat
    assert (t.q == t.q[:, :1]).all() and t.q[:, 0].max() == 1 << 20 and t.q[:, 0].argmax() in (127, 128)
    want = np.sin((np.arange(M.H) + 0.5) * np.pi / M.H) * np.cos(0.25 * np.pi / M.H)  # the mean of sin over the two sub-samples of a row
    assert np.abs(t.q[:, 0].astype(np.float64) / (1 << 20) - want / want.max()).max() < 4e-6  # (a few fp32 roundings and the floor of 2^-20)
    sun = np.array([0.3, 0.8, 0.52], f32)
    sun /= np.linalg.norm(sun)
    _check_against_restatement(envmap, oracle, ("hosek", oracle.hosek_cook(3.0, 0.3, sun), sun), 0.125, 13)


def test_the_header_on_the_host_equals_the_restatement_with_more_sub_samples(envmap, oracle):
    """K = clamp(ceil(width / 512), 2, 16): 1024 texels across still give 2, 1100 give 3"""
    assert [M.subsamples(w) for w in (0, 1, 512, 1024, 1025, 1536, 8192, 100000)] == [2, 2, 2, 2, 3, 3, 16, 16]
    img = M.sun_image(1100, 8, patch=1, elevation_deg=45.0)
    _check_against_restatement(envmap, oracle, ("ibl", img), 0.25, 14)


def test_no_cell_has_probability_zero(envmap, oracle):
    """A black image, a one-texel image and NaN / infinite texels: every cell keeps an integer weight >= 1 and a positive probability.  Black: all weights 1 (uniform in
    (phi, theta)); one texel: the constant's sin theta profile to the rounding of the quotient; NaN and infinite texel components count as 0, so the cells they reach keep the weight 1"""
    black = np.zeros((32, 64, 4), f32)
    t = M.Table(M.weights_of(("ibl", black), oracle))
    assert (t.q == 1).all() and t.total == M.CELLS and (t.cell_p > 0).all()
    one = np.full((1, 1, 4), 0.7, f32)
    t1, tc = M.Table(M.weights_of(("ibl", one), oracle)), M.Table(M.weights_of(("constant",), oracle))
    assert np.abs(t1.q.astype(np.int64) - tc.q.astype(np.int64)).max() <= 2 and t1.q.min() >= 1 and (t1.cell_p > 0).all()  # (0.7 s / (0.7 s_max) and s / s_max round apart)
    bad = M.sun_image()
    bad[3, 5, 0], bad[3, 6, 1], bad[20, 40, :3], bad[10, 10, 2] = np.nan, np.inf, -np.inf, -5.0
    d, st = M.subsample_dirs(2, oracle)
    rad = M.radiance(("ibl", bad), d, oracle)
    assert not np.isfinite(rad).all()
    tb = M.Table(M.cell_means(M.lum(rad), st))
    assert tb.q.min() >= 1 and tb.q.max() == 1 << 20 and (tb.cell_p > 0).all() and np.isfinite(tb.cdf_row).all() and np.isfinite(tb.cdf_m).all()
    got = envmap(rad, 0.25, np.zeros((0, 5), f32), np.zeros((0, 6), f32))
    assert (got["q"] == tb.q.astype(np.uint32)).all() and (got["cell_p"] == _bits(tb.cell_p)).all()
    for t in (t, t1, tb):
        assert (np.diff(t.cdf_row.astype(np.float64), axis=1) >= 0).all() and (np.diff(t.cdf_m.astype(np.float64)) >= 0).all()


def test_the_density_integrates_to_one(oracle):
    """The table term: integral over a cell of P_cell * W * H / (2 pi^2 sin theta) d omega = P_cell * W * H / (2 pi^2) * (2 pi / W) * (pi / H) = P_cell exactly, so the term
    integrates to sum(q) / T, which is 1 in integer arithmetic.  The whole mixture by Gauss-Legendre quadrature on the cell boundaries in float64: with the normal
    along +y the horizon is a row boundary and the rule is exact to rounding (1e-9); for a tilted normal the cosine term's kink crosses cells, where a 3-point rule is
    off by at most the cell's solid angle times the kink's jump in slope times the cell size, ~ 2 pi * (pi / 256) * (pi / 256) / pi summed along the horizon < 1e-3"""
    t = M.Table(M.weights_of(("ibl", M.sun_image()), oracle))
    assert int(t.q.sum()) == t.total and int(t.row_sum.sum()) == t.total and (t.q.sum(axis=1) == t.row_sum).all()
    x, wx = np.polynomial.legendre.leggauss(3)
    th = (np.arange(M.H)[:, None] + 0.5 * (x[None, :] + 1.0)) * np.pi / M.H
    ph = (np.arange(M.W)[:, None] + 0.5 * (x[None, :] + 1.0)) * 2 * np.pi / M.W
    wt, wp = np.broadcast_to(0.5 * wx * np.pi / M.H, th.shape), np.broadcast_to(0.5 * wx * 2 * np.pi / M.W, ph.shape)
    T, P = np.meshgrid(th.ravel(), ph.ravel(), indexing="ij")
    Wq = (wt.ravel() * np.sin(th.ravel()))[:, None] * wp.ravel()[None, :]
    dirs = np.stack([np.sin(T) * np.cos(P), np.cos(T), np.sin(T) * np.sin(P)], axis=-1).reshape(-1, 3)
    for beta in (0.0, 0.25, 0.5):
        for normal, tol in (([0.0, 1.0, 0.0], 1e-9), ([0.6, 0.64, 0.48], 1e-3)):
            total = float(Wq.ravel() @ M.mixture_density64(t, beta, dirs, normal))
            assert abs(total - 1.0) < tol, (beta, normal, total)


def test_draws_from_the_table_map_back_to_their_cell(oracle, capsys):
    """Of 2^20 table draws of the restatement, the share whose direction the look-up's mapping puts into a neighbouring cell stays under the cap of 1e-3, and every
    such direction lies in a cell next to the drawn one"""
    n = 1 << 20
    rng = np.random.default_rng(5)
    u = rng.random((n, 2)).astype(f32)
    nrm = np.tile(np.array([[0.0, 1.0, 0.0]], f32), (n, 1))
    for env in (("ibl", M.sun_image()), ("constant",)):
        t = M.Table(M.weights_of(env, oracle))
        d, p, c = M.sample_table(t, 0.0, u[:, 0], u[:, 1], nrm, oracle)
        back = M.cell_of(d, oracle)
        off = back != c
        share = off.mean()
        with capsys.disabled():
            print(f"\n[env sampling] {env[0]}: {off.sum()} of {n} table draws map back to a neighbouring cell ({share:.2e}; cap 1e-3)")
        assert share <= 1e-3
        di = np.abs(back[off] % M.W - c[off] % M.W)
        dj = np.abs(back[off] // M.W - c[off] // M.W)
        pole = (c[off] // M.W == 0) | (c[off] // M.W == M.H - 1)
        assert ((np.minimum(di, M.W - di) <= 1) & (dj <= 1) | pole).all()
        assert np.isfinite(p).all() and (p > 0).all()
