"""Sampling of area lights by power, the parts that need no GPU: the ABI (symbols, struct, header), the refusals decided before the context, the facades and rtcamp's
flags, and csrc/fh_lights.h compiled for the host (with -fsanitize=address,undefined) into a stand-alone program that is given areas and emission colours and must
reproduce, bit for bit, the weights, integer weights, CDF, pick probabilities and picks of the numpy restatement (light_sampling_model.py).  Then what the float64
model must satisfy: its mean is Lambert's polygon formula whatever the pick distribution, and the rule that chose the default uniform share."""
import ctypes as C
import inspect
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from fredholm_amd import native as N

import light_sampling_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINK = ["-L" + os.path.join(ROOT, "fredholm_amd"), "-lfredholm_hip", "-Wl,-rpath," + os.path.join(ROOT, "fredholm_amd"), "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
FH_E_INVALID = -1
f32 = np.float32


def test_symbols_struct_and_header_agree(tmp_path):
    L = N.load_library()
    want = {"fh_set_light_sampling": [C.c_void_p, C.POINTER(N.LightSamplingParamsC)],
            "fh_get_light_sampling": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(N.LightSamplingParamsC)],
            "fh_kat_light_table": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)],
            "fh_kat_light_pick": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]}
    for name, sig in want.items():
        assert name in N.EXPORTS
        fn = getattr(L, name)
        assert fn.restype is C.c_int and fn.argtypes == N.SIGNATURES[name] == sig, name
    hdr = " ".join(open(os.path.join(ROOT, "include", "fredholm_hip.h")).read().split())
    hdr_test = " ".join(open(os.path.join(ROOT, "include", "fredholm_hip_test.h")).read().split())
    for decl in ("int fh_set_light_sampling(fh_ctx* ctx, const fh_light_sampling_params* params);", "int fh_get_light_sampling(fh_ctx* ctx, int* on, fh_light_sampling_params* params);",
                 "#define FH_LIGHT_UNIFORM_FRACTION_DEFAULT %sf" % repr(N.LIGHT_UNIFORM_FRACTION_DEFAULT)):
        assert decl in hdr, decl
    for decl in ("int fh_kat_light_table(fh_ctx* ctx, uint32_t* q, float* cdf, float* pick_p_per_light, uint64_t* total);",
                 "int fh_kat_light_pick(fh_ctx* ctx, uint32_t n, const float* u1, uint32_t* index, float* p);"):
        assert decl in hdr_test, decl
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fredholm_hip.h"\nint main(void) { printf("%zu %zu %.9g\\n", sizeof(fh_light_sampling_params), '
                   'offsetof(fh_light_sampling_params, uniform_fraction), (double)FH_LIGHT_UNIFORM_FRACTION_DEFAULT); return 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(got[0]), int(got[1])] == [C.sizeof(N.LightSamplingParamsC), N.LightSamplingParamsC.uniform_fraction.offset] == [4, 0]
    assert float(got[2]) == float(f32(N.LIGHT_UNIFORM_FRACTION_DEFAULT))


def test_the_refusal_is_decided_before_the_context_is_looked_at():
    """with a NULL context: a fraction outside (0, 1] is refused with its message; good fractions and NULL (off) get as far as the context check"""
    L = N.lib()
    for bad in (0.0, -0.01, 1.5, float("nan"), float("inf"), -float("inf"), float(np.nextafter(f32(1), f32(2)))):
        assert M.refused(bad)
        assert L.fh_set_light_sampling(None, C.byref(N.LightSamplingParamsC(bad))) == FH_E_INVALID
        assert L.fh_last_error(None).decode() == "fh_set_light_sampling: uniform_fraction must be in (0, 1]", bad
    L.fh_denoise_history_reset(None)
    marker = L.fh_last_error(None)
    for good in (1.0, 0.0625, 0.125, 0.25, 0.5, float(np.nextafter(f32(0), f32(1)))):
        assert not M.refused(good)
        assert L.fh_set_light_sampling(None, C.byref(N.LightSamplingParamsC(good))) == FH_E_INVALID and L.fh_last_error(None) == marker, good
    assert L.fh_set_light_sampling(None, None) == FH_E_INVALID and L.fh_last_error(None) == marker
    on = C.c_int(0)
    assert L.fh_get_light_sampling(None, C.byref(on), None) == FH_E_INVALID
    for hook in ("fh_kat_light_table", "fh_kat_light_pick"):
        assert getattr(L, hook)(*[0 if a is C.c_uint32 else None for a in N.SIGNATURES[hook]]) == FH_E_INVALID


def test_python_facade_has_the_methods_with_the_library_default():
    from fredholm_amd.renderer import Renderer
    assert inspect.signature(Renderer.set_light_sampling).parameters["uniform_fraction"].default == N.LIGHT_UNIFORM_FRACTION_DEFAULT
    assert N.LIGHT_UNIFORM_FRACTION_DEFAULT in (0.5, 0.25, 0.125, 0.0625)
    for name in ("clear_light_sampling", "get_light_sampling"):
        assert callable(getattr(Renderer, name))


# ------------------------------------------------------------------ the C++ facade over stubbed entry points
FACADE = r"""
#include "fredholm/renderer.h"
#include <cstdio>
#include <cstring>
extern "C" int fh_ctx_create(int, fh_ctx** out) { *out = reinterpret_cast<fh_ctx*>(0x10); return FH_OK; }  // never dereferenced: the entries are the ones below
extern "C" int fh_ctx_create_group(const int*, uint32_t, fh_ctx** out) { *out = reinterpret_cast<fh_ctx*>(0x10); return FH_OK; }
extern "C" int fh_ctx_destroy(fh_ctx*) { return FH_OK; }
extern "C" const char* fh_last_error(fh_ctx*) { return "uniform_fraction must be in (0, 1]"; }
extern "C" int fh_set_light_sampling(fh_ctx*, const fh_light_sampling_params* p)
{
  if (p) std::printf("fh_set_light_sampling %g\n", (double)p->uniform_fraction);
  else std::printf("fh_set_light_sampling off\n");
  return p && !(p->uniform_fraction > 0.0f && p->uniform_fraction <= 1.0f) ? FH_E_INVALID : FH_OK;
}
int main(int argc, char** argv)
{
  const char* what = argc > 1 ? argv[1] : "default";
  try {
    optwl::Context context;
    fredholm::Renderer renderer(context.get_context());
    if (std::strcmp(what, "set") == 0) renderer.set_light_sampling(0.5f);
    if (std::strcmp(what, "on") == 0) renderer.set_light_sampling();
    if (std::strcmp(what, "off") == 0) renderer.clear_light_sampling();
    std::printf("ready\n");
  } catch (const std::exception& e) { std::printf("error %s\n", e.what()); return 3; }
  return 0;
}
"""


@pytest.fixture(scope="module")
def facade(tmp_path_factory):
    d = tmp_path_factory.mktemp("light_sampling_facade")
    (d / "facade.cpp").write_text(FACADE)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(d / "facade.cpp"), *LINK, "-lpthread", "-o", str(d / "facade")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(d / "facade")


def _run(exe, *args, env=None, rc=0):
    e = {k: v for k, v in os.environ.items() if k not in ("FH_LIGHT_SAMPLING", "FH_ENV_SAMPLING", "FH_DEVICES")}
    e.update(env or {})
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=e)
    assert r.returncode == rc, (r.stdout, r.stderr)
    return r.stdout.splitlines()


def test_the_environment_variable_and_the_facade_reach_the_entry_point(facade):
    default = "fh_set_light_sampling %g" % N.LIGHT_UNIFORM_FRACTION_DEFAULT
    assert _run(facade) == ["ready"]  # (unset: the switch is not touched)
    assert _run(facade, env={"FH_LIGHT_SAMPLING": "0"}) == ["ready"]
    assert _run(facade, env={"FH_LIGHT_SAMPLING": "1"}) == [default, "ready"]
    assert _run(facade, env={"FH_LIGHT_SAMPLING": "0.125"}) == ["fh_set_light_sampling 0.125", "ready"]
    assert _run(facade, env={"FH_LIGHT_SAMPLING": "bright"}, rc=3)[0].startswith("error FH_LIGHT_SAMPLING")
    assert _run(facade, env={"FH_LIGHT_SAMPLING": "1.5"}, rc=3)[-1].startswith("error ")  # (the library's refusal is thrown)
    assert _run(facade, "on") == [default, "ready"]
    assert _run(facade, "set", env={"FH_LIGHT_SAMPLING": "1"}) == [default, "fh_set_light_sampling 0.5", "ready"]  # (what the application sets afterwards wins)
    assert _run(facade, "off", env={"FH_LIGHT_SAMPLING": "1"}) == [default, "fh_set_light_sampling off", "ready"]


def test_rtcamp_refuses_the_fraction_without_the_switch_and_bad_values(tmp_path):
    rt = tmp_path / "rtcamp"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "rtcamp.cpp"), *LINK, "-lpthread", "-o", str(rt)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(rt), "--scene", "x.obj", "--light-uniform-fraction", "0.25"], capture_output=True, text=True)
    assert run.returncode == 2 and "--light-uniform-fraction goes with --light-sampling" in run.stderr, run.stderr
    for bad in ("0", "-0.1", "1.5", "nan"):
        run = subprocess.run([str(rt), "--scene", "x.obj", "--light-sampling", "--light-uniform-fraction", bad], capture_output=True, text=True)
        assert run.returncode == 2 and "--light-uniform-fraction must be in (0, 1]" in run.stderr, (bad, run.stderr)
    run = subprocess.run([str(rt)], capture_output=True, text=True)
    assert run.returncode == 2 and "--light-sampling" in run.stderr and "--light-uniform-fraction" in run.stderr


# ------------------------------------------------------------------ fh_lights.h on the host against the restatement
LIGHTS = r"""
// reads: U, n and n x (area, r, g, b); m and m draws u1.  writes: the 16 points (bu, bv); w [n]; q [n]; cdf [n + 1]; p [n]; the total (two words); per draw (index, p)
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
  if (std::fread(&U, 4, 1, in) != 1 || std::fread(&n, 4, 1, in) != 1 || n == 0) return 2;
  const fh_light_sampling_params prm = {U};
  if (const char* why = light_sampling_refusal(&prm)) { std::fprintf(stderr, "%s\n", why); return 3; }
  for (int s = 0; s < kLightPoints; ++s) { float b[2]; light_point(s, &b[0], &b[1]); std::fwrite(b, 4, 2, out); }
  std::vector<float> rec((size_t)n * 4), w(n), cdf((size_t)n + 1), p(n);
  std::vector<uint32_t> q(n);
  if (std::fread(rec.data(), 4, rec.size(), in) != rec.size()) return 2;
  for (uint32_t k = 0; k < n; ++k) w[k] = light_weight(rec[4 * k], rec[4 * k + 1], rec[4 * k + 2], rec[4 * k + 3]);
  uint64_t total = 0;
  light_build_host(w.data(), n, U, q.data(), cdf.data(), p.data(), &total);
  std::fwrite(w.data(), 4, n, out); std::fwrite(q.data(), 4, n, out); std::fwrite(cdf.data(), 4, cdf.size(), out); std::fwrite(p.data(), 4, n, out);
  std::fwrite(&total, 8, 1, out);
  if (std::fread(&m, 4, 1, in) != 1) return 2;
  for (uint32_t s = 0; s < m; ++s) {
    float u1;
    if (std::fread(&u1, 4, 1, in) != 1) return 2;
    const uint32_t k = light_pick(cdf.data(), n, U, u1);
    std::fwrite(&k, 4, 1, out); std::fwrite(&p[k], 4, 1, out);
  }
  std::fclose(in);
  std::fclose(out);
  return 0;
}
"""


@pytest.fixture(scope="module")
def lights(tmp_path_factory):
    """csrc/fh_lights.h compiled for the host, with the address and undefined-behaviour sanitizers, into a stand-alone program"""
    d = tmp_path_factory.mktemp("lights_host")
    (d / "lights.cpp").write_text(LIGHTS)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-I" + os.path.join(ROOT, "fredholm_amd", "csrc"), str(d / "lights.cpp"), "-o", str(d / "lights")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(U, rec, draws, rc=0):
        """rec: [n, 4] (area, r, g, b); draws [m]"""
        n = len(rec)
        blob = struct.pack("<fI", U, n) + np.ascontiguousarray(rec, f32).tobytes() + struct.pack("<I", len(draws)) + np.ascontiguousarray(draws, f32).tobytes()
        (d / "in.bin").write_bytes(blob)
        r = subprocess.run([str(d / "lights"), str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
        assert r.returncode == rc, r.stderr
        if rc:
            return r.stderr
        raw = np.frombuffer((d / "out.bin").read_bytes(), dtype=np.uint32)
        sizes = [2 * M.N_POINTS, n, n, n + 1, n, 2, 2 * len(draws)]
        assert raw.size == sum(sizes)
        parts = np.split(raw, np.cumsum(sizes)[:-1])
        return dict(points=parts[0].reshape(-1, 2), w=parts[1], q=parts[2], cdf=parts[3], p=parts[4], total=int(parts[5][0]) | int(parts[5][1]) << 32, picks=parts[6].reshape(-1, 2))
    return run


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _vectors():
    rng = np.random.default_rng(7)
    out = []

    def rec(areas, cols):
        return np.concatenate([np.asarray(areas, f32)[:, None], np.asarray(cols, f32).reshape(len(areas), 3)], axis=1)
    for n in (1, 2, 3):
        out.append(("n = %d" % n, rec(rng.uniform(0.1, 3.0, n), rng.uniform(0.0, 5.0, (n, 3)))))
    out.append(("all equal", rec(np.full(9, 0.75), np.tile([1.0, 2.0, 3.0], (9, 1)))))
    out.append(("all zero", rec(np.full(5, 2.0), np.zeros((5, 3)))))
    big = rec(np.full(40, 1.0), np.ones((40, 3)))
    big[17, 0] = 2.0 ** 25
    out.append(("one weight 2^25 x the rest: the floor q = 1 binds", big))
    odd = rec(rng.uniform(0.1, 3.0, 12), rng.uniform(0.0, 5.0, (12, 3)))
    odd[1, 1] = np.nan; odd[2, 2] = np.inf; odd[3, 3] = -np.inf; odd[4, 1:] = -1.0; odd[5, 0] = 0.0; odd[6, 0] = np.inf; odd[7, 1:] = 3.3e38; odd[8, 1:] = 1e38; odd[8, 0] = 1e10
    out.append(("NaN and infinite entries", odd))
    for n in (255, 256, 257, 1023, 1024, 1025, 65537):
        out.append(("n = %d" % n, rec(2.0 ** rng.uniform(-10, 4, n), rng.uniform(0.0, 5.0, (n, 3)) * rng.choice([0.0, 1.0, 50.0], (n, 1)))))
    return out


VECTORS = _vectors()


@pytest.mark.parametrize("U", (0.25, 1.0, 0.0625))
def test_the_header_on_the_host_equals_the_restatement_bit_for_bit(lights, U):
    assert (_bits(np.array(M.points(), f32)) == lights(U, VECTORS[0][1], [])["points"]).all()
    rng = np.random.default_rng(11)
    for what, rec in VECTORS:
        w = M.weight(rec[:, 0], rec[:, 1:])
        assert np.isfinite(w).all() and (w >= 0).all(), what
        t = M.Table(w, U)
        assert (t.q >= 1).all() and t.total == int(t.q.astype(np.uint64).sum()), what
        below = lambda x: np.nextafter(f32(x), f32(-1))
        edge = [0.0, below(U), U, below(1.0), below(below(1.0)), 0.5]
        # draws that land on CDF entries exactly, and just below them
        on_cdf = (f32(U) + (f32(1) - f32(U)) * t.cdf[rng.integers(0, t.n + 1, 64)]).astype(f32)
        u1 = np.concatenate([np.array(edge, f32), on_cdf, below(on_cdf), rng.random(4000).astype(f32)])
        u1 = u1[(u1 >= 0) & (u1 < 1)]
        got = lights(U, rec, u1)
        assert (got["w"] == _bits(w)).all(), what
        assert (got["q"] == t.q).all() and got["total"] == t.total, what
        assert (got["cdf"] == _bits(t.cdf)).all() and (got["p"] == _bits(t.p)).all(), what
        k, p = t.pick(u1)
        assert (got["picks"][:, 0] == k).all() and (got["picks"][:, 1] == _bits(p)).all(), what
        assert (k < t.n).all() and (p > 0).all(), what
    if U == 0.25:
        w = M.weight(VECTORS[5][1][:, 0], VECTORS[5][1][:, 1:])
        t = M.Table(w, U)
        assert t.q[17] == 1 << 20 and (np.delete(t.q, 17) == 1).all()
        assert (M.Table(M.weight(VECTORS[4][1][:, 0], VECTORS[4][1][:, 1:]), U).q == 1).all()


def test_the_program_refuses_what_the_library_refuses(lights):
    for bad in (0.0, -1.0, 1.5, float("nan")):
        assert "uniform_fraction must be in (0, 1]" in lights(bad, VECTORS[0][1], [], rc=3)


# ------------------------------------------------------------------ the float64 model
def test_the_model_mean_is_lamberts_formula_whatever_the_pick():
    from light_sampling_scenes import MODEL_X, MODEL_RHO, model_lights
    tris, les = model_lights()
    want = M.lambert_polygon(MODEL_X, (0.0, 1.0, 0.0), MODEL_RHO, tris, les)
    n = len(tris)
    for pick in (np.full(n, 1.0 / n), np.linspace(1.0, 3.0, n) / np.linspace(1.0, 3.0, n).sum()):
        mean, var, mu4 = M.lambert_floor_variance(MODEL_X, (0.0, 1.0, 0.0), MODEL_RHO, tris, les, pick)
        assert np.allclose(mean, want, rtol=2e-4), (mean, want)
        assert (var > 0).all() and (mu4 > var ** 2).all()


def test_the_default_share_follows_its_rule():
    """profiles/light_sampling_model.json: the largest share among 1/2, 1/4, 1/8, 1/16 whose predicted variance on the model scene is within 1.25 x of the best of them"""
    from light_sampling_scenes import model_prediction
    rec = json.load(open(os.path.join(ROOT, "profiles", "light_sampling_model.json")))
    shares = [0.5, 0.25, 0.125, 0.0625]
    var = {u: model_prediction(u)["variance_on"] for u in shares}
    best = min(var.values())
    chosen = max(u for u in shares if var[u] <= 1.25 * best)
    assert chosen == N.LIGHT_UNIFORM_FRACTION_DEFAULT == rec["default_uniform_fraction"]
    for u in shares:
        assert np.isclose(var[u], rec["variance_on"][repr(u)], rtol=1e-9)
