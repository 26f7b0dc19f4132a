"""CPU tests of local exposure (include/fredholm_hip.h: fh_set_local_exposure ... fh_get_local_exposure_base): the exported symbols and the layout of the struct,
every refusal -- decided from the arguments alone, with a NULL context --, the facades (kernels/post-process.h with FH_LOCAL_EXPOSURE, the Python methods, rtcamp's
flags), and csrc/fh_local_exposure.h compiled for the host (with -fsanitize=address,undefined) into a stand-alone program whose log image, quarter image, base,
upsampled base, gain and tone-mapped pixels must equal, bit for bit, the numpy restatement the device tests use (tests/test_gpu_local_exposure.py), on those tests'
images.  The kernels are tested on the GPU.

FLOAT32 AGAINST FLOAT64.  bound(passes), the distance allowed between the float32 restatement and its float64 twin, counts the float32 roundings on the way to a value,
each taken at half an ulp of the largest magnitude a log-luminance has here (below 32 stops: e = 32 * 2^-24 = 1.9e-6), to first order, where a rounding moves a
result by at most its own size -- the means of steps 2 - 4 are convex combinations, and the relative error of a weight moves a mean by its share of the mean times
the tap's distance from it, which the edge stop keeps small for every tap whose share is not.  Per pixel: step 1, 6 (two products, a product and two sums in lum,
the log2); step 2, 16 (15 sums, the division); step 3, per pass 8 per tap (difference, scaling, square, two for the exponential, the kernel product, the product
with D_q, the sum) for 25 taps, and the division: 201; step 4, 6 for the coordinates and weights, 8 per tap for four taps, the division: 39; step 5, 6 (the log2 of
the exposure, two sums, the product, the power, all in stops).  bound(passes) = (67 + 201 * passes) * e: 5.1e-4 stops for 1 pass, 1.7e-3 for 4, 2.4e-3 for 6.  It is asserted
on the base, on B and on log2(x) -- on images without negative channels, since lum() of a negative and a positive channel cancels, and what is left of such a sum has
no relative accuracy in either format; the pixels where the two formats disagree on `den > 1e-6` (step 4 is discontinuous there) are counted, and there are none.
Measured (printed by the test): 5.6e-6 stops at the most.

OPERATOR PROPERTIES, asserted on the float64 twin (the device equals the float32 restatement bit for bit and that one the twin within the bound above): a 128 x 96
step in the middle column between two plateaus E stops apart with Gaussian log-noise of 0.3 stops, defaults (factor 4, 4 passes, sigma_range 1).
halo = the worst |B - plateau| over all pixels, detail = std(l - B) / 0.3, contrast = the distance of the plateau means after the gain over E.
  E = 3: halo 0.0403, detail 0.9983, contrast 0.4994;  E = 6: halo 0.0241, detail 0.9984, contrast 0.4997;  E = 10: halo 0.0241, detail 0.9984, contrast 0.4998.
Asserted: halo <= 0.05 stops, detail in [0.95, 1.05], |contrast * E - 0.5 * E| <= 0.05.
The operator's limits, stated and not tested as successes.  An edge of 2 stops is inside 2 sigma_range and is smoothed by design: halo 0.49 stops.  The middle
column is a block boundary of the quarter image; with the step two columns to its left the blocks that straddle it average both plateaus, and the worst pixel beside
it is off by 1.31 stops at E = 3, 0.26 at E = 6 and 0.024 at E = 10 (detail 1.027, 0.997, 0.998): the halo is one block wide and shrinks as the edge grows past
sigma_range, because step 4 then gives the mixed quarter pixel no weight."""
import ctypes as C
import inspect
import os
import struct
import subprocess

import numpy as np
import pytest

from fredholm_amd import native as N

import test_gpu_local_exposure as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINK = ["-L" + os.path.join(ROOT, "fredholm_amd"), "-lfredholm_hip", "-Wl,-rpath," + os.path.join(ROOT, "fredholm_amd"), "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
FH_E_INVALID = -1
FIELDS = [name for name, _ in N.LocalExposureParamsC._fields_]  # (at import: every test of this file is about the feature and needs the library that has it)
E_STOP = 32 * 2.0 ** -24


def bound(passes):
    return (67 + 201 * passes) * E_STOP


def _params_c(**kw):
    p = X.params(**kw)
    return N.LocalExposureParamsC(*[p[k] for k in FIELDS])


def test_symbols_struct_and_header_agree(tmp_path):
    assert FIELDS == ["highlights", "shadows", "pivot", "max_stops", "sigma_range", "passes"]
    L = N.load_library()
    want = {"fh_set_local_exposure": [C.c_void_p, C.POINTER(N.LocalExposureParamsC)],
            "fh_get_local_exposure": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(N.LocalExposureParamsC)],
            "fh_local_exposure_analyse": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32],
            "fh_get_local_exposure_base": [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]}
    for name, sig in want.items():
        assert name in N.EXPORTS
        fn = getattr(L, name)
        assert fn.restype is C.c_int and fn.argtypes == N.SIGNATURES[name] == sig, name
    hdr = " ".join(open(os.path.join(ROOT, "include", "fredholm_hip.h")).read().split())
    for decl in ("int fh_set_local_exposure(fh_ctx* ctx, const fh_local_exposure_params* params);",
                 "int fh_get_local_exposure(fh_ctx* ctx, int* on, fh_local_exposure_params* params);",
                 "int fh_local_exposure_analyse(fh_ctx* ctx, const float* image_rgba, uint32_t width, uint32_t height);",
                 "int fh_get_local_exposure_base(fh_ctx* ctx, float* base, uint32_t* w4, uint32_t* h4);"):
        assert decl in hdr, decl
    prints = "".join(f'printf("%zu\\n", offsetof(fh_local_exposure_params, {f}));' for f in FIELDS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fredholm_hip.h"\nint main(void) { printf("%zu %zu\\n", sizeof(fh_local_exposure_params), '
                   'sizeof(fh_post_params)); ' + prints + ' return 0; }\n')
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:2] == [C.sizeof(N.LocalExposureParamsC), C.sizeof(N.PostParamsC)] == [24, 20]  # fh_post_params does not change
    assert got[2:] == [getattr(N.LocalExposureParamsC, f).offset for f in FIELDS] == [4 * k for k in range(6)]


nan, inf = float("nan"), float("inf")
REFUSALS = [
    ([dict(highlights=-0.1), dict(highlights=1.5), dict(highlights=nan)], "highlights must be in [0, 1]"),
    ([dict(shadows=-0.1), dict(shadows=inf), dict(shadows=nan)], "shadows must be in [0, 1]"),
    ([dict(pivot=0.0), dict(pivot=-1.0), dict(pivot=nan), dict(pivot=inf)], "pivot must be finite and > 0"),
    ([dict(max_stops=-1.0), dict(max_stops=nan), dict(max_stops=inf)], "max_stops must be finite and >= 0"),
    ([dict(sigma_range=0.0), dict(sigma_range=-1.0), dict(sigma_range=nan), dict(sigma_range=inf)], "sigma_range must be finite and > 0"),
    ([dict(passes=0), dict(passes=7), dict(passes=0xffffffff)], "passes must be 1 .. 6"),
]


def test_every_refusal_is_decided_before_the_context_is_looked_at():
    """with a NULL context: each bad parameter is refused with its own message; good parameters and NULL (off) get as far as the context check"""
    L = N.lib()
    for cases, why in REFUSALS:
        for bad in cases:
            assert L.fh_set_local_exposure(None, C.byref(_params_c(**bad))) == FH_E_INVALID
            assert L.fh_last_error(None).decode() == "fh_set_local_exposure: " + why, bad
    L.fh_denoise_history_reset(None)
    marker = L.fh_last_error(None)
    for good in (dict(), dict(highlights=0.0, shadows=1.0), dict(max_stops=0.0), dict(passes=1), dict(passes=6), dict(sigma_range=0.25), dict(pivot=1e-3)):
        assert L.fh_set_local_exposure(None, C.byref(_params_c(**good))) == FH_E_INVALID and L.fh_last_error(None) == marker, good
    assert L.fh_set_local_exposure(None, None) == FH_E_INVALID
    on, w4, h4 = C.c_int(0), C.c_uint32(0), C.c_uint32(0)
    assert L.fh_get_local_exposure(None, C.byref(on), None) == FH_E_INVALID
    assert L.fh_get_local_exposure_base(None, None, C.byref(w4), C.byref(h4)) == FH_E_INVALID
    assert L.fh_get_local_exposure_base(None, None, None, C.byref(h4)) == FH_E_INVALID
    assert L.fh_last_error(None).decode() == "fh_get_local_exposure_base: null argument"
    for img, w, h in ((None, 4, 4), (C.c_void_p(16), 0, 4), (C.c_void_p(16), 4, 0), (C.c_void_p(16), 32769, 1), (C.c_void_p(16), 1, 32769)):
        assert L.fh_local_exposure_analyse(None, img, w, h) == FH_E_INVALID
        assert L.fh_last_error(None).decode() == "fh_local_exposure_analyse: needs an image of 1 .. 32768 pixels each way"


def test_python_facade_has_the_methods_with_the_library_defaults():
    from fredholm_amd.renderer import Renderer
    sig = inspect.signature(Renderer.set_local_exposure).parameters
    assert list(sig)[1:] == FIELDS
    for k, v in X.DEFAULTS.items():
        assert sig[k].default == v, k
    for name in ("clear_local_exposure", "get_local_exposure", "local_exposure_base"):
        assert callable(getattr(Renderer, name))
    assert list(inspect.signature(Renderer.local_exposure_analyse).parameters)[1:] == ["image_ptr", "width", "height"]
    hdr = open(os.path.join(ROOT, "fredholm_amd", "csrc", "fh_local_exposure.h")).read()
    assert "{0.5f, 0.5f, 0.18f, 4.0f, 1.0f, 4u}" in hdr and "{0.5f, 0.5f, 0.18f, 4.0f, 1.0f, 4u}" in open(os.path.join(ROOT, "fredholm_amd", "csrc", "context.h")).read()


# ------------------------------------------------------------------ the C++ facade over stubbed entry points
FACADE = r"""
#include "kernels/post-process.h"
#include <cstdio>
#include <cstring>
extern "C" int fh_ctx_create(int, fh_ctx** out) { *out = reinterpret_cast<fh_ctx*>(0x10); return FH_OK; }  // never dereferenced: the entries are the ones below
extern "C" int fh_ctx_create_group(const int*, uint32_t, fh_ctx** out) { *out = reinterpret_cast<fh_ctx*>(0x10); return FH_OK; }
extern "C" const char* fh_last_error(fh_ctx*) { return "stub"; }
extern "C" int fh_post_process(fh_ctx*, const float*, float*, float*, int, int, const fh_post_params*, float*) { std::printf("fh_post_process\n"); return FH_OK; }
extern "C" int fh_set_auto_exposure(fh_ctx*, const fh_auto_exposure_params*) { std::printf("fh_set_auto_exposure\n"); return FH_OK; }
extern "C" int fh_get_auto_exposure_state(fh_ctx*, fh_auto_exposure_state*) { return FH_OK; }
extern "C" int fh_auto_exposure_reset(fh_ctx*) { return FH_OK; }
extern "C" int fh_set_local_exposure(fh_ctx*, const fh_local_exposure_params* p)
{
  if (p) std::printf("fh_set_local_exposure %g %g %g %g %g %u\n", (double)p->highlights, (double)p->shadows, (double)p->pivot, (double)p->max_stops, (double)p->sigma_range, p->passes);
  else std::printf("fh_set_local_exposure off\n");
  return FH_OK;
}
int main(int argc, char** argv)
{
  const char* what = argc > 1 ? argv[1] : "default";
  PostProcessParams pp{false, 2.0f, 5.0f, 80.0f, 1.0f};
  auto launch = [&] { post_process_kernel_launch(nullptr, nullptr, nullptr, 64, 48, pp, nullptr); };
  try {
    if (std::strcmp(what, "set") == 0) { LocalExposureParams l; l.highlights = 0.75f; l.sigma_range = 2.0f; l.passes = 3; set_local_exposure(&l); }
    if (std::strcmp(what, "off") == 0) set_local_exposure(nullptr);
    launch();
    launch();  // (the variable is read once)
  } catch (const std::exception& e) { std::printf("error %s\n", e.what()); return 3; }
  return 0;
}
"""


@pytest.fixture(scope="module")
def facade(tmp_path_factory):
    d = tmp_path_factory.mktemp("local_exposure_facade")
    src = d / "facade.cpp"
    src.write_text(FACADE)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(d / "facade")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(d / "facade")


def _run(exe, *args, env=None, rc=0):
    e = {k: v for k, v in os.environ.items() if k not in ("FH_AUTO_EXPOSURE", "FH_LOCAL_EXPOSURE", "FH_DEVICES")}
    e.update(env or {})
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=e)
    assert r.returncode == rc, (r.stdout, r.stderr)
    return r.stdout.splitlines()


def test_the_environment_variable_and_set_local_exposure_reach_the_entry_point(facade):
    twice = ["fh_post_process", "fh_post_process"]
    defaults = "fh_set_local_exposure 0.5 0.5 0.18 4 1 4"
    assert _run(facade) == twice  # (unset: the switch is not touched)
    assert _run(facade, env={"FH_LOCAL_EXPOSURE": "0"}) == twice
    assert _run(facade, env={"FH_LOCAL_EXPOSURE": "1"}) == [defaults] + twice
    assert _run(facade, env={"FH_LOCAL_EXPOSURE": "0.25"}) == ["fh_set_local_exposure 0.25 0.25 0.18 4 1 4"] + twice  # a strength: both shares
    assert _run(facade, env={"FH_LOCAL_EXPOSURE": "soft"}, rc=3)[0].startswith("error FH_LOCAL_EXPOSURE")
    mine = "fh_set_local_exposure 0.75 0.5 0.18 4 2 3"
    assert _run(facade, "set") == [mine] + twice
    assert _run(facade, "set", env={"FH_LOCAL_EXPOSURE": "1"}) == [mine] + twice  # (what the application set wins)
    assert _run(facade, "off", env={"FH_LOCAL_EXPOSURE": "1"}) == ["fh_set_local_exposure off"] + twice
    assert _run(facade, env={"FH_LOCAL_EXPOSURE": "1", "FH_AUTO_EXPOSURE": "1"}) == ["fh_set_auto_exposure", defaults] + twice  # the two switches are independent


def test_rtcamp_refuses_local_flags_without_the_switch_and_bad_values(tmp_path):
    rt = tmp_path / "rtcamp"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "rtcamp.cpp"), *LINK, "-lpthread", "-o", str(rt)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for flags in (["--local-highlights", "0.3"], ["--local-shadows", "0.3"], ["--local-sigma", "2"], ["--local-passes", "3"]):
        run = subprocess.run([str(rt), "--scene", "x.obj", *flags], capture_output=True, text=True)
        assert run.returncode == 2 and flags[0] + " goes with --local-exposure" in run.stderr, (flags, run.stderr)
    for flags in (["--local-highlights", "1.5"], ["--local-highlights", "nan"], ["--local-shadows", "-0.1"], ["--local-sigma", "0"], ["--local-sigma", "inf"],
                  ["--local-passes", "0"], ["--local-passes", "7"]):
        run = subprocess.run([str(rt), "--scene", "x.obj", "--local-exposure", *flags], capture_output=True, text=True)
        assert run.returncode == 2 and flags[0] + " must be" in run.stderr, (flags, run.stderr)
    run = subprocess.run([str(rt), "--scene", "x.obj", "--local-exposure", "--local-sigma"], capture_output=True, text=True)
    assert run.returncode == 2 and "missing value" in run.stderr
    run = subprocess.run([str(rt)], capture_output=True, text=True)
    assert run.returncode == 2 and "--local-exposure" in run.stderr and "--local-passes" in run.stderr


# ------------------------------------------------------------------ fh_local_exposure.h on the host against the restatement
PROGRAM = r"""
// reads: 6 words of fh_local_exposure_params, the exposure, w, h, then w * h * 4 floats; writes the log image (w * h), the quarter image and the base (w4 * h4 each),
// B and x (w * h each) and the tone-mapped r, g, b of every pixel with chromatic aberration 0 (3 * w * h)
#include <cstdio>
#include <vector>
#include "fh_local_exposure.h"
#include "fh_tonemap.h"
int main(int argc, char** argv)
{
  if (argc != 3) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) return 2;
  fh_local_exposure_params p;
  float exposure = 0.0f;
  uint32_t wh[2] = {0, 0};
  if (std::fread(&p, sizeof p, 1, in) != 1 || std::fread(&exposure, 4, 1, in) != 1 || std::fread(wh, 4, 2, in) != 2) return 2;
  if (const char* why = fh::local_exposure_refusal(&p)) { std::fprintf(stderr, "%s\n", why); return 3; }
  const int w = (int)wh[0], h = (int)wh[1], w4 = fh::lx_quarter(w), h4 = fh::lx_quarter(h);
  std::vector<float> px(4 * (size_t)w * h);
  if (std::fread(px.data(), 16, (size_t)w * h, in) != (size_t)w * h) return 2;
  const fh::LxConsts c = fh::lx_consts(p);
  std::vector<float> L((size_t)w * h), q[2] = {std::vector<float>((size_t)w4 * h4), std::vector<float>((size_t)w4 * h4)}, B((size_t)w * h), x((size_t)w * h), rgb(3 * (size_t)w * h);
  for (int i = 0; i < w * h; ++i) L[i] = fh::lx_log(px[4 * i], px[4 * i + 1], px[4 * i + 2]);
  for (int Y = 0; Y < h4; ++Y)
    for (int X = 0; X < w4; ++X) {
      const int n_cols = w - 4 * X < 4 ? w - 4 * X : 4, n_rows = h - 4 * Y < 4 ? h - 4 * Y : 4;
      float row[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      for (int k = 0; k < n_rows; ++k) {
        float l[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int a = 0; a < n_cols; ++a) l[a] = L[(4 * X + a) + w * (4 * Y + k)];
        row[k] = fh::lx_row_sum(l[0], l[1], l[2], l[3], n_cols);
      }
      q[0][X + w4 * Y] = fh::lx_block_mean(row[0], row[1], row[2], row[3], n_rows, n_cols);
    }
  std::fwrite(L.data(), 4, L.size(), out);
  std::fwrite(q[0].data(), 4, q[0].size(), out);
  for (uint32_t it = 0; it < p.passes; ++it)
    for (int Y = 0; Y < h4; ++Y)
      for (int X = 0; X < w4; ++X) q[(it + 1) & 1][X + w4 * Y] = fh::lx_atrous(q[it & 1].data(), w4, h4, X, Y, 1 << it, c.inv_sr);
  const std::vector<float>& base = q[p.passes & 1];
  std::fwrite(base.data(), 4, base.size(), out);
  for (int j = 0; j < h; ++j)
    for (int i = 0; i < w; ++i) {
      const int k = i + w * j;
      B[k] = fh::lx_upsample(base.data(), w4, h4, i, j, L[k], c.inv_sr);
      x[k] = fh::lx_gain(B[k], exposure, c);
      for (int ch = 0; ch < 3; ++ch) rgb[3 * k + ch] = fh::srgb1(fh::uchimura1(px[4 * k + ch] * x[k]));
    }
  std::fwrite(B.data(), 4, B.size(), out);
  std::fwrite(x.data(), 4, x.size(), out);
  std::fwrite(rgb.data(), 4, rgb.size(), out);
  std::fclose(in);
  std::fclose(out);
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """csrc/fh_local_exposure.h compiled for the host, with the address and undefined-behaviour sanitizers, into a stand-alone program"""
    d = tmp_path_factory.mktemp("local_exposure_host")
    src = d / "lx.cpp"
    src.write_text(PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-I" + os.path.join(ROOT, "fredholm_amd", "csrc"), str(src), "-o", str(d / "lx")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(p, exposure, img):
        h, w = img.shape[:2]
        blob = struct.pack("<5fI", *[p[k] for k in FIELDS]) + struct.pack("<fII", exposure, w, h) + np.ascontiguousarray(img, dtype=np.float32).tobytes()
        (d / "in.bin").write_bytes(blob)
        r = subprocess.run([str(d / "lx"), str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        raw = np.frombuffer((d / "out.bin").read_bytes(), dtype=np.float32)
        n, (h4, w4) = w * h, ((h + 3) // 4, (w + 3) // 4)
        cuts = np.cumsum([n, h4 * w4, h4 * w4, n, n, 3 * n])
        assert raw.size == cuts[-1]
        L, D0, base, B, x, rgb = np.split(raw, cuts[:-1])
        return dict(L=L.reshape(h, w), D0=D0.reshape(h4, w4), base=base.reshape(h4, w4), B=B.reshape(h, w), x=x.reshape(h, w), rgb=rgb.reshape(h, w, 3))
    return run


def test_the_header_on_the_host_equals_the_restatement_bit_for_bit(program, oracle):
    ops = X.Ops32(oracle)
    for (w, h) in X.FRAMES:
        for which, p in X.PARAMS.items():
            for exposure in (X.iso_exposure(oracle, 80.0), np.float32(0.0371)):
                img = X.image(w, h)
                got = program(p, float(exposure), img)
                base, x, diag = X.local_gain(ops, img, p, exposure)
                for name, want in (("L", diag["L"]), ("D0", diag["D0"]), ("base", base), ("B", diag["B"]), ("x", x)):
                    assert np.array_equal(X._bits(got[name]), X._bits(want)), (w, h, which, name, np.argwhere(X._bits(got[name]) != X._bits(want))[:4])
                want = X.tone_map(oracle, img, x, 0.0)
                assert X.same_bits(got["rgb"], want).all(), (w, h, which)
    # the images of the chain variants, and a black one
    for img in (X.image(70, 45, X.MILD_SPECIALS, seed=1), X.image(70, 45, seed=1), np.zeros((45, 70, 4), np.float32)):
        got = program(X.DEFAULTS, 0.5, img)
        base, x, diag = X.local_gain(ops, img, X.DEFAULTS, np.float32(0.5))
        assert np.array_equal(X._bits(got["base"]), X._bits(base)) and np.array_equal(X._bits(got["x"]), X._bits(x))


def test_the_float32_and_float64_restatements_agree_within_the_bound(oracle, capsys):
    """bound(passes) of the docstring on the device tests' frames and parameters (no negative channels): printed, then asserted"""
    worst, flips = 0.0, 0
    for (w, h) in X.FRAMES:
        for which, p in X.PARAMS.items():
            img = X.image(w, h, [0.0, np.nan, np.inf, 3.2e38])
            e = X.iso_exposure(oracle, 80.0)
            b32, x32, d32 = X.local_gain(X.Ops32(oracle), img, p, e)
            b64, x64, d64 = X.local_gain(X.Ops64, img, p, e)
            same_branch = d32["fell_back"] == d64["fell_back"]
            flips += int((~same_branch).sum())
            dist = max(np.abs(b32 - b64).max(), np.abs(d32["B"] - d64["B"])[same_branch].max(), np.abs(np.log2(x32.astype(np.float64)) - np.log2(x64))[same_branch].max())
            worst = max(worst, dist)
            assert dist <= bound(p["passes"]), (w, h, which, dist)
    with capsys.disabled():
        print(f"\nlocal exposure: float32 against float64 restatement, largest distance {worst:.3g} stops (bound {bound(1):.3g} .. {bound(6):.3g}), branch flips {flips}")
    assert flips == 0


# ------------------------------------------------------------------ operator properties, on the float64 twin
def step_image(edge_stops, w=128, h=96, noise=0.3, seed=7):
    """grey: two plateaus edge_stops apart, symmetric about the pivot, the step in the middle column; Gaussian log-noise"""
    rng = np.random.default_rng(seed)
    plateau = np.where(np.arange(w)[None, :] < w // 2, -0.5 * edge_stops, 0.5 * edge_stops) + np.log2(0.18) + np.zeros((h, 1))
    img = np.ones((h, w, 4), np.float32)
    img[..., :3] = np.exp2(plateau + rng.normal(0.0, noise, (h, w)))[..., None].astype(np.float32)
    return img, plateau


def operator_figures(edge_stops):
    img, plateau = step_image(edge_stops)
    base, x, diag = X.local_gain(X.Ops64, img, X.DEFAULTS, 1.0)
    halo = float(np.abs(diag["B"] - plateau).max())
    detail = float(np.std(diag["L"] - diag["B"]) / 0.3)
    after = diag["L"] + np.log2(x)
    left = np.arange(img.shape[1]) < img.shape[1] // 2
    contrast = float((after[:, ~left].mean() - after[:, left].mean()) / edge_stops)
    return halo, detail, contrast


@pytest.mark.parametrize("edge_stops", [3, 6, 10])
def test_an_edge_stays_in_the_base_and_the_noise_out_of_it(edge_stops, capsys):
    halo, detail, contrast = operator_figures(edge_stops)
    with capsys.disabled():
        print(f"\nlocal exposure: {edge_stops}-stop edge: halo {halo:.4f} stops, detail {detail:.4f}, contrast {contrast:.4f}")
    assert halo <= 0.05
    assert 0.95 <= detail <= 1.05
    assert abs(contrast * edge_stops - (1.0 - 0.5) * edge_stops) <= 0.05
