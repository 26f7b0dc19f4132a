"""CPU tests of the adaptive-sampling interface (include/fredholm_hip.h: fh_set_adaptive_sampling): the exported symbols and their ctypes signatures, the
parameter struct's layout, the C++ facade and the batch driver's flags.  The behaviour itself is tested on the GPU (test_gpu_adaptive_sampling.py)."""
import ctypes as C
import os
import subprocess

from fredholm_amd import native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fh_set_adaptive_sampling", "fh_get_adaptive_sampling", "fh_get_sample_counts", "fh_get_luminance_moments", "fh_active_pixel_count", "fh_kat_set_issued")
LINK = ["-L" + os.path.join(ROOT, "fredholm_amd"), "-lfredholm_hip", "-Wl,-rpath," + os.path.join(ROOT, "fredholm_amd"), "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]


def test_new_symbols_are_exported_with_their_signatures():
    L = N.load_library()
    for name in NEW:
        assert name in N.EXPORTS
        fn = getattr(L, name)
        assert fn.restype is C.c_int
        assert fn.argtypes == N.SIGNATURES[name], name
    assert N.SIGNATURES["fh_set_adaptive_sampling"][1]._type_ is N.AdaptiveParamsC
    # the declarations in the headers carry the same names
    hdr = open(os.path.join(ROOT, "include", "fredholm_hip.h")).read() + open(os.path.join(ROOT, "include", "fredholm_hip_test.h")).read()
    for name in NEW:
        assert f"int {name}(fh_ctx* ctx" in hdr, name


def test_params_struct_has_the_header_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fredholm_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(fh_adaptive_params), offsetof(fh_adaptive_params, threshold), '
                   'offsetof(fh_adaptive_params, floor), offsetof(fh_adaptive_params, min_samples), offsetof(fh_adaptive_params, step)); return 0; }\n')
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = N.AdaptiveParamsC
    assert got == [C.sizeof(S), S.threshold.offset, S.floor.offset, S.min_samples.offset, S.step.offset] == [16, 0, 4, 8, 12]


def test_facade_methods_compile_and_link(tmp_path):
    src = tmp_path / "adaptive_facade.cpp"
    src.write_text("""
#include "fredholm/renderer.h"
#include <cstdio>
int main()
{
  optwl::Context context;
  fredholm::Renderer renderer(context.get_context());
  renderer.set_resolution(64, 48);
  renderer.init_render_states();
  renderer.set_adaptive_sampling(0.05f);
  renderer.set_adaptive_sampling(0.05f, 32, 4, 0.02f);
  cwl::CUDABuffer<uint32_t> counts(64 * 48);
  cwl::CUDABuffer<float2> moments(64 * 48);
  renderer.get_sample_counts(counts);
  renderer.get_luminance_moments(moments);
  std::printf("%u\\n", renderer.active_pixel_count());
  renderer.clear_adaptive_sampling();
  return 0;
}
""")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), *LINK, "-o", str(tmp_path / "adaptive_facade")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_rtcamp_builds_with_the_adaptive_flags(tmp_path):
    exe = tmp_path / "rtcamp"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "rtcamp.cpp"), *LINK, "-lpthread", "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(ROOT, "examples", "rtcamp.cpp")).read()
    for flag in ("--noise-threshold", "--min-spp", "--adaptive-step"):
        assert f'"{flag}"' in src
    # bad adaptive arguments are refused before any device work
    run = subprocess.run([str(exe), "--scene", "x.obj", "--noise-threshold", "0.05", "--min-spp", "1"], capture_output=True, text=True)
    assert run.returncode == 2 and "--min-spp" in run.stderr
