"""CPU tests of the adaptive-sampling policy interface (include/fredholm_hip.h: fh_set_adaptive_policy): the exported symbols and their ctypes signatures, the
C++ facade and the batch driver's flags.  The behaviour itself is tested on the GPU (test_gpu_adaptive_policy.py)."""
import ctypes as C
import os
import subprocess

import pytest

from fredholm_amd import native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fh_set_adaptive_policy", "fh_get_adaptive_policy", "fh_adaptive_next_boundary")
LINK = ["-L" + os.path.join(ROOT, "fredholm_amd"), "-lfredholm_hip", "-Wl,-rpath," + os.path.join(ROOT, "fredholm_amd"), "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]


def test_new_symbols_are_exported_with_their_signatures():
    L = N.load_library()
    for name in NEW:
        assert name in N.EXPORTS
        fn = getattr(L, name)
        assert fn.restype is C.c_int
        assert fn.argtypes == N.SIGNATURES[name], name
    assert N.SIGNATURES["fh_set_adaptive_policy"] == [C.c_void_p, C.c_uint32, C.c_uint32]
    assert N.SIGNATURES["fh_get_adaptive_policy"] == [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    assert N.SIGNATURES["fh_adaptive_next_boundary"] == [C.c_void_p, C.POINTER(C.c_uint32)]
    hdr = open(os.path.join(ROOT, "include", "fredholm_hip.h")).read()
    assert "int fh_set_adaptive_policy(fh_ctx* ctx, uint32_t block, uint32_t growth);" in hdr
    assert "int fh_get_adaptive_policy(fh_ctx* ctx, uint32_t* block, uint32_t* growth);" in hdr
    assert "int fh_adaptive_next_boundary(fh_ctx* ctx, uint32_t* samples);" in hdr


def test_python_facade_has_the_policy_methods():
    from fredholm_amd.renderer import Renderer
    import inspect
    sig = inspect.signature(Renderer.set_adaptive_policy)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("block", 1), ("growth", 1)]
    assert callable(Renderer.adaptive_policy) and callable(Renderer.adaptive_next_boundary)


def test_facade_methods_compile_and_link(tmp_path):
    src = tmp_path / "policy_facade.cpp"
    src.write_text("""
#include "fredholm/renderer.h"
#include <cstdio>
int main()
{
  optwl::Context context;
  fredholm::Renderer renderer(context.get_context());
  renderer.set_resolution(64, 48);
  renderer.init_render_states();
  renderer.set_adaptive_policy();
  renderer.set_adaptive_policy(4, 2);
  uint32_t block = 0, growth = 0;
  renderer.adaptive_policy(block, growth);
  renderer.set_adaptive_sampling(0.05f);
  std::printf("%u %u %u\\n", block, growth, renderer.adaptive_next_boundary());
  return 0;
}
""")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), *LINK, "-o", str(tmp_path / "policy_facade")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.fixture(scope="module")
def rtcamp(tmp_path_factory):
    exe = tmp_path_factory.mktemp("rtcamp_policy") / "rtcamp"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "rtcamp.cpp"), *LINK, "-lpthread", "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def test_rtcamp_has_the_policy_flags(rtcamp):
    src = open(os.path.join(ROOT, "examples", "rtcamp.cpp")).read()
    for flag in ("--adaptive-block", "--adaptive-growth"):
        assert f'"{flag}"' in src
    assert "adaptive_next_boundary" in src  # (growth 2: the frame loop's calls end on boundaries)


@pytest.mark.parametrize("flag,value", [("--adaptive-block", "3"), ("--adaptive-block", "0"), ("--adaptive-block", "16"), ("--adaptive-growth", "3"), ("--adaptive-growth", "0")])
def test_rtcamp_refuses_values_outside_the_sets_before_any_device_work(rtcamp, flag, value):
    run = subprocess.run([rtcamp, "--scene", "x.obj", "--noise-threshold", "0.05", flag, value], capture_output=True, text=True)
    assert run.returncode == 2 and flag in run.stderr, (run.returncode, run.stderr)
