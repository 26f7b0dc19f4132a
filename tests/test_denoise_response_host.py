"""CPU tests of the interface of the temporal stage's history clipping (include/fredholm_hip.h: fh_set_denoise_response, fh_get_denoise_response): the exported symbols,
the layout of fh_response_params, the refusal -- decided from the argument alone --, the facades (fredholm::Denoiser::set_response, FH_DENOISER, the Python methods,
rtcamp's flags), and the restatement the replay tool and the device tests share (tests/test_gpu_denoise_response.py) against a window computed by hand.  The stage
itself is tested on the GPU."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

from fredholm_amd import native as N

import test_gpu_denoise_response as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINK = ["-L" + os.path.join(ROOT, "fredholm_amd"), "-lfredholm_hip", "-Wl,-rpath," + os.path.join(ROOT, "fredholm_amd"), "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
FH_E_INVALID = -1


def test_symbols_struct_and_header_agree(tmp_path):
    L = N.load_library()
    want = {"fh_set_denoise_response": [C.c_void_p, C.POINTER(N.ResponseParamsC)], "fh_get_denoise_response": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(N.ResponseParamsC)]}
    for name, sig in want.items():
        assert name in N.EXPORTS
        fn = getattr(L, name)
        assert fn.restype is C.c_int and fn.argtypes == N.SIGNATURES[name] == sig, name
    hdr = " ".join(open(os.path.join(ROOT, "include", "fredholm_hip.h")).read().split())
    assert "int fh_set_denoise_response(fh_ctx* ctx, const fh_response_params* params);" in hdr
    assert "int fh_get_denoise_response(fh_ctx* ctx, int* on, fh_response_params* params);" in hdr
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fredholm_hip.h"\nint main(void) { printf("%zu %zu\\n", sizeof(fh_response_params), offsetof(fh_response_params, gamma)); return 0; }\n')
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(N.ResponseParamsC), N.ResponseParamsC.gamma.offset] == [4, 0]


def test_a_bad_gamma_is_refused_before_the_context_is_looked_at():
    """with a NULL context: a bad gamma is refused with its own message, a good one and NULL (off) get as far as the context check"""
    L = N.lib()
    for bad in (0.0, -1.0, -0.0, float("nan"), float("inf"), -float("inf")):
        assert L.fh_set_denoise_response(None, C.byref(N.ResponseParamsC(bad))) == FH_E_INVALID
        msg = L.fh_last_error(None).decode()
        assert msg == "fh_set_denoise_response: gamma must be finite and > 0", (bad, msg)
    L.fh_denoise_history_reset(None)
    for good in (1.0, 1e-6, 1e6):
        assert L.fh_set_denoise_response(None, C.byref(N.ResponseParamsC(good))) == FH_E_INVALID
    assert L.fh_set_denoise_response(None, None) == FH_E_INVALID
    on = C.c_int(0)
    assert L.fh_get_denoise_response(None, C.byref(on), None) == FH_E_INVALID and L.fh_get_denoise_response(None, None, None) == FH_E_INVALID


def test_python_facade_has_the_methods_with_the_library_default():
    from fredholm_amd.renderer import Renderer
    assert inspect.signature(Renderer.set_denoise_response).parameters["gamma"].default == 1.0
    assert callable(Renderer.clear_denoise_response) and callable(Renderer.get_denoise_response)


SOURCE = r"""
#include "fredholm/denoiser.h"
#include <cstdio>
#include <cstring>
extern "C" int fh_denoise(fh_ctx*, uint32_t, uint32_t, const float*, const float*, const float*, float*, int) { std::printf("fh_denoise\n"); return FH_OK; }
extern "C" int fh_denoise_temporal(fh_ctx*, uint32_t, uint32_t, const fh_denoise_inputs*, const fh_camera*, const fh_temporal_params*, const fh_denoise_params*, float*, int)
{
  std::printf("fh_denoise_temporal\n");
  return FH_OK;
}
extern "C" int fh_set_denoise_motion(fh_ctx*, int on) { std::printf("fh_set_denoise_motion %d\n", on); return FH_OK; }
extern "C" int fh_set_denoise_response(fh_ctx*, const fh_response_params* params)
{
  if (params) std::printf("fh_set_denoise_response %g\n", (double)params->gamma);
  else std::printf("fh_set_denoise_response off\n");
  return FH_OK;
}
int main(int argc, char** argv)
{
  fh_ctx* ctx = reinterpret_cast<fh_ctx*>(0x10);  // never dereferenced: the entries are the ones above
  auto f4 = [](uintptr_t a) { return reinterpret_cast<const float4*>(a); };
  const char* what = argc > 1 ? argv[1] : "default";
  fredholm::Denoiser denoiser(ctx, 64, 48, f4(0x100), f4(0x200), f4(0x300), f4(0x400), false);
  if (std::strcmp(what, "on") == 0) { denoiser.set_mode(fredholm::Denoiser::Temporal); denoiser.set_response(true); }
  if (std::strcmp(what, "gamma") == 0) { denoiser.set_mode(fredholm::Denoiser::Temporal); denoiser.set_response(true, 2.5f); }
  if (std::strcmp(what, "off") == 0) { denoiser.set_mode(fredholm::Denoiser::Temporal); denoiser.set_response(false); }
  if (std::strcmp(what, "atrous") == 0) { denoiser.set_mode(fredholm::Denoiser::Atrous); denoiser.set_response(true); }
  denoiser.set_guides(f4(0x500), reinterpret_cast<const float*>(0x600));
  denoiser.set_camera(fredholm::Camera(make_float3(1, 2, 3), 0.5f));
  denoiser.denoise();
  denoiser.denoise();  // (the switch is sent once)
  std::printf("response %d %g\n", denoiser.response() ? 1 : 0, (double)denoiser.response_gamma());
  return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("response_modes")
    src = d / "modes.cpp"
    src.write_text(SOURCE)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), *LINK, "-o", str(d / "modes")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(d / "modes")


def _run(exe, *args, env=None):
    e = {k: v for k, v in os.environ.items() if k != "FH_DENOISER"}
    e.update(env or {})
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=e)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def test_set_response_and_the_environment_variable_reach_the_entry_point(exe):
    twice = ["fh_denoise_temporal", "fh_denoise_temporal"]
    assert _run(exe, "on") == ["fh_set_denoise_response 1"] + twice + ["response 1 1"]
    assert _run(exe, "gamma") == ["fh_set_denoise_response 2.5"] + twice + ["response 1 2.5"]
    assert _run(exe, "off") == ["fh_set_denoise_response off"] + twice + ["response 0 1"]
    assert _run(exe, env={"FH_DENOISER": "temporal-response"}) == ["fh_set_denoise_response 1"] + twice + ["response 1 1"]
    assert _run(exe, env={"FH_DENOISER": "temporal-motion-response"}) == ["fh_set_denoise_motion 1", "fh_set_denoise_response 1"] + twice + ["response 1 1"]
    assert _run(exe, env={"FH_DENOISER": "temporal"}) == twice + ["response 0 1"]  # (neither switch is touched)
    assert _run(exe, "atrous") == ["fh_denoise", "fh_denoise", "response 1 1"]    # (the switch belongs to the Temporal mode)


def test_rtcamp_knows_the_response_denoisers_and_the_gamma_flag(tmp_path):
    rt = tmp_path / "rtcamp"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "rtcamp.cpp"), *LINK, "-lpthread", "-o", str(rt)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(rt), "--scene", "x.obj", "--denoiser", "temporal-bogus"], capture_output=True, text=True)
    assert run.returncode == 2 and "temporal-response" in run.stderr and "temporal-motion-response" in run.stderr
    for bad in ("0", "-1", "nan", "inf"):
        run = subprocess.run([str(rt), "--scene", "x.obj", "--denoiser", "temporal-response", "--denoise-gamma", bad], capture_output=True, text=True)
        assert run.returncode == 2 and "--denoise-gamma" in run.stderr, (bad, run.stderr)
    run = subprocess.run([str(rt), "--scene", "x.obj", "--denoiser", "temporal", "--denoise-gamma", "1.5"], capture_output=True, text=True)
    assert run.returncode == 2 and "--denoise-gamma" in run.stderr and "response" in run.stderr  # (a gamma no denoiser would use is refused, not ignored)


def test_window_and_clip_of_a_hand_computed_case():
    """no GPU: a 3 x 3 frame, so every window is the whole frame, cut by the frame's edges (the taps beyond them are skipped).  Colours (r = g = b) 1 .. 9 row by row, the corner (2, 2)
    a miss, (0, 0) with a normal at right angles to the others.  Centre (1, 1): counting taps 2 .. 8 (7 of them: not the miss, not the turned normal), S1 = 35,
    S2 = 203, mu = 5, var = 203 / 7 - 25 = 4, sd = 2; gamma 0.5: the box is [4, 6].  A history of 10 is clipped to 6, u = |6 - 10| / (1 + 1e-6), k1 = 1 + u:
    h_h 8 becomes 8 / k1 and v_h 0.5 becomes 0.5 * k1.  A history of 5.5 stays, with u = 0.  (0, 0) has its window to itself: n = 1, not clipped."""
    for dt in (np.float64, np.float32):
        c = np.repeat(np.arange(1, 10, dtype=dt).reshape(3, 3, 1), 3, axis=2)
        nrm = np.zeros((3, 3, 4), np.float32)
        nrm[..., 2] = 1.0
        nrm[2, 2] = 0.0
        nrm[0, 0] = (1.0, 0.0, 0.0, 0.0)
        n, lo, hi, gsd = R.window_box(dt, c, nrm, 0.5, 0.5)
        assert n[1, 1] == 7 and n[0, 0] == 1 and n[0, 1] == 7 and n[2, 2] == 1  # (reach 2 in a 3 x 3 frame: every window is the frame; the miss counts itself only, and has no history anyway)
        assert np.allclose(lo[1, 1], 4.0, rtol=1e-6) and np.allclose(hi[1, 1], 6.0, rtol=1e-6) and np.allclose(gsd[1, 1], 1.0, rtol=1e-6)
        c_h = np.full((3, 3, 3), dt(10.0))
        c_h[1, 1, 1] = 5.5
        cc, v2, h2, u, _ = R.clip_history(dt, c, nrm, c_h, np.full((3, 3), dt(0.5)), np.full((3, 3), dt(8.0)), 0.5, 0.5)
        want_u = 4.0 / (1.0 + 1e-6)
        assert np.allclose(cc[1, 1], (6.0, 5.5, 6.0), rtol=1e-6) and np.isclose(u[1, 1], want_u, rtol=1e-6)
        assert np.isclose(h2[1, 1], 8.0 / (1.0 + want_u), rtol=1e-6) and np.isclose(v2[1, 1], 0.5 * (1.0 + want_u), rtol=1e-6)
        assert u[0, 0] == 0 and (cc[0, 0] == 10).all() and h2[0, 0] == 8 and v2[0, 0] == 0.5
        c_h[...] = 5.5
        cc, v2, h2, u, _ = R.clip_history(dt, c, nrm, c_h, np.full((3, 3), dt(0.5)), np.full((3, 3), dt(8.0)), 0.5, 0.5)
        assert u[1, 1] == 0 and (cc[1, 1] == 5.5).all() and h2[1, 1] == 8 and v2[1, 1] == 0.5
    # C's fmax drops a NaN where numpy's maximum returns it
    assert np.fmax(np.float32(np.nan), np.float32(0)) == 0 and np.isnan(np.maximum(np.float32(np.nan), np.float32(0)))
