"""CPU tests of the interface of temporal accumulation (include/fredholm_hip.h: fh_denoise_temporal, fh_denoise_history_reset, fh_denoise_history_info): the exported
symbols and their ctypes signatures, the layout of fh_temporal_params, the refusals -- decided from the arguments alone, before the context or the device is touched --
the host-only check program (tools/temporal_host_check.cpp: refusals, camera inversion and the plan of a call), and the facades: fredholm::Denoiser's Temporal mode, Renderer::set_seed,
the Python methods and rtcamp's flag.  The stage itself is tested on the GPU (test_gpu_denoise_temporal.py)."""
import ctypes as C
import inspect
import json
import os
import subprocess

import numpy as np
import pytest

from fredholm_amd import native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINK = ["-L" + os.path.join(ROOT, "fredholm_amd"), "-lfredholm_hip", "-Wl,-rpath," + os.path.join(ROOT, "fredholm_amd"), "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
FH_E_INVALID = -1


def test_symbols_are_exported_with_their_signatures():
    L = N.load_library()
    want = {
        "fh_denoise_temporal": [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(N.DenoiseInputsC), C.POINTER(N.CameraC), C.POINTER(N.TemporalParamsC), C.POINTER(N.DenoiseParamsC),
                                C.c_void_p, C.c_int],
        "fh_denoise_history_reset": [C.c_void_p],
        "fh_denoise_history_info": [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
    }
    for name, sig in want.items():
        assert name in N.EXPORTS
        fn = getattr(L, name)
        assert fn.restype is C.c_int and fn.argtypes == N.SIGNATURES[name] == sig, name
    hdr = " ".join(open(os.path.join(ROOT, "include", "fredholm_hip.h")).read().split())
    assert ("int fh_denoise_temporal(fh_ctx* ctx, uint32_t width, uint32_t height, const fh_denoise_inputs* inputs, const fh_camera* camera, const fh_temporal_params* temporal, "
            "const fh_denoise_params* params, float* denoised, int upscale2x);") in hdr
    assert "int fh_denoise_history_reset(fh_ctx* ctx);" in hdr
    assert "int fh_denoise_history_info(fh_ctx* ctx, uint32_t* width, uint32_t* height, uint32_t* frames);" in hdr


def test_struct_has_the_header_layout(tmp_path):
    fields = ("alpha_min", "max_history", "normal_cos_min", "plane_tol")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fredholm_hip.h"\nint main(void) {\n  printf("%zu %zu\\n", sizeof(fh_temporal_params), sizeof(fh_camera));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(fh_temporal_params, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    T = N.TemporalParamsC
    assert [name for name, _ in T._fields_] == list(fields)
    want = [C.sizeof(T), C.sizeof(N.CameraC)] + [getattr(T, f).offset for f in fields]
    assert got == want == [16, 60, 0, 4, 8, 12]  # (60: the 15 floats the still-camera comparison covers, no padding)


def _camera(fov=1.0, t00=1.0):
    c = N.CameraC()
    for k, v in enumerate((t00, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)):
        c.transform[k] = v
    c.fov, c.F, c.focus = fov, 8.0, 100.0
    return c


OK_T, OK_P = (0.2, 32.0, 0.9, 0.02), (2.0, 1.0, 0.2, 7, 5)
FULL = [0x1000 * (k + 1) for k in range(7)]  # (made-up device addresses: never dereferenced)


def _call(ptrs=FULL, temporal=OK_T, params=OK_P, camera="default", w=8, h=8, dst=1 << 20):
    i = N.DenoiseInputsC(*ptrs)
    cam = _camera() if camera == "default" else camera
    rc = N.lib().fh_denoise_temporal(None, w, h, C.byref(i), None if cam is None else C.byref(cam), None if temporal is None else C.byref(N.TemporalParamsC(*temporal)),
                                     None if params is None else C.byref(N.DenoiseParamsC(*params)), dst, 0)
    return rc, N.lib().fh_last_error(None).decode()


def test_every_refusal_is_decided_before_the_context_is_touched():
    """a refused call returns before it looks at the context (here NULL: no GPU is needed); a call whose arguments are in order gets as far as the context check"""
    accepted = [dict(), dict(temporal=None), dict(params=None), dict(temporal=None, params=None), dict(temporal=(0.0, 1.0, 1.0, 1e-6)), dict(temporal=(1.0, 1e6, -0.999, 10.0)),
                dict(ptrs=FULL[:5] + [None, None])]
    for kw in accepted:
        rc, msg = _call(**kw)
        assert rc == FH_E_INVALID and msg == "fh_denoise_temporal: null context", (kw, msg)
    refused = [(dict(camera=None), "null camera"),
               (dict(ptrs=FULL[:3] + [None, None] + FULL[5:]), "position and depth layers are required"),
               (dict(ptrs=FULL[:3] + [None] + FULL[4:]), "position and depth are given together"), (dict(ptrs=FULL[:4] + [None] + FULL[5:]), "position and depth are given together"),
               (dict(ptrs=FULL[:5] + [None] + FULL[6:]), "moments and counts"), (dict(ptrs=FULL[:6] + [None]), "moments and counts"),
               (dict(camera=_camera(fov=0.0)), "fov"), (dict(camera=_camera(fov=float("nan"))), "fov"), (dict(camera=_camera(t00=0.0)), "inverted"),
               (dict(camera=_camera(t00=float("inf"))), "inverted"),
               (dict(dst=None), "null argument"), (dict(w=0), "width"), (dict(h=32769), "width")]
    for k in range(3):
        refused.append((dict(ptrs=[None if j == k else p for j, p in enumerate(FULL)]), "required"))
    bad = {0: ("alpha_min", (-0.1, 1.5, float("nan"), float("inf"))), 1: ("max_history", (0.5, 0.0, -3.0, float("nan"), float("inf"))),
           2: ("normal_cos_min", (-1.0, -2.0, 1.5, float("nan"))), 3: ("plane_tol", (0.0, -1.0, float("nan"), float("inf")))}
    for k, (word, values) in bad.items():
        for v in values:
            refused.append((dict(temporal=OK_T[:k] + (v,) + OK_T[k + 1:]), word))
    for v in (0.0, float("nan")):
        refused.append((dict(params=(v, 1.0, 0.2, 7, 5)), "sigma"))
    refused += [(dict(params=(2.0, 1.0, 0.2, 11, 5)), "normal_power_log2"), (dict(params=(2.0, 1.0, 0.2, 7, 0)), "passes"), (dict(params=(2.0, 1.0, 0.2, 7, 7)), "passes")]
    messages = set()
    for kw, word in refused:
        rc, msg = _call(**kw)
        assert rc == FH_E_INVALID and msg.startswith("fh_denoise_temporal: ") and word in msg and "null context" not in msg, (kw, msg)
        messages.add(msg)
    assert len(messages) >= 14  # null camera, missing pair, half pairs and each parameter have messages of their own
    L = N.lib()
    assert L.fh_denoise_temporal(None, 8, 8, None, None, None, None, 1 << 20, 0) == FH_E_INVALID and "null argument" in L.fh_last_error(None).decode()
    assert L.fh_denoise_history_reset(None) == FH_E_INVALID
    assert L.fh_denoise_history_info(None, None, None, None) == FH_E_INVALID


def test_host_check_program_passes(tmp_path):
    """the refusals, the camera inversion and the plan of a call as a stand-alone host program (the one the host sanitizers are run on); its inverse agrees with numpy's in double"""
    exe = tmp_path / "temporal_host_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", os.path.join(ROOT, "tools", "temporal_host_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "ok" in run.stdout, run.stdout
    # the plan of a call (temporal_call_plan, temporal_feed_plan): given the table, the program replays every row of it, and the table has rows for both functions
    cases = os.path.join(ROOT, "tests", "golden", "temporal_plan_cases.json")
    rows = json.load(open(cases))
    replayed = subprocess.run([str(exe), cases], capture_output=True, text=True)
    assert replayed.returncode == 0 and "temporal_host_check: ok (%d cases)" % len(rows) in replayed.stdout and len(rows) >= 300, replayed.stdout
    assert {r["fn"] for r in rows} == {"temporal_call_plan", "temporal_feed_plan"}
    # a table it cannot read, or one with one expected value flipped, fails and names the case
    assert subprocess.run([str(exe), str(tmp_path / "missing.json")], capture_output=True, text=True).returncode != 0
    for fn, col in (("temporal_call_plan", 4), ("temporal_call_plan", 2), ("temporal_feed_plan", 0)):
        k = max(i for i, r in enumerate(rows) if r["fn"] == fn)
        flipped = [dict(r, out=list(r["out"])) for r in rows]
        flipped[k]["out"][col] ^= 1
        bad = tmp_path / "bad.json"
        bad.write_text(json.dumps(flipped))
        r = subprocess.run([str(exe), str(bad)], capture_output=True, text=True)
        assert r.returncode != 0 and "temporal_host_check: 1 failures" in r.stdout and "FAILED case %d (%s)" % (k, fn) in r.stdout, r.stdout
    from fredholm_amd.renderer import look_at_transform
    t = look_at_transform((0.3, 1.1, 3.4), (0.2, -0.1, -1.0))
    out = subprocess.run([str(exe)] + [repr(float(v)) for v in t.reshape(12)] + ["1.0", "8.0", "100.0"], capture_output=True, text=True, check=True).stdout.split()
    got = np.array([float.fromhex(v) for v in out], np.float64).reshape(3, 4)
    m = np.eye(4)
    m[:3] = t.astype(np.float64)
    assert np.abs(got - np.linalg.inv(m)[:3]).max() <= 1e-6


def test_python_facade_has_the_methods_with_the_library_defaults():
    from fredholm_amd.renderer import Renderer
    d = {p.name: p.default for p in inspect.signature(Renderer.denoise_temporal).parameters.values()}
    assert [d[k] for k in ("alpha_min", "max_history", "normal_cos_min", "plane_tol")] == [0.2, 32.0, 0.5, 0.02]
    assert [d[k] for k in ("sigma_l", "sigma_z", "sigma_a", "normal_power_log2", "passes", "upscale")] == [2.0, 1.0, 0.2, 7, 5, False]
    assert d["moments_ptr"] is None and d["counts_ptr"] is None
    assert d["position_ptr"] is inspect.Parameter.empty and d["depth_ptr"] is inspect.Parameter.empty and d["camera"] is inspect.Parameter.empty
    assert callable(Renderer.reset_denoise_history) and callable(Renderer.denoise_history_info)


SOURCE = r"""
#include "fredholm/denoiser.h"
#include "fredholm/renderer.h"
#include <cstdio>
#include <cstring>
extern "C" int fh_denoise(fh_ctx*, uint32_t, uint32_t, const float*, const float*, const float*, float*, int) { std::printf("fh_denoise\n"); return FH_OK; }
extern "C" int fh_denoise_guided(fh_ctx*, uint32_t, uint32_t, const fh_denoise_inputs*, const fh_denoise_params*, float*, int) { std::printf("fh_denoise_guided\n"); return FH_OK; }
extern "C" int fh_denoise_temporal(fh_ctx*, uint32_t width, uint32_t height, const fh_denoise_inputs* in, const fh_camera* camera, const fh_temporal_params* temporal,
                                   const fh_denoise_params* params, float* denoised, int upscale2x)
{
  std::printf("fh_denoise_temporal %u %u %p %p %p %p %p %p %p %p %p %d cam %g %g %g %g", width, height, (const void*)in->beauty, (const void*)in->normal, (const void*)in->albedo,
              (const void*)in->position, (const void*)in->depth, (const void*)in->moments, (const void*)in->counts, (const void*)params, (void*)denoised, upscale2x,
              (double)camera->transform[3], (double)camera->transform[7], (double)camera->transform[11], (double)camera->fov);
  if (temporal) std::printf(" temporal %g %g %g %g", (double)temporal->alpha_min, (double)temporal->max_history, (double)temporal->normal_cos_min, (double)temporal->plane_tol);
  std::printf("\n");
  return FH_OK;
}
extern "C" int fh_denoise_history_reset(fh_ctx*) { std::printf("fh_denoise_history_reset\n"); return FH_OK; }
extern "C" int fh_render(fh_ctx*, const fh_camera*, const float*, const fh_render_layers*, uint32_t n_samples, uint32_t max_depth, uint32_t seed)
{
  std::printf("fh_render %u %u seed %u\n", n_samples, max_depth, seed);
  return FH_OK;
}
int main(int argc, char** argv)
{
  fh_ctx* ctx = reinterpret_cast<fh_ctx*>(0x10);  // never dereferenced: the entries are the ones above
  auto f4 = [](uintptr_t a) { return reinterpret_cast<const float4*>(a); };
  const char* what = argc > 1 ? argv[1] : "default";
  if (std::strcmp(what, "seed") == 0) {
    fredholm::Renderer renderer(ctx);
    fredholm::Camera camera(make_float3(1, 2, 3));
    fredholm::RenderLayer layer{};
    renderer.render(camera, make_float3(0, 0, 0), layer, 16, 5);
    renderer.set_seed(7);
    renderer.render(camera, make_float3(0, 0, 0), layer, 16, 5);
    const fh_camera c = renderer.camera_params(camera);
    std::printf("camera_params %g %g %g\n", (double)c.transform[3], (double)c.transform[7], (double)c.transform[11]);
    return 0;
  }
  fredholm::Denoiser denoiser(ctx, 64, 48, f4(0x100), f4(0x200), f4(0x300), f4(0x400), false);
  if (std::strcmp(what, "temporal") == 0) denoiser.set_mode(fredholm::Denoiser::Temporal);
  if (std::strcmp(what, "atrous") == 0) denoiser.set_mode(fredholm::Denoiser::Atrous);
  if (std::strcmp(what, "params") == 0) { denoiser.set_mode(fredholm::Denoiser::Temporal); denoiser.set_temporal_params(0.5f, 8.0f, 0.75f, 0.25f); }
  if (std::strcmp(what, "reset") == 0) { denoiser.reset_history(); return 0; }
  denoiser.set_guides(f4(0x500), reinterpret_cast<const float*>(0x600));
  if (std::strcmp(what, "nocamera") != 0) denoiser.set_camera(fredholm::Camera(make_float3(1, 2, 3), 0.5f));
  try { denoiser.denoise(); } catch (const std::exception& e) { std::printf("exception %s\n", e.what()); return 0; }
  return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("temporal_modes")
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
    return r.stdout.split()


NIL = "(nil)"
TEMPORAL = ["fh_denoise_temporal", "64", "48", "0x100", "0x200", "0x300", "0x500", "0x600", NIL, NIL, NIL, "0x400", "0", "cam", "1", "2", "3", "0.5"]


def test_temporal_mode_and_the_environment_variable_reach_the_new_entry(exe):
    assert _run(exe, "temporal") == TEMPORAL
    assert _run(exe, env={"FH_DENOISER": "temporal"}) == TEMPORAL
    assert _run(exe, "atrous", env={"FH_DENOISER": "temporal"})[0] == "fh_denoise"
    assert _run(exe)[0] == "fh_denoise" and _run(exe, env={"FH_DENOISER": "guided"})[0] == "fh_denoise_guided"
    assert _run(exe, "params") == TEMPORAL + ["temporal", "0.5", "8", "0.75", "0.25"]
    assert _run(exe, "reset") == ["fh_denoise_history_reset"]
    out = _run(exe, "nocamera", env={"FH_DENOISER": "temporal"})
    assert out[0] == "exception" and "set_camera" in " ".join(out)


def test_renderer_set_seed_reaches_fh_render_and_defaults_to_one(exe):
    assert _run(exe, "seed") == ["fh_render", "16", "5", "seed", "1", "fh_render", "16", "5", "seed", "7", "camera_params", "1", "2", "3"]


def test_rtcamp_knows_the_temporal_denoiser_and_still_refuses_others(tmp_path):
    rt = tmp_path / "rtcamp"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "rtcamp.cpp"), *LINK, "-lpthread", "-o", str(rt)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(rt), "--scene", "x.obj", "--denoiser", "bogus"], capture_output=True, text=True)
    assert run.returncode == 2 and "--denoiser" in run.stderr and "temporal" in run.stderr
    src = open(os.path.join(ROOT, "examples", "rtcamp.cpp")).read()
    assert 'denoiser_name != "temporal"' in src and "renderer.set_seed(1u + uint32_t(frame_idx))" in src
