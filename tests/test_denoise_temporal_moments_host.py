"""CPU tests of the temporal moments of the temporal stage (include/fredholm_hip.h: fh_set_denoise_temporal_moments; fredholm_amd/csrc/denoise.hip: k_temporal<., ., true>):
the restatement that the replay tool and the device tests share (tests/test_gpu_denoise_temporal_moments.py imports it from here) against a 3 x 2 frame computed by hand,
the exported symbols, the layout of fh_temporal_moments_params, the refusal -- decided from the argument alone -- and the facades
(fredholm::Denoiser::set_temporal_moments, FH_DENOISE_TEMPORAL_MOMENTS, the Python methods, rtcamp's flags).  The stage itself is tested on the GPU."""
import ctypes as C
import inspect
import json
import os
import subprocess

import numpy as np
import pytest

from fredholm_amd import native as N

import test_gpu_denoise_response as R
from test_gpu_denoise_response import T, TDEF, _hit, inv_tan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINK = ["-L" + os.path.join(ROOT, "fredholm_amd"), "-lfredholm_hip", "-Wl,-rpath," + os.path.join(ROOT, "fredholm_amd"), "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
FH_E_INVALID = -1
MIN_HISTORY = 2.0  # the library's default: the float64 replay's choice (profiles/denoise_temporal_moments_replay.json: default_min_history)


# ------------------------------------------------------------------ the restatement
def frame_moments(dt, c):
    """(l, l * l) of the preparation's colour c"""
    l = T._lum(c, dt)
    return np.stack([l, l * l], axis=-1).astype(dt)


def blend_moments(dt, have, c, v, mu_h, h_h, alpha_min, max_history, min_history, replace_v):
    """(mu_acc, v, long): the blended moments, the variance the blend of (c, v) is given -- the preparation's v, or, where replace_v (the call has no sample moments)
    and the pixel has a history of h >= min_history, fmax(mu_acc.y - mu_acc.x * mu_acc.x, 0) -- and which pixels took it.  h_h: the history length after the clip"""
    m = frame_moments(dt, c)
    with np.errstate(all="ignore"):
        hn = np.minimum(h_h + dt(1), dt(np.float32(max_history)))
        a = np.maximum(dt(1) / hn, dt(np.float32(alpha_min)))
        b = dt(1) - a
        mu_acc = np.where(have[..., None], b[..., None] * mu_h + a[..., None] * m, m).astype(dt)
        long = have & (hn >= dt(np.float32(min_history)))
        var = np.fmax(mu_acc[..., 1] - mu_acc[..., 0] * mu_acc[..., 0], dt(0))  # (C's fmax: a NaN difference gives 0)
        return mu_acc, (np.where(long, var, v) if replace_v else v).astype(dt), long


class MomentsRestatement(R.ResponseRestatement):
    """the response restatement (gamma None: the clip off) with the context's third switch: min_history None is off (the parent's calls), else
    fh_set_denoise_temporal_moments: every call keeps the moments, and a call without sample moments takes its variance from them"""

    min_history = None
    long = None

    def call_r(self, layers, cam15, ids=None, table=None, use_moments=True, upscale=False, temporal=None, sigma_l=2.0, sigma_z=1.0, sigma_a=0.2, normal_power_log2=7, passes=5):
        if self.min_history is None:
            self.long = None
            return super().call_r(layers, cam15, ids, table, use_moments, upscale, temporal, sigma_l, sigma_z, sigma_a, normal_power_log2, passes)
        moved = table is not None and bool(table[2].any())
        dt, tp, cam15 = self.dt, dict(TDEF, **(temporal or {})), np.asarray(cam15, np.float32)
        with np.errstate(all="ignore"):
            c, v, af = T.prepare(dt, layers["beauty"], layers["normal"], layers["albedo"], layers["moments"] if use_moments else None, layers["counts"] if use_moments else None,
                                 normal_power_log2)
            self.c_in, self.v_in = c, v
            hit = _hit(layers["normal"][..., :3])
            if self.hist is None or self.hist["v"].shape != v.shape:  # no history: the guided filter's (c, v), and the frame's moments
                self.reset()
                self.have, self.carried, self.u, self.n = np.zeros(v.shape, bool), np.zeros(v.shape, bool), None, None
                c_h, v_h, h_h, mu_h = np.zeros(c.shape, dt), np.zeros(v.shape, dt), np.zeros(v.shape, dt), np.zeros(v.shape + (2,), dt)
            else:
                args = (cam15, layers["normal"], layers["position"], layers["depth"], ids, table if moved else None, tp["normal_cos_min"], tp["plane_tol"])
                self.have, c_h, v_h, h_h, self.carried = R.lookup(dt, self.hist, *args)
                # the moments through the same look-up: the own tap, or the same valid taps, weights, order and division by S as the colour, per component
                as_colour = dict(self.hist, c=np.concatenate([self.hist["mu"], np.zeros(v.shape + (1,), dt)], axis=2))
                mu_h = R.lookup(dt, as_colour, *args)[1][..., :2]
                self.u = self.n = None
                if self.gamma is not None:  # the clip changes (c_h, v_h, h_h) and leaves the moments alone
                    c_h, v_h, h_h, self.u, self.n = R.clip_history(dt, c, layers["normal"], c_h, v_h, h_h, self.gamma, tp["normal_cos_min"])
            mu, v, self.long = blend_moments(dt, self.have, c, v, mu_h, h_h, tp["alpha_min"], tp["max_history"], self.min_history, not use_moments)
            c, v, h = R.blend(dt, self.have, hit, c, v, c_h, v_h, h_h, tp["alpha_min"], tp["max_history"])
            self.hist = dict(c=c, v=v, h=h, mu=mu, P=layers["position"][..., :3].astype(dt), N=layers["normal"][..., :3].astype(dt), cam=cam15.copy(),
                             m=T.world_to_camera(cam15[:12]), f=inv_tan(cam15[12]))
            self.frames += 1
            out = T.passes_of(dt, self.exp, c, v, af, layers["normal"], layers["albedo"], layers["position"], layers["depth"], sigma_l, sigma_z, sigma_a, normal_power_log2, passes, upscale)
        assert out.dtype == dt
        return out


def moments_restatements(oracle, gamma, min_history):
    r64, r32 = MomentsRestatement(np.float64, np.exp), MomentsRestatement(np.float32, lambda x: oracle.elementary("exp", x).reshape(x.shape))
    r64.gamma = r32.gamma = gamma
    r64.min_history = r32.min_history = min_history
    return r64, r32


def kinds(st, normal):
    """(pixels with a history of h >= min_history, with a shorter history, hit pixels without a history) of the restatement's last call"""
    hit = _hit(normal[..., :3])
    return int(st.long.sum()), int((st.have & ~st.long).sum()), int((hit & ~st.have).sum())


# ------------------------------------------------------------------ the restatement against a frame computed by hand
def test_moments_of_a_hand_computed_case():
    """3 x 2, a still camera, grey colours (lum of (x, x, x) is x up to the rounding of the three weights' sum, hence the tolerances), no sample moments, min_history 3,
    alpha_min 0.2.  Stored history: mu = (2, 5) everywhere, v_h = 0.5, c_h = 2.
      (0, 0): h_h = 3, c = 4: h = 4, a = 0.25, b = 0.75: mu_acc = (0.75 * 2 + 0.25 * 4, 0.75 * 5 + 0.25 * 16) = (2.5, 7.75); 4 >= 3: v = 7.75 - 6.25 = 1.5;
              v_acc = 0.5625 * 0.5 + 0.0625 * 1.5 = 0.375.
      (1, 0): h_h = 1, c = 4: h = 2, a = b = 0.5: mu_acc = (3, 10.5); 2 < 3: v stays the spatial estimate v_s: v_acc = 0.25 * 0.5 + 0.25 * v_s.
      (2, 0): the stored normal is a miss's: no history: mu_acc = (4, 16), v_acc = v_s, h = 1.
      (0, 1): a miss in the current frame: mu_acc = (l, l * l) of its colour 4, h = 0, and (c, v) pass through.
      (1, 1): h_h = 3 and mu = (3, 8): 0.75 * 8 + 4 = 10, (0.75 * 3 + 1)^2 = 10.5625: the difference is negative, v = fmax(-0.5625, 0) = 0: v_acc = 0.5625 * 0.5."""
    for dt in (np.float64, np.float32):
        tol = dict(rtol=1e-6)  # (float64: the three luminance weights, rounded to float32, sum to 1 + 1e-8)
        st = MomentsRestatement(dt, np.exp)
        st.min_history = 3.0
        nrm = np.zeros((2, 3, 4), np.float32)
        nrm[..., 2] = 1.0
        nrm[1, 0] = 0.0
        pos = np.zeros((2, 3, 4), np.float32)
        pos[..., 0], pos[..., 1], pos[..., 2] = np.arange(3)[None, :], np.arange(2)[:, None], -3.0
        lay = dict(beauty=np.full((2, 3, 4), 4.0, np.float32), albedo=np.ones((2, 3, 4), np.float32), normal=nrm, position=pos, depth=np.full((2, 3), 3.0, np.float32),
                   moments=None, counts=None)
        cam = np.asarray([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1.0, 8.0, 100.0], np.float32)
        hist_n = nrm[..., :3].astype(dt).copy()
        hist_n[0, 2] = 0.0
        hist_n[1, 0] = (0, 0, 1)
        h_h = np.asarray([[3, 1, 3], [3, 3, 3]], dt)
        mu = np.tile(np.asarray([2, 5], dt), (2, 3, 1))
        mu[1, 1] = (3, 8)
        st.hist = dict(c=np.full((2, 3, 3), dt(2)), v=np.full((2, 3), dt(0.5)), h=h_h, mu=mu, P=pos[..., :3].astype(dt), N=hist_n, cam=cam.copy(), m=T.world_to_camera(cam[:12]),
                       f=inv_tan(cam[12]))
        v_s = T.prepare(dt, lay["beauty"], lay["normal"], lay["albedo"], None, None, 7)[1]
        st.call_r(lay, cam, use_moments=False, passes=1)
        got = st.hist
        assert st.have.tolist() == [[True, True, False], [False, True, True]] and st.long.tolist() == [[True, False, False], [False, True, True]]
        assert kinds(st, nrm) == (3, 1, 1)
        assert np.allclose(got["mu"][0, 0], (2.5, 7.75), **tol) and np.isclose(got["v"][0, 0], 0.375, rtol=1e-5) and got["h"][0, 0] == 4
        assert np.allclose(got["mu"][0, 1], (3.0, 10.5), **tol) and np.isclose(got["v"][0, 1], 0.25 * 0.5 + 0.25 * float(v_s[0, 1]), **tol) and got["h"][0, 1] == 2
        assert np.allclose(got["mu"][0, 2], (4.0, 16.0), **tol) and got["v"][0, 2] == v_s[0, 2] and got["h"][0, 2] == 1
        assert np.allclose(got["mu"][1, 0], (4.0, 16.0), **tol) and got["v"][1, 0] == v_s[1, 0] and got["h"][1, 0] == 0
        assert np.allclose(got["mu"][1, 1], (3.25, 10.0), **tol) and np.isclose(got["v"][1, 1], 0.5625 * 0.5, **tol) and got["h"][1, 1] == 4
        # the same call WITH sample moments keeps the moments and leaves v alone
        st.hist = dict(got, h=h_h, mu=mu, c=np.full((2, 3, 3), dt(2)), v=np.full((2, 3), dt(0.5)), N=hist_n)
        lay2 = dict(lay, moments=np.tile(np.asarray([4.0, 17.0], np.float32), (2, 3, 1)), counts=np.full((2, 3), 5, np.uint32))
        v_m = T.prepare(dt, lay2["beauty"], lay2["normal"], lay2["albedo"], lay2["moments"], lay2["counts"], 7)[1]
        st.call_r(lay2, cam, use_moments=True, passes=1)
        assert np.allclose(st.hist["mu"][0, 0], (2.5, 7.75), **tol) and np.isclose(st.hist["v"][0, 0], 0.5625 * 0.5 + 0.0625 * float(v_m[0, 0]), **tol) and np.isclose(v_m[0, 0], 0.25, **tol)


def test_the_switched_off_restatement_is_the_response_restatement(oracle):
    """min_history None: the parent's bits, clip off and on, with and without sample moments; and with the switch on a call WITH sample moments has them too, as has
    every call under a min_history no history reaches"""
    calls = R.response_case("5x3", "moved") + R.response_case("5x3", "carried-still")[1:]
    for gamma in (None, R.GAMMA):
        for use_moments in (True, False):
            for min_history in (None, 2.0, 1e30):
                if min_history == 2.0 and not use_moments:
                    continue
                mine, parent = moments_restatements(oracle, gamma, min_history)[1], R.response_restatements(oracle, gamma)[1]
                for call in calls:
                    assert R._bits(R._restate(mine, call, use_moments=use_moments, passes=1), R._restate(parent, call, use_moments=use_moments, passes=1))
                    assert np.array_equal(mine.have, parent.have) and R._bits(mine.hist["h"], parent.hist["h"])
                    assert (mine.long is None) == (min_history is None)


# ------------------------------------------------------------------ the interface
def test_symbols_struct_and_header_agree(tmp_path):
    L = N.load_library()
    want = {"fh_set_denoise_temporal_moments": [C.c_void_p, C.POINTER(N.TemporalMomentsParamsC)],
            "fh_get_denoise_temporal_moments": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(N.TemporalMomentsParamsC)]}
    for name, sig in want.items():
        assert name in N.EXPORTS
        fn = getattr(L, name)
        assert fn.restype is C.c_int and fn.argtypes == N.SIGNATURES[name] == sig, name
    hdr = " ".join(open(os.path.join(ROOT, "include", "fredholm_hip.h")).read().split())
    assert "typedef struct fh_temporal_moments_params { float min_history;" in hdr
    assert "int fh_set_denoise_temporal_moments(fh_ctx* ctx, const fh_temporal_moments_params* params);" in hdr
    assert "int fh_get_denoise_temporal_moments(fh_ctx* ctx, int* on, fh_temporal_moments_params* params);" in hdr
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fredholm_hip.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(fh_temporal_moments_params), '
                   'offsetof(fh_temporal_moments_params, min_history), sizeof(fh_response_noise_params), sizeof(fh_response_params)); return 0; }\n')
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(N.TemporalMomentsParamsC), N.TemporalMomentsParamsC.min_history.offset, 4, 4] == [4, 0, 4, 4]


def test_a_bad_min_history_is_refused_before_the_context_is_looked_at():
    """with a NULL context: a bad min_history is refused with its own message, a good one and NULL (off) get as far as the context check"""
    L = N.lib()
    for bad in (float("nan"), float("inf"), -float("inf"), 0.5, -1.0, 0.0, 0.99999994):
        assert L.fh_set_denoise_temporal_moments(None, C.byref(N.TemporalMomentsParamsC(bad))) == FH_E_INVALID
        msg = L.fh_last_error(None).decode()
        assert msg == "fh_set_denoise_temporal_moments: min_history must be finite and >= 1", (bad, msg)
    assert L.fh_set_denoise_response_noise(None, C.byref(N.ResponseNoiseParamsC(0.0))) == FH_E_INVALID  # (another message, so that the next calls are seen not to be refusals)
    for good in (1.0, 4.0, 1e30, 3.0e38):
        assert L.fh_set_denoise_temporal_moments(None, C.byref(N.TemporalMomentsParamsC(good))) == FH_E_INVALID
        assert "min_history" not in L.fh_last_error(None).decode()
    assert L.fh_set_denoise_temporal_moments(None, None) == FH_E_INVALID
    on = C.c_int(0)
    assert L.fh_get_denoise_temporal_moments(None, C.byref(on), None) == FH_E_INVALID and L.fh_get_denoise_temporal_moments(None, None, None) == FH_E_INVALID


def test_the_default_min_history_is_the_replays_choice_in_every_facade():
    from fredholm_amd.renderer import Renderer
    with open(os.path.join(ROOT, "profiles", "denoise_temporal_moments_replay.json")) as f:
        rec = json.loads(f.readline())
    assert rec["default_min_history"] == MIN_HISTORY
    # the rule, recomputed from the record: the smallest sum over the four clip-off steady sequences of relMSE / the spatial-estimate call's relMSE; ties to the smaller
    sums = {float(m): sum(rec["steady"][name][f"min_history={m}"] / rec["steady"][name]["spatial"] for name in ("moving_16spp", "moving_4spp", "moving_1spp", "still_1spp"))
            for m in rec["min_histories"]}
    assert sorted(sums) == [2.0, 3.0, 4.0, 6.0] and min(sorted(sums), key=lambda m: sums[m]) == MIN_HISTORY, sums
    assert inspect.signature(Renderer.set_denoise_temporal_moments).parameters["min_history"].default == MIN_HISTORY
    assert callable(Renderer.clear_denoise_temporal_moments) and callable(Renderer.get_denoise_temporal_moments)
    text = f"{MIN_HISTORY:g}"
    assert f"finite and >= 1; default {text} */" in open(os.path.join(ROOT, "include", "fredholm_hip.h")).read()
    assert f"void set_temporal_moments(bool on, float min_history = {text}.0f)" in open(os.path.join(ROOT, "include", "fredholm", "denoiser.h")).read()
    assert f"float moments_min_history = {text}.0f;" in open(os.path.join(ROOT, "fredholm_amd", "csrc", "context.h")).read()
    assert f"float denoise_min_history = {text}.0f;" in open(os.path.join(ROOT, "examples", "rtcamp.cpp")).read()


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
extern "C" int fh_set_denoise_temporal_moments(fh_ctx*, const fh_temporal_moments_params* params)
{
  if (params) std::printf("fh_set_denoise_temporal_moments %g\n", (double)params->min_history);
  else std::printf("fh_set_denoise_temporal_moments off\n");
  return FH_OK;
}
int main(int argc, char** argv)
{
  fh_ctx* ctx = reinterpret_cast<fh_ctx*>(0x10);  // never dereferenced: the entries are the ones above
  auto f4 = [](uintptr_t a) { return reinterpret_cast<const float4*>(a); };
  const char* what = argc > 1 ? argv[1] : "default";
  fredholm::Denoiser denoiser(ctx, 64, 48, f4(0x100), f4(0x200), f4(0x300), f4(0x400), false);
  if (std::strcmp(what, "on") == 0) { denoiser.set_mode(fredholm::Denoiser::Temporal); denoiser.set_temporal_moments(true); }
  if (std::strcmp(what, "six") == 0) { denoiser.set_mode(fredholm::Denoiser::Temporal); denoiser.set_temporal_moments(true, 6.0f); }
  if (std::strcmp(what, "off") == 0) { denoiser.set_mode(fredholm::Denoiser::Temporal); denoiser.set_temporal_moments(false); }
  if (std::strcmp(what, "temporal") == 0) denoiser.set_mode(fredholm::Denoiser::Temporal);
  if (std::strcmp(what, "atrous") == 0) { denoiser.set_mode(fredholm::Denoiser::Atrous); denoiser.set_temporal_moments(true); }
  denoiser.set_guides(f4(0x500), reinterpret_cast<const float*>(0x600));
  denoiser.set_camera(fredholm::Camera(make_float3(1, 2, 3), 0.5f));
  denoiser.denoise();
  denoiser.denoise();  // (the switches are sent once)
  std::printf("moments %d %g\n", denoiser.temporal_moments() ? 1 : 0, (double)denoiser.temporal_moments_min_history());
  return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("temporal_moments_modes")
    src = d / "modes.cpp"
    src.write_text(SOURCE)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), *LINK, "-o", str(d / "modes")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(d / "modes")


def _run(exe, *args, env=None):
    e = {k: v for k, v in os.environ.items() if k not in ("FH_DENOISER", "FH_DENOISE_TEMPORAL_MOMENTS")}
    e.update(env or {})
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=e)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def test_set_temporal_moments_and_the_environment_variable_reach_the_entry_point(exe):
    twice = ["fh_denoise_temporal", "fh_denoise_temporal"]
    d = f"{MIN_HISTORY:g}"
    assert _run(exe, "on") == [f"fh_set_denoise_temporal_moments {d}"] + twice + [f"moments 1 {d}"]
    assert _run(exe, "six") == ["fh_set_denoise_temporal_moments 6"] + twice + ["moments 1 6"]
    assert _run(exe, "off") == ["fh_set_denoise_temporal_moments off"] + twice + [f"moments 0 {d}"]
    assert _run(exe, "temporal") == twice + [f"moments 0 {d}"]  # (never set: the entry point is not called)
    assert _run(exe, "atrous") == ["fh_denoise", "fh_denoise", f"moments 1 {d}"]  # (the switch belongs to the Temporal mode)
    on = {"FH_DENOISE_TEMPORAL_MOMENTS": "1"}
    assert _run(exe, env=dict(on, FH_DENOISER="temporal")) == [f"fh_set_denoise_temporal_moments {d}"] + twice + [f"moments 1 {d}"]
    assert _run(exe, env=dict(on, FH_DENOISER="temporal-motion-response")) == ["fh_set_denoise_motion 1", "fh_set_denoise_response 1", f"fh_set_denoise_temporal_moments {d}"] + twice + [f"moments 1 {d}"]
    assert _run(exe, "temporal", env={"FH_DENOISE_TEMPORAL_MOMENTS": "2.5"}) == ["fh_set_denoise_temporal_moments 2.5"] + twice + ["moments 1 2.5"]
    assert _run(exe, "temporal", env={"FH_DENOISE_TEMPORAL_MOMENTS": "0"}) == twice + [f"moments 0 {d}"]
    assert _run(exe, env=on) == ["fh_denoise", "fh_denoise", f"moments 1 {d}"]  # (FH_DENOISER gets no new value: the variable alone does not choose the mode)


def test_rtcamp_knows_the_two_flags(tmp_path):
    rt = tmp_path / "rtcamp"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "rtcamp.cpp"), *LINK, "-lpthread", "-o", str(rt)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    usage = subprocess.run([str(rt)], capture_output=True, text=True)
    assert usage.returncode == 2 and "--denoise-temporal-moments" in usage.stderr and "--denoise-min-history" in usage.stderr
    for name in ("atrous", "guided"):
        run = subprocess.run([str(rt), "--scene", "x.obj", "--denoiser", name, "--denoise-temporal-moments"], capture_output=True, text=True)
        assert run.returncode == 2 and "--denoise-temporal-moments" in run.stderr and "temporal" in run.stderr
    for bad in ("0", "0.5", "-1", "nan", "inf"):
        run = subprocess.run([str(rt), "--scene", "x.obj", "--denoiser", "temporal", "--denoise-temporal-moments", "--denoise-min-history", bad], capture_output=True, text=True)
        assert run.returncode == 2 and "--denoise-min-history" in run.stderr, (bad, run.stderr)
    run = subprocess.run([str(rt), "--scene", "x.obj", "--denoiser", "temporal-response", "--denoise-min-history", "3"], capture_output=True, text=True)
    assert run.returncode == 2 and "--denoise-min-history" in run.stderr and "--denoise-temporal-moments" in run.stderr  # (a value no switch would use is refused, not ignored)
    header = open(os.path.join(ROOT, "examples", "rtcamp.cpp")).read().split("#include")[0]
    assert "--denoise-temporal-moments [--denoise-min-history H]" in header
