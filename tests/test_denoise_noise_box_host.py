"""CPU tests of the noise box of the temporal stage's history clipping (include/fredholm_hip.h: fh_set_denoise_response_noise, step 4b): the restatement the replay
tool and the device tests share (tests/test_gpu_denoise_noise_box.py imports it from here) against a 5 x 3 frame computed by hand, the rules for non-finite
half-widths, the exported symbols, the layout of fh_response_noise_params, the refusal -- decided from the argument alone -- and the facades
(fredholm::Denoiser::set_response_noise, FH_DENOISER, the Python methods, rtcamp's flags).  The stage itself is tested on the GPU."""
import ctypes as C
import inspect
import json
import math
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
KAPPA = 6.0  # the library's default: the float64 replay's choice (profiles/denoise_noise_box_replay.json: default_kappa)


# ------------------------------------------------------------------ the restatement
def noise_box(dt, c, v, cc, u_s, v_h, kappa):
    """step 4b of the header: (cd, u, w) from the current frame's (c, v), the clipped history cc with its excess u_s, and the history variance as looked up.
    fmax and fmin with C semantics (a NaN operand loses); w is the noise box's own excess, u the larger of the two"""
    with np.errstate(all="ignore"):
        s = (dt(np.float32(kappa)) * np.sqrt(v + v_h)).astype(dt)
        cd = np.fmin(np.fmax(cc, c - s[..., None]), c + s[..., None])
        wk = np.abs(cd - cc) / (s + dt(np.float32(1e-6)))[..., None]
        w = np.fmax(np.fmax(wk[..., 0], wk[..., 1]), wk[..., 2])
        return cd.astype(dt), np.fmax(u_s, w).astype(dt), w.astype(dt)


def clip_history_noise(dt, c, v, normal, c_h, v_h, h_h, gamma, kappa, normal_cos_min):
    """steps 1 to 4, 4b and 5: (cd, v_h', h_h', u, u_s, w, n)"""
    cc, _, _, u_s, n = R.clip_history(dt, c, normal, c_h, v_h, h_h, gamma, normal_cos_min)
    cd, u, w = noise_box(dt, c, v, cc, u_s, v_h, kappa)
    with np.errstate(all="ignore"):
        k1 = dt(1) + u
        return cd, (v_h * k1).astype(dt), (h_h / k1).astype(dt), u, u_s, w, n


class NoiseBoxRestatement(R.ResponseRestatement):
    """the response restatement with the context's second switch: kappa None is off (the parent's calls).  Like the device, the step runs only while gamma is set
    and the call has moments; without_moments = True (the replay's rows that justify this; the device never does it) runs it on the 7 x 7 spatial variance too"""

    kappa = u_s = w = None
    without_moments = False

    def call_r(self, layers, cam15, ids=None, table=None, use_moments=True, upscale=False, temporal=None, sigma_l=2.0, sigma_z=1.0, sigma_a=0.2, normal_power_log2=7, passes=5):
        inert = self.kappa is None or self.gamma is None or not (use_moments or self.without_moments)
        if inert or self.hist is None or self.hist["v"].shape != layers["depth"].shape:
            self.u_s = self.w = None
            return super().call_r(layers, cam15, ids, table, use_moments, upscale, temporal, sigma_l, sigma_z, sigma_a, normal_power_log2, passes)
        moved = table is not None and bool(table[2].any())
        dt, tp, cam15 = self.dt, dict(TDEF, **(temporal or {})), np.asarray(cam15, np.float32)
        with np.errstate(all="ignore"):
            c, v, af = T.prepare(dt, layers["beauty"], layers["normal"], layers["albedo"], layers["moments"] if use_moments else None, layers["counts"] if use_moments else None,
                                 normal_power_log2)
            self.c_in, self.v_in = c, v
            self.have, c_h, v_h, h_h, self.carried = R.lookup(dt, self.hist, cam15, layers["normal"], layers["position"], layers["depth"], ids, table if moved else None,
                                                              tp["normal_cos_min"], tp["plane_tol"])
            cd, v_h, h_h, self.u, self.u_s, self.w, self.n = clip_history_noise(dt, c, v, layers["normal"], c_h, v_h, h_h, self.gamma, self.kappa, tp["normal_cos_min"])
            c, v, h = R.blend(dt, self.have, _hit(layers["normal"][..., :3]), c, v, cd, v_h, h_h, tp["alpha_min"], tp["max_history"])
            self.hist = dict(c=c, v=v, h=h, P=layers["position"][..., :3].astype(dt), N=layers["normal"][..., :3].astype(dt), cam=cam15.copy(), m=T.world_to_camera(cam15[:12]),
                             f=inv_tan(cam15[12]))
            self.frames += 1
            out = T.passes_of(dt, self.exp, c, v, af, layers["normal"], layers["albedo"], layers["position"], layers["depth"], sigma_l, sigma_z, sigma_a, normal_power_log2, passes, upscale)
        assert out.dtype == dt
        return out


def noise_restatements(oracle, gamma, kappa):
    r64, r32 = NoiseBoxRestatement(np.float64, np.exp), NoiseBoxRestatement(np.float32, lambda x: oracle.elementary("exp", x).reshape(x.shape))
    r64.gamma = r32.gamma = gamma
    r64.kappa = r32.kappa = kappa
    return r64, r32


def noise_counts(st):
    """(pixels the noise box clips, pixels it leaves alone) among the pixels of the restatement's last call that have a history"""
    if st.w is None:
        return 0, 0
    return int((st.w[st.have] > 0).sum()), int((st.w[st.have] == 0).sum())


# ------------------------------------------------------------------ the restatement against a frame computed by hand
def _frame(dt):
    """5 x 3, every row 2 2 4 6 6 in all three channels, every normal (0, 0, 1): a window is the columns x - 2 .. x + 2 of all three rows"""
    c = np.repeat(np.tile(np.asarray([2, 2, 4, 6, 6], dt), (3, 1))[..., None], 3, axis=2)
    nrm = np.zeros((3, 5, 4), np.float32)
    nrm[..., 2] = 1.0
    return c, nrm


def test_noise_box_of_a_hand_computed_case():
    """gamma 1, kappa 2, middle row.  Centre (2, 1), c = 4: its window is the frame, n = 15, mu = 60 / 15 = 4, var = (6 * 4 + 6 * 4) / 15 = 3.2, sd = 1.78885, the spatial
    box [2.21115, 5.78885]; v = 0.01, v_h = 0.03: s = 2 * sqrt(0.04) = 0.4, the noise box [3.6, 4.4].
      red, c_h = 5: inside the spatial box (u_r = 0), clipped by the noise box to 4.4, w_r = 0.6 / (0.4 + 1e-6);
      green, c_h = 8: the spatial box clips to 5.78885, u_g = 2.21115 / (1.78885 + 1e-6) = 1.23607; the noise box to 4.4, w_g = 1.38885 / (0.4 + 1e-6) = 3.47213;
      blue, c_h = 4.2: inside both.  u_s = u_g, w = w_g, u = w_g (the noise box's is the larger): h_h 8 becomes 8 / (1 + w_g), v_h becomes 0.03 * (1 + w_g).
    (1, 1), c = 2: columns 0 .. 3, n = 12, mu = 42 / 12 = 3.5, var = 180 / 12 - 12.25 = 2.75, sd = 1.65831, the spatial box [1.84169, 5.15831]; v = 0.09,
    v_h = 0.16: s = 2 * 0.5 = 1, the noise box [1, 3].  c_h = 50 in all channels: the spatial box clips to 5.15831, u_s = 44.84169 / (1.65831 + 1e-6) = 27.0405; the
    noise box to 3, w = 2.15831 / (1 + 1e-6); u = u_s (the spatial box's is the larger).
    (0, 1), c = 2: columns 0 .. 2, n = 9, mu = 24 / 9, var = 72 / 9 - 64 / 9 = 8 / 9, sd = 0.942809, the spatial box [1.72386, 3.60948]; v = 1, v_h = 3: s = 4,
    the noise box [-2, 6].  c_h = 7: the spatial box clips to 3.60948, which the noise box leaves alone: w = 0, u = u_s = 3.39052 / (0.942809 + 1e-6)."""
    for dt in (np.float64, np.float32):
        tol = dict(rtol=2e-6 if dt is np.float32 else 1e-12)
        c, nrm = _frame(dt)
        c_h = np.full((3, 5, 3), dt(3.0))
        c_h[1, 2] = (5.0, 8.0, 4.2)
        c_h[1, 1] = 50.0
        c_h[1, 0] = 7.0
        v, v_h = np.full((3, 5), dt(0.01)), np.full((3, 5), dt(0.03))
        v[1, 1], v_h[1, 1] = 0.09, 0.16
        v[1, 0], v_h[1, 0] = 1.0, 3.0
        h_h = np.full((3, 5), dt(8.0))
        cd, v2, h2, u, u_s, w, n = clip_history_noise(dt, c, v, nrm, c_h, v_h, h_h, 1.0, 2.0, 0.5)
        assert n[1, 2] == 15 and n[1, 1] == 12 and n[1, 0] == 9
        e6 = float(np.float32(1e-6))
        s = 2.0 * math.sqrt(float(dt(0.01)) + float(dt(0.03)))
        sd, hi = math.sqrt(3.2), 4.0 + math.sqrt(3.2)
        u_g, w_r, w_g = (8.0 - hi) / (sd + e6), (5.0 - (4.0 + s)) / (s + e6), (hi - (4.0 + s)) / (s + e6)
        assert np.allclose(cd[1, 2], (4.0 + s, 4.0 + s, 4.2), **tol)
        assert np.isclose(u_s[1, 2], u_g, **tol) and np.isclose(w[1, 2], w_g, **tol) and w_g > w_r > u_g > 0 and u[1, 2] == w[1, 2]
        assert np.isclose(h2[1, 2], 8.0 / (1.0 + w_g), **tol) and np.isclose(v2[1, 2], float(dt(0.03)) * (1.0 + w_g), **tol)
        sd, hi = math.sqrt(2.75), 3.5 + math.sqrt(2.75)
        assert np.allclose(cd[1, 1], 3.0, **tol) and np.isclose(u_s[1, 1], (50.0 - hi) / (sd + e6), **tol) and np.isclose(w[1, 1], (hi - 3.0) / (1.0 + e6), rtol=1e-5)
        assert u[1, 1] == u_s[1, 1] > w[1, 1] > 0
        sd, hi = math.sqrt(8.0 / 9.0), 24.0 / 9.0 + math.sqrt(8.0 / 9.0)
        assert np.allclose(cd[1, 0], hi, **tol) and w[1, 0] == 0 and u[1, 0] == u_s[1, 0] and np.isclose(u_s[1, 0], (7.0 - hi) / (sd + e6), rtol=1e-5)
        # a history inside both boxes keeps its bits, and so do h_h and v_h
        c_h[...] = c + dt(0.125)
        cd, v2, h2, u, u_s, w, n = clip_history_noise(dt, c, v, nrm, c_h, v_h, h_h, 1.0, 2.0, 0.5)
        assert (u[1] == 0).all() and (cd[1] == c_h[1]).all() and (h2[1] == 8).all() and (v2[1] == v_h[1]).all()


def test_too_few_taps_still_meet_the_noise_box():
    """step 3: the 5 x 3 frame with the centre's neighbours made misses as the response suite's _alone does: n = 1, cc = c_h and u_s = 0 whatever the history -- and
    step 4b still clamps it: c = 4, s = 0.4, c_h = (5, 8, 4.2) becomes (4.4, 4.4, 4.2), u = w = 3.6 / (0.4 + 1e-6)"""
    for dt in (np.float64, np.float32):
        c, nrm = _frame(dt)
        lay = R._alone(dict(normal=nrm, position=np.ones((3, 5, 4), np.float32), depth=np.ones((3, 5), np.float32)), 2, 1)
        assert (lay["normal"][1, 2, :3] == (0, 0, 1)).all() and np.count_nonzero(_hit(lay["normal"][..., :3])) == 1
        c_h = np.full((3, 5, 3), dt(3.0))
        c_h[1, 2] = (5.0, 8.0, 4.2)
        v, v_h, h_h = np.full((3, 5), dt(0.01)), np.full((3, 5), dt(0.03)), np.full((3, 5), dt(8.0))
        cc, _, h_s, u_only, n = R.clip_history(dt, c, lay["normal"], c_h, v_h, h_h, 1.0, 0.5)
        assert n[1, 2] == 1 and u_only[1, 2] == 0 and (cc[1, 2] == c_h[1, 2]).all() and h_s[1, 2] == 8
        cd, v2, h2, u, u_s, w, n = clip_history_noise(dt, c, v, lay["normal"], c_h, v_h, h_h, 1.0, 2.0, 0.5)
        s = 2.0 * math.sqrt(float(dt(0.01)) + float(dt(0.03)))
        want = (8.0 - (4.0 + s)) / (s + float(np.float32(1e-6)))
        assert n[1, 2] == 1 and u_s[1, 2] == 0
        assert np.allclose(cd[1, 2], (4.0 + s, 4.0 + s, 4.2), rtol=2e-6) and np.isclose(u[1, 2], want, rtol=2e-6) and u[1, 2] == w[1, 2]
        assert np.isclose(h2[1, 2], 8.0 / (1.0 + want), rtol=2e-6)


def test_non_finite_half_widths():
    """step 6b of the header, float32 (one pixel each): a NaN s clips nothing and leaves u_s; an infinite s -- an infinite variance, v + v_h past FLT_MAX,
    kappa * sqrt past FLT_MAX -- clips nothing; s = 0 makes the box the point c; a NaN history becomes c - s and its NaN excess loses"""
    f = np.float32
    c, cc, u_s = np.full((1, 1, 3), f(4.0)), np.asarray([[[5.0, 8.0, -100.0]]], f), np.full((1, 1), f(0.25))

    def run(v, v_h, kappa=2.0, cc=cc):
        return noise_box(f, c, np.full((1, 1), f(v)), cc, u_s, np.full((1, 1), f(v_h)), kappa)
    for v, v_h, kappa in ((np.nan, 0.03, 2.0), (0.01, np.nan, 2.0), (np.inf, 0.03, 2.0), (0.01, np.inf, 2.0), (3e38, 3e38, 2.0), (1e20, 0.0, 1e30), (-1.0, 0.0, 2.0)):
        cd, u, w = run(v, v_h, kappa)
        assert (cd.view(np.uint32) == cc.view(np.uint32)).all() and u[0, 0] == f(0.25), (v, v_h, kappa)
        assert np.isnan(w[0, 0]) if (np.isnan(v) or np.isnan(v_h) or v < 0) else w[0, 0] == 0, (v, v_h, kappa)
    with np.errstate(over="ignore"):
        assert np.isinf(f(3e38) + f(3e38)) and np.isinf(f(1e30) * np.sqrt(f(1e20)))
    cd, u, w = run(0.0, 0.0)
    assert (cd == 4).all() and np.isclose(w[0, 0], 104.0 / 1e-6, rtol=1e-5) and u[0, 0] == w[0, 0]
    nan_cc = np.asarray([[[np.nan, 4.1, 4.0]]], f)
    cd, u, w = run(0.01, 0.03, cc=nan_cc)
    assert cd[0, 0, 0] == f(4.0) - f(2.0) * np.sqrt(f(0.01) + f(0.03)) and (cd[0, 0, 1:] == nan_cc[0, 0, 1:]).all() and u[0, 0] == f(0.25)
    # C's fmin drops a NaN where numpy's minimum returns it
    assert np.fmin(f(np.nan), f(1)) == 1 and np.isnan(np.minimum(f(np.nan), f(1)))


def test_the_switched_off_restatement_is_the_response_restatement(oracle):
    """kappa None, gamma None with a kappa (stored, inert), and a call without moments: the parent's bits"""
    calls = R.response_case("5x3", "moved")
    for gamma, kappa, use_moments in ((R.GAMMA, None, True), (None, KAPPA, True), (R.GAMMA, KAPPA, False)):
        mine, parent = noise_restatements(oracle, gamma, kappa)[1], R.response_restatements(oracle, gamma)[1]
        for call in calls:
            assert R._bits(R._restate(mine, call, use_moments=use_moments, passes=1), R._restate(parent, call, use_moments=use_moments, passes=1))
            assert mine.w is None


# ------------------------------------------------------------------ the interface
def test_symbols_struct_and_header_agree(tmp_path):
    L = N.load_library()
    want = {"fh_set_denoise_response_noise": [C.c_void_p, C.POINTER(N.ResponseNoiseParamsC)],
            "fh_get_denoise_response_noise": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(N.ResponseNoiseParamsC)]}
    for name, sig in want.items():
        assert name in N.EXPORTS
        fn = getattr(L, name)
        assert fn.restype is C.c_int and fn.argtypes == N.SIGNATURES[name] == sig, name
    hdr = " ".join(open(os.path.join(ROOT, "include", "fredholm_hip.h")).read().split())
    assert "int fh_set_denoise_response_noise(fh_ctx* ctx, const fh_response_noise_params* params);" in hdr
    assert "int fh_get_denoise_response_noise(fh_ctx* ctx, int* on, fh_response_noise_params* params);" in hdr
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fredholm_hip.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(fh_response_noise_params), '
                   'offsetof(fh_response_noise_params, kappa), sizeof(fh_response_params), offsetof(fh_response_params, gamma)); return 0; }\n')
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(N.ResponseNoiseParamsC), N.ResponseNoiseParamsC.kappa.offset, 4, 0] == [4, 0, 4, 0]  # (fh_response_params keeps its layout)


def test_a_bad_kappa_is_refused_before_the_context_is_looked_at():
    """with a NULL context: a bad kappa is refused with its own message, a good one and NULL (off) get as far as the context check"""
    L = N.lib()
    for bad in (0.0, -1.0, -0.0, float("nan"), float("inf"), -float("inf")):
        assert L.fh_set_denoise_response_noise(None, C.byref(N.ResponseNoiseParamsC(bad))) == FH_E_INVALID
        msg = L.fh_last_error(None).decode()
        assert msg == "fh_set_denoise_response_noise: kappa must be finite and > 0", (bad, msg)
    L.fh_denoise_history_reset(None)
    for good in (6.0, 1e-6, 1e30):
        assert L.fh_set_denoise_response_noise(None, C.byref(N.ResponseNoiseParamsC(good))) == FH_E_INVALID
    assert L.fh_set_denoise_response_noise(None, None) == FH_E_INVALID
    on = C.c_int(0)
    assert L.fh_get_denoise_response_noise(None, C.byref(on), None) == FH_E_INVALID and L.fh_get_denoise_response_noise(None, None, None) == FH_E_INVALID


def test_the_default_kappa_is_the_replays_choice_in_every_facade():
    from fredholm_amd.renderer import Renderer
    with open(os.path.join(ROOT, "profiles", "denoise_noise_box_replay.json")) as f:
        rec = json.loads(f.readline())
    assert rec["default_kappa"] == KAPPA
    assert inspect.signature(Renderer.set_denoise_response_noise).parameters["kappa"].default == KAPPA
    assert callable(Renderer.clear_denoise_response_noise) and callable(Renderer.get_denoise_response_noise)
    hdr = open(os.path.join(ROOT, "include", "fredholm", "denoiser.h")).read()
    assert "void set_response_noise(bool on, float kappa = 6.0f)" in hdr
    assert "float response_kappa = 6.0f;" in open(os.path.join(ROOT, "fredholm_amd", "csrc", "context.h")).read()
    assert "float denoise_kappa = 6.0f;" in open(os.path.join(ROOT, "examples", "rtcamp.cpp")).read()


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
extern "C" int fh_set_denoise_response_noise(fh_ctx*, const fh_response_noise_params* params)
{
  if (params) std::printf("fh_set_denoise_response_noise %g\n", (double)params->kappa);
  else std::printf("fh_set_denoise_response_noise off\n");
  return FH_OK;
}
int main(int argc, char** argv)
{
  fh_ctx* ctx = reinterpret_cast<fh_ctx*>(0x10);  // never dereferenced: the entries are the ones above
  auto f4 = [](uintptr_t a) { return reinterpret_cast<const float4*>(a); };
  const char* what = argc > 1 ? argv[1] : "default";
  fredholm::Denoiser denoiser(ctx, 64, 48, f4(0x100), f4(0x200), f4(0x300), f4(0x400), false);
  if (std::strcmp(what, "on") == 0) { denoiser.set_mode(fredholm::Denoiser::Temporal); denoiser.set_response(true); denoiser.set_response_noise(true); }
  if (std::strcmp(what, "kappa") == 0) { denoiser.set_mode(fredholm::Denoiser::Temporal); denoiser.set_response(true); denoiser.set_response_noise(true, 4.5f); }
  if (std::strcmp(what, "off") == 0) { denoiser.set_mode(fredholm::Denoiser::Temporal); denoiser.set_response_noise(false); }
  if (std::strcmp(what, "alone") == 0) { denoiser.set_mode(fredholm::Denoiser::Temporal); denoiser.set_response_noise(true); }
  if (std::strcmp(what, "atrous") == 0) { denoiser.set_mode(fredholm::Denoiser::Atrous); denoiser.set_response_noise(true); }
  denoiser.set_guides(f4(0x500), reinterpret_cast<const float*>(0x600));
  denoiser.set_camera(fredholm::Camera(make_float3(1, 2, 3), 0.5f));
  denoiser.denoise();
  denoiser.denoise();  // (the switches are sent once)
  std::printf("noise %d %g\n", denoiser.response_noise() ? 1 : 0, (double)denoiser.response_noise_kappa());
  return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("noise_box_modes")
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


def test_set_response_noise_and_the_environment_variable_reach_the_entry_point(exe):
    twice = ["fh_denoise_temporal", "fh_denoise_temporal"]
    assert _run(exe, "on") == ["fh_set_denoise_response 1", "fh_set_denoise_response_noise 6"] + twice + ["noise 1 6"]
    assert _run(exe, "kappa") == ["fh_set_denoise_response 1", "fh_set_denoise_response_noise 4.5"] + twice + ["noise 1 4.5"]
    assert _run(exe, "off") == ["fh_set_denoise_response_noise off"] + twice + ["noise 0 6"]
    assert _run(exe, "alone") == ["fh_set_denoise_response_noise 6"] + twice + ["noise 1 6"]  # (stored by the context, inert there: the response switch is not touched)
    assert _run(exe, env={"FH_DENOISER": "temporal-response-noise"}) == ["fh_set_denoise_response 1", "fh_set_denoise_response_noise 6"] + twice + ["noise 1 6"]
    assert _run(exe, env={"FH_DENOISER": "temporal-motion-response-noise"}) == ["fh_set_denoise_motion 1", "fh_set_denoise_response 1", "fh_set_denoise_response_noise 6"] + twice + ["noise 1 6"]
    assert _run(exe, env={"FH_DENOISER": "temporal-response"}) == ["fh_set_denoise_response 1"] + twice + ["noise 0 6"]  # (the noise switch is not touched)
    assert _run(exe, "atrous") == ["fh_denoise", "fh_denoise", "noise 1 6"]  # (the switch belongs to the Temporal mode)


def test_rtcamp_knows_the_noise_denoisers_and_the_kappa_flag(tmp_path):
    rt = tmp_path / "rtcamp"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "rtcamp.cpp"), *LINK, "-lpthread", "-o", str(rt)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(rt), "--scene", "x.obj", "--denoiser", "temporal-bogus"], capture_output=True, text=True)
    assert run.returncode == 2 and "temporal-response-noise" in run.stderr and "temporal-motion-response-noise" in run.stderr
    for bad in ("0", "-1", "nan", "inf"):
        run = subprocess.run([str(rt), "--scene", "x.obj", "--denoiser", "temporal-response-noise", "--denoise-kappa", bad], capture_output=True, text=True)
        assert run.returncode == 2 and "--denoise-kappa" in run.stderr, (bad, run.stderr)
    for name in ("temporal", "temporal-response", "temporal-motion-response"):
        run = subprocess.run([str(rt), "--scene", "x.obj", "--denoiser", name, "--denoise-kappa", "4"], capture_output=True, text=True)
        assert run.returncode == 2 and "--denoise-kappa" in run.stderr and "noise" in run.stderr  # (a kappa no denoiser would use is refused, not ignored)
    usage = subprocess.run([str(rt)], capture_output=True, text=True)
    assert usage.returncode == 2 and "--denoise-kappa" in usage.stderr
