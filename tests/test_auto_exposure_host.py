"""CPU tests of auto-exposure (include/fredholm_hip.h: fh_set_auto_exposure ... fh_get_luminance_histogram): the exported symbols and the layout of the two structs,
every refusal -- decided from the arguments alone, with a NULL context --, the facades (kernels/post-process.h with FH_AUTO_EXPOSURE, the Python methods, rtcamp's
flags), and csrc/fh_meter.h compiled for the host (with -fsanitize=address,undefined) into a stand-alone program whose bins and states must equal, bit for bit, the
numpy restatement the device tests use (tests/test_gpu_auto_exposure.py), plus rank cuts computed by hand.  The kernels are tested on the GPU."""
import ctypes as C
import inspect
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from fredholm_amd import native as N

import test_gpu_auto_exposure as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINK = ["-L" + os.path.join(ROOT, "fredholm_amd"), "-lfredholm_hip", "-Wl,-rpath," + os.path.join(ROOT, "fredholm_amd"), "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
FH_E_INVALID = -1
PARAM_FIELDS = ["key", "compensation_ev", "min_ev", "max_ev", "low", "high", "speed_up", "speed_down", "frame_time", "log2_lo", "log2_hi", "flags"]
STATE_FIELDS = ["ev", "target_ev", "mean_log2", "metered", "unmetered", "frames"]


def _params_c(**kw):
    p = A.params(**{k: v for k, v in kw.items() if k != "flags"})
    return N.AutoExposureParamsC(*[p[k] for k in PARAM_FIELDS[:-1]], kw.get("flags", 0))


def test_symbols_structs_and_header_agree(tmp_path):
    L = N.load_library()
    want = {"fh_set_auto_exposure": [C.c_void_p, C.POINTER(N.AutoExposureParamsC)],
            "fh_get_auto_exposure": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(N.AutoExposureParamsC)],
            "fh_auto_exposure_reset": [C.c_void_p],
            "fh_meter_exposure": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32],
            "fh_get_auto_exposure_state": [C.c_void_p, C.POINTER(N.AutoExposureStateC)],
            "fh_get_luminance_histogram": [C.c_void_p, C.POINTER(C.c_uint32)]}
    for name, sig in want.items():
        assert name in N.EXPORTS
        fn = getattr(L, name)
        assert fn.restype is C.c_int and fn.argtypes == N.SIGNATURES[name] == sig, name
    hdr = " ".join(open(os.path.join(ROOT, "include", "fredholm_hip.h")).read().split())
    for decl in ("int fh_set_auto_exposure(fh_ctx* ctx, const fh_auto_exposure_params* params);",
                 "int fh_get_auto_exposure(fh_ctx* ctx, int* on, fh_auto_exposure_params* params);",
                 "int fh_auto_exposure_reset(fh_ctx* ctx);",
                 "int fh_meter_exposure(fh_ctx* ctx, const float* image_rgba, uint32_t width, uint32_t height);",
                 "int fh_get_auto_exposure_state(fh_ctx* ctx, fh_auto_exposure_state* state);",
                 "int fh_get_luminance_histogram(fh_ctx* ctx, uint32_t hist[257]);",
                 "#define FH_AE_BLOOM_RELATIVE 1u"):
        assert decl in hdr, decl
    fields = [("fh_auto_exposure_params", f) for f in PARAM_FIELDS] + [("fh_auto_exposure_state", f) for f in STATE_FIELDS]
    prints = "".join(f'printf("%zu\\n", offsetof({s}, {f}));' for s, f in fields)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fredholm_hip.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(fh_auto_exposure_params), '
                   'sizeof(fh_auto_exposure_state), sizeof(fh_post_params)); ' + prints + ' return 0; }\n')
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:3] == [C.sizeof(N.AutoExposureParamsC), C.sizeof(N.AutoExposureStateC), C.sizeof(N.PostParamsC)] == [48, 24, 20]
    assert got[3:] == [getattr(N.AutoExposureParamsC, f).offset for f in PARAM_FIELDS] + [getattr(N.AutoExposureStateC, f).offset for f in STATE_FIELDS]
    assert got[3:] == [4 * k for k in range(12)] + [4 * k for k in range(6)]
    assert N.AE_BLOOM_RELATIVE == 1


nan, inf = float("nan"), float("inf")
REFUSALS = [
    ([dict(key=0.0), dict(key=-1.0), dict(key=nan), dict(key=inf)], "key must be finite and > 0"),
    ([dict(compensation_ev=nan), dict(compensation_ev=inf)], "compensation_ev must be finite"),
    ([dict(min_ev=nan), dict(max_ev=inf), dict(min_ev=-inf)], "min_ev and max_ev must be finite"),
    ([dict(min_ev=1.0, max_ev=0.5)], "min_ev must not exceed max_ev"),
    ([dict(log2_lo=nan), dict(log2_hi=inf)], "log2_lo and log2_hi must be finite"),
    ([dict(log2_lo=0.0, log2_hi=0.0), dict(log2_lo=1.0, log2_hi=-1.0), dict(log2_lo=-40.0, log2_hi=40.0)], "log2_hi - log2_lo must be in (0, 64]"),
    ([dict(low=-0.1), dict(high=1.5), dict(low=nan), dict(high=nan)], "low and high must be in [0, 1]"),
    ([dict(low=0.5, high=0.5), dict(low=0.9, high=0.1)], "low must be below high"),
    ([dict(speed_up=-1.0), dict(speed_down=nan), dict(speed_up=inf)], "speed_up and speed_down must be finite and >= 0"),
    ([dict(frame_time=nan), dict(frame_time=-1.0)], "frame_time must be >= 0 (+inf: no adaptation)"),
    ([dict(flags=2), dict(flags=0x80000001)], "unknown flag bits"),
]


def test_every_refusal_is_decided_before_the_context_is_looked_at():
    """with a NULL context: each bad parameter is refused with its own message; good parameters and NULL (off) get as far as the context check"""
    L = N.lib()
    for cases, why in REFUSALS:
        for bad in cases:
            assert L.fh_set_auto_exposure(None, C.byref(_params_c(**bad))) == FH_E_INVALID
            assert L.fh_last_error(None).decode() == "fh_set_auto_exposure: " + why, bad
    L.fh_denoise_history_reset(None)
    marker = L.fh_last_error(None)
    for good in (dict(), dict(frame_time=inf), dict(frame_time=0.0), dict(speed_up=0.0, speed_down=0.0), dict(min_ev=2.0, max_ev=2.0), dict(low=0.0, high=1.0),
                 dict(log2_lo=-32.0, log2_hi=32.0), dict(flags=1)):
        assert L.fh_set_auto_exposure(None, C.byref(_params_c(**good))) == FH_E_INVALID and L.fh_last_error(None) == marker, good
    assert L.fh_set_auto_exposure(None, None) == FH_E_INVALID
    on, st, hist = C.c_int(0), N.AutoExposureStateC(), (C.c_uint32 * 257)()
    assert L.fh_get_auto_exposure(None, C.byref(on), None) == FH_E_INVALID and L.fh_auto_exposure_reset(None) == FH_E_INVALID
    assert L.fh_get_auto_exposure_state(None, C.byref(st)) == FH_E_INVALID and L.fh_get_luminance_histogram(None, hist) == FH_E_INVALID
    for img, w, h in ((None, 4, 4), (C.c_void_p(16), 0, 4), (C.c_void_p(16), 4, 0), (C.c_void_p(16), 32769, 1)):
        assert L.fh_meter_exposure(None, img, w, h) == FH_E_INVALID
        assert L.fh_last_error(None).decode() == "fh_meter_exposure: needs an image of 1 .. 32768 pixels each way"


def test_python_facade_has_the_methods_with_the_library_defaults():
    from fredholm_amd.renderer import Renderer
    sig = inspect.signature(Renderer.set_auto_exposure).parameters
    for k, v in A.DEFAULTS.items():
        assert sig[k].default == v, k
    assert sig["bloom_relative"].default is False
    for name in ("clear_auto_exposure", "get_auto_exposure", "auto_exposure_state", "auto_exposure_reset", "luminance_histogram"):
        assert callable(getattr(Renderer, name))
    assert list(inspect.signature(Renderer.meter_exposure).parameters)[1:] == ["image_ptr", "width", "height"]


# ------------------------------------------------------------------ the C++ facade over stubbed entry points
FACADE = r"""
#include "kernels/post-process.h"
#include <cstdio>
#include <cstring>
extern "C" int fh_ctx_create(int, fh_ctx** out) { *out = reinterpret_cast<fh_ctx*>(0x10); return FH_OK; }  // never dereferenced: the entries are the ones below
extern "C" int fh_ctx_create_group(const int*, uint32_t, fh_ctx** out) { *out = reinterpret_cast<fh_ctx*>(0x10); return FH_OK; }
extern "C" const char* fh_last_error(fh_ctx*) { return "stub"; }
extern "C" int fh_post_process(fh_ctx*, const float*, float*, float*, int, int, const fh_post_params*, float*) { std::printf("fh_post_process\n"); return FH_OK; }
extern "C" int fh_set_auto_exposure(fh_ctx*, const fh_auto_exposure_params* p)
{
  if (p) std::printf("fh_set_auto_exposure %g %g %g %g %g %g %g %g %g %g %g %u\n", (double)p->key, (double)p->compensation_ev, (double)p->min_ev, (double)p->max_ev, (double)p->low,
                     (double)p->high, (double)p->speed_up, (double)p->speed_down, (double)p->frame_time, (double)p->log2_lo, (double)p->log2_hi, p->flags);
  else std::printf("fh_set_auto_exposure off\n");
  return FH_OK;
}
extern "C" int fh_get_auto_exposure_state(fh_ctx*, fh_auto_exposure_state* s) { s->ev = 1.5f; s->frames = 7; std::printf("fh_get_auto_exposure_state\n"); return FH_OK; }
extern "C" int fh_auto_exposure_reset(fh_ctx*) { std::printf("fh_auto_exposure_reset\n"); return FH_OK; }
int main(int argc, char** argv)
{
  const char* what = argc > 1 ? argv[1] : "default";
  PostProcessParams pp{false, 2.0f, 5.0f, 80.0f, 1.0f};
  auto launch = [&] { post_process_kernel_launch(nullptr, nullptr, nullptr, 64, 48, pp, nullptr); };
  try {
    if (std::strcmp(what, "set") == 0) { AutoExposureParams a; a.key = 0.25f; a.frame_time = 0.125f; a.bloom_relative = true; set_auto_exposure(&a); }
    if (std::strcmp(what, "off") == 0) set_auto_exposure(nullptr);
    launch();
    launch();  // (the variable is read once)
    if (std::strcmp(what, "state") == 0) { const fh_auto_exposure_state s = get_auto_exposure_state(); reset_auto_exposure(); std::printf("state %g %u\n", (double)s.ev, s.frames); }
  } catch (const std::exception& e) { std::printf("error %s\n", e.what()); return 3; }
  return 0;
}
"""


@pytest.fixture(scope="module")
def facade(tmp_path_factory):
    d = tmp_path_factory.mktemp("auto_exposure_facade")
    src = d / "facade.cpp"
    src.write_text(FACADE)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(d / "facade")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(d / "facade")


def _run(exe, *args, env=None, rc=0):
    e = {k: v for k, v in os.environ.items() if k not in ("FH_AUTO_EXPOSURE", "FH_DEVICES")}
    e.update(env or {})
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=e)
    assert r.returncode == rc, (r.stdout, r.stderr)
    return r.stdout.splitlines()


def test_the_environment_variable_and_set_auto_exposure_reach_the_entry_point(facade):
    twice = ["fh_post_process", "fh_post_process"]
    defaults = "fh_set_auto_exposure 0.18 0 -16 16 0.1 0.9 3 1 0.0333333 -16 16 0"
    assert _run(facade) == twice  # (unset: the switch is not touched)
    assert _run(facade, env={"FH_AUTO_EXPOSURE": "0"}) == twice
    assert _run(facade, env={"FH_AUTO_EXPOSURE": "1"}) == [defaults] + twice
    assert _run(facade, env={"FH_AUTO_EXPOSURE": "0.3"}) == [defaults.replace("0.18", "0.3")] + twice
    assert _run(facade, env={"FH_AUTO_EXPOSURE": "bright"}, rc=3)[0].startswith("error FH_AUTO_EXPOSURE")
    mine = "fh_set_auto_exposure 0.25 0 -16 16 0.1 0.9 3 1 0.125 -16 16 1"
    assert _run(facade, "set") == [mine] + twice
    assert _run(facade, "set", env={"FH_AUTO_EXPOSURE": "1"}) == [mine] + twice  # (what the application set wins)
    assert _run(facade, "off", env={"FH_AUTO_EXPOSURE": "1"}) == ["fh_set_auto_exposure off"] + twice
    assert _run(facade, "state") == twice + ["fh_get_auto_exposure_state", "fh_auto_exposure_reset", "state 1.5 7"]


def test_rtcamp_refuses_exposure_flags_without_the_switch_and_bad_values(tmp_path):
    rt = tmp_path / "rtcamp"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "rtcamp.cpp"), *LINK, "-lpthread", "-o", str(rt)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for flags in (["--exposure-key", "0.2"], ["--exposure-comp", "1"], ["--exposure-speed", "3", "1"], ["--bloom-relative"]):
        run = subprocess.run([str(rt), "--scene", "x.obj", *flags], capture_output=True, text=True)
        assert run.returncode == 2 and flags[0] + " goes with --auto-exposure" in run.stderr, (flags, run.stderr)
    for flags, what in ((["--exposure-key", "0"], "--exposure-key"), (["--exposure-key", "nan"], "--exposure-key"), (["--exposure-comp", "inf"], "--exposure-comp"),
                        (["--exposure-speed", "-1", "1"], "--exposure-speed"), (["--exposure-speed", "1", "nan"], "--exposure-speed")):
        run = subprocess.run([str(rt), "--scene", "x.obj", "--auto-exposure", *flags], capture_output=True, text=True)
        assert run.returncode == 2 and what + " " in run.stderr, (flags, run.stderr)
    run = subprocess.run([str(rt), "--scene", "x.obj", "--auto-exposure", "--exposure-speed", "1"], capture_output=True, text=True)
    assert run.returncode == 2 and "missing value" in run.stderr
    run = subprocess.run([str(rt)], capture_output=True, text=True)
    assert run.returncode == 2 and "--auto-exposure" in run.stderr and "--bloom-relative" in run.stderr


# ------------------------------------------------------------------ fh_meter.h on the host against the restatement
METER = r"""
// reads: 12 words of fh_auto_exposure_params, n_frames, then per frame n_pixels and n_pixels * 4 floats; writes per frame 257 counts, the 6 words of the state, the exposure
#include <cstdio>
#include <vector>
#include "fh_meter.h"
int main(int argc, char** argv)
{
  if (argc != 3) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) return 2;
  fh_auto_exposure_params p;
  uint32_t n_frames = 0;
  if (std::fread(&p, sizeof p, 1, in) != 1 || std::fread(&n_frames, 4, 1, in) != 1) return 2;
  if (const char* why = fh::auto_exposure_refusal(&p)) { std::fprintf(stderr, "%s\n", why); return 3; }
  const fh::MeterConsts mc = fh::meter_consts(p);
  fh_auto_exposure_state st = {};
  for (uint32_t f = 0; f < n_frames; ++f) {
    uint32_t n = 0;
    if (std::fread(&n, 4, 1, in) != 1) return 2;
    std::vector<float> px(4 * (size_t)n);
    if (n && std::fread(px.data(), 16, n, in) != n) return 2;
    std::vector<uint32_t> hist(fh::kMeterWords, 0u);
    for (uint32_t i = 0; i < n; ++i) hist[fh::meter_bin(px[4 * i], px[4 * i + 1], px[4 * i + 2], mc.log2_lo, mc.scale)]++;
    fh::meter_resolve(hist.data(), mc, &st);
    const float exposure = fh::meter_exposure(st.ev);
    std::fwrite(hist.data(), 4, hist.size(), out);
    std::fwrite(&st, sizeof st, 1, out);
    std::fwrite(&exposure, 4, 1, out);
  }
  std::fclose(in);
  std::fclose(out);
  return 0;
}
"""


@pytest.fixture(scope="module")
def meter(tmp_path_factory):
    """csrc/fh_meter.h compiled for the host, with the address and undefined-behaviour sanitizers, into a stand-alone program"""
    d = tmp_path_factory.mktemp("meter_host")
    src = d / "meter.cpp"
    src.write_text(METER)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-I" + os.path.join(ROOT, "fredholm_amd", "csrc"), str(src), "-o", str(d / "meter")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(p, frames):
        """frames: images or ready-made lists of pixels; returns per frame (hist, state dict, exposure)"""
        blob = struct.pack("<11fI", *[p[k] for k in PARAM_FIELDS[:-1]], 0) + struct.pack("<I", len(frames))
        for f in frames:
            px = np.ascontiguousarray(f, dtype=np.float32).reshape(-1, 4)
            blob += struct.pack("<I", px.shape[0]) + px.tobytes()
        (d / "in.bin").write_bytes(blob)
        r = subprocess.run([str(d / "meter"), str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        raw = np.frombuffer((d / "out.bin").read_bytes(), dtype=np.uint32).reshape(len(frames), 257 + 7)
        out = []
        for row in raw:
            fl = row[257:].view(np.float32)
            out.append((row[:257].copy(), dict(ev=fl[0], target_ev=fl[1], mean_log2=fl[2], metered=int(row[260]), unmetered=int(row[261]), frames=int(row[262])), fl[6]))
        return out
    return run


def _same(got, want):
    return A._same_state(got, want)


def test_the_header_on_the_host_equals_the_restatement_bit_for_bit(meter, oracle):
    cases = [(A.params(frame_time=math.inf), [A.image(kind, w, h) for w, h in A.SIZES[:6] for kind in ("mixed", "constant", "black")]),
             (A.params(speed_up=6.0, speed_down=2.0), A.sequence_images()),
             (A.params(key=0.5, compensation_ev=-1.25, low=0.0, high=1.0, log2_lo=-7.5, log2_hi=9.0, frame_time=0.25), A.sequence_images(33, 9)),
             (A.params(min_ev=-1.0, max_ev=1.0, low=0.45, high=0.55, log2_lo=-40.0, log2_hi=24.0, speed_up=0.0), A.sequence_images(16, 16)),
             (A.params(frame_time=math.inf), [A.image("mixed", 1024, 640)])]
    for p, frames in cases:
        want = None
        independent = math.isinf(p["frame_time"])
        for f, (hist, state, exposure) in zip(frames, meter(p, frames)):
            wh = A.histogram(oracle, f, p)
            assert np.array_equal(hist, wh), np.flatnonzero(hist != wh)[:8]
            want = A.resolve(oracle, wh, p, want)
            assert _same(state, want), (state, want)
            assert A._bits(exposure) == A._bits(A.exposure_of(oracle, want["ev"]))
            if independent and want["frames"]:  # a = 1: ev + (target - ev) is the target to a rounding, not always to the bit
                assert abs(float(want["ev"]) - float(want["target_ev"])) <= 4e-6


def test_the_float32_and_float64_restatements_agree_within_the_bound(oracle, capsys):
    """STATE_BOUND of the device test, on its own sequence and on two more: printed, then asserted"""
    worst = 0.0
    for p, frames in ((A.params(speed_up=6.0, speed_down=2.0), A.sequence_images()), (A.params(), A.sequence_images(96, 72)),
                      (A.params(frame_time=math.inf), A.sequence_images(16, 16))):
        s32 = s64 = None
        for f in frames:
            hist = A.histogram(oracle, f, p)
            s32, s64 = A.resolve(oracle, hist, p, s32), A.resolve64(hist, p, s64)
            worst = max(worst, abs(float(s32["ev"]) - s64["ev"]), abs(float(s32["target_ev"]) - s64["target_ev"]), abs(float(s32["mean_log2"]) - s64["mean_log2"]))
    with capsys.disabled():
        print(f"\nauto-exposure: float32 against float64 restatement, largest distance {worst:.3g} (bound {A.STATE_BOUND:.3g})")
    assert worst <= A.STATE_BOUND


def test_rank_cuts_by_hand(meter, oracle):
    """bins of width 1/8 from -16: 2^k lies in bin 128 + 8k, centre k + 1/16.  key 1, so target = -mean"""
    grey = lambda l: [l / 1.0000001, l / 1.0000001, l / 1.0000001, 1.0]  # lum() of three equal channels is their value times 1.0000001: stay inside the bin
    p = A.params(key=1.0, frame_time=math.inf)
    # N = 1: cut = 0, end = 0 -> end = 1, cut = 0: the one pixel is kept
    assert A.rank_cuts(1, 0.1, 0.9) == (0, 1)
    (hist, st, _), = meter(p, [[grey(1.5)]])
    assert hist[128 + 4] == 1 and st["metered"] == 1 and st["mean_log2"] == 0.5 + 1 / 16 and st["ev"] == -(0.5 + 1 / 16)
    # N = 10, low 0.1 / high 0.9: cut = (uint32)(10 * (double)0.1f) = 1, end = (uint32)(10 * (double)0.9f) = 8 (0.9f is below 0.9): ranks 1 .. 7 are kept
    assert A.rank_cuts(10, 0.1, 0.9) == (1, 8)
    px = [grey(2.0 ** k * 1.5) for k in range(10)]  # ranks 0 .. 9 in bins 132, 140, ..., centres k + 9/16
    (hist, st, _), = meter(p, [px])
    assert [int(hist[132 + 8 * k]) for k in range(10)] == [1] * 10 and st["metered"] == 10
    assert st["mean_log2"] == np.float32(sum(k + 9 / 16 for k in range(1, 8)) / 7)
    kept = A.kept_counts(hist, 1, 8)
    assert kept.sum() == 7 and kept[132] == 0 and kept[132 + 8 * 8] == 0 and kept[132 + 8 * 9] == 0 and kept[132 + 8] == 1
    # all pixels in one bin: the mean is that bin's centre whatever the cuts
    (hist, st, _), = meter(p, [[grey(6.0)] * 37 + [[0.0, 0.0, 0.0, 1.0]] * 5])
    assert hist[128 + 8 * 2 + 4] == 37 and hist[256] == 5 and st["metered"] == 37 and st["unmetered"] == 5 and st["mean_log2"] == 2.5 + 1 / 16
    # end <= cut: low 0.5 / high 0.55 of N = 4: cut = 2, end = 2 -> end = 3: rank 2 alone
    assert A.rank_cuts(4, 0.5, 0.55) == (2, 3)
    (hist, st, _), = meter(A.params(key=1.0, frame_time=math.inf, low=0.5, high=0.55), [[grey(2.0 ** k * 1.5) for k in range(4)]])
    assert st["mean_log2"] == 2 + 9 / 16
    # ... and at the top: low 0.99 / high 1 of N = 4: cut = 3, end = 4
    assert A.rank_cuts(4, 0.99, 1.0) == (3, 4) and A.rank_cuts(4, 1.0 - 1e-9, 1.0) == (3, 4)
    # bins 0 and 255 take what lies beyond the range: 2^-20 and 2^20 with the range -16 .. 16; low 0 / high 1 keeps both: the mean of the two centres
    (hist, st, _), = meter(A.params(key=1.0, frame_time=math.inf, low=0.0, high=1.0), [[grey(2.0 ** -20), grey(2.0 ** 20), grey(1e-40), grey(3.0e38)]])
    assert hist[0] == 2 and hist[255] == 2 and st["mean_log2"] == 0.0 and st["ev"] == 0.0
    for (h, s, _), f in zip(meter(p, [px]), [px]):
        assert _same(s, A.resolve(oracle, A.histogram(oracle, np.array(f, np.float32), p), p, None))
