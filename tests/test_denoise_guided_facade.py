"""CPU test of fredholm::Denoiser's modes (include/fredholm/denoiser.h).  A small program defines fh_denoise and fh_denoise_guided itself -- the executable's
definitions are the ones the header-only facade binds to, the rest comes from the library -- and prints which entry a denoise() reached and with what: the default
reaches fh_denoise, set_mode(Guided) and the environment variable FH_DENOISER=guided reach fh_denoise_guided with the guides set_guides() was given."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINK = ["-L" + os.path.join(ROOT, "fredholm_amd"), "-lfredholm_hip", "-Wl,-rpath," + os.path.join(ROOT, "fredholm_amd"), "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]

SOURCE = r"""
#include "fredholm/denoiser.h"
#include <cstdio>
#include <cstring>
extern "C" int fh_denoise(fh_ctx*, uint32_t width, uint32_t height, const float* beauty, const float* normal, const float* albedo, float* denoised, int upscale2x)
{
  std::printf("fh_denoise %u %u %p %p %p %p %d\n", width, height, (const void*)beauty, (const void*)normal, (const void*)albedo, (void*)denoised, upscale2x);
  return FH_OK;
}
extern "C" int fh_denoise_guided(fh_ctx*, uint32_t width, uint32_t height, const fh_denoise_inputs* in, const fh_denoise_params* params, float* denoised, int upscale2x)
{
  std::printf("fh_denoise_guided %u %u %p %p %p %p %p %p %p %p %p %d\n", width, height, (const void*)in->beauty, (const void*)in->normal, (const void*)in->albedo, (const void*)in->position,
              (const void*)in->depth, (const void*)in->moments, (const void*)in->counts, (const void*)params, (void*)denoised, upscale2x);
  return FH_OK;
}
int main(int argc, char** argv)
{
  fh_ctx* ctx = reinterpret_cast<fh_ctx*>(0x10);  // never dereferenced: both entries are the ones above
  auto f4 = [](uintptr_t a) { return reinterpret_cast<const float4*>(a); };
  fredholm::Denoiser denoiser(ctx, 64, 48, f4(0x100), f4(0x200), f4(0x300), f4(0x400), argc > 2 && std::strcmp(argv[2], "upscale") == 0);
  const char* what = argc > 1 ? argv[1] : "default";
  if (std::strcmp(what, "guided") == 0) denoiser.set_mode(fredholm::Denoiser::Guided);
  if (std::strcmp(what, "atrous") == 0) denoiser.set_mode(fredholm::Denoiser::Atrous);
  if (std::strcmp(what, "guides") == 0) {
    denoiser.set_mode(fredholm::Denoiser::Guided);
    denoiser.set_guides(f4(0x500), reinterpret_cast<const float*>(0x600), reinterpret_cast<const float2*>(0x700), reinterpret_cast<const uint32_t*>(0x800));
  }
  if (std::strcmp(what, "planes") == 0) {
    denoiser.set_mode(fredholm::Denoiser::Guided);
    denoiser.set_guides(f4(0x500), reinterpret_cast<const float*>(0x600));
  }
  denoiser.denoise();
  return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("denoiser_modes")
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


def test_default_reaches_fh_denoise(exe):
    assert _run(exe) == ["fh_denoise", "64", "48", "0x100", "0x200", "0x300", "0x400", "0"]
    assert _run(exe, "default", "upscale")[-1] == "1"
    assert _run(exe, env={"FH_DENOISER": "atrous"})[0] == "fh_denoise"
    assert _run(exe, env={"FH_DENOISER": ""})[0] == "fh_denoise"


def test_set_mode_guided_reaches_the_new_entry(exe):
    assert _run(exe, "guided") == ["fh_denoise_guided", "64", "48", "0x100", "0x200", "0x300", NIL, NIL, NIL, NIL, NIL, "0x400", "0"]
    assert _run(exe, "guides", "upscale") == ["fh_denoise_guided", "64", "48", "0x100", "0x200", "0x300", "0x500", "0x600", "0x700", "0x800", NIL, "0x400", "1"]
    assert _run(exe, "planes") == ["fh_denoise_guided", "64", "48", "0x100", "0x200", "0x300", "0x500", "0x600", NIL, NIL, NIL, "0x400", "0"]


def test_environment_variable_selects_guided_and_set_mode_wins(exe):
    assert _run(exe, env={"FH_DENOISER": "guided"}) == ["fh_denoise_guided", "64", "48", "0x100", "0x200", "0x300", NIL, NIL, NIL, NIL, NIL, "0x400", "0"]
    assert _run(exe, "atrous", env={"FH_DENOISER": "guided"})[0] == "fh_denoise"


def test_rtcamp_has_the_denoiser_flag(tmp_path):
    rt = tmp_path / "rtcamp"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "rtcamp.cpp"), *LINK, "-lpthread", "-o", str(rt)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(rt), "--scene", "x.obj", "--denoiser", "median"], capture_output=True, text=True)
    assert run.returncode == 2 and "--denoiser" in run.stderr
