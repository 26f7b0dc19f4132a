"""CPU test of the tone map's fetch addresses (csrc/fh_tonemap.h: tonemap_fetch, the one place the three tone-map kernels of post.hip take them from).  The helper is
compiled for the host (with -fsanitize=address,undefined) into a stand-alone program, and its three addresses are compared, as integers and for every pixel of the
frame, with fetch_model below: a numpy float32 model written from the reference's tone_mapping_kernel (post-process.cu:122-136, with sutil's float2 / float, which
multiplies by 1.0f / s, and its clamp, fmaxf(a, fminf(f, b))), vectorised over the frame -- not a transcription of the helper.  The helper must equal
min(model, w * h - 1): an address past the last pixel reads the last pixel (include/fredholm_hip.h, fh_post_process); the reference leaves that case undefined.

Where the model leaves the image.  A clamped coordinate of exactly 1 in y makes the float sum at least w * h.  That takes no exotic input: the blue fetch is
uv - 2 * d with d = (uv - 0.5) / (w * h) * ca, so a negative ca pushes the bottom rows past 1 once 2 * 0.5 * |ca| / (w * h) reaches the distance of row h - 1 from 1,
which is 1 / h: ca = -0.25 * w and everything below.  A positive ca >= w * h flips the frame about its centre and pushes the top rows past 1.  +-inf does the
same with d = +-inf, and where uv is exactly 0.5 (even sizes) d = 0 * inf = NaN; NaN makes every d NaN.  clamp(NaN) is 1, because fminf(NaN, 1) is 1 -- and since
the red fetch is uv - 0.0f * d, a non-finite d moves red too.  The largest sum is w * h + w (both coordinates 1); nothing is ever negative.  The test asserts the
overrun for the values above at 16 x 16 and 64 x 48, so that the bound is exercised and not merely present."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SHAPES = [(1, 1), (5, 3), (16, 7), (7, 40), (16, 16), (33, 17), (64, 48), (70, 50), (48, 130)]
inf, nan = float("inf"), float("nan")


def overrunning(w, h):
    """values of chromatic_aberration at which the reference's address leaves a w x h image (16 x 16 and 64 x 48: asserted below)"""
    return [-0.25 * w, -1.0 * w, -0.1 * w * h, 1.0 * w * h, 2.0 * w * h, inf, -inf, nan]


def aberrations(w, h):
    wh = w * h
    return [0.0, 1.0, -1.0, 1.5, 0.02 * wh, 0.1 * wh, 0.45 * wh, 0.5 * wh] + overrunning(w, h)


def fetch_model(w, h, ca):
    """the reference's image_idx_r, _g, _b for every pixel: (3, h, w) int64, NOT limited to the image"""
    j, i = np.mgrid[0:h, 0:w]
    uv = np.stack([i.astype(f32) / f32(w), j.astype(f32) / f32(h)])  # make_float2(float(i) / width, float(j) / height)
    with np.errstate(all="ignore"):
        d = (uv - f32(0.5)) * (f32(1) / f32(w * h)) * f32(ca)         # (uv - 0.5f) / (width * height) * chromatic_aberration
        out = []
        for k in (0.0, 1.0, 2.0):
            c = np.fmax(f32(0), np.fmin(uv - f32(k) * d, f32(1)))     # clamp(uv - k * d, 0, 1)
            s = c[0] * f32(w) + f32(w) * (c[1] * f32(h))              # uv.x * width + width * (uv.y * height), converted to int: truncation
            assert s.dtype == np.float32 and np.isfinite(s).all()
            out.append(np.trunc(s).astype(np.int64))
    return np.stack(out)


PROGRAM = r"""
// reads records of (int32 w, int32 h, float ca); writes for each the r, g and b addresses of every pixel, row-major: 3 * w * h int32
#include <cstdint>
#include <cstdio>
#include <vector>
#include "fh_tonemap.h"
int main(int argc, char** argv)
{
  if (argc != 3) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) return 2;
  struct { int32_t w, h; float ca; } rec;
  while (std::fread(&rec, sizeof rec, 1, in) == 1) {
    const size_t n = (size_t)rec.w * rec.h;
    std::vector<int32_t> a(3 * n);
    for (int j = 0; j < rec.h; ++j)
      for (int i = 0; i < rec.w; ++i) {
        const fh::TonemapFetch f = fh::tonemap_fetch(i, j, rec.w, rec.h, rec.ca);
        a[i + rec.w * j] = f.r; a[n + i + rec.w * j] = f.g; a[2 * n + i + rec.w * j] = f.b;
      }
    std::fwrite(a.data(), 4, a.size(), out);
  }
  std::fclose(in);
  std::fclose(out);
  return 0;
}
"""


@pytest.fixture(scope="module")
def helper(tmp_path_factory):
    """csrc/fh_tonemap.h compiled for the host, with the address and undefined-behaviour sanitizers, into a stand-alone program: cases -> list of (3, h, w) int32"""
    d = tmp_path_factory.mktemp("post_chain_host")
    src = d / "fetch.cpp"
    src.write_text(PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-I" + os.path.join(ROOT, "fredholm_amd", "csrc"), str(src), "-o", str(d / "fetch")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(cases):
        (d / "in.bin").write_bytes(b"".join(struct.pack("<iif", w, h, ca) for w, h, ca in cases))
        r = subprocess.run([str(d / "fetch"), str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        raw = np.frombuffer((d / "out.bin").read_bytes(), dtype=np.int32)
        assert raw.size == sum(3 * w * h for w, h, _ in cases)
        return [a.reshape(3, h, w) for a, (w, h, _) in zip(np.split(raw, np.cumsum([3 * w * h for w, h, _ in cases])[:-1]), cases)]
    return run


def test_the_helper_is_the_reference_model_limited_to_the_last_pixel(helper):
    cases = [(w, h, ca) for w, h in SHAPES for ca in aberrations(w, h)]
    limited = 0
    for (w, h, ca), got in zip(cases, helper(cases)):
        model = fetch_model(w, h, ca)
        assert model.min() >= 0 and model.max() <= w * h + w, (w, h, ca)
        assert np.array_equal(got, np.minimum(model, w * h - 1)), (w, h, ca, np.argwhere(got != np.minimum(model, w * h - 1))[:4])
        assert got.min() >= 0 and got.max() < w * h, (w, h, ca)
        limited += int((model > w * h - 1).sum())
        if ca == 0.0:
            assert np.array_equal(got, np.broadcast_to(np.arange(w * h).reshape(h, w), (3, h, w)))  # no aberration: every channel from the pixel itself
    assert limited > 0


@pytest.mark.parametrize("w,h", [(16, 16), (64, 48)])
def test_the_reference_model_leaves_the_image_where_the_bound_is_needed(w, h):
    """non-vacuity: each of these values puts an address of the unbounded model past the last pixel; none of the ordinary ones does"""
    for ca in overrunning(w, h):
        model = fetch_model(w, h, ca)
        assert model.max() > w * h - 1, (w, h, ca, model.max())
        assert model.max() <= w * h + w and (abs(ca) < w * h or model.max() == w * h + w), (w, h, ca, model.max())  # (flipped or non-finite: both coordinates reach 1)
    for ca in (0.0, 1.0, -1.0, 1.5, 0.02 * w * h, 0.1 * w * h, 0.45 * w * h):
        assert fetch_model(w, h, ca).max() <= w * h - 1, (w, h, ca)
    assert (fetch_model(w, h, nan) == w * h + w).all()  # clamp(NaN) is 1 in x and in y, for red too: 0.0f * NaN is NaN
