// fh_local_exposure.h -- local exposure of the post chain (host + device): the log-luminance of a pixel, the ordered mean of a 4 x 4 block, one pixel of an edge-stopping
// a-trous pass on the quarter image, the joint bilateral upsampling of the base to an output pixel, the gain, and the host-side refusals and constants.  Shared by
// post.hip (k_lx_down, k_lx_atrous, k_tone_map_local), capi.hip (fh_set_local_exposure) and the stand-alone program of tests/test_local_exposure_host.py.  The arithmetic
// is the one include/fredholm_hip.h states under fh_local_exposure_params: fp32 without contraction, / correctly rounded, sums in the order written.  The reference has
// no counterpart (its tone map has one exposure per frame).
#pragma once
#include <cmath>
#include <cstdint>

#include "fh_meter.h"

namespace fh {

constexpr int kLxFactor = 4;       // the quarter image: one pixel per 4 x 4 block, partial blocks at the right and bottom edges included
constexpr int kLxMaxPasses = 6;
constexpr float kLxFloor = 0x1p-24f;  // luminance floor of the log image: black, negative and unmetered pixels sit 24 stops down

// what the kernels take by value: fh_local_exposure_params with everything that needs the host's elementary functions done (lx_consts)
struct LxConsts {
  float highlights, shadows, log2pivot, max_stops, inv_sr;
};

FH_MT int lx_quarter(int n) { return (n + kLxFactor - 1) / kLxFactor; }
FH_MT int lx_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// 1. the log image
FH_MT float lx_log(float r, float g, float b) { return fhe_log2(fmaxf(meter_lum(meter_finite(r), meter_finite(g), meter_finite(b)), kLxFloor)); }

// 2. the quarter image: the first n (1 .. 4) values of a row added left to right; the first n_rows row sums added top to bottom and divided by the number of pixels
FH_MT float lx_row_sum(float l0, float l1, float l2, float l3, int n)
{
  float s = l0;
  if (n > 1) s += l1;
  if (n > 2) s += l2;
  if (n > 3) s += l3;
  return s;
}
FH_MT float lx_block_mean(float r0, float r1, float r2, float r3, int n_rows, int n_cols) { return lx_row_sum(r0, r1, r2, r3, n_rows) / (float)(n_rows * n_cols); }

// 3. pixel (X, Y) of one a-trous pass with hole s on the w4 x h4 image D
FH_MT float lx_atrous(const float* D, int w4, int h4, int X, int Y, int s, float inv_sr)
{
  const float kern[3] = {3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
  const float dp = D[X + w4 * Y];
  float num = 0.0f, den = 0.0f;
  for (int dy = -2; dy <= 2; ++dy)
    for (int dx = -2; dx <= 2; ++dx) {
      const float dq = D[lx_clampi(X + s * dx, w4 - 1) + w4 * lx_clampi(Y + s * dy, h4 - 1)];
      const float t = (dq - dp) * inv_sr;
      const float wt = (kern[dx < 0 ? -dx : dx] * kern[dy < 0 ? -dy : dy]) * fhe_exp(-(t * t));
      num += wt * dq;
      den += wt;
    }
  return num / den;  // the centre tap has weight 9/64: never zero
}

// 4. the base at output pixel (i, j) whose own log-luminance is lp: four taps of the quarter-resolution base, bilinear weights times the edge stop against lp
FH_MT float lx_upsample(const float* base, int w4, int h4, int i, int j, float lp, float inv_sr)
{
  const float fx = ((float)i + 0.5f) * 0.25f - 0.5f, fy = ((float)j + 0.5f) * 0.25f - 0.5f;
  const float x0 = floorf(fx), y0 = floorf(fy);
  const float tx = fx - x0, ty = fy - y0;
  const int xi[2] = {lx_clampi((int)x0, w4 - 1), lx_clampi((int)x0 + 1, w4 - 1)}, yi[2] = {lx_clampi((int)y0, h4 - 1), lx_clampi((int)y0 + 1, h4 - 1)};
  const float wx[2] = {1.0f - tx, tx}, wy[2] = {1.0f - ty, ty};
  float num = 0.0f, den = 0.0f;
  for (int b = 0; b < 2; ++b)
    for (int a = 0; a < 2; ++a) {
      const float q = base[xi[a] + w4 * yi[b]];
      const float t = (q - lp) * inv_sr;
      const float wt = (wy[b] * wx[a]) * fhe_exp(-(t * t));
      num += wt * q;
      den += wt;
    }
  return den > 1e-6f ? num / den : lp;
}

// 5. what the tone map multiplies r, g, b by in place of `exposure`
FH_MT float lx_gain(float B, float exposure, const LxConsts& c)
{
  const float d = (B + fhe_log2(exposure)) - c.log2pivot;
  float g = -(d > 0.0f ? c.highlights : c.shadows) * d;
  g = fmaxf(-c.max_stops, fminf(g, c.max_stops));
  return exposure * fhe_pow(2.0f, g);
}

// ---- host only
inline const fh_local_exposure_params& local_exposure_defaults()
{
  static const fh_local_exposure_params d = {0.5f, 0.5f, 0.18f, 4.0f, 1.0f, 4u};
  return d;
}

// every refusal is decided from the parameters alone; nullptr: acceptable (params == nullptr switches off)
inline const char* local_exposure_refusal(const fh_local_exposure_params* p)
{
  if (!p) return nullptr;
  if (!(p->highlights >= 0.0f && p->highlights <= 1.0f)) return "highlights must be in [0, 1]";
  if (!(p->shadows >= 0.0f && p->shadows <= 1.0f)) return "shadows must be in [0, 1]";
  if (!(p->pivot > 0.0f) || !std::isfinite(p->pivot)) return "pivot must be finite and > 0";
  if (!(p->max_stops >= 0.0f) || !std::isfinite(p->max_stops)) return "max_stops must be finite and >= 0";
  if (!(p->sigma_range > 0.0f) || !std::isfinite(p->sigma_range)) return "sigma_range must be finite and > 0";
  if (p->passes < 1u || p->passes > (uint32_t)kLxMaxPasses) return "passes must be 1 .. 6";
  return nullptr;
}

inline LxConsts lx_consts(const fh_local_exposure_params& p)
{
  LxConsts c;
  c.highlights = p.highlights; c.shadows = p.shadows;
  c.log2pivot = fhe_log2(p.pivot);
  c.max_stops = p.max_stops;
  c.inv_sr = 1.0f / p.sigma_range;
  return c;
}

}  // namespace fh
