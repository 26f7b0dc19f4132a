// fh_lights.h -- sampling of area lights by power (host + device): the weight of an emitter, its quantisation, the CDF over the emitters, the pick probabilities, the
// pick itself and the host-side refusals of fh_set_light_sampling.  Shared by lights.hip (the build kernels), render.hip (the LT variants of shade_hit and
// resolve_light_ray), kat.hip (fh_kat_light_*), capi.hip (fh_set_light_sampling) and the stand-alone program of tests/test_light_sampling_host.py.  The arithmetic is the
// one include/fredholm_hip.h states under fh_light_sampling_params: fp32 without contraction, / and sqrt correctly rounded, everything in the order written; the CDF
// entries and the table shares are quotients of integers formed in double and rounded once.  The reference has no counterpart (pt.cu:860-889 picks uniformly).
#pragma once
#include <cmath>
#include <cstdint>

#include "fh_envmap.h"

namespace fh {

constexpr int kLightPoints = 16;              // barycentric points a textured emitter's colour is averaged over
constexpr float kLightQuant = kEnvQuant;      // 2^20: an emitter's weight against the largest
constexpr float kLightBelowOne = kEnvBelowOne;

// the table as the kernels see it (device pointers) and as the host program builds it (host pointers)
struct LightTable {
  const float* cdf;      // [n_lights + 1]  ascending, first 0, last 1
  const float* pick_p;   // [n_faces]       the pick probability P of the emitter that is this face; 0 for a face that does not emit
  float uniform;         // U: share of the picks that stay uniform
};

// point s of the set, s in [0, 16): the centroids of the 16 congruent triangles a triangle splits into with four segments per edge -- the ten that point the way
// it does (s = 0..9: rows j = 0..3 of 4 - j points, (3 i + 1, 3 j + 1) / 12), then the six that point the other way (s = 10..15: rows j = 0..2 of 3 - j, (3 i + 2, 3 j + 2) / 12)
FH_EV void light_point(int s, float* bu, float* bv)
{
  int i = s, j = 0, n = 4, off = 1;
  if (s >= 10) { i = s - 10; n = 3; off = 2; }
  while (i >= n - j) { i -= n - j; ++j; }
  *bu = (float)(3 * i + off) / 12.0f;
  *bv = (float)(3 * j + off) / 12.0f;
}
// the texture coordinate shade_hit forms at barycentrics (bu, bv): t0, t1, t2 are the corner's
FH_EV float light_lerp(float t0, float t1, float t2, float bu, float bv) { const float bw = 1.0f - bu - bv; return bw * t0 + bu * t1 + bv * t2; }
// the weight of an emitter from its area and its emission colour (the mean over the point set when textured)
FH_EV float light_weight(float area, float r, float g, float b) { return fminf(area * fmaxf(env_lum(r, g, b), 0.0f), 3.0e38f); }
FH_EV uint32_t light_quantise(float w, float w_max) { return env_quantise(w, w_max); }
// P_k of an emitter with integer weight q among n, the integer total being `total`
FH_EV float light_pick_p(uint32_t q, uint64_t total, uint32_t n, float uniform) { return (1.0f - uniform) * env_ratio(q, total) + uniform / (float)n; }
// the interval of `cdf` (n + 1 ascending entries, cdf[0] = 0, cdf[n] = 1) that holds u in [0, 1): the largest k with cdf[k] <= u, by bisection.  env_search restated
// with unsigned indices, not called: a second caller of that function changed the instruction streams of the kernels that already call it (k_shade_env, k_tail_env)
FH_EV uint32_t light_search(const float* cdf, uint32_t n, float u)
{
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (cdf[mid] <= u) lo = mid; else hi = mid;
  }
  return lo;
}
// the pick from the draw u1 in [0, 1): the emitter's index in light order
FH_EV uint32_t light_pick(const float* cdf, uint32_t n, float uniform, float u1)
{
  if (u1 < uniform) {
    const float u = u1 / uniform;
    const uint32_t k = (uint32_t)(u * n);
    return k < n - 1u ? k : n - 1u;
  }
  const float u = fminf((u1 - uniform) / (1.0f - uniform), kLightBelowOne);
  return light_search(cdf, n, u);
}

// ---- host only
// the whole build as the kernels of lights.hip run it in parallel, in a loop: w = the n weights; out: q [n], cdf [n + 1], p [n] (per light), the total
inline void light_build_host(const float* w, uint32_t n, float uniform, uint32_t* q, float* cdf, float* p, uint64_t* total_out)
{
  float w_max = 0.0f;
  for (uint32_t k = 0; k < n; ++k) w_max = fmaxf(w_max, w[k]);
  uint64_t total = 0;
  for (uint32_t k = 0; k < n; ++k) { q[k] = light_quantise(w[k], w_max); total += q[k]; }
  uint64_t run = 0;
  for (uint32_t k = 0; k < n; ++k) {
    cdf[k] = env_ratio(run, total);
    run += q[k];
    p[k] = light_pick_p(q[k], total, n, uniform);
  }
  cdf[n] = 1.0f;
  *total_out = total;
}

// nullptr: acceptable (params == nullptr switches off)
inline const char* light_sampling_refusal(const fh_light_sampling_params* p)
{
  if (!p) return nullptr;
  if (!(p->uniform_fraction > 0.0f && p->uniform_fraction <= 1.0f)) return "uniform_fraction must be in (0, 1]";
  return nullptr;
}

}  // namespace fh
