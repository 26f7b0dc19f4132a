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
  // fh_set_light_resampling: the emitters' proxies [n_lights], built with the table, and M (1: no resampling, the table's pick as it is)
  const struct LightProxy* proxy = nullptr;
  uint32_t candidates = 1;
};

// what the resampling knows of an emitter: two float4 -- (centroid, area) and (mean shading normal or the zero vector, 0)
struct alignas(16) LightProxy {
  float cx, cy, cz, area;
  float mx, my, mz, pad;
};
static_assert(sizeof(LightProxy) == 32, "two float4 per emitter");

constexpr uint32_t kLightCandidatesMax = 16;
constexpr float kLightFloor = 0.0625f;                       // 1/16: added to both clamped cosines of the geometric weight
constexpr float kLightGeomMin = 1e-30f, kLightGeomMax = 1e30f;

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
// with unsigned indices, not called: a second caller of that function changed the instruction streams of the kernels that already call it (k_shade and k_tail with the environment table)
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

// ---- fh_set_light_resampling: the proxy of an emitter, the geometric weight of a proxy seen from a point, and the choice among M candidates of the table
// the proxy from the world-space corners p0, p1, p2, the corners' shading normals n0, n1, n2 (three floats each) and the area the table computed
FH_EV LightProxy light_proxy(const float* p0, const float* p1, const float* p2, const float* n0, const float* n1, const float* n2, float area)
{
  LightProxy pr;
  pr.cx = ((p0[0] + p1[0]) + p2[0]) / 3.0f;
  pr.cy = ((p0[1] + p1[1]) + p2[1]) / 3.0f;
  pr.cz = ((p0[2] + p1[2]) + p2[2]) / 3.0f;
  pr.area = area;
  const float sx = (n0[0] + n1[0]) + n2[0], sy = (n0[1] + n1[1]) + n2[1], sz = (n0[2] + n1[2]) + n2[2];
  const float len = sqrtf((sx * sx + sy * sy) + sz * sz);
  const bool ok = len > 0.0f && len <= 3.0e38f;  // (false for 0, infinity and NaN)
  pr.mx = ok ? sx / len : 0.0f;
  pr.my = ok ? sy / len : 0.0f;
  pr.mz = ok ? sz / len : 0.0f;
  pr.pad = 0.0f;
  return pr;
}
// G of a proxy seen from so with shading normal ns: positive and finite whatever the operands
FH_EV float light_geom(const LightProxy& pr, float sox, float soy, float soz, float nsx, float nsy, float nsz)
{
  const float vx = pr.cx - sox, vy = pr.cy - soy, vz = pr.cz - soz;
  const float r2 = (vx * vx + vy * vy) + vz * vz;
  const float r = sqrtf(r2);
  const float dx = vx / r, dy = vy / r, dz = vz / r;
  const float cs = fmaxf((nsx * dx + nsy * dy) + nsz * dz, 0.0f) + kLightFloor;
  const float cl = fmaxf(-((pr.mx * dx + pr.my * dy) + pr.mz * dz), 0.0f) + kLightFloor;
  const float g = cs * cl / (r2 + pr.area);
  return fminf(fmaxf(g, kLightGeomMin), kLightGeomMax);  // (fmaxf first: a NaN goes to the lower bound)
}
// candidate k of M from the one draw: t = u1 * M, j = min((uint32)t, M - 1), v = t - j; u_k = min((k + v) / M, below one)
FH_EV float light_candidate_v(float u1, uint32_t m)
{
  const float t = u1 * (float)m;
  const uint32_t j = (uint32_t)t < m - 1u ? (uint32_t)t : m - 1u;
  return t - (float)j;
}
FH_EV float light_candidate_u(uint32_t k, float v, uint32_t m) { return fminf(((float)k + v) / (float)m, kLightBelowOne); }

struct LightChoice {
  uint32_t index;  // the chosen emitter, in light order
  float ratio;     // G_y / (S / (float)M): what pdf_area is multiplied by in the division of the shadow ray's contribution
  float sum;       // S
};
// The choice among the t.candidates candidates.  Two passes over the candidates, the second repeating the first's arithmetic (the same operands give the same bits):
// nothing per candidate is kept in registers between them, which the fused tail has none to spare for.
FH_EV LightChoice light_resample(const LightTable& t, uint32_t n, float u1, float u_sel, float sox, float soy, float soz, float nsx, float nsy, float nsz)
{
  const uint32_t m = t.candidates;
  const float v = light_candidate_v(u1, m);
  float sum = 0.0f;
  for (uint32_t k = 0; k < m; ++k) sum += light_geom(t.proxy[light_pick(t.cdf, n, t.uniform, light_candidate_u(k, v, m))], sox, soy, soz, nsx, nsy, nsz);
  const float thr = u_sel * sum;
  float run = 0.0f, g = 0.0f;
  uint32_t y = 0;
  for (uint32_t k = 0; k < m; ++k) {
    y = light_pick(t.cdf, n, t.uniform, light_candidate_u(k, v, m));
    g = light_geom(t.proxy[y], sox, soy, soz, nsx, nsy, nsz);
    run += g;
    if (run > thr) break;
  }
  return LightChoice{y, g / (sum / (float)m), sum};
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

// nullptr: acceptable (params == nullptr switches off)
inline const char* light_resampling_refusal(const fh_light_resampling_params* p)
{
  if (!p) return nullptr;
  const int m = p->candidates;
  if (!(m == 1 || m == 2 || m == 4 || m == 8 || m == 16)) return "candidates must be 1, 2, 4, 8 or 16";
  return nullptr;
}

}  // namespace fh

#if defined(__HIPCC__)
#include "fh_sampler.h"
namespace fh {
constexpr uint32_t kLightSelSalt = 0x9e3779b9u;  // include/fredholm_hip.h prints it
// u_sel of a shaded hit: a hash of what identifies the hit's area draw, NOT a function of that draw
FH_HD float light_usel(uint32_t image_idx, uint32_t n_spp, uint32_t dim_area, uint32_t seed_hash)
{
  return (float)(xxhash32(image_idx, n_spp, dim_area, seed_hash ^ kLightSelSalt) >> 8) * 5.9604644775390625e-8f;  // 2^-24
}
}  // namespace fh
#endif
