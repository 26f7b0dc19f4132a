// fh_envmap.h -- importance sampling of the environment (host + device): the lat-long table of fh_set_env_sampling, its quantisation and CDFs, the draw from it, the
// mixture density and the host-side refusals.  Shared by envmap.hip (the build kernels), render.hip (the ENV variants of shade_hit), kat.hip (fh_kat_env_*), capi.hip
// (fh_set_env_sampling) and the stand-alone program of tests/test_env_sampling_host.py.  The arithmetic is the one include/fredholm_hip.h states under
// fh_env_sampling_params: fp32 without contraction, / and sqrt correctly rounded, everything in the order written; the CDF entries and cell probabilities are quotients
// of integers formed in double and rounded once.  The reference has no counterpart (pt.cu:796-815 leaves it as a TODO).
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/fh_elementary.h"
#include "../../include/fredholm_hip.h"

#if defined(__HIPCC__)
#define FH_EV __host__ __device__ __forceinline__
#else
#define FH_EV inline
#endif

namespace fh {

constexpr int kEnvW = 512, kEnvH = 256;          // cells in phi, in theta
constexpr int kEnvCells = kEnvW * kEnvH;
constexpr int kEnvRowCdf = kEnvW + 1;            // entries of one row's conditional CDF (first 0, last 1)
constexpr float kEnvPi = 3.14159265358979323846f;
constexpr float kEnvTwoPi = 2.0f * kEnvPi;
constexpr float kEnvQuant = 1048576.0f;          // 2^20: a cell's weight against the table's maximum
constexpr float kEnvSinFloor = 9.5367431640625e-7f;  // 2^-20: sin theta of the density is not taken below this (the poles)
constexpr float kEnvBelowOne = 0.99999994f;      // largest float below 1: the position inside a cell stays inside it

// the table as the kernels see it (device pointers) and as the host program builds it (host pointers)
struct EnvTable {
  const float* cdf_row;   // [kEnvH][kEnvRowCdf]  conditional CDF of phi given the row
  const float* cdf_m;     // [kEnvH + 1]          marginal CDF of the rows
  const float* cell_p;    // [kEnvH][kEnvW]       probability of a cell: weight / total
  float beta;             // cosine fraction of the mixture
};

struct EnvDir { float x, y, z; };

FH_EV uint32_t env_subsamples(uint32_t ibl_w) { const uint32_t k = (ibl_w + (uint32_t)kEnvW - 1u) / (uint32_t)kEnvW; return k < 2u ? 2u : (k > 16u ? 16u : k); }

// direction of the table position (u, v) in [0, 1)^2: the inverse of env_radiance's direction -> (phi / 2 pi, theta / pi)
FH_EV EnvDir env_direction(float u, float v, float* sin_theta)
{
  float st, ct, sp, cp;
  fhe_sincos(v * kEnvPi, &st, &ct);
  fhe_sincos(u * kEnvTwoPi, &sp, &cp);
  if (sin_theta) *sin_theta = st;
  return EnvDir{st * cp, ct, st * sp};
}
// sub-sample (a, b) of K x K in cell (i, j)
FH_EV void env_subsample_uv(int i, int j, int a, int b, int k, float* u, float* v)
{
  *u = ((float)i + ((float)a + 0.5f) / (float)k) / (float)kEnvW;
  *v = ((float)j + ((float)b + 0.5f) / (float)k) / (float)kEnvH;
}
FH_EV float env_finite(float v) { return (v != v || fabsf(v) > 3.0e38f) ? 0.0f : v; }
FH_EV float env_lum(float r, float g, float b) { return (env_finite(r) * 0.2126729f + env_finite(g) * 0.7151522f) + env_finite(b) * 0.0721750f; }
// what one sub-sample adds to its cell's sum: the luminance there (1 for a constant background), never negative, times sin theta
FH_EV float env_sample_weight(float l, float sin_theta) { return fminf(fmaxf(l, 0.0f), 3.0e38f) * fmaxf(sin_theta, 0.0f); }
// the cell's weight from the serial sum of its k * k sub-samples (b outer, a inner); a sum that overflowed stays finite
FH_EV float env_cell_mean(float sum, int k) { return fminf(sum / (float)(k * k), 3.0e38f); }
// the integer weight of a cell; w_max == 0 (a black environment): every cell 1
FH_EV uint32_t env_quantise(float w, float w_max)
{
  if (!(w_max > 0.0f)) return 1u;
  const uint32_t q = (uint32_t)((w / w_max) * kEnvQuant);
  return q < 1u ? 1u : q;
}
FH_EV float env_ratio(uint64_t num, uint64_t den) { return (float)((double)num / (double)den); }

// the interval of `cdf` (n + 1 ascending entries, cdf[0] = 0, cdf[n] = 1) that holds u in [0, 1): the largest k with cdf[k] <= u, by bisection
FH_EV int env_search(const float* cdf, int n, float u)
{
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cdf[mid] <= u) lo = mid; else hi = mid;
  }
  return lo;
}
// position of u inside interval k, in [0, 1)
FH_EV float env_remap(const float* cdf, int k, float u) { return fminf((u - cdf[k]) / (cdf[k + 1] - cdf[k]), kEnvBelowOne); }

// the mixture density of direction d for a surface whose shading normal is n, d lying in cell `cell` (j * kEnvW + i)
FH_EV float env_mixture_pdf(const EnvTable& t, uint32_t cell, EnvDir d, EnvDir n)
{
  const float st = fmaxf(fhe_sqrt(d.x * d.x + d.z * d.z), kEnvSinFloor);
  const float cosn = d.x * n.x + d.y * n.y + d.z * n.z;
  const float pt = (t.cell_p[cell] * (float)kEnvCells) / ((2.0f * (kEnvPi * kEnvPi)) * st);
  return (1.0f - t.beta) * pt + t.beta * (fmaxf(cosn, 0.0f) / kEnvPi);
}
// the cell a direction lies in, through env_radiance's mapping
FH_EV uint32_t env_cell_of(EnvDir d)
{
  const float theta = fhe_acos(fmaxf(-1.0f, fminf(d.y, 1.0f)));
  float phi = fhe_atan2(d.z, d.x);
  if (phi < 0) phi += kEnvTwoPi;
  const float fi = (phi / kEnvTwoPi) * (float)kEnvW, fj = (theta / kEnvPi) * (float)kEnvH;
  const int i = fi >= (float)(kEnvW - 1) ? kEnvW - 1 : (fi > 0.0f ? (int)fi : 0), j = fj >= (float)(kEnvH - 1) ? kEnvH - 1 : (fj > 0.0f ? (int)fj : 0);
  return (uint32_t)(j * kEnvW + i);
}
// evaluator: density of any world direction
FH_EV float env_pdf(const EnvTable& t, EnvDir d, EnvDir n, uint32_t* cell)
{
  const uint32_t c = env_cell_of(d);
  if (cell) *cell = c;
  return env_mixture_pdf(t, c, d, n);
}
// which branch the sky slot's draw takes, and the rescaled first coordinate: true = cosine hemisphere
FH_EV bool env_select_cosine(float beta, float* ux)
{
  if (*ux < beta) { *ux = *ux / beta; return true; }
  *ux = fminf((*ux - beta) / (1.0f - beta), kEnvBelowOne);
  return false;
}
// the table branch: row by the marginal from ux, column by the row's conditional from uy, a continuous position inside the cell
FH_EV EnvDir env_sample_table(const EnvTable& t, float ux, float uy, EnvDir n, float* pdf, uint32_t* cell)
{
  const int j = env_search(t.cdf_m, kEnvH, ux);
  const float* row = t.cdf_row + (size_t)j * kEnvRowCdf;
  const int i = env_search(row, kEnvW, uy);
  const float v = ((float)j + env_remap(t.cdf_m, j, ux)) / (float)kEnvH;
  const float u = ((float)i + env_remap(row, i, uy)) / (float)kEnvW;
  const EnvDir d = env_direction(u, v, nullptr);
  const uint32_t c = (uint32_t)(j * kEnvW + i);
  *cell = c;
  *pdf = env_mixture_pdf(t, c, d, n);
  return d;
}

// ---- host only
// the whole build as the kernels of envmap.hip run it in parallel, in a loop: w = the kEnvCells cell means; out: q [kEnvCells], cdf_row, cdf_m, cell_p as in EnvTable
inline void env_build_host(const float* w, uint32_t* q, float* cdf_row, float* cdf_m, float* cell_p)
{
  float w_max = 0.0f;
  for (int c = 0; c < kEnvCells; ++c) w_max = fmaxf(w_max, w[c]);
  uint64_t total = 0;
  uint32_t row_sum[kEnvH];
  for (int j = 0; j < kEnvH; ++j) {
    uint32_t s = 0;
    for (int i = 0; i < kEnvW; ++i) { q[j * kEnvW + i] = env_quantise(w[j * kEnvW + i], w_max); s += q[j * kEnvW + i]; }
    row_sum[j] = s;
    total += s;
  }
  uint64_t run = 0;
  for (int j = 0; j < kEnvH; ++j) {
    cdf_m[j] = env_ratio(run, total);
    run += row_sum[j];
    uint32_t p = 0;
    for (int i = 0; i < kEnvW; ++i) {
      cdf_row[j * kEnvRowCdf + i] = env_ratio(p, row_sum[j]);
      p += q[j * kEnvW + i];
      cell_p[j * kEnvW + i] = env_ratio(q[j * kEnvW + i], total);
    }
    cdf_row[j * kEnvRowCdf + kEnvW] = 1.0f;
  }
  cdf_m[kEnvH] = 1.0f;
}

// nullptr: acceptable (params == nullptr switches off)
inline const char* env_sampling_refusal(const fh_env_sampling_params* p)
{
  if (!p) return nullptr;
  if (!(p->cosine_fraction >= 0.0f && p->cosine_fraction < 1.0f)) return "cosine_fraction must be in [0, 1)";
  return nullptr;
}

}  // namespace fh

#if defined(__HIPCC__)
#include "fh_sampler.h"
namespace fh {
FH_HD EnvDir env_dir(f3 v) { return EnvDir{v.x, v.y, v.z}; }
// the sky slot's draw while the switch is on: world direction, its mixture density and the cell the density was taken from
FH_HD f3 env_sample(const EnvTable& t, f2 u, f3 tangent, f3 ns, f3 bitangent, float& pdf, uint32_t& cell)
{
  float ux = u.x;
  if (env_select_cosine(t.beta, &ux)) {
    const f3 d = to_world(cosine_hemisphere(mk2(ux, u.y)), tangent, ns, bitangent);
    pdf = env_pdf(t, env_dir(d), env_dir(ns), &cell);
    return d;
  }
  const EnvDir d = env_sample_table(t, ux, u.y, env_dir(ns), &pdf, &cell);
  return mk3(d.x, d.y, d.z);
}
}  // namespace fh
#endif
