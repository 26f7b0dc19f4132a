// denoise.hip -- the variance-guided denoiser (fh_denoise_guided): the spatial filter of SVGF (Schied et al., HPG 2017) on albedo-demodulated radiance.
//
// Where the slot's a-trous filter (post.hip: k_atrous) stops at colour edges by the colour distance relative to the local level, this one divides the
// luminance distance by the standard deviation the pixel is KNOWN to have: from the luminance moments adaptive sampling keeps (fh_get_luminance_moments,
// fh_get_sample_counts), or, without them, from a 7x7 normal-weighted spatial estimate.  The variance is filtered along with the colour (weights squared),
// so every pass sees the noise its predecessors left.  The normative statement of the arithmetic is in include/fredholm_hip.h; everything is fp32 without
// contraction, exp is fhe_exp and sqrt is correctly rounded, so a float32 restatement in the same tap order gives the same bits.
//
// Shape of a pass with hole s = 2^i: the 25 taps of pixel p lie at p + s * (dx, dy), so the pixels of one residue class mod s form a dense lattice whose taps
// are lattice neighbours.  A workgroup owns 32 x 8 pixels of ONE class, {x0 + s * u, y0 + s * v}; their taps are the 36 x 12 lattice points around them, which
// it stages once into LDS (14 floats per point: colour, variance, normal, luminance, albedo, position) and then reads 25 times per pixel, where k_atrous fetches three
// float4 per tap from global memory.  A 16-lane group of ds_read_b128 (MI355X: lanes {0-3, 12-15, 20-27} and so on) lies within one 32-pixel row of the tile
// and reads 16 consecutive float4: all 64 banks once, whatever the row pitch.  The variance also lives in a float plane of its own: the 3x3 prefilter reads
// DENSE neighbours, which the lattice does not hold.
#include <hip/hip_runtime.h>

#include <cmath>

#include "context.h"
#include "fh_tonemap.h"

namespace fh {
namespace {

constexpr int kTW = 32, kTH = 8;                 // pixels of a residue class per workgroup
constexpr int kGW = kTW + 4, kGH = kTH + 4;      // staged lattice points
constexpr int kGN = kGW * kGH;
constexpr float kAlbedoFloor = 0.01f;
constexpr unsigned kXcds = 8;                   // MI355X

__device__ __forceinline__ float gd_finite(float v) { return (v != v || fabsf(v) > 3.0e38f) ? 0.0f : v; }  // dn_finite of post.hip
__device__ __forceinline__ int gd_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
// fhe_exp (fh_elementary.h) with its three range checks as selects after the polynomial, not as branches around it: the same operations on every argument
// fhe_exp evaluates it for, hence the same bits, and 24 taps without 72 branches.  (Outside the range the polynomial's value is discarded.)
__device__ __forceinline__ float gd_exp(float x)
{
  const float n = fhe_rint(x * 1.44269504088896341f);
  float r = fmaf(-n, 0.693359375f, x);
  r = fmaf(-n, -2.12194440e-4f, r);
  float p = fmaf(r, 1.9875691500e-4f, 1.3981999507e-3f);
  p = fmaf(r, p, 8.3334519073e-3f);
  p = fmaf(r, p, 4.1665795894e-2f);
  p = fmaf(r, p, 1.6666665459e-1f);
  p = fmaf(r, p, 5.0000001201e-1f);
  const float e = fmaf(r * r, p, r) + 1.0f;
  const int ni = (int)n;
  const int n1 = ni / 2, n2 = ni - n1;
  const float f1 = fhe_u2f((uint32_t)(n1 + 127) << 23);
  const float f2 = fhe_u2f((uint32_t)(n2 + 127) << 23);
  float in_range = (e * f1) * f2;
  asm("" : "+v"(in_range));  // (an empty statement the value has to pass through: keeps the compiler from moving the polynomial back under branches)
  float y = x < -103.972084045410f ? 0.0f : in_range;
  y = x > 88.72283905206835f ? INFINITY : y;
  return x != x ? x : y;
}

// max(0, d) squared power_log2 times; NP >= 0: the count is known when the kernel is compiled (no loop per tap)
template <int NP = -1>
__device__ __forceinline__ float gd_normal_weight(float d, uint32_t power_log2)
{
  float wn = fmaxf(0.0f, d);
  if constexpr (NP >= 0) {
#pragma unroll
    for (int k = 0; k < NP; ++k) wn = wn * wn;
  } else {
    for (uint32_t k = 0; k < power_log2; ++k) wn = wn * wn;
  }
  return wn;
}

// demodulated radiance c and its luminance l; with moments also the variance of l (MOMENTS: out = (c, v), and v into the plane; else out = (c, l))
template <bool MOMENTS>
__global__ void __launch_bounds__(256) k_guided_prepare(const float4* beauty, const float4* albedo, const float2* moments, const uint32_t* counts, int n_px, float4* out, float* vplane)
{
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n_px) return;
  const float4 b = beauty[p], a = albedo[p];
  const float cx = gd_finite(b.x) / fmaxf(a.x, kAlbedoFloor), cy = gd_finite(b.y) / fmaxf(a.y, kAlbedoFloor), cz = gd_finite(b.z) / fmaxf(a.z, kAlbedoFloor);
  const float l = luminance_rgb(cx, cy, cz);
  if constexpr (!MOMENTS) {
    out[p] = make_float4(cx, cy, cz, l);
  } else {
    const float2 m = moments[p];
    const uint32_t n = counts[p];
    float v = l * l;
    if (n >= 2u) {
      const float r = l / fmaxf(m.x, 1e-3f);
      v = fmaxf(m.y - m.x * m.x, 0.0f) / (float)(n - 1u) * (r * r);
    }
    out[p] = make_float4(cx, cy, cz, v);
    vplane[p] = v;
  }
}

// without moments: the variance of l over the 7x7 clamped window, weighted by the normal stop
__global__ void __launch_bounds__(256) k_guided_spatial_variance(const float4* cl, const float4* normal, int w, int h, uint32_t power_log2, float4* out, float* vplane)
{
  const int x = blockIdx.x * 32 + threadIdx.x, y = blockIdx.y * 8 + threadIdx.y;
  if (x >= w || y >= h) return;
  const int p = x + w * y;
  const float4 np = normal[p];
  float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
  for (int dy = -3; dy <= 3; ++dy)
    for (int dx = -3; dx <= 3; ++dx) {
      const int q = gd_clamp(x + dx, w - 1) + w * gd_clamp(y + dy, h - 1);
      const float4 nq = normal[q];
      const float lq = cl[q].w;
      const float wn = gd_normal_weight<>(np.x * nq.x + np.y * nq.y + np.z * nq.z, power_log2);
      s0 += wn; s1 += wn * lq; s2 += wn * (lq * lq);
    }
  const float S = fmaxf(s0, 1e-6f), m1 = s1 / S, m2 = s2 / S;
  const float v = fmaxf(m2 - m1 * m1, 0.0f);
  const float4 c = cl[p];
  out[p] = make_float4(c.x, c.y, c.z, v);
  vplane[p] = v;
}

struct GuidedArgs {
  const float4* cv;       // (c.rgb, v) of the previous pass
  const float* vplane;    // v again, dense
  const float4* normal;
  const float4* albedo;
  const float4* position; // POS only
  const float* depth;     // POS only
  float4* cv_out;         // !LAST
  float* vplane_out;      // !LAST
  float4* image_out;      // LAST
  int w, h, shift;        // hole s = 1 << shift
  float sigma_l, sigma_z, sa2;
  uint32_t power_log2;
  int upscale;
  unsigned groups_x, groups_y;  // workgroups of the pass: tiles x residues
};

// NP: normal_power_log2 when it is the default, else -1 (read from the arguments)
template <bool POS, bool LAST, int NP>
__global__ void __launch_bounds__(256) k_guided_pass(const GuidedArgs A)
{
  __shared__ float4 s_cv[kGN];   // c.rgb, v
  __shared__ float4 s_n[kGN];    // N.xyz, lum(c)
  __shared__ float4 s_a[kGN];    // A.rgb, P.x
  __shared__ float2 s_p[POS ? kGN : 1];  // P.y, P.z
  const int w = A.w, h = A.h, s = 1 << A.shift, mask = s - 1;
  // The pixels of neighbouring residue classes lie in the same cache lines (a workgroup takes 16 bytes per plane of every line it touches), and the dispatcher
  // deals consecutive workgroups out to the eight XCDs, each with an L2 of its own: so renumber, giving each XCD (blockIdx % 8) a contiguous run of the
  // (tile, residue) order, residue fastest.  Its neighbouring classes then run on it one after the other and find the lines in its L2.  (Only speed depends on this.)
  const unsigned run = gridDim.x / kXcds, id = (blockIdx.x % kXcds) * run + blockIdx.x / kXcds;
  if (id >= A.groups_x * A.groups_y) return;  // (the whole workgroup: the grid is rounded up to a multiple of 8)
  const int bx = (int)(id % A.groups_x), by = (int)(id / A.groups_x);
  const int x0 = (bx >> A.shift) * (kTW * s) + (bx & mask);
  const int y0 = (by >> A.shift) * (kTH * s) + (by & mask);
  if (x0 >= w || y0 >= h) return;  // (the whole workgroup)
  const int tid = threadIdx.y * kTW + threadIdx.x;
  for (int k = tid; k < kGN; k += 256) {
    const int gx = k % kGW, gy = k / kGW;
    const int q = gd_clamp(x0 + (gx - 2) * s, w - 1) + w * gd_clamp(y0 + (gy - 2) * s, h - 1);
    const float4 n = A.normal[q], a = A.albedo[q];
    float4 P = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if constexpr (POS) P = A.position[q];
    const float4 cv = A.cv[q];
    s_cv[k] = cv;
    s_n[k] = make_float4(n.x, n.y, n.z, luminance_rgb(cv.x, cv.y, cv.z));
    s_a[k] = make_float4(a.x, a.y, a.z, P.x);
    if constexpr (POS) s_p[k] = make_float2(P.y, P.z);
  }
  __syncthreads();
  const int x = x0 + (int)threadIdx.x * s, y = y0 + (int)threadIdx.y * s;
  if (x >= w || y >= h) return;
  const int p = x + w * y;
  // sd_p from the 3x3 binomial of the variance over the dense neighbours
  float g = 0.0f;
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) {
      const float bw = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
      g += bw * A.vplane[gd_clamp(x + dx, w - 1) + w * gd_clamp(y + dy, h - 1)];
    }
  const float sd = A.sigma_l * fhe_sqrt(g) + 1e-6f;
  const int kc = (threadIdx.y + 2) * kGW + threadIdx.x + 2;
  const float4 np = s_n[kc], ap = s_a[kc];
  const float lp = np.w;
  float2 pp = make_float2(0.0f, 0.0f);
  float kz = 0.0f;
  if constexpr (POS) {
    pp = s_p[kc];
    kz = A.sigma_z * 0.01f * fmaxf(A.depth[p], 1e-3f) * (float)s;
  }
  const float kern[3] = {3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
  float sx = 0.0f, sy = 0.0f, sz = 0.0f, sw = 0.0f, sv = 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int k = kc + dy * kGW + dx;
      const float4 cq = s_cv[k];
      float wgt = 9.0f / 64.0f;
      if (dx != 0 || dy != 0) {
        const float4 nq = s_n[k], aq = s_a[k];
        const float wn = gd_normal_weight<NP>(np.x * nq.x + np.y * nq.y + np.z * nq.z, A.power_log2);
        float ez = 0.0f;
        if constexpr (POS) {
          const float2 pq = s_p[k];
          const float ddx = aq.w - ap.w, ddy = pq.x - pp.x, ddz = pq.y - pp.y;
          ez = fabsf(np.x * ddx + np.y * ddy + np.z * ddz) / (kz * fhe_sqrt((float)(dx * dx + dy * dy)) + 1e-6f);
        }
        const float dax = aq.x - ap.x, day = aq.y - ap.y, daz = aq.z - ap.z;
        const float ea = (dax * dax + day * day + daz * daz) / A.sa2;
        const float el = fabsf(nq.w - lp) / sd;
        wgt = kern[dx < 0 ? -dx : dx] * kern[dy < 0 ? -dy : dy] * wn * gd_exp(-(ez + ea + el));
      }
      sx += wgt * cq.x; sy += wgt * cq.y; sz += wgt * cq.z; sw += wgt; sv += wgt * wgt * cq.w;
    }
  const float ox = sx / sw, oy = sy / sw, oz = sz / sw;  // the centre tap has weight 9/64: never zero
  if constexpr (!LAST) {
    const float v = sv / (sw * sw);
    A.cv_out[p] = make_float4(ox, oy, oz, v);
    A.vplane_out[p] = v;
  } else {
    const float4 o = make_float4(ox * fmaxf(ap.x, kAlbedoFloor), oy * fmaxf(ap.y, kAlbedoFloor), oz * fmaxf(ap.z, kAlbedoFloor), 1.0f);
    if (!A.upscale) { A.image_out[p] = o; return; }
    float4* d = A.image_out + (size_t)(2 * w) * (size_t)(2 * y) + (size_t)(2 * x);  // (32768^2 pixels: the doubled image is past 2^31 elements)
    d[0] = o; d[1] = o; d[2 * w] = o; d[2 * w + 1] = o;
  }
}

template <bool POS, int NP>
void launch_pass(const GuidedArgs& a, bool last, dim3 grid, hipStream_t st)
{
  if (last) hipLaunchKernelGGL((k_guided_pass<POS, true, NP>), grid, dim3(kTW, kTH), 0, st, a);
  else hipLaunchKernelGGL((k_guided_pass<POS, false, NP>), grid, dim3(kTW, kTH), 0, st, a);
}

}  // namespace

int denoise_guided_submit(fh_ctx* ctx, int w, int h, const fh_denoise_inputs* in, const fh_denoise_params* pr, float* out, int upscale)
{
  hipStream_t st = ctx->stream;
  const size_t px = (size_t)w * h;
  if (ctx->guided_pixels < px) {  // two (c, v) images and two variance planes, kept in the context
    for (int k = 0; k < 2; ++k) {
      if (ctx->d_guided_cv[k]) (void)hipFree(ctx->d_guided_cv[k]);
      if (ctx->d_guided_var[k]) (void)hipFree(ctx->d_guided_var[k]);
      ctx->d_guided_cv[k] = nullptr; ctx->d_guided_var[k] = nullptr;
    }
    ctx->guided_pixels = 0;
    for (int k = 0; k < 2; ++k) {
      FH_HIP(hipMalloc((void**)&ctx->d_guided_cv[k], px * sizeof(float4)));
      FH_HIP(hipMalloc((void**)&ctx->d_guided_var[k], px * sizeof(float)));
    }
    ctx->guided_pixels = px;
  }
  const float4 *beauty = (const float4*)in->beauty, *normal = (const float4*)in->normal, *albedo = (const float4*)in->albedo;
  const dim3 lin((unsigned)((px + 255) / 256));
  if (in->moments) {
    hipLaunchKernelGGL((k_guided_prepare<true>), lin, dim3(256), 0, st, beauty, albedo, (const float2*)in->moments, in->counts, (int)px, ctx->d_guided_cv[0], ctx->d_guided_var[0]);
  } else {
    hipLaunchKernelGGL((k_guided_prepare<false>), lin, dim3(256), 0, st, beauty, albedo, (const float2*)nullptr, (const uint32_t*)nullptr, (int)px, ctx->d_guided_cv[1], (float*)nullptr);
    hipLaunchKernelGGL(k_guided_spatial_variance, dim3((w + 31) / 32, (h + 7) / 8), dim3(32, 8), 0, st, (const float4*)ctx->d_guided_cv[1], normal, w, h, pr->normal_power_log2,
                       ctx->d_guided_cv[0], ctx->d_guided_var[0]);
  }
  GuidedArgs a{};
  a.normal = normal; a.albedo = albedo; a.position = (const float4*)in->position; a.depth = in->depth;
  a.w = w; a.h = h; a.sigma_l = pr->sigma_l; a.sigma_z = pr->sigma_z; a.sa2 = pr->sigma_a * pr->sigma_a; a.power_log2 = pr->normal_power_log2; a.upscale = upscale;
  for (uint32_t it = 0; it < pr->passes; ++it) {
    const bool last = it + 1 == pr->passes;
    const int s = 1 << it;
    a.cv = ctx->d_guided_cv[it & 1]; a.vplane = ctx->d_guided_var[it & 1];
    a.cv_out = ctx->d_guided_cv[(it + 1) & 1]; a.vplane_out = ctx->d_guided_var[(it + 1) & 1];
    a.image_out = (float4*)out; a.shift = (int)it;
    a.groups_x = (unsigned)(((w + kTW * s - 1) / (kTW * s)) * s); a.groups_y = (unsigned)(((h + kTH * s - 1) / (kTH * s)) * s);
    const dim3 grid((a.groups_x * a.groups_y + kXcds - 1) / kXcds * kXcds);
    const bool np_default = pr->normal_power_log2 == 7;
    if (in->position) { if (np_default) launch_pass<true, 7>(a, last, grid, st); else launch_pass<true, -1>(a, last, grid, st); }
    else { if (np_default) launch_pass<false, 7>(a, last, grid, st); else launch_pass<false, -1>(a, last, grid, st); }
  }
  FH_HIP(hipGetLastError());
  return FH_OK;
}

}  // namespace fh
