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
//
// fh_denoise_temporal runs the same preparation and the same passes with one launch between them, k_temporal below: the frame's (c, v) blended with the context's
// history of the frames before it, found again through the world position and the previous call's camera.  k_temporal<LOOK, CLIP, MOM> is one template.  LOOK is how the
// history is found: fh_denoise_temporal_motion, where an instance moved, carries the pixels of moved instances to where their surface was.  CLIP is what happens to it
// before the blend: while fh_set_denoise_response is on it is clamped to the current frame's local colour statistics, and with fh_set_denoise_response_noise on as well
// and moments given, also to the pixel's own measured noise.  MOM (fh_set_denoise_temporal_moments): the history also holds the luminance moments (mu1, mu2), looked up and
// blended like the colour, and a call without sample moments takes its variance from them where the history is long enough.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "context.h"
#include "fh_tonemap.h"
#include "motion_host.h"

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

// ---- the temporal stage of fh_denoise_temporal (include/fredholm_hip.h states it operation by operation): one streaming launch between the preparation and the passes.
// A pixel reads its own (c, v), N, P, Z, looks its history up -- at itself when the camera stood still, else at the 2 x 2 taps around where the previous camera saw
// P -- blends, and writes the new history, which is also what the first pass reads.  32 x 8 pixels per workgroup like the passes: a wave is two rows of 32, whose taps
// after a small camera step are again two or three rows of neighbouring 16-byte elements in each of the three history images.
//
// One kernel template, k_temporal<LOOK, CLIP, MOM>, whose parts below are each written once; the host picks the instance (the choice is the same for every pixel).  The build
// is fp32 without contraction, so a part gives the same bits in every instance it is inlined into, and the GPU suites hold each instance to the restatement's bits.
// LOOK is one of kLookNone .. kLookMotion, CLIP one of kClipOff .. kClipColourNoise (temporal_host.h, beside the plan that picks them).

struct TemporalArgs {
  const float4* cv;       // (c.rgb, v) of the preparation
  const float4* normal;
  const float4* position;
  const float* depth;
  const float4* h_cv;     // the history read (LOOK != kLookNone): (c_acc.rgb, v_acc)
  const float4* h_ph;     // (P, h)
  const float4* h_n;      // N
  float4* o_cv;           // the history written; o_cv is the (c, v) image of the first pass
  float4* o_ph;
  float4* o_n;
  float* vplane;          // v_acc, dense, for the first pass
  int w, h;
  float m[12];            // world-to-camera rows of the camera the history was written with
  float f, W, H;          // its cam_inv_tan; width and height as floats
  float alpha_min, max_history, cos_min, plane_tol;
  // kLookMotion
  const uint32_t* ids;     // the instance each pixel's chief ray sees (fh_primary_instances)
  const fh_motion* motion; // n_instances entries, on the device
  uint32_t n_instances;
  int still;               // the camera has the stored camera's bits
  float gamma, kappa;      // CLIP: fh_set_denoise_response, fh_set_denoise_response_noise
  // MOM (fh_set_denoise_temporal_moments): at the end, so that the instances without it keep their argument offsets
  const float2* h_mu;      // the history read: the luminance moments (mu1, mu2)
  float2* o_mu;            // the history written
  float min_history;       // the history length from which the temporal variance replaces the preparation's
  int replace_v;           // the call has no sample moments: v may be replaced
};
// what a pixel found of its history: colour, variance, length
struct History { float x, y, z, v, h; };
// ... and, with MOM, the luminance moments; without it the type is empty, and the instances without moments are the code they were
template <bool MOM> struct Moments {};
template <> struct Moments<true> { float x = 0.0f, y = 0.0f; };

__device__ __forceinline__ bool td_hit(const float4 n) { return n.x != 0.0f || n.y != 0.0f || n.z != 0.0f; }
// the two stops of a history tap (its normal nq and position ph.xyz) seen from the pixel (np, pp); lim = plane_tol * max(Z_p, 1e-3)
__device__ __forceinline__ bool td_valid(const TemporalArgs& A, const float4 np, const float4 pp, float lim, const float4 nq, const float4 ph)
{
  const float dn = (np.x * nq.x + np.y * nq.y) + np.z * nq.z;
  const float dx = ph.x - pp.x, dy = ph.y - pp.y, dz = ph.z - pp.z;
  const float dp = fabsf((np.x * dx + np.y * dy) + np.z * dz);
  return td_hit(nq) && dn >= A.cos_min && dp <= lim;
}

// the still camera's look-up: the pixel's own history, if it passes the two stops; false: no history
template <bool MOM>
__device__ __forceinline__ bool td_own_tap(const TemporalArgs& A, int p, const float4 np, const float4 pp, float lim, History& H, Moments<MOM>& mu)
{
  const float4 qc = A.h_cv[p], qp = A.h_ph[p], qn = A.h_n[p];
  H = {qc.x, qc.y, qc.z, qc.w, qp.w};
  if constexpr (MOM) { const float2 qm = A.h_mu[p]; mu.x = qm.x; mu.y = qm.y; }
  return td_valid(A, np, pp, lim, qn, qp);
}

// the moved camera's look-up: where the stored camera saw pp, the 2 x 2 taps around it that pass the two stops seen from (np, pp), renormalised; false: no history
template <bool MOM>
__device__ __forceinline__ bool td_reproject(const TemporalArgs& A, const float4 np, const float4 pp, float lim, History& H, Moments<MOM>& mu)
{
  bool have = false;
  const float qx = ((A.m[0] * pp.x + A.m[1] * pp.y) + A.m[2] * pp.z) + A.m[3];
  const float qy = ((A.m[4] * pp.x + A.m[5] * pp.y) + A.m[6] * pp.z) + A.m[7];
  const float qz = ((A.m[8] * pp.x + A.m[9] * pp.y) + A.m[10] * pp.z) + A.m[11];
  const float t = (A.f - qz) / A.f;
  if (t > 0.0f) {
    const float xs = (A.W + (A.H * qx) / t) * 0.5f - 0.5f, ys = (A.H - (A.H * qy) / t) * 0.5f - 0.5f;
    const float ix = floorf(xs), iy = floorf(ys), fx = xs - ix, fy = ys - iy;
    float S = 0.0f;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const float tx = ix + (float)i, ty = iy + (float)j;
        const bool inside = tx >= 0.0f && tx <= A.W - 1.0f && ty >= 0.0f && ty <= A.H - 1.0f;  // (false for NaN: the clamps below then give pixel 0)
        const int q = (int)fminf(fmaxf(tx, 0.0f), A.W - 1.0f) + A.w * (int)fminf(fmaxf(ty, 0.0f), A.H - 1.0f);
        const float4 qc = A.h_cv[q], qp = A.h_ph[q], qn = A.h_n[q];
        Moments<MOM> qm;
        if constexpr (MOM) { const float2 t = A.h_mu[q]; qm.x = t.x; qm.y = t.y; }
        const float wgt = (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy);
        if (inside && td_valid(A, np, pp, lim, qn, qp)) {
          S += wgt; H.x += wgt * qc.x; H.y += wgt * qc.y; H.z += wgt * qc.z; H.v += wgt * qc.w; H.h += wgt * qp.w;
          if constexpr (MOM) { mu.x += wgt * qm.x; mu.y += wgt * qm.y; }
        }
      }
    have = S >= 1e-3f;
    H.x = H.x / S; H.y = H.y / S; H.z = H.z / S; H.v = H.v / S; H.h = H.h / S;
    if constexpr (MOM) { mu.x = mu.x / S; mu.y = mu.y / S; }
  }
  return have;
}

// the look-up of a pixel that hit something (H and mu come in as zeros).  kLookMotion (the header states it): a pixel of an instance that moved is CARRIED to where its
// surface was, by the instance's affine map, and is reprojected from there whatever the camera did; the other pixels take their own tap under a still camera and the
// reprojection otherwise.  It reads 4 more bytes per pixel than kLookReproject and an 88-byte table entry that a wave shares.
template <int LOOK, bool MOM>
__device__ __forceinline__ bool td_lookup(const TemporalArgs& A, int p, const float4 np, const float4 pp, History& H, Moments<MOM>& mu)
{
  if constexpr (LOOK == kLookNone) {
    return false;
  } else {
    const float lim = A.plane_tol * fmaxf(A.depth[p], 1e-3f);
    bool own = LOOK == kLookOwn;
    float4 nb = np, pb = pp;
    if constexpr (LOOK == kLookMotion) {
      const uint32_t inst = A.ids[p];
      const bool carried = inst < A.n_instances && A.motion[inst < A.n_instances ? inst : 0u].moved != 0u;
      own = !carried && A.still;
      if (carried) {
        const float* a = A.motion[inst].point;
        const float* g = A.motion[inst].normal;
        pb.x = ((a[0] * pp.x + a[1] * pp.y) + a[2] * pp.z) + a[3];
        pb.y = ((a[4] * pp.x + a[5] * pp.y) + a[6] * pp.z) + a[7];
        pb.z = ((a[8] * pp.x + a[9] * pp.y) + a[10] * pp.z) + a[11];
        nb.x = (g[0] * np.x + g[1] * np.y) + g[2] * np.z;
        nb.y = (g[3] * np.x + g[4] * np.y) + g[5] * np.z;
        nb.z = (g[6] * np.x + g[7] * np.y) + g[8] * np.z;
      }
    }
    return own ? td_own_tap<MOM>(A, p, np, pp, lim, H, mu) : td_reproject<MOM>(A, nb, pb, lim, H, mu);
  }
}

// the clip (fh_set_denoise_response; the header states it step by step): the history a pixel found is clamped, before the blend, to mean +- gamma * standard deviation
// of the CURRENT frame's colour over the pixel's 5 x 5 window, and shortened by how far outside that box it lay.  The 25 taps come from the staged tile (k_temporal);
// kc: the pixel's place in it; cv: its own (c, v).  kClipColourNoise (fh_set_denoise_response_noise, step 4b): the clipped history is clamped once more, to the pixel's
// own colour +- kappa standard deviations of what it measured -- the preparation's variance v plus the history's v_h, both in registers already -- and shortened by the
// larger of the two excesses.  No new load, no more LDS.
template <int CLIP>
__device__ __forceinline__ void td_clip(const TemporalArgs& A, const float4* s_cv, const float4* s_n, int kc, const float4 np, const float4 cv, History& H)
{
  // 1: the window.  A tap that does not count adds + 0, which changes no bit of a sum that started at + 0.
  float n = 0.0f, s1x = 0.0f, s1y = 0.0f, s1z = 0.0f, s2x = 0.0f, s2y = 0.0f, s2z = 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int k = kc + dy * kGW + dx;
      const float4 cq = s_cv[k], nq = s_n[k];
      const bool counts = (dx == 0 && dy == 0) || (td_hit(nq) && (np.x * nq.x + np.y * nq.y) + np.z * nq.z >= A.cos_min);
      n += counts ? 1.0f : 0.0f;
      s1x += counts ? cq.x : 0.0f; s1y += counts ? cq.y : 0.0f; s1z += counts ? cq.z : 0.0f;
      s2x += counts ? cq.x * cq.x : 0.0f; s2y += counts ? cq.y * cq.y : 0.0f; s2z += counts ? cq.z * cq.z : 0.0f;
    }
  float u = 0.0f;
  if (n >= 2.0f) {  // (3: a window of the pixel alone clips nothing)
    // 2: the box; 4: the clip.  fmaxf and fminf drop a NaN operand.
    const float mx = s1x / n, my = s1y / n, mz = s1z / n;
    const float gx = A.gamma * fhe_sqrt(fmaxf(s2x / n - mx * mx, 0.0f)), gy = A.gamma * fhe_sqrt(fmaxf(s2y / n - my * my, 0.0f)), gz = A.gamma * fhe_sqrt(fmaxf(s2z / n - mz * mz, 0.0f));
    const float ccx = fminf(fmaxf(H.x, mx - gx), mx + gx), ccy = fminf(fmaxf(H.y, my - gy), my + gy), ccz = fminf(fmaxf(H.z, mz - gz), mz + gz);
    const float ux = fabsf(ccx - H.x) / (gx + 1e-6f), uy = fabsf(ccy - H.y) / (gy + 1e-6f), uz = fabsf(ccz - H.z) / (gz + 1e-6f);
    u = fmaxf(fmaxf(ux, uy), uz);
    H.x = ccx; H.y = ccy; H.z = ccz;
  }
  if constexpr (CLIP == kClipColourNoise) {
    // 4b: the noise box around the pixel's own colour, also where step 3 left the history alone; v_h as looked up.  A NaN s drops out of every fmaxf and fminf.
    const float s = A.kappa * fhe_sqrt(cv.w + H.v);
    const float dx = fminf(fmaxf(H.x, cv.x - s), cv.x + s), dy = fminf(fmaxf(H.y, cv.y - s), cv.y + s), dz = fminf(fmaxf(H.z, cv.z - s), cv.z + s);
    const float wx = fabsf(dx - H.x) / (s + 1e-6f), wy = fabsf(dy - H.y) / (s + 1e-6f), wz = fabsf(dz - H.z) / (s + 1e-6f);
    u = fmaxf(u, fmaxf(fmaxf(wx, wy), wz));
    H.x = dx; H.y = dy; H.z = dz;
  }
  if (CLIP == kClipColourNoise || n >= 2.0f) {  // 5: the shortened history (where step 3 left it alone and there is no step 4b, it keeps its length)
    const float k1 = 1.0f + u;
    H.h = H.h / k1; H.v = H.v * k1;
  }
}

// the blend of the frame's (c, v) with the history, if there is one, and the four stores.  MOM: the moments (l, l * l) of the frame's luminance are blended with the
// history's mu (never clipped) by the same weights and stored as well; where the call has no sample moments and the history is min_history long, their variance takes
// the place of the preparation's v
template <bool MOM>
__device__ __forceinline__ void td_blend_store(const TemporalArgs& A, int p, const float4 cv, const float4 np, const float4 pp, bool have, const History& H, const Moments<MOM>& mu)
{
  float cx = cv.x, cy = cv.y, cz = cv.z, v = cv.w, hist = td_hit(np) ? 1.0f : 0.0f;
  Moments<MOM> m;
  if constexpr (MOM) {
    const float l = luminance_rgb(cx, cy, cz);
    m.x = l; m.y = l * l;
  }
  if (have) {
    hist = fminf(H.h + 1.0f, A.max_history);
    const float a = fmaxf(1.0f / hist, A.alpha_min), b = 1.0f - a;
    cx = b * H.x + a * cx; cy = b * H.y + a * cy; cz = b * H.z + a * cz;
    if constexpr (MOM) {
      m.x = b * mu.x + a * m.x; m.y = b * mu.y + a * m.y;
      if (A.replace_v && hist >= A.min_history) v = fmaxf(m.y - m.x * m.x, 0.0f);
    }
    v = (b * b) * H.v + (a * a) * v;
  }
  if constexpr (MOM) A.o_mu[p] = make_float2(m.x, m.y);
  A.o_cv[p] = make_float4(cx, cy, cz, v);
  A.o_ph[p] = make_float4(pp.x, pp.y, pp.z, hist);
  A.o_n[p] = np;
  A.vplane[p] = v;
}

// With the clip, the workgroup's 32 x 8 pixels take their 25 taps from the 36 x 12 tile of (c.rgb, v) and N it stages once: 432 x 32 bytes = 13.5 KiB of LDS.  Neither LDS
// (eleven workgroups a CU) nor the wave slots (eight) limit residency: the 83 VGPRs the unrolled window takes do, at 5 waves per SIMD = 5 workgroups per CU.  A tile
// element outside the frame is staged with N = 0, which is what a miss has: neither counts.  Every thread of a partial tile stages (the loop runs over the tile, not
// over the live pixels) and only then do the threads without a pixel leave.  A row of 32 pixels reads 32 consecutive float4 of a tile row per tap: every bank once per
// 16 lanes.  Without the clip the arrays are never referenced: no LDS, and the pixel's (c, v) and N come from global memory.
template <int LOOK, int CLIP, bool MOM>
__global__ void __launch_bounds__(256) k_temporal(const TemporalArgs A)
{
  static_assert(LOOK != kLookNone || CLIP == kClipOff, "without a history there is nothing to clip");
  constexpr bool kTile = CLIP != kClipOff;
  __shared__ float4 s_cv[kTile ? kGN : 1];  // c.rgb, v of the preparation
  __shared__ float4 s_n[kTile ? kGN : 1];   // N; 0 outside the frame
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  if constexpr (kTile) {
    const int tid = threadIdx.y * kTW + threadIdx.x;
    for (int k = tid; k < kGN; k += 256) {
      const int qx = x0 + k % kGW - 2, qy = y0 + k / kGW - 2;
      float4 cq = make_float4(0.0f, 0.0f, 0.0f, 0.0f), nq = cq;
      if (qx >= 0 && qx < A.w && qy >= 0 && qy < A.h) { cq = A.cv[qx + A.w * qy]; nq = A.normal[qx + A.w * qy]; }
      s_cv[k] = cq;
      s_n[k] = nq;
    }
    __syncthreads();
  }
  const int x = x0 + (int)threadIdx.x, y = y0 + (int)threadIdx.y;
  if (x >= A.w || y >= A.h) return;
  const int p = x + A.w * y;
  const int kc = ((int)threadIdx.y + 2) * kGW + (int)threadIdx.x + 2;
  float4 cv, np;
  if constexpr (kTile) { cv = s_cv[kc]; np = s_n[kc]; } else { cv = A.cv[p]; np = A.normal[p]; }
  const float4 pp = A.position[p];
  History H = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  Moments<MOM> mu;
  bool have = false;
  if (td_hit(np)) {
    have = td_lookup<LOOK, MOM>(A, p, np, pp, H, mu);
    if constexpr (kTile)
      if (have) td_clip<CLIP>(A, s_cv, s_n, kc, np, cv, H);
  }
  td_blend_store<MOM>(A, p, cv, np, pp, have, H, mu);
}

using TemporalLaunch = void (*)(const TemporalArgs&, dim3, hipStream_t);
template <int LOOK, int CLIP, bool MOM>
void temporal_launch(const TemporalArgs& a, dim3 grid, hipStream_t st)
{
  hipLaunchKernelGGL((k_temporal<LOOK, CLIP, MOM>), grid, dim3(kTW, kTH), 0, st, a);
}
// [MOM][LOOK][CLIP]: the twenty instances in use.  Without a history there is nothing to clip: temporal_call_plan never picks an empty entry
constexpr TemporalLaunch kTemporalLaunch[2][4][3] = {
    {{temporal_launch<kLookNone, kClipOff, false>, nullptr, nullptr},
     {temporal_launch<kLookOwn, kClipOff, false>, temporal_launch<kLookOwn, kClipColour, false>, temporal_launch<kLookOwn, kClipColourNoise, false>},
     {temporal_launch<kLookReproject, kClipOff, false>, temporal_launch<kLookReproject, kClipColour, false>, temporal_launch<kLookReproject, kClipColourNoise, false>},
     {temporal_launch<kLookMotion, kClipOff, false>, temporal_launch<kLookMotion, kClipColour, false>, temporal_launch<kLookMotion, kClipColourNoise, false>}},
    {{temporal_launch<kLookNone, kClipOff, true>, nullptr, nullptr},
     {temporal_launch<kLookOwn, kClipOff, true>, temporal_launch<kLookOwn, kClipColour, true>, temporal_launch<kLookOwn, kClipColourNoise, true>},
     {temporal_launch<kLookReproject, kClipOff, true>, temporal_launch<kLookReproject, kClipColour, true>, temporal_launch<kLookReproject, kClipColourNoise, true>},
     {temporal_launch<kLookMotion, kClipOff, true>, temporal_launch<kLookMotion, kClipColour, true>, temporal_launch<kLookMotion, kClipColourNoise, true>}},
};

}  // namespace

namespace {

// two (c, v) images and two variance planes, kept in the context
int guided_scratch(fh_ctx* ctx, size_t px)
{
  if (ctx->d_guided_var[1].size() < px) {  // (the last of the four: all were made)
    for (int k = 0; k < 2; ++k) { ctx->d_guided_cv[k].reset(); ctx->d_guided_var[k].reset(); }
    for (int k = 0; k < 2; ++k) {
      FH_HIP(ctx->d_guided_cv[k].alloc(px));
      FH_HIP(ctx->d_guided_var[k].alloc(px));
    }
  }
  return FH_OK;
}

// (c, v) into d_guided_cv[0] and v into d_guided_var[0]
void guided_prepare(fh_ctx* ctx, int w, int h, const fh_denoise_inputs* in, const fh_denoise_params* pr)
{
  hipStream_t st = ctx->stream;
  const size_t px = (size_t)w * h;
  const float4 *beauty = (const float4*)in->beauty, *normal = (const float4*)in->normal, *albedo = (const float4*)in->albedo;
  const dim3 lin((unsigned)((px + 255) / 256));
  if (in->moments) {
    hipLaunchKernelGGL((k_guided_prepare<true>), lin, dim3(256), 0, st, beauty, albedo, (const float2*)in->moments, in->counts, (int)px, ctx->d_guided_cv[0], ctx->d_guided_var[0]);
  } else {
    hipLaunchKernelGGL((k_guided_prepare<false>), lin, dim3(256), 0, st, beauty, albedo, (const float2*)nullptr, (const uint32_t*)nullptr, (int)px, ctx->d_guided_cv[1], (float*)nullptr);
    hipLaunchKernelGGL(k_guided_spatial_variance, dim3((w + 31) / 32, (h + 7) / 8), dim3(32, 8), 0, st, (const float4*)ctx->d_guided_cv[1], normal, w, h, pr->normal_power_log2,
                       ctx->d_guided_cv[0], ctx->d_guided_var[0]);
  }
}

// the passes; cv0: the (c, v) image the first one reads (its variance plane is d_guided_var[0])
int guided_passes(fh_ctx* ctx, int w, int h, const fh_denoise_inputs* in, const fh_denoise_params* pr, const float4* cv0, float* out, int upscale)
{
  hipStream_t st = ctx->stream;
  GuidedArgs a{};
  a.normal = (const float4*)in->normal; a.albedo = (const float4*)in->albedo; a.position = (const float4*)in->position; a.depth = in->depth;
  a.w = w; a.h = h; a.sigma_l = pr->sigma_l; a.sigma_z = pr->sigma_z; a.sa2 = pr->sigma_a * pr->sigma_a; a.power_log2 = pr->normal_power_log2; a.upscale = upscale;
  for (uint32_t it = 0; it < pr->passes; ++it) {
    const bool last = it + 1 == pr->passes;
    const int s = 1 << it;
    a.cv = it == 0 ? cv0 : ctx->d_guided_cv[it & 1]; a.vplane = ctx->d_guided_var[it & 1];
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

}  // namespace

int denoise_guided_submit(fh_ctx* ctx, int w, int h, const fh_denoise_inputs* in, const fh_denoise_params* pr, float* out, int upscale)
{
  if (const int rc = guided_scratch(ctx, (size_t)w * h)) return rc;
  guided_prepare(ctx, w, h, in, pr);
  return guided_passes(ctx, w, h, in, pr, ctx->d_guided_cv[0], out, upscale);
}

namespace {

// the motion table into the context's device buffer, through pinned memory: the caller's array is free again when the call returns
int motion_upload(fh_ctx* ctx, uint32_t n, const fh_motion* motion)
{
  if (ctx->h_motion.size() < n) {  // (the second of the two: both were made)
    (void)hipStreamSynchronize(ctx->stream);  // (a call queued earlier may still read the old table)
    ctx->d_motion.reset(); ctx->h_motion.reset();
    FH_HIP(ctx->d_motion.alloc(n));
    FH_HIP(ctx->h_motion.alloc(n));
  }
  if (!ctx->ev_motion) FH_HIP(ctx->ev_motion.create(hipEventDisableTiming));
  else FH_HIP(hipEventSynchronize(ctx->ev_motion));  // the copy of the call before has left the pinned buffer
  std::memcpy(ctx->h_motion, motion, (size_t)n * sizeof(fh_motion));
  FH_HIP(hipMemcpyAsync(ctx->d_motion, ctx->h_motion, (size_t)n * sizeof(fh_motion), hipMemcpyHostToDevice, ctx->stream));
  FH_HIP(hipEventRecord(ctx->ev_motion, ctx->stream));
  return FH_OK;
}

// the one launch between the preparation and the passes: buffer hist.cur is read, the other written (hist.commit makes it the current one)
void temporal_stage(fh_ctx* ctx, const TemporalCallPlan& plan, int w, int h, const fh_denoise_inputs* in, const fh_temporal_params* tp, const uint32_t* ids, uint32_t n_instances)
{
  const fh_ctx::TemporalHistory& hist = ctx->hist;
  const int from = hist.cur, to = from ^ 1;
  TemporalArgs a{};
  a.cv = ctx->d_guided_cv[0]; a.normal = (const float4*)in->normal; a.position = (const float4*)in->position; a.depth = in->depth;
  a.h_cv = hist.d_cv[from]; a.h_ph = hist.d_ph[from]; a.h_n = hist.d_n[from];
  a.o_cv = hist.d_cv[to]; a.o_ph = hist.d_ph[to]; a.o_n = hist.d_n[to];
  a.vplane = ctx->d_guided_var[0];
  a.w = w; a.h = h; a.W = (float)w; a.H = (float)h;
  for (int k = 0; k < 12; ++k) a.m[k] = hist.w2c[k];
  a.f = hist.inv_tan;
  a.alpha_min = tp->alpha_min; a.max_history = tp->max_history; a.cos_min = tp->normal_cos_min; a.plane_tol = tp->plane_tol;
  a.ids = ids; a.motion = ctx->d_motion; a.n_instances = n_instances; a.still = plan.still ? 1 : 0;
  a.gamma = ctx->response_gamma; a.kappa = ctx->response_kappa;
  if (plan.mom) { a.h_mu = hist.d_mu[from]; a.o_mu = hist.d_mu[to]; a.min_history = ctx->moments_min_history; a.replace_v = plan.replace_v ? 1 : 0; }
  kTemporalLaunch[plan.mom][plan.look][plan.clip](a, dim3((w + kTW - 1) / kTW, (h + kTH - 1) / kTH), ctx->stream);
}

}  // namespace

// ids == nullptr: no motion stage (fh_denoise_temporal, or no instance moved)
int denoise_temporal_submit(fh_ctx* ctx, int w, int h, const fh_denoise_inputs* in, const fh_camera* cam, const float w2c[12], float inv_tan, const fh_temporal_params* tp,
                            const fh_denoise_params* pr, const uint32_t* ids, uint32_t n_instances, const fh_motion* motion, float* out, int upscale)
{
  fh_ctx::TemporalHistory& hist = ctx->hist;
  const size_t px = (size_t)w * h;
  if (const int rc = guided_scratch(ctx, px)) return rc;
  // the plan is made from the history as the call finds it; ensure() acts on the same temporal_grow
  const TemporalCallPlan plan = temporal_call_plan({hist.frames, hist.w, hist.h, hist.capacity(), hist.moment_capacity(), std::memcmp(cam, &hist.camera, sizeof(fh_camera)) == 0},
                                                   {(uint32_t)w, (uint32_t)h, ids != nullptr, in->moments != nullptr},
                                                   {ctx->denoise_response != 0, ctx->denoise_response_noise != 0, ctx->denoise_temporal_moments != 0});
  FH_HIP(hist.ensure(px, plan.mom));
  if (!plan.history_kept) hist.restart();  // (a call at another size than the history's; after a grow, ensure() has done it)
  if (plan.with_motion)
    if (const int rc = motion_upload(ctx, n_instances, motion)) return rc;
  guided_prepare(ctx, w, h, in, pr);
  temporal_stage(ctx, plan, w, h, in, tp, ids, n_instances);
  hist.commit(*cam, w2c, inv_tan, (uint32_t)w, (uint32_t)h);  // (whether or not the passes then fail: the stage is queued)
  return guided_passes(ctx, w, h, in, pr, hist.d_cv[hist.cur], out, upscale);
}

namespace {

// fh_denoise_temporal after its refusals.  Under fh_set_denoise_motion the context feeds the call what fh_denoise_temporal_motion is fed by its caller: the motion table
// from the snapshot of the instance matrices the history was written under, and the id plane of this camera.  Everything that can fail is decided before the first launch.
int temporal_feed_motion(fh_ctx* ctx, uint32_t width, uint32_t height, const fh_denoise_inputs* in, const fh_camera* camera, const float w2c[12], float inv_tan,
                         const fh_temporal_params* tp, const fh_denoise_params* pr, float* denoised, int upscale)
{
  fh_ctx::TemporalHistory& hist = ctx->hist;
  // alive is what denoise_temporal_submit's plan will call history_kept, and the table and the id plane below are made only for a call that looks them up.  The two agree
  // because of what the record keeps true while frames != 0: commit() follows an ensure() for w x h pixels, so capacity() >= w * h and no main grow at this size; and
  // with the moments on, that ensure() made the moment image as large as the rest, while the switch itself drops the history whenever it changes, so no moment grow either.
  // (tools/temporal_host_check.cpp asserts it over its cases.)
  const bool alive = hist.frames != 0 && hist.w == width && hist.h == height;
  const TemporalFeedPlan feed = temporal_feed_plan(ctx->denoise_motion != 0, alive, hist.o2w, hist.w2o, ctx->h_o2w, ctx->h_w2o, ctx->scene_loaded && ctx->bvh_valid);
  if (feed.refusal) return fail(ctx, FH_E_INVALID, std::string("fh_denoise_temporal: ") + feed.refusal);
  std::vector<fh_motion> table;
  const uint32_t* ids = nullptr;
  if (feed.feed_motion) {
    table.resize(ctx->h_o2w.size() / 12);
    for (size_t i = 0; i < table.size(); ++i) {
      motion_entry(hist.o2w.data() + 12 * i, hist.w2o.data() + 12 * i, ctx->h_o2w.data() + 12 * i, ctx->h_w2o.data() + 12 * i, &table[i]);
      if (!motion_finite(table[i])) return fail(ctx, FH_E_INVALID, "fh_denoise_temporal: the motion of an instance is not finite (fh_set_denoise_motion)");
    }
    const size_t px = (size_t)width * height;
    if (ctx->d_motion_ids.size() < px) {
      (void)hipStreamSynchronize(ctx->stream);
      FH_HIP(ctx->d_motion_ids.alloc(px));
    }
    if (const int rc = primary_instances_submit(ctx, camera, width, height, ctx->d_motion_ids)) return rc;
    ids = ctx->d_motion_ids;
  }
  const int rc = denoise_temporal_submit(ctx, (int)width, (int)height, in, camera, w2c, inv_tan, tp, pr, ids, (uint32_t)table.size(), ids ? table.data() : nullptr, denoised, upscale);
  if (rc == FH_OK && ctx->denoise_motion) { hist.o2w = ctx->h_o2w; hist.w2o = ctx->h_w2o; }  // the snapshot: what the next call's table is made from
  return rc;
}

}  // namespace
}  // namespace fh

using namespace fh;

extern "C" {

// every refusal is decided from the arguments alone, before the context or the device is touched: a refused call changes nothing
int fh_denoise_guided(fh_ctx* ctx, uint32_t width, uint32_t height, const fh_denoise_inputs* in, const fh_denoise_params* params, float* denoised, int upscale2x)
{
  const fh_denoise_params pr = params ? *params : kDenoiseDefaults;
  const char* why = guided_refusal(width, height, in, pr, denoised);
  if (!why && !ctx) why = "null context";
  if (why) return fail(ctx, FH_E_INVALID, std::string("fh_denoise_guided: ") + why);
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  return denoise_guided_submit(ctx, (int)width, (int)height, in, &pr, denoised, upscale2x ? 1 : 0);
}

// fh_denoise_guided with the temporal stage in front of its passes; refusals as there (temporal_host.h)
int fh_denoise_temporal(fh_ctx* ctx, uint32_t width, uint32_t height, const fh_denoise_inputs* in, const fh_camera* camera, const fh_temporal_params* temporal,
                        const fh_denoise_params* params, float* denoised, int upscale2x)
{
  const fh_denoise_params pr = params ? *params : kDenoiseDefaults;
  const fh_temporal_params tp = temporal ? *temporal : kTemporalDefaults;
  float w2c[12], inv_tan = 0.0f;
  const char* why = temporal_refusal(width, height, in, camera, tp, pr, denoised, w2c, &inv_tan);
  if (!why && !ctx) why = "null context";
  if (why) return fail(ctx, FH_E_INVALID, std::string("fh_denoise_temporal: ") + why);
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  return temporal_feed_motion(ctx, width, height, in, camera, w2c, inv_tan, &tp, &pr, denoised, upscale2x ? 1 : 0);
}

int fh_denoise_history_reset(fh_ctx* ctx)
{
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  ctx->hist.drop();
  return FH_OK;
}

int fh_denoise_history_info(fh_ctx* ctx, uint32_t* width, uint32_t* height, uint32_t* frames)
{
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  if (width) *width = ctx->hist.w;
  if (height) *height = ctx->hist.h;
  if (frames) *frames = ctx->hist.frames;
  return FH_OK;
}

// the switch of the clipped temporal stage: broadcast on a group like fh_set_denoise_motion (the work it switches on runs on the lead)
int fh_set_denoise_response(fh_ctx* ctx, const fh_response_params* params)
{
  if (const char* why = response_refusal(params)) return fail(ctx, FH_E_INVALID, std::string("fh_set_denoise_response: ") + why);
  FH_GROUP_EACH(ctx, kGroupCallPlain, fh_set_denoise_response(m_, params));
  if (!ctx) return FH_E_INVALID;
  ctx->denoise_response = params ? 1 : 0;
  if (params) ctx->response_gamma = params->gamma;
  return FH_OK;
}

int fh_get_denoise_response(fh_ctx* ctx, int* on, fh_response_params* params)
{
  FH_GROUP_LEAD(ctx);
  if (!ctx || !on) return FH_E_INVALID;
  *on = ctx->denoise_response;
  if (params) params->gamma = ctx->response_gamma;
  return FH_OK;
}

// the noise box of the clipped stage: stored and broadcast like the switch above, and read only while that one is on
int fh_set_denoise_response_noise(fh_ctx* ctx, const fh_response_noise_params* params)
{
  if (const char* why = response_noise_refusal(params)) return fail(ctx, FH_E_INVALID, std::string("fh_set_denoise_response_noise: ") + why);
  FH_GROUP_EACH(ctx, kGroupCallPlain, fh_set_denoise_response_noise(m_, params));
  if (!ctx) return FH_E_INVALID;
  ctx->denoise_response_noise = params ? 1 : 0;
  if (params) ctx->response_kappa = params->kappa;
  return FH_OK;
}

int fh_get_denoise_response_noise(fh_ctx* ctx, int* on, fh_response_noise_params* params)
{
  FH_GROUP_LEAD(ctx);
  if (!ctx || !on) return FH_E_INVALID;
  *on = ctx->denoise_response_noise;
  if (params) params->kappa = ctx->response_kappa;
  return FH_OK;
}

// the moments of the temporal stage: broadcast like the switches above.  Turning it on or off drops the history (the stored history has, or lacks, the moment image);
// the image itself is allocated by the next call (TemporalHistory::ensure) and freed here when the switch goes off
int fh_set_denoise_temporal_moments(fh_ctx* ctx, const fh_temporal_moments_params* params)
{
  if (const char* why = temporal_moments_refusal(params)) return fail(ctx, FH_E_INVALID, std::string("fh_set_denoise_temporal_moments: ") + why);
  FH_GROUP_EACH(ctx, kGroupCallPlain, fh_set_denoise_temporal_moments(m_, params));
  if (!ctx) return FH_E_INVALID;
  const int on = params ? 1 : 0;
  if (on != ctx->denoise_temporal_moments) {
    ctx->hist.drop();
    if (!on && (ctx->hist.d_mu[0] || ctx->hist.d_mu[1])) {
      if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, FH_E_HIP, "hipSetDevice failed");
      (void)hipStreamSynchronize(ctx->stream);  // (a call queued earlier may still write them)
      ctx->hist.release_moments();
    }
  }
  ctx->denoise_temporal_moments = on;
  if (params) ctx->moments_min_history = params->min_history;
  return FH_OK;
}

int fh_get_denoise_temporal_moments(fh_ctx* ctx, int* on, fh_temporal_moments_params* params)
{
  FH_GROUP_LEAD(ctx);
  if (!ctx || !on) return FH_E_INVALID;
  *on = ctx->denoise_temporal_moments;
  if (params) params->min_history = ctx->moments_min_history;
  return FH_OK;
}

}  // extern "C"
