// render.hip -- the wavefront path tracer: kernels + per-frame submission.
//
// Replaces Renderer::render -> optixLaunch of the megakernel in fredholm/modules/pt.cu
// (__raygen__rg :418-502, __closesthit__radiance :680-944, __closesthit__light :952-999,
// __miss__* :504-543).  One reference launch thread = one pixel looping over samples and bounces;
// here a pass starts `B` samples for every owned pixel as independent path slots and advances all
// of them one bounce at a time:
//
//   k_generate               CMJ slots 0/1 -> thin-lens camera ray, throughput 1; rays that miss the scene bounds are
//                            finished here (sky / background) and never enter a queue            (pt.cu:433-454, :504-523)
//   k_trace_closest_stream   closest hit for the radiance-ray queue: waves draw chunks of the queue, refill idle lanes in
//                            flight and test candidate triangles cooperatively (fh_trace.h: traverse_stream)
//   k_route                  sorts the hits into one queue per shading class (BSDF-sorted shading) with block-aggregated
//                            appends: ballot + popcount per wave, LDS prefix per block, one atomic per block and class
//   k_shade<LOBES>           surface + BSDF + NEE samples + light ray + next direction + Russian roulette for the next bounce;
//                            emits secondary rays with their pre-weighted contributions and the cell key of the hit point
//   k_miss_primary           sky / background for paths that leave the scene at depth 0               (pt.cu:504-523)
//   k_cell_hist/scan/scatter counting sort of the secondary and next-bounce queues by the cell of the ray origin
//   k_trace_secondary_stream any-hit shadow rays (and the BSDF-sampled light ray) of every shaded path, in the reference's
//                            order; adds the contributions that turn out unoccluded
//   k_tail                   all remaining bounces of the few paths still alive after the wavefront bounces, one kernel
//   k_accumulate             NaN guard + running mean of the 6 AOVs, sample_count += B                (pt.cu:474-501)
// The *_static and *_coop kernels are the fixed-batch forms (binary-BVH fallback of tiny scenes, FH_STREAM=0 / FH_COOP=0).
//
// Sampler slots are addressed absolutely (fh_sampler.h): at bounce b the Sobol' dimension base is
// 1 + b*n1 and the CMJ slot base is 2 + b*n2 with n1 = 3 + [lights], n2 = 3 + [directional] + [lights],
// which reproduces the draw order of SURVEY.md appendix A without per-path sampler state.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "context.h"
#include "fh_bsdf.h"
#include "fh_dark_sky.h"
#include "fh_envmap.h"
#include "fh_tonemap.h"
#include "fh_trace.h"
#include "render_plan_host.h"

namespace fh {

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kLutReflFloats = 16 * 16 * 2, kLutSheenFloats = 16 * 16;  // lut.cu:5-93, :917-955
constexpr uint32_t kMatLds = 32;  // material records staged in LDS by the shade kernels when the scene has at most this many
#ifndef FH_SECONDARY_BLOCKS_HEAVY
#define FH_SECONDARY_BLOCKS_HEAVY 5  // resident workgroups per CU the secondary streaming kernel is compiled for when it carries the emitter / any-hit code
#endif
#ifndef FH_STREAM_BLOCKS
#define FH_STREAM_BLOCKS 7  // resident workgroups per CU (= waves per SIMD) the streaming traversal kernels are compiled and launched for: 512 / that registers per lane (72 at seven), 160 KB / that of LDS
                            // (seven stack levels next to the cooperative-test records; deeper levels spill).  Six / seven / eight measured on the same box (profiles/README.md r4-1): configs[3] 542 / 598 / 539
                            // Msamples/s, configs[2] 6552 / 6702 / 6017 -- at eight the secondary kernel spills registers and keeps four stack levels in LDS
#endif
#ifndef FH_STREAM_BLOCKS_ALPHA
#define FH_STREAM_BLOCKS_ALPHA FH_STREAM_BLOCKS  // the same for the secondary-ray kernel with the any-hit test compiled in
#endif
#ifndef FH_STREAM_BLOCKS_CLOSEST
#define FH_STREAM_BLOCKS_CLOSEST FH_STREAM_BLOCKS  // the same for the closest-hit kernel, which needs fewer registers than the secondary-ray kernel
#endif
#ifndef FH_STREAM_BLOCKS_FILLER
#define FH_STREAM_BLOCKS_FILLER 6  // workgroups per CU the streaming kernels are LAUNCHED with while a filler launch of k_sky_pixels is resident (stream_plan)
#endif
#ifndef FH_SHADE_BLOCKS
#define FH_SHADE_BLOCKS 2  // resident workgroups per CU the specialised shade kernels are compiled for (register budget = 512 / that per lane): they take 159-182 registers
#endif                     // since their products go to memory as they are made (PoolSink); the generic seven-lobe kernel keeps one wave per SIMD (350 registers).
// A second set is compiled for THREE workgroups per CU (168 registers, 6-7 of them spilled: 28-44 B of scratch), and it is the set every scene gets (render_submit;
// FH_SHADE_WGS=2|3 forces either).  Round 3 gave it to textured scenes only -- their hits wait for texels and a third wave per SIMD covers that (configs[3]: shade 3.87 -> 3.53 s
// alone; with two, today, 676 -> 644 Msamples/s) -- because the untextured ones lost with it then (configs[1] 2210 -> 2025).  On round 5's build they gain as well
// (profiles/r05_tunables.log: configs[1] 2751 -> 2823, configs[2] 7841 -> 7972, configs[4] with the flush threshold below 5559 -> 5772).

// generator matrices of the N Sobol' dimensions a kernel draws from, staged in LDS in their byte-indexed form (4 KB per dimension, FrameDev::sobol_bytes):
// the XOR over the 32 index bits is four LDS reads instead of 32 bit tests (~85 instructions less per draw; the shade kernels draw three or four per hit)
template <int N>
struct SobolRows {
  uint32_t m[N][1024];
};

template <int N>
FH_D void load_sobol_rows(SobolRows<N>& rows, const uint32_t* tables, const uint32_t* dims)
{
  static_assert(kBlock == 256, "one uint4 per thread and dimension");
#pragma unroll
  for (int r = 0; r < N; ++r)
    reinterpret_cast<uint4*>(rows.m[r])[threadIdx.x] = reinterpret_cast<const uint4*>(tables + (size_t)(dims[r] & 1023u) * 1024u)[threadIdx.x];
  __syncthreads();
}

// Wave priority of the kernels of a pass, raised once at entry.  k_sky_pixels stays at 0: its filler launch shares SIMDs with these kernels for as long as the call's passes
// run, and the issue arbiter takes priority first and age second -- at equal priority a sky wave, which lives for a whole call, is the oldest on its SIMD and the pass
// waves get what it leaves.  Among themselves the pass kernels stay equal.
#ifndef FH_PASS_PRIORITY
#define FH_PASS_PRIORITY 1
#endif
FH_D void pass_priority()
{
  if (FH_PASS_PRIORITY) __builtin_amdgcn_s_setprio(FH_PASS_PRIORITY);
}

// the sky coefficients of the frame, copied to the workgroup's LDS; the caller's next barrier publishes them
FH_D void stage_sky(FrameDev& fr, HosekSky& lds_sky)
{
  if (!fr.has_hosek) return;
  if (threadIdx.x < sizeof(HosekSky) / 4u) reinterpret_cast<float*>(&lds_sky)[threadIdx.x] = reinterpret_cast<const float*>(fr.hosek)[threadIdx.x];
  fr.hosek = &lds_sky;
}

// sample n_spp of pixel (px, py): CMJ slots 0 / 1 -> thin-lens camera ray (pt.cu:433-454, camera.cu:24-53) and the Russian roulette of bounce 0, which has probability 1 but
// still consumes (and can fail on) a draw (pt.cu:457-461).  Returns whether the path is alive.
FH_D bool camera_ray(const FrameDev& fr, const uint32_t* sobol_dim1, uint32_t image_idx, uint32_t px, uint32_t py, uint32_t n_spp, f2 u, f2 u_lens, f3& org, f3& dir);
FH_D bool camera_sample(const FrameDev& fr, const uint32_t* sobol_dim1, uint32_t image_idx, uint32_t px, uint32_t py, uint32_t n_spp, f3& org, f3& dir)
{
  return camera_ray(fr, sobol_dim1, image_idx, px, py, n_spp, cmj_draw(n_spp, image_idx, 0u, fr.seed_hash), cmj_draw(n_spp, image_idx, 1u, fr.seed_hash), org, dir);
}
// (u, u_lens: CMJ slots 0 and 1 of the sample)
FH_D bool camera_ray(const FrameDev& fr, const uint32_t* sobol_dim1, uint32_t image_idx, uint32_t px, uint32_t py, uint32_t n_spp, f2 u, f2 u_lens, f3& org, f3& dir)
{
  // Divisions in their short form (fh_vec.h: div_r, div_r_nofix; the claims are binary exponents).  The camera's own numbers are the caller's and are not validated, so
  // the sites they reach keep the fix-up, and their claims hold for 2^-20 <= 1 / tan(fov / 2) <= 2^20, 2^-40 <= |a + b| <= 2^40, a lens radius and a transform
  // of at most 2^20 (an image is at most 65535 pixels a side: the pixel lists pack x and y into 16 bits each).
  // uv: the numerator is a difference of floats below 2^18 that carry at most 24 bits -- +0 (x - x rounds to +0, never -0) or at least 2^-24 of the larger -- over 1 <= height < 2^16
  // (the divisor is re-read per sample behind an empty asm: left to itself the compiler keeps the refined reciprocal of the frame's height, and what goes with it, live across
  // the whole sample loop -- five more scalar spills in k_sky_pixels<true>, which then needs scratch memory; the reciprocal's three instructions per sample cost less)
  float height = fr.height;
  asm volatile("" : "+v"(height));
  float uvx = div_r_nofix<-40, 18, 0, 16>(2.0f * (px + u.x) - fr.width, height);
  const float uvy = div_r_nofix<-40, 18, 0, 16>(2.0f * (py + u.y) - fr.height, height);
  uvx = -uvx;
  u = u_lens;
  // thin lens (camera.cu:24-53); a + b and the lens radius are the same for every ray: computed once on the host, in fp32 with the reference's operations
  const float f = fr.cam_inv_tan;
  const f3 p_sensor = mk3(uvx, uvy, 0.0f);
  const f3 p_lens_center = mk3(0.0f, 0.0f, f);
  const f2 pd = fr.cam_lens_radius * concentric_disk(u);
  const f3 p_lens = p_lens_center + mk3(pd.x, pd.y, 0.0f);
  const f3 s2c = normalize_r<-20, 21>(p_lens_center - p_sensor);  // f <= |(-uvx, -uvy, f)| <= f + 2^19: |uv| <= 2 x 65535 each
  const f3 p_object = p_sensor + div_r<-40, 40, -41, 1>(fr.cam_a_plus_b, s2c.z) * s2c;  // s2c.z = f x RN(1 / |.|): at least 2^-20 / 2^21, at most 1 and a rounding
  org = xform_point(fr.cam_xf, p_lens);
  f3 d = normalize_r<-42, 84>(p_object - p_lens);  // the object point lies |a + b| / s2c.z <= 2^81 along s2c, the lens point within 2^21 of the sensor's; along the axis they are a + b - f apart, taken to be 2^-42 at least
  d.z *= -1.0f;
  dir = xform_dir(fr.cam_xf, d);
  const uint32_t sidx = image_idx + n_spp * fr.width * fr.height;
  const float rr = sobol_draw_bytes(sobol_dim1, sidx, 1u, fr.seed_hash);
  return fr.max_depth > 0 && !(rr >= 1.0f);
}

// ------------------------------------------------------------------------------------------------
// grid: x over the owned pixels (grid-stride), y = sample of the pass -- slot p = sample * n_owned + pixel without a division per path, and the pixel's
// coordinates come packed from the ownership list instead of from image_idx / width and % width (four integer divisions by run-time values were ~60 of the
// kernel's ~1070 non-FMA instructions per path)
constexpr int kGenChunks = 4;  // (eight measure the same: profiles/README.md r4-20)
__global__ void __launch_bounds__(kBlock) k_generate(FrameDev fr, PoolDev pool, const uint32_t* issued, const uint32_t* owned, const uint32_t* owned_xy, uint32_t n_owned)
{
  pass_priority();
  __shared__ SobolRows<1> rows;
  __shared__ HosekSky s_sky;
  stage_sky(fr, s_sky);
  const uint32_t dims[1] = {1u};
  load_sobol_rows<1>(rows, fr.sobol_bytes, dims);
  // A workgroup takes kGenChunks x 256 consecutive pixels per round and appends the paths that enter the scene with ONE returning atomic (block_queue_reserve): with one per
  // wave, an interior -- every camera ray enters -- spent most of the kernel waiting for queue positions (configs[3]: 188 -> see profiles/README.md r4)
  const uint32_t stride = gridDim.x * blockDim.x * kGenChunks;
  const uint32_t k = blockIdx.y;
  __shared__ uint32_t s_reserve[2][5 * kGenChunks];
  uint32_t iter = 0;
  for (uint32_t base = blockIdx.x * blockDim.x * kGenChunks; base < n_owned; base += stride) {
   uint32_t packed = 0u;  // per chunk one byte: bit 7 = this lane's path enters the scene, bits 0-5 = its rank among the entering lanes of its wave
   uint32_t* const scratch = s_reserve[iter & 1u];
#pragma unroll 1
   for (int c = 0; c < kGenChunks; ++c) {  // (a loop, not four copies: the body is 18 KB of code)
    const uint32_t i = base + (uint32_t)c * blockDim.x + threadIdx.x;
    const bool valid = i < n_owned;
    const uint32_t p = k * n_owned + i;  // slot p = sample-major: lanes of a wave hold neighbouring pixels of one sample index
    bool enter = false;
    if (valid) {
      const uint32_t image_idx = owned[i];
      const uint32_t n_spp = issued[image_idx] + k;  // sample index = samples started on this pixel so far (pt.cu:423: params.sample_count)
      const uint32_t xy = owned_xy[i];
      f3 org, dir;
      const bool alive = camera_sample(fr, rows.m[0], image_idx, xy & 0xffffu, xy >> 16, n_spp, org, dir);
      // camera rays that miss the (padded) scene bounds cannot hit anything: they are finished right here
      // (radiance = 0 + 1 * environment, pt.cu:504-523) and never enter the traversal queue, so the waves of
      // bounce 0 only hold rays that enter the scene and no path state is written for the others
      RayPre rp;  // (only what the slab test reads: origin and reciprocal direction, as ray_prepare forms them)
      rp.o = org;
      rp.inv = safe_reciprocal_r(dir);
      float tn;
      enter = alive && slab_test(rp, fr.scene_lo.x, fr.scene_lo.y, fr.scene_lo.z, fr.scene_hi.x, fr.scene_hi.y, fr.scene_hi.z, 1e9f, tn);
      if (enter) {
        pool.ray_o[p] = mk4(org, 1e9f);
        pool.ray_d[p] = mk4(dir, 0.0f);
        pool.thr[p] = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
        pool.rad[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        pool.pixel[p] = image_idx;
        pool.nspp[p] = n_spp;
        pool.flags[p] = 0u;
      } else {
        const f3 r = alive ? mk3(0.0f) + mk3(1.0f) * env_radiance(fr, dir) : mk3(0.0f);
        pool.rad[p] = mk4(r, 0.0f);
        pool.flags[p] = 2u;  // finished here and in no queue: only k_accumulate reads the slot again (radiance and flags)
      }
    }
    const unsigned long long m = __ballot(enter);
    if ((threadIdx.x & 63u) == 0u) scratch[4 * c + (threadIdx.x >> 6)] = (uint32_t)__popcll(m);
    packed |= ((enter ? 0x80u : 0u) | (uint32_t)__popcll(m & ((1ull << (threadIdx.x & 63u)) - 1ull))) << (8 * c);
   }
   __syncthreads();
   if (threadIdx.x == 0u) {
     uint32_t total = 0;
     for (uint32_t c = 0; c < 4u * kGenChunks; ++c) { const uint32_t v = scratch[c]; scratch[c] = total; total += v; }
     scratch[4 * kGenChunks] = total ? atomicAdd(&pool.counters[CNT_RAD], total) : 0u;
   }
   __syncthreads();
   ++iter;  // (the next round writes the other scratch area: a lane may still be reading this one)
#pragma unroll
   for (int c = 0; c < kGenChunks; ++c)
     if ((packed >> (8 * c)) & 0x80u)
       pool.q_rad[0][scratch[4 * kGenChunks] + scratch[4 * c + (threadIdx.x >> 6)] + ((packed >> (8 * c)) & 63u)] = k * n_owned + base + (uint32_t)c * blockDim.x + threadIdx.x;
  }
}

// samples started per owned pixel, bumped after k_generate has read it for every path of the pass
__global__ void __launch_bounds__(kBlock) k_bump_issued(uint32_t* issued, const uint32_t* owned, uint32_t n_owned, uint32_t n_batch)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_owned) issued[owned[i]] += n_batch;
}

// ------------------------------------------------------------------------------------------------
// Pixels that cannot see the scene.  On the bench's soup 79 % of the pixels are sky from corner to corner: not one ray of their footprint, through any point of
// the lens, reaches the scene's bounds.  Every sample of such a pixel is a camera ray plus an environment lookup; sent through the wavefront machinery it costs a
// path slot of 284 bytes, a radiance record written by k_generate and read back by k_accumulate, and it makes a pass hold a fifth of the paths that do work.  So
// a call that brings enough samples splits its owned pixels once per camera: k_split_pixels sorts them into the pixels the passes render (`wave`) and the sky
// pixels, and k_sky_pixels renders ALL samples of the call for a sky pixel in one go -- camera sample, environment, NaN guard, running means -- with the same
// device functions in the same order as k_generate / k_accumulate, i.e. the same bits, no pool memory and one read and one write of the six layers per call.
//
// The test is conservative.  In camera space every ray of pixel (px, py) starts on the lens disk (centre A0 = (0, 0, f), radius R) and runs through the
// z-mirrored image B of its focus point, B = (k uvx, k uvy, 2 f - (a + b)) with k = 1 - (a + b) / f and (uvx, uvy) inside the pixel, so the rays are the lines
// through a disk of radius R around A0 and a square of half-diagonal rho = sqrt(2) |k| / H around B0.  A point of such a line at parameter s (A + s (B - A))
// is at most R |1 - s| + rho |s| <= R + (R + rho) |s| away from the centre line's point at s; with d0 the distance of the sphere's centre from the centre line,
// tau the position of its foot along it and L = |B0 - A0|, no line of the family comes nearer than d0 sqrt(1 - (m / L)^2) - R - m |tau| / L, m = R + rho.  The
// pixel is sky when that exceeds the bounding sphere of the padded scene bounds with a margin (0.1 % of the radius and of the distance, far above the rounding
// of these few operations).  k_sky_pixels still runs k_generate's own bounds test per sample and counts a violation (fh_sync reports it): the split can only
// lose speed, never a ray that hits.
//
// Dark sky pixels (dark_on; render_plan_host.h: dark_sky_verdict).  Under the Hosek sky a ray that points below the horizon carries NaN, which the guard counts as zero.
// A sky pixel whose every ray points below the horizon (fh_dark_sky.h: dark_sky_pixel, from the centre line and the family radius m formed here) goes to a third
// list and never enters k_sky_pixels: k_dark_pixels applies the updates of the running means that samples of value zero make, and nothing else.  The per-sample bounds
// test (`violations`) does NOT run for these pixels; they are a subset of the pixels the tests above proved to be sky, by the same geometry.
struct SplitDev {
  f3 centre;      // bounding sphere of the padded scene bounds, camera space
  float radius;
  float far;      // distance of the farthest corner of the padded scene bounds from the lens centre
  uint32_t dark_on;
  uint32_t* wave_px; uint32_t* wave_xy; uint32_t* sky_px; uint32_t* sky_xy; uint32_t* dark_px; uint32_t* dark_xy;
  uint32_t* counters;  // [0] wave pixels, [1] sky pixels, [2] bounds-test violations seen by k_sky_pixels, [4] dark sky pixels
};
__global__ void __launch_bounds__(kBlock) k_split_pixels(FrameDev fr, SplitDev sp, const uint32_t* owned, const uint32_t* owned_xy, uint32_t n_owned)
{
  __shared__ uint32_t s_reserve[2][15];
  uint32_t iter = 0;
  for (uint32_t base = blockIdx.x * blockDim.x; base < n_owned; base += gridDim.x * blockDim.x) {
    const uint32_t i = base + threadIdx.x;
    bool sky = false, wave = false, dark = false;
    uint32_t px = 0, xy = 0;
    if (i < n_owned) {
      px = owned[i]; xy = owned_xy[i];
      const float x = (float)(xy & 0xffffu) + 0.5f, y = (float)(xy >> 16) + 0.5f;
      const float uvx = -(2.0f * x - (float)fr.width) / (float)fr.height, uvy = (2.0f * y - (float)fr.height) / (float)fr.height;
      const float f = fr.cam_inv_tan, k = 1.0f - fr.cam_a_plus_b / f;
      const f3 a0 = mk3(0.0f, 0.0f, f), b0 = mk3(k * uvx, k * uvy, 2.0f * f - fr.cam_a_plus_b);
      const f3 ab = b0 - a0;
      const float L = length(ab);
      const float m = fabsf(fr.cam_lens_radius) + 1.41421357f * fabsf(k) / (float)fr.height * 1.001f;
      const f3 w = sp.centre - a0;
      const float tau = dot(w, ab) / L;
      const float d0 = sqrt_cr(fmaxf(dot(w, w) - tau * tau, 0.0f));
      const float q = 1.0f - (m / L) * (m / L);
      const float nearest = d0 * sqrt_cr(fmaxf(q, 0.0f)) - fabsf(fr.cam_lens_radius) - m * fabsf(tau) / L;
      sky = L > 0.0f && q > 0.0f && nearest > sp.radius * 1.001f + 1e-3f * (length(w) + 1.0f);  // (NaN anywhere: not sky)
      // The sphere is a loose fit of a box (a cube's has 2.4 times its silhouette): a second test, against the bounds themselves.  A ray of the pixel that reaches a point P
      // of the bounds does so at a parameter |s| <= (|P - A0| + R) / (L - m), and there it is within R + m |s| of the centre line's point at s (above).  So with the bounds
      // grown by d = R + m (far + R) / (L - m) on every side -- `far` the distance of their farthest corner from the lens centre -- the centre LINE, a rigid transform away
      // in world space, passes through the grown box whenever any ray of the pixel reaches the bounds; a centre line that misses the grown box makes the pixel sky.
      if (!sky && L > m * 1.01f) {
        const float d = (fabsf(fr.cam_lens_radius) + m * (sp.far + fabsf(fr.cam_lens_radius)) / (L - m)) * 1.001f + 1e-3f * (sp.far + 1.0f);
        const f3 o = xform_point(fr.cam_xf, a0), dir = xform_dir(fr.cam_xf, (1.0f / L) * ab);  // (unit length: the line parameters below are world distances)
        float tn = -3.0e38f, tf = 3.0e38f;
        bool miss = false;
        const float oo[3] = {o.x, o.y, o.z}, dd[3] = {dir.x, dir.y, dir.z}, lo[3] = {fr.scene_lo.x - d, fr.scene_lo.y - d, fr.scene_lo.z - d}, hi[3] = {fr.scene_hi.x + d, fr.scene_hi.y + d, fr.scene_hi.z + d};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          if (fabsf(dd[a]) < 1e-12f) miss = miss || oo[a] < lo[a] || oo[a] > hi[a];  // parallel to this pair of planes (a NaN compares false: not a miss)
          else {
            const float t0 = (lo[a] - oo[a]) / dd[a], t1 = (hi[a] - oo[a]) / dd[a];
            tn = fmaxf(tn, fminf(t0, t1)); tf = fminf(tf, fmaxf(t0, t1));
          }
        }
        // (the interval is widened by a thousandth of the distances involved: the parameters are quotients of quantities of the scene's size, rounded a few times)
        miss = miss || tn - 1e-3f * (fabsf(tn) + sp.far) > tf + 1e-3f * (fabsf(tf) + sp.far);
        sky = miss && dd[0] == dd[0] && dd[1] == dd[1] && dd[2] == dd[2] && d == d;
      }
      wave = !sky;
      if (sky && sp.dark_on) {  // ab = B0 - A0 is the centre ray's direction after camera_ray's z flip; the transform is a rotation (split_pixels)
        const f3 c = xform_dir(fr.cam_xf, (1.0f / L) * ab);
        dark = c.x == c.x && c.z == c.z && dark_sky_pixel(c.y, m, L);
        sky = !dark;
      }
    }
    uint32_t* const counters3[3] = {sp.counters, sp.counters + 1, sp.counters + 4};
    const bool act[3] = {wave, sky, dark};
    uint32_t pos[3];
    block_queue_reserve<3>(counters3, act, pos, s_reserve[iter & 1u]);
    ++iter;
    if (wave) { sp.wave_px[pos[0]] = px; sp.wave_xy[pos[0]] = xy; }
    if (sky) { sp.sky_px[pos[1]] = px; sp.sky_xy[pos[1]] = xy; }
    if (dark) { sp.dark_px[pos[2]] = px; sp.dark_xy[pos[2]] = xy; }
  }
}

// ------------------------------------------------------------------------------------------------
// Adaptive sampling (fh_set_adaptive_sampling).  The moments (m1, m2) are running means of the luminance y of the NaN-guarded radiance and of y * y, updated with the
// beauty layer's coefficients; a pixel whose count n is a boundary (n >= min_samples, n % step == 0) and whose relative error estimate is within the threshold gets
// no further samples.  Its state then no longer changes, so the predicate keeps holding until fh_init_render_states: the selection below can re-evaluate it from the
// state alone, and a pixel that stops after s samples holds the bits a plain render holds after s samples.
// fh_set_adaptive_policy: with growth 2 the boundaries are b0 * 2^k only (b0: the first multiple of step >= min_samples).  With guard blocks (block > 1) a pixel gets
// no further samples when every pixel of its aligned block x block square is converged: k_adaptive_mark writes the sequence number of the selection into the word of
// every block that holds an unconverged pixel, and a pixel is active when its block's word holds that number.  All pixels of a block share their count, so a stopped
// block stays stopped, and the rule is as stateless as the per-pixel one.
struct AdaptiveDev {
  float2* moments;
  const uint32_t* count;  // sample_count
  float threshold, floor;
  uint32_t min_samples, step;
  uint32_t growth, b0;           // b0 = 0: no boundary fits 32 bits
  uint32_t* marks;               // null: the per-pixel rule
  uint32_t tag, block_shift, blocks_x, width;
};

FH_D bool adaptive_boundary(const AdaptiveDev& ad, uint32_t n)
{
  if (ad.growth == 1u) return n >= ad.min_samples && n % ad.step == 0u;
  if (ad.b0 == 0u || n < ad.b0 || n % ad.b0 != 0u) return false;
  const uint32_t q = n / ad.b0;
  return (q & (q - 1u)) == 0u;
}

FH_D bool adaptive_converged(const AdaptiveDev& ad, uint32_t n, float m1, float m2)
{
  if (!adaptive_boundary(ad, n)) return false;
  float d = m2 - m1 * m1;
  if (d < 0.0f) d = 0.0f;  // (NaN stays NaN)
  const float var = d * ((float)n / (float)(n - 1u));
  const float e2 = var / (float)n;
  const float ref = m1 > ad.floor ? m1 : ad.floor;  // (NaN m1: floor)
  const float t = ad.threshold * ref;
  return ad.threshold > 0.0f && e2 <= t * t;  // (any NaN: not converged)
}

FH_D void moments_update(float& m1, float& m2, float coef, float fn, f3 radiance)
{
  const float y = luminance_rgb(radiance.x, radiance.y, radiance.z);
  m1 = coef * (fn * m1 + y);
  m2 = coef * (fn * m2 + y * y);
}

// all `n_samples` samples of this call for the sky pixels: k_generate's path for a ray that misses the scene bounds and k_accumulate's update of the running means, fused.
// ADAPTIVE: also the moments, and a pixel stops at the first boundary where it is converged (issued = first + samples taken, counted in SkyAdaptive::taken for fh_stats.paths).
// With guard blocks the launch is one round of the pixels the selection left active: it stops nothing itself (a pixel that is converged alone follows its block).
// The adaptive form takes its extra state through the pointer in place of `violations`: the kernel arguments of the plain form stay as they are.
struct SkyAdaptive {
  AdaptiveDev ad;
  uint32_t* violations;
  unsigned long long* taken;
};
// Register budget.  The kernel is compiled for kSkyWaves waves per SIMD, i.e. at most 512 / 6 -> 80 registers per lane, so that one of its waves fits beside six waves of
// the streaming traversal kernels (6 x 72 + 80 = 512): it runs in the issue slots they leave idle (SkyLaunches: filler and drain).  Three things keep it there: the
// Hosek channels are evaluated one after the other (hosek_radiance_form<true>); the sample loop carries the beauty mean and the moments only; and the five AOV means, which
// for a sky sample are n times `coef * (fn * a + 0)` -- no input of the sample enters -- are brought up to date AFTER the loop, when the camera and sky state is dead,
// value for value with the operations the loop applied.  A pixel whose AOV values all hold the bit pattern +0 skips even that: coef * (fn * 0 + 0) is +0 exactly
// (coef > 0, fn >= 0, both finite).  -0 and NaN take the update.
//
// Work distribution.  The list is cut into groups of 64 consecutive entries, one per wave; `cursor` counts the groups handed out.  A wave claims the next group with one
// atomic of its first lane, renders it, and returns for another until the cursor has passed the end: the only exit, and no wave ever waits for another.  Launches that
// share a cursor share the list: each group is claimed exactly once, whichever launch's wave comes first.
constexpr int kSkyWaves = 6;
constexpr uint32_t kSkyGroup = 64;
template <bool ADAPTIVE>
__global__ void __launch_bounds__(kBlock, kSkyWaves) k_sky_pixels(FrameDev fr, LayersDev layers, uint32_t* issued, const uint32_t* sky_px, const uint32_t* sky_xy, uint32_t n_sky, uint32_t n_samples,
                                                                std::conditional_t<ADAPTIVE, const SkyAdaptive*, uint32_t*> violations_or_adaptive, uint32_t* cursor)
{
  static_assert(kSkyGroup == 64u, "a group is one wave's lanes");
  uint32_t* violations;
  const AdaptiveDev* adp = nullptr;  // (read where it is used: fourteen more scalars held for the whole kernel cost vector registers, as lanes that scalars spill to)
  if constexpr (ADAPTIVE) { adp = &violations_or_adaptive->ad; violations = violations_or_adaptive->violations; }
  else violations = violations_or_adaptive;
  unsigned long long n_taken = 0;
  __shared__ SobolRows<1> rows;
  __shared__ HosekSky s_sky;
  stage_sky(fr, s_sky);
  const uint32_t dims[1] = {1u};
  load_sobol_rows<1>(rows, fr.sobol_bytes, dims);
  const uint32_t n_groups = (n_sky + kSkyGroup - 1u) / kSkyGroup;
  const uint32_t lane = threadIdx.x & 63u;
  for (;;) {
    uint32_t group = 0u;
    if (lane == 0u) group = atomicAdd(cursor, 1u);
    group = __shfl(group, 0);
    if (group >= n_groups) break;  // (the same for every lane of the wave)
    const uint32_t i = group * kSkyGroup + lane;
    if (i < n_sky) {  // (the last group may be short; its lanes meet again below, before the next claim)
    const uint32_t image_idx = sky_px[i], xy = sky_xy[i];
    const uint32_t first = issued[image_idx];
    uint32_t n_spp = layers.sample_count[image_idx];
    f3 beauty = mk3(layers.beauty[image_idx]);
    bool violated = false;
    CmjBlock b0{}, b1{};  // sixteen consecutive samples share most of their two CMJ draws (fh_sampler.h: cmj_block)
    float2 m = make_float2(0.0f, 0.0f);
    if constexpr (ADAPTIVE) m = adp->moments[image_idx];
    uint32_t taken = 0;
    for (; taken < n_samples; ++taken) {
      if constexpr (ADAPTIVE) { if (!adp->marks && adaptive_converged(*adp, n_spp, m.x, m.y)) break; }
      f3 org, dir;
      const uint32_t n = first + taken;
      if (taken == 0u || (n & 15u) == 0u) {
        b0 = cmj_block(n >> 4, image_idx, 0u, fr.seed_hash);
        b1 = cmj_block(n >> 4, image_idx, 1u, fr.seed_hash);
      }
      const bool alive = camera_ray(fr, rows.m[0], image_idx, xy & 0xffffu, xy >> 16, n, cmj_draw_in_block(b0, n), cmj_draw_in_block(b1, n), org, dir);
      RayPre rp;
      rp.o = org;
      rp.inv = safe_reciprocal_r(dir);
      float tn;
      violated = violated || (alive && slab_test(rp, fr.scene_lo.x, fr.scene_lo.y, fr.scene_lo.z, fr.scene_hi.x, fr.scene_hi.y, fr.scene_hi.z, 1e9f, tn));
      const f3 L = alive ? mk3(0.0f) + mk3(1.0f) * env_radiance<true>(fr, dir) : mk3(0.0f);  // (k_generate: radiance of a path that ends at the scene bounds)
      const f3 radiance = bad3(L) ? mk3(0.0f) : L;                                            // (k_accumulate: NaN guard, then the running means; a sky sample has no AOVs)
      const float coef = div_r_nofix<0, 0, 0, 32>(1.0f, n_spp + 1.0f);  // a count below 2^32, plus one
      const float fn = (float)n_spp;
      beauty = coef * (fn * beauty + radiance);
      if constexpr (ADAPTIVE) moments_update(m.x, m.y, coef, fn, radiance);
      n_spp++;
    }
    if (violated) atomicAdd(violations, 1u);
    if constexpr (ADAPTIVE) { adp->moments[image_idx] = m; n_taken += taken; }
    issued[image_idx] = first + taken;
    layers.sample_count[image_idx] = n_spp;
    layers.beauty[image_idx] = mk4(beauty, 1.0f);
    // the AOV means: `taken` updates with a sample that carries none
    f3 position = mk3(layers.position[image_idx]), normal = mk3(layers.normal[image_idx]), albedo = mk3(layers.albedo[image_idx]);
    float depth = layers.depth[image_idx];
    const float4 tc4 = layers.texcoord[image_idx];
    float tcx = tc4.x, tcy = tc4.y;
    const uint32_t any_bits = __float_as_uint(position.x) | __float_as_uint(position.y) | __float_as_uint(position.z) | __float_as_uint(normal.x) | __float_as_uint(normal.y) |
                              __float_as_uint(normal.z) | __float_as_uint(albedo.x) | __float_as_uint(albedo.y) | __float_as_uint(albedo.z) | __float_as_uint(depth) |
                              __float_as_uint(tcx) | __float_as_uint(tcy);
    if (any_bits != 0u) {
      uint32_t n_aov = n_spp - taken;
#pragma unroll 1
      for (uint32_t k = 0; k < taken; ++k) {
        const float coef = div_r_nofix<0, 0, 0, 32>(1.0f, n_aov + 1.0f);
        const float fn = (float)n_aov;
        position = coef * (fn * position + mk3(0.0f));
        normal = coef * (fn * normal + mk3(0.0f));
        depth = coef * (fn * depth + 0.0f);
        tcx = coef * (fn * tcx + 0.0f);
        tcy = coef * (fn * tcy + 0.0f);
        albedo = coef * (fn * albedo + mk3(0.0f));
        n_aov++;
      }
    }
    layers.position[image_idx] = mk4(position, 1.0f);
    layers.normal[image_idx] = mk4(normal, 1.0f);
    layers.depth[image_idx] = depth;
    layers.texcoord[image_idx] = make_float4(tcx, tcy, 0.0f, 1.0f);
    layers.albedo[image_idx] = mk4(albedo, 1.0f);
    }
  }
  if constexpr (ADAPTIVE) {  // (one global atomic per workgroup)
    __shared__ unsigned long long s_taken;
    if (threadIdx.x == 0u) s_taken = 0ull;
    __syncthreads();
    if (n_taken) atomicAdd(&s_taken, n_taken);
    __syncthreads();
    if (threadIdx.x == 0u && s_taken) atomicAdd(violations_or_adaptive->taken, s_taken);
  }
}

// all `n_samples` samples of this call for the DARK sky pixels (k_split_pixels): every one of them is zero after the NaN guard -- a path that is not alive has
// radiance 0, and one that is looks below the horizon of the Hosek sky and carries NaN -- so what k_sky_pixels would do to such a pixel is n_samples times
// x = coef * (fn * x + 0) on the beauty mean and on the five AOV means, and the two counts.  The same operations on the same operands, one lane per pixel; no camera,
// no sampler, no sky.  A group of values that all hold the bit pattern +0 stays that (k_sky_pixels' own shortcut for the AOVs; it holds for the beauty mean alike).
__global__ void __launch_bounds__(kBlock) k_dark_pixels(LayersDev layers, uint32_t* issued, const uint32_t* dark_px, uint32_t n_dark, uint32_t n_samples)
{
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_dark; i += gridDim.x * blockDim.x) {
    const uint32_t image_idx = dark_px[i];
    const uint32_t first = layers.sample_count[image_idx];
    f3 beauty = mk3(layers.beauty[image_idx]);
    if ((__float_as_uint(beauty.x) | __float_as_uint(beauty.y) | __float_as_uint(beauty.z)) != 0u) {
      uint32_t n_spp = first;
#pragma unroll 1
      for (uint32_t k = 0; k < n_samples; ++k) {
        const float coef = div_r_nofix<0, 0, 0, 32>(1.0f, n_spp + 1.0f);
        const float fn = (float)n_spp;
        beauty = coef * (fn * beauty + mk3(0.0f));
        n_spp++;
      }
    }
    f3 position = mk3(layers.position[image_idx]), normal = mk3(layers.normal[image_idx]), albedo = mk3(layers.albedo[image_idx]);
    float depth = layers.depth[image_idx];
    const float4 tc4 = layers.texcoord[image_idx];
    float tcx = tc4.x, tcy = tc4.y;
    const uint32_t any_bits = __float_as_uint(position.x) | __float_as_uint(position.y) | __float_as_uint(position.z) | __float_as_uint(normal.x) | __float_as_uint(normal.y) |
                              __float_as_uint(normal.z) | __float_as_uint(albedo.x) | __float_as_uint(albedo.y) | __float_as_uint(albedo.z) | __float_as_uint(depth) |
                              __float_as_uint(tcx) | __float_as_uint(tcy);
    if (any_bits != 0u) {
      uint32_t n_aov = first;
#pragma unroll 1
      for (uint32_t k = 0; k < n_samples; ++k) {
        const float coef = div_r_nofix<0, 0, 0, 32>(1.0f, n_aov + 1.0f);
        const float fn = (float)n_aov;
        position = coef * (fn * position + mk3(0.0f));
        normal = coef * (fn * normal + mk3(0.0f));
        depth = coef * (fn * depth + 0.0f);
        tcx = coef * (fn * tcx + 0.0f);
        tcy = coef * (fn * tcy + 0.0f);
        albedo = coef * (fn * albedo + mk3(0.0f));
        n_aov++;
      }
    }
    issued[image_idx] += n_samples;
    layers.sample_count[image_idx] = first + n_samples;
    layers.beauty[image_idx] = mk4(beauty, 1.0f);
    layers.position[image_idx] = mk4(position, 1.0f);
    layers.normal[image_idx] = mk4(normal, 1.0f);
    layers.depth[image_idx] = depth;
    layers.texcoord[image_idx] = make_float4(tcx, tcy, 0.0f, 1.0f);
    layers.albedo[image_idx] = mk4(albedo, 1.0f);
  }
}

// The stable compaction of a base list (the owned pixels, or the pixels the passes render when the call splits off the sky) into the pixels still active:
// per-workgroup counts, one scan of them, and a scatter that keeps the base list's order (the 8x8 pixel blocks of the ownership list stay together).
// `blocks` holds one count per workgroup of 256 base entries, then the total.
FH_D bool adaptive_unconverged(const AdaptiveDev& ad, uint32_t image_idx)
{
  const float2 m = ad.moments[image_idx];
  return !adaptive_converged(ad, ad.count[image_idx], m.x, m.y);
}

FH_D bool adaptive_active(const AdaptiveDev& ad, uint32_t image_idx)
{
  if (ad.marks) {
    const uint32_t y = image_idx / ad.width, x = image_idx - y * ad.width;
    return ad.marks[(y >> ad.block_shift) * ad.blocks_x + (x >> ad.block_shift)] == ad.tag;
  }
  return adaptive_unconverged(ad, image_idx);
}

// one lane per owned pixel (sky pixels included), blocks addressed by image coordinates: the order of the list changes nothing.  Every writer of a word writes the
// same value, so plain stores do; a lane whose neighbour below holds an unconverged pixel of the same block leaves the store to it (the list keeps rows of a block together).
__global__ void __launch_bounds__(kBlock) k_adaptive_mark(AdaptiveDev ad, const uint32_t* owned_px, const uint32_t* owned_xy, uint32_t n_owned)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  uint32_t key = 0xffffffffu;  // (no block has this index: a frame has at most 65535 x 65535 pixels and a block at least four)
  if (i < n_owned && adaptive_unconverged(ad, owned_px[i])) {
    const uint32_t xy = owned_xy[i];
    key = ((xy >> 16) >> ad.block_shift) * ad.blocks_x + ((xy & 0xffffu) >> ad.block_shift);
  }
  const uint32_t below = __shfl_up(key, 1);
  if (key != 0xffffffffu && ((threadIdx.x & 63u) == 0u || below != key)) ad.marks[key] = ad.tag;
}

__global__ void __launch_bounds__(kBlock) k_adaptive_count(AdaptiveDev ad, const uint32_t* base_px, uint32_t n_base, uint32_t* blocks)
{
  __shared__ uint32_t s_w[kBlock / 64];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool act = i < n_base && adaptive_active(ad, base_px[i]);
  const unsigned long long m = __ballot(act);
  if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = (uint32_t)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0u) blocks[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// one workgroup: exclusive scan of the n_blocks counts in place, the total after them
__global__ void __launch_bounds__(kBlock) k_adaptive_scan(uint32_t* blocks, uint32_t n_blocks)
{
  __shared__ uint32_t s[kBlock];
  const uint32_t per = (n_blocks + kBlock - 1u) / kBlock;
  const uint32_t lo = threadIdx.x * per < n_blocks ? threadIdx.x * per : n_blocks;
  const uint32_t hi = lo + per < n_blocks ? lo + per : n_blocks;
  uint32_t sum = 0;
  for (uint32_t b = lo; b < hi; ++b) sum += blocks[b];
  s[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0u) {
    uint32_t t = 0;
    for (uint32_t k = 0; k < (uint32_t)kBlock; ++k) { const uint32_t v = s[k]; s[k] = t; t += v; }
    blocks[n_blocks] = t;
  }
  __syncthreads();
  uint32_t run = s[threadIdx.x];
  for (uint32_t b = lo; b < hi; ++b) { const uint32_t v = blocks[b]; blocks[b] = run; run += v; }
}

__global__ void __launch_bounds__(kBlock) k_adaptive_select(AdaptiveDev ad, const uint32_t* base_px, const uint32_t* base_xy, uint32_t n_base, const uint32_t* blocks,
                                                          uint32_t* out_px, uint32_t* out_xy)
{
  __shared__ uint32_t s_w[kBlock / 64];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t px = 0;
  bool act = false;
  if (i < n_base) { px = base_px[i]; act = adaptive_active(ad, px); }
  const unsigned long long m = __ballot(act);
  if (lane == 0u) s_w[wave] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t pos = blocks[blockIdx.x] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
  for (uint32_t w = 0; w < wave; ++w) pos += s_w[w];
  if (act) { out_px[pos] = px; out_xy[pos] = base_xy[i]; }
}

// ------------------------------------------------------------------------------------------------
// closest hit: one lane per ray, grid-stride over the queue (binary-BVH fallback shares this kernel)
template <bool COUNT, bool WIDE, bool ALPHA>
__global__ void __launch_bounds__(kBlock) k_trace_closest_static(SceneDev sc, PoolDev pool, uint32_t depth, TraceCounters tc)
{
  pass_priority();
  const uint32_t* cnt = pool.counters + depth * kCounterStride;
  const uint32_t count = cnt[CNT_RAD];
  const uint32_t* q = pool.q_rad[depth & 1u];
  uint32_t nn = 0, nt = 0, nr = 0;
  WaveSteps ws;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
    const uint32_t p = q[i];
    if (COUNT) nr++;
    const float4 o = pool.ray_o[p], d = pool.ray_d[p];
    HitRec h;
    const uint32_t nn0 = nn;
    if (WIDE) traverse_bvh8<false, COUNT, false, ALPHA>(sc.bvh8, mk3(o), mk3(d), o.w, h, nn, nt, &ws, nullptr, 0, &sc);
    else traverse_bvh2<false, COUNT, ALPHA>(sc.bvh2, mk3(o), mk3(d), o.w, h, nn, nt, &sc);
    if (COUNT) { const uint32_t k = nn - nn0; int b = 0; while (b < 7 && k > (8u << b)) ++b; atomicAdd(tc.hist + b, 1ull); }
    pool.hit[p] = make_float4(h.t, h.u, h.v, __uint_as_float(h.prim));
    pool.q_prim[i] = h.prim;
  }
  if (COUNT) {
    atomicAdd(tc.nodes, (unsigned long long)nn);
    atomicAdd(tc.tris, (unsigned long long)nt);
    atomicAdd(tc.rays, (unsigned long long)nr);
    if (ws.node) atomicAdd(tc.wave_nodes, (unsigned long long)ws.node);
    if (ws.tri) atomicAdd(tc.wave_tris, (unsigned long long)ws.tri);
  }
}

// closest hit over the 8-wide BVH, wave-cooperative triangle tests (fh_trace.h: traverse_bvh8_coop)
template <bool COUNT, bool ALPHA>
__global__ void __launch_bounds__(kBlock) k_trace_closest_coop(SceneDev sc, PoolDev pool, uint32_t depth, TraceCounters tc, uint32_t flush)
{
  pass_priority();
  extern __shared__ __attribute__((aligned(16))) uint2 lds_stack[];  // [entry][thread], sized by the launcher for the depth of the BVH
  __shared__ __attribute__((aligned(16))) unsigned char lds[(kBlock / 64) * kCoopLdsBytesPerWave];
  const CoopLds cl = coop_lds(lds, threadIdx.x >> 6);
  const uint32_t* cnt = pool.counters + depth * kCounterStride;
  const uint32_t count = cnt[CNT_RAD];
  const uint32_t* q = pool.q_rad[depth & 1u];
  uint32_t nn = 0, nt = 0, nr = 0;
  WaveSteps ws;
  // the loop bound is per wave, so that all 64 lanes enter the traversal together
  for (uint32_t base = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < count; base += gridDim.x * blockDim.x) {
    const uint32_t i = base + (threadIdx.x & 63u);
    const bool valid = i < count;
    const uint32_t p = valid ? q[i] : 0u;
    if (COUNT && valid) nr++;
    const float4 o = valid ? pool.ray_o[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f), d = valid ? pool.ray_d[p] : make_float4(0.0f, 0.0f, 1.0f, 0.0f);
    HitRec h;
    const uint32_t nn0 = nn;
    traverse_bvh8_coop<false, COUNT, true, ALPHA>(sc.bvh8, valid, mk3(o), mk3(d), o.w, h, nn, nt, &ws, cl, flush, lds_stack, (int)sc.bvh8.depth, &sc);
    if (COUNT && valid) { const uint32_t k = nn - nn0; int b = 0; while (b < 7 && k > (8u << b)) ++b; atomicAdd(tc.hist + b, 1ull); }
    if (valid) { pool.hit[p] = make_float4(h.t, h.u, h.v, __uint_as_float(h.prim)); pool.q_prim[i] = h.prim; }
  }
  if (COUNT) {
    atomicAdd(tc.nodes, (unsigned long long)nn);
    atomicAdd(tc.tris, (unsigned long long)nt);
    atomicAdd(tc.rays, (unsigned long long)nr);
    if (ws.node) atomicAdd(tc.wave_nodes, (unsigned long long)ws.node);
    if (ws.tri) atomicAdd(tc.wave_tris, (unsigned long long)ws.tri);
  }
}

// ------------------------------------------------------------------------------------------------
// Streaming kernels (fh_trace.h: traverse_stream): the grid is sized to the resident wave slots of the chip; every wave draws
// chunks of the bounce's queue from a global cursor (ChunkFeed) and hands the rays to its lanes as they become idle.

// instrumented build: per-lane histogram of nodes visited per ray (8 bins x 16 bits; a lane traces far fewer than 65535 rays),
// flushed once per lane instead of one contended atomic per ray
struct HistPack {
  unsigned long long w[2] = {0ull, 0ull};
  FH_D void add(uint32_t nodes) { int b = 0; while (b < 7 && nodes > (8u << b)) ++b; if (b < 4) w[0] += 1ull << (16 * b); else w[1] += 1ull << (16 * (b - 4)); }
  FH_D void flush(unsigned long long* hist) const
  {
    for (int b = 0; b < 8; ++b) { const unsigned long long v = (w[b >> 2] >> (16 * (b & 3))) & 0xffffull; if (v) atomicAdd(hist + b, v); }
  }
};

// Queue entries a wave takes per global atomic.  `chunk` packs the range the launcher allows: low 16 bits the default, high 16 bits the maximum.  The cursor
// is ONE address and serves ~55 M returning atomics/s: at 64 rays per atomic that caps a launch at ~3.5 G rays/s, which rays through a tiny BVH exceed
// (Cornell box: 4.2 -> 13 G closest-hit rays/s with 256).  Large chunks cost elsewhere -- a queue shorter than waves x chunk leaves waves without work, and on a
// big BVH consecutive chunks traced by different waves at the same time share the caches -- so the launcher raises the maximum only for small trees and the
// kernel stays below a quarter of a wave's even share of the queue.
FH_D uint32_t stream_chunk_for(uint32_t count, uint32_t chunk)
{
  const uint32_t lo = chunk & 0xffffu, hi = chunk >> 16;
  if (hi <= lo) return lo;
  const uint32_t share = count / (gridDim.x * (kBlock / 64u) * 4u);
  const uint32_t c = share & ~63u;
  return c < lo ? lo : (c > hi ? hi : c);
}

// Small launches (the reference's callers render 1 or 16 samples per call, controller.cpp:224, rtcamp8.cpp:183-189).  The grid of a streaming launch is every
// resident wave slot of the chip; with a short queue every one of those waves draws one chunk and runs it at a fraction of its lanes, six to a SIMD, all
// competing for the SIMD's issue slots: the launch then takes (steps of its longest ray) x (six mostly empty waves' node tests) -- 0.34 ms for the 330 k
// camera rays of a 1-spp 1080p frame of the 1 M-triangle scene, which at the kernel's throughput are 0.07 ms of work.  So only as many workgroups take part
// as the queue can give `min_rays` entries per wave: the others leave at once, the SIMDs hold one or two waves whose steps are as short as memory latency lets them
// be, and in-wave refill keeps their lanes busy.  Big launches are untouched (every workgroup takes part from 6144 x min_rays entries on).
FH_D bool stream_block_idle(uint32_t count, uint32_t min_rays) { return blockIdx.x != 0u && (unsigned long long)blockIdx.x * (kBlock / 64u) * min_rays >= count; }

template <bool ALPHA>
struct AlphaLds { static FH_D void attach(CoopLds&) {} };
template <>
struct AlphaLds<true> {
  static FH_D void attach(CoopLds& cl)
  {
    __shared__ __attribute__((aligned(16))) unsigned char lds_alpha[kAlphaLdsBytesPerBlock];
    alpha_ring(cl, lds_alpha, threadIdx.x >> 6);
  }
};

// direction.w of a ray record (store_secondary below, PoolSink::next): 0 = no ray; otherwise 1 + the wide node the ray starts its traversal at (1: the root)
FH_D bool sec_present(const float4& d4) { return __float_as_uint(d4.w) != 0u; }
FH_D uint32_t start_node_of(const float4& d4) { const uint32_t b = __float_as_uint(d4.w); return b ? b - 1u : 0u; }

template <bool COUNT>
struct ClosestStream {
  static constexpr bool all_any = false;
  static constexpr bool can_climb = false;
  const PoolDev& pool;
  const uint32_t* q;
  ChunkFeed feed;
  uint32_t p = 0, qi = 0;  // path slot and queue entry of the lane's ray
  uint32_t start = 0;      // wide node the ray starts its traversal at (0: the root; camera rays)
  uint32_t n_rays = 0;
  unsigned long long* hist;
  HistPack hp;
  FH_D ClosestStream(const PoolDev& pl, const uint32_t* qq, const ChunkFeed& f, unsigned long long* hs) : pool(pl), q(qq), feed(f), hist(hs) {}
  FH_D bool advance(f3&, f3&, float&, bool&) { return false; }
  FH_D bool take(uint32_t i, f3& o, f3& d, float& tmax, bool& any)
  {
    if (i >= feed.end) return false;
    p = q[i];
    qi = i;
    const float4 o4 = pool.ray_o[p], d4 = pool.ray_d[p];
    o = mk3(o4); d = mk3(d4); tmax = o4.w; any = false;
    start = start_node_of(d4);
    if (COUNT) n_rays++;
    return true;
  }
  FH_D void commit(bool, const HitRec& h, uint32_t nodes)
  {
    pool.hit[p] = make_float4(h.t, h.u, h.v, __uint_as_float(h.prim));
    pool.q_prim[qi] = h.prim;
    if (COUNT) hp.add(nodes);
  }
  FH_D bool drained() const { return feed.drained(); }
  FH_D bool followup() const { return false; }
  FH_D uint32_t start_node() const { return start; }
};

template <bool COUNT, bool ALPHA>
__global__ void __launch_bounds__(kBlock, COUNT ? 1 : FH_STREAM_BLOCKS_CLOSEST) k_trace_closest_stream(SceneDev sc, PoolDev pool, uint32_t depth, TraceCounters tc, uint32_t flush, uint32_t refill, uint32_t chunk, uint32_t min_rays,
                                                                 StackSpill spill)
{
  pass_priority();
  __shared__ __attribute__((aligned(16))) unsigned char lds[(kBlock / 64) * kCoopLdsBytesPerWave];
  const uint32_t count = pool.counters[depth * kCounterStride + CNT_RAD];
  if (stream_block_idle(count, min_rays)) return;
  const ClockStamp stamp;
  CoopLds cl = coop_lds(lds, threadIdx.x >> 6);
  AlphaLds<AlphaDefer<false, ALPHA>::value>::attach(cl);  // candidates waiting for their any-hit test (fh_trace.h: alpha_ring): LDS of the kernels with the test compiled in only
  uint32_t nn = 0, nt = 0;
  WaveSteps ws;
  ClosestStream<COUNT> pol(pool, pool.q_rad[depth & 1u], ChunkFeed(pool.counters + depth * kCounterStride + CNT_CUR_CLOSEST, count, stream_chunk_for(count, chunk)), tc.hist);
  extern __shared__ __attribute__((aligned(16))) uint2 lds_stack[];  // the traversal stack of every lane: [entry][thread], as many entries as the BVH has levels
  // (no LDS copy of the top nodes here, fh_trace.h stage_top_nodes: the closest-hit launch gained 0.9 % alone on configs[2] and LOST 1.7 % on configs[3], where the ring of parked any-hit tests already takes its LDS)
  traverse_stream<false, COUNT, true, ALPHA>(sc.bvh8, pol, nn, nt, &ws, cl, flush, refill, lds_stack, (int)sc.bvh8.depth, &sc, spill);
  stamp.commit(tc.clk);
  if (COUNT) {
    atomicAdd(tc.nodes, (unsigned long long)nn);
    atomicAdd(tc.tris, (unsigned long long)nt);
    atomicAdd(tc.rays, (unsigned long long)pol.n_rays);
    pol.hp.flush(tc.hist);
    if (ws.node) atomicAdd(tc.wave_nodes, (unsigned long long)ws.node);
    if (ws.tri) atomicAdd(tc.wave_tris, (unsigned long long)ws.tri);
  }
}

// ------------------------------------------------------------------------------------------------
// Sort the hits of this bounce into per-class queues.  Appends are aggregated per block: wave
// ballot + popcount, a prefix over the block's waves in LDS, one atomic per block and class.
constexpr int kRouteChunks = 8;
__global__ void __launch_bounds__(kBlock) k_route(SceneDev sc, PoolDev pool, uint32_t depth, uint32_t n_classes, unsigned long long* hit_counter)
{
  pass_priority();
  // A workgroup takes kRouteChunks x 256 consecutive entries per round and reserves its part of every class queue with ONE returning atomic per class: a class counter is one
  // address, the chip serves ~85 M returning atomics per address and second, and with 256 entries per atomic the 357 M closest hits of a configs[2] frame were 1.4 M atomics per
  // counter -- 16.4 ms of the kernel's 16.6 (profiles/README.md r4-20)
  __shared__ uint32_t wave_cnt[kMaxClasses][kRouteChunks * (kBlock / 64)];
  __shared__ uint32_t block_base[kMaxClasses];
  uint32_t* cnt = pool.counters + depth * kCounterStride;
  const uint32_t count = cnt[CNT_RAD];
  const uint32_t* q = pool.q_rad[depth & 1u];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t base = blockIdx.x * blockDim.x * kRouteChunks; base < count; base += gridDim.x * blockDim.x * kRouteChunks) {
    uint32_t p[kRouteChunks], cls[kRouteChunks], rank[kRouteChunks];
#pragma unroll
    for (int c = 0; c < kRouteChunks; ++c) {
      const uint32_t i = base + (uint32_t)c * blockDim.x + threadIdx.x;
      p[c] = 0u; cls[c] = 0xffu; rank[c] = 0u;
      if (i < count) {
        p[c] = q[i];
        const uint32_t prim = pool.q_prim[i];  // (= the face id bits of pool.hit[p].w, from a stream)
        if (prim != 0xffffffffu) cls[c] = sc.face_cls[prim] & 0x1fu;
      }
    }
#pragma unroll
    for (int c = 0; c < kRouteChunks; ++c)
      for (uint32_t k = 0; k < n_classes; ++k) {
        const unsigned long long m = __ballot(cls[c] == k);
        if (lane == 0) wave_cnt[k][c * (kBlock / 64) + wave] = (uint32_t)__popcll(m);
        if (cls[c] == k) rank[c] = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      }
    __syncthreads();
    if (threadIdx.x < n_classes) {
      uint32_t total = 0;
      for (uint32_t w = 0; w < kRouteChunks * (kBlock / 64); ++w) { const uint32_t v = wave_cnt[threadIdx.x][w]; wave_cnt[threadIdx.x][w] = total; total += v; }
      block_base[threadIdx.x] = total ? atomicAdd(&cnt[CNT_CLS + threadIdx.x], total) : 0u;
      if (hit_counter && total) atomicAdd(hit_counter, (unsigned long long)total);  // instrumented runs: surface hits that get shaded
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kRouteChunks; ++c)
      if (cls[c] < n_classes) pool.q_cls[(size_t)cls[c] * pool.capacity + block_base[cls[c]] + wave_cnt[cls[c]][c * (kBlock / 64) + wave] + rank[c]] = p[c];
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------
// paths that leave the scene at depth 0 see the environment directly (pt.cu:504-523)
__global__ void __launch_bounds__(kBlock) k_miss_primary(FrameDev fr, PoolDev pool)
{
  pass_priority();
  __shared__ HosekSky s_sky;
  stage_sky(fr, s_sky);
  __syncthreads();
  const uint32_t count = pool.counters[CNT_RAD];
  const uint32_t* q = pool.q_rad[0];
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
    if (pool.q_prim[i] != 0xffffffffu) continue;  // (the closest hit's face id of queue entry i, as k_route reads it: no path record is touched for a ray that hit)
    const uint32_t p = q[i];
    if (pool.flags[p] & 4u) continue;  // bug-compat mode: an earlier sample of this launch already hit something (k_firsthit_scan)
    const f3 T = mk3(pool.thr[p]);
    const f3 d = mk3(pool.ray_d[p]);
    const f3 r = mk3(pool.rad[p]) + T * env_radiance(fr, d);
    pool.rad[p] = mk4(r, 0.0f);
  }
}

// ------------------------------------------------------------------------------------------------
FH_D int tex_id(const MaterialDev& m, int word) { return __float_as_int(m.w[word]); }

// fill_shading_params (pt.cu:181-280): material constants, overridden by texture lookups where a texture id is set
FH_D MatParams load_params(const SceneDev& sc, const MaterialDev& m, float tu, float tv)
{
  MatParams p;
  p.diffuse = m.w[0];
  p.base_color = tex_id(m, 4) >= 0 ? tex_rgb(sc, tex_id(m, 4), tu, tv) : mk3(m.w[1], m.w[2], m.w[3]);
  p.diffuse_roughness = m.w[5];
  p.specular = m.w[6];
  p.specular_color = tex_id(m, 10) >= 0 ? tex_rgb(sc, tex_id(m, 10), tu, tv) : mk3(m.w[7], m.w[8], m.w[9]);
  p.specular_roughness = clampf(tex_id(m, 12) >= 0 ? tex_rgba(sc, tex_id(m, 12), tu, tv).x : m.w[11], 0.01f, 1.0f);
  p.metalness = tex_id(m, 14) >= 0 ? tex_rgba(sc, tex_id(m, 14), tu, tv).x : m.w[13];
  if (tex_id(m, 15) >= 0) {  // glTF metallic-roughness texture: G = roughness, B = metalness (pt.cu:230-236)
    const float4 mr = tex_rgba(sc, tex_id(m, 15), tu, tv);
    p.specular_roughness = clampf(mr.y, 0.01f, 1.0f);
    p.metalness = clampf(mr.z, 0.0f, 1.0f);
  }
  p.coat = clampf(tex_id(m, 17) >= 0 ? tex_rgba(sc, tex_id(m, 17), tu, tv).x : m.w[16], 0.0f, 1.0f);
  p.coat_color = mk3(1.0f, 1.0f, 1.0f);  // fill_shading_params never copies material.coat_color (pt.cu:238-255)
  p.coat_roughness = clampf(tex_id(m, 22) >= 0 ? tex_rgba(sc, tex_id(m, 22), tu, tv).y : m.w[21], 0.0f, 1.0f);
  p.transmission = m.w[23];
  p.transmission_color = mk3(m.w[24], m.w[25], m.w[26]);
  p.sheen = m.w[27];
  p.sheen_color = mk3(m.w[28], m.w[29], m.w[30]);
  p.sheen_roughness = m.w[31];
  p.subsurface = m.w[32];
  p.subsurface_color = mk3(m.w[33], m.w[34], m.w[35]);
  p.thin_walled = m.w[36];
  return p;
}

// get_emission (pt.cu:131-139)
FH_D f3 emission_of(const SceneDev& sc, const MaterialDev& m, float tu, float tv)
{
  return tex_id(m, 41) >= 0 ? tex_rgb(sc, tex_id(m, 41), tu, tv) : mk3(m.w[38], m.w[39], m.w[40]);
}

// (direction.w of a ray record: 0 = no ray in this place; otherwise 1 + the wide node the ray starts its traversal at -- the node that holds the face it leaves, fh_trace.h:
// bottom-up start -- or 1 = the root.  Read as BITS everywhere: small integers are denormal floats.)
// (contribution.w, read as bits: 0 = the ray's final contribution; kSecWeight = a WEIGHT, to be multiplied by the environment's radiance along the ray's direction
// if the ray escapes -- the deferred mode of the sky and light slots, k_sky_resolve)
constexpr uint32_t kSecWeight = 1u;
FH_D void store_secondary(const PoolDev& pool, uint32_t slot, uint32_t p, f3 o, float tmax, f3 d, bool active, f3 c, uint32_t start_bits = 1u, uint32_t marker = 0u)
{
  const size_t k = pool.sec_at(slot, p);
  pool.sec[k + 1] = mk4(d, __uint_as_float(active ? start_bits : 0u));
  if (!active) return;  // (nobody reads origin or contribution of a place without a ray)
  pool.sec[k] = mk4(o, tmax);
  pool.sec[k + 2] = mk4(c, __uint_as_float(marker));
}


// Sobol' dimensions and CMJ slots of one bounce
struct BounceSlots {
  uint32_t has_lights;
  uint32_t dim_area, dim_light, dim_next, dim_rr;
  uint32_t slot_dir, slot_sky, slot_area, slot_light, slot_next;
  FH_D void set(const FrameDev& fr, uint32_t n_lights, uint32_t depth)
  {
    has_lights = n_lights > 0 ? 1u : 0u;
    const uint32_t dim0 = 1u + depth * fr.n1;  // this bounce's RR dimension (already consumed)
    dim_area = dim0 + 1u;                      // only drawn if has_lights
    dim_light = dim0 + 1u + has_lights;
    dim_next = dim_light + 1u;
    dim_rr = 1u + (depth + 1u) * fr.n1;
    const uint32_t slot0 = 2u + depth * fr.n2;
    slot_dir = slot0;
    slot_sky = slot0 + fr.has_dir;
    slot_area = slot_sky + 1u;
    slot_light = slot_sky + 1u + has_lights;
    slot_next = slot_light + 1u;
  }
  FH_D void load_rows(SobolRows<4>& rows, const uint32_t* tables) const
  {
    const uint32_t dims[4] = {dim_area, dim_light, dim_next, dim_rr};
    load_sobol_rows<4>(rows, tables, dims);
  }
};

struct SecRay { f3 o; float tmax; f3 d; bool active; f3 c; };

// A shadow ray whose pre-multiplied contribution is exactly (+-0, +-0, +-0) cannot change a bit of the result whatever it hits: the radiance it would be added to starts at
// +0 and a sum is -0 only when both terms are, so x + (+-0) == x for every radiance x that can occur.  The reference traces it all the same (pt.cu:837-857 sends the sky's
// shadow ray for a black constant background too: one of three secondary rays per bounce of a Cornell box); here such a ray is stored as "no ray in this
// place".  NaN compares unequal to 0 and stays: a NaN contribution of an unoccluded ray must still reach the radiance and zero the sample (pt.cu:474-478).
FH_D bool contributes(f3 c) { return !(c.x == 0.0f && c.y == 0.0f && c.z == 0.0f); }

// What one shaded hit produces (pt.cu:680-944) goes to a SINK as soon as it exists, so that a kernel that only stores the products
// (k_shade) does not keep them alive in registers next to the BSDF state; k_tail, which traces the rays itself, collects them in
// registers.  Sink interface:
//   aov(position, normal, albedo, u, v)         first hit only                              (pt.cu:745-751)
//   emissive(L)                                 first hit on an emitter: the path ends      (pt.cu:754-759)
//   secondary(slot, origin, tmax, dir, active, contribution)      one per enabled NEE slot, in the reference's order
//   light_pending(T, cos, f, pdf)               scenes with emitters: what the light ray's MIS weight needs once its hit is known
//   next(origin, dir, T)                        the path continues
struct ShadeOut {      // register sink (k_tail)
  bool emissive_done = false;  // first hit on an emitter: radiance updated, path ends, nothing else valid
  bool shaded = false;         // secondary rays valid
  bool cont = false;           // next ray valid
  f3 L;                // radiance after a directly visible emitter
  f3 T;                // throughput for the next bounce (after Russian roulette)
  SecRay sec[SEC_COUNT];
  f3 lp_T, lp_f;       // light ray with emitters: throughput before the update, BSDF value
  float lp_cos, lp_pdf;
  f3 next_o, next_d;
  FH_D ShadeOut() { for (uint32_t k = 0; k < SEC_COUNT; ++k) sec[k].active = false; }
  FH_D void aov(f3, f3, f3, float, float) {}
  FH_D void emissive(f3 l) { L = l; emissive_done = true; }
  FH_D void secondary(uint32_t slot, f3 o, float tmax, f3 d, bool active, f3 c) { shaded = true; sec[slot] = SecRay{o, tmax, d, active, c}; }
  FH_D void light_pending(f3 t, float c, f3 f, float pdf) { lp_T = t; lp_cos = c; lp_f = f; lp_pdf = pdf; }
  FH_D void next(f3 o, f3 d, f3 t) { cont = true; next_o = o; next_d = d; T = t; }
  FH_D void start_node(uint32_t) {}  // (the fused tail's rays start at the root)
};

struct PoolSink {      // memory sink (k_shade): path slot p of the pool
  const PoolDev& pool;
  uint32_t p;
  float hit_t;
  bool shaded = false, cont = false;
  f3 origin;           // where the path's rays leave the surface (cell key of the bounce queues)
  uint32_t start_bits; // 1 + the wide node that holds the face the rays leave (1: they start at the root)
  FH_D PoolSink(const PoolDev& pl, uint32_t slot, float t, uint32_t sb = 1u) : pool(pl), p(slot), hit_t(t), origin(mk3(0.0f)), start_bits(sb) {}
  FH_D void aov(f3 position, f3 normal, f3 albedo, float u, float v)
  {
    pool.aov_position[p] = mk4(position, 0.0f);
    pool.aov_normal[p] = mk4(normal, 0.0f);
    pool.aov_albedo[p] = mk4(albedo, 0.0f);
    pool.aov_texdepth[p] = make_float4(u, v, hit_t, 0.0f);
    pool.flags[p] |= 1u;
  }
  FH_D void emissive(f3 l) { pool.rad[p] = mk4(l, 0.0f); }
  FH_D void start_node(uint32_t bits) { start_bits = bits ? bits : 1u; }
  FH_D void secondary(uint32_t slot, f3 o, float tmax, f3 d, bool active, f3 c)
  {
    store_secondary(pool, slot, p, o, tmax, d, active, c, start_bits);
    if (!shaded) origin = o;  // all rays of a path leave (almost) the same point
    shaded = true;
  }
  // (deferred mode: the ray carries its weight w; what it adds if it escapes, w * env_radiance(d), is formed by k_sky_resolve)
  FH_D void secondary_weight(uint32_t slot, f3 o, float tmax, f3 d, f3 w)
  {
    store_secondary(pool, slot, p, o, tmax, d, true, w, start_bits, kSecWeight);
    if (!shaded) origin = o;
    shaded = true;
  }
  FH_D void light_pending(f3 t, float c, f3 f, float pdf) { pool.lp_a[p] = mk4(t, c); pool.lp_b[p] = mk4(f, pdf); }
  FH_D void next(f3 o, f3 d, f3 t)
  {
    pool.ray_o[p] = mk4(o, 1e9f);
    pool.ray_d[p] = mk4(d, __uint_as_float(start_bits));
    pool.thr[p] = mk4(t, 0.0f);
    if (!shaded) origin = o;
    cont = true;
  }
};

// ENV (fh_set_env_sampling): the sky ray is drawn from the mixture of fh_envmap.h and the two light-ray weights that stand against it use that density; `env` is read
// by these variants only, and nothing else of the hit differs
// LT (fh_set_light_sampling): the emitter of the area shadow ray is picked from the table of fh_lights.h and its density is the pick's probability over the area; `ltab`
// is read by these variants only.  (The BSDF-sampled light ray's side of it is resolve_light_ray<true>.)
// DEFER (PoolSink, scenes without emitters, no ENV / LT): the sky ray and the light ray are stored with their WEIGHT and the environment is evaluated by k_sky_resolve for
// the rays that escape -- four of five do not.  A weight of exactly zero keeps today's path, because its ray is traced today only when the radiance is NaN (every
// direction below the Hosek horizon) and that NaN must reach the sample: the environment is evaluated here and the product stored as final.  A non-zero weight whose
// product would have been +-0 is now traced and adds +-0, which changes no bit (above `contributes`).
template <uint32_t LOBES, bool ENV = false, bool LT = false, bool DEFER = false, class Sink>
FH_D void shade_hit(const SceneDev& sc, const FrameDev& fr, const SobolRows<4>& rows, const BounceSlots& bs, uint32_t depth, float4 hit, f3 rd, f3 T, f3 L, uint32_t image_idx, uint32_t n_spp,
                    Sink& out, bool first = true, const EnvTable* env = nullptr, const LightTable* ltab = nullptr)
{
  static_assert(!DEFER || (!ENV && !LT), "the deferred slots are those of the plain draw");
  const uint32_t has_lights = bs.has_lights;
  const uint32_t prim = __float_as_uint(hit.w);
  const float bu = hit.y, bv = hit.z;
  const uint32_t sidx = image_idx + n_spp * fr.width * fr.height;

  // surface (pt.cu:141-179) from the pre-transformed face record
  const float4 r0 = sc.face_rec[kFaceRec * (size_t)prim], r1 = sc.face_rec[kFaceRec * (size_t)prim + 1], r2 = sc.face_rec[kFaceRec * (size_t)prim + 2];
  const float4 r3 = sc.face_rec[kFaceRec * (size_t)prim + 3], r4 = sc.face_rec[kFaceRec * (size_t)prim + 4], r5 = sc.face_rec[kFaceRec * (size_t)prim + 5];
  const float4 r6 = sc.face_rec[kFaceRec * (size_t)prim + 6];
  // (.z of the record's last vector: 1 + the wide node that holds the face, written by the BVH build -- where this bounce's first-hit rays start their traversal, fh_trace.h)
  out.start_node(sc.face_node ? __float_as_uint(r6.z) : 0u);
  const f3 p0 = mk3(r0), p1 = mk3(r1), p2 = mk3(r2);
  const float bw = 1.0f - bu - bv;
  const f3 x = bw * p0 + bu * p1 + bv * p2;
  f3 ng = normalize(cross(p1 - p0, p2 - p0));
  f3 ns = normalize(bw * mk3(r3) + bu * mk3(r4) + bv * mk3(r5));
  const float tu = bw * r0.w + bu * r2.w + bv * r4.w;
  const float tv = bw * r1.w + bu * r3.w + bv * r5.w;
  const bool entering = dot(-rd, ng) > 0;
  ns = entering ? ns : -ns;
  ng = entering ? ng : -ng;
  f3 tangent, bitangent;
  onb(ns, tangent, bitangent);
  const MaterialDev& mat = sc.materials[__float_as_uint(r6.x)];
  const MatParams sp = load_params(sc, mat, tu, tv);
  const f3 ns_geo = ns, tangent_geo = tangent, bitangent_geo = bitangent;  // surf_info frame before the maps
  if (tex_id(mat, 42) >= 0) {  // bump mapping with a height map (pt.cu:709-731)
    const fht_texture& hm = sc.textures[tex_id(mat, 42)];
    const float du = 1.0f / hm.width, dv = 1.0f / hm.height;
    const float hv = tex_rgba(sc, tex_id(mat, 42), tu, tv).x;
    const float dfdu = tex_rgba(sc, tex_id(mat, 42), tu + du, tv).x - hv;
    const float dfdv = tex_rgba(sc, tex_id(mat, 42), tu, tv + dv).x - hv;
    tangent = normalize(tangent_geo + dfdu * ns_geo);
    bitangent = normalize(bitangent_geo + dfdv * ns_geo);
    ns = normalize(cross(tangent, bitangent));
  }
  if (tex_id(mat, 43) >= 0) {  // normal mapping (pt.cu:733-742)
    f3 value = tex_rgb(sc, tex_id(mat, 43), tu, tv);
    value = 2.0f * value - 1.0f;
    ns = normalize(to_world(value, tangent_geo, bitangent_geo, ns_geo));
    onb(ns, tangent, bitangent);
  }

  if (depth == 0 && first) {  // first hit: AOVs and directly visible emitters (pt.cu:745-760); `first` is false only in the bug-compat mode (k_firsthit_scan)
    out.aov(x, ns, sp.base_color, tu, tv);
    if (mat.emissive) {
      out.emissive(L + T * emission_of(sc, mat, tu, tv));
      return;
    }
  }
  const f3 wo = to_local(-rd, tangent, ns, bitangent);
  Bsdf<LOBES> bsdf;
  bsdf.init(wo, sp, entering, fr.lut);
  const f3 so = offset_origin(x, ng);

  // directional light (pt.cu:772-793)
  if (fr.has_dir) {
    const f2 pdisk = concentric_disk(cmj_draw(n_spp, image_idx, bs.slot_dir, fr.seed_hash));
    f3 t, b;
    onb(fr.dir_dir, t, b);
    const f3 pl = 1e9f * fr.dir_dir + fr.dir_disk_radius * (t * pdisk.x + b * pdisk.y);
    const f3 sd = normalize(pl - so);
    const f3 wi = to_local(sd, tangent, ns, bitangent);
    const f3 f = bsdf.eval(wo, wi);
    const float pdf = 1.0f;
    const float w = pdf / (pdf + bsdf.eval_pdf(wo, wi));
    const f3 c = clamp01(T * w * f * abs_cos(wi) / pdf) * fr.dir_le;
    out.secondary(SEC_DIR, so, 1e9f - 0.001f, sd, contributes(c), c);
  }
  // sky / constant background (pt.cu:817-857)
  if constexpr (ENV) {
    float pdf;
    uint32_t cell;
    const f3 sd = env_sample(*env, cmj_draw(n_spp, image_idx, bs.slot_sky, fr.seed_hash), tangent, ns, bitangent, pdf, cell);
    const f3 wi = to_local(sd, tangent, ns, bitangent);
    // A direction at or below the shading horizon adds nothing.  The table draws over the whole sphere, and the BSDF's evaluation is not meant for down there: today's
    // draw never asks it, and what it answers is the upper side's value with |cos| (rho / pi for the diffuse lobe), so a surface that faces the sun with its geometry
    // and not with its shading normal would be lit through its back.  (The ray starts on the outer side whatever its direction, so below the geometric horizon the
    // surface itself stops it, as it does a transmissive floor's today.)
    // Nor does a weight that is not finite.  Every hit on the back side of an opaque surface has one: all lobe weights are 0 there, the lobe pmf is 0 / 0 and eval_pdf
    // NaN.  regularize_weight would make it 1, and the expectation of 1 * L(d) is the integral of p * L -- a glow under the cosine draw, the sun's radiance times its
    // share of the table under this one (measured on the textured interior, whose curtains and cards are seen from both sides: a frame mean of 42 against 0.08).
    f3 c = mk3(0.0f);
    if (wi.y > 0.0f) {
      const f3 f = bsdf.eval(wo, wi);
      const float w = pdf / (pdf + bsdf.eval_pdf(wo, wi));
      const f3 weight = T * w * f * abs_cos(wi) / pdf;
      if (!bad3(weight)) c = clamp01(weight) * env_radiance(fr, sd);
    }
    out.secondary(SEC_SKY, so, 1e9f - 0.001f, sd, contributes(c), c);
  } else {
    const f3 wi = cosine_hemisphere(cmj_draw(n_spp, image_idx, bs.slot_sky, fr.seed_hash));
    const f3 sd = to_world(wi, tangent, ns, bitangent);
    const f3 f = bsdf.eval(wo, wi);
    const float pdf = abs_cos(wi) / kPi;
    const float w = pdf / (pdf + bsdf.eval_pdf(wo, wi));
    if constexpr (DEFER) {
      const f3 cw = clamp01(T * w * f * abs_cos(wi) / pdf);
      if (contributes(cw)) out.secondary_weight(SEC_SKY, so, 1e9f - 0.001f, sd, cw);
      else {
        const f3 c = cw * env_radiance(fr, sd);
        out.secondary(SEC_SKY, so, 1e9f - 0.001f, sd, contributes(c), c);
      }
    } else {
      const f3 c = clamp01(T * w * f * abs_cos(wi) / pdf) * env_radiance(fr, sd);
      out.secondary(SEC_SKY, so, 1e9f - 0.001f, sd, contributes(c), c);
    }
  }
  // area lights (pt.cu:860-889, :282-322)
  if (has_lights) {
    const float u1 = sobol_draw_bytes(rows.m[0], sidx, bs.dim_area, fr.seed_hash);
    const f2 u2 = cmj_draw(n_spp, image_idx, bs.slot_area, fr.seed_hash);
    uint32_t li;
    float ris = 1.0f;  // fh_set_light_resampling: G_y / (S / M) of the chosen candidate (a run-time branch of the LT forms, not a third axis of them)
    if constexpr (LT) {
      if (ltab->candidates > 1u) {
        const LightChoice ch = light_resample(*ltab, sc.n_lights, u1, light_usel(image_idx, n_spp, bs.dim_area, fr.seed_hash), so.x, so.y, so.z, ns.x, ns.y, ns.z);
        li = ch.index;
        ris = ch.ratio;
      } else {
        li = light_pick(ltab->cdf, sc.n_lights, ltab->uniform, u1);
      }
    } else {
      li = (uint32_t)(u1 * sc.n_lights);
      li = li < sc.n_lights - 1u ? li : sc.n_lights - 1u;
    }
    const AreaLightDev lt = sc.lights[li];
    const f2 bc = triangle_barycentric(u2);
    const float4 l0 = sc.face_rec[kFaceRec * (size_t)lt.face], l1 = sc.face_rec[kFaceRec * (size_t)lt.face + 1], l2 = sc.face_rec[kFaceRec * (size_t)lt.face + 2];
    const float4 l3 = sc.face_rec[kFaceRec * (size_t)lt.face + 3], l4 = sc.face_rec[kFaceRec * (size_t)lt.face + 4], l5 = sc.face_rec[kFaceRec * (size_t)lt.face + 5];
    const float lw = 1.0f - bc.x - bc.y;
    const f3 lp = lw * mk3(l0) + bc.x * mk3(l1) + bc.y * mk3(l2);
    const f3 ln = lw * mk3(l3) + bc.x * mk3(l4) + bc.y * mk3(l5);
    const float area = 0.5f * length(cross(mk3(l1) - mk3(l0), mk3(l2) - mk3(l0)));
    const MaterialDev& lm = sc.materials[lt.material];
    const f3 le = emission_of(sc, lm, lw * l0.w + bc.x * l2.w + bc.y * l4.w, lw * l1.w + bc.x * l3.w + bc.y * l5.w);
    float pdf_area;
    if constexpr (LT) pdf_area = ltab->pick_p[lt.face] / area;
    else pdf_area = 1.0f / (sc.n_lights * area);
    const f3 sd = normalize(lp - so);
    const float r = length(lp - so);
    const bool facing = dot(-sd, ln) > 0.0f;
    const f3 wi = to_local(sd, tangent, ns, bitangent);
    const f3 f = bsdf.eval(wo, wi);
    const float pdf = r * r / fabsf(dot(-sd, ln)) * pdf_area;
    const float w = pdf / (pdf + bsdf.eval_pdf(wo, wi));  // (the table's density, resampled or not: what resolve_light_ray<true> weighs the other site with)
    float pdf_div = pdf;
    if constexpr (LT) {
      if (ltab->candidates > 1u) pdf_div = r * r / fabsf(dot(-sd, ln)) * (pdf_area * ris);
    }
    const f3 c = clamp01(T * w * f * abs_cos(wi) / pdf_div) * le;
    out.secondary(SEC_AREA, so, r - 0.001f, sd, facing && contributes(c), c);
  }
  // BSDF-sampled light ray (pt.cu:893-925)
  {
    f3 f;
    float pdf;
    const float u1 = sobol_draw_bytes(rows.m[1], sidx, bs.dim_light, fr.seed_hash);
    const f2 u2 = cmj_draw(n_spp, image_idx, bs.slot_light, fr.seed_hash);
    const f3 wi = bsdf.sample(wo, u1, u2, f, pdf);
    const f3 ld = to_world(wi, tangent, ns, bitangent);
    const bool transmitted = dot(ld, ng) < 0;
    const f3 lo = offset_origin(x, transmitted ? -ng : ng);
    if (has_lights) {
      // the MIS weight needs the hit (emitter or sky): finished once the closest hit is known
      if constexpr (ENV) {
        // resolve_light_ray takes pdf_light = cos' / pi on a miss and T * w * f * cos' / pdf in both branches: with cos' = pi * p(ld) the miss density is the
        // mixture's p(ld), and f' = f * |cos| / cos' keeps the product T * w * f * |cos| / pdf where the ray escapes and where it finds an emitter
        const float cosp = kPi * env_pdf(*env, env_dir(ld), env_dir(ns), nullptr);
        out.light_pending(T, cosp, f * (abs_cos(wi) / cosp), pdf);
      } else {
        out.light_pending(T, abs_cos(wi), f, pdf);
      }
      out.secondary(SEC_LIGHT, lo, 1e9f, ld, true, mk3(0.0f));
    } else {
      // no emitters: the ray contributes only if it escapes, with the sky's cosine pdf (pt.cu:917-919), or the mixture's
      float pdf_light = abs_cos(wi) / kPi;
      if constexpr (ENV) pdf_light = env_pdf(*env, env_dir(ld), env_dir(ns), nullptr);
      const float w = pdf / (pdf + pdf_light);
      if constexpr (DEFER) {
        const f3 cw = clamp01(T * w * f * abs_cos(wi) / pdf);
        if (contributes(cw)) out.secondary_weight(SEC_LIGHT, lo, 1e9f, ld, cw);
        else {
          const f3 c = cw * env_radiance(fr, ld);
          out.secondary(SEC_LIGHT, lo, 1e9f, ld, contributes(c), c);
        }
      } else {
        const f3 c = clamp01(T * w * f * abs_cos(wi) / pdf) * env_radiance(fr, ld);
        out.secondary(SEC_LIGHT, lo, 1e9f, ld, contributes(c), c);
      }
    }
  }
  // next direction (pt.cu:928-943) and the next bounce's Russian roulette (pt.cu:457-471)
  {
    f3 f;
    float pdf;
    const float u1 = sobol_draw_bytes(rows.m[2], sidx, bs.dim_next, fr.seed_hash);
    const f2 u2 = cmj_draw(n_spp, image_idx, bs.slot_next, fr.seed_hash);
    const f3 wi = bsdf.sample(wo, u1, u2, f, pdf);
    const f3 wd = to_world(wi, tangent, ns, bitangent);
    f3 Tn = T;
    Tn *= f * abs_cos(wi) / pdf;
    const bool transmitted = dot(wd, ng) < 0;
    const f3 no = offset_origin(x, transmitted ? -ng : ng);
    if (!bad3(Tn) && depth + 1u < fr.max_depth) {
      const float prr = clampf(lum(Tn), 0.0f, 1.0f);
      const float u = sobol_draw_bytes(rows.m[3], sidx, bs.dim_rr, fr.seed_hash);
      if (!(u >= prr)) out.next(no, wd, Tn / prr);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Spatial ordering of the bounce queues.  Rays leaving hit points are incoherent; traced in the order the shade kernels emit them,
// the lanes of a wave walk unrelated parts of the BVH and every L2 sees all of it.  Sorting 4 M random rays of the 1 M-triangle
// soup by the Morton cell of their origin made the same traversal kernel 1.4-1.55x faster (tools/sort_probe.py), so the queue
// entries are brought into cell order first: a counting sort over kCells keys (histogram, scan, scatter), ~0.3 ms for 40 M entries.
// Only the ORDER of queue entries changes: every path's arithmetic is untouched, so results are bit-identical.
FH_D uint32_t spread3(uint32_t v) { return (v & 1u) | ((v & 2u) << 2) | ((v & 4u) << 4) | ((v & 8u) << 6); }  // 4 bits -> every third bit
FH_D uint32_t cell_of(const FrameDev& fr, f3 p)
{
  const float m = (float)((1u << kCellBits) - 1u);
  const float fx = fminf(fmaxf((p.x - fr.scene_lo.x) * fr.cell_scale.x, 0.0f), m), fy = fminf(fmaxf((p.y - fr.scene_lo.y) * fr.cell_scale.y, 0.0f), m),
              fz = fminf(fmaxf((p.z - fr.scene_lo.z) * fr.cell_scale.z, 0.0f), m);
  return spread3((uint32_t)fx) | (spread3((uint32_t)fy) << 1) | (spread3((uint32_t)fz) << 2);
}

constexpr int kSortBlock = 1024;
// contiguous share of block b of n items
FH_D void block_share(uint32_t n, uint32_t& lo, uint32_t& hi)
{
  const uint32_t per = (n + gridDim.x - 1u) / gridDim.x;
  lo = blockIdx.x * per < n ? blockIdx.x * per : n;
  hi = lo + per < n ? lo + per : n;
}

__global__ void __launch_bounds__(kSortBlock) k_cell_hist(const uint32_t* count_ptr, const uint16_t* keys, uint32_t* hist)
{
  pass_priority();
  __shared__ uint32_t h[kCells];
  for (uint32_t b = threadIdx.x; b < kCells; b += kSortBlock) h[b] = 0u;
  __syncthreads();
  uint32_t lo, hi;
  block_share(*count_ptr, lo, hi);
  for (uint32_t i = lo + threadIdx.x; i < hi; i += kSortBlock) atomicAdd(&h[keys[i] & (kCells - 1u)], 1u);
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < kCells; b += kSortBlock)
    if (h[b]) atomicAdd(&hist[b], h[b]);
}

// exclusive scan of the histogram into the cursors; the histogram is left zero for the next sort
__global__ void __launch_bounds__(kSortBlock) k_cell_scan(uint32_t* hist, uint32_t* cursor)
{
  pass_priority();
  __shared__ uint32_t part[kSortBlock];
  constexpr uint32_t per = kCells / kSortBlock;
  uint32_t v[per], sum = 0;
  for (uint32_t k = 0; k < per; ++k) { v[k] = hist[threadIdx.x * per + k]; hist[threadIdx.x * per + k] = 0u; sum += v[k]; }
  part[threadIdx.x] = sum;
  __syncthreads();
  for (uint32_t off = 1; off < kSortBlock; off <<= 1) {
    const uint32_t add = threadIdx.x >= off ? part[threadIdx.x - off] : 0u;
    __syncthreads();
    part[threadIdx.x] += add;
    __syncthreads();
  }
  uint32_t run = part[threadIdx.x] - sum;
  for (uint32_t k = 0; k < per; ++k) { cursor[threadIdx.x * per + k] = run; run += v[k]; }
}

__global__ void __launch_bounds__(kSortBlock) k_cell_scatter(const uint32_t* count_ptr, const uint32_t* q_in, const uint16_t* keys, uint32_t* cursor, uint32_t* q_out)
{
  pass_priority();
  __shared__ uint32_t h[kCells];     // entries of this block per cell, then the running rank inside the block's range of that cell
  __shared__ uint32_t base[kCells];  // start of this block's range inside the cell's global range
  for (uint32_t b = threadIdx.x; b < kCells; b += kSortBlock) h[b] = 0u;
  __syncthreads();
  uint32_t lo, hi;
  block_share(*count_ptr, lo, hi);
  for (uint32_t i = lo + threadIdx.x; i < hi; i += kSortBlock) atomicAdd(&h[keys[i] & (kCells - 1u)], 1u);
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < kCells; b += kSortBlock) {
    base[b] = h[b] ? atomicAdd(&cursor[b], h[b]) : 0u;
    h[b] = 0u;
  }
  __syncthreads();
  for (uint32_t i = lo + threadIdx.x; i < hi; i += kSortBlock) {
    const uint32_t b = keys[i] & (kCells - 1u);
    q_out[base[b] + atomicAdd(&h[b], 1u)] = q_in[i];
  }
}

// The opt-in sampling modes hand their tables to k_shade and to the secondary-ray kernels as a trailing parameter pack: empty for the plain kernel, (EnvTable) for
// fh_set_env_sampling, (UnreadEnvTable, LightTable) or (EnvTable, LightTable) for fh_set_light_sampling; the secondary-ray kernels take nothing or (pick_p).  A pack, not a
// device function shared by several kernels: the body stays inside the kernel and a plain instantiation keeps its name, its arguments and its instruction stream -- after
// ANY edit of these bodies compare a device listing of render.hip with the one before it (tools/kernel_asm_diff.py): the plain kernels may differ in nothing.
struct UnreadEnvTable { EnvTable t; };  // holds the place, and the kernarg offsets, of the environment table in the (-, LightTable) forms: table_of<EnvTable> does not find it
struct DeferSky {};  // k_shade's pack of the deferred mode (shade_hit<..., DEFER>): no table, only the name of the form.  The secondary-ray kernel's is (esc), the escape masks it writes
template <class T>
FH_D const T* table_of() { return nullptr; }
template <class T, class First, class... Rest>
FH_D const T* table_of(const First& f, const Rest&... r)
{
  if constexpr (std::is_same<T, First>::value) return &f;
  else return table_of<T>(r...);
}
FH_D const float* pick_p_of() { return nullptr; }
FH_D const float* pick_p_of(const float* pick_p) { return pick_p; }
FH_D const float* pick_p_of(uint8_t*) { return nullptr; }
FH_D uint8_t* esc_of() { return nullptr; }
FH_D uint8_t* esc_of(const float*) { return nullptr; }
FH_D uint8_t* esc_of(uint8_t* esc) { return esc; }

// (with tables: compiled for the lobe sets of the fused tail (TailLobes), FH_SHADE_BLOCKS workgroups per CU)
template <uint32_t LOBES, int BLOCKS = FH_SHADE_BLOCKS, class... Tables>
__global__ void __launch_bounds__(kBlock, (LOBES == L_ALL ? 1 : BLOCKS)) k_shade(SceneDev sc, FrameDev fr, PoolDev pool, uint32_t cls, uint32_t depth, Tables... tables)
{
  constexpr bool ENV = (std::is_same<Tables, EnvTable>::value || ...), LT = (std::is_same<Tables, LightTable>::value || ...);
  constexpr bool DEFER = (std::is_same<Tables, DeferSky>::value || ...);
  const EnvTable* const env = table_of<EnvTable>(tables...);
  const LightTable* const ltab = table_of<LightTable>(tables...);
  pass_priority();
  // (the grid is sized for every path of the pass; the blocks beyond this class's queue leave before they stage anything)
  if (blockIdx.x * blockDim.x >= pool.counters[depth * kCounterStride + CNT_CLS + cls]) return;
  __shared__ SobolRows<4> rows;
  // the shade kernels run one wave per SIMD (512 registers per lane), so nothing hides a dependent global load: the small tables every
  // hit reads -- the two albedo LUTs and, when there are few of them, the material records -- are staged in LDS once per workgroup
  __shared__ float s_lut[kLutReflFloats + kLutSheenFloats];
  __shared__ MaterialDev s_mat[kMatLds];
  for (uint32_t i = threadIdx.x; i < kLutReflFloats; i += blockDim.x) s_lut[i] = fr.lut.reflection[i];
  for (uint32_t i = threadIdx.x; i < kLutSheenFloats; i += blockDim.x) s_lut[kLutReflFloats + i] = fr.lut.sheen[i];
  fr.lut.reflection = s_lut;
  fr.lut.sheen = s_lut + kLutReflFloats;
  if (sc.n_materials <= kMatLds) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(sc.materials);
    uint32_t* dst = reinterpret_cast<uint32_t*>(s_mat);
    for (uint32_t i = threadIdx.x; i < sc.n_materials * (uint32_t)(sizeof(MaterialDev) / 4); i += blockDim.x) dst[i] = src[i];
    sc.materials = s_mat;
  }
  __shared__ float s_srgb[256];  // the sRGB decode table: twelve lookups per fetch of a colour texture
  if (sc.n_textures) {
    s_srgb[threadIdx.x] = sc.srgb_lut[threadIdx.x];
    sc.srgb_lut = s_srgb;
  }
  __shared__ HosekSky s_sky;
  stage_sky(fr, s_sky);
  BounceSlots bs;
  bs.set(fr, sc.n_lights, depth);
  bs.load_rows(rows, fr.sobol_bytes);  // (ends with the workgroup barrier that also publishes the tables above)

  uint32_t* cnt = pool.counters + depth * kCounterStride;
  uint32_t* cnt_next = cnt + kCounterStride;
  const uint32_t count = cnt[CNT_CLS + cls];
  const uint32_t* q = pool.q_cls + (size_t)cls * pool.capacity;
  const uint32_t qnext = (depth + 1u) & 1u;
  const uint32_t stride = gridDim.x * blockDim.x;
  __shared__ uint32_t s_reserve[2][10];  // (two areas, used alternately: block_queue_reserve)
  uint32_t iter = 0;
  for (uint32_t base = blockIdx.x * blockDim.x; base < count; base += stride) {
    const uint32_t i = base + threadIdx.x;
    const bool valid = i < count;
    bool shaded = false, cont = false;
    uint32_t p = 0, cell = 0;
    if (valid) {
      p = q[i];
      const float4 hit = pool.hit[p];
      PoolSink o(pool, p, hit.x);
      const bool first = depth != 0 || (pool.flags[p] & 4u) == 0u;
      const f3 L = depth == 0u ? mk3(pool.rad[p]) : mk3(0.0f);  // the radiance so far only enters at a directly visible emitter (first hit): later bounces skip the load
      shade_hit<LOBES, ENV, LT, DEFER>(sc, fr, rows, bs, depth, hit, mk3(pool.ray_d[p]), mk3(pool.thr[p]), L, pool.pixel[p], pool.nspp[p], o, first, env, ltab);
      shaded = o.shaded;
      cont = o.cont;
      if (shaded || cont) cell = cell_of(fr, o.origin);
    }
    // queue positions of both appends: one returning atomic per workgroup and queue (fh_device.h: block_queue_reserve)
    uint32_t* const counters2[2] = {&cnt[CNT_SEC], &cnt_next[CNT_RAD]};
    const bool act[2] = {shaded, cont};
    uint32_t pos[2];
    block_queue_reserve<2>(counters2, act, pos, s_reserve[iter & 1u]);
    ++iter;
    if (shaded) { pool.q_sec[pos[0]] = p; pool.key_sec[pos[0]] = (uint16_t)cell; }
    if (cont) { pool.q_rad[qnext][pos[1]] = p; pool.key_rad[pos[1]] = (uint16_t)cell; }
  }
}

// ------------------------------------------------------------------------------------------------
// Finish the BSDF-sampled light ray of a scene with emitters once its closest hit is known
// (pt.cu:952-999 closest-hit light, :531-543 miss light, :910-924 MIS weight).
// LT (fh_set_light_sampling): the emitter's density is its pick probability over its area; pick_p (fh_lights.h: per face) is read by that variant only
template <bool LT = false>
FH_D f3 resolve_light_ray(const SceneDev& sc, const FrameDev& fr, f3 T, float cosw, f3 f, float pdf, f3 ro, f3 ld, bool hit, const HitRec& h, const float* pick_p = nullptr)
{
  f3 le = mk3(0.0f);
  float pdf_light = cosw / kPi;
  bool add = false;
  if (hit) {
    if (sc.face_cls[h.prim] & 0x80u) {
      const size_t fb = kFaceRec * (size_t)h.prim;
      const float4 l0 = sc.face_rec[fb], l1 = sc.face_rec[fb + 1], l2 = sc.face_rec[fb + 2], l3 = sc.face_rec[fb + 3], l4 = sc.face_rec[fb + 4], l5 = sc.face_rec[fb + 5];
      const float lw = 1.0f - h.u - h.v;
      const f3 lp = lw * mk3(l0) + h.u * mk3(l1) + h.v * mk3(l2);
      const f3 ln = lw * mk3(l3) + h.u * mk3(l4) + h.v * mk3(l5);
      if (dot(-ld, ln) > 0.0f) {
        const MaterialDev& lm = sc.materials[__float_as_uint(sc.face_rec[fb + 6].x)];
        le = emission_of(sc, lm, lw * l0.w + h.u * l2.w + h.v * l4.w, lw * l1.w + h.u * l3.w + h.v * l5.w);
        const float area = 0.5f * length(cross(mk3(l1) - mk3(l0), mk3(l2) - mk3(l0)));
        const f3 dl = lp - ro;
        const float r2 = dot(dl, dl);
        float pdf_area;
        if constexpr (LT) pdf_area = pick_p[h.prim] / area;
        else pdf_area = 1.0f / (sc.n_lights * area);
        pdf_light = r2 / fabsf(dot(-ld, ln)) * pdf_area;
        add = true;
      }
    }
  } else {
    le = env_radiance(fr, ld);
    add = true;
  }
  if (!add) return mk3(0.0f);
  const float w = pdf / (pdf + pdf_light);
  return clamp01(T * w * f * cosw / pdf) * le;
}

// secondary rays, binary-BVH fallback: one thread per shaded path, its rays in the reference's order
// PickP (fh_set_light_sampling), here and in the three kernels below: nothing, or the table's pick probabilities per face, which resolve_light_ray<true> reads.  The
// forms that take them are compiled with LIGHTS only: without emitters the mode does nothing.
template <bool COUNT, bool WIDE, bool LIGHTS, bool ALPHA, class... PickP>
__global__ void __launch_bounds__(kBlock) k_trace_secondary_static(SceneDev sc, FrameDev fr, PoolDev pool, uint32_t depth, TraceCounters tc, PickP... pp)
{
  constexpr bool LT = sizeof...(PickP) != 0;
  static_assert(LIGHTS || !LT, "pick probabilities without emitters");
  const float* const pick_p = pick_p_of(pp...);
  pass_priority();
  extern __shared__ __attribute__((aligned(16))) uint2 lds_stack[];  // [entry][thread], sized by the launcher for the depth of the BVH
  __shared__ HosekSky s_sky;  // (light rays that escape see the sky: resolve_light_ray)
  if (LIGHTS) { stage_sky(fr, s_sky); __syncthreads(); }
  const uint32_t count = pool.counters[depth * kCounterStride + CNT_SEC];
  constexpr bool has_lights = LIGHTS;
  uint32_t nn = 0, nt = 0, nr = 0;
  WaveSteps ws;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
    const uint32_t p = pool.q_sec[i];
    f3 L = mk3(pool.rad[p]);
#pragma unroll
    for (uint32_t slot = SEC_DIR; slot <= SEC_LIGHT; ++slot) {
      if (slot == SEC_DIR && !fr.has_dir) continue;
      if (slot == SEC_AREA && !has_lights) continue;
      const size_t k = pool.sec_at(slot, p);
      const float4 d = pool.sec[k + 1];
      if (!sec_present(d)) continue;
      const float4 o = pool.sec[k];
      HitRec h;
      if (COUNT) nr++;
      if (slot == SEC_LIGHT && has_lights) {
        const bool hit = WIDE ? traverse_bvh8<false, COUNT, true, ALPHA>(sc.bvh8, mk3(o), mk3(d), o.w, h, nn, nt, &ws, lds_stack, (int)sc.bvh8.depth, &sc)
                              : traverse_bvh2<false, COUNT, ALPHA>(sc.bvh2, mk3(o), mk3(d), o.w, h, nn, nt, &sc);
        const float4 la = pool.lp_a[p], lb = pool.lp_b[p];
        L += resolve_light_ray<LT>(sc, fr, mk3(la), la.w, mk3(lb), lb.w, mk3(o), mk3(d), hit, h, pick_p);
      } else {
        const uint32_t nn0 = nn;
        const bool occluded = WIDE ? traverse_bvh8<true, COUNT, true, ALPHA>(sc.bvh8, mk3(o), mk3(d), o.w, h, nn, nt, &ws, lds_stack, (int)sc.bvh8.depth, &sc)
                                   : traverse_bvh2<true, COUNT, ALPHA>(sc.bvh2, mk3(o), mk3(d), o.w, h, nn, nt, &sc);
        if (COUNT) { const uint32_t kk = nn - nn0; int b = 0; while (b < 7 && kk > (8u << b)) ++b; atomicAdd(tc.hist + b, 1ull); }
        if (!occluded) L += mk3(pool.sec[k + 2]);
      }
    }
    pool.rad[p] = mk4(L, 0.0f);
  }
  if (COUNT) {
    atomicAdd(tc.nodes, (unsigned long long)nn);
    atomicAdd(tc.tris, (unsigned long long)nt);
    atomicAdd(tc.rays, (unsigned long long)nr);
    if (ws.node) atomicAdd(tc.wave_nodes, (unsigned long long)ws.node);
    if (ws.tri) atomicAdd(tc.wave_tris, (unsigned long long)ws.tri);
  }
}

// secondary rays over the 8-wide BVH with wave-cooperative triangle tests: a lane owns one shaded path and walks its
// secondary-ray slots in the reference's order; a slot is traversed by the whole wave when any lane has a ray in it
template <bool COUNT, bool LIGHTS, bool ALPHA, class... PickP>
__global__ void __launch_bounds__(kBlock, COUNT ? 1 : (LIGHTS ? 5 : 6)) k_trace_secondary_coop(SceneDev sc, FrameDev fr, PoolDev pool, uint32_t depth, TraceCounters tc, uint32_t flush, PickP... pp)
{
  constexpr bool LT = sizeof...(PickP) != 0;
  static_assert(LIGHTS || !LT, "pick probabilities without emitters");
  const float* const pick_p = pick_p_of(pp...);
  pass_priority();
  extern __shared__ __attribute__((aligned(16))) uint2 lds_stack[];  // [entry][thread], sized by the launcher for the depth of the BVH
  __shared__ __attribute__((aligned(16))) unsigned char lds[(kBlock / 64) * kCoopLdsBytesPerWave];
  const CoopLds cl = coop_lds(lds, threadIdx.x >> 6);
  __shared__ HosekSky s_sky;  // (light rays that escape see the sky: resolve_light_ray)
  if (LIGHTS) { stage_sky(fr, s_sky); __syncthreads(); }
  const uint32_t count = pool.counters[depth * kCounterStride + CNT_SEC];
  constexpr bool has_lights = LIGHTS;
  uint32_t nn = 0, nt = 0, nr = 0;
  WaveSteps ws;
  for (uint32_t base = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < count; base += gridDim.x * blockDim.x) {
    const uint32_t i = base + (threadIdx.x & 63u);
    const bool in_range = i < count;
    const uint32_t p = in_range ? pool.q_sec[i] : 0u;
    f3 L = in_range ? mk3(pool.rad[p]) : mk3(0.0f);
#pragma unroll
    for (uint32_t slot = SEC_DIR; slot <= SEC_LIGHT; ++slot) {
      if (slot == SEC_DIR && !fr.has_dir) continue;
      if (slot == SEC_AREA && !has_lights) continue;
      const size_t k = pool.sec_at(slot, p);
      const float4 d = in_range ? pool.sec[k + 1] : make_float4(0.0f, 0.0f, 1.0f, 0.0f);
      const bool valid = in_range && sec_present(d);
      if (__ballot(valid) == 0ull) continue;
      const float4 o = valid ? pool.sec[k] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      HitRec h;
      if (COUNT && valid) nr++;
      if (slot == SEC_LIGHT && has_lights) {
        const bool hit = traverse_bvh8_coop<false, COUNT, true, ALPHA>(sc.bvh8, valid, mk3(o), mk3(d), o.w, h, nn, nt, &ws, cl, flush, lds_stack, (int)sc.bvh8.depth, &sc);
        if (valid) {
          const float4 la = pool.lp_a[p], lb = pool.lp_b[p];
          L += resolve_light_ray<LT>(sc, fr, mk3(la), la.w, mk3(lb), lb.w, mk3(o), mk3(d), hit, h, pick_p);
        }
      } else {
        const uint32_t nn0 = nn;
        const bool occluded = traverse_bvh8_coop<true, COUNT, true, ALPHA>(sc.bvh8, valid, mk3(o), mk3(d), o.w, h, nn, nt, &ws, cl, flush, lds_stack, (int)sc.bvh8.depth, &sc);
        if (COUNT && valid) { const uint32_t kk = nn - nn0; int b = 0; while (b < 7 && kk > (8u << b)) ++b; atomicAdd(tc.hist + b, 1ull); }
        if (valid && !occluded) L += mk3(pool.sec[k + 2]);
      }
    }
    if (in_range) pool.rad[p] = mk4(L, 0.0f);
  }
  if (COUNT) {
    atomicAdd(tc.nodes, (unsigned long long)nn);
    atomicAdd(tc.tris, (unsigned long long)nt);
    atomicAdd(tc.rays, (unsigned long long)nr);
    if (ws.node) atomicAdd(tc.wave_nodes, (unsigned long long)ws.node);
    if (ws.tri) atomicAdd(tc.wave_tris, (unsigned long long)ws.tri);
  }
}

// secondary rays, streaming: a lane's item is one shaded path; its secondary-ray slots are traced one after the other by the
// same lane, so the additions into the path's radiance keep the reference's order (directional, sky, area, BSDF-sampled)
// (Items that are single RAYS instead of paths -- so that a small launch would end in its longest ray, not in its longest path -- were built and measured in round 6, bit-identical
// and SLOWER: the rays of a path share their first nodes, and the launches of one-pass calls are not bound by a lane's chain.  tools/patches/r6_ray_items.patch, profiles/README.md r6-8.)
// LT (fh_set_light_sampling): the light rays are finished by resolve_light_ray<true>, which reads pick_p
// DEFER (no emitters): the lane does not carry the path's radiance.  It notes which slots' rays escaped and leaves that mask, one byte, at the QUEUE POSITION of its
// item (esc[i]: dense, read back coalesced); k_sky_resolve adds what the escaped rays contribute, in the same slot order.  Neither pool.rad nor the contributions are touched here.
template <bool COUNT, bool LIGHTS, bool LT = false, bool DEFER = false>
struct SecondaryStream {
  static_assert(!DEFER || !LIGHTS, "light rays that find an emitter are finished in the commit");
  static constexpr bool all_any = !LIGHTS;  // without emitters every secondary ray stops at its first hit
  static constexpr bool can_climb = true;   // first-hit rays may start at the node of the face they leave (fh_trace.h: bottom-up start)
  const SceneDev& sc;
  const FrameDev& fr;
  const PoolDev& pool;
  ChunkFeed feed;
  uint32_t p = 0, slot = 0;
  uint32_t start = 0;  // wide node the lane's current ray starts its traversal at (0: the root)
  bool active = false;
  f3 L;
  uint32_t n_rays = 0;
  unsigned long long* hist;
  HistPack hp;
  const float* pick_p;
  uint32_t item = 0, escaped = 0;  // DEFER: queue position of the lane's item; bit s: the ray of slot s escaped
  uint8_t* esc;
  FH_D SecondaryStream(const SceneDev& s, const FrameDev& f, const PoolDev& pl, const ChunkFeed& cf, unsigned long long* hs, const float* pp = nullptr, uint8_t* es = nullptr)
      : sc(s), fr(f), pool(pl), feed(cf), L(mk3(0.0f)), hist(hs), pick_p(pp), esc(es) {}
  // first slot >= from of path p that holds a ray
  FH_D bool scan(uint32_t from, f3& o, f3& d, float& tmax, bool& any)
  {
    for (uint32_t s = from; s <= SEC_LIGHT; ++s) {
      if (s == SEC_DIR && !fr.has_dir) continue;
      if (s == SEC_AREA && !LIGHTS) continue;
      const size_t k = pool.sec_at(s, p);
      const float4 d4 = pool.sec[k + 1];
      if (!sec_present(d4)) continue;
      const float4 o4 = pool.sec[k];
      o = mk3(o4); d = mk3(d4); tmax = o4.w;
      start = start_node_of(d4);
      any = !(s == SEC_LIGHT && LIGHTS);
      slot = s;
      if (COUNT) n_rays++;
      return true;
    }
    return false;
  }
  FH_D void finish()
  {
    if (!active) return;
    if constexpr (DEFER) esc[item] = (uint8_t)escaped;
    else pool.rad[p] = mk4(L, 0.0f);
    active = false;
  }
  FH_D bool advance(f3& o, f3& d, float& tmax, bool& any)
  {
    if (!active) return false;
    if (scan(slot + 1u, o, d, tmax, any)) return true;
    finish();
    return false;
  }
  FH_D bool take(uint32_t i, f3& o, f3& d, float& tmax, bool& any)
  {
    if (i >= feed.end) return false;
    return take_item(i, o, d, tmax, any);
  }
  FH_D bool take_item(uint32_t i, f3& o, f3& d, float& tmax, bool& any)
  {
    p = pool.q_sec[i];
    if constexpr (DEFER) { item = i; escaped = 0u; }
    else L = mk3(pool.rad[p]);
    active = true;
    if (scan(0u, o, d, tmax, any)) return true;
    active = false;  // a path without secondary rays: its radiance stays as it is
    if constexpr (DEFER) esc[i] = 0u;  // (every entry of the queue reads back: nothing escaped)
    return false;
  }
  FH_D void commit(bool hit, const HitRec& h, uint32_t nodes)
  {
    const size_t k = pool.sec_at(slot, p);
    if (slot == SEC_LIGHT && LIGHTS) {
      const float4 o = pool.sec[k], d = pool.sec[k + 1];
      const float4 la = pool.lp_a[p], lb = pool.lp_b[p];
      L += resolve_light_ray<LT>(sc, fr, mk3(la), la.w, mk3(lb), lb.w, mk3(o), mk3(d), hit, h, pick_p);
    } else {
      if (COUNT) hp.add(nodes);
      if constexpr (DEFER) { if (!hit) escaped |= 1u << slot; }
      else if (!hit) L += mk3(pool.sec[k + 2]);
    }
  }
  FH_D bool drained() const { return feed.drained(); }
  FH_D bool followup() const { return active && slot < SEC_LIGHT; }
  FH_D uint32_t start_node() const { return start; }
};

template <bool COUNT, bool LIGHTS, bool ALPHA, class... PickP>
__global__ void __launch_bounds__(kBlock, COUNT ? 1 : (LIGHTS ? FH_SECONDARY_BLOCKS_HEAVY : (ALPHA ? FH_STREAM_BLOCKS_ALPHA : FH_STREAM_BLOCKS))) k_trace_secondary_stream(SceneDev sc, FrameDev fr, PoolDev pool, uint32_t depth, TraceCounters tc, uint32_t flush, uint32_t refill, uint32_t chunk, uint32_t min_rays, StackSpill spill, PickP... pp)
{
  constexpr bool LT = (std::is_same<PickP, const float*>::value || ...), DEFER = (std::is_same<PickP, uint8_t*>::value || ...);  // the pack: nothing, (pick_p) or (esc)
  static_assert(LIGHTS || !LT, "pick probabilities without emitters");
  static_assert(!LIGHTS || !DEFER, "escape masks with emitters");
  const float* const pick_p = pick_p_of(pp...);
  pass_priority();
  extern __shared__ __attribute__((aligned(16))) uint2 lds_stack[];  // [entry][thread], sized by the launcher for the depth of the BVH
  __shared__ __attribute__((aligned(16))) unsigned char lds[(kBlock / 64) * kCoopLdsBytesPerWave];
  const uint32_t count = pool.counters[depth * kCounterStride + CNT_SEC];
  if (stream_block_idle(count, min_rays)) return;
  __shared__ HosekSky s_sky;  // (light rays that escape see the sky: resolve_light_ray)
  if (LIGHTS) { stage_sky(fr, s_sky); __syncthreads(); }
  const ClockStamp stamp;
  CoopLds cl = coop_lds(lds, threadIdx.x >> 6);
  AlphaLds<AlphaDefer<true, ALPHA>::value>::attach(cl);  // candidates waiting for their any-hit test (fh_trace.h: alpha_ring): LDS of the kernels with the test compiled in only
  uint32_t nn = 0, nt = 0;
  WaveSteps ws;
  SecondaryStream<COUNT, LIGHTS, LT, DEFER> pol(sc, fr, pool, ChunkFeed(pool.counters + depth * kCounterStride + CNT_CUR_SEC, count, stream_chunk_for(count, chunk)), tc.hist, pick_p, esc_of(pp...));
  __shared__ uint4 lds_top[kTopNodes * 4];
  stage_top_nodes(sc.bvh8, lds_top);
  traverse_stream<true, COUNT, true, ALPHA>(sc.bvh8, pol, nn, nt, &ws, cl, flush, refill, lds_stack, (int)sc.bvh8.depth, &sc, spill, lds_top,
                                            spill.probe ? pool.counters + depth * kCounterStride + CNT_COST_NODE : nullptr);
  pol.finish();
  stamp.commit(tc.clk);
  if (COUNT) {
    atomicAdd(tc.nodes, (unsigned long long)nn);
    atomicAdd(tc.tris, (unsigned long long)nt);
    atomicAdd(tc.rays, (unsigned long long)pol.n_rays);
    pol.hp.flush(tc.hist);
    if (ws.node) atomicAdd(tc.wave_nodes, (unsigned long long)ws.node);
    if (ws.tri) atomicAdd(tc.wave_tris, (unsigned long long)ws.tri);
  }
}

// ------------------------------------------------------------------------------------------------
// The deferred mode's second half, one launch per bounce behind k_trace_secondary_stream<..., esc>: what the escaped shadow rays add to their paths.
// A workgroup takes kResolveItems consecutive entries of the secondary queue per round, four per thread:
//   (a) every thread reads the escape masks of its entries and counts their escaped sky and light rays; a block scan gives each of them a place in a dense list
//       (entry of the round, slot) that lives in LDS;
//   (b) the threads walk the list densely -- no lane idles beside an occluded ray, which is what an evaluation inside the traversal's commit would cost -- read the ray's
//       direction and weight, and leave w * env_radiance(d) in LDS at the ray's place in the list (a contribution stored as final, marker 0, is passed through);
//   (c) the owner of an entry with a non-zero mask adds to its path's radiance in slot order: the directional light's contribution from the record, sky and light from LDS.
// Same functions, same operand values and the same order of additions as SecondaryStream::commit / finish without DEFER: every bit stays.  No global atomics.
// dbg (FH_DEBUG_TAIL, else null): [0] += escaped sky and light rays, [1] += queue entries seen.
constexpr uint32_t kResolveItems = 4u * kBlock;
__global__ void __launch_bounds__(kBlock) k_sky_resolve(FrameDev fr, PoolDev pool, const uint8_t* esc, uint32_t depth, unsigned long long* dbg)
{
  const uint32_t count = pool.counters[depth * kCounterStride + CNT_SEC];
  if (blockIdx.x * kResolveItems >= count) return;
  __shared__ HosekSky s_sky;
  stage_sky(fr, s_sky);  // (published by the first barrier of the scan)
  __shared__ uint32_t s_p[kResolveItems];           // path slot of the round's entries that have an escaped ray
  __shared__ uint16_t s_list[2u * kResolveItems];   // entry of the round << 2 | slot
  __shared__ float s_c[3][2u * kResolveItems];      // contribution of list entry e
  __shared__ uint32_t s_wave[kBlock / 64];
  constexpr uint32_t kDeferred = (1u << SEC_SKY) | (1u << SEC_LIGHT);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t tile = blockIdx.x * kResolveItems; tile < count; tile += gridDim.x * kResolveItems) {
    uint32_t m[4], n = 0;
#pragma unroll
    for (uint32_t r = 0; r < 4u; ++r) {
      const uint32_t li = r * kBlock + threadIdx.x, i = tile + li;
      m[r] = i < count ? esc[i] : 0u;
      if (m[r]) s_p[li] = pool.q_sec[i];
      n += (uint32_t)__popc(m[r] & kDeferred);
    }
    uint32_t incl = n;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
      const uint32_t v = __shfl_up(incl, d);
      if (lane >= d) incl += v;
    }
    if (lane == 63u) s_wave[wave] = incl;
    __syncthreads();
    uint32_t base = incl - n, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < kBlock / 64u; ++w) {
      const uint32_t v = s_wave[w];
      if (w < wave) base += v;
      total += v;
    }
    {
      uint32_t pos = base;
#pragma unroll
      for (uint32_t r = 0; r < 4u; ++r) {
        const uint32_t li = r * kBlock + threadIdx.x;
        if (m[r] & (1u << SEC_SKY)) s_list[pos++] = (uint16_t)(li << 2 | SEC_SKY);
        if (m[r] & (1u << SEC_LIGHT)) s_list[pos++] = (uint16_t)(li << 2 | SEC_LIGHT);
      }
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < total; e += kBlock) {
      const uint32_t entry = s_list[e];
      const size_t k = pool.sec_at(entry & 3u, s_p[entry >> 2]);
      const float4 d4 = pool.sec[k + 1], c4 = pool.sec[k + 2];
      f3 c = mk3(c4);
      if (__float_as_uint(c4.w) == kSecWeight) c = c * env_radiance(fr, mk3(d4));
      s_c[0][e] = c.x; s_c[1][e] = c.y; s_c[2][e] = c.z;
    }
    __syncthreads();
    {
      uint32_t pos = base;
#pragma unroll
      for (uint32_t r = 0; r < 4u; ++r) {
        if (!m[r]) continue;
        const uint32_t p = s_p[r * kBlock + threadIdx.x];
        f3 L = mk3(pool.rad[p]);
        if (m[r] & (1u << SEC_DIR)) L += mk3(pool.sec[pool.sec_at(SEC_DIR, p) + 2]);
        if (m[r] & (1u << SEC_SKY)) { L += mk3(s_c[0][pos], s_c[1][pos], s_c[2][pos]); ++pos; }
        if (m[r] & (1u << SEC_LIGHT)) { L += mk3(s_c[0][pos], s_c[1][pos], s_c[2][pos]); ++pos; }
        pool.rad[p] = mk4(L, 0.0f);
      }
    }
    if (dbg && threadIdx.x == 0u) { atomicAdd(dbg, (unsigned long long)total); atomicAdd(dbg + 1, (unsigned long long)(count - tile < kResolveItems ? count - tile : kResolveItems)); }
    __syncthreads();  // (the next round reuses the lists)
  }
}

// One launch for the secondary rays of bounce b AND the closest-hit rays of bounce b + 1 (calls of ONE pass: the reference's 1- and 16-sample calls).  The two do not
// depend on each other -- the secondary rays read the secondary-ray records and add to the radiance, the closest-hit rays read the path's ray and write its hit -- and as two
// launches each of them ends in its own few long rays with most of the chip idle.  Here the wave's work queue is the secondary queue followed by the next bounce's radiance
// queue (one cursor over both): a lane holds either a path with its secondary rays or one closest-hit ray, every ray stops at its first hit or not as its kind says
// (traverse_stream's per-lane flag), and the launch has ONE end.  Same device functions, same per-path order of operations: the bits do not change.
template <bool LIGHTS, bool LT = false>
struct MergedStream {
  static constexpr bool all_any = false;
  static constexpr bool can_climb = false;
  SecondaryStream<false, LIGHTS, LT> sec;
  const PoolDev& next;        // the view whose radiance queue of bounce b + 1 is traced
  const uint32_t* q_closest;
  uint32_t n_sec;
  ChunkFeed feed;
  uint32_t pc = 0, qc = 0;    // path slot and entry (in the next bounce's radiance queue) of the lane's closest-hit ray
  uint32_t start_closest = 0;
  bool closest = false;       // the lane's current item is a closest-hit ray
  FH_D MergedStream(const SceneDev& s, const FrameDev& f, const PoolDev& ps, const PoolDev& pn, const uint32_t* qc, uint32_t ns, const ChunkFeed& cf, const float* pp = nullptr)
      : sec(s, f, ps, cf, nullptr, pp), next(pn), q_closest(qc), n_sec(ns), feed(cf) {}
  FH_D bool advance(f3& o, f3& d, float& tmax, bool& any) { return closest ? false : sec.advance(o, d, tmax, any); }
  FH_D bool take(uint32_t i, f3& o, f3& d, float& tmax, bool& any)
  {
    if (i >= feed.end) return false;
    if (i < n_sec) { closest = false; return sec.take_item(i, o, d, tmax, any); }
    closest = true;
    qc = i - n_sec;
    pc = q_closest[qc];
    const float4 o4 = next.ray_o[pc], d4 = next.ray_d[pc];
    o = mk3(o4); d = mk3(d4); tmax = o4.w; any = false;
    start_closest = start_node_of(d4);
    return true;
  }
  FH_D uint32_t start_node() const { return closest ? start_closest : sec.start; }
  FH_D void commit(bool hit, const HitRec& h, uint32_t nodes)
  {
    if (closest) { next.hit[pc] = make_float4(h.t, h.u, h.v, __uint_as_float(h.prim)); next.q_prim[qc] = h.prim; }
    else sec.commit(hit, h, nodes);
  }
  FH_D bool drained() const { return feed.drained(); }
  FH_D bool followup() const { return !closest && sec.followup(); }
};

template <bool LIGHTS, bool ALPHA, class... PickP>
__global__ void __launch_bounds__(kBlock, LIGHTS ? FH_SECONDARY_BLOCKS_HEAVY : (ALPHA ? FH_STREAM_BLOCKS_ALPHA : FH_STREAM_BLOCKS)) k_trace_merged_stream(SceneDev sc, FrameDev fr, PoolDev ps, PoolDev pn, uint32_t depth, TraceCounters tc, uint32_t flush, uint32_t refill, uint32_t chunk, uint32_t min_rays, StackSpill spill, PickP... pp)
{
  constexpr bool LT = sizeof...(PickP) != 0;
  static_assert(LIGHTS || !LT, "pick probabilities without emitters");
  const float* const pick_p = pick_p_of(pp...);
  pass_priority();
  extern __shared__ __attribute__((aligned(16))) uint2 lds_stack[];
  __shared__ __attribute__((aligned(16))) unsigned char lds[(kBlock / 64) * kCoopLdsBytesPerWave];
  const uint32_t n_sec = ps.counters[depth * kCounterStride + CNT_SEC], n_closest = ps.counters[(depth + 1u) * kCounterStride + CNT_RAD];
  const uint32_t count = n_sec + n_closest;
  if (stream_block_idle(count, min_rays)) return;
  __shared__ HosekSky s_sky;
  if (LIGHTS) { stage_sky(fr, s_sky); __syncthreads(); }
  const ClockStamp stamp;
  CoopLds cl = coop_lds(lds, threadIdx.x >> 6);
  AlphaLds<AlphaDefer<true, ALPHA>::value>::attach(cl);  // candidates waiting for their any-hit test (fh_trace.h: alpha_ring): LDS of the kernels with the test compiled in only
  uint32_t nn = 0, nt = 0;
  MergedStream<LIGHTS, LT> pol(sc, fr, ps, pn, pn.q_rad[(depth + 1u) & 1u], n_sec, ChunkFeed(ps.counters + depth * kCounterStride + CNT_CUR_SEC, count, stream_chunk_for(count, chunk)), pick_p);
  __shared__ uint4 lds_top[kTopNodes * 4];
  stage_top_nodes(sc.bvh8, lds_top);
  traverse_stream<true, false, true, ALPHA>(sc.bvh8, pol, nn, nt, nullptr, cl, flush, refill, lds_stack, (int)sc.bvh8.depth, &sc, spill, lds_top,
                                            spill.probe ? ps.counters + depth * kCounterStride + CNT_COST_NODE : nullptr);
  pol.sec.finish();
  stamp.commit(tc.clk);
}

// ------------------------------------------------------------------------------------------------
// Tail: after the first bounces only a few thousand of the millions of paths of a pass are still alive,
// and a bounce-synchronous wavefront then costs one worst-case ray latency per kernel and bounce.
// k_tail finishes those paths in one launch: each lane carries its path through all remaining bounces
// (trace -> shade -> secondary rays -> Russian roulette), so slow rays of different paths overlap
// instead of adding up.  Same device functions, same per-path operation order as the wavefront
// kernels, hence the same bits.
// One instantiation per lobe set, like k_shade: the generic seven-lobe form needs 430 registers (one wave per SIMD, so the 128 Ki paths a small pass hands over took two
// rounds), the forms for the lobe sets real scenes have fit two waves per SIMD.
//
// The rays of a bounce are traced PACKED.  A path in the tail has up to five rays per bounce -- its secondary rays and, once it is shaded, the closest-hit ray of the
// NEXT bounce, which depends on none of them -- and by its third bounce most lanes of a wave have no path left.  Traced one kind after the other, each kind costs the wave its
// longest ray (~1 us per dependent step with the SIMD to itself), three to five times per bounce; instead all rays of the wave are numbered (kind by kind, lane by lane:
// ballot + popcount), staged in LDS 64 at a time, traced by whichever lanes the numbering gives them to -- each ray stops at its first hit or not as its kind says -- and the
// results go back to their owners through LDS.  The additions into a path's radiance stay in the reference's order (they are applied from the returned results, slot by slot), so
// the bits do not change; the chain of a bounce is one traversal and one shade instead of three traversals and one shade once a wave is sparse.
constexpr uint32_t kTailRays = SEC_COUNT + 1u;  // the secondary-ray slots and the next bounce's closest-hit ray
static_assert(kTailRays == 5u, "trace_all spells its per-lane fallback out ray by ray");
__device__ __attribute__((noinline)) bool tail_trace_lane(const SceneDev& sc, uint2* lds_stack, bool any, f3 o, f3 d, float tmax, HitRec& h)
{
  uint32_t a = 0, b = 0;
  if (!sc.use_bvh8) return any ? traverse<true, false>(sc, o, d, tmax, h, a, b) : traverse<false, false>(sc, o, d, tmax, h, a, b);
  if (sc.has_alpha) return any ? traverse_bvh8<true, false, true, true>(sc.bvh8, o, d, tmax, h, a, b, nullptr, lds_stack, (int)sc.bvh8.depth, &sc)
                               : traverse_bvh8<false, false, true, true>(sc.bvh8, o, d, tmax, h, a, b, nullptr, lds_stack, (int)sc.bvh8.depth, &sc);
  return any ? traverse_bvh8<true, false, true, false>(sc.bvh8, o, d, tmax, h, a, b, nullptr, lds_stack, (int)sc.bvh8.depth, &sc)
             : traverse_bvh8<false, false, true, false>(sc.bvh8, o, d, tmax, h, a, b, nullptr, lds_stack, (int)sc.bvh8.depth, &sc);
}
struct TailRay { bool has = false; bool any = true; f3 o = mk3(0.0f), d = mk3(0.0f, 0.0f, 1.0f); float tmax = 0.0f; HitRec h = HitRec{0.0f, 0.0f, 0.0f, 0xffffffffu}; bool hit = false; };  // (no indeterminate field: r6-13)

// k_tail keeps three kernel NAMES over one body text, render_tail_body.inc, and is not a pack template as k_shade is: it calls tail_trace_lane out of line, so every tail
// kernel carries the LDS-kernel id the compiler numbers such kernels by, in the order of their mangled names (s_mov_b32 s15, <id> before each call).  As
// k_tail<LOBES, Tables...> the forms of one lobe set sort next to each other and the plain kernels get other ids: 15 of the 16 listings then differ.
template <uint32_t LOBES>
__global__ void __launch_bounds__(kBlock, LOBES == L_ALL ? 1 : 2) k_tail(SceneDev sc, FrameDev fr, PoolDev pool, uint32_t first_depth, uint32_t coop_flush)
{
  constexpr bool ENV = false, LT = false;
  const EnvTable* const env = nullptr;
  const LightTable* const ltab = nullptr;
#include "render_tail_body.inc"
}
template <uint32_t LOBES>
__global__ void __launch_bounds__(kBlock, LOBES == L_ALL ? 1 : 2) k_tail_env(SceneDev sc, FrameDev fr, PoolDev pool, uint32_t first_depth, uint32_t coop_flush, EnvTable env_table)
{
  constexpr bool ENV = true, LT = false;
  const EnvTable* const env = &env_table;
  const LightTable* const ltab = nullptr;
#include "render_tail_body.inc"
}
// (fh_set_light_sampling: the tail shades and resolves its light rays inline, so its twin reads the table at both sites)
template <uint32_t LOBES, bool ENV_ON>
__global__ void __launch_bounds__(kBlock, LOBES == L_ALL ? 1 : 2) k_tail_lt(SceneDev sc, FrameDev fr, PoolDev pool, uint32_t first_depth, uint32_t coop_flush, EnvTable env_table, LightTable light_table)
{
  constexpr bool ENV = ENV_ON, LT = true;
  const EnvTable* const env = &env_table;
  const LightTable* const ltab = &light_table;
#include "render_tail_body.inc"
}

// ------------------------------------------------------------------------------------------------
// FH_FLAG_REFERENCE_FIRSTHIT: the reference declares its payload outside the per-launch sample loop and never resets `firsthit`
// (pt.cu:432-433), so within ONE launch of n_samples > 1 only the first sample that hits anything records AOVs and sees emitters directly
// (:745-760), later primary misses add no sky (:509), and every sample averages the AOVs of that first hit again (:483-487).  The state is
// one bit per pixel, carried across the passes of a launch: after the depth-0 trace this kernel walks each pixel's samples in order and marks
// the paths that come after the first hitting one (flag 4).
__global__ void __launch_bounds__(kBlock) k_firsthit_scan(PoolDev pool, const uint32_t* owned, uint32_t n_owned, uint32_t n_batch, uint32_t* seen_state)
{
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_owned; i += gridDim.x * blockDim.x) {
    const uint32_t image_idx = owned[i];
    bool seen = seen_state[image_idx] != 0u;
    for (uint32_t k = 0; k < n_batch; ++k) {
      const uint32_t p = k * n_owned + i;
      const uint32_t fl = pool.flags[p];
      const bool in_queue = (fl & 2u) == 0u;  // otherwise the path ended in k_generate (missed the scene bounds): a primary miss
      if (seen) {
        pool.flags[p] = fl | 4u;
        if (!in_queue) pool.rad[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // its sky contribution is dropped (pt.cu:509)
      } else if (in_queue && __float_as_uint(pool.hit[p].w) != 0xffffffffu) {
        seen = true;  // this sample is the launch's first hit: it behaves normally
      }
    }
    seen_state[image_idx] = seen ? 1u : 0u;
  }
}

// ------------------------------------------------------------------------------------------------
// ADAPTIVE: the luminance moments too, through the pointer in place of `carry` (the bug-compat mode's; the two do not combine)
template <bool QUIRK, bool ADAPTIVE = false>
__global__ void __launch_bounds__(kBlock) k_accumulate(PoolDev pool, LayersDev layers, const uint32_t* owned, uint32_t n_owned, uint32_t n_batch,
                                                     std::conditional_t<ADAPTIVE, float2, float4>* carry)
{
  pass_priority();
  static_assert(!(QUIRK && ADAPTIVE), "FH_FLAG_REFERENCE_FIRSTHIT does not combine with adaptive sampling");
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_owned; i += gridDim.x * blockDim.x) {
    const uint32_t image_idx = owned[i];
    uint32_t n_spp = layers.sample_count[image_idx];
    f3 beauty = mk3(layers.beauty[image_idx]), position = mk3(layers.position[image_idx]), normal = mk3(layers.normal[image_idx]), albedo = mk3(layers.albedo[image_idx]);
    float depth = layers.depth[image_idx];
    const float4 tc4 = layers.texcoord[image_idx];
    float tcx = tc4.x, tcy = tc4.y;
    // bug-compat mode: the payload's AOVs persist from the launch's first hit (pt.cu:483-487); carried across the passes of the launch
    f3 apos = mk3(0.0f), anrm = mk3(0.0f), aalb = mk3(0.0f);
    float au = 0.0f, av = 0.0f, ad = 0.0f;
    if constexpr (QUIRK) {
      apos = mk3(carry[4 * (size_t)image_idx]); anrm = mk3(carry[4 * (size_t)image_idx + 1]); aalb = mk3(carry[4 * (size_t)image_idx + 2]);
      const float4 td = carry[4 * (size_t)image_idx + 3];
      au = td.x; av = td.y; ad = td.z;
    }
    float2 m = make_float2(0.0f, 0.0f);
    if constexpr (ADAPTIVE) m = carry[image_idx];
    for (uint32_t k = 0; k < n_batch; ++k) {
      const uint32_t p = k * n_owned + i;
      const f3 L = mk3(pool.rad[p]);
      const f3 radiance = bad3(L) ? mk3(0.0f) : L;
      if (!QUIRK) { apos = mk3(0.0f); anrm = mk3(0.0f); aalb = mk3(0.0f); au = av = ad = 0.0f; }
      if (pool.flags[p] & 1u) {
        apos = mk3(pool.aov_position[p]);
        anrm = mk3(pool.aov_normal[p]);
        aalb = mk3(pool.aov_albedo[p]);
        const float4 td = pool.aov_texdepth[p];
        au = td.x; av = td.y; ad = td.z;
      }
      const float coef = div_r_nofix<0, 0, 0, 32>(1.0f, n_spp + 1.0f);  // a count below 2^32, plus one
      const float fn = (float)n_spp;
      beauty = coef * (fn * beauty + radiance);
      position = coef * (fn * position + apos);
      normal = coef * (fn * normal + anrm);
      depth = coef * (fn * depth + ad);
      tcx = coef * (fn * tcx + au);
      tcy = coef * (fn * tcy + av);
      albedo = coef * (fn * albedo + aalb);
      if constexpr (ADAPTIVE) moments_update(m.x, m.y, coef, fn, radiance);
      n_spp++;
    }
    if constexpr (ADAPTIVE) carry[image_idx] = m;
    if constexpr (QUIRK) {
      carry[4 * (size_t)image_idx] = mk4(apos, 0.0f); carry[4 * (size_t)image_idx + 1] = mk4(anrm, 0.0f); carry[4 * (size_t)image_idx + 2] = mk4(aalb, 0.0f);
      carry[4 * (size_t)image_idx + 3] = make_float4(au, av, ad, 0.0f);
    }
    layers.sample_count[image_idx] = n_spp;
    layers.beauty[image_idx] = mk4(beauty, 1.0f);
    layers.position[image_idx] = mk4(position, 1.0f);
    layers.normal[image_idx] = mk4(normal, 1.0f);
    layers.depth[image_idx] = depth;
    layers.texcoord[image_idx] = make_float4(tcx, tcy, 0.0f, 1.0f);
    layers.albedo[image_idx] = mk4(albedo, 1.0f);
  }
}

// counting sort of one bounce queue by the cell keys stored next to it (kernels above); `bins` = histogram (zero on entry and exit) + cursors
void sort_queue_by_cell(hipStream_t st, uint32_t blocks, const uint32_t* count_ptr, const uint32_t* q_in, const uint16_t* keys, uint32_t* bins, uint32_t* q_out)
{
  hipLaunchKernelGGL(k_cell_hist, dim3(blocks), dim3(kSortBlock), 0, st, count_ptr, keys, bins);
  hipLaunchKernelGGL(k_cell_scan, dim3(1), dim3(kSortBlock), 0, st, bins, bins + kCells);
  hipLaunchKernelGGL(k_cell_scatter, dim3(blocks), dim3(kSortBlock), 0, st, count_ptr, q_in, keys, bins + kCells, q_out);
}

template <typename F>
void with_bool(bool b, F&& f)
{
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

uint32_t grid_for(uint32_t n)  // multiple of 8 (one share per XCD), at most 8192 blocks, grid-stride beyond
{
  uint32_t b = (n + kBlock - 1) / kBlock;
  b = (b + 7u) & ~7u;
  return b < 8 ? 8 : (b > 8192 ? 8192 : b);
}

// A kernel template that ends in a pack of tables is named as a value (its address for the runtime's queries) through the pointer type of the instantiation that is meant;
// a launch deduces the pack from its arguments.
template <class... Tables>
using ShadeFn = void (*)(SceneDev, FrameDev, PoolDev, uint32_t, uint32_t, Tables...);
template <class... PickP>
using SecondaryStaticFn = void (*)(SceneDev, FrameDev, PoolDev, uint32_t, TraceCounters, PickP...);
template <class... PickP>
using SecondaryCoopFn = void (*)(SceneDev, FrameDev, PoolDev, uint32_t, TraceCounters, uint32_t, PickP...);
template <class... PickP>
using SecondaryStreamFn = void (*)(SceneDev, FrameDev, PoolDev, uint32_t, TraceCounters, uint32_t, uint32_t, uint32_t, uint32_t, StackSpill, PickP...);
template <class... PickP>
using MergedStreamFn = void (*)(SceneDev, FrameDev, PoolDev, PoolDev, uint32_t, TraceCounters, uint32_t, uint32_t, uint32_t, uint32_t, StackSpill, PickP...);

// The trailing arguments of a call's k_shade launches (fh_set_env_sampling, fh_set_light_sampling): none, (env), (env that is not read, lt) or (env, lt)
template <typename F>
void with_tables(bool env_on, const EnvTable& env, const LightTable* lt, F&& f)
{
  if (lt && env_on) f(env, *lt);
  else if (lt) f(UnreadEnvTable{env}, *lt);
  else if (env_on) f(env);
  else f();
}

// The lobe ladder: of the variants a kernel is compiled in, most specific first, the first that contains every lobe of `lobes`; the last one is taken when none does
// (L_ALL).  f gets the variant's mask as a std::integral_constant.  (L_METAL | L_SPEC | L_DIFF: glTF metallic-roughness materials; with L_COAT: KHR_materials_clearcoat.)
template <uint32_t... V>
struct LobeSet {};
using ShadeLobes = LobeSet<L_DIFF, L_METAL, L_SPEC | L_DIFF, L_METAL | L_SPEC | L_DIFF, L_COAT | L_METAL | L_SPEC | L_DIFF, L_ALL>;  // k_shade
using TailLobes = LobeSet<L_DIFF, L_METAL | L_SPEC | L_DIFF, L_COAT | L_METAL | L_SPEC | L_DIFF, L_ALL>;                            // k_tail
template <typename F, uint32_t V, uint32_t... Rest>
void with_compiled_lobes(uint32_t lobes, LobeSet<V, Rest...>, F&& f)
{
  if constexpr (sizeof...(Rest) == 0) f(std::integral_constant<uint32_t, V>{});
  else if ((lobes & ~V) == 0) f(std::integral_constant<uint32_t, V>{});
  else with_compiled_lobes(lobes, LobeSet<Rest...>{}, f);
}

void dispatch_shade(hipStream_t st, uint32_t grid, uint32_t lobes, const SceneDev& sc, const FrameDev& fr, const PoolDev& pool, uint32_t cls, uint32_t depth, bool three, const EnvTable* env,
                    const EnvTable& env_table, const LightTable* lt, bool defer = false)
{
  with_tables(env != nullptr, env_table, lt, [&](auto... tables) {
    constexpr bool plain = sizeof...(tables) == 0;  // the forms that take tables are compiled for the tail's lobe sets, and at FH_SHADE_BLOCKS only
    with_compiled_lobes(lobes, std::conditional_t<plain, ShadeLobes, TailLobes>{}, [&](auto V) {
      constexpr uint32_t LOBES = decltype(V)::value;
      if constexpr (plain && LOBES != L_ALL) {
        // (the deferred forms exist in the three-workgroup set only; a class of the generic kernel stores final contributions, which k_sky_resolve passes through)
        if (three && defer) { hipLaunchKernelGGL((k_shade<LOBES, 3>), dim3(grid), dim3(kBlock), 0, st, sc, fr, pool, cls, depth, DeferSky{}); return; }
        if (three) { hipLaunchKernelGGL((k_shade<LOBES, 3>), dim3(grid), dim3(kBlock), 0, st, sc, fr, pool, cls, depth); return; }
      }
      hipLaunchKernelGGL(k_shade<LOBES>, dim3(grid), dim3(kBlock), 0, st, sc, fr, pool, cls, depth, tables...);
    });
  });
}

// The streaming trace kernels a scene is traced by, typed: the runtime queries (occupancy, fh_kernel_info) take the address, launch_closest launches what it is handed.
// (Of the secondary-ray kernel this is the form without pick_p, which is the one the queries have always asked about; launch_secondary names the template itself.)
template <typename F>
void with_closest_stream(bool count, bool alpha, F&& f)
{
  with_bool(count, [&](auto C) { with_bool(alpha, [&](auto A) { f(k_trace_closest_stream<decltype(C)::value, decltype(A)::value>); }); });
}
template <typename F>
void with_secondary_stream(bool count, bool lights, bool alpha, F&& f)
{
  with_bool(count, [&](auto C) { with_bool(lights, [&](auto Li) { with_bool(alpha, [&](auto A) {
    f(SecondaryStreamFn<>(k_trace_secondary_stream<decltype(C)::value, decltype(Li)::value, decltype(A)::value>));
  }); }); });
}
const void* stream_kernel(bool secondary, bool count, bool lights, bool alpha)
{
  const void* fn = nullptr;
  if (!secondary) with_closest_stream(count, alpha, [&](auto kernel) { fn = (const void*)kernel; });
  else with_secondary_stream(count, lights, alpha, [&](auto kernel) { fn = (const void*)kernel; });
  return fn;
}

// registers / LDS / scratch / resident workgroups per CU of the shade kernel a class of `lobes` is shaded by (fh_kernel_info, which >= 2): the same choice as dispatch_shade
template <uint32_t LOBES>
hipError_t shade_attributes_of(bool three, hipFuncAttributes& at, int& blocks)
{
  const ShadeFn<> fn = (three && LOBES != L_ALL) ? ShadeFn<>(k_shade<LOBES, (LOBES == L_ALL ? FH_SHADE_BLOCKS : 3)>) : ShadeFn<>(k_shade<LOBES>);
  const hipError_t e = hipFuncGetAttributes(&at, (const void*)fn);
  if (e != hipSuccess) return e;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, fn, kBlock, 0);
}
hipError_t shade_attributes(uint32_t lobes, bool three, hipFuncAttributes& at, int& blocks, uint32_t& compiled_lobes)
{
  hipError_t e = hipSuccess;
  with_compiled_lobes(lobes, ShadeLobes{}, [&](auto V) { compiled_lobes = decltype(V)::value; e = shade_attributes_of<decltype(V)::value>(three, at, blocks); });
  return e;
}

struct Span {
  fh_ctx* ctx; hipStream_t st; int kind; Event a, b; bool on;
  Span(fh_ctx* c, hipStream_t s, int k) : ctx(c), st(s), kind(k), on((c->flags & FH_FLAG_TIME_KERNELS) != 0)
  {
    if (on) { a = take_event(ctx); b = take_event(ctx); (void)hipEventRecord(a, st); }
  }
  ~Span()
  {
    if (on) { (void)hipEventRecord(b, st); ctx->spans.push_back({std::move(a), std::move(b), kind}); }
  }
};

}  // namespace

Event take_event(fh_ctx* ctx)
{
  Event e;
  if (!ctx->event_pool.empty()) { e = std::move(ctx->event_pool.back()); ctx->event_pool.pop_back(); }
  else (void)e.create();
  return e;
}

SceneDev scene_dev(const fh_ctx* ctx)
{
  SceneDev s{};
  s.face_rec = ctx->d_face_rec;
  s.face_cls = ctx->d_face_cls;
  s.materials = ctx->d_materials;
  s.lights = ctx->d_lights;
  s.n_faces = ctx->n_faces;
  s.n_lights = ctx->n_lights;
  s.n_materials = ctx->n_materials;
  s.textures = ctx->d_textures;
  s.srgb_lut = ctx->d_srgb_lut;
  s.n_textures = ctx->n_textures;
  s.alpha_rec = ctx->d_alpha_rec;
  s.has_alpha = (ctx->has_alpha || ctx->tun.force_alpha) ? 1u : 0u;
  s.bvh2.nodes = ctx->d_bvh2_nodes;
  s.bvh2.tris = ctx->d_bvh2_tris;
  s.bvh2.n_nodes = ctx->bvh2_n_nodes;
  s.bvh2.n_tris = ctx->bvh2_n_tris;
  s.bvh8.nodes = ctx->d_bvh8_nodes;
  s.bvh8.tris = ctx->d_bvh8_tris;
  s.bvh8.n_nodes = ctx->bvh8_n_nodes;
  s.bvh8.n_tris = ctx->bvh8_n_tris;
  s.bvh8.depth = stack_entries_for(ctx->bvh8_depth);
  s.use_bvh8 = ctx->use_bvh8 ? 1u : 0u;
  // bottom-up start (fh_trace.h): rays that leave a surface begin at the wide node that holds the face.  Only the streaming kernels climb; they trace trees of 4096 nodes and more
  // (what the scene CAN do; submit_pass switches it per pass, start_at_faces: forced by FH_BOTTOM_UP, else by what the first passes of the scene measure)
  const bool bottom_up = ctx->tun.bottom_up != 0 && ctx->use_bvh8 && ctx->d_bvh8_parent && ctx->d_face_node && ctx->tun.coop && ctx->tun.stream && (ctx->tun.stream_forced || ctx->bvh8_n_nodes >= 4096u) &&
                         ctx->bvh8_n_tris < kCoopMaxTris && !((ctx->has_alpha || ctx->tun.force_alpha));
  s.bvh8.parent = bottom_up ? ctx->d_bvh8_parent : nullptr;
  s.face_node = bottom_up ? ctx->d_face_node : nullptr;
  return s;
}

#if defined(FH_CHECK_DIV_RANGES)
int div_range_violations_read(fh_ctx* ctx, uint64_t* n)
{
  unsigned int v = 0;
  FH_HIP(hipMemcpyFromSymbol(&v, HIP_SYMBOL(fh::fh_div_range_violations), sizeof v));
  *n = v;
  return FH_OK;
}
#endif
// fh_kernel_info: registers / static LDS / scratch of the streaming kernel variant this scene is traced by, and how it is launched
int kernel_info(fh_ctx* ctx, int which, uint32_t out[6])
{
  for (int k = 0; k < 6; ++k) out[k] = 0u;
  if (which >= 2) {  // the shade kernel of shading class which - 2 of the scene: out[3] = resident workgroups per CU (x 4 waves / 4 SIMDs = waves per SIMD), out[4] = its lobe mask as compiled
    const uint32_t c = (uint32_t)(which - 2);
    if (c >= ctx->n_classes) return fail(ctx, FH_E_INVALID, "fh_kernel_info: the scene has no such shading class");
    hipFuncAttributes sa{};
    int blocks = 0;
    uint32_t compiled = 0;
    const bool three = ctx->tun.shade_wgs ? ctx->tun.shade_wgs == 3u : true;
    const hipError_t se = shade_attributes(ctx->class_lobes[c], three, sa, blocks, compiled);
    if (se != hipSuccess) return fail(ctx, FH_E_HIP, std::string("hipFuncGetAttributes: ") + hipGetErrorString(se));
    out[0] = (uint32_t)sa.numRegs; out[1] = (uint32_t)sa.sharedSizeBytes; out[2] = (uint32_t)sa.localSizeBytes; out[3] = (uint32_t)(blocks > 0 ? blocks : 0); out[4] = compiled; out[5] = ctx->class_lobes[c];
    return FH_OK;
  }
  const bool alpha = ctx->has_alpha || ctx->tun.force_alpha;
  hipFuncAttributes at{};
  const hipError_t e = hipFuncGetAttributes(&at, stream_kernel(which != 0, false, ctx->n_lights > 0, alpha));
  if (e != hipSuccess) return fail(ctx, FH_E_HIP, std::string("hipFuncGetAttributes: ") + hipGetErrorString(e));
  out[0] = (uint32_t)at.numRegs;
  out[1] = (uint32_t)at.sharedSizeBytes;
  out[2] = (uint32_t)at.localSizeBytes;
  out[3] = ctx->info_blocks[which];
  out[4] = ctx->info_entries[which];
  out[5] = stack_entries_for(ctx->bvh8_depth);
  return FH_OK;
}

void pool_release(fh_ctx* ctx)
{
  (void)drain_passes(ctx, true);  // nothing may still be running out of the buffers (the counter snapshots trail the accumulate)
  for (fh_ctx::PassSlot& s : ctx->slot) s.release();
}

int pool_ensure(fh_ctx* ctx, int slot, uint32_t capacity)
{
  // what a path record has to hold depends on the scene and the lights: a place per kind of secondary ray, the pending light-ray record (emitters
  // only), one queue per shading class.  A pool only grows: in paths, or when a later frame needs a kind of ray / a class it has no place for.
  fh_ctx::PoolShape need;
  need.dir = ctx->has_dir;
  need.lights = ctx->n_lights > 0;
  need.classes = ctx->n_classes < 1u ? 1u : ctx->n_classes;
  fh_ctx::PassSlot& S = ctx->slot[slot];
  const fh_ctx::PoolShape& have = S.shape;
  if (S.pool.capacity >= capacity && (have.dir || !need.dir) && (have.lights || !need.lights) && have.classes >= need.classes) return FH_OK;
  if (S.pool.capacity) {  // growing: nothing may still be running out of the old buffers
    FH_HIP(drain_passes(ctx, false));
    if (ctx->pool_target_by_caller && S.pool.capacity > capacity) capacity = S.pool.capacity;  // (a default-sized pool is re-made at the size the memory cap of this call allows)
    need.dir = need.dir || have.dir; need.lights = need.lights || have.lights; need.classes = need.classes > have.classes ? need.classes : have.classes;
    S.release();
  }
  PoolDev& P = S.pool;
  const hipStream_t st = pass_stream(ctx, slot);
  auto alloc = [&](auto*& ptr, size_t count) -> hipError_t {
    DeviceBuffer<uint8_t> buf;
    hipError_t e = buf.alloc(count * sizeof(*ptr));
    void* const raw = buf.get();
    if (e == hipSuccess) { S.allocs.push_back(std::move(buf)); S.alloc_bytes += count * sizeof(*ptr); ptr = (decltype(ptr))raw; }
    // FH_POISON=1 (tests): a new pool starts out full of 0xa5 instead of whatever the allocation held, so a kernel that reads a record or a queue entry nobody wrote shows at once
    if (e == hipSuccess && ctx->tun.poison_pools) e = hipMemsetAsync(raw, 0xa5, count * sizeof(*ptr), st);
    return e;
  };
  const size_t n = capacity;
  const uint32_t i_dir = 0u, i_sky = need.dir ? 1u : 0u, i_area = i_sky + 1u, i_light = i_sky + 1u + (need.lights ? 1u : 0u);
  const uint32_t sec_count = i_light + 1u;
  auto all = [&]() -> hipError_t {
    hipError_t e;
#define FH_POOL(ptr, count) if ((e = alloc(ptr, count)) != hipSuccess) return e
    float4 *state = nullptr, *aov = nullptr, *lp = nullptr;
    uint32_t* ident = nullptr;
    FH_POOL(state, n * 4); FH_POOL(P.rad, n); FH_POOL(ident, n * 2); FH_POOL(P.flags, n);
    FH_POOL(aov, n * 4); FH_POOL(P.sec, n * sec_count * 3);
    if (need.lights) FH_POOL(lp, n * 2);
    P.sec_count = sec_count;
    P.sec_index = i_dir | (i_sky << 8) | (i_area << 16) | (i_light << 24);
    P.ray_o.base = state; P.ray_d.base = state + 1; P.thr.base = state + 2; P.hit.base = state + 3;
    P.pixel.base = ident; P.nspp.base = ident + 1;
    P.aov_position.base = aov; P.aov_normal.base = aov + 1; P.aov_albedo.base = aov + 2; P.aov_texdepth.base = aov + 3;
    P.lp_a.base = lp; P.lp_b.base = lp ? lp + 1 : nullptr;
    FH_POOL(P.q_rad[0], n); FH_POOL(P.q_rad[1], n); FH_POOL(P.q_cls, n * need.classes); FH_POOL(P.q_sec, n); FH_POOL(P.q_prim, n);
    FH_POOL(P.counters, (size_t)kCounterStride * 66);  // up to 65 bounces per pass
    FH_POOL(P.key_sec, n); FH_POOL(P.key_rad, n); FH_POOL(P.q_tmp, n); FH_POOL(P.q_sec_sorted, n);
    FH_POOL(P.bins, (size_t)2 * kCells);
    FH_POOL(S.esc, n);  // (every entry a deferred secondary launch takes is written by it before k_sky_resolve reads it: no fill)
#undef FH_POOL
    // (on the stream this slot's passes run on, where the sorts that use the bins follow it: hipMemset on the null stream returns before the fill has run and is ordered
    // with NOTHING on a non-blocking stream -- a pass whose first sort overtook the fill counted into whatever the allocation held, turned that into scatter cursors and wrote
    // queue entries gigabytes away: the memory fault of profiles/README.md r4-10)
    return hipMemsetAsync(P.bins, 0, sizeof(uint32_t) * 2 * kCells, st);
  };
  const hipError_t e = all();
  if (e != hipSuccess) {  // leave the slot empty rather than half allocated: the next call starts from scratch
    S.release();
    return fail(ctx, FH_E_HIP, std::string("path pool allocation: ") + hipGetErrorString(e));
  }
  P.capacity = capacity;
  S.shape = need;
  return FH_OK;
}

// Dynamic LDS beyond the default limit has to be announced per kernel (hipFuncAttributeMaxDynamicSharedMemorySize).  Every kernel that keeps its stack in LDS
// is asked for its own static LDS (the fused tail carries 40 KB of tables next to the 14 KB of cooperative-test records the others have) and told the stack size when
// static + stack pass the default 64 KB; the largest static size is what fh_render checks against the CU's LDS.  Done once per BVH depth.
int configure_traversal_lds(fh_ctx* ctx, uint32_t stack_bytes)
{
  hipError_t err = hipSuccess;
  uint32_t max_static = kCoopLdsBytesPerBlock;
  auto set = [&](const void* fn) {
    hipFuncAttributes at{};
    if (hipFuncGetAttributes(&at, fn) == hipSuccess && (uint32_t)at.sharedSizeBytes > max_static) max_static = (uint32_t)at.sharedSizeBytes;
    if ((uint32_t)at.sharedSizeBytes + stack_bytes > 64u * 1024u) {
      const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)stack_bytes);
      if (e != hipSuccess) err = e;
    }
  };
  for (int c = 0; c < 2; ++c)
    for (int a = 0; a < 2; ++a)
      with_bool(c != 0, [&](auto C) { with_bool(a != 0, [&](auto A) {
        set((const void*)k_trace_closest_stream<decltype(C)::value, decltype(A)::value>);
        set((const void*)k_trace_closest_coop<decltype(C)::value, decltype(A)::value>);
        set((const void*)SecondaryStreamFn<uint8_t*>(k_trace_secondary_stream<decltype(C)::value, false, decltype(A)::value>));  // (the deferred mode's form: it leaves escape masks)
        for (int l = 0; l < 2; ++l)
          with_bool(l != 0, [&](auto Li) {
            set((const void*)SecondaryStreamFn<>(k_trace_secondary_stream<decltype(C)::value, decltype(Li)::value, decltype(A)::value>));
            set((const void*)MergedStreamFn<>(k_trace_merged_stream<decltype(Li)::value, decltype(A)::value>));
            set((const void*)SecondaryCoopFn<>(k_trace_secondary_coop<decltype(C)::value, decltype(Li)::value, decltype(A)::value>));
            set((const void*)SecondaryStaticFn<>(k_trace_secondary_static<decltype(C)::value, true, decltype(Li)::value, decltype(A)::value>));
            set((const void*)SecondaryStaticFn<>(k_trace_secondary_static<decltype(C)::value, false, decltype(Li)::value, decltype(A)::value>));
          });
      }); });
  set((const void*)k_tail<L_DIFF>);
  set((const void*)k_tail<L_METAL | L_SPEC | L_DIFF>);
  set((const void*)k_tail<L_COAT | L_METAL | L_SPEC | L_DIFF>);
  set((const void*)k_tail<L_ALL>);
  set((const void*)k_tail_env<L_DIFF>);
  set((const void*)k_tail_env<L_METAL | L_SPEC | L_DIFF>);
  set((const void*)k_tail_env<L_COAT | L_METAL | L_SPEC | L_DIFF>);
  set((const void*)k_tail_env<L_ALL>);
  for (int e = 0; e < 2; ++e)
    with_bool(e != 0, [&](auto E) {
      set((const void*)k_tail_lt<L_DIFF, decltype(E)::value>);
      set((const void*)k_tail_lt<L_METAL | L_SPEC | L_DIFF, decltype(E)::value>);
      set((const void*)k_tail_lt<L_COAT | L_METAL | L_SPEC | L_DIFF, decltype(E)::value>);
      set((const void*)k_tail_lt<L_ALL, decltype(E)::value>);
    });
  for (int a = 0; a < 2; ++a)  // fh_set_light_sampling: the forms that take pick_p, compiled with LIGHTS only
    with_bool(a != 0, [&](auto A) {
      set((const void*)MergedStreamFn<const float*>(k_trace_merged_stream<true, decltype(A)::value>));
      for (int c = 0; c < 2; ++c)
        with_bool(c != 0, [&](auto C) {
          set((const void*)SecondaryStreamFn<const float*>(k_trace_secondary_stream<decltype(C)::value, true, decltype(A)::value>));
          set((const void*)SecondaryCoopFn<const float*>(k_trace_secondary_coop<decltype(C)::value, true, decltype(A)::value>));
          set((const void*)SecondaryStaticFn<const float*>(k_trace_secondary_static<decltype(C)::value, true, true, decltype(A)::value>));
          set((const void*)SecondaryStaticFn<const float*>(k_trace_secondary_static<decltype(C)::value, false, true, decltype(A)::value>));
        });
    });
  if (err != hipSuccess) return fail(ctx, FH_E_HIP, std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize): ") + hipGetErrorString(err));
  ctx->lds_configured_bytes = stack_bytes;
  ctx->lds_static_max = max_static;
  return FH_OK;
}

// classify the owned pixels for this camera (k_split_pixels); cached until camera, resolution, ownership or scene bounds change
static int split_pixels(fh_ctx* ctx, const fh_camera* cam, const FrameDev& fr, bool dark)
{
  float key[32] = {};
  for (int i = 0; i < 12; ++i) key[i] = cam->transform[i];
  key[12] = cam->fov; key[13] = cam->F; key[14] = cam->focus;
  for (int i = 0; i < 3; ++i) { key[15 + i] = ctx->scene_lo[i]; key[18 + i] = ctx->scene_hi[i]; }
  key[21] = (float)ctx->width; key[22] = (float)ctx->height; key[23] = (float)ctx->n_owned; key[24] = (float)ctx->shard_rank; key[25] = (float)ctx->shard_world;
  key[26] = (float)ctx->tile_w; key[27] = (float)ctx->tile_h;
  key[28] = dark ? 1.0f : 0.0f;  // (the lists of a split made without the dark rule hold every sky pixel in the sky list: what an adaptive call needs)
  if (ctx->split_valid && std::memcmp(key, ctx->split_key, sizeof key) == 0) return FH_OK;
  ctx->split_valid = false;
  // the bound is derived for a rigid camera transform (rotation + translation): anything else renders every pixel through the passes
  const float* t = cam->transform;
  float dev = 0.0f;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      const float d = t[a] * t[b] + t[4 + a] * t[4 + b] + t[8 + a] * t[8 + b];  // columns of the 3x3 block
      dev = fmaxf(dev, fabsf(d - (a == b ? 1.0f : 0.0f)));
    }
  std::memcpy(ctx->split_key, key, sizeof key);
  ctx->n_wave_px = ctx->n_owned; ctx->n_sky_px = 0; ctx->n_dark_px = 0;
  if (!(dev < 1e-4f)) { ctx->split_valid = true; return FH_OK; }  // (valid: "no sky pixels" for this key)
  if (ctx->d_split[5].size() < ctx->n_owned) {  // (the last of the six: all were made)
    FH_HIP(hipDeviceSynchronize());
    for (int k = 0; k < 6; ++k) ctx->d_split[k].reset();
    for (int k = 0; k < 6; ++k) FH_HIP(ctx->d_split[k].alloc(ctx->n_owned));
  }
  // no launch of an earlier call may still read the lists that are rewritten here
  FH_HIP(drain_passes(ctx, true));
  SplitDev sp{};
  const float c[3] = {0.5f * (ctx->scene_lo[0] + ctx->scene_hi[0]), 0.5f * (ctx->scene_lo[1] + ctx->scene_hi[1]), 0.5f * (ctx->scene_lo[2] + ctx->scene_hi[2])};
  const float w[3] = {c[0] - t[3], c[1] - t[7], c[2] - t[11]};
  sp.centre = mk3(t[0] * w[0] + t[4] * w[1] + t[8] * w[2], t[1] * w[0] + t[5] * w[1] + t[9] * w[2], t[2] * w[0] + t[6] * w[1] + t[10] * w[2]);  // R^T (C - T)
  const float e[3] = {ctx->scene_hi[0] - ctx->scene_lo[0], ctx->scene_hi[1] - ctx->scene_lo[1], ctx->scene_hi[2] - ctx->scene_lo[2]};
  sp.radius = 0.5f * sqrtf(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
  {
    const float f = fr.cam_inv_tan, a0w[3] = {t[2] * f + t[3], t[6] * f + t[7], t[10] * f + t[11]};  // the lens centre (0, 0, f) in world space
    float far2 = 0.0f;
    for (int k = 0; k < 8; ++k) {
      float d2 = 0.0f;
      for (int a = 0; a < 3; ++a) { const float c = ((k >> a) & 1) ? ctx->scene_hi[a] : ctx->scene_lo[a]; d2 += (c - a0w[a]) * (c - a0w[a]); }
      far2 = fmaxf(far2, d2);
    }
    sp.far = sqrtf(far2) * 1.001f;
  }
  sp.wave_px = ctx->d_split[0]; sp.wave_xy = ctx->d_split[1]; sp.sky_px = ctx->d_split[2]; sp.sky_xy = ctx->d_split[3]; sp.dark_px = ctx->d_split[4]; sp.dark_xy = ctx->d_split[5];
  sp.dark_on = dark ? 1u : 0u;
  sp.counters = ctx->d_split_counters;
  FH_HIP(hipMemsetAsync(ctx->d_split_counters, 0, 8, ctx->stream));  // (the violation counter, word 2, keeps counting)
  FH_HIP(hipMemsetAsync(ctx->d_split_counters + 4, 0, 4, ctx->stream));
  hipLaunchKernelGGL(k_split_pixels, dim3(grid_for(ctx->n_owned)), dim3(kBlock), 0, ctx->stream, fr, sp, ctx->d_owned, ctx->d_owned_xy, ctx->n_owned);
  uint32_t n[5] = {0, 0, 0, 0, 0};  // (words 2 and 3, the violations and the cursor, are not looked at)
  FH_HIP(hipMemcpyAsync(n, ctx->d_split_counters, sizeof n, hipMemcpyDeviceToHost, ctx->stream));
  FH_HIP(hipStreamSynchronize(ctx->stream));
  if ((unsigned long long)n[0] + n[1] + n[4] != ctx->n_owned || (!dark && n[4])) return fail(ctx, FH_E_HIP, "k_split_pixels lost pixels");
  ctx->n_wave_px = n[0]; ctx->n_sky_px = n[1]; ctx->n_dark_px = n[4];
  ctx->split_valid = true;
  if (getenv("FH_DEBUG_BVH")) fprintf(stderr, "[split] %u of %u owned pixels cannot see the scene, %u of them dark (bounding sphere radius %.4f at camera-space (%.3f, %.3f, %.3f))\n", n[1] + n[4], ctx->n_owned, n[4], sp.radius, sp.centre.x, sp.centre.y, sp.centre.z);
  return FH_OK;
}

// the first boundary: the smallest multiple of step that is >= min_samples
static unsigned long long adaptive_b0(const fh_ctx* ctx)
{
  const unsigned long long step = ctx->adapt.step ? ctx->adapt.step : 1u;
  return (ctx->adapt.min_samples + step - 1ull) / step * step;
}

static AdaptiveDev adaptive_dev(const fh_ctx* ctx)
{
  const unsigned long long b0 = adaptive_b0(ctx);
  uint32_t shift = 0;
  while ((1u << shift) < ctx->adapt_block) ++shift;
  return AdaptiveDev{ctx->d_moments, ctx->d_sample_count, ctx->adapt.threshold, ctx->adapt.floor, ctx->adapt.min_samples, ctx->adapt.step,
                     ctx->adapt_growth, b0 <= 0xffffffffull ? (uint32_t)b0 : 0u,
                     ctx->adapt_block > 1u ? ctx->d_block_marks : nullptr, ctx->mark_seq, shift, (ctx->width + ctx->adapt_block - 1u) >> shift, ctx->width};
}

// samples from the count requested since fh_init_render_states to the next boundary of the policy (fh_adaptive_next_boundary; the rounds of growth 2)
uint32_t adaptive_to_boundary(const fh_ctx* ctx)
{
  const unsigned long long t = ctx->adapt_total, b0 = adaptive_b0(ctx);
  unsigned long long next = b0;
  if (t >= b0) {
    if (ctx->adapt_growth == 1u) next = t - t % ctx->adapt.step + ctx->adapt.step;
    else while (next <= t) next *= 2ull;
  }
  return next - t > 0xffffffffull ? 0xffffffffu : (uint32_t)(next - t);
}

// the device copy of the adaptive k_sky_pixels' state: made again whenever the parameters, the policy or the moments buffer change (capi.hip: adaptive_reset), when no
// launch reads it; with guard blocks also their marks (cleared, sequence 0: no block is marked)
int adaptive_upload(fh_ctx* ctx)
{
  FH_HIP(ctx->d_sky_adaptive.ensure(sizeof(SkyAdaptive)));
  FH_HIP(hipStreamSynchronize(ctx->stream));  // (earlier calls have joined the main stream)
  if (ctx->adapt_block > 1u) {
    const size_t b = ctx->adapt_block, words = (size_t)((ctx->width + b - 1u) / b) * ((ctx->height + b - 1u) / b);
    FH_HIP(ctx->d_block_marks.ensure(words));
    FH_HIP(hipMemsetAsync(ctx->d_block_marks, 0, 4ull * ctx->d_block_marks.size(), ctx->stream));  // (the selections run on this stream)
    ctx->mark_seq = 0;
  }
  const SkyAdaptive h{adaptive_dev(ctx), ctx->d_split_counters + 2, ctx->d_sky_taken};
  FH_HIP(hipMemcpy(ctx->d_sky_adaptive, &h, sizeof h, hipMemcpyHostToDevice));
  return FH_OK;
}

// the active pixels of a base list into ctx->d_active, ordered on `st`; waits for the count (the passes of a round are sized with it).  With guard blocks the blocks are
// marked first, from all owned pixels, and a sky list (the round's k_sky_pixels launch) is compacted next to the base list: d_active[2] / [3], one wait for both counts.
int adaptive_select(fh_ctx* ctx, hipStream_t st, const uint32_t* base_px, const uint32_t* base_xy, uint32_t n_base, uint32_t* n_active, const uint32_t* sky_px, const uint32_t* sky_xy,
                    uint32_t n_sky, uint32_t* n_sky_active)
{
  const bool blocks = ctx->adapt_block > 1u;
  // (d_active_blocks is made last: without it, an attempt failed half way)
  if (ctx->d_active[0].size() < ctx->n_owned || !ctx->d_active_blocks || !ctx->h_active_count || (blocks && !ctx->d_active[2])) {
    FH_HIP(hipDeviceSynchronize());  // (launches of earlier calls may still read the old lists)
    for (int k = 0; k < 4; ++k) ctx->d_active[k].reset();
    ctx->d_active_blocks.reset();
    FH_HIP(ctx->h_active_count.ensure(2));
    for (int k = 0; k < (blocks ? 4 : 2); ++k) FH_HIP(ctx->d_active[k].alloc(ctx->n_owned));
    FH_HIP(ctx->d_active_blocks.alloc(2ull * ((ctx->n_owned + kBlock - 1u) / kBlock + 1u)));
  }
  const size_t active_capacity = ctx->d_active[0].size();  // the owned pixels when the lists were made
  if (n_base > active_capacity || n_sky > active_capacity) return fail(ctx, FH_E_INVALID, "adaptive_select: base list longer than the owned pixels");
  if (n_sky && !(blocks && n_sky_active)) return fail(ctx, FH_E_INVALID, "adaptive_select: a sky list is compacted with guard blocks only");
  *n_active = 0;
  if (n_sky_active) *n_sky_active = 0;
  if (n_base == 0 && n_sky == 0) return FH_OK;
  if (blocks) {
    if (!ctx->d_block_marks) return fail(ctx, FH_E_INVALID, "adaptive_select: no block marks");
    if (++ctx->mark_seq == 0u) {  // (the sequence wrapped: words of 2^32 selections ago would read as marked)
      FH_HIP(hipMemsetAsync(ctx->d_block_marks, 0, 4ull * ctx->d_block_marks.size(), st));
      ctx->mark_seq = 1u;
    }
  }
  const AdaptiveDev ad = adaptive_dev(ctx);
  if (blocks) hipLaunchKernelGGL(k_adaptive_mark, dim3((ctx->n_owned + kBlock - 1u) / kBlock), dim3(kBlock), 0, st, ad, ctx->d_owned, ctx->d_owned_xy, ctx->n_owned);
  uint32_t* const scan_sky = ctx->d_active_blocks + ((active_capacity + kBlock - 1u) / kBlock + 1u);
  auto compact = [&](const uint32_t* px, const uint32_t* xy, uint32_t n, uint32_t* scan, uint32_t* out_px, uint32_t* out_xy, uint32_t* h_count) -> int {
    const uint32_t n_blocks = (n + kBlock - 1u) / kBlock;
    hipLaunchKernelGGL(k_adaptive_count, dim3(n_blocks), dim3(kBlock), 0, st, ad, px, n, scan);
    hipLaunchKernelGGL(k_adaptive_scan, dim3(1), dim3(kBlock), 0, st, scan, n_blocks);
    hipLaunchKernelGGL(k_adaptive_select, dim3(n_blocks), dim3(kBlock), 0, st, ad, px, xy, n, scan, out_px, out_xy);
    FH_HIP(hipMemcpyAsync(h_count, scan + n_blocks, 4, hipMemcpyDeviceToHost, st));
    return FH_OK;
  };
  if (n_base) { const int rc = compact(base_px, base_xy, n_base, ctx->d_active_blocks, ctx->d_active[0], ctx->d_active[1], ctx->h_active_count); if (rc) return rc; }
  if (n_sky) { const int rc = compact(sky_px, sky_xy, n_sky, scan_sky, ctx->d_active[2], ctx->d_active[3], ctx->h_active_count + 1); if (rc) return rc; }
  FH_HIP(hipStreamSynchronize(st));
  if (n_base) *n_active = ctx->h_active_count[0];
  if (n_sky) *n_sky_active = ctx->h_active_count[1];
  if (*n_active > n_base || (n_sky && *n_sky_active > n_sky)) return fail(ctx, FH_E_HIP, "adaptive_select: count beyond the base list");
  return FH_OK;
}

// ---- fh_render's submit path: render_submit (below) is a driver over the steps of this namespace; what they decide from plain values is in render_plan_host.h
namespace {

// The default pool size (32 Mi paths per pool) is a wish: whenever a pool has to be allocated -- the first frame, after fh_scene_upload changed what a path record
// holds, after a release -- all pools together are kept within A QUARTER of what the device has free at that moment, counting what the pools already hold as free.
// (A pool is allocated for the paths a pass really starts -- the pixels that can see the scene x the samples of the pass, pool_ensure -- so the cap is an upper bound.)
void cap_pool_target(fh_ctx* ctx)
{
  if (ctx->pool_target_by_caller) return;
  bool allocating = false;
  unsigned long long held = 0;
  for (int k = 0; k < (((ctx->flags & FH_FLAG_SERIAL_PASSES) != 0) ? 1 : ctx->n_slots); ++k) {
    const fh_ctx::PoolShape& have = ctx->slot[k].shape;
    if (ctx->slot[k].pool.capacity == 0 || (ctx->has_dir && !have.dir) || (ctx->n_lights > 0 && !have.lights) || have.classes < (ctx->n_classes < 1u ? 1u : ctx->n_classes)) allocating = true;
    held += (unsigned long long)ctx->slot[k].pool.capacity * pool_bytes_per_path(ctx);
  }
  if (!allocating) return;
  size_t free_b = 0, total_b = 0;
  ctx->pool_target = ctx->pool_target_default;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
    ctx->pool_target = pool_target_cap(free_b, held, ctx->pool_share, ctx->n_slots, pool_bytes_per_path(ctx), ctx->pool_target_default, ctx->n_owned);
  // (pools that exist already keep their size unless they have to be re-made: pool_ensure only grows)
}

// what the kernels of a call read about the frame: camera, environment, scene bounds, tables
FrameDev frame_dev(const fh_ctx* ctx, const fh_camera* cam, const float* bg, uint32_t seed, uint32_t max_depth)
{
  FrameDev fr{};
  fr.width = ctx->width; fr.height = ctx->height;
  fr.seed_hash = xxhash32(seed);
  fr.max_depth = max_depth;
  fr.has_dir = ctx->has_dir ? 1u : 0u;
  fr.has_hosek = ctx->has_hosek ? 1u : 0u;
  fr.has_ibl = ctx->d_ibl ? 1u : 0u;
  fr.ibl = fht_texture{nullptr, ctx->d_ibl, ctx->ibl_w, ctx->ibl_h, 0u};
  const uint32_t has_lights = ctx->n_lights > 0 ? 1u : 0u;
  fr.n1 = 3u + has_lights;
  fr.n2 = 3u + fr.has_dir + has_lights;
  for (int r = 0; r < 3; ++r) fr.cam_xf.r[r] = make_float4(cam->transform[4 * r], cam->transform[4 * r + 1], cam->transform[4 * r + 2], cam->transform[4 * r + 3]);
  fr.cam_inv_tan = 1.0f / tanf(0.5f * cam->fov);
  fr.cam_F = cam->F; fr.cam_focus = cam->focus;
  lens_values(fr.cam_inv_tan, cam->focus, cam->F, &fr.cam_a_plus_b, &fr.cam_lens_radius);
  fr.bg = mk3(bg[0], bg[1], bg[2]);
  fr.sky_intensity = ctx->sky_intensity;
  fr.sun_dir = mk3(ctx->sun_dir[0], ctx->sun_dir[1], ctx->sun_dir[2]);
  fr.hosek = ctx->d_hosek;
  fr.dir_le = mk3(ctx->dir_le[0], ctx->dir_le[1], ctx->dir_le[2]);
  fr.dir_dir = mk3(ctx->dir_dir[0], ctx->dir_dir[1], ctx->dir_dir[2]);
  fr.dir_disk_radius = 1e9f * tanf(0.5f * ctx->dir_angle * kPi / 180.0f);
  fr.scene_lo = mk3(ctx->scene_lo[0], ctx->scene_lo[1], ctx->scene_lo[2]);
  fr.scene_hi = mk3(ctx->scene_hi[0], ctx->scene_hi[1], ctx->scene_hi[2]);
  {
    const float cells = (float)(1u << kCellBits);
    const float ex = ctx->scene_hi[0] - ctx->scene_lo[0], ey = ctx->scene_hi[1] - ctx->scene_lo[1], ez = ctx->scene_hi[2] - ctx->scene_lo[2];
    fr.cell_scale = mk3(ex > 0.0f ? cells / ex : 0.0f, ey > 0.0f ? cells / ey : 0.0f, ez > 0.0f ? cells / ez : 0.0f);
  }
  fr.sobol = ctx->d_sobol;
  fr.sobol_bytes = ctx->d_sobol_bytes;
  fr.lut.reflection = ctx->d_lut_refl;
  fr.lut.sheen = ctx->d_lut_sheen;
  return fr;
}

LayersDev layers_dev(const fh_ctx* ctx, const fh_render_layers* layers)
{
  LayersDev L{};
  L.beauty = (float4*)layers->beauty; L.position = (float4*)layers->position; L.depth = layers->depth;
  L.normal = (float4*)layers->normal; L.texcoord = (float4*)layers->texcoord; L.albedo = (float4*)layers->albedo;
  L.sample_count = ctx->d_sample_count;
  return L;
}

// the pixels a call (in adaptive mode: a round) renders through the passes, as image indices and as x | y << 16; n_sky: the sky pixels beside them that k_sky_pixels
// renders, n_dark: the dark ones, which k_dark_pixels advances (ctx->d_split[2..5])
struct PixelLists { const uint32_t* px; const uint32_t* xy; uint32_t n_px, n_sky, n_dark; };

// ---- pixels that cannot see the scene are rendered by k_sky_pixels, the others by the passes (see k_split_pixels).  Worth its fixed cost -- one small launch and a
// host synchronisation whenever camera, resolution or scene bounds change -- for calls of many samples only: 2^27 camera paths, 64 spp of a 1080p frame
int choose_pixels(fh_ctx* ctx, const fh_camera* cam, const FrameDev& fr, uint32_t n_samples, bool quirk, PixelLists& out)
{
  out = PixelLists{ctx->d_owned, ctx->d_owned_xy, ctx->n_owned, 0u, 0u};
  const bool splits = ctx->tun.sky_split && !quirk && (unsigned long long)n_samples * ctx->n_owned >= (1ull << ctx->tun.sky_split_min_log2);
  if (!splits) return FH_OK;
  const bool dark = dark_sky_verdict(splits, fr.has_hosek != 0, fr.has_ibl != 0, ctx->adaptive, (ctx->flags & FH_FLAG_REFERENCE_FIRSTHIT) != 0, ctx->tun.dark_sky);
  const int rc = split_pixels(ctx, cam, fr, dark);
  if (rc) return rc;
  if (ctx->split_valid && ctx->n_sky_px + ctx->n_dark_px >= ctx->n_owned / 8u)  // (a handful of sky pixels is not worth a second kernel)
    out = PixelLists{ctx->d_split[0], ctx->d_split[1], ctx->n_wave_px, ctx->n_sky_px, ctx->n_dark_px};
  return FH_OK;
}

// FH_FLAG_REFERENCE_FIRSTHIT with more than one sample per launch: per-pixel state carried through the launch, passes run one after the other
int quirk_begin(fh_ctx* ctx)
{
  const size_t px = (size_t)ctx->width * ctx->height;
  if (ctx->d_quirk_aov.size() != px * 4) {  // (the second of the two: both were made)
    ctx->d_quirk_seen.reset(); ctx->d_quirk_aov.reset();
    FH_HIP(ctx->d_quirk_seen.alloc(px));
    FH_HIP(ctx->d_quirk_aov.alloc(px * 4));
  }
  FH_HIP(hipMemsetAsync(ctx->d_quirk_seen, 0, px * sizeof(uint32_t), ctx->stream));   // a launch starts with firsthit = true and a zeroed payload
  FH_HIP(hipMemsetAsync(ctx->d_quirk_aov, 0, px * 4 * sizeof(float4), ctx->stream));
  return FH_OK;
}

// A list of sky pixels is rendered by two launches of k_sky_pixels that pull groups of 64 pixels from one cursor.  The FILLER, a small fixed grid (FH_SKY_BLOCKS workgroups
// per CU) on the sky stream, starts with the passes and runs in the issue slots their kernels leave idle: one wave of 80 registers beside six traversal waves per SIMD, at
// wave priority 0 under the pass kernels' 1 (pass_priority).  The DRAIN, a grid that fills the machine, goes to the main stream behind the last pass of the call (or of the
// round) and finishes at full rate whatever the filler did not reach -- a call whose passes are short loses nothing to the filler's small grid.  Neither waits for the
// other: a group belongs to the wave that claimed it.  In line on the main stream (st == ctx->stream) one launch does it all.
struct SkyLaunches {
  fh_ctx* ctx;
  const FrameDev& fr;
  const LayersDev& L;
  bool adaptive;
  // (FH_FLAG_SERIAL_PASSES and FH_PIPELINE=0, the measuring modes: in line on the main stream, so that every kernel of the call is alone on the GPU, the spans add up and
  // a serial kernel trace shows the kernel's work instead of the time a starved background kernel was resident)
  hipStream_t st;
  uint32_t* cursor;
  uint32_t filler_wgs, full_wgs;
  struct Drain { const uint32_t* px; const uint32_t* xy; uint32_t n, n_samples; bool pending; } drain{nullptr, nullptr, 0u, 0u, false};

  SkyLaunches(fh_ctx* c, const FrameDev& f, const LayersDev& l, bool a)
      : ctx(c), fr(f), L(l), adaptive(a), st(((c->flags & FH_FLAG_SERIAL_PASSES) != 0 || c->n_slots == 1) ? c->stream : c->sky_stream), cursor(c->d_split_counters + 3),
        filler_wgs(st == c->stream ? 0u : (c->tun.sky_filler_grid ? c->tun.sky_filler_grid : c->tun.n_cus * c->tun.sky_blocks_per_cu)),
        full_wgs(c->tun.n_cus * (uint32_t)kSkyWaves)  // (every workgroup resident: the cursor balances them)
  {
  }
  void launch(hipStream_t s, uint32_t wgs, const uint32_t* px, const uint32_t* xy, uint32_t n, uint32_t ns)
  {
    Span sp(ctx, s, 4);
    const uint32_t full = (n + kBlock - 1u) / kBlock;  // (one group per wave)
    const uint32_t grid = wgs < full ? wgs : full;
    if (adaptive) hipLaunchKernelGGL(k_sky_pixels<true>, dim3(grid), dim3(kBlock), 0, s, fr, L, ctx->d_sample_issued, px, xy, n, ns, (const SkyAdaptive*)ctx->d_sky_adaptive.get(), cursor);
    else hipLaunchKernelGGL(k_sky_pixels<false>, dim3(grid), dim3(kBlock), 0, s, fr, L, ctx->d_sample_issued, px, xy, n, ns, ctx->d_split_counters + 2, cursor);
  }
  // (the caller has ordered the main stream behind every earlier launch that used the cursor)
  int begin(const uint32_t* px, const uint32_t* xy, uint32_t n, uint32_t ns)
  {
    FH_HIP(hipMemsetAsync(cursor, 0, 4, ctx->stream));
    if (st == ctx->stream) { launch(st, full_wgs, px, xy, n, ns); return FH_OK; }
    if (filler_wgs) {
      FH_HIP(hipEventRecord(ctx->ev_sky_cursor, ctx->stream));
      FH_HIP(hipStreamWaitEvent(st, ctx->ev_sky_cursor, 0));
      launch(st, filler_wgs, px, xy, n, ns);
    }
    drain = Drain{px, xy, n, ns, true};
    return FH_OK;
  }
  void end()  // on the main stream, which the caller has ordered behind the passes the launch is to follow
  {
    if (!drain.pending) return;
    launch(ctx->stream, full_wgs, drain.px, drain.xy, drain.n, drain.n_samples);
    drain.pending = false;
  }
};

// how the traversal kernels of a call are launched; of the streaming launches [0] is the closest-hit one, [1] the secondary-ray one (and the merged one)
struct StreamPlan {
  bool coop, stream, sort_queues, shade_three;
  uint32_t stack_bytes;                      // dynamic LDS of the fixed-batch kernels and of the fused tail: the whole stack
  uint32_t entries[2], lds_bytes[2];         // stack levels a streaming kernel keeps in LDS, and their bytes
  uint32_t grid[2];                          // workgroups of a streaming launch: all resident
  uint32_t spill_entries[2];                 // stack levels beyond the LDS part
  size_t spill_region;                       // uint2 per launch in flight of ctx->d_stack_spill
  uint32_t chunk[2];                         // packed chunk words (render_plan_host.h: stream_chunk_word)
};

// `filler`: a filler launch of k_sky_pixels runs beside the passes of this call
int stream_plan(fh_ctx* ctx, const SceneDev& sc, bool count, bool filler, StreamPlan& p)
{
  // device facts and developer switches were read once at fh_ctx_create (context.h: Tunables)
  const fh_ctx::Tunables& tun = ctx->tun;
  // wave-cooperative triangle tests (default for the wide BVH)
  p.coop = sc.use_bvh8 != 0 && sc.bvh8.n_tris < kCoopMaxTris && tun.coop;
  // streaming form (FH_STREAM=0: one fixed batch per wave).  Through a small tree every ray takes the same few steps: nothing to rebalance, and the fixed
  // batches run without the refill machinery (1000-triangle soup: closest 7.4 -> 4.6 ms, secondary 2.6 -> 1.0 ms per 256 spp; even at ~2 K nodes; behind at 20 K)
  p.stream = p.coop && tun.stream && (tun.stream_forced || ctx->bvh8_n_nodes >= 4096u);
  // the traversal stack of every lane lives in LDS, one entry per level of the BVH (bvh_build.hip records the depth); the streaming kernels may spill deep levels (below)
  const uint32_t stack_entries = stack_entries_for(ctx->bvh8_depth);
  p.stack_bytes = lds_stack_bytes(stack_entries);
  const uint32_t cfg_bytes = lds_stack_bytes(stack_entries + 1u);  // (+ 1: the anchor entry of rays that start below the root, fh_trace.h)
  if (sc.use_bvh8 && ctx->lds_configured_bytes != cfg_bytes) {  // kernels that may need more than the default 64 KB of LDS are told so once per BVH depth
    const int rc = configure_traversal_lds(ctx, cfg_bytes);
    if (rc) return rc;
  }
  if (sc.use_bvh8 && p.stack_bytes + ctx->lds_static_max > tun.lds_per_block) return fail(ctx, FH_E_UNSUPPORTED, "fh_render: BVH too deep for the LDS traversal stack");
  // all workgroups of a streaming launch are resident: as many per CU as its LDS (160 KB on gfx950) holds (at most 6: the kernels' register budget)
  // the streaming kernels' rays may start below the root: entry 0 of such a ray's stack is its anchor, the groups come on top (fh_trace.h: bottom-up start)
  const uint32_t stream_need = stack_entries + (sc.bvh8.parent ? 1u : 0u);
  // static LDS of a streaming kernel's workgroup: the cooperative-test records and, where candidates are parked for their any-hit test (AlphaDefer), the ring
  const uint32_t static_lds[2] = {kCoopLdsBytesPerBlock + (sc.has_alpha && AlphaDefer<false, true>::value ? kAlphaLdsBytesPerBlock : 0u),
                                  kCoopLdsBytesPerBlock + kTopLdsBytes + (sc.has_alpha && AlphaDefer<true, true>::value ? kAlphaLdsBytesPerBlock : 0u)};
  if (p.stream) {  // what the runtime says really fits (LDS granularity, registers of the variant in use): a grid above it would leave blocks queued behind the resident ones
    const uint32_t key = p.stack_bytes | (count ? 1u : 0u) | (sc.has_alpha ? 2u : 0u) | (sc.n_lights > 0 ? 4u : 0u) | (sc.bvh8.parent ? 8u : 0u) | (tun.stack_lds_entries << 20);
    if (ctx->occupancy_key != key) {
      auto occupancy = [&](bool secondary) {
        return [&, secondary](uint32_t entries) {
          int r = 0;
          (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&r, stream_kernel(secondary, count, sc.n_lights > 0, sc.has_alpha != 0), kBlock, lds_stack_bytes(entries));
          return r;
        };
      };
      // how many stack levels each of the two kernels keeps in LDS (render_plan_host.h: stream_lds_entries; FH_STREAM_BLOCKS_CLOSEST / FH_STREAM_BLOCKS: what they are compiled for)
      const StreamLds closest = stream_lds_entries(tun.lds_per_cu, FH_STREAM_BLOCKS_CLOSEST, static_lds[0], stream_need, tun.stack_lds_entries, occupancy(false));
      const StreamLds secondary = stream_lds_entries(tun.lds_per_cu, sc.n_lights > 0 ? FH_SECONDARY_BLOCKS_HEAVY : (sc.has_alpha ? FH_STREAM_BLOCKS_ALPHA : FH_STREAM_BLOCKS), static_lds[1],
                                                     stream_need, tun.stack_lds_entries, occupancy(true));
      ctx->stream_lds_entries = closest.entries; ctx->occupancy_blocks = closest.blocks;
      ctx->stream_lds_entries_secondary = secondary.entries; ctx->occupancy_blocks_secondary = secondary.blocks;
      ctx->occupancy_key = key;
      if (!count) {  // (what fh_kernel_info reports: the plan of the kernels that render, not of the instrumented variants a counting call has just been launched with)
        ctx->info_blocks[0] = ctx->occupancy_blocks; ctx->info_blocks[1] = ctx->occupancy_blocks_secondary;
        ctx->info_entries[0] = ctx->stream_lds_entries; ctx->info_entries[1] = ctx->stream_lds_entries_secondary;
      }
      if (getenv("FH_DEBUG_BVH"))
        fprintf(stderr, "[trace] stack of %u entries (%s); in LDS: closest %u (%u B + %u B per workgroup, %u resident workgroups per CU), secondary %u (%u B + %u B, %u workgroups)\n", stream_need, sc.bvh8.parent ? "rays start at the node of the face they leave" : "rays start at the root",
                ctx->stream_lds_entries, lds_stack_bytes(ctx->stream_lds_entries), static_lds[0], ctx->occupancy_blocks, ctx->stream_lds_entries_secondary,
                lds_stack_bytes(ctx->stream_lds_entries_secondary), static_lds[1], ctx->occupancy_blocks_secondary);
    }
  }
  // With a filler wave on every SIMD a seventh traversal workgroup per CU has no registers to go to: it would wait for one of the six to end and start as a straggler of a
  // persistent launch.  The passes of a call that started a filler are launched with six per CU (the compiled budget, FH_STREAM_BLOCKS, stays).
  const uint32_t wgs_cap = filler ? (uint32_t)FH_STREAM_BLOCKS_FILLER : 0xffffu;
  const uint32_t in_lds[2] = {ctx->stream_lds_entries, ctx->stream_lds_entries_secondary}, reported[2] = {ctx->occupancy_blocks, ctx->occupancy_blocks_secondary};
  const uint32_t compiled_for[2] = {FH_STREAM_BLOCKS_CLOSEST, FH_STREAM_BLOCKS > FH_SECONDARY_BLOCKS_HEAVY ? FH_STREAM_BLOCKS : FH_SECONDARY_BLOCKS_HEAVY};
  for (int k = 0; k < 2; ++k) {
    p.entries[k] = p.stream ? in_lds[k] : stream_need;
    p.lds_bytes[k] = lds_stack_bytes(p.entries[k]);
    p.grid[k] = tun.n_cus * stream_wgs(tun.lds_per_cu, p.lds_bytes[k], static_lds[k], compiled_for[k], p.stream ? reported[k] : 0u, wgs_cap);
    p.spill_entries[k] = p.entries[k] < stream_need ? stream_need - p.entries[k] : 0u;
  }
  // spill area of the streaming launches: [launch in flight: pass slot x (closest, secondary)][entry beyond the LDS part][thread of the launch]
  const size_t spill_threads = (size_t)(p.grid[0] > p.grid[1] ? p.grid[0] : p.grid[1]) * kBlock;
  p.spill_region = (size_t)(p.spill_entries[0] > p.spill_entries[1] ? p.spill_entries[0] : p.spill_entries[1]) * spill_threads;  // uint2 each
  if (p.spill_region * (2u * kPassSlots) > ctx->d_stack_spill.size()) {
    FH_HIP(hipDeviceSynchronize());  // (launches of earlier calls may still use the old area)
    FH_HIP(ctx->d_stack_spill.alloc(p.spill_region * (2u * kPassSlots)));
  }
  const uint32_t chunk_max = stream_chunk_max(tun.stream_chunk_fixed, tun.stream_chunk, ctx->bvh8_n_nodes);
  p.chunk[1] = stream_chunk_word(tun.stream_chunk, chunk_max);
  // (the closest-hit launch takes its own chunk size, FH_STREAM_CHUNK_CLOSEST)
  p.chunk[0] = stream_chunk_word(tun.stream_chunk_closest ? tun.stream_chunk_closest : tun.stream_chunk, chunk_max);
  // cell-ordered queues pay where rays of one cell share the nodes they fetch; a tree the fixed-batch kernels trace (under 4096 nodes) sits in the caches whatever
  // the order, and there the six sort launches per bounce are what a small frame waits for (Cornell box, 1 spp: 0.33 of 2.15 ms)
  p.sort_queues = tun.sort_queues && (p.stream || tun.sort_small);
  p.shade_three = tun.shade_wgs ? tun.shade_wgs == 3u : true;  // (above, FH_SHADE_BLOCKS)
  return FH_OK;
}

// The deferred mode of the sky and light slots where a pass is eligible and FH_SKY_DEFER says nothing (profiles/README.md, profiles/sky_defer_bench.json)
constexpr bool kSkyDeferByDefault = true;

// what every pass of one fh_render call shares
struct Call {
  fh_ctx* ctx;
  FrameDev fr;
  LayersDev L;
  SceneDev sc;  // what the scene CAN do (where rays start is a per-pass choice: Pass::sc)
  TraceCounters tc_closest, tc_shadow;
  uint32_t max_depth;
  bool adaptive, quirk, count;
  StreamPlan plan;
  EnvTable env;  // fh_set_env_sampling; env_on: the shade kernels and the fused tail of this call are the ENV variants
  bool env_on;
  LightTable lt;  // fh_set_light_sampling; lt_on (the switch is on AND the scene has emitters): the shade, tail and secondary-ray kernels of this call are the forms that take it
  bool lt_on;
};

// one pass: its pool slot and streams, and what was chosen for it
struct Pass {
  SceneDev sc;         // the call's scene with this pass's choice of where first-hit rays start
  int slot, probe;     // probe: while the scene's ray start is being probed, what this pass tries (0: the root, 1: the node of the face; -1: not a probing pass)
  hipStream_t st, sb;  // the pass's stream; the stream of its secondary launches (the same, but for the overlap form of a one-pass call)
  uint32_t grid, coop_flush, wave_depth;
  bool single_pass, merge, overlap;
  bool defer;          // the sky and light slots carry weights; k_sky_resolve follows every secondary launch (render_plan_host.h: sky_defer_verdict)
};

// the counter snapshots of earlier passes that have arrived: the share of a pass's paths alive at each depth (context.h: survival) and, while the scene's ray start is
// being probed, what the secondary launches cost (no host/device synchronisation: a snapshot is looked at when its event has passed)
void harvest_counters(fh_ctx* ctx)
{
  fh_ctx::TreeMeasurements& t = ctx->tree;
  for (int k = 0; k < kPassSlots; ++k) {
    fh_ctx::PassSlot::Snapshot& s = ctx->slot[k].snapshot;
    if (!(s.in_flight && hipEventQuery(s.ev) == hipSuccess)) continue;
    s.in_flight = false;
    const uint32_t* hc = s.h;
    t.survival_n = fold_survival(hc, kCounterStride, CNT_RAD, s.wave_depth, s.paths, t.survival, t.survival_n);  // the share of the pass's paths alive at each depth it ran as a wavefront (context.h: survival)
    if (s.bu >= 0 && t.bu_choice == 0) {  // (a pass of the scene's probing phase: what its secondary launches cost)
      fold_probe_cost(hc, kCounterStride, CNT_COST_NODE, CNT_COST_TRI, CNT_SEC, s.wave_depth, &t.bu_cost[s.bu], &t.bu_items[s.bu]);
      const int verdict = bottom_up_verdict(t.bu_cost, t.bu_items);
      if (verdict) {
        t.bu_choice = verdict;
        if (getenv("FH_DEBUG_BVH"))
          fprintf(stderr, "[trace] rays that leave a surface start at %s: %.0f against %.0f SIMD cycles of tests per shaded path (from the root / from the face)\n", t.bu_choice == 2 ? "the node of their face" : "the root",
                  t.bu_cost[0] / t.bu_items[0], t.bu_cost[1] / t.bu_items[1]);
      }
    }
    s.bu = -1;
    if (ctx->tun.debug_tail) { fprintf(stderr, "[tail] slot %d wd %u paths %u survivors:", k, s.wave_depth, s.paths); for (uint32_t d = 0; d <= s.wave_depth; ++d) fprintf(stderr, " %u", hc[d * kCounterStride + CNT_RAD]); fprintf(stderr, "\n"); }
  }
}

// ---- where a pass's first-hit rays start their traversal (fh_trace.h: bottom-up start): forced by FH_BOTTOM_UP=0 / 1; else the first passes after a build alternate and
// the device's own count of test rounds per shaded path decides (harvest_counters): a dense scene gains (1M-triangle soup: -12 %), an interior of long rays does not (-0.4 %)
bool start_at_faces(const Call& c, bool merge, int& probe)
{
  fh_ctx* const ctx = c.ctx;
  probe = -1;
  if (!(c.sc.bvh8.parent && c.plan.stream && (ctx->flags & FH_FLAG_ROOT_START) == 0u)) return false;
  if (ctx->tun.bottom_up == 1u) return true;
  if (ctx->tun.bottom_up != 2u) return false;
  // (only a pass whose secondary launch can climb is a probe: the merged launch of a one-pass call walks from the root whatever the pass says and counts no test
  // rounds, so counting it would fill one side of the comparison with cost 0 and fix the choice at "root" -- the reference's 1- and 16-sample calls come first in a GUI)
  if (ctx->tree.bu_choice == 0 && !c.count && !merge && !c.sc.has_alpha) {
    probe = (ctx->tree.bu_toggle++ & 1u) != 0u ? 1 : 0;
    return probe == 1;
  }
  return ctx->tree.bu_choice == 2;
}

StackSpill stack_spill(const Call& c, const Pass& p, int k, uint32_t probe_flag)
{
  return StackSpill{c.plan.spill_entries[k] ? c.ctx->d_stack_spill + (size_t)(2 * p.slot + k) * c.plan.spill_region : nullptr, c.plan.entries[k], probe_flag};
}

void launch_closest(const Call& c, const Pass& p, const PoolDev& pd, uint32_t depth)
{
  fh_ctx* const ctx = c.ctx;
  const StreamPlan& pl = c.plan;
  const SceneDev& sc = p.sc;
  Span sp(ctx, p.st, 0);
  if (pl.stream) {
    with_closest_stream(c.count, sc.has_alpha != 0, [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(p.grid < pl.grid[0] ? p.grid : pl.grid[0]), dim3(kBlock), pl.lds_bytes[0], p.st, sc, pd, depth, c.tc_closest, p.coop_flush, ctx->tun.stream_refill, pl.chunk[0],
                         ctx->tun.stream_min_rays, stack_spill(c, p, 0, 0u));
    });
  } else if (pl.coop) {
    with_bool(c.count, [&](auto C) { with_bool(sc.has_alpha != 0, [&](auto A) {
      hipLaunchKernelGGL((k_trace_closest_coop<decltype(C)::value, decltype(A)::value>), dim3(p.grid), dim3(kBlock), pl.stack_bytes, p.st, sc, pd, depth, c.tc_closest, p.coop_flush);
    }); });
  } else {
    with_bool(c.count, [&](auto C) { with_bool(sc.use_bvh8 != 0, [&](auto W) { with_bool(sc.has_alpha != 0, [&](auto A) {
      hipLaunchKernelGGL((k_trace_closest_static<decltype(C)::value, decltype(W)::value, decltype(A)::value>), dim3(p.grid), dim3(kBlock), 0, p.st, sc, pd, depth, c.tc_closest);
    }); }); });
  }
  ctx->stats.n_closest_launches++;
}

// The LIGHTS flag of a call's secondary-ray kernels and what its launches append for fh_set_light_sampling: (false), (true) or (true, pick_p) -- lt_on means emitters,
// and no kernel is compiled for (false, pick_p)
template <typename F>
void with_lights(const Call& c, const SceneDev& sc, F&& f)
{
  if (c.lt_on) f(std::true_type{}, c.lt.pick_p);
  else with_bool(sc.n_lights > 0, f);
}

void launch_secondary(const Call& c, const Pass& p, const PoolDev& ps, uint32_t depth)
{
  fh_ctx* const ctx = c.ctx;
  const StreamPlan& pl = c.plan;
  const SceneDev& sc = p.sc;
  if (p.defer) {  // (sky_defer_verdict: no emitters, the streaming kernel) -- the form that leaves escape masks, and right behind it, on the same stream, what they add
    uint8_t* const esc = ctx->slot[p.slot].esc;
    {
      Span sp(ctx, p.sb, 1);
      with_bool(c.count, [&](auto C) { with_bool(sc.has_alpha != 0, [&](auto A) {
        hipLaunchKernelGGL((k_trace_secondary_stream<decltype(C)::value, false, decltype(A)::value>), dim3(p.grid < pl.grid[1] ? p.grid : pl.grid[1]), dim3(kBlock), pl.lds_bytes[1], p.sb, sc, c.fr, ps,
                           depth, c.tc_shadow, p.coop_flush, ctx->tun.stream_refill, pl.chunk[1], ctx->tun.stream_min_rays, stack_spill(c, p, 1, p.probe >= 0 ? 1u : 0u), esc);
      }); });
    }
    Span sp(ctx, p.sb, 2);  // (the part of shading that moved)
    // (p.grid: a workgroup per 256 paths of the pass, at most 8192; grid-stride beyond, and the workgroups past the queue's end leave at once)
    hipLaunchKernelGGL(k_sky_resolve, dim3((p.grid + kResolveItems / kBlock - 1u) / (kResolveItems / kBlock)), dim3(kBlock), 0, p.sb, c.fr, ps, (const uint8_t*)esc, depth, ctx->tun.debug_tail ? ctx->d_resolve_dbg.get() : nullptr);
    ctx->stats.n_shadow_launches++;
    return;
  }
  Span sp(ctx, p.sb, 1);
  with_lights(c, sc, [&](auto Li, auto... pick_p) { with_bool(c.count, [&](auto C) { with_bool(sc.has_alpha != 0, [&](auto A) {
    if (pl.stream) {
      hipLaunchKernelGGL((k_trace_secondary_stream<decltype(C)::value, decltype(Li)::value, decltype(A)::value>), dim3(p.grid < pl.grid[1] ? p.grid : pl.grid[1]), dim3(kBlock), pl.lds_bytes[1], p.sb, sc, c.fr, ps,
                         depth, c.tc_shadow, p.coop_flush, ctx->tun.stream_refill, pl.chunk[1], ctx->tun.stream_min_rays, stack_spill(c, p, 1, p.probe >= 0 ? 1u : 0u), pick_p...);
    } else if (pl.coop) {
      hipLaunchKernelGGL((k_trace_secondary_coop<decltype(C)::value, decltype(Li)::value, decltype(A)::value>), dim3(p.grid), dim3(kBlock), pl.stack_bytes, p.sb, sc, c.fr, ps, depth, c.tc_shadow,
                         p.coop_flush, pick_p...);
    } else {
      with_bool(sc.use_bvh8 != 0, [&](auto W) {
        hipLaunchKernelGGL((k_trace_secondary_static<decltype(C)::value, decltype(W)::value, decltype(Li)::value, decltype(A)::value>), dim3(p.grid), dim3(kBlock), pl.stack_bytes, p.sb, sc, c.fr, ps,
                           depth, c.tc_shadow, pick_p...);
      });
    }
  }); }); });
  ctx->stats.n_shadow_launches++;
}

// one-pass calls where the streaming kernels trace the scene: the secondary rays of bounce `depth` and the closest-hit rays of bounce depth + 1 in ONE launch
void launch_merged(const Call& c, const Pass& p, const PoolDev& ps, const PoolDev& pd, uint32_t depth)
{
  fh_ctx* const ctx = c.ctx;
  const StreamPlan& pl = c.plan;
  const SceneDev& sc = p.sc;
  Span sp(ctx, p.st, 1);
  with_lights(c, sc, [&](auto Li, auto... pick_p) { with_bool(sc.has_alpha != 0, [&](auto A) {
    hipLaunchKernelGGL((k_trace_merged_stream<decltype(Li)::value, decltype(A)::value>), dim3(p.grid < pl.grid[1] ? p.grid : pl.grid[1]), dim3(kBlock), pl.lds_bytes[1], p.st, sc, c.fr, ps, pd, depth,
                       c.tc_shadow, p.coop_flush, ctx->tun.stream_refill, pl.chunk[1], ctx->tun.stream_min_rays, stack_spill(c, p, 1, p.probe >= 0 ? 1u : 0u), pick_p...);
  }); });
  ctx->stats.n_shadow_launches++;
  ctx->stats.n_closest_launches++;
}

// the fused tail finishes the survivors of the wavefront bounces: every class in one kernel, so it is compiled for every lobe a material of the scene can have
void launch_tail(const Call& c, const Pass& p, const PoolDev& pd, uint32_t n_paths)
{
  fh_ctx* const ctx = c.ctx;
  Span sp(ctx, p.st, 3);
  uint32_t lobes = 0;
  for (uint32_t cls = 0; cls < ctx->n_classes; ++cls) lobes |= ctx->class_lobes[cls];
  const dim3 tg(grid_for(n_paths / 16 + 1)), tb(kBlock);
  const uint32_t tl = p.sc.use_bvh8 ? c.plan.stack_bytes : 0u, tf = c.plan.coop ? p.coop_flush : 0u;
  if (c.lt_on) with_compiled_lobes(lobes, TailLobes{}, [&](auto V) { with_bool(c.env_on, [&](auto E) {
    hipLaunchKernelGGL((k_tail_lt<decltype(V)::value, decltype(E)::value>), tg, tb, tl, p.st, p.sc, c.fr, pd, p.wave_depth, tf, c.env, c.lt);
  }); });
  else if (c.env_on) with_compiled_lobes(lobes, TailLobes{}, [&](auto V) { hipLaunchKernelGGL(k_tail_env<decltype(V)::value>, tg, tb, tl, p.st, p.sc, c.fr, pd, p.wave_depth, tf, c.env); });
  else with_compiled_lobes(lobes, TailLobes{}, [&](auto V) { hipLaunchKernelGGL(k_tail<decltype(V)::value>, tg, tb, tl, p.st, p.sc, c.fr, pd, p.wave_depth, tf); });
  ctx->stats.n_tail_launches++;
}

// secondary rays of this bounce and the radiance rays of the next one, each into cell order.  ONE-PASS calls (r6-7): the order buys their launches nothing -- every
// line they touch is touched for the first time whatever the order -- and the six sort launches per bounce are pure chain: 4- and 16-sample calls of configs[3] are
// 3 % / 2 % faster without them; only the queue the fused tail takes over keeps its order (FH_SORT_ONEPASS=1: all, =0: none)
// pd, ps: the per-bounce views of the pool -- pd rotates the radiance queues through the sorted buffers, ps reads the sorted secondary queue
void sort_bounce_queues(const Call& c, const Pass& p, const PoolDev& pool, uint32_t depth, uint32_t sort_blocks, PoolDev& pd, PoolDev& ps, uint32_t*& q_spare)
{
  const fh_ctx::Tunables& tun = c.ctx->tun;
  Span sp(c.ctx, p.st, 6);
  const bool tail_next = depth + 1u == p.wave_depth && p.wave_depth < c.max_depth;
  const bool sort_sec = c.plan.sort_queues && (!p.single_pass || tun.sort_onepass == 1u);
  const bool sort_rad = c.plan.sort_queues && (!p.single_pass || tun.sort_onepass == 1u || (tun.sort_onepass == 2u && tail_next));
  ps = pd;
  if (sort_sec) {
    sort_queue_by_cell(p.st, sort_blocks, pool.counters + depth * kCounterStride + CNT_SEC, pool.q_sec, pool.key_sec, pool.bins, pool.q_sec_sorted);
    ps.q_sec = pool.q_sec_sorted;
  }
  if (sort_rad) {
    const uint32_t nxt = (depth + 1u) & 1u;
    sort_queue_by_cell(p.st, sort_blocks, pool.counters + (depth + 1u) * kCounterStride + CNT_RAD, pd.q_rad[nxt], pool.key_rad, pool.bins, q_spare);
    uint32_t* const unsorted = pd.q_rad[nxt];
    pd.q_rad[nxt] = q_spare;  // the next bounce reads the sorted queue ...
    q_spare = unsorted;       // ... and the buffer it came from is the next scratch target
  }
}

// One pass of nb samples over the pixels of `px`, of a call (round) of n_round samples in passes of `batch`.
// n_slots passes in flight (three by default, FH_PIPELINE): pass j lives in pool j % n_slots on the stream of that slot.  Only two things order consecutive passes: the sample
// indices (k_generate reads what k_bump_issued of the pass before wrote) and the running means (k_accumulate of pass j
// follows k_accumulate of pass j - 1, so the floating-point result is that of a serial run)
// (the bug-compat mode keeps every pass on the main stream: a pass needs the first-hit state the pass before it left)
// FH_FLAG_SERIAL_PASSES does the same for measurements: kernels then run alone on the GPU and their HIP-event spans are kernel times
int submit_pass(Call& c, const PixelLists& px, uint32_t nb, uint32_t batch, uint32_t n_round, uint32_t coop_flush, int& last_slot)
{
  fh_ctx* const ctx = c.ctx;
  const fh_ctx::Tunables& tun = ctx->tun;
  const uint32_t n_px = px.n_px, n_paths = n_px * nb, max_depth = c.max_depth;
  const bool serial = c.quirk || (ctx->flags & FH_FLAG_SERIAL_PASSES) != 0;
  const int n_slots = serial ? 1 : ctx->n_slots;
  Pass p{};
  p.grid = grid_for(n_paths);
  p.coop_flush = coop_flush;
  p.slot = serial ? 0 : (int)(ctx->pass_seq % (unsigned long long)n_slots);
  const int slot = p.slot, prev = serial ? ctx->last_slot_used : (slot + n_slots - 1) % n_slots;
  ctx->pass_seq++;
  ctx->stats.n_passes++;
  ctx->last_slot_used = slot;
  const hipStream_t st = p.st = pass_stream(ctx, slot);
  last_slot = slot;
  // A call that is ONE pass (the reference's callers: 1 or 16 samples per call) has no other pass to share the GPU with, and its bounces are chains of launches that
  // each end in a few long rays.  The secondary rays of bounce b and the closest-hit launch of bounce b + 1 do not depend on each other -- the secondary launch reads the
  // secondary-ray records and adds to the radiance, the closest-hit launch and the routing read rays and write hits -- so the secondary launch goes to a second stream;
  // the shade kernels of bounce b + 1, which overwrite the records it reads, wait for it.  (Calls of several passes overlap whole passes instead.)
  p.single_pass = !serial && batch >= n_round && n_round == nb;
  // ... or, where the streaming kernels trace the scene, both in ONE launch (k_trace_merged_stream): one end instead of two, no second stream (FH_MERGE=0: the two-stream form)
  p.merge = p.single_pass && c.plan.stream && !c.count && tun.merge_trace;
  p.overlap = p.single_pass && tun.overlap_secondary && !p.merge;
  p.defer = sky_defer_verdict(c.sc.n_lights > 0, c.fr.has_hosek != 0, c.fr.has_ibl != 0, c.env_on, c.lt_on, c.plan.stream, p.merge, c.plan.shade_three, tun.sky_defer, kSkyDeferByDefault);
  p.sb = st;
  if (p.overlap) {
    p.sb = (st == ctx->aux_stream[0]) ? ctx->aux_stream[1] : ctx->aux_stream[0];
    while (ctx->ev_bounce.size() < 2u * (max_depth + 1u)) {
      Event e;
      FH_HIP(e.create(hipEventDisableTiming));
      ctx->ev_bounce.push_back(std::move(e));
    }
  }
  // (The shade side of every bounce -- routing, shade kernels, queue sorts -- on a stream of its own, optionally of high priority, with the pass streams kept off some CUs,
  // was measured in round 4 and is slower: r4-6, tools/patches/r6_pruned_switches.patch.)
  { const int rc = pool_ensure(ctx, slot, n_px * batch); if (rc) return rc; }
  fh_ctx::PassSlot& S = ctx->slot[slot];
  const PoolDev& pool = S.pool;
  FH_HIP(hipMemsetAsync(pool.counters, 0, sizeof(uint32_t) * kCounterStride * (max_depth + 1), st));
  p.sc = c.sc;
  if (!start_at_faces(c, p.merge, p.probe)) { p.sc.bvh8.parent = nullptr; p.sc.face_node = nullptr; }
  if (prev != slot && ctx->slot[prev].gen_valid) FH_HIP(hipStreamWaitEvent(st, ctx->slot[prev].ev_gen, 0));
  {
    Span sp(ctx, st, 4);
    hipLaunchKernelGGL(k_generate, dim3(grid_for((n_px + kGenChunks - 1) / kGenChunks), nb), dim3(kBlock), 0, st, c.fr, pool, ctx->d_sample_issued, px.px, px.xy, n_px);
    hipLaunchKernelGGL(k_bump_issued, dim3((n_px + kBlock - 1) / kBlock), dim3(kBlock), 0, st, ctx->d_sample_issued, px.px, n_px, nb);
    ctx->stats.n_generate_launches++;
  }
  FH_HIP(hipEventRecord(S.ev_gen, st));
  S.gen_valid = true;
  ctx->stats.paths += n_paths;
  // bounces run as bounce-synchronous wavefront kernels; the survivors are finished by k_tail.  Adaptive mode picks the
  // first depth at which an earlier pass had at most tail_paths survivors (counts come from an asynchronous snapshot of
  // the device counters: no host/device synchronisation)
  // (a wavefront bounce costs two traversal launches, each as long as its longest ray whatever the number of rays, and a dozen small launches: 0.5 ms on the
  // 1 M-triangle scene against 0.14 ms for a bounce inside the fused tail, so in a small pass the tail takes over earlier -- 1-spp 1080p frames: configs[2] 3.02 -> 2.73 ms
  // at 128 Ki, configs[1] 1.90 -> 1.77 ms at 256 Ki; in a big pass the tail runs next to the streaming launches of the passes in flight, two waves per SIMD
  // against their six, and more paths in it cost 0-1 %)
  const uint32_t tail_paths = tun.tail_paths ? tun.tail_paths : (n_paths <= (1u << 22) ? 262144u : 65536u);
  harvest_counters(ctx);
  p.wave_depth = tail_wave_depth(ctx->tree.survival, ctx->tree.survival_n, n_paths, tail_paths, max_depth, ctx->tail_depth, tun.tail_depth, &ctx->auto_wave_depth);
  PoolDev pd = pool, ps = pool;  // per-bounce views: pd rotates the radiance queues through the sorted buffers, ps reads the sorted secondary queue
  uint32_t* q_spare = pool.q_tmp;
  const uint32_t sort_blocks = n_paths / 16384u < 1u ? 1u : (n_paths / 16384u > 512u ? 512u : n_paths / 16384u);
  for (uint32_t depth = 0; depth < p.wave_depth; ++depth) {
    if (!(p.merge && depth > 0)) launch_closest(c, p, pd, depth);  // (merged launches: the closest-hit rays of this bounce were traced next to the secondary rays of the bounce before)
    if (c.quirk && depth == 0) hipLaunchKernelGGL(k_firsthit_scan, dim3(grid_for(n_px)), dim3(kBlock), 0, st, pd, px.px, n_px, nb, ctx->d_quirk_seen);
    {
      Span sp(ctx, st, 6);
      hipLaunchKernelGGL(k_route, dim3(p.grid), dim3(kBlock), 0, st, p.sc, pd, depth, ctx->n_classes, c.count ? ctx->d_trace_counters + 26 : nullptr);
    }
    if (p.overlap && depth > 0) FH_HIP(hipStreamWaitEvent(st, ctx->ev_bounce[2u * (depth - 1u) + 1u], 0));  // the secondary launch of the bounce before reads what the shade kernels and the sorts below overwrite
    {
      Span sp(ctx, st, 2);
      for (uint32_t cls = 0; cls < ctx->n_classes; ++cls) dispatch_shade(st, p.grid, ctx->class_lobes[cls], p.sc, c.fr, pd, cls, depth, c.plan.shade_three, c.env_on ? &c.env : nullptr, c.env, c.lt_on ? &c.lt : nullptr, p.defer);
      if (depth == 0) hipLaunchKernelGGL(k_miss_primary, dim3(p.grid), dim3(kBlock), 0, st, c.fr, pd);
      ctx->stats.n_shade_launches += ctx->n_classes;
    }
    sort_bounce_queues(c, p, pool, depth, sort_blocks, pd, ps, q_spare);
    if (p.merge && depth + 1u < p.wave_depth) launch_merged(c, p, ps, pd, depth);
    else {
      if (p.overlap) { FH_HIP(hipEventRecord(ctx->ev_bounce[2u * depth], st)); FH_HIP(hipStreamWaitEvent(p.sb, ctx->ev_bounce[2u * depth], 0)); }
      launch_secondary(c, p, ps, depth);
    }
    if (p.overlap) FH_HIP(hipEventRecord(ctx->ev_bounce[2u * depth + 1u], p.sb));
  }
  if (p.overlap && p.wave_depth > 0) FH_HIP(hipStreamWaitEvent(st, ctx->ev_bounce[2u * (p.wave_depth - 1u) + 1u], 0));  // the tail and the accumulate read the radiance the last secondary launch completes
  if (p.wave_depth < max_depth) launch_tail(c, p, pd, n_paths);
  if (prev != slot && ctx->slot[prev].acc_valid) FH_HIP(hipStreamWaitEvent(st, ctx->slot[prev].ev_acc, 0));
  {
    Span sp(ctx, st, 5);
    if (c.quirk) hipLaunchKernelGGL((k_accumulate<true>), dim3(grid_for(n_px)), dim3(kBlock), 0, st, pool, c.L, px.px, n_px, nb, ctx->d_quirk_aov);
    else if (c.adaptive) hipLaunchKernelGGL((k_accumulate<false, true>), dim3(grid_for(n_px)), dim3(kBlock), 0, st, pool, c.L, px.px, n_px, nb, ctx->d_moments);
    else hipLaunchKernelGGL((k_accumulate<false>), dim3(grid_for(n_px)), dim3(kBlock), 0, st, pool, c.L, px.px, n_px, nb, (float4*)nullptr);
    ctx->stats.n_accumulate_launches++;
  }
  FH_HIP(hipEventRecord(S.ev_acc, st));
  S.acc_valid = true;
  fh_ctx::PassSlot::Snapshot& snap = S.snapshot;
  if (!snap.in_flight && snap.h) {
    FH_HIP(hipMemcpyAsync(snap.h, pool.counters, sizeof(uint32_t) * kCounterStride * (max_depth + 1), hipMemcpyDeviceToHost, st));
    FH_HIP(hipEventRecord(snap.ev, st));
    snap.in_flight = true;
    snap.wave_depth = p.wave_depth;
    snap.paths = n_paths;
    snap.bu = p.probe;
  }
  return FH_OK;
}

// Adaptive mode, the start of a round of n_round samples: the pixels still active are selected from the call's base list.  The selection waits for the round before it
// (wait_slot: the slot of its last pass, 0: the main stream itself or none), and its count, read back, sizes the passes of the round.
int select_round(const Call& c, SkyLaunches& sky, const PixelLists& base, bool guard_blocks, int wait_slot, uint32_t n_round, PixelLists& act, bool& sky_ran)
{
  fh_ctx* const ctx = c.ctx;
  if (wait_slot != 0) FH_HIP(hipStreamWaitEvent(ctx->stream, ctx->slot[wait_slot].ev_acc, 0));
  if (guard_blocks) sky.end();  // (the round's own sky launch: the next selection reads what it writes)
  if (sky_ran && sky.st != ctx->stream) { FH_HIP(hipEventRecord(ctx->ev_sky, sky.st)); FH_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_sky, 0)); }
  act.n_sky = 0;
  const int rc = guard_blocks && base.n_sky ? adaptive_select(ctx, ctx->stream, base.px, base.xy, base.n_px, &act.n_px, ctx->d_split[2], ctx->d_split[3], base.n_sky, &act.n_sky)
                                            : adaptive_select(ctx, ctx->stream, base.px, base.xy, base.n_px, &act.n_px);
  if (rc) return rc;
  act.px = ctx->d_active[0]; act.xy = ctx->d_active[1];
  if (act.n_sky) {  // (the selection has been waited for, and with it the drain of the round before)
    const int rc2 = sky.begin(ctx->d_active[2], ctx->d_active[3], act.n_sky, n_round);
    if (rc2) return rc2;
    ctx->sky_taken_pending = true;
    sky_ran = true;
  }
  return FH_OK;
}

}  // namespace

int render_submit(fh_ctx* ctx, const fh_camera* cam, const float* bg, const fh_render_layers* layers, uint32_t n_samples, uint32_t max_depth, uint32_t seed)
{
  if (!ctx->scene_loaded || !ctx->bvh_valid) return fail(ctx, FH_E_INVALID, "fh_render: scene not uploaded or BVH not built");
  if (ctx->width == 0 || ctx->height == 0 || !ctx->d_sample_count) return fail(ctx, FH_E_INVALID, "fh_render: resolution not set");
  if (max_depth > 64) return fail(ctx, FH_E_INVALID, "fh_render: max_depth > 64 is not supported");
  if (ctx->n_owned == 0 || n_samples == 0) return FH_OK;
  const bool adaptive = ctx->adaptive;
  const bool guard_blocks = adaptive && ctx->adapt_block > 1u;  // (the sky pixels then follow their blocks: one k_sky_pixels launch per round, on the round's selection)
  const bool quirk = (ctx->flags & FH_FLAG_REFERENCE_FIRSTHIT) != 0 && n_samples > 1;
  if (adaptive && quirk)
    return fail(ctx, FH_E_INVALID, "fh_render: FH_FLAG_REFERENCE_FIRSTHIT with n_samples > 1 does not combine with adaptive sampling (its first-hit state is per launch)");
  ctx->accumulated = true;
  cap_pool_target(ctx);

  const bool count = (ctx->flags & FH_FLAG_COUNT_TRAVERSAL) != 0;
  unsigned long long* const tc = ctx->d_trace_counters;
  const bool clocks = (ctx->flags & FH_FLAG_TIME_KERNELS) != 0;
  Call c{ctx, frame_dev(ctx, cam, bg, seed, max_depth), layers_dev(ctx, layers), SceneDev{},
         TraceCounters{tc, tc + 1, tc + 2, tc + 6, tc + 7, tc + 10, clocks ? tc + 27 : nullptr}, TraceCounters{tc + 3, tc + 4, tc + 5, tc + 8, tc + 9, tc + 18, clocks ? tc + 29 : nullptr},
         max_depth, adaptive, quirk, count, StreamPlan{}, env_table_dev(ctx), ctx->env_sampling != 0, light_table_dev(ctx), ctx->light_sampling != 0 && ctx->n_lights > 0};
  if (c.lt_on) { const int rc = light_table_ensure(ctx); if (rc) return rc; c.lt = light_table_dev(ctx); }  // (as the environment's, below: rebuilt on the main stream ahead of everything this call queues; the rebuild may allocate)
  if (c.env_on) { const int rc = env_table_ensure(ctx); if (rc) return rc; }  // (a stale table is rebuilt on the main stream, ahead of everything this call queues)
  PixelLists base;  // the pixels of the call
  { const int rc = choose_pixels(ctx, cam, c.fr, n_samples, quirk, base); if (rc) return rc; }
  const uint32_t target = ctx->pool_target > ctx->n_owned ? ctx->pool_target : ctx->n_owned;
  c.sc = scene_dev(ctx);
  if (quirk) { const int rc = quirk_begin(ctx); if (rc) return rc; }
  if (!ctx->render_pending) { (void)hipEventRecord(ctx->ev_render_begin, ctx->stream); ctx->render_pending = true; }
  // whatever the caller queued on the main stream before this call (clears, uploads) comes first on the second stream too
  FH_HIP(hipEventRecord(ctx->ev_enter, ctx->stream));
  for (int k = 0; k + 1 < ctx->n_slots; ++k) FH_HIP(hipStreamWaitEvent(ctx->aux_stream[k], ctx->ev_enter, 0));
  SkyLaunches sky(ctx, c.fr, c.L, adaptive);
  if (base.n_sky && sky.st != ctx->stream) FH_HIP(hipStreamWaitEvent(sky.st, ctx->ev_enter, 0));
  if (base.n_sky && !guard_blocks) {  // the sky pixels of this call, all samples at once (they share no pixel with the passes)
    const int rc = sky.begin(ctx->d_split[2], ctx->d_split[3], base.n_sky, n_samples);
    if (rc) return rc;
    if (adaptive) ctx->sky_taken_pending = true;  // (the samples it takes are counted on the device: fh_sync adds them to the stats)
    else {
      ctx->stats.paths += (uint64_t)base.n_sky * n_samples;
      ctx->stats.sky_pixel_samples += (uint64_t)base.n_sky * n_samples;
    }
  }
  if (base.n_dark) {  // the dark sky pixels (never in an adaptive call: dark_sky_verdict), on the main stream ahead of the passes: they share no pixel with anything else of this call
    Span sp(ctx, ctx->stream, 4);
    hipLaunchKernelGGL(k_dark_pixels, dim3(grid_for(base.n_dark)), dim3(kBlock), 0, ctx->stream, c.L, ctx->d_sample_issued, (const uint32_t*)ctx->d_split[4].get(), base.n_dark, n_samples);
    ctx->stats.paths += (uint64_t)base.n_dark * n_samples;  // (samples of sky pixels as before: counted, not rendered)
    ctx->stats.sky_pixel_samples += (uint64_t)base.n_dark * n_samples;
  }
  { const int rc = stream_plan(ctx, c.sc, count, base.n_sky && sky.filler_wgs, c.plan); if (rc) return rc; }
  if (ctx->tun.debug_tail) {  // (k_sky_resolve's list lengths of this call, printed below)
    if (!ctx->d_resolve_dbg) FH_HIP(ctx->d_resolve_dbg.alloc(2));
    FH_HIP(hipMemsetAsync(ctx->d_resolve_dbg, 0, 2 * sizeof(unsigned long long), ctx->stream));
    FH_HIP(hipEventRecord(ctx->ev_enter, ctx->stream));
    for (int k = 0; k + 1 < ctx->n_slots; ++k) FH_HIP(hipStreamWaitEvent(ctx->aux_stream[k], ctx->ev_enter, 0));
  }

  // (Small calls -- the reference's callers: 1 sample per call in the GUI, controller.cpp:224, 16 in rtcamp8, rtcamp8.cpp:183-189 -- cut into PIXEL sub-passes, each a pass of
  // its own in its own pool on its own stream, were built and measured in round 5: slower, configs[3] 1 spp 6.45 -> 8.24 ms.  tools/patches/r6_pruned_switches.patch, r5-4.)
  // Rounds: a plain call is one.  In adaptive mode a round ends where the samples requested since fh_init_render_states are a multiple of `step`, and the pixels
  // still active are selected from the call's base list at the start of every round (a call that starts between two boundaries selects too: that only drops the
  // pixels that stopped before; select_round).
  // (fh_set_adaptive_policy: with growth 2 a round runs to the next boundary b0 * 2^k, in as many passes as that takes.)
  PixelLists act = base;  // the pixels of the round; n_sky: the sky pixels the round's own selection left (guard blocks only)
  act.n_sky = 0;
  bool ran = false, sky_ran = false;
  int last_slot = 0;
  for (uint32_t call_done = 0; call_done < n_samples;) {
    uint32_t n_round = n_samples - call_done;
    if (adaptive) {
      const uint32_t to_boundary = ctx->adapt_growth == 1u ? ctx->adapt.step - ctx->adapt_total % ctx->adapt.step : adaptive_to_boundary(ctx);
      if (n_round > to_boundary) n_round = to_boundary;
      const int rc = select_round(c, sky, base, guard_blocks, ran ? last_slot : 0, n_round, act, sky_ran);
      if (rc) return rc;
    }
    const uint32_t batch = samples_per_pass(target, act.n_px, n_round, (uint32_t)ctx->n_slots, quirk, (ctx->flags & FH_FLAG_SERIAL_PASSES) != 0);
    // cooperative triangle tests: queued candidates that trigger a round.  48 (r5-12) -- but ONE-PASS calls of scenes without cut-outs keep 32
    // (r5-13, profiles/r05_latency_defaults.log: the soup's fh_render(1 / 4 / 16) take 2.02 / 3.37 / 7.02 ms with 32 and 2.21 / 3.62 / 7.32 with 48 -- a launch of few rays
    // waits longer for 48 candidates; the interior with cut-outs is 1 % faster with 48 there too).  FH_COOP_T fixes it for every call.
    const uint32_t coop_flush = (!ctx->tun.coop_flush_fixed && batch >= n_round && !c.sc.has_alpha && ctx->tun.coop_flush > 32u) ? 32u : ctx->tun.coop_flush;
    for (uint32_t done = 0; done < n_round && act.n_px; done += batch) {
      ran = true;
      const int rc = submit_pass(c, act, (n_round - done) < batch ? (n_round - done) : batch, batch, n_round, coop_flush, last_slot);
      if (rc) return rc;
    }
    call_done += n_round;
    ctx->adapt_total += n_round;
    if (adaptive && act.n_px == 0 && act.n_sky == 0) { ctx->adapt_total += n_samples - call_done; break; }  // (the active set only shrinks: no later round has a pixel)
  }
  // join: later work on the main stream (pack, post-process, copies, the caller's clears) sees every pass of this call
  // (the accumulates form a chain across the streams, so the last one implies all the others)
  if (last_slot != 0 && ran) FH_HIP(hipStreamWaitEvent(ctx->stream, ctx->slot[last_slot].ev_acc, 0));
  sky.end();
  if (base.n_sky && sky.st != ctx->stream) { FH_HIP(hipEventRecord(ctx->ev_sky, sky.st)); FH_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_sky, 0)); }
  FH_HIP(hipGetLastError());
  if (ctx->tun.debug_tail) {  // (a debug switch: this waits for the call)
    unsigned long long dbg[2] = {0ull, 0ull};
    FH_HIP(hipStreamSynchronize(ctx->stream));
    FH_HIP(hipMemcpy(dbg, ctx->d_resolve_dbg, sizeof(dbg), hipMemcpyDeviceToHost));
    if (base.n_sky || base.n_dark) fprintf(stderr, "[dark-sky] %u of %u sky pixels are dark\n", base.n_dark, base.n_sky + base.n_dark);
    if (dbg[1]) fprintf(stderr, "[sky-resolve] %llu queue entries, %llu escaped sky / light rays: %.4f per entry\n", dbg[1], dbg[0], (double)dbg[0] / (double)dbg[1]);
  }
  return FH_OK;
}

}  // namespace fh
