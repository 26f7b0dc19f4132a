// lights.hip -- the table behind fh_set_light_sampling: the emitters' weights (area x luminance of the emission), quantised to integers, with the CDF the shade kernels
// pick from and the pick probability of every face (fh_lights.h has the arithmetic, include/fredholm_hip.h states it).  One clear and five launches on the context
// stream, no host synchronisation once the buffers have their size:
//   k_light_weights  one lane per emitter: its weight, and the table's maximum (a max of non-negative floats, as bits: one atomicMax per workgroup)
//   k_light_chunks   one workgroup per chunk of kBlock emitters: the integer weights and the chunk's sum
//   k_light_offsets  one workgroup: the exclusive scan of the chunk sums (kBlock at a time, carrying the running sum) and the total
//   k_light_write    one workgroup per chunk: the scan inside the chunk, the CDF entries and the pick probabilities of the emitters' faces
//   k_light_proxies  one lane per emitter: centroid, area and mean shading normal, what fh_set_light_resampling weighs a candidate by (two float4 stores)
// Everything after the maximum is integer arithmetic, so no result depends on the order the lanes run in.
#include <hip/hip_runtime.h>

#include "context.h"
#include "fh_lights.h"
#include "fh_trace.h"

namespace fh {

namespace {

constexpr int kBlock = 256;  // lanes of a workgroup = emitters of a chunk (tests/test_gpu_light_sampling.py names it: its strips straddle 1, 4 and 256 chunks)

// get_emission (pt.cu:131-139), as render.hip's emission_of has it
__device__ __forceinline__ f3 light_emission(const SceneDev& sc, const MaterialDev& m, float tu, float tv)
{
  const int id = __float_as_int(m.w[41]);
  return id >= 0 ? tex_rgb(sc, id, tu, tv) : mk3(m.w[38], m.w[39], m.w[40]);
}

__global__ void __launch_bounds__(kBlock) k_light_weights(SceneDev sc, uint32_t n_faces, float* w, uint32_t* max_bits)
{
  __shared__ float s_max[kBlock / 64];
  const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
  float wk = 0.0f;
  if (k < sc.n_lights) {
    const AreaLightDev lt = sc.lights[k];
    if (lt.face < n_faces && lt.material < sc.n_materials) {  // (the upload's plan guarantees both; a table never reads past the arrays it was given)
      const size_t fb = kFaceRec * (size_t)lt.face;
      const float4 l0 = sc.face_rec[fb], l1 = sc.face_rec[fb + 1], l2 = sc.face_rec[fb + 2], l3 = sc.face_rec[fb + 3], l4 = sc.face_rec[fb + 4], l5 = sc.face_rec[fb + 5];
      const float area = 0.5f * length(cross(mk3(l1) - mk3(l0), mk3(l2) - mk3(l0)));
      const MaterialDev& lm = sc.materials[lt.material];
      f3 e = mk3(lm.w[38], lm.w[39], lm.w[40]);
      if (__float_as_int(lm.w[41]) >= 0) {
        f3 sum = mk3(0.0f);
        for (int s = 0; s < kLightPoints; ++s) {
          float bu, bv;
          light_point(s, &bu, &bv);
          sum += light_emission(sc, lm, light_lerp(l0.w, l2.w, l4.w, bu, bv), light_lerp(l1.w, l3.w, l5.w, bu, bv));
        }
        e = mk3(sum.x / (float)kLightPoints, sum.y / (float)kLightPoints, sum.z / (float)kLightPoints);
      }
      wk = light_weight(area, e.x, e.y, e.z);
    }
    w[k] = wk;
  }
  float m = wk + 0.0f;  // (-0, which a colour of negative zeros gives, becomes +0: as bits it would win the maximum below)
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
  if ((threadIdx.x & 63u) == 0u) s_max[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0u) {
    for (int q = 1; q < kBlock / 64; ++q) m = fmaxf(m, s_max[q]);
    atomicMax(max_bits, __float_as_uint(m));  // (m is +0 or positive, and finite: such floats order as their bits)
  }
}

// inclusive scan of one value per lane over the workgroup; returns the lane's exclusive prefix and the total (envmap.hip has the same)
template <typename T>
__device__ __forceinline__ T block_scan(T v, T* lds, T* total)
{
  lds[threadIdx.x] = v;
  __syncthreads();
  for (uint32_t off = 1; off < (uint32_t)kBlock; off <<= 1) {
    const T add = threadIdx.x >= off ? lds[threadIdx.x - off] : (T)0;
    __syncthreads();
    lds[threadIdx.x] += add;
    __syncthreads();
  }
  *total = lds[kBlock - 1];
  return lds[threadIdx.x] - v;
}

__global__ void __launch_bounds__(kBlock) k_light_chunks(const float* w, const uint32_t* max_bits, uint32_t n, uint32_t* q, uint32_t* chunk_sum)
{
  __shared__ uint32_t s_sum[kBlock / 64];
  const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
  const float w_max = __uint_as_float(*max_bits);
  const uint32_t qk = k < n ? light_quantise(w[k], w_max) : 0u;
  if (k < n) q[k] = qk;
  uint32_t sum = qk;  // the chunk's sum alone (at most kBlock * 2^20 = 2^28): a wave reduction and one LDS step; k_light_write makes the prefixes
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
  if ((threadIdx.x & 63u) == 0u) s_sum[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0u) {
    for (int v = 1; v < kBlock / 64; ++v) sum += s_sum[v];
    chunk_sum[blockIdx.x] = sum;
  }
}

// offsets[c] = sum of the chunks before c, c = 0 .. n_chunks; offsets[n_chunks] = T
__global__ void __launch_bounds__(kBlock) k_light_offsets(const uint32_t* chunk_sum, uint32_t n_chunks, unsigned long long* offsets)
{
  __shared__ unsigned long long lds[kBlock];
  unsigned long long carry = 0;
  for (uint32_t base = 0; base < n_chunks; base += kBlock) {  // (block-uniform bound: block_scan holds barriers)
    const uint32_t c = base + threadIdx.x;
    unsigned long long total;
    const unsigned long long before = block_scan<unsigned long long>(c < n_chunks ? chunk_sum[c] : 0u, lds, &total);
    if (c < n_chunks) offsets[c] = carry + before;
    carry += total;
    __syncthreads();  // (the next round overwrites lds)
  }
  if (threadIdx.x == 0u) offsets[n_chunks] = carry;
}

__global__ void __launch_bounds__(kBlock) k_light_write(const uint32_t* q, const unsigned long long* offsets, uint32_t n_chunks, const AreaLightDev* lights, uint32_t n, uint32_t n_faces,
                                                         float uniform, float* cdf, float* pick_p)
{
  __shared__ uint32_t lds[kBlock];
  const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t qk = k < n ? q[k] : 0u;
  uint32_t chunk_total;
  const uint32_t before = block_scan<uint32_t>(qk, lds, &chunk_total);
  if (k >= n) return;
  const unsigned long long total = offsets[n_chunks];
  cdf[k] = env_ratio(offsets[blockIdx.x] + before, total);
  if (k == n - 1u) cdf[n] = 1.0f;
  const uint32_t face = lights[k].face;
  if (face < n_faces) pick_p[face] = light_pick_p(qk, total, n, uniform);
}

// the proxies of fh_set_light_resampling, in emitter order.  The area is k_light_weights' expression
__global__ void __launch_bounds__(kBlock) k_light_proxies(SceneDev sc, uint32_t n_faces, LightProxy* proxy)
{
  const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= sc.n_lights) return;
  LightProxy pr = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  const uint32_t face = sc.lights[k].face;
  if (face < n_faces) {
    const size_t fb = kFaceRec * (size_t)face;
    const float4 l0 = sc.face_rec[fb], l1 = sc.face_rec[fb + 1], l2 = sc.face_rec[fb + 2], l3 = sc.face_rec[fb + 3], l4 = sc.face_rec[fb + 4], l5 = sc.face_rec[fb + 5];
    const float area = 0.5f * length(cross(mk3(l1) - mk3(l0), mk3(l2) - mk3(l0)));
    const float p0[3] = {l0.x, l0.y, l0.z}, p1[3] = {l1.x, l1.y, l1.z}, p2[3] = {l2.x, l2.y, l2.z};
    const float n0[3] = {l3.x, l3.y, l3.z}, n1[3] = {l4.x, l4.y, l4.z}, n2[3] = {l5.x, l5.y, l5.z};
    pr = light_proxy(p0, p1, p2, n0, n1, n2, area);
  }
  float4* const out = reinterpret_cast<float4*>(proxy + k);
  out[0] = make_float4(pr.cx, pr.cy, pr.cz, pr.area);
  out[1] = make_float4(pr.mx, pr.my, pr.mz, pr.pad);
}

uint32_t chunks_of(uint32_t n) { return (n + (uint32_t)kBlock - 1u) / (uint32_t)kBlock; }

}  // namespace

int light_sampling_set(fh_ctx* ctx, const fh_light_sampling_params* params)
{
  if (!params) { ctx->light_sampling = 0; return FH_OK; }
  if (!ctx->light_sampling || ctx->light_uniform_fraction != params->uniform_fraction) {
    // a pass of an earlier call may still be reading the table the next call rebuilds
    FH_HIP(drain_passes(ctx, false));
    ctx->light_stale = true;
  }
  ctx->light_sampling = 1;
  ctx->light_uniform_fraction = params->uniform_fraction;
  return FH_OK;
}

int light_table_ensure(fh_ctx* ctx)
{
  if (!ctx->light_stale || ctx->n_lights == 0) return FH_OK;
  const hipStream_t st = ctx->stream;
  const uint32_t n = ctx->n_lights, n_faces = ctx->n_faces, n_chunks = chunks_of(n);
  // exactly the scene's sizes: nothing of another scene's table survives an upload.  (Freeing a buffer waits for the device, so this happens only when a size changed.)
  if (ctx->d_light_cdf.size() != (size_t)n + 1 || ctx->d_light_pick_p.size() != (size_t)n_faces) {
    FH_HIP(ctx->d_light_w.alloc((size_t)n + 1));
    FH_HIP(ctx->d_light_q.alloc((size_t)n + n_chunks));
    FH_HIP(ctx->d_light_offsets.alloc((size_t)n_chunks + 1));
    FH_HIP(ctx->d_light_cdf.alloc((size_t)n + 1));
    FH_HIP(ctx->d_light_pick_p.alloc((size_t)n_faces));
    FH_HIP(ctx->d_light_proxy.alloc((size_t)n));
  }
  float* const w = ctx->d_light_w;
  uint32_t* const max_bits = reinterpret_cast<uint32_t*>(w + n);
  uint32_t* const q = ctx->d_light_q;
  uint32_t* const chunk_sum = q + n;
  FH_HIP(hipMemsetAsync(max_bits, 0, sizeof(uint32_t), st));
  FH_HIP(hipMemsetAsync(ctx->d_light_pick_p, 0, sizeof(float) * (size_t)n_faces, st));  // the faces that do not emit
  hipLaunchKernelGGL(k_light_weights, dim3(n_chunks), dim3(kBlock), 0, st, scene_dev(ctx), n_faces, w, max_bits);
  hipLaunchKernelGGL(k_light_chunks, dim3(n_chunks), dim3(kBlock), 0, st, (const float*)w, (const uint32_t*)max_bits, n, q, chunk_sum);
  hipLaunchKernelGGL(k_light_offsets, dim3(1), dim3(kBlock), 0, st, (const uint32_t*)chunk_sum, n_chunks, ctx->d_light_offsets.get());
  hipLaunchKernelGGL(k_light_write, dim3(n_chunks), dim3(kBlock), 0, st, (const uint32_t*)q, (const unsigned long long*)ctx->d_light_offsets.get(), n_chunks,
                     (const AreaLightDev*)ctx->d_lights.get(), n, n_faces, ctx->light_uniform_fraction, ctx->d_light_cdf.get(), ctx->d_light_pick_p.get());
  hipLaunchKernelGGL(k_light_proxies, dim3(n_chunks), dim3(kBlock), 0, st, scene_dev(ctx), n_faces, ctx->d_light_proxy.get());
  FH_HIP(hipGetLastError());
  ctx->light_stale = false;
  return FH_OK;
}

}  // namespace fh
