// envmap.hip -- the table behind fh_set_env_sampling: the environment's luminance on a 512 x 256 lat-long grid, quantised to integers, with the CDFs the shade
// kernels draw from (fh_envmap.h has the arithmetic, include/fredholm_hip.h states it).  Four launches on the context stream, no host synchronisation:
//   k_env_weights   one lane per cell: the mean of K x K sub-samples of lum(environment) * sin theta, and the table's maximum (a max of non-negative floats, as bits)
//   k_env_rows      one workgroup per row: the integer weights, their scan, the row sum and the row's conditional CDF
//   k_env_marginal  one workgroup: the scan of the row sums, the total and the marginal CDF
//   k_env_cells     one lane per cell: weight / total
// Everything after the maximum is integer arithmetic, so no result depends on the order the lanes run in.
#include <hip/hip_runtime.h>

#include "context.h"
#include "fh_envmap.h"

namespace fh {

namespace {

constexpr int kBlock = 256;
static_assert(kEnvW == 2 * kBlock && kEnvH == kBlock && kEnvCells % kBlock == 0, "the launches below are shaped for the 512 x 256 table");

// the environment as the table weighs it: sky intensity 1, and for a constant background the luminance 1 whatever its colour
__device__ __forceinline__ float env_table_lum(const FrameDev& fr, EnvDir d)
{
  if (!fr.has_ibl && !fr.has_hosek) return 1.0f;
  const f3 c = env_radiance(fr, mk3(d.x, d.y, d.z));
  return env_lum(c.x, c.y, c.z);
}

__global__ void __launch_bounds__(kBlock) k_env_weights(FrameDev fr, int k, float* w, uint32_t* max_bits)
{
  __shared__ float s_max[kBlock / 64];
  const int cell = (int)(blockIdx.x * kBlock + threadIdx.x);  // (the grid is kEnvCells / kBlock workgroups: every lane has a cell)
  const int i = cell % kEnvW, j = cell / kEnvW;
  float sum = 0.0f;
  for (int b = 0; b < k; ++b)
    for (int a = 0; a < k; ++a) {
      float u, v, st;
      env_subsample_uv(i, j, a, b, k, &u, &v);
      const EnvDir d = env_direction(u, v, &st);
      sum += env_sample_weight(env_table_lum(fr, d), st);
    }
  const float mean = env_cell_mean(sum, k);
  w[cell] = mean;
  float m = mean;
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
  if ((threadIdx.x & 63u) == 0u) s_max[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0u) {
    for (int q = 1; q < kBlock / 64; ++q) m = fmaxf(m, s_max[q]);
    atomicMax(max_bits, __float_as_uint(m));  // (m >= 0 and finite: floats of one sign order as their bits)
  }
}

// inclusive scan of one value per lane over the workgroup; returns the lane's exclusive prefix and the total
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

__global__ void __launch_bounds__(kBlock) k_env_rows(const float* w, const uint32_t* max_bits, uint32_t* q, uint32_t* row_sum, float* cdf_row)
{
  __shared__ uint32_t lds[kBlock];
  const int j = (int)blockIdx.x, i0 = 2 * (int)threadIdx.x;
  const float w_max = __uint_as_float(*max_bits);
  const uint32_t q0 = env_quantise(w[j * kEnvW + i0], w_max), q1 = env_quantise(w[j * kEnvW + i0 + 1], w_max);
  uint32_t total;
  const uint32_t before = block_scan<uint32_t>(q0 + q1, lds, &total);
  q[j * kEnvW + i0] = q0;
  q[j * kEnvW + i0 + 1] = q1;
  cdf_row[j * kEnvRowCdf + i0] = env_ratio(before, total);
  cdf_row[j * kEnvRowCdf + i0 + 1] = env_ratio(before + q0, total);
  if (threadIdx.x == 0u) { cdf_row[j * kEnvRowCdf + kEnvW] = 1.0f; row_sum[j] = total; }
}

__global__ void __launch_bounds__(kBlock) k_env_marginal(const uint32_t* row_sum, unsigned long long* total_out, float* cdf_m)
{
  __shared__ unsigned long long lds[kBlock];
  unsigned long long total;
  const unsigned long long before = block_scan<unsigned long long>(row_sum[threadIdx.x], lds, &total);
  cdf_m[threadIdx.x] = env_ratio(before, total);
  if (threadIdx.x == 0u) { cdf_m[kEnvH] = 1.0f; *total_out = total; }
}

__global__ void __launch_bounds__(kBlock) k_env_cells(const uint32_t* q, const unsigned long long* total, float* cell_p)
{
  const int cell = (int)(blockIdx.x * kBlock + threadIdx.x);
  cell_p[cell] = env_ratio(q[cell], *total);
}

}  // namespace

// the frame as the table sees the environment
FrameDev env_frame(const fh_ctx* ctx)
{
  FrameDev fr{};
  fr.has_hosek = ctx->has_hosek ? 1u : 0u;
  fr.has_ibl = ctx->d_ibl ? 1u : 0u;
  fr.ibl = fht_texture{nullptr, ctx->d_ibl, ctx->ibl_w, ctx->ibl_h, 0u};
  fr.bg = mk3(1.0f);
  fr.sky_intensity = 1.0f;
  fr.sun_dir = mk3(ctx->sun_dir[0], ctx->sun_dir[1], ctx->sun_dir[2]);
  fr.hosek = ctx->d_hosek;
  return fr;
}

int env_sampling_set(fh_ctx* ctx, const fh_env_sampling_params* params)
{
  if (!params) { ctx->env_sampling = 0; return FH_OK; }
  if (!ctx->d_env_cell_p) {
    FH_HIP(ctx->d_env_w.alloc((size_t)kEnvCells + 1));
    FH_HIP(ctx->d_env_q.alloc((size_t)kEnvCells + kEnvH));
    FH_HIP(ctx->d_env_total.alloc(1));
    FH_HIP(ctx->d_env_cdf_row.alloc((size_t)kEnvH * kEnvRowCdf));
    FH_HIP(ctx->d_env_cdf_m.alloc((size_t)kEnvH + 1));
    FH_HIP(ctx->d_env_cell_p.alloc((size_t)kEnvCells));
    ctx->env_stale = true;
  }
  if (!ctx->env_sampling) ctx->env_stale = true;
  ctx->env_sampling = 1;
  ctx->env_cosine_fraction = params->cosine_fraction;
  return FH_OK;
}

int env_table_ensure(fh_ctx* ctx)
{
  if (!ctx->env_stale) return FH_OK;
  const hipStream_t st = ctx->stream;
  float* const w = ctx->d_env_w;
  uint32_t* const max_bits = reinterpret_cast<uint32_t*>(w + kEnvCells);
  uint32_t* const q = ctx->d_env_q;
  uint32_t* const row_sum = q + kEnvCells;
  FH_HIP(hipMemsetAsync(max_bits, 0, sizeof(uint32_t), st));
  const int k = (int)env_subsamples(ctx->d_ibl ? ctx->ibl_w : 0u);
  hipLaunchKernelGGL(k_env_weights, dim3(kEnvCells / kBlock), dim3(kBlock), 0, st, env_frame(ctx), k, w, max_bits);
  hipLaunchKernelGGL(k_env_rows, dim3(kEnvH), dim3(kBlock), 0, st, (const float*)w, (const uint32_t*)max_bits, q, row_sum, ctx->d_env_cdf_row.get());
  hipLaunchKernelGGL(k_env_marginal, dim3(1), dim3(kBlock), 0, st, (const uint32_t*)row_sum, ctx->d_env_total.get(), ctx->d_env_cdf_m.get());
  hipLaunchKernelGGL(k_env_cells, dim3(kEnvCells / kBlock), dim3(kBlock), 0, st, (const uint32_t*)q, (const unsigned long long*)ctx->d_env_total.get(), ctx->d_env_cell_p.get());
  FH_HIP(hipGetLastError());
  ctx->env_stale = false;
  return FH_OK;
}

}  // namespace fh
