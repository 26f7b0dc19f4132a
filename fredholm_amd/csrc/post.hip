// post.hip -- bloom / chromatic aberration / exposure / Uchimura tone map / sRGB.
//
// Replaces post_process_kernel_launch (fredholm/kernels/src/post-process.cu:5-35) and its kernels
// bloom_kernel_0 (:60-74), bloom_kernel_1 (:76-109), tone_mapping_kernel (:111-153), copy_kernel (:49-58),
// helpers fredholm/kernels/include/kernels/post-process.h:13-124.
// Kept quirks: the launch grid is floor(W/16) x floor(H/16) blocks of 16x16, so rows/columns past the
// last full block are never written (:9-11); the blur weight is exp(-d^2 / (2*bloom_sigma)) (:97-98);
// the chromatic-aberration offset is divided by W*H (:124-125).  Not kept: a fetch address past the last pixel (:134-139, undefined there) reads the last pixel.
// The 33x33 blur reads its 48x48 source tile through LDS once per block instead of 1089 global
// loads per pixel; taps are summed in the reference's (v outer, u inner) order so results match
// the checker bit for bit.
#include <hip/hip_runtime.h>

#include <vector>

#include "context.h"
#include "fh_local_exposure.h"
#include "fh_meter.h"
#include "fh_tonemap.h"

namespace fh {
namespace {

constexpr int kR = 16;            // blur radius
constexpr int kT = 16;            // tile edge
constexpr int kS = kT + 2 * kR;   // staged edge (48)

__global__ void __launch_bounds__(256) k_bloom_threshold(const float4* in, int w, int gw, int gh, float threshold, float4* out)
{
  const int i = blockIdx.x * kT + threadIdx.x, j = blockIdx.y * kT + threadIdx.y;
  if (i >= gw || j >= gh) return;
  const float4 b = in[i + w * j];
  const float l = b.x * 0.2126729f + b.y * 0.7151522f + b.z * 0.0721750f;
  out[i + w * j] = l > threshold ? b : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

__global__ void __launch_bounds__(256) k_bloom_blur(const float4* in, const float4* hi, int w, int h, const float* weights, float wsum, float4* out)
{
  __shared__ float4 tile[kS * kS];
  __shared__ float wt[33 * 33];
  const int tid = threadIdx.y * kT + threadIdx.x;
  const int x0 = blockIdx.x * kT - kR, y0 = blockIdx.y * kT - kR;
  for (int k = tid; k < kS * kS; k += 256) {
    int x = x0 + k % kS, y = y0 + k / kS;
    x = x < 0 ? 0 : (x > w - 1 ? w - 1 : x);
    y = y < 0 ? 0 : (y > h - 1 ? h - 1 : y);
    tile[k] = hi[x + w * y];
  }
  for (int k = tid; k < 33 * 33; k += 256) wt[k] = weights[k];
  __syncthreads();
  const int i = blockIdx.x * kT + threadIdx.x, j = blockIdx.y * kT + threadIdx.y;
  float sx = 0.0f, sy = 0.0f, sz = 0.0f, sw = 0.0f;
  for (int v = 0; v < 33; ++v)
    for (int u = 0; u < 33; ++u) {
      const float hh = wt[v * 33 + u];
      const float4 b1 = tile[(threadIdx.y + v) * kS + threadIdx.x + u];
      sx += hh * b1.x; sy += hh * b1.y; sz += hh * b1.z; sw += hh * b1.w;
    }
  const float inv = 1.0f / wsum;
  const float4 b0 = in[i + w * j];
  out[i + w * j] = make_float4(b0.x + sx * inv, b0.y + sy * inv, b0.z + sz * inv, b0.w + sw * inv);
}

__global__ void __launch_bounds__(256) k_copy(const float4* in, int w, int gw, int gh, float4* out)
{
  const int i = blockIdx.x * kT + threadIdx.x, j = blockIdx.y * kT + threadIdx.y;
  if (i >= gw || j >= gh) return;
  out[i + w * j] = in[i + w * j];
}

__global__ void __launch_bounds__(256) k_tone_map(const float4* in, int w, int h, int gw, int gh, float exposure, float ca, float4* out)
{
  const int i = blockIdx.x * kT + threadIdx.x, j = blockIdx.y * kT + threadIdx.y;
  if (i >= gw || j >= gh) return;
  const TonemapFetch f = tonemap_fetch(i, j, w, h, ca);  // chromatic aberration: fh_tonemap.h
  float r = in[f.r].x, g = in[f.g].y, b = in[f.b].z;
  r *= exposure; g *= exposure; b *= exposure;
  r = srgb1(uchimura1(r)); g = srgb1(uchimura1(g)); b = srgb1(uchimura1(b));
  out[i + w * j] = make_float4(r, g, b, 1.0f);
}


// ------------------------------------------------------------------------------------------------
// Auto-exposure (fh_set_auto_exposure; the arithmetic is fh_meter.h's and stated in include/fredholm_hip.h).  No counterpart in the reference.
// k_meter_histogram counts every pixel of the input in one of 256 log2-luminance bins (word 256: unmetered) and leaves one 257-word slab per workgroup;
// k_meter_resolve sums the slabs, runs the serial resolve in one lane and writes the state and the exposure word; the metered forms of the threshold and the tone
// map read that word from device memory, so nothing comes back to the host between the metering and the chain.
constexpr int kMeterThreads = 256, kMeterWaves = kMeterThreads / 64, kMeterMaxBlocks = 512, kMeterLoads = 4, kResolveThreads = 1024;

struct MeterDev {
  fh_auto_exposure_state st;
  float exposure;              // fhe_pow(2, st.ev); valid while st.frames != 0
  uint32_t hist[kMeterWords];  // of the last metering call
};

// one count per valid lane into the wave's own histogram.  A wave's 64 pixels are neighbours and mostly share a bin (sky, a black background, a wall): in up to two
// rounds the lanes that agree with the first pending lane are counted by that lane with one plain add; what is left after that goes through LDS atomics.
// Called by whole waves (`valid` carries the image bound).
__device__ __forceinline__ void meter_count(uint32_t* h, int bin, bool valid)
{
  const int lane = (int)(threadIdx.x & 63u);
  for (int k = 0; k < 2; ++k) {
    const unsigned long long todo = __ballot(valid);
    if (todo == 0ull) return;
    const int leader = __ffsll((long long)todo) - 1;
    const int b0 = __shfl(bin, leader);
    const bool same = valid && bin == b0;
    const unsigned long long m = __ballot(same);
    if (lane == leader) h[b0] += (uint32_t)__popcll(m);
    if (same) valid = false;
  }
  if (valid) atomicAdd(&h[bin], 1u);
}

__global__ void __launch_bounds__(kMeterThreads) k_meter_histogram(const float4* in, uint32_t n, float log2_lo, float scale, uint32_t* slabs)
{
  __shared__ uint32_t s_h[kMeterWaves * kMeterWords];
  for (int k = threadIdx.x; k < kMeterWaves * kMeterWords; k += kMeterThreads) s_h[k] = 0u;
  __syncthreads();
  uint32_t* h = s_h + (threadIdx.x >> 6) * kMeterWords;
  const uint32_t stride = gridDim.x * (uint32_t)kMeterThreads;  // n <= 2^30 and kMeterLoads * stride <= 2^19: no index below wraps
  for (uint32_t base = blockIdx.x * (uint32_t)kMeterThreads; base < n; base += (uint32_t)kMeterLoads * stride) {  // (the trip count is the workgroup's: meter_count sees whole waves)
    float4 p[kMeterLoads];
    bool v[kMeterLoads];
#pragma unroll
    for (int k = 0; k < kMeterLoads; ++k) {  // all loads are issued before the first is used
      const uint32_t i = base + (uint32_t)k * stride + threadIdx.x;
      v[k] = i < n;
      p[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (v[k]) p[k] = in[i];
    }
#pragma unroll
    for (int k = 0; k < kMeterLoads; ++k) meter_count(h, meter_bin(p[k].x, p[k].y, p[k].z, log2_lo, scale), v[k]);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < kMeterWords; k += kMeterThreads) {
    uint32_t c = 0u;
    for (int wv = 0; wv < kMeterWaves; ++wv) c += s_h[wv * kMeterWords + k];
    slabs[(size_t)blockIdx.x * kMeterWords + k] = c;
  }
}

// one workgroup.  The slabs are summed by all lanes (integers: any order); the count before each bin comes from a scan, so the bins' terms of S are formed one per
// lane; what has to be serial -- the sum of the 256 doubles in bin order, and the state -- is left to one lane
__global__ void __launch_bounds__(kResolveThreads) k_meter_resolve(const uint32_t* slabs, uint32_t n_slabs, MeterConsts mc, MeterDev* md)
{
  constexpr int kParts = kResolveThreads / kMeterBins, kInFlight = 16;
  __shared__ uint32_t s_part[kParts * kMeterBins];
  __shared__ uint32_t s_scan[2][kMeterBins];
  __shared__ double s_term[kMeterBins];
  __shared__ uint32_t s_unmetered;
  const int t = threadIdx.x & (kMeterBins - 1), q = threadIdx.x / kMeterBins;
  if (threadIdx.x == 0) s_unmetered = 0u;
  __syncthreads();
  // lane (q, t) sums bin t of the slabs q, q + kParts, ...: kInFlight independent loads at a time (one workgroup reads all slabs, so this loop is bound by latency)
  uint32_t acc = 0u;
  for (uint32_t b = q; b < n_slabs; b += (uint32_t)(kInFlight * kParts)) {
    uint32_t x[kInFlight];
#pragma unroll
    for (int k = 0; k < kInFlight; ++k) {
      const uint32_t c = b + (uint32_t)(k * kParts);
      x[k] = c < n_slabs ? slabs[(size_t)c * kMeterWords + t] : 0u;
    }
#pragma unroll
    for (int k = 0; k < kInFlight; ++k) acc += x[k];
  }
  s_part[q * kMeterBins + t] = acc;
  uint32_t u = 0u;  // word 256 of every slab: one slab per lane and round
  for (uint32_t c = threadIdx.x; c < n_slabs; c += (uint32_t)kResolveThreads) u += slabs[(size_t)c * kMeterWords + kMeterBins];
  if (u != 0u) atomicAdd(&s_unmetered, u);
  __syncthreads();
  if (q == 0) {
    uint32_t c = 0u;
    for (int r = 0; r < kParts; ++r) c += s_part[r * kMeterBins + t];
    s_part[t] = c;
    s_scan[0][t] = c;
    md->hist[t] = c;
    if (t == 0) md->hist[kMeterBins] = s_unmetered;
  }
  __syncthreads();
  int cur = 0;
  for (int d = 1; d < kMeterBins; d <<= 1) {  // inclusive scan of the 256 counts
    if (q == 0) s_scan[cur ^ 1][t] = s_scan[cur][t] + (t >= d ? s_scan[cur][t - d] : 0u);
    cur ^= 1;
    __syncthreads();
  }
  const uint32_t n = s_scan[cur][kMeterBins - 1];
  if (n == 0u) return;  // nothing metered: the state is left alone (uniform: no barrier follows for some lanes only)
  uint32_t cut, end;
  meter_cuts(n, mc.low, mc.high, &cut, &end);
  if (q == 0) s_term[t] = meter_term(meter_kept(s_scan[cur][t] - s_part[t], s_part[t], cut, end), t, mc.log2_lo, mc.scale);
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int k = 0; k < kMeterBins; ++k) s += s_term[k];
    fh_auto_exposure_state st = md->st;
    meter_update(n, s_unmetered, s, cut, end, mc, &st);
    md->st = st;
    md->exposure = meter_exposure(st.ev);
  }
}

// k_bloom_threshold with the pixel's luminance scaled by the metered exposure (FH_AE_BLOOM_RELATIVE); iso_exposure: what it uses until a frame has been metered
__global__ void __launch_bounds__(256) k_bloom_threshold_metered(const float4* in, int w, int gw, int gh, float threshold, const MeterDev* md, float iso_exposure, float4* out)
{
  const int i = blockIdx.x * kT + threadIdx.x, j = blockIdx.y * kT + threadIdx.y;
  if (i >= gw || j >= gh) return;
  const float exposure = md->st.frames != 0u ? md->exposure : iso_exposure;
  const float4 b = in[i + w * j];
  const float l = b.x * 0.2126729f + b.y * 0.7151522f + b.z * 0.0721750f;
  out[i + w * j] = l * exposure > threshold ? b : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// k_tone_map with the exposure word read from device memory
__global__ void __launch_bounds__(256) k_tone_map_metered(const float4* in, int w, int h, int gw, int gh, const MeterDev* md, float iso_exposure, float ca, float4* out)
{
  const int i = blockIdx.x * kT + threadIdx.x, j = blockIdx.y * kT + threadIdx.y;
  if (i >= gw || j >= gh) return;
  const float exposure = md->st.frames != 0u ? md->exposure : iso_exposure;
  const TonemapFetch f = tonemap_fetch(i, j, w, h, ca);  // chromatic aberration: fh_tonemap.h
  float r = in[f.r].x, g = in[f.g].y, b = in[f.b].z;
  r *= exposure; g *= exposure; b *= exposure;
  r = srgb1(uchimura1(r)); g = srgb1(uchimura1(g)); b = srgb1(uchimura1(b));
  out[i + w * j] = make_float4(r, g, b, 1.0f);
}

// ------------------------------------------------------------------------------------------------
// Local exposure (fh_set_local_exposure; the arithmetic is fh_local_exposure.h's and stated in include/fredholm_hip.h).  No counterpart in the reference.
// k_lx_down reads the input once and leaves the log image and its 4 x 4 means; k_lx_atrous runs one edge-stopping pass on that quarter image; k_tone_map_local
// upsamples the base against each output pixel's own log-luminance, turns it into a gain and runs the tone map with it.
constexpr int kLxDownW = 64, kLxDownWaves = 4;  // a workgroup of k_lx_down: 64 columns x (4 waves x 4 rows)

// One wave per row of 4 x 4 blocks: lane x loads its column's pixel of each of the four rows -- a wave reads 1 KiB of consecutive float4 per row, all four loads
// issued before the first is used -- and the three lanes to the right of every fourth lane hand it their values, so the row sums are formed left to right in one
// lane, which then adds them top to bottom.  No LDS.
__global__ void __launch_bounds__(kLxDownW * kLxDownWaves) k_lx_down(const float4* in, int w, int h, int w4, float* logi, float* q0)
{
  const int x = blockIdx.x * kLxDownW + threadIdx.x;
  const int y0 = (blockIdx.y * kLxDownWaves + threadIdx.y) * kLxFactor;
  if (y0 >= h) return;  // (the whole wave: threadIdx.y is the wave)
  const bool col = x < w;
  const int n_rows = h - y0 < kLxFactor ? h - y0 : kLxFactor;
  const int n_cols = w - (x & ~3) < kLxFactor ? w - (x & ~3) : kLxFactor;  // of the block this lane lies in
  float4 p[kLxFactor];
#pragma unroll
  for (int k = 0; k < kLxFactor; ++k) {
    p[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (col && k < n_rows) p[k] = in[(size_t)x + (size_t)w * (size_t)(y0 + k)];
  }
  float row[kLxFactor];
#pragma unroll
  for (int k = 0; k < kLxFactor; ++k) {
    const float l = lx_log(p[k].x, p[k].y, p[k].z);
    if (col && k < n_rows) logi[(size_t)x + (size_t)w * (size_t)(y0 + k)] = l;
    const float l1 = __shfl_down(l, 1), l2 = __shfl_down(l, 2), l3 = __shfl_down(l, 3);  // by every lane of the wave
    row[k] = lx_row_sum(l, l1, l2, l3, n_cols);
  }
  if ((threadIdx.x & 3) == 0 && col) q0[(x >> 2) + w4 * (y0 >> 2)] = lx_block_mean(row[0], row[1], row[2], row[3], n_rows, n_cols);
}

__global__ void __launch_bounds__(256) k_lx_atrous(const float* src, int w4, int h4, int step, float inv_sr, float* dst)
{
  const int x = blockIdx.x * 16 + threadIdx.x, y = blockIdx.y * 16 + threadIdx.y;
  if (x >= w4 || y >= h4) return;
  dst[x + w4 * y] = lx_atrous(src, w4, h4, x, y, step, inv_sr);
}

// k_tone_map / k_tone_map_metered (md != nullptr) with the exposure multiplied by the output pixel's local gain
__global__ void __launch_bounds__(256) k_tone_map_local(const float4* in, const float* logi, const float* base, int w, int h, int gw, int gh, int w4, int h4, const MeterDev* md,
                                                        float iso_exposure, float ca, LxConsts lx, float4* out)
{
  const int i = blockIdx.x * kT + threadIdx.x, j = blockIdx.y * kT + threadIdx.y;
  if (i >= gw || j >= gh) return;
  const float exposure = (md && md->st.frames != 0u) ? md->exposure : iso_exposure;
  const float gain = lx_gain(lx_upsample(base, w4, h4, i, j, logi[i + w * j], lx.inv_sr), exposure, lx);
  const TonemapFetch f = tonemap_fetch(i, j, w, h, ca);  // chromatic aberration: fh_tonemap.h
  float r = in[f.r].x, g = in[f.g].y, b = in[f.b].z;
  r *= gain; g *= gain; b *= gain;
  r = srgb1(uchimura1(r)); g = srgb1(uchimura1(g)); b = srgb1(uchimura1(b));
  out[i + w * j] = make_float4(r, g, b, 1.0f);
}

// ------------------------------------------------------------------------------------------------
// Denoiser slot.  The reference calls NVIDIA's OptiX AI denoiser (fredholm/include/fredholm/denoiser.h:14-146: HDR model, albedo + normal
// guides, optional 2x upscale) -- a proprietary network with no counterpart here and nothing to be bit-compatible with.  What fills the slot is
// the classic guided filter it replaced in many renderers: the edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch, HPG 2010)
// on albedo-demodulated radiance, five passes of a 5x5 B3-spline kernel with hole sizes 1, 2, 4, 8, 16, edge-stopping weights on colour
// (relative to the local level, sigma halved per pass), normal and albedo.  Same inputs and output as the reference's class; `upscale` doubles the output by pixel replication.
constexpr float kDnSigmaColor = 2.0f, kDnSigmaNormal = 0.35f, kDnSigmaAlbedo = 0.2f, kDnAlbedoFloor = 0.01f;  // colour: relative to the mean of the two irradiances
constexpr int kDnPasses = 5;

__device__ __forceinline__ float dn_floor(float a) { return fmaxf(a, kDnAlbedoFloor); }
__device__ __forceinline__ float dn_finite(float v) { return (v != v || fabsf(v) > 3.0e38f) ? 0.0f : v; }

// pass `it`: src = irradiance of the previous pass (pass 0 reads beauty and demodulates); the last pass re-modulates and writes alpha 1
__global__ void __launch_bounds__(256) k_atrous(const float4* src, const float4* beauty, const float4* normal, const float4* albedo, int w, int h, int it, int last, int upscale, float4* dst)
{
  const int x = blockIdx.x * 16 + threadIdx.x, y = blockIdx.y * 16 + threadIdx.y;
  if (x >= w || y >= h) return;
  const int step = 1 << it;
  const float kern[3] = {3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
  const float inv_sc = 1.0f / (kDnSigmaColor * kDnSigmaColor * (1.0f / (float)(1 << (2 * it)))), inv_sn = 1.0f / (kDnSigmaNormal * kDnSigmaNormal),
              inv_sa = 1.0f / (kDnSigmaAlbedo * kDnSigmaAlbedo);
  auto irradiance = [&](int i) -> float4 {
    if (it != 0) return src[i];
    const float4 b = beauty[i], a = albedo[i];
    return make_float4(dn_finite(b.x) / dn_floor(a.x), dn_finite(b.y) / dn_floor(a.y), dn_finite(b.z) / dn_floor(a.z), 0.0f);
  };
  const int p = x + w * y;
  const float4 cp = irradiance(p), np = normal[p], ap = albedo[p];
  float sx = 0.0f, sy = 0.0f, sz = 0.0f, sw = 0.0f;
  for (int dy = -2; dy <= 2; ++dy)
    for (int dx = -2; dx <= 2; ++dx) {
      int qx = x + dx * step, qy = y + dy * step;
      qx = qx < 0 ? 0 : (qx > w - 1 ? w - 1 : qx);
      qy = qy < 0 ? 0 : (qy > h - 1 ? h - 1 : qy);
      const int q = qx + w * qy;
      const float4 cq = irradiance(q), nq = normal[q], aq = albedo[q];
      const float dcx = cq.x - cp.x, dcy = cq.y - cp.y, dcz = cq.z - cp.z;
      const float dnx = nq.x - np.x, dny = nq.y - np.y, dnz = nq.z - np.z;
      const float dax = aq.x - ap.x, day = aq.y - ap.y, daz = aq.z - ap.z;
      const float m = (cq.x + cq.y + cq.z) + (cp.x + cp.y + cp.z);  // colour distance relative to the local level: HDR input
      const float den = m * m * (1.0f / 9.0f) + 1e-4f;
      const float e = ((dcx * dcx + dcy * dcy + dcz * dcz) / den) * inv_sc + (dnx * dnx + dny * dny + dnz * dnz) * inv_sn + (dax * dax + day * day + daz * daz) * inv_sa;
      const float wgt = kern[dx < 0 ? -dx : dx] * kern[dy < 0 ? -dy : dy] * fhe_exp(-e);
      sx += wgt * cq.x; sy += wgt * cq.y; sz += wgt * cq.z; sw += wgt;
    }
  const float inv = 1.0f / sw;  // the centre tap has weight 9/64: never zero
  float4 o = make_float4(sx * inv, sy * inv, sz * inv, 0.0f);
  if (!last) { dst[p] = o; return; }
  o = make_float4(o.x * dn_floor(ap.x), o.y * dn_floor(ap.y), o.z * dn_floor(ap.z), 1.0f);
  if (!upscale) { dst[p] = o; return; }
  const int w2 = 2 * w;
  dst[2 * x + w2 * (2 * y)] = o; dst[2 * x + 1 + w2 * (2 * y)] = o; dst[2 * x + w2 * (2 * y + 1)] = o; dst[2 * x + 1 + w2 * (2 * y + 1)] = o;
}

}  // namespace

int post_process_submit(fh_ctx* ctx, const float* in, float* hi, float* tmp, int w, int h, const fh_post_params* pp, float* out)
{
  hipStream_t st = ctx->stream;
  // FH_FLAG_TIME_KERNELS: HIP events around the whole chain (fh_stats.post_ms, reduced at fh_sync like the render spans: kind 7)
  Event ev_a, ev_b;
  const bool timed = (ctx->flags & FH_FLAG_TIME_KERNELS) != 0;
  if (timed) { ev_a = take_event(ctx); ev_b = take_event(ctx); (void)hipEventRecord(ev_a, st); }
  const int bx = w / kT > 1 ? w / kT : 1, by = h / kT > 1 ? h / kT : 1;  // floor division, post-process.cu:9-11
  const int gw = bx * kT < w ? bx * kT : w, gh = by * kT < h ? by * kT : h;
  const dim3 grid(bx, by), block(kT, kT);
  // fh_set_auto_exposure: metering -> resolve -> the chain, all on the stream; the chain's metered kernels read what the resolve wrote
  const bool metered = ctx->auto_exposure != 0;
  const MeterDev* md = (const MeterDev*)ctx->d_meter.get();
  const float exposure = exposure_from_ev100(ev100_of(1.0f, 1.0f, pp->ISO));
  if (pp->use_bloom && (w < kT || h < kT)) return fail(ctx, FH_E_UNSUPPORTED, "bloom needs an image of at least 16x16 pixels");
  if (metered) {
    if (w > 32768 || h > 32768) return fail(ctx, FH_E_INVALID, "fh_post_process: auto-exposure meters images of at most 32768 x 32768 pixels");
    const int rc = meter_submit(ctx, in, (uint32_t)w, (uint32_t)h);
    if (rc != FH_OK) return rc;
  }
  // fh_set_local_exposure: the analysis of the input goes first; the tone map at the end reads the log image and the base it left
  const bool local = ctx->local_exposure != 0;
  if (local) {
    if (w > 32768 || h > 32768) return fail(ctx, FH_E_INVALID, "fh_post_process: local exposure analyses images of at most 32768 x 32768 pixels");
    const int rc = local_exposure_submit(ctx, in, (uint32_t)w, (uint32_t)h);
    if (rc != FH_OK) return rc;
  }
  if (pp->use_bloom) {
    // the 1089 weights depend on bloom_sigma only: computed and uploaded when sigma changes, kept in the context otherwise
    // (no allocation, copy or host synchronisation per frame)
    FH_HIP(ctx->d_bloom_weights.ensure(33 * 33));
    if (ctx->bloom_sigma_cached != pp->bloom_sigma) {
      std::vector<float> wt(33 * 33);
      float wsum = 0.0f;
      for (int v = -kR; v <= kR; ++v)
        for (int u = -kR; u <= kR; ++u) {
          const float dist2 = (float)(u * u + v * v);
          const float hh = fhe_exp(-dist2 / (2.0f * pp->bloom_sigma));
          wt[(v + kR) * 33 + (u + kR)] = hh;
          wsum += hh;
        }
      FH_HIP(hipStreamSynchronize(st));  // an earlier frame may still read the old weights
      FH_HIP(hipMemcpy(ctx->d_bloom_weights, wt.data(), wt.size() * sizeof(float), hipMemcpyHostToDevice));
      ctx->bloom_sigma_cached = pp->bloom_sigma;
      ctx->bloom_wsum = wsum;
    }
    if (metered && (ctx->ae_params.flags & FH_AE_BLOOM_RELATIVE)) hipLaunchKernelGGL(k_bloom_threshold_metered, grid, block, 0, st, (const float4*)in, w, gw, gh, pp->bloom_threshold, md, exposure, (float4*)hi);
    else hipLaunchKernelGGL(k_bloom_threshold, grid, block, 0, st, (const float4*)in, w, gw, gh, pp->bloom_threshold, (float4*)hi);
    hipLaunchKernelGGL(k_bloom_blur, grid, block, 0, st, (const float4*)in, (const float4*)hi, w, h, ctx->d_bloom_weights, ctx->bloom_wsum, (float4*)tmp);
  } else {
    hipLaunchKernelGGL(k_copy, grid, block, 0, st, (const float4*)in, w, gw, gh, (float4*)tmp);
  }
  if (local) hipLaunchKernelGGL(k_tone_map_local, grid, block, 0, st, (const float4*)tmp, (const float*)ctx->d_lx_log.get(), (const float*)ctx->d_lx_q[ctx->lx_passes_run & 1u].get(), w, h, gw, gh,
                                (int)ctx->lx_w4, (int)ctx->lx_h4, metered ? md : nullptr, exposure, pp->chromatic_aberration, lx_consts(ctx->lx_params), (float4*)out);
  else if (metered) hipLaunchKernelGGL(k_tone_map_metered, grid, block, 0, st, (const float4*)tmp, w, h, gw, gh, md, exposure, pp->chromatic_aberration, (float4*)out);
  else hipLaunchKernelGGL(k_tone_map, grid, block, 0, st, (const float4*)tmp, w, h, gw, gh, exposure, pp->chromatic_aberration, (float4*)out);
  if (timed) { (void)hipEventRecord(ev_b, st); ctx->spans.push_back({std::move(ev_a), std::move(ev_b), 7}); ctx->stats.n_post_launches++; }
  FH_HIP(hipGetLastError());
  return FH_OK;
}

// ---- auto-exposure, host side
int auto_exposure_set(fh_ctx* ctx, const fh_auto_exposure_params* params)
{
  if (!params) {
    if (ctx->d_meter) FH_HIP(hipMemsetAsync(ctx->d_meter, 0, sizeof(MeterDev), ctx->stream));  // the state is dropped; the allocation is kept for the next switch-on
    ctx->auto_exposure = 0;
    return FH_OK;
  }
  FH_HIP(ctx->d_meter.ensure(sizeof(MeterDev)));
  if (!ctx->auto_exposure) FH_HIP(hipMemsetAsync(ctx->d_meter, 0, sizeof(MeterDev), ctx->stream));  // off -> on: frames = 0; on -> on keeps the state
  ctx->auto_exposure = 1;
  ctx->ae_params = *params;
  return FH_OK;
}

int meter_submit(fh_ctx* ctx, const float* image, uint32_t w, uint32_t h)
{
  hipStream_t st = ctx->stream;
  const uint32_t n = w * h;  // w, h <= 32768
  const uint32_t per_block = (uint32_t)(kMeterLoads * kMeterThreads);
  uint32_t blocks = (n + per_block - 1u) / per_block;
  blocks = blocks < 1u ? 1u : (blocks > (uint32_t)kMeterMaxBlocks ? (uint32_t)kMeterMaxBlocks : blocks);
  if (ctx->d_meter_slabs.size() < (size_t)blocks * kMeterWords) {  // grows on demand, never per frame
    FH_HIP(hipStreamSynchronize(st));                              // an earlier call may still use the old slabs
    FH_HIP(ctx->d_meter_slabs.alloc((size_t)blocks * kMeterWords));
  }
  const MeterConsts mc = meter_consts(ctx->ae_params);
  hipLaunchKernelGGL(k_meter_histogram, dim3(blocks), dim3(kMeterThreads), 0, st, (const float4*)image, n, mc.log2_lo, mc.scale, ctx->d_meter_slabs);
  hipLaunchKernelGGL(k_meter_resolve, dim3(1), dim3(kResolveThreads), 0, st, (const uint32_t*)ctx->d_meter_slabs.get(), blocks, mc, (MeterDev*)ctx->d_meter.get());
  FH_HIP(hipGetLastError());
  return FH_OK;
}

int auto_exposure_reset(fh_ctx* ctx)
{
  FH_HIP(hipMemsetAsync(&((MeterDev*)ctx->d_meter.get())->st.frames, 0, sizeof(uint32_t), ctx->stream));
  return FH_OK;
}

int auto_exposure_read(fh_ctx* ctx, fh_auto_exposure_state* state, uint32_t* hist)
{
  MeterDev host;
  FH_HIP(hipMemcpyAsync(&host, ctx->d_meter, sizeof(MeterDev), hipMemcpyDeviceToHost, ctx->stream));
  FH_HIP(hipStreamSynchronize(ctx->stream));
  if (state) *state = host.st;
  if (hist) for (int k = 0; k < kMeterWords; ++k) hist[k] = host.hist[k];
  return FH_OK;
}

// ---- local exposure, host side
int local_exposure_set(fh_ctx* ctx, const fh_local_exposure_params* params)
{
  if (!params || !ctx->local_exposure) ctx->lx_w4 = ctx->lx_h4 = ctx->lx_passes_run = 0;  // off, or off -> on: no analysis to read back; the allocations are kept
  ctx->local_exposure = params ? 1 : 0;
  if (params) ctx->lx_params = *params;
  return FH_OK;
}

int local_exposure_submit(fh_ctx* ctx, const float* image, uint32_t w, uint32_t h)
{
  hipStream_t st = ctx->stream;
  const int w4 = lx_quarter((int)w), h4 = lx_quarter((int)h);  // w, h <= 32768
  const size_t n = (size_t)w * h, n4 = (size_t)w4 * h4;
  if (ctx->d_lx_log.size() < n || ctx->d_lx_q[0].size() < n4 || ctx->d_lx_q[1].size() < n4) {  // grow on demand, never per frame
    FH_HIP(hipStreamSynchronize(st));                                                       // an earlier call may still use the old images
    FH_HIP(ctx->d_lx_log.ensure(n));
    for (int k = 0; k < 2; ++k) FH_HIP(ctx->d_lx_q[k].ensure(n4));
  }
  const LxConsts lx = lx_consts(ctx->lx_params);
  hipLaunchKernelGGL(k_lx_down, dim3((w + kLxDownW - 1) / kLxDownW, (h + kLxDownWaves * kLxFactor - 1) / (kLxDownWaves * kLxFactor)), dim3(kLxDownW, kLxDownWaves), 0, st,
                     (const float4*)image, (int)w, (int)h, w4, ctx->d_lx_log.get(), ctx->d_lx_q[0].get());
  const dim3 grid((w4 + 15) / 16, (h4 + 15) / 16), block(16, 16);
  for (uint32_t it = 0; it < ctx->lx_params.passes; ++it)
    hipLaunchKernelGGL(k_lx_atrous, grid, block, 0, st, (const float*)ctx->d_lx_q[it & 1u].get(), w4, h4, 1 << it, lx.inv_sr, ctx->d_lx_q[(it + 1u) & 1u].get());
  ctx->lx_w4 = (uint32_t)w4; ctx->lx_h4 = (uint32_t)h4; ctx->lx_passes_run = ctx->lx_params.passes;
  FH_HIP(hipGetLastError());
  return FH_OK;
}

int local_exposure_read_base(fh_ctx* ctx, float* base, uint32_t* w4, uint32_t* h4)
{
  *w4 = ctx->lx_w4; *h4 = ctx->lx_h4;
  const size_t n4 = (size_t)ctx->lx_w4 * ctx->lx_h4;
  if (!base || n4 == 0) return FH_OK;
  FH_HIP(hipMemcpyAsync(base, ctx->d_lx_q[ctx->lx_passes_run & 1u].get(), n4 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  FH_HIP(hipStreamSynchronize(ctx->stream));
  return FH_OK;
}

int denoise_submit(fh_ctx* ctx, int w, int h, const float* beauty, const float* normal, const float* albedo, float* out, int upscale)
{
  hipStream_t st = ctx->stream;
  const size_t px = (size_t)w * h;
  for (int k = 0; k < 2; ++k) FH_HIP(ctx->d_denoise_tmp[k].ensure(px));  // two ping-pong irradiance buffers, kept in the context
  const dim3 grid((w + 15) / 16, (h + 15) / 16), block(16, 16);
  const float4* src = nullptr;
  for (int it = 0; it < kDnPasses; ++it) {
    const int last = it == kDnPasses - 1;
    float4* dst = last ? (float4*)out : ctx->d_denoise_tmp[it & 1];
    hipLaunchKernelGGL(k_atrous, grid, block, 0, st, src, (const float4*)beauty, (const float4*)normal, (const float4*)albedo, w, h, it, last, upscale, dst);
    src = dst;
  }
  FH_HIP(hipGetLastError());
  return FH_OK;
}

}  // namespace fh
