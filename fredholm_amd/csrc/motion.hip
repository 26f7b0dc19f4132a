// motion.hip -- per-instance motion vectors for the temporal stage (include/fredholm_hip.h): the id plane (fh_primary_instances), the host-side motion table
// (fh_motion_from_transforms), and the entry points that feed denoise.hip's k_temporal<kLookMotion, .> (fh_denoise_temporal_motion, fh_set_denoise_motion).
//
// k_primary_instances: every pixel builds its chief ray (fh_chief_ray.h) and traces it for its closest hit with the traversal code the render kernels run, entered
// the way fh_trace_rays (kat.hip) enters it: the wave-cooperative traversal with its per-wave LDS on trees small enough for it, `traverse` otherwise.  32 x 8 pixels
// per workgroup like the denoiser's kernels: a wave is two rows of 32 neighbouring pixels, whose rays walk the same nodes.  Pixels beyond the frame's edge stay in
// the cooperative traversal as invalid lanes (all 64 lanes enter together) and write nothing.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "context.h"
#include "fh_chief_ray.h"
#include "fh_trace.h"
#include "motion_host.h"

namespace fh {
namespace {

constexpr int kTW = 32, kTH = 8;
constexpr float kChiefTmax = 1e9f;  // what fh_render's camera rays are traced to

__device__ __forceinline__ void store_instance(const uint2* face_meta, uint32_t width, uint32_t x, uint32_t y, bool hit, uint32_t prim, uint32_t* ids)
{
  ids[(size_t)x + (size_t)width * y] = hit ? face_meta[prim].y : 0xffffffffu;
}

template <bool ALPHA>
__global__ void __launch_bounds__(256) k_primary_instances_coop(SceneDev sc, ChiefCam cam, const uint2* face_meta, uint32_t flush, uint32_t* ids)
{
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * kCoopLdsBytesPerWave];
  const uint32_t tid = threadIdx.y * kTW + threadIdx.x;
  const CoopLds cl = coop_lds(lds, tid >> 6);
  const uint32_t x = blockIdx.x * kTW + threadIdx.x, y = blockIdx.y * kTH + threadIdx.y;
  const bool valid = x < cam.width && y < cam.height;
  f3 org, dir;
  chief_ray(cam, valid ? x : 0u, valid ? y : 0u, org, dir);
  HitRec h;
  uint32_t a = 0, b = 0;
  const bool ok = traverse_bvh8_coop<false, false, false, ALPHA>(sc.bvh8, valid, org, dir, kChiefTmax, h, a, b, nullptr, cl, flush, nullptr, 0, &sc);
  if (valid) store_instance(face_meta, cam.width, x, y, ok, h.prim, ids);
}

__global__ void __launch_bounds__(256) k_primary_instances(SceneDev sc, ChiefCam cam, const uint2* face_meta, uint32_t* ids)
{
  const uint32_t x = blockIdx.x * kTW + threadIdx.x, y = blockIdx.y * kTH + threadIdx.y;
  if (x >= cam.width || y >= cam.height) return;
  f3 org, dir;
  chief_ray(cam, x, y, org, dir);
  HitRec h;
  uint32_t a = 0, b = 0;
  const bool ok = traverse<false, false>(sc, org, dir, kChiefTmax, h, a, b);
  store_instance(face_meta, cam.width, x, y, ok, h.prim, ids);
}

}  // namespace

int primary_instances_submit(fh_ctx* ctx, const fh_camera* cam, uint32_t w, uint32_t h, uint32_t* ids)
{
  ChiefCam c{};
  for (int r = 0; r < 3; ++r) c.xf.r[r] = make_float4(cam->transform[4 * r], cam->transform[4 * r + 1], cam->transform[4 * r + 2], cam->transform[4 * r + 3]);
  c.inv_tan = 1.0f / tanf(0.5f * cam->fov);
  c.apb = chief_a_plus_b(c.inv_tan, cam->focus);
  c.width = w; c.height = h;
  const SceneDev sd = scene_dev(ctx);
  const dim3 grid((w + kTW - 1) / kTW, (h + kTH - 1) / kTH), block(kTW, kTH);
  if (sd.use_bvh8 && sd.bvh8.n_tris < kCoopMaxTris && ctx->tun.coop) {
    if (sd.has_alpha) hipLaunchKernelGGL((k_primary_instances_coop<true>), grid, block, 0, ctx->stream, sd, c, ctx->d_face_meta, ctx->tun.coop_flush, ids);
    else hipLaunchKernelGGL((k_primary_instances_coop<false>), grid, block, 0, ctx->stream, sd, c, ctx->d_face_meta, ctx->tun.coop_flush, ids);
  } else {
    hipLaunchKernelGGL(k_primary_instances, grid, block, 0, ctx->stream, sd, c, ctx->d_face_meta, ids);
  }
  FH_HIP(hipGetLastError());
  return FH_OK;
}

}  // namespace fh

using namespace fh;

#define MCTX_CHECK(ctx)                     \
  if (!(ctx)) return FH_E_INVALID;          \
  if (hipSetDevice((ctx)->device) != hipSuccess) return fh::fail(ctx, FH_E_HIP, "hipSetDevice failed")

extern "C" {

int fh_primary_instances(fh_ctx* ctx, const fh_camera* camera, uint32_t width, uint32_t height, uint32_t* ids)
{
  FH_GROUP_LEAD(ctx);
  MCTX_CHECK(ctx);
  if (!camera || !ids || width == 0 || height == 0 || width > 32768 || height > 32768) return fail(ctx, FH_E_INVALID, "fh_primary_instances: bad argument");
  if (!ctx->scene_loaded || !ctx->bvh_valid) return fail(ctx, FH_E_INVALID, "fh_primary_instances: scene/BVH missing");
  return primary_instances_submit(ctx, camera, width, height, ids);
}

int fh_motion_from_transforms(uint32_t n, const float* o2w_prev, const float* w2o_prev, const float* o2w_cur, const float* w2o_cur, fh_motion* out)
{
  if (n == 0) return FH_OK;
  if (!o2w_prev || !w2o_prev || !o2w_cur || !w2o_cur || !out) return fail(nullptr, FH_E_INVALID, "fh_motion_from_transforms: null argument");
  for (uint32_t i = 0; i < n; ++i) motion_entry(o2w_prev + 12ull * i, w2o_prev + 12ull * i, o2w_cur + 12ull * i, w2o_cur + 12ull * i, out + i);
  return FH_OK;
}

// fh_denoise_temporal with the motion stage; every refusal is decided from the arguments alone (temporal_host.h, motion_host.h)
int fh_denoise_temporal_motion(fh_ctx* ctx, uint32_t width, uint32_t height, const fh_denoise_inputs* in, const fh_camera* camera, const fh_temporal_params* temporal,
                               const fh_denoise_params* params, const uint32_t* instance_ids, uint32_t n_instances, const fh_motion* motion, float* denoised, int upscale2x)
{
  const fh_denoise_params pr = params ? *params : kDenoiseDefaults;
  const fh_temporal_params tp = temporal ? *temporal : kTemporalDefaults;
  float w2c[12], inv_tan = 0.0f;
  bool any_moved = false;
  const char* why = temporal_refusal(width, height, in, camera, tp, pr, denoised, w2c, &inv_tan);
  if (!why) why = motion_refusal(instance_ids, n_instances, motion, &any_moved);
  if (!why && !ctx) why = "null context";
  if (why) return fail(ctx, FH_E_INVALID, std::string("fh_denoise_temporal_motion: ") + why);
  FH_GROUP_LEAD(ctx);
  MCTX_CHECK(ctx);
  return denoise_temporal_submit(ctx, (int)width, (int)height, in, camera, w2c, inv_tan, &tp, &pr, any_moved ? instance_ids : nullptr, n_instances, motion, denoised, upscale2x ? 1 : 0);
}

int fh_set_denoise_motion(fh_ctx* ctx, int on)
{
  FH_GROUP_EACH(ctx, kGroupCallPlain, fh_set_denoise_motion(m_, on));
  if (!ctx) return FH_E_INVALID;
  ctx->denoise_motion = on ? 1 : 0;
  if (!on) ctx->hist.forget_instances();
  return FH_OK;
}

int fh_get_denoise_motion(fh_ctx* ctx, int* on)
{
  FH_GROUP_LEAD(ctx);
  if (!ctx || !on) return FH_E_INVALID;
  *on = ctx->denoise_motion;
  return FH_OK;
}

}  // extern "C"
