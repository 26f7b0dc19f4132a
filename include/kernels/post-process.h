// kernels/post-process.h -- PostProcessParams + post_process_kernel_launch with the reference's signature
// (fredholm/kernels/include/kernels/post-process.h:4-10, :126-128), forwarding to fh_post_process.
// Beyond the reference: auto-exposure (fh_set_auto_exposure) and local exposure (fh_set_local_exposure), switches on the process-wide context, so
// post_process_kernel_launch keeps its signature.
#pragma once
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

#include "../cwl/util.h"
#include "../fredholm/types.h"

struct PostProcessParams {
  bool use_bloom;
  float bloom_threshold;
  float bloom_sigma;
  float ISO;
  float chromatic_aberration;
};

// fh_auto_exposure_params with the library's defaults
struct AutoExposureParams {
  float key = 0.18f;
  float compensation_ev = 0.0f;
  float min_ev = -16.0f, max_ev = 16.0f;
  float low = 0.10f, high = 0.90f;
  float speed_up = 3.0f, speed_down = 1.0f;
  float frame_time = 1.0f / 30.0f;  // seconds per post_process_kernel_launch; infinity: no adaptation
  float log2_lo = -16.0f, log2_hi = 16.0f;
  bool bloom_relative = false;      // FH_AE_BLOOM_RELATIVE
};

// fh_local_exposure_params with the library's defaults
struct LocalExposureParams {
  float highlights = 0.5f, shadows = 0.5f;  // share of the base layer's distance above / below the pivot that is removed
  float pivot = 0.18f;
  float max_stops = 4.0f;
  float sigma_range = 1.0f;
  uint32_t passes = 4;
};

namespace fh_post_detail
{
// the same for FH_LOCAL_EXPOSURE
inline bool& local_exposure_decided()
{
  static bool decided = false;
  return decided;
}
// the environment variable FH_AUTO_EXPOSURE has been looked at, or the application has set the switch itself (which wins)
inline bool& auto_exposure_decided()
{
  static bool decided = false;
  return decided;
}
}  // namespace fh_post_detail

// nullptr: off.  Throws what fh_set_auto_exposure refuses
inline void set_auto_exposure(const AutoExposureParams* params)
{
  fh_post_detail::auto_exposure_decided() = true;
  fh_ctx* ctx = cwl::require_context();
  if (!params) { cwl::check(ctx, fh_set_auto_exposure(ctx, nullptr), "fh_set_auto_exposure"); return; }
  const fh_auto_exposure_params p{params->key, params->compensation_ev, params->min_ev, params->max_ev, params->low, params->high, params->speed_up, params->speed_down,
                                  params->frame_time, params->log2_lo, params->log2_hi, params->bloom_relative ? FH_AE_BLOOM_RELATIVE : 0u};
  cwl::check(ctx, fh_set_auto_exposure(ctx, &p), "fh_set_auto_exposure");
}
inline fh_auto_exposure_state get_auto_exposure_state()
{
  fh_ctx* ctx = cwl::require_context();
  fh_auto_exposure_state s{};
  cwl::check(ctx, fh_get_auto_exposure_state(ctx, &s), "fh_get_auto_exposure_state");
  return s;
}
inline void reset_auto_exposure()
{
  fh_ctx* ctx = cwl::require_context();
  cwl::check(ctx, fh_auto_exposure_reset(ctx), "fh_auto_exposure_reset");
}

// A weak reference: a program that brings entry points of its own from before this switch (stubs under a test) still links, and asking for the switch there throws
extern "C" int fh_set_local_exposure(fh_ctx* ctx, const fh_local_exposure_params* params) __attribute__((weak));

// nullptr: off.  Throws what fh_set_local_exposure refuses
inline void set_local_exposure(const LocalExposureParams* params)
{
  fh_post_detail::local_exposure_decided() = true;
  if (!fh_set_local_exposure) throw std::runtime_error("fh_set_local_exposure: not in the library this program is linked with");
  fh_ctx* ctx = cwl::require_context();
  if (!params) { cwl::check(ctx, fh_set_local_exposure(ctx, nullptr), "fh_set_local_exposure"); return; }
  const fh_local_exposure_params p{params->highlights, params->shadows, params->pivot, params->max_stops, params->sigma_range, params->passes};
  cwl::check(ctx, fh_set_local_exposure(ctx, &p), "fh_set_local_exposure");
}

inline void post_process_kernel_launch(const float4* beauty_in, float4* beauty_high_luminance, float4* beauty_temp, int width, int height, const PostProcessParams& params,
                                       float4* beauty_out)
{
  fh_post_params p{params.use_bloom ? 1 : 0, params.bloom_threshold, params.bloom_sigma, params.ISO, params.chromatic_aberration};
  fh_ctx* ctx = cwl::require_context();
  // FH_AUTO_EXPOSURE, read once, gives applications that know nothing of the switch the feature (as FH_DENOISER does for the denoiser): "1" = the defaults,
  // any other number = that key, "0" or unset = off
  if (!fh_post_detail::auto_exposure_decided()) {
    fh_post_detail::auto_exposure_decided() = true;
    if (const char* e = std::getenv("FH_AUTO_EXPOSURE")) {
      char* end = nullptr;
      const float v = std::strtof(e, &end);
      if (end == e || *end != '\0') throw std::runtime_error(std::string("FH_AUTO_EXPOSURE: \"") + e + "\" is neither 1 (the defaults) nor a key such as 0.18");
      if (v != 0.0f) {
        AutoExposureParams ae;
        if (std::strcmp(e, "1") != 0) ae.key = v;
        set_auto_exposure(&ae);
      }
    }
  }
  // FH_LOCAL_EXPOSURE likewise: "1" = the defaults, any other number = that share for both highlights and shadows, "0" or unset = off
  if (!fh_post_detail::local_exposure_decided()) {
    fh_post_detail::local_exposure_decided() = true;
    if (const char* e = std::getenv("FH_LOCAL_EXPOSURE")) {
      char* end = nullptr;
      const float v = std::strtof(e, &end);
      if (end == e || *end != '\0') throw std::runtime_error(std::string("FH_LOCAL_EXPOSURE: \"") + e + "\" is neither 1 (the defaults) nor a share such as 0.5");
      if (v != 0.0f) {
        LocalExposureParams lx;
        if (std::strcmp(e, "1") != 0) lx.highlights = lx.shadows = v;
        set_local_exposure(&lx);
      }
    }
  }
  cwl::check(ctx, fh_post_process(ctx, reinterpret_cast<const float*>(beauty_in), reinterpret_cast<float*>(beauty_high_luminance), reinterpret_cast<float*>(beauty_temp), width, height, &p,
                                  reinterpret_cast<float*>(beauty_out)),
             "fh_post_process");
}
