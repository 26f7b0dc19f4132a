// fredholm/denoiser.h -- drop-in for the reference's Denoiser (fredholm/include/fredholm/denoiser.h:14-146), which wraps the proprietary OptiX
// AI denoiser (HDR model, albedo + normal guide layers, optional 2x upscaling model).  That network has no counterpart here; the class keeps the
// constructor / denoise() / wait_for_completion() surface the applications call (app/controller.cpp:70-78,232-236, app/rtcamp8.cpp:120-128,191-196)
// and runs the library's guided filter in its place: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) on albedo-demodulated
// radiance, steered by the same normal and albedo layers (fh_denoise).  Output size follows the reference: 2 x width by 2 x height when `upscale`.
// Beyond the reference: set_mode(Denoiser::Guided) runs the variance-guided filter (fh_denoise_guided) on the same layers plus whatever set_guides() was given --
// position and depth for the plane edge stop, the luminance moments and sample counts of adaptive sampling for the colour edge stop.  An application that is
// not edited gets it with the environment variable FH_DENOISER=guided (read by the constructor; set_mode wins).
// set_mode(Denoiser::Temporal) (FH_DENOISER=temporal) puts temporal accumulation in front of that filter (fh_denoise_temporal): it needs the position and depth
// guides and, before every denoise(), the camera the frame was rendered with (set_camera); the history lives in the context, reset_history() drops it.  Give the
// frames of a sequence samples of their own (Renderer::set_seed), or a still camera accumulates one image over and over.
// set_motion(true) (FH_DENOISER=temporal-motion: Temporal mode with it) switches the context's per-instance motion vectors on (fh_set_denoise_motion): the history of
// an instance that Renderer::set_time moved is looked up where the instance was.  The switch belongs to the context and is sent with the next denoise().
// set_response(true, gamma) (FH_DENOISER=temporal-response, temporal-motion-response) switches the context's history clipping on (fh_set_denoise_response): the
// history is clamped to the current frame's local colour box before the blend, so a change of lighting does not lag.  Sent with the next denoise() likewise.
// set_response_noise(true, kappa) (FH_DENOISER=temporal-response-noise, temporal-motion-response-noise: set_response(true) with it) switches the noise box of that
// clipping on (fh_set_denoise_response_noise).  It acts only in calls that are given luminance moments and sample counts (set_guides with both: they exist while
// adaptive sampling keeps them); without them, and without set_response, it does nothing.
// set_temporal_moments(true, min_history) switches the context's temporal moments on (fh_set_denoise_temporal_moments): the history also keeps the luminance moments,
// and a denoise() WITHOUT moments and counts takes its per-pixel variance from them once a pixel's history is min_history long.  The environment variable
// FH_DENOISE_TEMPORAL_MOMENTS does the same for an application that is not edited (unset or 0: off; 1: on with the default; any other number: on with that
// min_history); it acts in Temporal mode, whichever FH_DENOISER=temporal... spelling chose it.  Turning it on or off drops the history.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include <stdexcept>

#include "../cwl/util.h"
#include "camera.h"
#include "types.h"

namespace fredholm
{
class Denoiser
{
 public:
  Denoiser(fh_ctx* context, uint32_t width, uint32_t height, const float4* d_beauty, const float4* d_normal, const float4* d_albedo, const float4* d_denoised, bool upscale = false)
      : m_context(context), m_width(width), m_height(height), m_d_beauty(d_beauty), m_d_normal(d_normal), m_d_albedo(d_albedo), m_d_denoised(const_cast<float4*>(d_denoised)), m_upscale(upscale)
  {
    const char* env = std::getenv("FH_DENOISER");
    if (env && std::strcmp(env, "guided") == 0) m_mode = Guided;
    if (env && std::strcmp(env, "temporal") == 0) m_mode = Temporal;
    if (env && std::strcmp(env, "temporal-motion") == 0) { m_mode = Temporal; set_motion(true); }
    if (env && std::strcmp(env, "temporal-response") == 0) { m_mode = Temporal; set_response(true); }
    if (env && std::strcmp(env, "temporal-motion-response") == 0) { m_mode = Temporal; set_motion(true); set_response(true); }
    if (env && std::strcmp(env, "temporal-response-noise") == 0) { m_mode = Temporal; set_response(true); set_response_noise(true); }
    if (env && std::strcmp(env, "temporal-motion-response-noise") == 0) { m_mode = Temporal; set_motion(true); set_response(true); set_response_noise(true); }
    const char* mom = std::getenv("FH_DENOISE_TEMPORAL_MOMENTS");
    if (mom && *mom && std::strcmp(mom, "0") != 0) {
      if (std::strcmp(mom, "1") == 0) set_temporal_moments(true);
      else set_temporal_moments(true, float(std::atof(mom)));
    }
  }
  enum Mode { Atrous, Guided, Temporal };
  void set_mode(Mode mode) { m_mode = mode; }
  Mode mode() const { return m_mode; }
  // device pointers of width * height elements; position and depth go together, moments and counts go together, either pair may be null
  void set_guides(const float4* d_position, const float* d_depth, const float2* d_moments = nullptr, const uint32_t* d_counts = nullptr)
  {
    m_d_position = d_position; m_d_depth = d_depth; m_d_moments = d_moments; m_d_counts = d_counts;
  }
  // Temporal mode: the camera the layers were rendered with (what Renderer::render was given; for a scene with a camera of its own, Renderer::camera_params)
  void set_camera(const Camera& camera) { set_camera(camera.to_c()); }
  void set_camera(const fh_camera& camera) { m_camera = camera; m_has_camera = true; }
  void set_temporal_params(float alpha_min, float max_history, float normal_cos_min, float plane_tol)
  {
    m_temporal = fh_temporal_params{alpha_min, max_history, normal_cos_min, plane_tol};
    m_has_temporal = true;
  }
  // Temporal mode: carry the history of moved instances (fh_set_denoise_motion); takes effect with the next denoise()
  void set_motion(bool on) { m_motion = on; m_motion_pending = true; }
  bool motion() const { return m_motion; }
  // Temporal mode: clip the history to the current frame's colour box (fh_set_denoise_response); takes effect with the next denoise()
  void set_response(bool on, float gamma = 1.0f) { m_response = on; m_response_gamma = gamma; m_response_pending = true; }
  bool response() const { return m_response; }
  float response_gamma() const { return m_response_gamma; }
  // Temporal mode with set_response: clamp the clipped history to the pixel's measured noise too (fh_set_denoise_response_noise); needs moments; with the next denoise()
  void set_response_noise(bool on, float kappa = 6.0f) { m_noise = on; m_noise_kappa = kappa; m_noise_pending = true; }
  bool response_noise() const { return m_noise; }
  float response_noise_kappa() const { return m_noise_kappa; }
  // Temporal mode: keep the luminance moments in the history and take the variance of a call without sample moments from them (fh_set_denoise_temporal_moments);
  // takes effect with the next denoise(), and a change of `on` drops the history
  void set_temporal_moments(bool on, float min_history = 2.0f) { m_moments = on; m_moments_min_history = min_history; m_moments_pending = true; }
  bool temporal_moments() const { return m_moments; }
  float temporal_moments_min_history() const { return m_moments_min_history; }
  void reset_history()
  {
    fh_ctx* ctx = m_context ? m_context : cwl::require_context();
    cwl::check(ctx, fh_denoise_history_reset(ctx), "fh_denoise_history_reset");
  }
  void denoise()
  {
    fh_ctx* ctx = m_context ? m_context : cwl::require_context();
    if (m_mode == Temporal) {
      if (!m_has_camera) throw std::runtime_error("Denoiser: Temporal mode needs set_camera() before denoise()");
      if (m_motion_pending) {
        cwl::check(ctx, fh_set_denoise_motion(ctx, m_motion ? 1 : 0), "fh_set_denoise_motion");
        m_motion_pending = false;
      }
      if (m_response_pending) {
        const fh_response_params rp = {m_response_gamma};
        cwl::check(ctx, fh_set_denoise_response(ctx, m_response ? &rp : nullptr), "fh_set_denoise_response");
        m_response_pending = false;
      }
      if (m_noise_pending) {
        const fh_response_noise_params np = {m_noise_kappa};
        cwl::check(ctx, fh_set_denoise_response_noise(ctx, m_noise ? &np : nullptr), "fh_set_denoise_response_noise");
        m_noise_pending = false;
      }
      if (m_moments_pending) {
        const fh_temporal_moments_params mp = {m_moments_min_history};
        cwl::check(ctx, fh_set_denoise_temporal_moments(ctx, m_moments ? &mp : nullptr), "fh_set_denoise_temporal_moments");
        m_moments_pending = false;
      }
      const fh_denoise_inputs in = {reinterpret_cast<const float*>(m_d_beauty), reinterpret_cast<const float*>(m_d_normal), reinterpret_cast<const float*>(m_d_albedo),
                                    reinterpret_cast<const float*>(m_d_position), m_d_depth, reinterpret_cast<const float*>(m_d_moments), m_d_counts};
      cwl::check(ctx, fh_denoise_temporal(ctx, m_width, m_height, &in, &m_camera, m_has_temporal ? &m_temporal : nullptr, nullptr, reinterpret_cast<float*>(m_d_denoised), m_upscale ? 1 : 0),
                 "fh_denoise_temporal");
      return;
    }
    if (m_mode == Guided) {
      const fh_denoise_inputs in = {reinterpret_cast<const float*>(m_d_beauty), reinterpret_cast<const float*>(m_d_normal), reinterpret_cast<const float*>(m_d_albedo),
                                    reinterpret_cast<const float*>(m_d_position), m_d_depth, reinterpret_cast<const float*>(m_d_moments), m_d_counts};
      cwl::check(ctx, fh_denoise_guided(ctx, m_width, m_height, &in, nullptr, reinterpret_cast<float*>(m_d_denoised), m_upscale ? 1 : 0), "fh_denoise_guided");
      return;
    }
    cwl::check(ctx, fh_denoise(ctx, m_width, m_height, reinterpret_cast<const float*>(m_d_beauty), reinterpret_cast<const float*>(m_d_normal), reinterpret_cast<const float*>(m_d_albedo),
                               reinterpret_cast<float*>(m_d_denoised), m_upscale ? 1 : 0),
               "fh_denoise");
  }
  void wait_for_completion() const { CUDA_SYNC_CHECK(); }

 private:
  fh_ctx* m_context;
  uint32_t m_width, m_height;
  const float4* m_d_beauty;
  const float4* m_d_normal;
  const float4* m_d_albedo;
  float4* m_d_denoised;
  bool m_upscale;
  Mode m_mode = Atrous;
  const float4* m_d_position = nullptr;
  const float* m_d_depth = nullptr;
  const float2* m_d_moments = nullptr;
  const uint32_t* m_d_counts = nullptr;
  fh_camera m_camera{};
  fh_temporal_params m_temporal{};
  bool m_has_camera = false, m_has_temporal = false;
  bool m_motion = false, m_motion_pending = false;
  bool m_response = false, m_response_pending = false;
  float m_response_gamma = 1.0f;
  bool m_noise = false, m_noise_pending = false;
  float m_noise_kappa = 6.0f;
  bool m_moments = false, m_moments_pending = false;
  float m_moments_min_history = 2.0f;
};
}  // namespace fredholm
