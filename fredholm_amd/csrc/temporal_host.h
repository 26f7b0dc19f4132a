// temporal_host.h -- the host-only part of fh_denoise_temporal (include/fredholm_hip.h): the refusals, which are decided from the arguments alone, the
// inversion of the camera, and the plan of a call: what becomes of the history, which of the twenty k_temporal a call launches (temporal_call_plan) and whether the
// context feeds itself a motion table (temporal_feed_plan).  Plain C++ without HIP, so that it also compiles into a stand-alone program
// (tools/temporal_host_check.cpp) for the host sanitizers.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/fredholm_hip.h"

namespace fh {

constexpr fh_denoise_params kDenoiseDefaults = {2.0f, 1.0f, 0.2f, 7u, 5u};  // what a null fh_denoise_params means (the header states them)
constexpr fh_temporal_params kTemporalDefaults = {0.2f, 32.0f, 0.5f, 0.02f};  // ... and a null fh_temporal_params

// why fh_denoise_guided refuses these arguments, or nullptr (the context is not looked at)
inline const char* guided_refusal(uint32_t width, uint32_t height, const fh_denoise_inputs* in, const fh_denoise_params& pr, const float* denoised)
{
  auto bad_sigma = [](float s) { return !(s > 0.0f) || !std::isfinite(s); };
  if (!in || !denoised) return "null argument";
  if (!in->beauty || !in->normal || !in->albedo) return "the beauty, normal and albedo layers are required";
  if ((in->position == nullptr) != (in->depth == nullptr)) return "position and depth are given together or not at all";
  if ((in->moments == nullptr) != (in->counts == nullptr)) return "moments and counts are given together or not at all";
  if (width == 0 || height == 0 || width > 32768 || height > 32768) return "width and height must be in 1..32768";
  if (bad_sigma(pr.sigma_l) || bad_sigma(pr.sigma_z) || bad_sigma(pr.sigma_a)) return "sigma_l, sigma_z and sigma_a must be finite and > 0";
  if (pr.normal_power_log2 > 10) return "normal_power_log2 must be at most 10";
  if (pr.passes < 1 || pr.passes > 6) return "passes must be in 1..6";
  return nullptr;
}

// world-to-camera rows of a camera-to-world 3x4, by the cofactor formula of the header: in double, rounded once to float.  False: not invertible.
inline bool camera_world_to_camera(const float t[12], float out[12])
{  // (compiled with -ffp-contract=off like everything here: the numpy restatement of the tests reproduces these doubles)
  const double R00 = t[0], R01 = t[1], R02 = t[2], R10 = t[4], R11 = t[5], R12 = t[6], R20 = t[8], R21 = t[9], R22 = t[10];
  const double T[3] = {t[3], t[7], t[11]};
  const double Cf[3][3] = {{R11 * R22 - R12 * R21, R02 * R21 - R01 * R22, R01 * R12 - R02 * R11},
                           {R12 * R20 - R10 * R22, R00 * R22 - R02 * R20, R02 * R10 - R00 * R12},
                           {R10 * R21 - R11 * R20, R01 * R20 - R00 * R21, R00 * R11 - R01 * R10}};
  const double det = (R00 * Cf[0][0] + R01 * Cf[1][0]) + R02 * Cf[2][0];
  if (!(det != 0.0) || !std::isfinite(det)) return false;
  for (int i = 0; i < 3; ++i) {
    const double m0 = Cf[i][0] / det, m1 = Cf[i][1] / det, m2 = Cf[i][2] / det;
    const double m3 = -((m0 * T[0] + m1 * T[1]) + m2 * T[2]);
    out[4 * i] = (float)m0; out[4 * i + 1] = (float)m1; out[4 * i + 2] = (float)m2; out[4 * i + 3] = (float)m3;
    for (int j = 0; j < 4; ++j)
      if (!std::isfinite(out[4 * i + j])) return false;
  }
  return true;
}

// why fh_denoise_temporal refuses these arguments, or nullptr; on acceptance w2c and *inv_tan hold the inverted camera and its cam_inv_tan
inline const char* temporal_refusal(uint32_t width, uint32_t height, const fh_denoise_inputs* in, const fh_camera* camera, const fh_temporal_params& tp, const fh_denoise_params& pr,
                                    const float* denoised, float w2c[12], float* inv_tan)
{
  if (const char* why = guided_refusal(width, height, in, pr, denoised)) return why;
  if (!camera) return "null camera";
  if (!in->position) return "the position and depth layers are required";
  if (!(tp.alpha_min >= 0.0f && tp.alpha_min <= 1.0f)) return "alpha_min must be in [0, 1]";
  if (!(tp.max_history >= 1.0f) || !std::isfinite(tp.max_history)) return "max_history must be finite and >= 1";
  if (!(tp.normal_cos_min > -1.0f && tp.normal_cos_min <= 1.0f)) return "normal_cos_min must be in (-1, 1]";
  if (!(tp.plane_tol > 0.0f) || !std::isfinite(tp.plane_tol)) return "plane_tol must be finite and > 0";
  *inv_tan = 1.0f / tanf(0.5f * camera->fov);  // render.hip: cam_inv_tan
  if (!(*inv_tan > 0.0f) || !std::isfinite(*inv_tan)) return "the camera's fov gives no finite focal length";
  if (!camera_world_to_camera(camera->transform, w2c)) return "the camera's transform cannot be inverted";
  return nullptr;
}

// why fh_set_denoise_response refuses these parameters, or nullptr (NULL parameters switch the mode off and are never refused)
inline const char* response_refusal(const fh_response_params* params)
{
  if (params && (!(params->gamma > 0.0f) || !std::isfinite(params->gamma))) return "gamma must be finite and > 0";
  return nullptr;
}

// why fh_set_denoise_response_noise refuses these parameters, or nullptr (NULL parameters switch the step off and are never refused)
inline const char* response_noise_refusal(const fh_response_noise_params* params)
{
  if (params && (!(params->kappa > 0.0f) || !std::isfinite(params->kappa))) return "kappa must be finite and > 0";
  return nullptr;
}

// why fh_set_denoise_temporal_moments refuses these parameters, or nullptr (NULL parameters switch it off and are never refused)
inline const char* temporal_moments_refusal(const fh_temporal_moments_params* params)
{
  if (params && (!(params->min_history >= 1.0f) || !std::isfinite(params->min_history))) return "min_history must be finite and >= 1";
  return nullptr;
}

// ---- the plan of a call (denoise.hip: denoise_temporal_submit, temporal_feed_motion) ----

enum { kLookNone, kLookOwn, kLookReproject, kLookMotion };  // LOOK: there is no history; the camera stood still; it moved; fh_denoise_temporal_motion with a moved instance
enum { kClipOff, kClipColour, kClipColourNoise };          // CLIP: fh_set_denoise_response off; on; on with fh_set_denoise_response_noise and moments

// which buffers of the history a call of px pixels allocates anew: the main six where they are too small, the moment image of fh_set_denoise_temporal_moments where it is
// smaller than the rest of the history will be (a new buffer holds nothing: either grow drops the history).  Stated here for the plan and for the record that acts on it
// (context.h: TemporalHistory::ensure).
struct TemporalGrow { bool main, moments; };
inline TemporalGrow temporal_grow(size_t capacity, size_t moment_capacity, size_t px, bool with_moments)
{
  const bool main = capacity < px;
  return {main, with_moments && moment_capacity < (main ? px : capacity)};
}

struct TemporalHistoryFacts {
  uint32_t frames, w, h;             // frames = 0: there is no history
  size_t capacity, moment_capacity;  // pixels the main buffers / the moment image have room for
  bool same_camera;                  // the call's camera equals the history's, byte for byte
};
struct TemporalCallFacts { uint32_t w, h; bool has_ids, has_sample_moments; };  // has_ids: an id plane and a motion table of which at least one entry has moved
struct TemporalSwitches { bool response, response_noise, temporal_moments; };  // fh_set_denoise_response, _response_noise, _temporal_moments
struct TemporalCallPlan {
  bool grow_main, grow_moments;  // temporal_grow
  bool history_kept;             // the call looks its history up; false: it starts one
  bool with_motion;              // the motion table is uploaded
  int look, clip;                // k_temporal<look, clip, mom>; kLookNone goes with kClipOff only
  bool mom, replace_v;           // replace_v: the variance comes from the history's moments where it is long enough
  bool still;                    // same_camera as the kernel is told (kLookMotion: the pixels of unmoved instances look up their own place)
};
inline TemporalCallPlan temporal_call_plan(const TemporalHistoryFacts& hist, const TemporalCallFacts& call, const TemporalSwitches& on)
{
  TemporalCallPlan p{};
  const TemporalGrow grow = temporal_grow(hist.capacity, hist.moment_capacity, (size_t)call.w * call.h, on.temporal_moments);
  p.grow_main = grow.main; p.grow_moments = grow.moments;
  // growing drops the history; so does any other change of width x height
  p.history_kept = hist.frames != 0 && !grow.main && !grow.moments && hist.w == call.w && hist.h == call.h;
  p.with_motion = call.has_ids && p.history_kept;  // (without a history nothing is looked up: the plain first call)
  p.still = hist.same_camera;
  p.look = !p.history_kept ? kLookNone : p.with_motion ? kLookMotion : p.still ? kLookOwn : kLookReproject;
  // fh_set_denoise_response clips whatever history the call looks up; fh_set_denoise_response_noise adds its step only with moments (the measured variance exists only then)
  p.clip = p.look == kLookNone || !on.response ? kClipOff : on.response_noise && call.has_sample_moments ? kClipColourNoise : kClipColour;
  p.mom = on.temporal_moments; p.replace_v = p.mom && !call.has_sample_moments;
  return p;
}

// fh_denoise_temporal under fh_set_denoise_motion: the history is kept with the instance matrices it was written under (hist_*; empty: no snapshot), and where they differ
// from the context's (h_*) the call carries the moved instances' pixels itself.  alive: there is a history at the call's size.  refusal: why the call is refused, or nullptr
struct TemporalFeedPlan { bool feed_motion; const char* refusal; };
inline TemporalFeedPlan temporal_feed_plan(bool denoise_motion, bool alive, const std::vector<float>& hist_o2w, const std::vector<float>& hist_w2o, const std::vector<float>& h_o2w,
                                           const std::vector<float>& h_w2o, bool tree_built)
{
  const size_t nf = h_o2w.size();
  const bool moved = denoise_motion && alive && nf != 0 && hist_o2w.size() == nf && hist_w2o.size() == nf && h_w2o.size() == nf &&
                     (std::memcmp(hist_o2w.data(), h_o2w.data(), nf * sizeof(float)) != 0 || std::memcmp(hist_w2o.data(), h_w2o.data(), nf * sizeof(float)) != 0);
  if (!moved) return {false, nullptr};
  if (!tree_built) return {false, "instances moved and the BVH has not been built (fh_set_denoise_motion)"};
  return {true, nullptr};
}

}  // namespace fh
