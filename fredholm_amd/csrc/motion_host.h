// motion_host.h -- the host-only part of the per-instance motion vectors (include/fredholm_hip.h: fh_motion_from_transforms, fh_denoise_temporal_motion): the
// motion table from two sets of instance matrices, the refusals, and the two per-frame constants of the chief ray.  Plain C++ without HIP like temporal_host.h,
// so that it also compiles into a stand-alone program for the host sanitizers.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "temporal_host.h"

namespace fh {

// one entry of the table, by the header's formulas: in double, rounded once (compiled with -ffp-contract=off: the numpy restatement reproduces these doubles)
inline void motion_entry(const float* o2w_prev, const float* w2o_prev, const float* o2w_cur, const float* w2o_cur, fh_motion* out)
{
  out->moved = (std::memcmp(o2w_prev, o2w_cur, 48) != 0 || std::memcmp(w2o_prev, w2o_cur, 48) != 0) ? 1u : 0u;
  const float *A = o2w_prev, *B = w2o_cur, *Cc = o2w_cur, *D = w2o_prev;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) {
      double s = ((double)A[4 * i] * (double)B[j] + (double)A[4 * i + 1] * (double)B[4 + j]) + (double)A[4 * i + 2] * (double)B[8 + j];
      if (j == 3) s = s + (double)A[4 * i + 3];
      out->point[4 * i + j] = (float)s;
    }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      out->normal[3 * i + j] = (float)(((double)Cc[4 * j] * (double)D[i] + (double)Cc[4 * j + 1] * (double)D[4 + i]) + (double)Cc[4 * j + 2] * (double)D[8 + i]);
}

inline bool motion_finite(const fh_motion& m)
{
  for (float v : m.point)
    if (!std::isfinite(v)) return false;
  for (float v : m.normal)
    if (!std::isfinite(v)) return false;
  return true;
}

// why fh_denoise_temporal_motion refuses its three own arguments, or nullptr; *any_moved: an entry has `moved` set
inline const char* motion_refusal(const uint32_t* instance_ids, uint32_t n_instances, const fh_motion* motion, bool* any_moved)
{
  *any_moved = false;
  if ((instance_ids == nullptr) != (motion == nullptr)) return "instance_ids and motion are given together or not at all";
  if (n_instances == 0 && instance_ids) return "n_instances is 0";
  if (!motion) return nullptr;
  for (uint32_t i = 0; i < n_instances; ++i) {
    if (!motion_finite(motion[i])) return "a motion entry is not finite";
    if (motion[i].moved) *any_moved = true;
  }
  return nullptr;
}

// a + b of the thin lens (render.hip: cam_a_plus_b), in fp32 operation by operation (volatile: no contraction, no double-precision intermediates)
inline float chief_a_plus_b(float inv_tan, float focus)
{
  volatile float f = inv_tan, b = focus;
  volatile float inv_b = 1.0f / b;
  volatile float den = 1.0f + f;
  den = den - inv_b;
  volatile float a = 1.0f / den;
  volatile float apb = a + b;
  return apb;
}

}  // namespace fh
