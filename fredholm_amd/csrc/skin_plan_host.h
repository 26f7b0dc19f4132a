// skin_plan_host.h -- every refusal of fh_set_skin and fh_set_joint_matrices (scene.hip), as pure functions of the caller's arguments and of plain values of the
// context: a message, or null for arguments the call accepts.  Decided before the context or the device is touched, so a refused call changes nothing.  Plain C++
// without HIP like scene_plan_host.h, so that it also compiles into a stand-alone program for the tests and the host sanitizers.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/fredholm_hip.h"

namespace fh {

constexpr uint32_t kSkinMaxJoints = 65536;  // a joint index is a uint16

// what the two calls need to know of the context
struct SkinFacts {
  bool scene_loaded;
  uint32_t n_vertices;  // of the uploaded scene
  uint32_t n_joints;    // of the skin that is set; 0: none
};

inline bool skin_vertex_unskinned(const float* w) { return w[0] == 0.0f && w[1] == 0.0f && w[2] == 0.0f && w[3] == 0.0f; }

// desc != null (null clears the skin and is never refused on a context with a scene)
inline const char* skin_refusal(const SkinFacts& f, const fh_skin_desc* d)
{
  if (!f.scene_loaded) return "fh_set_skin: no scene loaded";
  if (!d) return nullptr;
  if (d->n_vertices != f.n_vertices) return "fh_set_skin: n_vertices differs from the uploaded scene's";
  if (!d->joints || !d->weights) return "fh_set_skin: null arrays";
  if (d->n_joints == 0 || d->n_joints > kSkinMaxJoints) return "fh_set_skin: n_joints must be in [1, 65536]";
  for (size_t v = 0; v < d->n_vertices; ++v) {
    const float* w = d->weights + 4 * v;
    for (int k = 0; k < 4; ++k)
      if (!std::isfinite(w[k])) return "fh_set_skin: a weight is not finite";
    if (skin_vertex_unskinned(w)) continue;
    for (int k = 0; k < 4; ++k)
      if (d->joints[4 * v + k] >= d->n_joints) return "fh_set_skin: a joint index of a weighted vertex is outside the palette";
  }
  return nullptr;
}

// vertices with a non-zero weight (fh_get_skin_info)
inline uint32_t skin_count_skinned(const fh_skin_desc& d)
{
  uint32_t n = 0;
  for (size_t v = 0; v < d.n_vertices; ++v) n += skin_vertex_unskinned(d.weights + 4 * v) ? 0u : 1u;
  return n;
}

inline const char* joint_matrices_refusal(const SkinFacts& f, uint32_t n, const float* m3x4)
{
  if (!f.scene_loaded) return "fh_set_joint_matrices: no scene loaded";
  if (f.n_joints == 0) return "fh_set_joint_matrices: no skin set";
  if (!m3x4) return "fh_set_joint_matrices: null arrays";
  if (n != f.n_joints) return "fh_set_joint_matrices: the matrix count differs from the skin's n_joints";
  for (size_t k = 0; k < 12 * (size_t)n; ++k)
    if (!std::isfinite(m3x4[k])) return "fh_set_joint_matrices: a matrix entry is not finite";
  return nullptr;
}

}  // namespace fh
