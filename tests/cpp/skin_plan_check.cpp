// skin_plan_check.cpp -- csrc/skin_plan_host.h as a stand-alone program, for tests/test_skinning_host.py: no GPU, no library.
// reads cases until the file ends and prints one line per case: the refusal's message, or "ok".  A case is
//   kind (0: fh_set_skin, 1: fh_set_joint_matrices), then the facts: scene_loaded, n_vertices, n_joints (uint32 each), then
//   kind 0: desc given, desc.n_vertices, desc.n_joints, joints given, weights given, k, then 4 k uint16 and 4 k floats
//   kind 1: n, matrices given, k, then 12 k floats
#include <cstdint>
#include <cstdio>
#include <vector>

#include "skin_plan_host.h"

static bool rd(FILE* f, uint32_t* v) { return std::fread(v, 4, 1, f) == 1; }

int main(int argc, char** argv)
{
  if (argc != 2) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  uint32_t kind;
  while (rd(in, &kind)) {
    uint32_t loaded, nv, nj;
    if (!rd(in, &loaded) || !rd(in, &nv) || !rd(in, &nj)) return 2;
    const fh::SkinFacts facts = {loaded != 0, nv, nj};
    const char* why = nullptr;
    if (kind == 0) {
      uint32_t given, dnv, dnj, jgiven, wgiven, k;
      if (!rd(in, &given) || !rd(in, &dnv) || !rd(in, &dnj) || !rd(in, &jgiven) || !rd(in, &wgiven) || !rd(in, &k)) return 2;
      std::vector<uint16_t> joints(4 * (size_t)k);
      std::vector<float> weights(4 * (size_t)k);
      if (std::fread(joints.data(), 2, joints.size(), in) != joints.size() || std::fread(weights.data(), 4, weights.size(), in) != weights.size()) return 2;
      const fh_skin_desc d = {dnv, dnj, jgiven ? joints.data() : nullptr, wgiven ? weights.data() : nullptr};
      why = fh::skin_refusal(facts, given ? &d : nullptr);
      if (!why && given) std::printf("ok %u\n", fh::skin_count_skinned(d));
      else std::printf("%s\n", why ? why : "ok");
    } else {
      uint32_t n, given, k;
      if (!rd(in, &n) || !rd(in, &given) || !rd(in, &k)) return 2;
      std::vector<float> m(12 * (size_t)k);
      if (std::fread(m.data(), 4, m.size(), in) != m.size()) return 2;
      why = fh::joint_matrices_refusal(facts, n, given ? m.data() : nullptr);
      std::printf("%s\n", why ? why : "ok");
    }
  }
  std::fclose(in);
  return 0;
}
