// skin_host.cpp -- csrc/fh_skin.h on the host, for tests/test_skinning_host.py (compiled there with the address and undefined-behaviour sanitizers).
// reads:  n_joints, the palette (12 floats per joint), n, then per-vertex arrays one after the other: joints (4 uint16), weights (4 floats), positions (3), normals (3)
// writes: the posed positions (3 floats per vertex), then the posed normals
#include <cstdint>
#include <cstdio>
#include <vector>

#include "fh_skin.h"

int main(int argc, char** argv)
{
  if (argc != 3) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) return 2;
  uint32_t nj = 0, n = 0;
  if (std::fread(&nj, 4, 1, in) != 1 || nj == 0) return 2;
  std::vector<float> palette(12 * (size_t)nj);
  if (std::fread(palette.data(), 4, palette.size(), in) != palette.size()) return 2;
  if (std::fread(&n, 4, 1, in) != 1) return 2;
  std::vector<uint16_t> joints(4 * (size_t)n);
  std::vector<float> weights(4 * (size_t)n), p(3 * (size_t)n), nrm(3 * (size_t)n), po(3 * (size_t)n), no(3 * (size_t)n);
  if (std::fread(joints.data(), 2, joints.size(), in) != joints.size() || std::fread(weights.data(), 4, weights.size(), in) != weights.size() ||
      std::fread(p.data(), 4, p.size(), in) != p.size() || std::fread(nrm.data(), 4, nrm.size(), in) != nrm.size())
    return 2;
  for (size_t v = 0; v < n; ++v) fh::skin_vertex(palette.data(), &joints[4 * v], &weights[4 * v], &p[3 * v], &nrm[3 * v], &po[3 * v], &no[3 * v]);
  std::fwrite(po.data(), 4, po.size(), out);
  std::fwrite(no.data(), 4, no.size(), out);
  std::fclose(in);
  std::fclose(out);
  return 0;
}
