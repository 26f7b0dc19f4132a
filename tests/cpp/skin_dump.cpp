// test helper: load a model file with the drop-in fredholm::Scene and dump what its skins yield
//   skin_dump out.bin file time1 [time2 ...]
// chunks: joints, weights, palette bases, then per time the palette of joint_matrices_3x4() and the two instance-transform arrays after update_animation(time)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fredholm/scene.h"

template <typename T>
static void put(std::FILE* f, const std::vector<T>& v)
{
  const unsigned long long n = v.size() * sizeof(T);
  std::fwrite(&n, sizeof n, 1, f);
  if (n) std::fwrite(v.data(), 1, n, f);
}

int main(int argc, char** argv)
{
  if (argc < 3) return 2;
  try {
    fredholm::Scene scene;
    scene.load_model(argv[2], true);
    std::FILE* f = std::fopen(argv[1], "wb");
    if (!f) return 3;
    put(f, scene.m_joints); put(f, scene.m_weights);
    std::vector<unsigned> bases;
    for (const auto& sk : scene.m_skins) { bases.push_back(sk.base); bases.push_back(unsigned(sk.joints.size())); }
    put(f, bases);
    for (int i = 3; i < argc; ++i) {
      scene.update_animation(float(std::atof(argv[i])));
      put(f, scene.joint_matrices_3x4());
      std::vector<float> o2w, w2o;
      scene.transforms_3x4(o2w, w2o);
      put(f, o2w); put(f, w2o);
    }
    std::fclose(f);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
