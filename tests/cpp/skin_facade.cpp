// test helper: fredholm::Renderer::load_scene + set_time on a skinned model file, for tests/test_gpu_skinning.py
//   skin_facade out.bin file time1 [time2 ...]
// writes, after the load and after every set_time, the posed vertices and normals fh_get_posed_geometry gives (3 floats per vertex each)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fredholm/renderer.h"
#include "optwl/optwl.h"

int main(int argc, char** argv)
{
  if (argc < 3) return 2;
  try {
    optwl::Context context;
    fredholm::Renderer renderer(context.get_context());
    renderer.load_scene(argv[2]);
    fredholm::Scene scene;  // (the facade keeps its scene to itself: the vertex count comes from a second load)
    scene.load_model(argv[2], true);
    const size_t n_vertices = scene.m_vertices.size();
    renderer.build_ias();
    std::FILE* f = std::fopen(argv[1], "wb");
    if (!f) return 3;
    uint32_t n_joints = 0, n_skinned = 0;
    int posed = 0;
    for (int i = 2; i < argc; ++i) {
      if (i > 2) renderer.set_time(float(std::atof(argv[i])));
      if (fh_get_skin_info(context.get_context(), &n_joints, &n_skinned, &posed) != FH_OK || !posed) return 4;
      std::vector<float> pv(3 * n_vertices), pn(pv.size());
      if (fh_get_posed_geometry(context.get_context(), pv.data(), pn.data()) != FH_OK) return 5;
      std::fwrite(pv.data(), 4, pv.size(), f);
      std::fwrite(pn.data(), 4, pn.size(), f);
    }
    std::fclose(f);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
