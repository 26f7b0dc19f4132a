// tools/temporal_host_check.cpp -- the host-only part of fh_denoise_temporal (fredholm_amd/csrc/temporal_host.h: the refusals and the camera inversion) as a
// stand-alone program, for the host sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/temporal_host_check.cpp -o temporal_host_check && ./temporal_host_check
// Needs no GPU and no library.  Prints the world-to-camera rows of the cameras given on the command line (15 floats each: transform, fov, F, focus) as hex floats, or,
// without arguments, checks itself: M' * transform = identity to a few ulp for rotated, translated and scaled cameras, and every refusal has its message.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../fredholm_amd/csrc/temporal_host.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static void look_at(const double o[3], const double fwd[3], float scale, float t[12])
{
  double f[3], r[3], u[3];
  const double lf = std::sqrt(fwd[0] * fwd[0] + fwd[1] * fwd[1] + fwd[2] * fwd[2]);
  for (int k = 0; k < 3; ++k) f[k] = fwd[k] / lf;
  r[0] = -f[2]; r[1] = 0.0; r[2] = f[0];  // cross(f, (0, 1, 0))
  const double lr = std::sqrt(r[0] * r[0] + r[2] * r[2]);
  for (int k = 0; k < 3; ++k) r[k] /= lr;
  u[0] = r[1] * f[2] - r[2] * f[1]; u[1] = r[2] * f[0] - r[0] * f[2]; u[2] = r[0] * f[1] - r[1] * f[0];
  for (int k = 0; k < 3; ++k) { t[4 * k] = float(scale * r[k]); t[4 * k + 1] = float(scale * u[k]); t[4 * k + 2] = float(-scale * f[k]); t[4 * k + 3] = float(o[k]); }
}

static const char* refusal(const fh_denoise_inputs* in, const fh_camera* cam, fh_temporal_params tp, const float* out = reinterpret_cast<const float*>(0x1000), uint32_t w = 8)
{
  const fh_denoise_params pr = {2.0f, 1.0f, 0.2f, 7u, 5u};
  float w2c[12], f = 0.0f;
  return fh::temporal_refusal(w, 8, in, cam, tp, pr, out, w2c, &f);
}

int main(int argc, char** argv)
{
  if (argc > 1) {
    for (int a = 1; a + 14 < argc; a += 15) {
      float t[12], m[12];
      for (int k = 0; k < 12; ++k) t[k] = std::strtof(argv[a + k], nullptr);
      if (!fh::camera_world_to_camera(t, m)) { std::printf("singular\n"); continue; }
      for (int k = 0; k < 12; ++k) std::printf("%a%c", double(m[k]), k == 11 ? '\n' : ' ');
    }
    return 0;
  }
  const double origins[3][3] = {{0, 1, 3}, {278, 273, -800}, {-1.5, 0.25, 7.0}}, forwards[3][3] = {{0, 0, -1}, {0.3, -0.2, 1.0}, {-1.0, 0.1, 0.05}};
  const float scales[3] = {1.0f, 0.01f, 3.0f};
  for (int c = 0; c < 3; ++c) {
    float t[12], m[12];
    look_at(origins[c], forwards[c], scales[c], t);
    EXPECT(fh::camera_world_to_camera(t, m));
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 4; ++j) {  // M' * [R | T] = [I | 0]
        double s = j == 3 ? m[4 * i + 3] : 0.0;
        for (int k = 0; k < 3; ++k) s += double(m[4 * i + k]) * double(t[4 * k + j]);
        const double want = i == j ? 1.0 : 0.0, tol = j == 3 ? 1e-6 * (1.0 + std::fabs(origins[c][0]) + std::fabs(origins[c][1]) + std::fabs(origins[c][2])) / scales[c] : 1e-6;
        EXPECT(std::fabs(s - want) <= tol);
      }
  }
  float z[12] = {}, m[12];
  EXPECT(!fh::camera_world_to_camera(z, m));
  float nan_t[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, NAN, 0};
  EXPECT(!fh::camera_world_to_camera(nan_t, m));

  const float* p = reinterpret_cast<const float*>(0x1000);  // (never dereferenced)
  const fh_denoise_inputs full = {p, p, p, p, p, p, reinterpret_cast<const uint32_t*>(p)};
  const fh_camera cam = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, 1.0f, 8.0f, 100.0f};
  const fh_temporal_params ok = {0.2f, 32.0f, 0.9f, 0.02f};
  auto has = [](const char* msg, const char* word) { return msg && std::strstr(msg, word); };
  EXPECT(refusal(&full, &cam, ok) == nullptr);
  EXPECT(has(refusal(&full, nullptr, ok), "null camera"));
  EXPECT(has(refusal(nullptr, &cam, ok), "null argument"));
  EXPECT(has(refusal(&full, &cam, ok, nullptr), "null argument"));
  EXPECT(has(refusal(&full, &cam, ok, p, 0), "width"));
  fh_denoise_inputs in = full; in.position = nullptr;
  EXPECT(has(refusal(&in, &cam, ok), "together"));
  in.depth = nullptr;
  EXPECT(has(refusal(&in, &cam, ok), "required"));
  in = full; in.moments = nullptr;
  EXPECT(has(refusal(&in, &cam, ok), "moments and counts"));
  in.counts = nullptr;
  EXPECT(refusal(&in, &cam, ok) == nullptr);
  const float bad_alpha[] = {-0.1f, 1.5f, NAN}, bad_hist[] = {0.5f, NAN, INFINITY}, bad_cos[] = {-1.0f, 1.5f, NAN}, bad_tol[] = {0.0f, -1.0f, NAN, INFINITY};
  for (float v : bad_alpha) { fh_temporal_params t = ok; t.alpha_min = v; EXPECT(has(refusal(&full, &cam, t), "alpha_min")); }
  for (float v : bad_hist) { fh_temporal_params t = ok; t.max_history = v; EXPECT(has(refusal(&full, &cam, t), "max_history")); }
  for (float v : bad_cos) { fh_temporal_params t = ok; t.normal_cos_min = v; EXPECT(has(refusal(&full, &cam, t), "normal_cos_min")); }
  for (float v : bad_tol) { fh_temporal_params t = ok; t.plane_tol = v; EXPECT(has(refusal(&full, &cam, t), "plane_tol")); }
  fh_camera c2 = cam; c2.fov = 0.0f;
  EXPECT(has(refusal(&full, &c2, ok), "fov"));
  c2 = cam; c2.transform[0] = 0.0f;
  EXPECT(has(refusal(&full, &c2, ok), "inverted"));
  const fh_temporal_params edge = {0.0f, 1.0f, 1.0f, 1e-6f};
  EXPECT(refusal(&full, &cam, edge) == nullptr);
  const fh_temporal_params edge2 = {1.0f, 1e6f, -0.999f, 10.0f};
  EXPECT(refusal(&full, &cam, edge2) == nullptr);
  std::printf(failures ? "temporal_host_check: %d failures\n" : "temporal_host_check: ok\n", failures);
  return failures ? 1 : 0;
}
