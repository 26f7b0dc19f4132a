// tools/motion_host_check.cpp -- the host-only part of the per-instance motion vectors (fredholm_amd/csrc/motion_host.h: the motion table and the refusals of
// fh_denoise_temporal_motion) as a stand-alone program, for the host sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/motion_host_check.cpp -o motion_host_check && ./motion_host_check
// Needs no GPU and no library.  Checks itself: equal matrices are not moved and give the identity maps, a translation gives its inverse translation and the identity
// normal map, point carries a point of the current pose to the previous pose for a rotated and scaled instance, normal is the inverse transpose of point's linear
// part, and every refusal has its message.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../fredholm_amd/csrc/motion_host.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// o2w = rotation about y by `a` times diag(s) plus t; w2o its inverse, both rounded to float
static void pose(double a, const double s[3], const double t[3], float o2w[12], float w2o[12])
{
  const double c = std::cos(a), sn = std::sin(a);
  const double R[3][3] = {{c, 0, sn}, {0, 1, 0}, {-sn, 0, c}};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) o2w[4 * i + j] = float(R[i][j] * s[j]);
    o2w[4 * i + 3] = float(t[i]);
  }
  for (int i = 0; i < 3; ++i) {
    double ti = 0.0;
    for (int j = 0; j < 3; ++j) { w2o[4 * i + j] = float(R[j][i] / s[i]); ti -= R[j][i] / s[i] * t[j]; }
    w2o[4 * i + 3] = float(ti);
  }
}

int main()
{
  const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  fh_motion m{};
  fh::motion_entry(I, I, I, I, &m);
  EXPECT(m.moved == 0u);
  for (int k = 0; k < 12; ++k) EXPECT(m.point[k] == I[k]);
  const float T[12] = {1, 0, 0, 0.25f, 0, 1, 0, -0.5f, 0, 0, 1, 0.125f}, Ti[12] = {1, 0, 0, -0.25f, 0, 1, 0, 0.5f, 0, 0, 1, -0.125f};
  fh::motion_entry(I, I, T, Ti, &m);
  EXPECT(m.moved == 1u);
  for (int k = 0; k < 12; ++k) EXPECT(m.point[k] == Ti[k]);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) EXPECT(m.normal[3 * i + j] == (i == j ? 1.0f : 0.0f));
  const double s0[3] = {0.5, 1.7, 1.1}, s1[3] = {0.8, 1.2, 2.0}, t0[3] = {0.1, 0.2, -0.3}, t1[3] = {0.4, -0.1, 0.6};
  float po[12], pw[12], co[12], cw[12];
  pose(0.3, s0, t0, po, pw);
  pose(1.1, s1, t1, co, cw);
  fh::motion_entry(po, pw, co, cw, &m);
  EXPECT(m.moved == 1u && fh::motion_finite(m));
  const double obj[3] = {0.3, -0.7, 0.45};
  double cur[3], prev[3], back[3];
  for (int i = 0; i < 3; ++i) {
    cur[i] = co[4 * i] * obj[0] + co[4 * i + 1] * obj[1] + co[4 * i + 2] * obj[2] + co[4 * i + 3];
    prev[i] = po[4 * i] * obj[0] + po[4 * i + 1] * obj[1] + po[4 * i + 2] * obj[2] + po[4 * i + 3];
  }
  for (int i = 0; i < 3; ++i) {
    back[i] = m.point[4 * i] * cur[0] + m.point[4 * i + 1] * cur[1] + m.point[4 * i + 2] * cur[2] + m.point[4 * i + 3];
    EXPECT(std::fabs(back[i] - prev[i]) < 2e-6);
  }
  for (int i = 0; i < 3; ++i)      // normal^T * L(point) = identity
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
      for (int k = 0; k < 3; ++k) s += (double)m.normal[3 * k + i] * (double)m.point[4 * k + j];
      EXPECT(std::fabs(s - (i == j ? 1.0 : 0.0)) < 2e-6);
    }
  // the refusals
  const uint32_t* ids = reinterpret_cast<const uint32_t*>(0x1000);
  std::vector<fh_motion> table(3);
  for (fh_motion& e : table) fh::motion_entry(I, I, I, I, &e);
  bool any = true;
  EXPECT(fh::motion_refusal(nullptr, 0, nullptr, &any) == nullptr && !any);
  EXPECT(fh::motion_refusal(nullptr, 3, nullptr, &any) == nullptr && !any);
  EXPECT(fh::motion_refusal(ids, 3, table.data(), &any) == nullptr && !any);
  fh::motion_entry(I, I, T, Ti, &table[2]);
  EXPECT(fh::motion_refusal(ids, 3, table.data(), &any) == nullptr && any);
  EXPECT(fh::motion_refusal(ids, 3, nullptr, &any) != nullptr && !any);
  EXPECT(fh::motion_refusal(nullptr, 3, table.data(), &any) != nullptr);
  EXPECT(fh::motion_refusal(ids, 0, table.data(), &any) != nullptr);
  table[1].normal[8] = NAN;
  EXPECT(fh::motion_refusal(ids, 3, table.data(), &any) != nullptr);
  table[1].normal[8] = 1.0f;
  table[0].point[3] = INFINITY;
  EXPECT(fh::motion_refusal(ids, 3, table.data(), &any) != nullptr);
  EXPECT(fh::motion_refusal(ids, 0, nullptr, &any) != nullptr);
  const float apb = fh::chief_a_plus_b(1.0f, 10000.0f);
  EXPECT(apb > 10000.0f && apb < 10001.0f);
  std::printf(failures ? "%d failures\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
