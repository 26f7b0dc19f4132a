// fh_skin.h -- linear-blend skinning of one vertex (host + device): the blended joint matrix, the posed position and the posed normal.  Shared by scene.hip
// (k_skin_vertices) and the stand-alone program of tests/test_skinning_host.py (tests/cpp/skin_host.cpp).  The arithmetic is the one include/fredholm_hip.h states
// under fh_skin_desc: fp32 without contraction, / and sqrt correctly rounded, every product and sum rounded in the order written.  Plain C++ on float arrays, so that
// it compiles without HIP; the position is fh_vec.h's xform_point restated (same products, same left-to-right sum).  The reference has no counterpart (its glTF
// reader loads no skins).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define FH_SK __host__ __device__ __forceinline__
#else
#define FH_SK inline
#endif

namespace fh {

FH_SK bool skin_unskinned(const float w[4]) { return w[0] == 0.0f && w[1] == 0.0f && w[2] == 0.0f && w[3] == 0.0f; }

// B = ((w0 J0 + w1 J1) + w2 J2) + w3 J3, entry by entry of the row-major 3 x 4 matrices
FH_SK void skin_blend(const float* j0, const float* j1, const float* j2, const float* j3, const float w[4], float b[12])
{
  for (int e = 0; e < 12; ++e) b[e] = ((w[0] * j0[e] + w[1] * j1[e]) + w[2] * j2[e]) + w[3] * j3[e];
}

// xform_point(B, p): row r is ((B[r][0] p.x + B[r][1] p.y) + B[r][2] p.z) + B[r][3] * 1
FH_SK void skin_point(const float b[12], const float p[3], float out[3])
{
  for (int r = 0; r < 3; ++r) out[r] = b[4 * r] * p[0] + b[4 * r + 1] * p[1] + b[4 * r + 2] * p[2] + b[4 * r + 3] * 1.0f;
}

FH_SK void skin_cross(const float* a, const float* c, float out[3])
{
  out[0] = a[1] * c[2] - a[2] * c[1];
  out[1] = a[2] * c[0] - a[0] * c[2];
  out[2] = a[0] * c[1] - a[1] * c[0];
}
FH_SK float skin_dot(const float* a, const float* c) { return a[0] * c[0] + a[1] * c[1] + a[2] * c[2]; }

// the bind normal through the cofactor matrix of B's 3 x 3 part (the inverse transpose without its division by the determinant), turned where the determinant is
// negative and rescaled to the bind normal's length; the bind normal itself where the result has no direction
FH_SK void skin_normal(const float b[12], const float n[3], float out[3])
{
  float c0[3], c1[3], c2[3];
  skin_cross(b + 4, b + 8, c0);
  skin_cross(b + 8, b, c1);
  skin_cross(b, b + 4, c2);
  float m[3] = {skin_dot(c0, n), skin_dot(c1, n), skin_dot(c2, n)};
  if (skin_dot(b, c0) < 0.0f) { m[0] = -m[0]; m[1] = -m[1]; m[2] = -m[2]; }
  const float len_n = sqrtf(skin_dot(n, n)), len_m = sqrtf(skin_dot(m, m));
  if (!(len_m > 0.0f && len_m <= 3.402823466e38f)) { out[0] = n[0]; out[1] = n[1]; out[2] = n[2]; return; }
  const float s = len_n / len_m;
  out[0] = m[0] * s; out[1] = m[1] * s; out[2] = m[2] * s;
}

// one vertex: j, w its four joints and weights, palette 12 floats per joint (every j[k] below the palette's size unless all weights are 0)
FH_SK void skin_vertex(const float* palette, const uint16_t j[4], const float w[4], const float p[3], const float n[3], float p_out[3], float n_out[3])
{
  if (skin_unskinned(w)) {
    for (int k = 0; k < 3; ++k) { p_out[k] = p[k]; n_out[k] = n[k]; }
    return;
  }
  float b[12];
  skin_blend(palette + 12 * (size_t)j[0], palette + 12 * (size_t)j[1], palette + 12 * (size_t)j[2], palette + 12 * (size_t)j[3], w, b);
  skin_point(b, p, p_out);
  skin_normal(b, n, n_out);
}

}  // namespace fh
