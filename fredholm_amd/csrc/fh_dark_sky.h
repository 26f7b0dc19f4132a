// fh_dark_sky.h -- sky pixels every sample of which the NaN guard zeroes: the rule k_split_pixels applies (render.hip), in a form a host program can include
// (tools/dark_sky_check.cpp).
//
// Under the Hosek sky a camera ray that leaves the scene bounds with a direction below the horizon carries NaN: hosek_radiance_form takes sqrt_cr(fhe_cos(fhe_acos(v.y))),
// which is the root of a negative number for v.y < 0, and c[7] * zenith enters every channel (0 * NaN and inf * NaN are NaN as well).  k_sky_pixels and k_accumulate count
// such a sample as zero (bad3).  A sky pixel ALL rays of which point below the horizon therefore only ever adds zeros to its means, whatever its samples draw.
//
// The rays of a pixel are the lines through the lens disk (radius R around A0) and the pixel's square in the mirrored focus plane (half-diagonal rho around B0), see
// k_split_pixels.  With u0 = B0 - A0, L = |u0| and m = R + rho every ray has u = B - A with |u - u0| <= m and |u| >= L - m, so its unit direction differs from the
// centre line's by | u / |u| - u0 / |u0| | <= |u - u0| / |u| + | |u0| - |u| | / |u| <= 2 m / (L - m) in norm, hence in y, and a rigid camera transform keeps that.
//
// kDarkMargin: fhe_cos(fhe_acos(x)) is negative, and its root NaN, for EVERY float x in [-1, -2^-11] (tools/dark_sky_check.cpp goes through all of them; the host
// build of fh_elementary.h has the device's bits).  The rule asks for twice that, -2^-10: the bound above is one of real numbers, and the direction the device forms
// -- two normalisations, a 3x3 transform that is orthonormal to 1e-4 (split_pixels) -- is off by rounding, some 1e-6 for unit vectors and up to 1e-4 for the
// transform; 2^-11 ~ 4.9e-4 of slack and the 1e-3 the rule adds on top cover both.
#pragma once
#if defined(__HIPCC__)
#include "fh_vec.h"
#elif !defined(FH_HD)
#define FH_HD inline
#endif

namespace fh {

constexpr float kDarkMargin = 0.0009765625f;  // 2^-10

// cy: world-space y of the pixel's unit centre direction (after the z flip and the camera transform); m = R + rho and L as k_split_pixels forms them.
// Conservative: false for a pixel near the horizon, for L <= 1.01 m (a family of rays that wide has no useful bound) and for NaN in any argument.
FH_HD bool dark_sky_pixel(float cy, float m, float L)
{
  if (!(L > 1.01f * m)) return false;
  const float spread = 2.0f * m / (L - m) * 1.001f + 1e-3f;
  return cy + spread < -kDarkMargin;
}

}  // namespace fh
