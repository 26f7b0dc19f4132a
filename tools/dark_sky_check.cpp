// tools/dark_sky_check.cpp -- what the dark-sky-pixel rule rests on, as a stand-alone host program (tests/test_dark_sky_host.py builds and runs it; no GPU):
//   g++ -std=c++17 -O2 -Wall -Werror -ffp-contract=off tools/dark_sky_check.cpp -o dark_sky_check && ./dark_sky_check
//   (the same line with -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all runs it under the sanitizers)
// (a) For EVERY float x in [-1, -2^-11], fhe_cos(fhe_acos(x)) < 0 and fhe_sqrt of it is NaN: hosek_radiance_form's `zenith` for a direction with v.y = x, so the
//     radiance is NaN in every channel and the guard counts the sample as zero.  The host build of include/fh_elementary.h has the device's bits.
//     kDarkMargin = 2^-10 is TWICE that threshold: dark_sky_pixel bounds the y of the real-number direction of every ray of a pixel, and the factor of two (4.9e-4)
//     is the slack for the float rounding of the direction the device forms -- two normalisations and a transform orthonormal to 1e-4.
// (b) render_plan_host.h: dark_sky_verdict over its whole truth table, the expectation written as the reasons that rule the mode out.
// (c) fh_dark_sky.h: dark_sky_pixel, fed as k_split_pixels feeds it, against brute force: 200 random cameras from pin-hole to F = 1 in any orientation, 64 pixels each,
//     and for each pixel 16 points of the lens rim x 16 corner and edge points of the pixel through a double-precision restatement of camera_ray's thin lens (the
//     direction is monotone along a segment between two points of either set, so the extremes lie on the boundaries).  No pixel the rule calls dark has a ray with
//     d_y >= -2^-10.  The share of truly dark pixels the rule misses is printed, not asserted: the rule may only lose speed.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../include/fh_elementary.h"
#include "../fredholm_amd/csrc/fh_dark_sky.h"
#include "../fredholm_amd/csrc/render_plan_host.h"

namespace {

int failures = 0;

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
double uniform()  // splitmix64, [0, 1)
{
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z ^= z >> 31;
  return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

void check_zenith()
{
  const uint32_t first = fhe_f2u(-1.0f), last = fhe_f2u(-0.00048828125f);  // bit patterns of negative floats grow with the magnitude
  uint64_t n = 0, bad = 0;
  for (uint32_t u = last; u <= first; ++u) {
    const float x = fhe_u2f(u);
    const float ct = fhe_cos(fhe_acos(x));
    const float zenith = fhe_sqrt(ct);
    ++n;
    if (!(ct < 0.0f) || zenith == zenith) {
      if (bad < 5) std::printf("FAILED (a): x = %.9g (0x%08x): cos(acos(x)) = %.9g, sqrt = %.9g\n", (double)x, u, (double)ct, (double)zenith);
      ++bad;
    }
  }
  if (bad) { ++failures; std::printf("FAILED (a): %llu of %llu values\n", (unsigned long long)bad, (unsigned long long)n); }
  std::printf("(a) %llu floats in [-1, -2^-11]: zenith is NaN for all but %llu\n", (unsigned long long)n, (unsigned long long)bad);
  if (fh::kDarkMargin != 2.0f * 0.00048828125f) { ++failures; std::printf("FAILED (a): kDarkMargin is not 2^-10\n"); }
}

void check_verdict()
{
  int cases = 0, on = 0;
  for (unsigned bits = 0; bits < 32u; ++bits)
    for (unsigned forced = 0; forced < 4u; ++forced) {
      const bool splits = bits & 1u, hosek = bits & 2u, ibl = bits & 4u, adaptive = bits & 8u, firsthit = bits & 16u;
      bool expect = true;
      if (!splits) expect = false;          // the lists come from the split
      if (!hosek) expect = false;           // a constant background is not NaN below the horizon
      if (ibl) expect = false;              // env_radiance looks at the IBL first
      if (adaptive) expect = false;         // the moments of a dark pixel stop it: the old path keeps that bookkeeping
      if (firsthit) expect = false;
      if (forced == 0u) expect = false;     // FH_DARK_SKY=0
      const bool got = fh::dark_sky_verdict(splits, hosek, ibl, adaptive, firsthit, forced);
      ++cases;
      on += got ? 1 : 0;
      if (got != expect) { ++failures; std::printf("FAILED (b): bits=0x%02x forced=%u: got %d, expected %d\n", bits, forced, (int)got, (int)expect); }
    }
  if (on != 3) { ++failures; std::printf("FAILED (b): %d cases switch the mode on, expected 3 (one input, forced 1, 2, 3)\n", on); }
  std::printf("(b) dark_sky_verdict: %d cases\n", cases);
}

struct Cam { float t[12]; float inv_tan, apb, lens_radius; uint32_t width, height; };

// k_split_pixels' centre line, family radius and centre direction for pixel (px, py), in fp32 with its operations, and the rule's answer
bool rule_says_dark(const Cam& c, uint32_t px, uint32_t py)
{
  const float x = (float)px + 0.5f, y = (float)py + 0.5f;
  const float uvx = -(2.0f * x - (float)c.width) / (float)c.height, uvy = (2.0f * y - (float)c.height) / (float)c.height;
  const float f = c.inv_tan, k = 1.0f - c.apb / f;
  const float ab[3] = {k * uvx - 0.0f, k * uvy - 0.0f, (2.0f * f - c.apb) - f};
  const float L = fhe_sqrt(ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2]);
  const float m = fabsf(c.lens_radius) + 1.41421357f * fabsf(k) / (float)c.height * 1.001f;
  const float s = 1.0f / L;
  const float d[3] = {s * ab[0], s * ab[1], s * ab[2]};
  const float cx = c.t[0] * d[0] + c.t[1] * d[1] + c.t[2] * d[2], cy = c.t[4] * d[0] + c.t[5] * d[1] + c.t[6] * d[2], cz = c.t[8] * d[0] + c.t[9] * d[1] + c.t[10] * d[2];
  return cx == cx && cz == cz && fh::dark_sky_pixel(cy, m, L);
}

// camera_ray's thin lens in double precision: world-space y of the unit direction of the ray through image point (ix, iy) (pixels) and lens point (lx, ly)
double ray_dir_y(const Cam& c, double ix, double iy, double lx, double ly)
{
  const double W = c.width, H = c.height, f = c.inv_tan, apb = c.apb;
  const double uvx = -(2.0 * ix - W) / H, uvy = (2.0 * iy - H) / H;
  double s2c[3] = {0.0 - uvx, 0.0 - uvy, f};
  const double n = std::sqrt(s2c[0] * s2c[0] + s2c[1] * s2c[1] + s2c[2] * s2c[2]);
  for (double& v : s2c) v /= n;
  const double t = apb / s2c[2];
  const double obj[3] = {uvx + t * s2c[0], uvy + t * s2c[1], t * s2c[2]};
  double d[3] = {obj[0] - lx, obj[1] - ly, obj[2] - f};
  const double dn = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  for (double& v : d) v /= dn;
  d[2] = -d[2];
  return (double)c.t[4] * d[0] + (double)c.t[5] * d[1] + (double)c.t[6] * d[2];
}

void check_rule()
{
  const double kPi = 3.14159265358979323846;
  const uint32_t sizes[5][2] = {{64, 48}, {96, 64}, {640, 360}, {1920, 1080}, {333, 777}};
  uint64_t pixels = 0, called_dark = 0, truly_dark = 0, missed = 0, wrong = 0;
  for (int ci = 0; ci < 200; ++ci) {
    Cam c{};
    // a uniform random rotation from a unit quaternion; columns = the camera's axes in world space, a translation that does not matter to directions
    double q[4], qn = 0.0;
    for (double& v : q) { v = 2.0 * uniform() - 1.0; qn += v * v; }
    if (qn < 1e-3) { --ci; continue; }
    for (double& v : q) v /= std::sqrt(qn);
    const double R[9] = {1 - 2 * (q[2] * q[2] + q[3] * q[3]), 2 * (q[1] * q[2] - q[0] * q[3]), 2 * (q[1] * q[3] + q[0] * q[2]),
                         2 * (q[1] * q[2] + q[0] * q[3]), 1 - 2 * (q[1] * q[1] + q[3] * q[3]), 2 * (q[2] * q[3] - q[0] * q[1]),
                         2 * (q[1] * q[3] - q[0] * q[2]), 2 * (q[2] * q[3] + q[0] * q[1]), 1 - 2 * (q[1] * q[1] + q[2] * q[2])};
    for (int r = 0; r < 3; ++r) { for (int k = 0; k < 3; ++k) c.t[4 * r + k] = (float)R[3 * r + k]; c.t[4 * r + 3] = (float)(10.0 * uniform() - 5.0); }
    const float fov = (float)((20.0 + 80.0 * uniform()) * kPi / 180.0);
    const float F = ci % 4 == 0 ? 1.0f : (float)std::pow(10.0, 6.0 * uniform());  // F = 1 ... 1e6 (a pin-hole for all purposes)
    const float focus = (float)std::pow(10.0, -0.3 + 4.3 * uniform());             // 0.5 ... 1e4
    c.inv_tan = 1.0f / tanf(0.5f * fov);
    fh::lens_values(c.inv_tan, focus, F, &c.apb, &c.lens_radius);
    c.width = sizes[ci % 5][0]; c.height = sizes[ci % 5][1];
    for (int pi = 0; pi < 64; ++pi) {
      const uint32_t px = (uint32_t)(uniform() * c.width), py = (uint32_t)(uniform() * c.height);
      const bool dark = rule_says_dark(c, px, py);
      double max_y = -2.0;
      for (int li = 0; li < 16; ++li) {
        const double a = 2.0 * kPi * li / 16.0, lx = (double)c.lens_radius * std::cos(a), ly = (double)c.lens_radius * std::sin(a);
        for (int e = 0; e < 16; ++e) {  // the pixel's boundary, four points per side, corners included
          const int side = e / 4;
          const double s = (e % 4) / 4.0;
          const double ox = side == 0 ? s : side == 1 ? 1.0 : side == 2 ? 1.0 - s : 0.0, oy = side == 0 ? 0.0 : side == 1 ? s : side == 2 ? 1.0 : 1.0 - s;
          max_y = std::fmax(max_y, ray_dir_y(c, px + ox, py + oy, lx, ly));
        }
      }
      const bool truly = max_y < -(double)fh::kDarkMargin;
      ++pixels;
      called_dark += dark ? 1 : 0;
      truly_dark += truly ? 1 : 0;
      if (truly && !dark) ++missed;
      if (dark && !truly) {
        if (wrong < 5) std::printf("FAILED (c): camera %d pixel (%u, %u) of %u x %u is called dark, a ray has d_y = %.6g\n", ci, px, py, c.width, c.height, max_y);
        ++wrong;
      }
    }
  }
  if (wrong) { ++failures; std::printf("FAILED (c): %llu pixels called dark have a ray at or above -2^-10\n", (unsigned long long)wrong); }
  if (called_dark < pixels / 10) { ++failures; std::printf("FAILED (c): only %llu of %llu pixels called dark: the test is not testing\n", (unsigned long long)called_dark, (unsigned long long)pixels); }
  std::printf("(c) %llu pixels, %llu called dark, %llu truly dark, the rule misses %.2f %% of them\n", (unsigned long long)pixels, (unsigned long long)called_dark,
              (unsigned long long)truly_dark, truly_dark ? 100.0 * (double)missed / (double)truly_dark : 0.0);
}

}  // namespace

int main()
{
  check_verdict();
  check_rule();
  check_zenith();
  if (failures) { std::printf("dark_sky_check: %d failures\n", failures); return 1; }
  std::printf("dark_sky_check: ok\n");
  return 0;
}
