// tools/sky_defer_check.cpp -- render_plan_host.h: sky_defer_verdict over its whole truth table, as a stand-alone host program (tests/test_gpu_sky_defer.py builds and
// runs it; no GPU).  The expectation is written the other way round from the function: it names the reasons that rule the mode OUT, one by one.
//   g++ -std=c++17 -Wall -Werror tools/sky_defer_check.cpp -o sky_defer_check && ./sky_defer_check
#include <cstdio>

#include "../fredholm_amd/csrc/render_plan_host.h"

int main()
{
  int failures = 0, cases = 0, on = 0;
  for (unsigned bits = 0; bits < 256u; ++bits)
    for (unsigned forced = 0; forced < 4u; ++forced)
      for (int by_default = 0; by_default < 2; ++by_default) {
        const bool emitters = bits & 1u, hosek = bits & 2u, ibl = bits & 4u, env_sampling = bits & 8u, light_tables = bits & 16u, stream = bits & 32u, merged = bits & 64u, three = bits & 128u;
        bool expect = true;
        if (emitters) expect = false;                  // the light ray's weight needs its hit
        if (!hosek && !ibl) expect = false;            // a constant background keeps its pruning
        if (env_sampling || light_tables) expect = false;
        if (!stream || merged) expect = false;         // only the streaming secondary launch of its own leaves escape masks
        if (!three) expect = false;                    // the deferred shade kernels exist in the three-workgroup set
        if (forced == 0u) expect = false;
        if (forced >= 2u && !by_default) expect = false;
        const bool got = fh::sky_defer_verdict(emitters, hosek, ibl, env_sampling, light_tables, stream, merged, three, forced, by_default != 0);
        ++cases;
        on += got ? 1 : 0;
        if (got != expect) {
          ++failures;
          std::printf("FAILED case bits=0x%02x forced=%u by_default=%d: got %d, expected %d\n", bits, forced, by_default, (int)got, (int)expect);
        }
      }
  // eligible inputs: no emitters, (hosek | ibl) 3 of 4, no env, no tables, stream, not merged, three = 3 of 256; on for forced 1 (x2) and forced 2, 3 with by_default (x2)
  if (on != 3 * 4) { ++failures; std::printf("FAILED: %d cases switch the mode on, expected 12\n", on); }
  if (failures) { std::printf("sky_defer_check: %d failures\n", failures); return 1; }
  std::printf("sky_defer_check: ok (%d cases)\n", cases);
  return 0;
}
