// render_plan_host.h -- the host-only decisions of fh_render's submit path (render.hip: render_submit and its steps) as pure functions of plain values: how large the
// path pools may be, how a call is cut into passes, how much of the traversal stack stays in LDS, how many workgroups a streaming launch gets, the packed chunk words,
// where the fused tail takes over, where rays start, and the two lens constants of the frame.  Plain C++ without HIP like temporal_host.h and motion_host.h, so that it
// also compiles into a stand-alone program (tools/render_plan_check.cpp) for the tests and the host sanitizers.  Every expression keeps the integer widths, the order
// and the floating-point type it had inside render_submit: tests/golden/render_plan_cases.json holds what those lines gave.
#pragma once
#include <cmath>
#include <cstdint>

namespace fh {

// The default pool size is a wish: all pools together are kept within A QUARTER of what the device has free, counting what the pools already hold (`held`) as free.
// (pool_share: the members of a group on this device.)  Never below one path per owned pixel.
inline uint32_t pool_target_cap(unsigned long long free_bytes, unsigned long long held, uint32_t pool_share, int n_slots, unsigned long long bytes_per_path, uint32_t target_default,
                                uint32_t n_owned)
{
  const unsigned long long cap = (free_bytes + held) / (4ull * pool_share) / ((unsigned long long)n_slots * bytes_per_path);
  if (cap < target_default) return cap > n_owned ? (uint32_t)cap : n_owned;
  return target_default;
}

// samples per pass of a run of n_samples samples over n_px pixels (the whole call; in adaptive mode, one round) with room for `target` paths in a pool
inline uint32_t samples_per_pass(uint32_t target, uint32_t n_px, uint32_t n_samples, uint32_t n_slots, bool quirk, bool serial)
{
  uint32_t batch = n_px ? target / n_px : n_samples;
  if (batch > n_samples) batch = n_samples;
  if (batch > 65535u) batch = 65535u;  // (k_generate's grid has one row per sample of the pass)
  if (batch < 1) batch = 1;
  if (batch < n_samples) {  // equal passes, and whole rounds of the passes in flight: a call of 1024 samples with room for 248 per pass runs six passes of 171, not four of
    // 248 and a runt of 32 -- the last pass of an incomplete round has nothing to overlap with (configs[2]: 3 / 4 / 5 / 6 passes measure 7700 / 7577 / 7578 / 7598 Msamples/s, r5-5)
    uint32_t passes = (n_samples + batch - 1u) / batch;
    if (n_slots > 1u && passes > n_slots && passes % n_slots != 0u && (passes / n_slots + 1u) * n_slots <= n_samples) passes = (passes / n_slots + 1u) * n_slots;
    batch = (n_samples + passes - 1u) / passes;
  }
  // (the passes of a call overlap, three in flight: a big call that would fit one or two passes is cut into three of the same size -- unless its passes run one after
  // the other anyway: the bug-compat mode and the measuring mode, where a split is pure overhead)
  if (!quirk && !serial && (n_samples + batch - 1u) / batch < n_slots && n_samples >= n_slots && (unsigned long long)n_samples * n_px >= 3ull << 24) batch = (n_samples + n_slots - 1u) / n_slots;
  return batch;
}

// The stack costs LDS, and LDS costs resident workgroups.  Each of the two streaming kernels keeps as many stack levels in LDS as still give it the workgroups per CU it is
// compiled for (`blocks_wanted`: at n workgroups per CU one has lds_per_cu / n bytes, and what the static LDS leaves is the stack's, 1280 bytes per entry) and spills the
// deeper levels, which are rarely reached, to global memory (GroupStack<true>).  forced_entries (FH_STACK_LDS=n) fixes the number, 99 keeps everything in LDS.
// occupancy(entries): resident workgroups per CU of the kernel with that many entries in LDS -- the HIP query in the library, a table in the check program.
struct StreamLds { uint32_t entries, blocks; };
template <typename Occupancy>
inline StreamLds stream_lds_entries(uint32_t lds_per_cu, uint32_t blocks_wanted, uint32_t static_lds, uint32_t stream_need, uint32_t forced_entries, Occupancy&& occupancy)
{
  const uint32_t lds_share = lds_per_cu / blocks_wanted;
  const uint32_t fit = lds_share > static_lds + 1280u ? (lds_share - static_lds) / 1280u : 1u;
  const uint32_t floor_entries = fit < 8u ? fit : 8u;
  uint32_t entries = stream_need;
  int got = occupancy(entries);
  if (forced_entries) entries = forced_entries < stream_need ? forced_entries : stream_need;
  else if (stream_need > floor_entries) {
    const int best = occupancy(floor_entries);
    while (entries > floor_entries && got < best) { --entries; got = occupancy(entries); }
  }
  if (entries != stream_need) got = occupancy(entries);
  return StreamLds{entries, got > 0 ? (uint32_t)got : 0u};
}

// workgroups per CU of a streaming launch: what the CU's LDS holds of `bytes` of stack + static_lds, at most what the kernel is compiled for, at most what the runtime
// reported (0: nothing reported, or not a streaming launch), at most `cap` (FH_STREAM_BLOCKS_FILLER while a sky filler runs beside the passes)
inline uint32_t stream_wgs(uint32_t lds_per_cu, uint32_t bytes, uint32_t static_lds, uint32_t compiled_for, uint32_t reported, uint32_t cap)
{
  uint32_t w = lds_per_cu / (bytes + static_lds);
  w = w > compiled_for ? compiled_for : (w < 1u ? 1u : w);
  if (reported && reported < w) w = reported;
  return w > cap ? cap : w;
}

// (rays through a small tree are cheap enough to run into the atomic rate of the work cursor: allow larger chunks there, stream_chunk_for)
inline uint32_t stream_chunk_max(bool chunk_fixed, uint32_t chunk, uint32_t n_nodes)
{
  return chunk_fixed ? chunk : (n_nodes < 512u ? 256u : (n_nodes < 4096u ? 128u : chunk));
}
// what a streaming launch is given: queue entries a wave takes per global atomic, and above them the adaptive maximum (0: none)
inline uint32_t stream_chunk_word(uint32_t chunk, uint32_t chunk_max)
{
  return (chunk & 0xffffu) | ((chunk_max > chunk ? chunk_max : 0u) << 16);
}

// Bounces the pass runs as wavefront kernels before k_tail finishes the survivors: the first depth at which THIS pass of n_paths paths is expected to have at most
// tail_paths survivors, by the share of an earlier pass's paths alive at each depth (context.h: survival); then the context's and the environment's fixed depths, and
// the clamp to [1, max_depth].  *auto_depth: the pick before the overrides (kept for the debug print).
inline uint32_t tail_wave_depth(const double* survival, uint32_t survival_n, uint32_t n_paths, uint32_t tail_paths, uint32_t max_depth, uint32_t forced_ctx, uint32_t forced_env,
                                uint32_t* auto_depth)
{
  uint32_t pick = 0;
  if (!survival_n) pick = n_paths > (1u << 22) ? max_depth : 2u;  // (nothing known: a big pass runs without the tail -- a wavefront bounce of few paths costs it 0.5 ms, a tail of millions of paths seconds)
  else {
    const uint32_t known = survival_n - 1u;
    for (uint32_t d = 1; d <= known && !pick; ++d)
      if ((double)n_paths * survival[d] <= (double)tail_paths) pick = d;
    if (!pick) {
      // too many survivors even at the last depth counted: extrapolate with the survival ratio of the last bounce.  (Snapshots only
      // arrive when the host happens to be behind the GPU -- after a synchronisation -- so the depth has to be right in one step.)
      const double last = (double)n_paths * survival[known], prev = known ? (double)n_paths * survival[known - 1u] : 0.0;
      uint32_t more = 1;
      if (last > 0.0 && prev > last) {
        const double steps = std::ceil(std::log((double)tail_paths / last) / std::log(last / prev));
        more = steps < 1.0 ? 1u : (steps > 16.0 ? 16u : (uint32_t)steps);
      }
      pick = known + more;
    }
  }
  *auto_depth = pick;
  uint32_t wave_depth = forced_ctx ? forced_ctx : pick;
  if (forced_env) wave_depth = forced_env;
  if (wave_depth < 1u) wave_depth = 1u;
  if (wave_depth > max_depth) wave_depth = max_depth;
  return wave_depth;
}

// A counter snapshot of a finished pass (`stride` words per bounce, word `rad_index` of each: the entries of the radiance queue the bounce consumed) folded into the
// shares alive per depth: entries 0 .. min(wave_depth, 65) are overwritten, and a shallower snapshot does not shorten what is known (a pass the tail took over early
// says nothing about the deeper shares: what an earlier pass of this scene measured stays).  Returns the new survival_n; a snapshot of no paths changes nothing.
inline uint32_t fold_survival(const uint32_t* counters, uint32_t stride, uint32_t rad_index, uint32_t wave_depth, uint32_t paths, double* survival, uint32_t survival_n)
{
  if (!paths) return survival_n;
  const uint32_t n = wave_depth < 65u ? wave_depth : 65u;
  for (uint32_t d = 0; d <= n; ++d) survival[d] = (double)counters[d * stride + rad_index] / (double)paths;
  return survival_n < n + 1u ? n + 1u : survival_n;
}

// What the secondary launches of a probing pass cost, added to *cost, and the shaded paths they served, added to *items, over the pass's wavefront bounces
inline void fold_probe_cost(const uint32_t* counters, uint32_t stride, uint32_t node_index, uint32_t tri_index, uint32_t sec_index, uint32_t wave_depth, double* cost, double* items)
{
  constexpr double kNodeRoundCycles = 510.0, kTriRoundCycles = 175.0;  // SIMD cycles of a wave-level node-test / triangle-test round: the issue model's weights
  double c = 0.0, n = 0.0;
  for (uint32_t d = 0; d < wave_depth; ++d) { c += kNodeRoundCycles * counters[d * stride + node_index] + kTriRoundCycles * counters[d * stride + tri_index]; n += counters[d * stride + sec_index]; }
  *cost += c; *items += n;
}

// Where the first-hit rays of a scene start, from what the probing passes cost (SIMD cycles of tests, by the issue model's weights) per shaded path:
// 0: keep probing (under 65536 items on either side), 1: at the root, 2: at the node of the face they leave -- only where that is at least 5 % cheaper
inline int bottom_up_verdict(const double cost[2], const double items[2])
{
  if (!(items[0] >= 65536.0 && items[1] >= 65536.0)) return 0;
  const double off = cost[0] / items[0], on = cost[1] / items[1];
  return on < 0.95 * off ? 2 : 1;
}

// camera.cu:33-36, in fp32 like the device code these lines used to be in (volatile: no contraction, no double-precision intermediates): a + b of the thin lens and
// the lens radius.  These bits reach the frame.
inline void lens_values(float inv_tan, float focus, float F, float* a_plus_b, float* lens_radius)
{
  volatile float f = inv_tan, b = focus;
  volatile float inv_b = 1.0f / b;
  volatile float den = 1.0f + f;
  den = den - inv_b;
  volatile float a = 1.0f / den;
  volatile float apb = a + b;
  volatile float two_f = 2.0f * f;
  volatile float lr = two_f / F;
  *a_plus_b = apb;
  *lens_radius = lr;
}

// Whether a pass stores the sky and light slots of its shadow rays as WEIGHTS and k_sky_resolve evaluates the environment for the rays that escaped (render.hip):
// only where the environment is worth deferring (Hosek sky or IBL; a constant background is one multiply and keeps its zero-contribution pruning), where nothing else
// finishes those slots (emitters: resolve_light_ray; env / light-table sampling: their own weights) and where the kernels that know the mode run -- the streaming
// secondary-ray launch of its own (not the merged launch of a one-pass call, not the fixed-batch kernels) after the three-workgroup shade set.
// forced (FH_SKY_DEFER): 0 off, 1 on where eligible, anything else: `by_default`.
inline bool sky_defer_verdict(bool emitters, bool hosek, bool ibl, bool env_sampling, bool light_tables, bool stream_secondary, bool merged, bool shade_three, uint32_t forced, bool by_default)
{
  const bool eligible = !emitters && (hosek || ibl) && !env_sampling && !light_tables && stream_secondary && !merged && shade_three;
  if (forced == 0u) return false;
  if (forced == 1u) return eligible;
  return eligible && by_default;
}

// Whether k_split_pixels sets the DARK sky pixels apart -- those every ray of which points below the horizon of the Hosek sky, so that every sample is NaN and counts
// as zero (fh_dark_sky.h) -- and k_dark_pixels advances their means without rendering a sample: only in a call that splits off its sky pixels, only where a camera
// ray that leaves the scene sees the Hosek sky (an IBL comes first in env_radiance; a constant background is not NaN), and not in the modes that need more than the
// means of a pixel: an adaptive call (the moments of a dark pixel would stop it at its first boundary: the old path does that bookkeeping) and FH_FLAG_REFERENCE_FIRSTHIT.
// forced (FH_DARK_SKY): 0 off, anything else: on where eligible.
inline bool dark_sky_verdict(bool splits_sky, bool hosek, bool ibl, bool adaptive, bool reference_firsthit, uint32_t forced)
{
  const bool eligible = splits_sky && hosek && !ibl && !adaptive && !reference_firsthit;
  return forced != 0u && eligible;
}

}  // namespace fh
