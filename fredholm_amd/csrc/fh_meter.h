// fh_meter.h -- auto-exposure of the post chain (host + device): the per-pixel bin, the resolve of a 257-word luminance histogram into the exposure state, and the
// host-side refusals and constants.  Shared by post.hip (k_meter_histogram, k_meter_resolve), capi.hip (fh_set_auto_exposure) and the stand-alone programs of
// tests/test_auto_exposure_host.py.  The arithmetic is the one include/fredholm_hip.h states under fh_auto_exposure_params: fp32 without contraction, the rank cuts and
// the sum S in double, everything in the order written.  The reference has no counterpart (its exposure is PostProcessParams::ISO alone).
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/fh_elementary.h"
#include "../../include/fredholm_hip.h"

#if defined(__HIPCC__)
#define FH_MT __host__ __device__ __forceinline__
#else
#define FH_MT inline
#endif

namespace fh {

constexpr int kMeterBins = 256;                // bins of the histogram; word [kMeterBins] counts the unmetered pixels
constexpr int kMeterWords = kMeterBins + 1;

// what the kernels take by value: fh_auto_exposure_params with everything that needs the host's elementary functions done (meter_consts)
struct MeterConsts {
  float log2_lo, scale;      // scale = 256 / (log2_hi - log2_lo)
  float low, high;
  float log2key, compensation_ev, min_ev, max_ev;
  float a_up, a_down;        // a_x = 1 - exp(-frame_time * speed_x); exactly 1 for an infinite frame_time
};

FH_MT float meter_finite(float v) { return (v != v || fabsf(v) > 3.0e38f) ? 0.0f : v; }
FH_MT float meter_lum(float r, float g, float b) { return (r * 0.2126729f + g * 0.7151522f) + b * 0.0721750f; }

// the bin of one pixel: 0 .. 255, or kMeterBins for an unmetered one (!(l > 0)).  The clamp is done on the float, before the conversion: the same value wherever
// (int)floorf(.) is defined, and defined for every finite log2_lo
FH_MT int meter_bin(float r, float g, float b, float log2_lo, float scale)
{
  const float l = meter_lum(meter_finite(r), meter_finite(g), meter_finite(b));
  if (!(l > 0.0f)) return kMeterBins;
  const float t = floorf((fhe_log2(l) - log2_lo) * scale);
  return t < 0.0f ? 0 : (t > 255.0f ? 255 : (int)t);
}

FH_MT float meter_bin_centre(int b, float log2_lo, float scale) { return ((float)b + 0.5f) / scale + log2_lo; }

// the resolve in the pieces post.hip's k_meter_resolve runs in parallel (one bin per lane) and meter_resolve below runs in a loop: the same functions, the same bits
FH_MT void meter_cuts(uint32_t n, float low, float high, uint32_t* cut, uint32_t* end)
{
  uint32_t c = (uint32_t)((double)n * (double)low), e = (uint32_t)((double)n * (double)high);
  if (e <= c) { e = c + 1 < n ? c + 1 : n; c = e - 1; }
  *cut = c; *end = e;
}
// c0: the count in the bins before this one, h: the bin's own
FH_MT uint32_t meter_kept(uint32_t c0, uint32_t h, uint32_t cut, uint32_t end)
{
  const uint32_t c1 = c0 + h;
  const uint32_t lo = c0 > cut ? c0 : cut, hi = c1 < end ? c1 : end;
  return hi > lo ? hi - lo : 0u;
}
// the bin's term of S; the terms are summed serially in bin order
FH_MT double meter_term(uint32_t kept, int b, float log2_lo, float scale) { return (double)kept * (double)meter_bin_centre(b, log2_lo, scale); }
// n > 0 metered pixels, S over the end - cut kept ranks
FH_MT void meter_update(uint32_t n, uint32_t unmetered, double s, uint32_t cut, uint32_t end, const MeterConsts& mc, fh_auto_exposure_state* st)
{
  const float mean_log2 = (float)(s / (double)(end - cut));
  const float target = fmaxf(mc.min_ev, fminf((mc.log2key - mean_log2) + mc.compensation_ev, mc.max_ev));
  float ev = target;
  if (st->frames != 0) {
    const float a = target > st->ev ? mc.a_up : mc.a_down;
    ev = st->ev + (target - st->ev) * a;
  }
  st->ev = ev; st->target_ev = target; st->mean_log2 = mean_log2;
  st->metered = n; st->unmetered = unmetered; st->frames += 1;
}

// hist: 257 words.  Returns 0 and leaves *st alone when no pixel was metered; otherwise updates every field of *st and returns 1
FH_MT int meter_resolve(const uint32_t* hist, const MeterConsts& mc, fh_auto_exposure_state* st)
{
  uint32_t n = 0;
  for (int b = 0; b < kMeterBins; ++b) n += hist[b];
  if (n == 0) return 0;
  uint32_t cut, end;
  meter_cuts(n, mc.low, mc.high, &cut, &end);
  double s = 0.0;
  uint32_t c0 = 0;
  for (int b = 0; b < kMeterBins; ++b) {
    s += meter_term(meter_kept(c0, hist[b], cut, end), b, mc.log2_lo, mc.scale);
    c0 += hist[b];
  }
  meter_update(n, hist[kMeterBins], s, cut, end, mc, st);
  return 1;
}

FH_MT float meter_exposure(float ev) { return fhe_pow(2.0f, ev); }

// ---- host only
inline const fh_auto_exposure_params& auto_exposure_defaults()
{
  static const fh_auto_exposure_params d = {0.18f, 0.0f, -16.0f, 16.0f, 0.10f, 0.90f, 3.0f, 1.0f, 1.0f / 30.0f, -16.0f, 16.0f, 0u};
  return d;
}

// every refusal is decided from the parameters alone; nullptr: acceptable (params == nullptr switches off)
inline const char* auto_exposure_refusal(const fh_auto_exposure_params* p)
{
  if (!p) return nullptr;
  if (!(p->key > 0.0f) || !std::isfinite(p->key)) return "key must be finite and > 0";
  if (!std::isfinite(p->compensation_ev)) return "compensation_ev must be finite";
  if (!std::isfinite(p->min_ev) || !std::isfinite(p->max_ev)) return "min_ev and max_ev must be finite";
  if (p->min_ev > p->max_ev) return "min_ev must not exceed max_ev";
  if (!std::isfinite(p->log2_lo) || !std::isfinite(p->log2_hi)) return "log2_lo and log2_hi must be finite";
  const float range = p->log2_hi - p->log2_lo;
  if (!(range > 0.0f) || !(range <= 64.0f)) return "log2_hi - log2_lo must be in (0, 64]";
  if (!(p->low >= 0.0f && p->low <= 1.0f) || !(p->high >= 0.0f && p->high <= 1.0f)) return "low and high must be in [0, 1]";
  if (p->low >= p->high) return "low must be below high";
  if (!(p->speed_up >= 0.0f) || !std::isfinite(p->speed_up) || !(p->speed_down >= 0.0f) || !std::isfinite(p->speed_down)) return "speed_up and speed_down must be finite and >= 0";
  if (!(p->frame_time >= 0.0f)) return "frame_time must be >= 0 (+inf: no adaptation)";
  if (p->flags & ~(uint32_t)FH_AE_BLOOM_RELATIVE) return "unknown flag bits";
  return nullptr;
}

inline MeterConsts meter_consts(const fh_auto_exposure_params& p)
{
  MeterConsts mc;
  mc.log2_lo = p.log2_lo; mc.scale = 256.0f / (p.log2_hi - p.log2_lo);
  mc.low = p.low; mc.high = p.high;
  mc.log2key = fhe_log2(p.key); mc.compensation_ev = p.compensation_ev; mc.min_ev = p.min_ev; mc.max_ev = p.max_ev;
  const bool no_adaptation = std::isinf(p.frame_time);
  mc.a_up = no_adaptation ? 1.0f : 1.0f - fhe_exp(-p.frame_time * p.speed_up);
  mc.a_down = no_adaptation ? 1.0f : 1.0f - fhe_exp(-p.frame_time * p.speed_down);
  return mc;
}

}  // namespace fh
