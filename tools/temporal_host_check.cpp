// tools/temporal_host_check.cpp -- the host-only part of fh_denoise_temporal (fredholm_amd/csrc/temporal_host.h: the refusals, the camera inversion and the plan of a
// call) as a stand-alone program, for the host sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/temporal_host_check.cpp -o temporal_host_check && ./temporal_host_check
// Needs no GPU and no library.  Prints the world-to-camera rows of the cameras given on the command line (15 floats each: transform, fov, F, focus) as hex floats, or,
// without arguments, checks itself: M' * transform = identity to a few ulp for rotated, translated and scaled cameras, every refusal has its message, and the plan gives
// what the code's own comments state.  With the path of a table of cases as its one argument (tests/golden/temporal_plan_cases.json: the inputs and outputs of the same
// decisions while they were still spread over denoise_temporal_submit and fh_denoise_temporal) it also replays every row to equality:
//   ./temporal_host_check tests/golden/temporal_plan_cases.json
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

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

using u64 = unsigned long long;
struct Row { std::string fn; std::vector<u64> in, out; };

// the fixture's own small format: a list of {"fn": name, "in": [unsigned integers], "out": [unsigned integers]}
static bool read_rows(const char* path, std::vector<Row>& rows)
{
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  std::string text;
  char buf[4096];
  for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, n);
  std::fclose(f);
  auto numbers = [&](size_t& at, const char* key, std::vector<u64>& out) {
    at = text.find(key, at);
    if (at == std::string::npos) return false;
    at = text.find('[', at);
    if (at == std::string::npos) return false;
    for (++at; at < text.size() && text[at] != ']';) {
      if (text[at] >= '0' && text[at] <= '9') {
        char* end = nullptr;
        out.push_back(std::strtoull(text.c_str() + at, &end, 10));
        at = (size_t)(end - text.c_str());
      } else if (text[at] == ',' || text[at] == ' ' || text[at] == '\n') ++at;
      else return false;
    }
    return at < text.size();
  };
  for (size_t at = 0; (at = text.find("\"fn\": \"", at)) != std::string::npos;) {
    Row r;
    at += 7;
    const size_t end = text.find('"', at);
    if (end == std::string::npos) return false;
    r.fn = text.substr(at, end - at);
    at = end;
    if (!numbers(at, "\"in\":", r.in) || !numbers(at, "\"out\":", r.out)) return false;
    rows.push_back(r);
  }
  return true;
}

static fh::TemporalCallPlan call_plan(const std::vector<u64>& in)
{  // frames, the history's w, h, capacity, moment capacity, same camera; the call's w, h, ids, sample moments; response, response noise, temporal moments
  return fh::temporal_call_plan({(uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], (size_t)in[3], (size_t)in[4], in[5] != 0}, {(uint32_t)in[6], (uint32_t)in[7], in[8] != 0, in[9] != 0},
                                {in[10] != 0, in[11] != 0, in[12] != 0});
}

// one row against the header; false: the row's shape is wrong or a value differs
static bool replay(const Row& r)
{
  const std::vector<u64>& in = r.in;
  const std::vector<u64>& out = r.out;
  if (r.fn == "temporal_call_plan") {
    if (in.size() != 13 || out.size() != 9) return false;
    const fh::TemporalCallPlan p = call_plan(in);
    const u64 got[9] = {p.grow_main, p.grow_moments, p.history_kept, p.with_motion, (u64)p.look, (u64)p.clip, p.mom, p.replace_v, p.still};
    for (int k = 0; k < 9; ++k)
      if (got[k] != out[k]) return false;
    // no table entry that does not exist is ever indexed
    if (p.look < fh::kLookNone || p.look > fh::kLookMotion || p.clip < fh::kClipOff || p.clip > fh::kClipColourNoise || (p.look == fh::kLookNone && p.clip != fh::kClipOff)) return false;
    // What temporal_feed_motion (denoise.hip) relies on: where the record's invariants hold -- a history was committed after an ensure() for its size, and with the
    // moments on that ensure() made the moment image as large as the rest -- "alive" as the feed sees it is "history_kept" as the plan sees it.
    const bool invariants = in[0] == 0 || (in[3] >= in[1] * in[2] && (in[12] == 0 || in[4] >= in[3]));
    const bool alive = in[0] != 0 && in[1] == in[6] && in[2] == in[7];
    return !invariants || alive == p.history_kept;
  }
  if (r.fn == "temporal_feed_plan") {  // fh_set_denoise_motion, alive, floats of h_o2w, of the snapshot's o2w and w2o, of h_w2o, which pair differs (0: none, 1: o2w, 2: w2o), tree built
    if (in.size() != 8 || out.size() != 2) return false;
    const std::vector<float> h_o2w((size_t)in[2], 1.0f), h_w2o((size_t)in[5], 1.0f);
    std::vector<float> o2w((size_t)in[3], 1.0f), w2o((size_t)in[4], 1.0f);  // (exactly the floats the row names: a read past them is the sanitizer's)
    if (in[6] == 1 && !o2w.empty()) o2w.back() = 2.0f;
    if (in[6] == 2 && !w2o.empty()) w2o.back() = 2.0f;
    const fh::TemporalFeedPlan p = fh::temporal_feed_plan(in[0] != 0, in[1] != 0, o2w, w2o, h_o2w, h_w2o, in[7] != 0);
    if ((p.refusal != nullptr) != (out[1] != 0) || (p.refusal && !std::strstr(p.refusal, "the BVH has not been built"))) return false;
    return p.feed_motion == (out[0] != 0);
  }
  return false;  // (a function this program does not know)
}

// the cases the code's own comments state
static void plan_by_hand()
{
  using namespace fh;
  // frames, w, h, capacity, moment capacity, same camera | w, h, ids, sample moments | response, noise, moments
  auto plan = [](std::vector<u64> in) { return call_plan(in); };
  TemporalCallPlan p = plan({0, 0, 0, 40, 0, 0, 8, 5, 0, 1, 1, 1, 0});  // no history: nothing to look up, nothing to clip
  EXPECT(!p.history_kept && p.look == kLookNone && p.clip == kClipOff && !p.grow_main && !p.grow_moments);
  p = plan({3, 8, 5, 40, 0, 1, 8, 5, 0, 1, 0, 0, 0});
  EXPECT(p.history_kept && p.look == kLookOwn && p.clip == kClipOff && p.still && !p.mom && !p.replace_v);
  p = plan({3, 8, 5, 40, 0, 0, 8, 5, 0, 1, 0, 0, 0});
  EXPECT(p.history_kept && p.look == kLookReproject && !p.still);
  p = plan({3, 8, 5, 40, 0, 1, 8, 5, 1, 1, 0, 0, 0});  // ids and a live history
  EXPECT(p.with_motion && p.look == kLookMotion && p.still);
  p = plan({0, 0, 0, 40, 0, 1, 8, 5, 1, 1, 0, 0, 0});  // ids without one: no upload
  EXPECT(!p.with_motion && p.look == kLookNone);
  p = plan({3, 8, 5, 40, 0, 0, 8, 5, 0, 0, 1, 0, 0});
  EXPECT(p.clip == kClipColour);
  p = plan({3, 8, 5, 40, 0, 0, 8, 5, 0, 1, 1, 1, 0});
  EXPECT(p.clip == kClipColourNoise);
  p = plan({3, 8, 5, 40, 0, 0, 8, 5, 0, 0, 1, 1, 0});  // the noise box needs the measured variance
  EXPECT(p.clip == kClipColour);
  p = plan({3, 8, 5, 40, 0, 0, 8, 5, 0, 1, 0, 1, 0});  // ... and the colour box
  EXPECT(p.clip == kClipOff);
  p = plan({3, 8, 5, 40, 40, 0, 8, 5, 0, 0, 0, 0, 1});
  EXPECT(p.history_kept && p.mom && p.replace_v && !p.grow_moments);
  p = plan({3, 8, 5, 40, 40, 0, 8, 5, 0, 1, 0, 0, 1});
  EXPECT(p.mom && !p.replace_v);
  p = plan({3, 8, 5, 40, 0, 1, 5, 8, 0, 1, 1, 0, 0});  // a size change within capacity
  EXPECT(!p.history_kept && !p.grow_main && p.look == kLookNone && p.clip == kClipOff);
  p = plan({3, 16, 10, 160, 0, 1, 8, 5, 1, 1, 0, 0, 0});
  EXPECT(!p.history_kept && !p.grow_main && !p.with_motion);
  p = plan({3, 5, 3, 15, 0, 1, 8, 5, 0, 1, 0, 0, 0});  // a larger frame
  EXPECT(p.grow_main && !p.grow_moments && !p.history_kept && p.look == kLookNone);
  p = plan({3, 8, 5, 40, 0, 1, 8, 5, 0, 1, 0, 0, 1});  // the moments switch on with no moment image
  EXPECT(!p.grow_main && p.grow_moments && !p.history_kept && p.look == kLookNone && p.mom);
  p = plan({0, 0, 0, 15, 15, 1, 8, 5, 0, 1, 0, 0, 1});  // both at once: the moment image is as large as the main buffers will be
  EXPECT(p.grow_main && p.grow_moments);
  const TemporalGrow g = temporal_grow(15, 15, 15, true);
  EXPECT(!g.main && !g.moments);

  const std::vector<float> a(24, 1.0f), none;
  std::vector<float> b(24, 1.0f);
  b[7] = 1.5f;
  EXPECT(!temporal_feed_plan(false, true, b, a, a, a, true).feed_motion);  // the switch is off
  EXPECT(!temporal_feed_plan(true, false, b, a, a, a, true).feed_motion);  // no history at this size
  EXPECT(!temporal_feed_plan(true, true, a, a, a, a, false).feed_motion && !temporal_feed_plan(true, true, a, a, a, a, false).refusal);  // nothing moved: the tree is not needed
  EXPECT(!temporal_feed_plan(true, true, none, none, a, a, true).feed_motion);  // no snapshot
  EXPECT(!temporal_feed_plan(true, true, none, none, none, none, true).feed_motion);  // no instances
  EXPECT(temporal_feed_plan(true, true, b, a, a, a, true).feed_motion && temporal_feed_plan(true, true, a, b, a, a, true).feed_motion);
  const TemporalFeedPlan refused = temporal_feed_plan(true, true, a, b, a, a, false);
  EXPECT(!refused.feed_motion && refused.refusal && !std::strcmp(refused.refusal, "instances moved and the BVH has not been built (fh_set_denoise_motion)"));
  EXPECT(kTemporalDefaults.alpha_min == 0.2f && kTemporalDefaults.max_history == 32.0f && kTemporalDefaults.normal_cos_min == 0.5f && kTemporalDefaults.plane_tol == 0.02f);
}

int main(int argc, char** argv)
{
  if (argc > 2) {
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

  plan_by_hand();
  if (argc < 2) {  // no table given: the checks above are all (the program depends on no file but the header)
    std::printf(failures ? "temporal_host_check: %d failures\n" : "temporal_host_check: ok\n", failures);
    return failures ? 1 : 0;
  }
  std::vector<Row> rows;
  if (!read_rows(argv[1], rows) || rows.size() < 100u) { std::printf("FAILED: cannot read the cases of %s\n", argv[1]); ++failures; }
  for (const char* name : {"temporal_call_plan", "temporal_feed_plan"}) {  // (a table without rows for a function would pass for nothing)
    size_t n = 0;
    for (const Row& r : rows) n += r.fn == name ? 1u : 0u;
    if (!n) { std::printf("FAILED: no case of %s\n", name); ++failures; }
  }
  for (size_t i = 0; i < rows.size(); ++i)
    if (!replay(rows[i])) { std::printf("FAILED case %zu (%s)\n", i, rows[i].fn.c_str()); ++failures; }
  if (failures) std::printf("temporal_host_check: %d failures\n", failures);
  else std::printf("temporal_host_check: ok (%zu cases)\n", rows.size());
  return failures ? 1 : 0;
}
