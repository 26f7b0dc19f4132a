// tools/bvh_plan_check.cpp -- the host-only decisions of the BVH build (fredholm_amd/csrc/bvh_plan_host.h) as a stand-alone program, for the tests and the host
// sanitizers.  From the repository root:
//   g++ -std=c++17 -O1 -Wall -Werror -ffp-contract=off tools/bvh_plan_check.cpp -o bvh_plan_check && ./bvh_plan_check
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/bvh_plan_check.cpp -o bvh_plan_check && ./bvh_plan_check
// Needs no GPU and no library.  (a) the cases the code's own comments state, derived by hand; (b) every row of tests/golden/bvh_plan_cases.json (or of the file given
// as the argument): inputs and what the same lines gave while they were still inside bvh_build_device, equal to the last bit (tools/README.md says how the file was made).
// Every value of the file is an unsigned integer; a double or a float is its IEEE-754 bit pattern, an error code its 32-bit pattern, the value of an environment
// variable its index in `vocab` below.  Prints "bvh_plan_check: ok" or the number of failures.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../fredholm_amd/csrc/bvh_plan_host.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

typedef unsigned long long u64;
static double as_double(u64 bits) { double d; std::memcpy(&d, &bits, 8); return d; }
static float as_float(u64 bits) { const uint32_t u = (uint32_t)bits; float f; std::memcpy(&f, &u, 4); return f; }
static u64 float_bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// values of the environment variables in the table (0: not set)
static const char* const vocab[] = {nullptr, "", "0", "1", "lbvh", "ploc", "auto", "greedy", "optimal", "00", "01", "no"};
static const u64 n_vocab = sizeof vocab / sizeof vocab[0];
// fredholm_hip.h, fh_trace.h, bvh_build.hip
static const int kInvalid = -1, kUnsupported = -3;
static const uint32_t kStack = 48u, kCoopMaxTris = 1u << 26, kLeafMax8 = 3u, kLeafMax2 = 4u, kNodeVec = 4u;
static const char* const limit_msgs[] = {nullptr, "BVH8 collapse lost triangles", "BVH8 deeper than the traversal stack (48 levels)",
                                         "BVH8 with 2^24 or more nodes (the traversal stack keeps node indices in 24 bits)",
                                         "BVH8 with 2^23 or more nodes (the cooperative triangle queue keeps triangle slots in 26 bits)"};

static fh::BuildSwitches no_switches() { return fh::build_switches(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr); }
static fh::BuildSwitches with_builder(const char* v) { return fh::build_switches(nullptr, nullptr, v, nullptr, nullptr, nullptr, nullptr); }

// a scene of large triangles: cells of thr give `at_unit / (thr / thr0)` references, i.e. every doubling of the cells halves them
static int doublings_needed(uint32_t n, uint32_t at_unit, uint32_t* total, int* calls)
{
  float thr = 1.0f;
  *calls = 0;
  fh::split_search(n, &thr, total, [&](float cell, uint32_t* found) { ++*calls; *found = (uint32_t)((float)at_unit / cell); return 0; });
  int d = 0;
  for (float t = 1.0f; t < thr; t *= 2.0f) ++d;
  return d;
}

static void hand_derived()
{
  const fh::BuildSwitches off = no_switches();
  EXPECT(off.refit && off.split && off.builder == 0 && off.absorb && !off.greedy && !off.bvh2 && !off.debug);
  // pad: 2^-16 of the largest coordinate, of 1e-3 for a scene smaller than that; the scene box is the bounds -+ 2 pad
  const float tiny[6] = {-0.5e-3f, 0.0f, 0.0f, 0.25e-3f, 0.5e-3f, 0.0f}, unit[6] = {-1.0f, -0.5f, 0.0f, 0.5f, 1.0f, 0.25f};
  EXPECT(fh::scene_padding(tiny).pad == 1e-3f * (1.0f / 65536.0f));
  EXPECT(fh::scene_padding(unit).pad == 1.0f / 65536.0f);
  EXPECT(fh::scene_padding(unit).lo[0] == -1.0f - 2.0f / 65536.0f && fh::scene_padding(unit).hi[1] == 1.0f + 2.0f / 65536.0f && fh::scene_padding(unit).hi[2] == 0.25f + 2.0f / 65536.0f);
  // splitting: from 256 faces, unless FH_SPLIT=0
  EXPECT(!fh::split_enabled(255u, off) && fh::split_enabled(256u, off));
  EXPECT(!fh::split_enabled(256u, fh::build_switches(nullptr, "0", nullptr, nullptr, nullptr, nullptr, nullptr)));
  EXPECT(fh::split_enabled(256u, fh::build_switches(nullptr, "1", nullptr, nullptr, nullptr, nullptr, nullptr)));
  const float lo[3] = {0.0f, 0.0f, 0.0f}, hi[3] = {16.0f, 64.0f, 32.0f};
  EXPECT(fh::split_cells(lo, hi).thr == 2.0f && fh::split_cells(lo, hi).eps == 64.0f * 1e-6f);
  // at most 1.5 references per face and 4096 more
  EXPECT(fh::split_fits(1000u * 3u / 2u + 4096u, 1000u) && !fh::split_fits(1000u * 3u / 2u + 4097u, 1000u));
  // 1000 large triangles and a limit of 5596 references: 10000 references in the first cells take one doubling, 40000 three, 400000 more than six: no split
  uint32_t total = 0;
  int calls = 0;
  EXPECT(doublings_needed(1000u, 5000u, &total, &calls) == 0 && calls == 1 && total == 5000u);
  EXPECT(doublings_needed(1000u, 10000u, &total, &calls) == 1 && calls == 2 && total == 5000u);
  EXPECT(doublings_needed(1000u, 40000u, &total, &calls) == 3 && calls == 4 && total == 5000u);
  EXPECT(doublings_needed(1000u, 400000u, &total, &calls) == 6 && calls == 6 && total == 1000u);
  EXPECT(doublings_needed(1000u, 5596u * 32u, &total, &calls) == 5 && calls == 6 && total == 5596u);  // (the sixth attempt is the last that counts)
  // an error of the counting ends the search with that error
  float thr = 1.0f;
  EXPECT(fh::split_search(1000u, &thr, &total, [](float, uint32_t*) { return -2; }) == -2);
  // PLOC replaces the radix tree where the sum of its inner-node areas is at least 7 % lower
  const fh::BuilderPlan deciding = fh::builder_plan(0, off);
  EXPECT(deciding.mode == 0 && deciding.deciding && deciding.ploc);
  const double a929[2] = {1000.0, 929.0}, a930[2] = {1000.0, 0.93 * 1000.0}, a931[2] = {1000.0, 931.0};
  EXPECT(fh::builder_verdict(deciding, false, a929).ploc && fh::builder_verdict(deciding, false, a929).choice == 2);
  EXPECT(!fh::builder_verdict(deciding, false, a930).ploc && fh::builder_verdict(deciding, false, a930).choice == 1);
  EXPECT(!fh::builder_verdict(deciding, false, a931).ploc && fh::builder_verdict(deciding, false, a931).choice == 1);
  // every mode of the context x value of FH_BVH_BUILDER x outcome of PLOC: the variable wins where it names a builder; a failed PLOC is the radix tree (and stays
  // the choice) in auto mode and an error under ploc; decided scenes do not decide again
  for (int choice = 0; choice < 3; ++choice)
    for (const char* env : {(const char*)nullptr, "lbvh", "ploc", "auto", ""}) {
      const fh::BuilderPlan p = fh::builder_plan(choice, with_builder(env));
      const int mode = env && !std::strcmp(env, "lbvh") ? 1 : (env && !std::strcmp(env, "ploc") ? 2 : choice);
      EXPECT(p.mode == mode && p.deciding == (mode == 0) && p.ploc == (mode != 1));
      EXPECT(fh::ploc_failure_is_error(p) == (mode != 0));
      for (int failed = 0; failed < 2; ++failed) {
        if (failed && !p.ploc) continue;  // (no PLOC, nothing to fail)
        const fh::BuilderVerdict better = fh::builder_verdict(p, failed != 0, a929), worse = fh::builder_verdict(p, failed != 0, a931);
        if (failed) EXPECT(!better.ploc && better.choice == 1 && !worse.ploc && worse.choice == 1);
        else if (mode == 0) EXPECT(better.ploc && better.choice == 2 && !worse.ploc && worse.choice == 1);
        else EXPECT(better.ploc == (mode == 2) && worse.ploc == (mode == 2) && better.choice == 0 && worse.choice == 0);
      }
    }
  // a refit is kept up to 1.5x the area the tree had when it was built
  EXPECT(fh::refit_accepted(150.0, 100.0) && !fh::refit_accepted(150.00000000000003, 100.0) && fh::refit_accepted(0.0, 0.0));
  EXPECT(fh::refit_eligible(true, true, true, 100u, 100u, off));
  EXPECT(!fh::refit_eligible(false, true, true, 100u, 100u, off) && !fh::refit_eligible(true, false, true, 100u, 100u, off) && !fh::refit_eligible(true, true, false, 100u, 100u, off));
  EXPECT(!fh::refit_eligible(true, true, true, 0u, 0u, off) && !fh::refit_eligible(true, true, true, 100u, 150u, off));
  EXPECT(!fh::refit_eligible(true, true, true, 100u, 100u, fh::build_switches("0", nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)));
  // up to three faces a single wide node, four the binary root alone, five the full pipeline
  EXPECT(fh::tree_shape(0u, kLeafMax8, kLeafMax2) == fh::TreeShape::Empty && fh::tree_shape(1u, kLeafMax8, kLeafMax2) == fh::TreeShape::WideRoot);
  EXPECT(fh::tree_shape(3u, kLeafMax8, kLeafMax2) == fh::TreeShape::WideRoot && fh::tree_shape(4u, kLeafMax8, kLeafMax2) == fh::TreeShape::BinaryRoot);
  EXPECT(fh::tree_shape(5u, kLeafMax8, kLeafMax2) == fh::TreeShape::Full);
  // the collapse: FH_ABSORB=0 and FH_COLLAPSE=greedy
  EXPECT(fh::collapse_plan(off).leaf_max8 == 1u && fh::collapse_plan(off).absorb8 == 1u && fh::collapse_plan(off).optimal_cut);
  EXPECT(fh::collapse_plan(fh::build_switches(nullptr, nullptr, nullptr, "0", nullptr, nullptr, nullptr)).absorb8 == 0u);
  EXPECT(!fh::collapse_plan(fh::build_switches(nullptr, nullptr, nullptr, nullptr, "greedy", nullptr, nullptr)).optimal_cut);
  // each limit at its edge, and their order
  auto limit = [](uint32_t placed, uint32_t nr, uint32_t levels, uint32_t nodes) { return fh::collapse_limits(placed, nr, levels, nodes, kStack, kCoopMaxTris, kInvalid, kUnsupported); };
  EXPECT(limit(1000u, 1000u, 48u, 500u).code == 0 && limit(1000u, 1000u, 48u, 500u).msg == nullptr);
  EXPECT(limit(999u, 1000u, 49u, 1u << 24).code == kInvalid && !std::strcmp(limit(999u, 1000u, 49u, 1u << 24).msg, limit_msgs[1]));
  EXPECT(limit(1000u, 1000u, 49u, 1u << 24).code == kUnsupported && !std::strcmp(limit(1000u, 1000u, 49u, 1u << 24).msg, limit_msgs[2]));
  EXPECT(limit(1000u, 1000u, 48u, 1u << 24).code == kUnsupported && !std::strcmp(limit(1000u, 1000u, 48u, 1u << 24).msg, limit_msgs[3]));
  EXPECT(limit(1000u, 1000u, 48u, (1u << 24) - 1u).code == kUnsupported && !std::strcmp(limit(1000u, 1000u, 48u, (1u << 24) - 1u).msg, limit_msgs[4]));
  EXPECT(limit(1000u, 1000u, 48u, kCoopMaxTris / 8u).code == kUnsupported && !std::strcmp(limit(1000u, 1000u, 48u, kCoopMaxTris / 8u).msg, limit_msgs[4]));
  EXPECT(limit(1000u, 1000u, 48u, kCoopMaxTris / 8u - 1u).code == 0);
  // (with a cooperative queue of 2^28 slots the 24-bit limit is the one that binds)
  EXPECT(fh::collapse_limits(9u, 9u, 1u, (1u << 24) - 1u, kStack, 1u << 28, kInvalid, kUnsupported).code == 0);
  EXPECT(!std::strcmp(fh::collapse_limits(9u, 9u, 1u, 1u << 24, kStack, 1u << 28, kInvalid, kUnsupported).msg, limit_msgs[3]));
  // kept for a refit: no split references, and the level ranges cover the nodes
  EXPECT(fh::tree_refittable(1000u, 1000u, 300u, 300u) && !fh::tree_refittable(1001u, 1000u, 300u, 300u) && !fh::tree_refittable(1000u, 1000u, 299u, 300u));
  // the numbers of fh_stats, with FH_BVH2 on both layouts: 64-byte nodes either way, eight 48-byte triangle slots per wide node
  const fh::BuildSwitches bvh2 = fh::build_switches(nullptr, nullptr, nullptr, nullptr, nullptr, "1", nullptr);
  EXPECT(fh::traverse_wide(true, off) && !fh::traverse_wide(false, off) && !fh::traverse_wide(true, bvh2) && !fh::traverse_wide(false, bvh2));
  const fh::TreeStats wide = fh::tree_stats(true, 300u, 5u, 999u, 1000u, kNodeVec), binary = fh::tree_stats(false, 300u, 5u, 999u, 1000u, kNodeVec);
  EXPECT(wide.nodes == 300u && wide.node_bytes == 64u * 300u && wide.tri_bytes == 48u * 8u * 300u && wide.depth == 5u);
  EXPECT(binary.nodes == 999u && binary.node_bytes == 64u * 999u && binary.tri_bytes == 48u * 1000u && binary.depth == 0u);
}

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

static const char* env_value(u64 code) { return code < n_vocab ? vocab[code] : nullptr; }

// one row against the header; false: the row's shape is wrong or a value differs
static bool replay(const Row& r)
{
  const std::vector<u64>& in = r.in;
  const std::vector<u64>& out = r.out;
  if (r.fn == "build_switches") {  // FH_REFIT, FH_SPLIT, FH_BVH_BUILDER, FH_ABSORB, FH_COLLAPSE, FH_BVH2, FH_DEBUG_BVH
    if (in.size() != 7 || out.size() != 7) return false;
    for (u64 v : in) if (v >= n_vocab) return false;
    const fh::BuildSwitches sw = fh::build_switches(env_value(in[0]), env_value(in[1]), env_value(in[2]), env_value(in[3]), env_value(in[4]), env_value(in[5]), env_value(in[6]));
    return sw.refit == (out[0] != 0) && sw.split == (out[1] != 0) && (u64)sw.builder == out[2] && sw.absorb == (out[3] != 0) && sw.greedy == (out[4] != 0) && sw.bvh2 == (out[5] != 0) && sw.debug == (out[6] != 0);
  }
  if (r.fn == "scene_padding") {
    if (in.size() != 6 || out.size() != 7) return false;
    const float b[6] = {as_float(in[0]), as_float(in[1]), as_float(in[2]), as_float(in[3]), as_float(in[4]), as_float(in[5])};
    const fh::ScenePad s = fh::scene_padding(b);
    return float_bits(s.pad) == out[0] && float_bits(s.lo[0]) == out[1] && float_bits(s.lo[1]) == out[2] && float_bits(s.lo[2]) == out[3] && float_bits(s.hi[0]) == out[4] && float_bits(s.hi[1]) == out[5] &&
           float_bits(s.hi[2]) == out[6];
  }
  if (r.fn == "split_cells") {
    if (in.size() != 6 || out.size() != 2) return false;
    const float lo[3] = {as_float(in[0]), as_float(in[1]), as_float(in[2])}, hi[3] = {as_float(in[3]), as_float(in[4]), as_float(in[5])};
    const fh::SplitCells c = fh::split_cells(lo, hi);
    return float_bits(c.thr) == out[0] && float_bits(c.eps) == out[1];
  }
  if (r.fn == "refit_eligible")
    return in.size() == 6 && out.size() == 1 && in[5] < n_vocab &&
           fh::refit_eligible(in[0] != 0, in[1] != 0, in[2] != 0, (uint32_t)in[3], (uint32_t)in[4], fh::build_switches(env_value(in[5]), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)) == (out[0] != 0);
  if (r.fn == "refit_accepted") return in.size() == 2 && out.size() == 1 && fh::refit_accepted(as_double(in[0]), as_double(in[1])) == (out[0] != 0);
  if (r.fn == "tree_shape") return in.size() == 1 && out.size() == 1 && (u64)fh::tree_shape((uint32_t)in[0], kLeafMax8, kLeafMax2) == out[0];
  if (r.fn == "split_enabled")
    return in.size() == 2 && out.size() == 1 && in[1] < n_vocab && fh::split_enabled((uint32_t)in[0], fh::build_switches(nullptr, env_value(in[1]), nullptr, nullptr, nullptr, nullptr, nullptr)) == (out[0] != 0);
  if (r.fn == "split_search") {  // faces, the first threshold, what the six attempts would count; out: references, the threshold kept, attempts made, split?
    if (in.size() != 8 || out.size() != 4) return false;
    float thr = as_float(in[1]);
    uint32_t total = 0;
    u64 calls = 0;
    const int rc = fh::split_search((uint32_t)in[0], &thr, &total, [&](float, uint32_t* found) { *found = calls < 6 ? (uint32_t)in[2 + calls] : 0u; ++calls; return 0; });
    return rc == 0 && total == out[0] && float_bits(thr) == out[1] && calls == out[2] && (total > (uint32_t)in[0]) == (out[3] != 0);
  }
  if (r.fn == "builder") {  // the context's choice, FH_BVH_BUILDER, FH_DEBUG_BVH set?, a PLOC that runs fails?, the two area sums; out: error, PLOC taken, the context's choice afterwards
    if (in.size() != 6 || out.size() != 3 || in[1] >= n_vocab) return false;
    const fh::BuilderPlan plan = fh::builder_plan((int)in[0], fh::build_switches(nullptr, nullptr, env_value(in[1]), nullptr, nullptr, nullptr, in[2] ? "1" : nullptr));
    const bool failed = plan.ploc && in[3] != 0;
    if (failed && fh::ploc_failure_is_error(plan)) return out[0] == (u64)(uint32_t)kInvalid && out[2] == in[0];
    const double h[2] = {as_double(in[4]), as_double(in[5])};
    const fh::BuilderVerdict v = fh::builder_verdict(plan, failed, h);
    return out[0] == 0 && v.ploc == (out[1] != 0) && (u64)(v.choice ? v.choice : (int)in[0]) == out[2];
  }
  if (r.fn == "collapse_plan") {  // FH_ABSORB, FH_COLLAPSE
    if (in.size() != 2 || out.size() != 3 || in[0] >= n_vocab || in[1] >= n_vocab) return false;
    const fh::CollapsePlan p = fh::collapse_plan(fh::build_switches(nullptr, nullptr, nullptr, env_value(in[0]), env_value(in[1]), nullptr, nullptr));
    return p.leaf_max8 == out[0] && p.absorb8 == out[1] && p.optimal_cut == (out[2] != 0);
  }
  if (r.fn == "collapse_limits") {  // triangles placed, references, levels, nodes; out: the error code, the message (1 .. 4 in the order of the checks, 0 none)
    if (in.size() != 4 || out.size() != 2 || out[1] > 4) return false;
    const fh::BuildError e = fh::collapse_limits((uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], (uint32_t)in[3], kStack, kCoopMaxTris, kInvalid, kUnsupported);
    return (u64)(uint32_t)e.code == out[0] && (out[1] ? e.msg && !std::strcmp(e.msg, limit_msgs[out[1]]) : e.msg == nullptr);
  }
  if (r.fn == "tree_refittable") return in.size() == 4 && out.size() == 1 && fh::tree_refittable((uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], (uint32_t)in[3]) == (out[0] != 0);
  if (r.fn == "tree_stats") {  // wide tree built?, FH_BVH2, wide nodes, levels, binary nodes, binary triangles; out: wide layout traversed?, then the four numbers
    if (in.size() != 6 || out.size() != 5 || in[1] >= n_vocab) return false;
    const bool wide = fh::traverse_wide(in[0] != 0, fh::build_switches(nullptr, nullptr, nullptr, nullptr, nullptr, env_value(in[1]), nullptr));
    const fh::TreeStats s = fh::tree_stats(wide, (uint32_t)in[2], (uint32_t)in[3], (uint32_t)in[4], (uint32_t)in[5], kNodeVec);
    return wide == (out[0] != 0) && s.nodes == out[1] && s.node_bytes == out[2] && s.tri_bytes == out[3] && s.depth == out[4];
  }
  return false;  // (a function this program does not know)
}

int main(int argc, char** argv)
{
  hand_derived();
  std::string path = argc > 1 ? argv[1] : "";
  if (path.empty()) {  // beside this file: ../tests/golden
    path = __FILE__;
    const size_t slash = path.find_last_of('/');
    path = (slash == std::string::npos ? std::string(".") : path.substr(0, slash)) + "/../tests/golden/bvh_plan_cases.json";
  }
  std::vector<Row> rows;
  if (!read_rows(path.c_str(), rows) || rows.size() < 100u) { std::printf("FAILED: cannot read the cases of %s\n", path.c_str()); ++failures; }
  const char* const names[] = {"build_switches", "scene_padding", "split_cells", "refit_eligible", "refit_accepted", "tree_shape", "split_enabled", "split_search", "builder", "collapse_plan",
                               "collapse_limits", "tree_refittable", "tree_stats"};
  for (const char* name : names) {  // (a table without rows for a function would pass for nothing)
    size_t n = 0;
    for (const Row& r : rows) n += r.fn == name ? 1u : 0u;
    if (!n) { std::printf("FAILED: no case of %s\n", name); ++failures; }
  }
  for (size_t i = 0; i < rows.size(); ++i)
    if (!replay(rows[i])) { std::printf("FAILED case %zu (%s)\n", i, rows[i].fn.c_str()); ++failures; }
  if (failures) std::printf("bvh_plan_check: %d failures\n", failures);
  else std::printf("bvh_plan_check: ok (%zu cases)\n", rows.size());
  return failures ? 1 : 0;
}
