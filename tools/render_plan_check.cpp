// tools/render_plan_check.cpp -- the host-only decisions of fh_render's submit path (fredholm_amd/csrc/render_plan_host.h) as a stand-alone program, for the tests and
// the host sanitizers.  From the repository root:
//   g++ -std=c++17 -O1 -Wall -Werror -ffp-contract=off tools/render_plan_check.cpp -o render_plan_check && ./render_plan_check
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/render_plan_check.cpp -o render_plan_check && ./render_plan_check
// Needs no GPU and no library.  (a) the cases the code's own comments state, derived by hand; (b) every row of tests/golden/render_plan_cases.json (or of the file given
// as the argument): inputs and what the same lines gave while they were still inside render_submit, equal to the last bit (tools/README.md says how the file was made).
// Every value of the file is an unsigned integer; a double or a float is its IEEE-754 bit pattern.  Prints "render_plan_check: ok" or the number of failures.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../fredholm_amd/csrc/render_plan_host.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

typedef unsigned long long u64;
static double as_double(u64 bits) { double d; std::memcpy(&d, &bits, 8); return d; }
static float as_float(u64 bits) { const uint32_t u = (uint32_t)bits; float f; std::memcpy(&f, &u, 4); return f; }
static u64 double_bits(double d) { u64 b; std::memcpy(&b, &d, 8); return b; }
static u64 float_bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

static uint32_t passes_of(uint32_t n_samples, uint32_t batch) { return (n_samples + batch - 1u) / batch; }

static void hand_derived()
{
  // 1024 samples with room for 248 per pass and three slots: six passes of 171, not four of 248 and a runt
  EXPECT(fh::samples_per_pass(248u * 2073600u, 2073600u, 1024u, 3u, false, false) == 171u);
  EXPECT(fh::samples_per_pass(248u * 3072u, 3072u, 1024u, 1u, false, false) == 205u);  // (one slot: five equal passes)
  // a call that fits one pass, of at least 3 * 2^24 paths and n_samples >= n_slots, is cut into n_slots passes -- unless its passes run one after the other anyway.
  // 1080p x 26 (tests/test_gpu_parity.py: test_large_one_pass_calls...): the default pool of 32 Mi paths holds 16 samples per pixel, two passes are what the call needs
  // and three is the cut for overlap; measuring mode and bug-compat mode keep the two; bug-compat with a pool of two samples per pixel runs thirteen
  const uint32_t px = 1920u * 1080u;
  EXPECT(passes_of(26u, fh::samples_per_pass(1u << 25, px, 26u, 3u, false, false)) == 3u);
  EXPECT(passes_of(26u, fh::samples_per_pass(1u << 25, px, 26u, 3u, false, true)) == 2u);
  EXPECT(passes_of(26u, fh::samples_per_pass(1u << 25, px, 26u, 3u, true, false)) == 2u);
  EXPECT(passes_of(26u, fh::samples_per_pass(px * 2u, px, 26u, 3u, true, false)) == 13u);
  EXPECT(fh::samples_per_pass(px * 26u, px, 26u, 3u, false, false) == 9u);           // (room for all 26: cut into three all the same)
  EXPECT(fh::samples_per_pass(px * 26u, px, 26u, 3u, true, false) == 26u);
  EXPECT(fh::samples_per_pass(px * 26u, px, 26u, 3u, false, true) == 26u);
  EXPECT(fh::samples_per_pass(px * 26u, px, 2u, 3u, false, false) == 2u);            // (fewer samples than slots)
  EXPECT(fh::samples_per_pass(px * 24u, px, 24u, 3u, false, false) == 24u);          // (under 3 * 2^24 paths)
  EXPECT(fh::samples_per_pass(px * 25u, px, 25u, 3u, false, false) == 9u);           // (25 x 1080p is above)
  // the batch is clamped to 65535: k_generate's grid has one row per sample of the pass
  EXPECT(fh::samples_per_pass(0xffffffffu, 16u, 100000u, 1u, false, false) == 50000u);  // (two equal passes, not 65535 and a runt)
  EXPECT(fh::samples_per_pass(0xffffffffu, 16u, 65535u, 1u, false, false) == 65535u);
  EXPECT(fh::samples_per_pass(0xffffffffu, 0u, 70000u, 1u, false, false) == 35000u);
  EXPECT(fh::samples_per_pass(0xffffffffu, 1u, 131070u, 3u, true, false) == 65535u);
  // nothing known about the scene: a big pass runs without the tail, a small one hands over after two bounces
  uint32_t picked = 0;
  EXPECT(fh::tail_wave_depth(nullptr, 0u, (1u << 22) + 1u, 65536u, 7u, 0u, 0u, &picked) == 7u && picked == 7u);
  EXPECT(fh::tail_wave_depth(nullptr, 0u, 1u << 22, 262144u, 7u, 0u, 0u, &picked) == 2u && picked == 2u);
  EXPECT(fh::tail_wave_depth(nullptr, 0u, 1u << 22, 262144u, 1u, 0u, 0u, &picked) == 1u && picked == 2u);  // (the clamp to max_depth)
  // the extrapolation beyond the last depth counted takes 1 .. 16 steps
  const double slow[3] = {1.0, 0.999, 0.998}, halves[2] = {1.0, 0.5}, flat[2] = {1.0, 1.0};
  EXPECT(fh::tail_wave_depth(slow, 3u, 1u << 25, 65536u, 64u, 0u, 0u, &picked) == 18u && picked == 2u + 16u);
  EXPECT(fh::tail_wave_depth(halves, 2u, 1u << 20, 70000u, 64u, 0u, 0u, &picked) == 4u && picked == 1u + 3u);  // (2^19 survivors at depth 1, under 70000 three halvings later)
  EXPECT(fh::tail_wave_depth(halves, 2u, 1u << 17, 65536u, 64u, 0u, 0u, &picked) == 1u && picked == 1u);       // (found in the curve: no extrapolation)
  EXPECT(fh::tail_wave_depth(flat, 2u, 1u << 20, 65536u, 64u, 0u, 0u, &picked) == 2u && picked == 1u + 1u);    // (no ratio to go by: one step)
  EXPECT(fh::tail_wave_depth(halves, 2u, 1u << 20, 70000u, 64u, 6u, 0u, &picked) == 6u && picked == 4u);       // (the context's depth ...)
  EXPECT(fh::tail_wave_depth(halves, 2u, 1u << 20, 70000u, 64u, 6u, 9u, &picked) == 9u && picked == 4u);       // (... and the environment's over it)
  // where rays start: no verdict under 65536 items on either side, the face's node only where it is at least 5 % cheaper
  const double it_few[2] = {65535.0, 1.0e6}, it_few2[2] = {1.0e6, 65535.0}, it[2] = {65536.0, 65536.0};
  const double c_on[2] = {65536.0 * 100.0, 65536.0 * 94.0}, c_edge[2] = {65536.0 * 100.0, 65536.0 * 95.0}, c_off[2] = {65536.0 * 100.0, 65536.0 * 120.0};
  EXPECT(fh::bottom_up_verdict(c_on, it_few) == 0 && fh::bottom_up_verdict(c_on, it_few2) == 0);
  EXPECT(fh::bottom_up_verdict(c_on, it) == 2);
  EXPECT(fh::bottom_up_verdict(c_edge, it) == 1);
  EXPECT(fh::bottom_up_verdict(c_off, it) == 1);
  // the shares alive per depth, from counter snapshots of 16 words per bounce whose word 0 is the bounce's radiance-queue entries: a snapshot of wave depth 7 fills
  // entries 0 .. 7; one of wave depth 2 after it overwrites entries 0 .. 2 only and does not shorten what is known
  {
    std::vector<uint32_t> deep(8 * 16, 0u), shallow(3 * 16, 0u), none(6 * 16, 77u), full(66 * 16, 0u);
    for (uint32_t d = 0; d < 8u; ++d) deep[d * 16u] = 1024u >> d;
    for (uint32_t d = 0; d < 3u; ++d) shallow[d * 16u] = 300u - 100u * d;
    double sv[66] = {};
    uint32_t n = fh::fold_survival(deep.data(), 16u, 0u, 7u, 1024u, sv, 0u);
    EXPECT(n == 8u);
    for (uint32_t d = 0; d < 8u; ++d) EXPECT(sv[d] == 1.0 / (double)(1u << d));
    EXPECT(sv[8] == 0.0);
    n = fh::fold_survival(shallow.data(), 16u, 0u, 2u, 400u, sv, n);
    EXPECT(n == 8u && sv[0] == 0.75 && sv[1] == 0.5 && sv[2] == 0.25);
    for (uint32_t d = 3; d < 8u; ++d) EXPECT(sv[d] == 1.0 / (double)(1u << d));
    // a snapshot of a pass that started no paths changes nothing
    double before[66];
    std::memcpy(before, sv, sizeof sv);
    EXPECT(fh::fold_survival(none.data(), 16u, 0u, 5u, 0u, sv, n) == 8u && std::memcmp(before, sv, sizeof sv) == 0);
    // a wave depth above 65 is capped: 66 entries, the table's size (the snapshot buffer holds 66 bounces)
    for (uint32_t d = 0; d < 66u; ++d) full[d * 16u] = 66u - d;
    double capped[66] = {};
    EXPECT(fh::fold_survival(full.data(), 16u, 0u, 1000u, 66u, capped, 0u) == 66u && capped[0] == 1.0 && capped[65] == 1.0 / 66.0);
    EXPECT(fh::fold_survival(full.data(), 16u, 0u, 65u, 66u, capped, 3u) == 66u && fh::fold_survival(full.data(), 16u, 0u, 64u, 66u, capped, 3u) == 65u);
  }
  // the probe cost of a two-bounce table: 510 cycles per node-test round (word 12), 175 per triangle-test round (word 13), per shaded path with secondary rays (word 1);
  // added to what the side has already, and a third bounce in the buffer that the pass did not run as a wavefront is not counted
  {
    std::vector<uint32_t> t(3 * 16, 0u);
    t[12] = 10u; t[13] = 4u; t[1] = 100u;
    t[16 + 12] = 3u; t[16 + 13] = 2u; t[16 + 1] = 50u;
    t[32 + 12] = 999u; t[32 + 13] = 999u; t[32 + 1] = 999u;
    double cost = 1000.0, items = 7.0;
    fh::fold_probe_cost(t.data(), 16u, 12u, 13u, 1u, 2u, &cost, &items);
    EXPECT(cost == 1000.0 + (510.0 * 10.0 + 175.0 * 4.0) + (510.0 * 3.0 + 175.0 * 2.0) && cost == 8680.0 && items == 157.0);
    fh::fold_probe_cost(t.data(), 16u, 12u, 13u, 1u, 0u, &cost, &items);  // (no wavefront bounce: nothing)
    EXPECT(cost == 8680.0 && items == 157.0);
  }
  // the pools together stay within a quarter of the free memory; never under one path per owned pixel; the default where it fits
  EXPECT(fh::pool_target_cap(12ull << 30, 0ull, 1u, 3, 256ull, 1u << 25, 3072u) == (1u << 22));
  EXPECT(fh::pool_target_cap(1ull << 20, 0ull, 1u, 3, 256ull, 1u << 25, 3072u) == 3072u);
  EXPECT(fh::pool_target_cap(200ull << 30, 0ull, 1u, 3, 256ull, 1u << 25, 3072u) == (1u << 25));
  // the chunk words: the adaptive maximum rides in the high half, only where it is above the chunk itself
  EXPECT(fh::stream_chunk_max(false, 64u, 100u) == 256u && fh::stream_chunk_max(false, 64u, 4095u) == 128u && fh::stream_chunk_max(false, 64u, 4096u) == 64u && fh::stream_chunk_max(true, 64u, 100u) == 64u);
  EXPECT(fh::stream_chunk_word(64u, 256u) == (64u | 256u << 16) && fh::stream_chunk_word(128u, 128u) == 128u);
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

// one row against the header; false: the row's shape is wrong or a value differs
static bool replay(const Row& r)
{
  const std::vector<u64>& in = r.in;
  const std::vector<u64>& out = r.out;
  if (r.fn == "pool_target_cap")
    return in.size() == 7 && out.size() == 1 && fh::pool_target_cap(in[0], in[1], (uint32_t)in[2], (int)in[3], in[4], (uint32_t)in[5], (uint32_t)in[6]) == out[0];
  if (r.fn == "samples_per_pass")
    return in.size() == 6 && out.size() == 1 && fh::samples_per_pass((uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], (uint32_t)in[3], in[4] != 0, in[5] != 0) == out[0];
  if (r.fn == "stream_lds_entries") {  // ..., then the occupancy the runtime would report for 0, 1, ... entries in LDS (an int as its 32-bit pattern)
    if (in.size() < 6 || in.size() != 6 + in[5] || out.size() != 2) return false;
    bool inside = true;
    const fh::StreamLds got = fh::stream_lds_entries((uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], (uint32_t)in[3], (uint32_t)in[4], [&](uint32_t entries) {
      if (entries >= in[5]) { inside = false; return 0; }
      return (int)(uint32_t)in[6 + entries];
    });
    return inside && got.entries == out[0] && got.blocks == out[1];
  }
  if (r.fn == "stream_wgs")
    return in.size() == 6 && out.size() == 1 && fh::stream_wgs((uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], (uint32_t)in[3], (uint32_t)in[4], (uint32_t)in[5]) == out[0];
  if (r.fn == "stream_chunk") {  // FH_STREAM_CHUNK given?, the chunk, the closest-hit launch's own chunk (0: the same), nodes of the tree
    if (in.size() != 4 || out.size() != 3) return false;
    const uint32_t chunk = (uint32_t)in[1], chunk_max = fh::stream_chunk_max(in[0] != 0, chunk, (uint32_t)in[3]), closest = in[2] ? (uint32_t)in[2] : chunk;
    return chunk_max == out[0] && fh::stream_chunk_word(chunk, chunk_max) == out[1] && fh::stream_chunk_word(closest, chunk_max) == out[2];
  }
  if (r.fn == "tail_wave_depth") {  // ..., then the survival curve
    if (in.size() < 6 || in.size() != 6 + in[5] || in[5] > 66 || out.size() != 2) return false;
    double survival[66] = {};
    for (u64 d = 0; d < in[5]; ++d) survival[d] = as_double(in[6 + d]);
    uint32_t picked = 0;
    const uint32_t depth = fh::tail_wave_depth(survival, (uint32_t)in[5], (uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], (uint32_t)in[3], (uint32_t)in[4], &picked);
    return depth == out[0] && picked == out[1];
  }
  if (r.fn == "bottom_up_verdict") {
    if (in.size() != 4 || out.size() != 1) return false;
    const double cost[2] = {as_double(in[0]), as_double(in[1])}, items[2] = {as_double(in[2]), as_double(in[3])};
    return (u64)fh::bottom_up_verdict(cost, items) == out[0];
  }
  if (r.fn == "fold_survival") {  // stride, index of the radiance word, wave depth, paths, survival_n, the counter words (their number first), the 66 shares; out: survival_n, the 66 shares
    if (in.size() < 6 || in.size() != 6 + in[5] + 66 || in[4] > 66 || out.size() != 67) return false;
    const std::vector<uint32_t> counters(in.begin() + 6, in.begin() + 6 + (long)in[5]);  // (exactly the words the row holds: a read past them is the sanitizer's)
    std::vector<double> survival(66);
    for (size_t d = 0; d < 66; ++d) survival[d] = as_double(in[6 + in[5] + d]);
    bool same = fh::fold_survival(counters.data(), (uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], (uint32_t)in[3], survival.data(), (uint32_t)in[4]) == out[0];
    for (size_t d = 0; d < 66; ++d) same = same && double_bits(survival[d]) == out[1 + d];
    return same;
  }
  if (r.fn == "fold_probe_cost") {  // stride, indices of the node-round, triangle-round and shaded-path words, wave depth, cost and items so far, the counter words (their number first)
    if (in.size() < 8 || in.size() != 8 + in[7] || out.size() != 2) return false;
    const std::vector<uint32_t> counters(in.begin() + 8, in.end());
    double cost = as_double(in[5]), items = as_double(in[6]);
    fh::fold_probe_cost(counters.data(), (uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], (uint32_t)in[3], (uint32_t)in[4], &cost, &items);
    return double_bits(cost) == out[0] && double_bits(items) == out[1];
  }
  if (r.fn == "lens_values") {
    if (in.size() != 3 || out.size() != 2) return false;
    float apb = 0.0f, lr = 0.0f;
    fh::lens_values(as_float(in[0]), as_float(in[1]), as_float(in[2]), &apb, &lr);
    return float_bits(apb) == out[0] && float_bits(lr) == out[1];
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
    path = (slash == std::string::npos ? std::string(".") : path.substr(0, slash)) + "/../tests/golden/render_plan_cases.json";
  }
  std::vector<Row> rows;
  if (!read_rows(path.c_str(), rows) || rows.size() < 100u) { std::printf("FAILED: cannot read the cases of %s\n", path.c_str()); ++failures; }
  const char* const names[] = {"pool_target_cap", "samples_per_pass", "stream_lds_entries", "stream_wgs", "stream_chunk", "tail_wave_depth", "fold_survival", "fold_probe_cost", "bottom_up_verdict", "lens_values"};
  for (const char* name : names) {  // (a table without rows for a function would pass for nothing)
    size_t n = 0;
    for (const Row& r : rows) n += r.fn == name ? 1u : 0u;
    if (!n) { std::printf("FAILED: no case of %s\n", name); ++failures; }
  }
  for (size_t i = 0; i < rows.size(); ++i)
    if (!replay(rows[i])) { std::printf("FAILED case %zu (%s)\n", i, rows[i].fn.c_str()); ++failures; }
  if (failures) std::printf("render_plan_check: %d failures\n", failures);
  else std::printf("render_plan_check: ok (%zu cases)\n", rows.size());
  return failures ? 1 : 0;
}
