// bvh_plan_host.h -- the host-only decisions of the BVH build (bvh_build.hip: bvh_build_device and its steps) as pure functions of plain values: the switches of a
// build, the padding and the scene box, when a tree is refitted and when the refit is kept, which shape a face count gets, the early split clipping's threshold
// search, which binary tree feeds the collapse, the limits of the wide tree, whether it is kept for a refit, and the tree numbers of fh_stats.  Plain C++ without HIP
// like render_plan_host.h, so that it also compiles into a stand-alone program (tools/bvh_plan_check.cpp) for the tests and the host sanitizers.  Every expression
// keeps the integer widths, the order and the floating-point type it had inside bvh_build_device: tests/golden/bvh_plan_cases.json holds what those lines gave.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

namespace fh {

// The developer switches of a build, from the values of their environment variables (null: not set).  Read at the top of EVERY build (bvh_build.hip:
// read_build_switches): the tests set and clear them between builds of one process.
struct BuildSwitches {
  bool refit;    // FH_REFIT=0: every build is a full rebuild
  bool split;    // FH_SPLIT=0: no early split clipping
  int builder;   // FH_BVH_BUILDER: 1 lbvh, 2 ploc, 0 anything else (the context's own choice)
  bool absorb;   // FH_ABSORB=0: plain largest-child-first collapse
  bool greedy;   // FH_COLLAPSE=greedy: the largest-child-first rule instead of the cut of least summed wide-node area
  bool bvh2;     // FH_BVH2 (any value): traverse the binary layout instead of the wide one
  bool debug;    // FH_DEBUG_BVH (any value): the [bvh] lines on stderr, and the area sums they print
};
inline BuildSwitches build_switches(const char* refit, const char* split, const char* builder, const char* absorb, const char* collapse, const char* bvh2, const char* debug)
{
  BuildSwitches sw;
  sw.refit = !(refit && refit[0] == '0');
  sw.split = !(split && split[0] == '0');
  sw.builder = 0;
  if (builder) { if (std::strcmp(builder, "ploc") == 0) sw.builder = 2; else if (std::strcmp(builder, "lbvh") == 0) sw.builder = 1; }
  sw.absorb = absorb ? absorb[0] != '0' : true;
  sw.greedy = collapse && std::strcmp(collapse, "greedy") == 0;
  sw.bvh2 = bvh2 != nullptr;
  sw.debug = debug != nullptr;
  return sw;
}

// Leaf and node boxes are padded by 2^-16 of the largest coordinate of the scene (of 1e-3 for a scene that small); the scene box by twice that.
// b: the decoded bounds of the geometry, min x y z then max x y z.
struct ScenePad { float pad, lo[3], hi[3]; };
inline ScenePad scene_padding(const float b[6])
{
  ScenePad s;
  float maxabs = 0.0f;
  for (int k = 0; k < 6; ++k) maxabs = fmaxf(maxabs, fabsf(b[k]));
  s.pad = fmaxf(maxabs, 1e-3f) * (1.0f / 65536.0f);
  for (int k = 0; k < 3; ++k) { s.lo[k] = b[k] - 2.0f * s.pad; s.hi[k] = b[3 + k] + 2.0f * s.pad; }
  return s;
}

// Instance transforms changed, topology did not: the wide tree is refitted.  A refit whose boxes have grown to more than 1.5x the area the tree had when it was
// built is discarded for a rebuild: the instances have moved too far for the old topology.
inline bool refit_eligible(bool refit_ok, bool use_bvh8, bool have_boxes, uint32_t n, uint32_t bvh8_n_tris, const BuildSwitches& sw)
{
  return refit_ok && use_bvh8 && have_boxes && n && bvh8_n_tris == n && sw.refit;
}
inline bool refit_accepted(double area, double area_built) { return area <= 1.5 * area_built; }

// What a face count builds: nothing; one wide node with a leaf child per face (and the binary root beside it); the binary root alone, whose one leaf holds up to
// leaf_max2 faces; the full pipeline.
enum class TreeShape { Empty, WideRoot, BinaryRoot, Full };
inline TreeShape tree_shape(uint32_t n, uint32_t leaf_max8, uint32_t leaf_max2)
{
  if (n == 0) return TreeShape::Empty;
  if (n <= leaf_max2) return n <= leaf_max8 ? TreeShape::WideRoot : TreeShape::BinaryRoot;
  return TreeShape::Full;
}

// Early split clipping: large triangles enter the build as several boxes, clipped to cells of `thr`, a 32nd of the scene's largest extent.
inline bool split_enabled(uint32_t n, const BuildSwitches& sw) { return n >= 256 && sw.split; }
struct SplitCells { float thr, eps; };
inline SplitCells split_cells(const float scene_lo[3], const float scene_hi[3])
{
  const float extent = fmaxf(fmaxf(scene_hi[0] - scene_lo[0], scene_hi[1] - scene_lo[1]), scene_hi[2] - scene_lo[2]);
  return SplitCells{extent / 32.0f, extent * 1e-6f};
}
inline bool split_fits(uint32_t total, uint32_t n)
{
  const double split_budget = 1.5;  // references per face the split may produce at most
  return (unsigned long long)total <= (unsigned long long)((double)n * split_budget) + 4096ull;
}
// A scene made of large triangles only: coarser cells, six attempts, until the references fit.  count(thr, &total): the references that cells of thr give (the
// kernels and the read-back in the library, a model in the check program); nonzero: its error, which ends the search.  *total > n: split with *thr; a search that
// failed leaves *total = n, no split references.
template <typename Count>
inline int split_search(uint32_t n, float* thr, uint32_t* total, Count&& count)
{
  *total = n;
  for (int attempt = 0; attempt < 6; ++attempt, *thr *= 2.0f) {
    if (const int rc = count(*thr, total)) return rc;
    if (split_fits(*total, n)) break;
    *total = n;
  }
  return 0;
}

// Which binary tree the collapse takes.  mode 1: the radix tree, 2: PLOC, 0 (auto): the first build after an upload makes both and keeps PLOC when the sum of its
// inner-node areas is at least 7 % below the radix tree's; later builds of the same scene reuse the choice (fh_ctx::builder_choice).
struct BuilderPlan { int mode; bool deciding, ploc; };
inline BuilderPlan builder_plan(int builder_choice, const BuildSwitches& sw)
{
  const int mode = sw.builder ? sw.builder : builder_choice;
  const bool deciding = mode == 0;
  return BuilderPlan{mode, deciding, mode == 2 || deciding};
}
// a PLOC that made no progress or did not end in one inner node: in auto mode the radix tree is still valid, an explicit ploc reports the error
inline bool ploc_failure_is_error(const BuilderPlan& plan) { return !plan.deciding; }
// h: the sums of the inner-node areas, radix tree then PLOC (read only while deciding).  choice: the new fh_ctx::builder_choice, 0: it stays
struct BuilderVerdict { bool ploc; int choice; };
inline BuilderVerdict builder_verdict(const BuilderPlan& plan, bool ploc_failed, const double h[2])
{
  if (ploc_failed) return BuilderVerdict{false, 1};
  if (!plan.deciding) return BuilderVerdict{plan.ploc, 0};
  const bool ploc = h[1] < 0.93 * h[0];
  return BuilderVerdict{ploc, ploc ? 2 : 1};
}

struct CollapsePlan { uint32_t leaf_max8, absorb8; bool optimal_cut; };
inline CollapsePlan collapse_plan(const BuildSwitches& sw)
{
  const uint32_t leaf_max8 = 1;  // one triangle per leaf child (the node layout has one triangle slot per child slot): box tests are ~4x cheaper than triangle tests (profiles/README.md)
  return CollapsePlan{leaf_max8, sw.absorb ? 1u : 0u, leaf_max8 == 1 && !sw.greedy};
}

// What the collapse must not exceed, in the order the checks are made.  code 0: within the limits.  invalid / unsupported: FH_E_INVALID / FH_E_UNSUPPORTED;
// stack_levels, coop_max_tris: kBvh8Stack, kCoopMaxTris of fh_trace.h.
struct BuildError { int code; const char* msg; };
inline BuildError collapse_limits(uint32_t tris_placed, uint32_t nr, uint32_t levels, uint32_t nodes, uint32_t stack_levels, uint32_t coop_max_tris, int invalid, int unsupported)
{
  if (tris_placed != nr) return BuildError{invalid, "BVH8 collapse lost triangles"};
  if (levels > stack_levels) return BuildError{unsupported, "BVH8 deeper than the traversal stack (48 levels)"};
  if (nodes >= (1u << 24)) return BuildError{unsupported, "BVH8 with 2^24 or more nodes (the traversal stack keeps node indices in 24 bits)"};
  if (nodes >= coop_max_tris / 8u) return BuildError{unsupported, "BVH8 with 2^23 or more nodes (the cooperative triangle queue keeps triangle slots in 26 bits)"};
  return BuildError{0, nullptr};
}

// Split references carry clipped boxes that a moved triangle no longer has, so scenes that use them are rebuilt instead of refitted; and the level ranges must
// cover the nodes (a collapse cut off at 64 levels does not).
inline bool tree_refittable(uint32_t nr, uint32_t n, uint32_t level_end, uint32_t nodes) { return nr == n && level_end == nodes; }

// the layout the rays traverse: the wide one where it was built, unless FH_BVH2 asks for the binary one
inline bool traverse_wide(bool built_wide, const BuildSwitches& sw) { return built_wide && !sw.bvh2; }
// the tree numbers of fh_stats for the layout that is traversed (wide tree: node_vec 16-byte vectors per node and eight triangle slots per node)
struct TreeStats { unsigned long long nodes, node_bytes, tri_bytes, depth; };
inline TreeStats tree_stats(bool use_bvh8, uint32_t bvh8_n_nodes, uint32_t bvh8_depth, uint32_t bvh2_n_nodes, uint32_t bvh2_n_tris, uint32_t node_vec)
{
  TreeStats s;
  s.nodes = use_bvh8 ? bvh8_n_nodes : bvh2_n_nodes;
  s.node_bytes = use_bvh8 ? 16ull * node_vec * bvh8_n_nodes : 64ull * bvh2_n_nodes;
  s.tri_bytes = use_bvh8 ? 48ull * 8ull * bvh8_n_nodes : 48ull * bvh2_n_tris;
  s.depth = use_bvh8 ? bvh8_depth : 0;
  return s;
}

}  // namespace fh
