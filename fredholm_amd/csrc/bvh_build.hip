// bvh_build.hip -- on-device BVH construction.
//
// Replaces Renderer::build_gas / build_ias (fredholm/include/fredholm/renderer.h:434-552), i.e. the
// closed-source optixAccelBuild.  Pipeline, all on the context stream:
//   1. per-face world-space bounds + scene bounds              (k_face_bounds)
//   2. 63-bit Morton code of the box centre                    (k_morton)
//   3. rocPRIM radix sort of (code, face)                      (sort)
//   4. Karras 2012 radix-tree hierarchy, one thread per node   (k_hierarchy)
//   5. bottom-up box refit with arrival counters               (k_refit)
//   6. emit the traversal layout: 64-byte two-child nodes whose children are inner nodes or leaves of
//      <= 4 Morton-contiguous triangles, and the triangle array in leaf order (k_emit2 / k_emit_tris)
//   6a. optionally PLOC instead of the radix tree (chosen per scene by summed inner-node area) and (round 5, measured and taken out: tools/patches) SAH refinement by parallel reinsertion (FH_SAH_ITERS; off: it lowers
//      the area and not the visits, profiles/README.md r5-1)
//   7. collapse to the 8-wide quantised layout the traversal kernels prefer (bvh8 section), with the way up -- per wide node parent << 3 | child slot, per face the node
//      that holds it (also written into the face record) -- for rays that start at their face (fh_trace.h)
// Triangle order is the Morton order, so leaf reads are contiguous 48-byte records.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include <rocprim/rocprim.hpp>

#include <chrono>
#include <cstdlib>

#include "bvh_plan_host.h"
#include "context.h"
#include "fh_trace.h"

namespace fh {

namespace {

constexpr uint32_t kLeafMax2 = 4;

__device__ __forceinline__ int float_order(float f)
{
  const int i = __float_as_int(f);
  return i >= 0 ? i : i ^ 0x7fffffff;
}
__host__ __device__ __forceinline__ float order_float(int i)
{
  const int j = i >= 0 ? i : i ^ 0x7fffffff;
  float f;
  memcpy(&f, &j, 4);
  return f;
}

// bounds[0..2] = min (ordered ints), bounds[3..5] = max
__global__ void k_face_bounds(const float4* face_rec, uint32_t n, float4* lo, float4* hi, int* bounds)
{
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  float l[3] = {3e38f, 3e38f, 3e38f}, h[3] = {-3e38f, -3e38f, -3e38f};
  if (f < n) {
    const float4 a = face_rec[kFaceRec * (size_t)f], b = face_rec[kFaceRec * (size_t)f + 1], c = face_rec[kFaceRec * (size_t)f + 2];
    l[0] = fminf(a.x, fminf(b.x, c.x)); l[1] = fminf(a.y, fminf(b.y, c.y)); l[2] = fminf(a.z, fminf(b.z, c.z));
    h[0] = fmaxf(a.x, fmaxf(b.x, c.x)); h[1] = fmaxf(a.y, fmaxf(b.y, c.y)); h[2] = fmaxf(a.z, fmaxf(b.z, c.z));
    lo[f] = make_float4(l[0], l[1], l[2], 0.0f);
    hi[f] = make_float4(h[0], h[1], h[2], 0.0f);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float mn = l[k], mx = h[k];
    for (int off = 32; off > 0; off >>= 1) {
      mn = fminf(mn, __shfl_xor(mn, off));
      mx = fmaxf(mx, __shfl_xor(mx, off));
    }
    if ((threadIdx.x & 63) == 0) {
      atomicMin(&bounds[k], float_order(mn));
      atomicMax(&bounds[3 + k], float_order(mx));
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Early split clipping (Ernst & Greiner, "Early Split Clipping for Bounding Volume Hierarchies", RT 2007).  A triangle that is
// large against the scene (a floor, a wall, a cable) has a bounding box that most rays enter without coming near the triangle.
// Such a triangle enters the build as several REFERENCES instead: its box is cut into a grid along its two longest axes, the
// triangle is clipped to every cell and each non-empty cell becomes a leaf with the tight box of the clipped polygon.  All
// references of a face store the same triangle; a ray that meets two of them computes the identical (t, face) pair, which the
// closest-hit order treats as one hit.  Faces below the size threshold keep their single box, so a scene without large triangles
// (the bench soup) builds exactly as before.
// ------------------------------------------------------------------------------------------------
constexpr int kMaxSplitCells = 64;  // references per face at most

struct SplitGrid { int a, b, ka, kb; };  // axes (a = longest) and cells per axis

__device__ __forceinline__ float axis_of(const float4& v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }

__device__ inline SplitGrid split_grid(const float4& lo, const float4& hi, float thr)
{
  const float e[3] = {hi.x - lo.x, hi.y - lo.y, hi.z - lo.z};
  int a = 0;
  if (e[1] > e[a]) a = 1;
  if (e[2] > e[a]) a = 2;
  int b = (a + 1) % 3;
  const int c = (a + 2) % 3;
  if (e[c] > e[b]) b = c;
  SplitGrid g{a, b, 1, 1};
  if (!(e[a] > thr)) return g;
  float fa = ceilf(e[a] / thr), fb = e[b] > thr ? ceilf(e[b] / thr) : 1.0f;
  while (fa * fb > (float)kMaxSplitCells) { if (fa >= fb) fa = ceilf(fa * 0.5f); else fb = ceilf(fb * 0.5f); }
  g.ka = (int)fa; g.kb = (int)fb;
  return g;
}

// clip the polygon (<= 8 vertices) against the half-space  sign * (p[axis] - plane) >= 0
__device__ inline int clip_poly(float (*p)[3], int n, int axis, float plane, float sign)
{
  float out[9][3];
  int m = 0;
  for (int i = 0; i < n; ++i) {
    const float* cur = p[i];
    const float* nxt = p[(i + 1) % n];
    const float dc = sign * (cur[axis] - plane), dn = sign * (nxt[axis] - plane);
    if (dc >= 0.0f) { out[m][0] = cur[0]; out[m][1] = cur[1]; out[m][2] = cur[2]; ++m; }
    if ((dc >= 0.0f) != (dn >= 0.0f)) {
      const float t = dc / (dc - dn);
      out[m][0] = cur[0] + t * (nxt[0] - cur[0]); out[m][1] = cur[1] + t * (nxt[1] - cur[1]); out[m][2] = cur[2] + t * (nxt[2] - cur[2]);
      out[m][axis] = plane;
      ++m;
    }
  }
  for (int i = 0; i < m; ++i) { p[i][0] = out[i][0]; p[i][1] = out[i][1]; p[i][2] = out[i][2]; }
  return m;
}

// box of the part of triangle (v0, v1, v2) inside cell (i, j) of the grid; false if the cell is empty
__device__ inline bool split_cell_box(const float4& v0, const float4& v1, const float4& v2, const float4& lo, const float4& hi, const SplitGrid& g, int i, int j, float eps,
                                      float4& clo, float4& chi)
{
  float poly[9][3] = {{v0.x, v0.y, v0.z}, {v1.x, v1.y, v1.z}, {v2.x, v2.y, v2.z}};
  int n = 3;
  const float la = axis_of(lo, g.a), ha = axis_of(hi, g.a), lb = axis_of(lo, g.b), hb = axis_of(hi, g.b);
  const float a0 = la + (ha - la) * ((float)i / (float)g.ka), a1 = i + 1 == g.ka ? ha : la + (ha - la) * ((float)(i + 1) / (float)g.ka);
  const float b0 = lb + (hb - lb) * ((float)j / (float)g.kb), b1 = j + 1 == g.kb ? hb : lb + (hb - lb) * ((float)(j + 1) / (float)g.kb);
  n = clip_poly(poly, n, g.a, a0, 1.0f); if (n < 3) return false;
  n = clip_poly(poly, n, g.a, a1, -1.0f); if (n < 3) return false;
  if (g.kb > 1) {
    n = clip_poly(poly, n, g.b, b0, 1.0f); if (n < 3) return false;
    n = clip_poly(poly, n, g.b, b1, -1.0f); if (n < 3) return false;
  }
  float mn[3] = {3e38f, 3e38f, 3e38f}, mx[3] = {-3e38f, -3e38f, -3e38f};
  for (int k = 0; k < n; ++k)
    for (int c = 0; c < 3; ++c) { mn[c] = fminf(mn[c], poly[k][c]); mx[c] = fmaxf(mx[c], poly[k][c]); }
  // a little slack for the rounding of the clip points, but never beyond the triangle's own box
  clo = make_float4(fmaxf(mn[0] - eps, lo.x), fmaxf(mn[1] - eps, lo.y), fmaxf(mn[2] - eps, lo.z), 0.0f);
  chi = make_float4(fminf(mx[0] + eps, hi.x), fminf(mx[1] + eps, hi.y), fminf(mx[2] + eps, hi.z), 0.0f);
  return true;
}

// pass 1: references per face (1 = unsplit)
__global__ void k_split_count(const float4* face_rec, const float4* face_lo, const float4* face_hi, uint32_t n, float thr, float eps, uint32_t* count)
{
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n) return;
  const float4 lo = face_lo[f], hi = face_hi[f];
  const SplitGrid g = split_grid(lo, hi, thr);
  uint32_t c = 1;
  if (g.ka * g.kb > 1) {
    const float4 v0 = face_rec[kFaceRec * (size_t)f], v1 = face_rec[kFaceRec * (size_t)f + 1], v2 = face_rec[kFaceRec * (size_t)f + 2];
    c = 0;
    float4 a, b;
    for (int i = 0; i < g.ka; ++i)
      for (int j = 0; j < g.kb; ++j)
        if (split_cell_box(v0, v1, v2, lo, hi, g, i, j, eps, a, b)) ++c;
    if (c == 0) c = 1;  // degenerate triangle: keep its box
  }
  count[f] = c;
}

// pass 2: write the references
__global__ void k_split_emit(const float4* face_rec, const float4* face_lo, const float4* face_hi, uint32_t n, float thr, float eps, const uint32_t* count, const uint32_t* offset,
                             uint32_t* ref_face, float4* ref_lo, float4* ref_hi)
{
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n) return;
  const float4 lo = face_lo[f], hi = face_hi[f];
  uint32_t o = offset[f];
  const SplitGrid g = split_grid(lo, hi, thr);
  if (g.ka * g.kb > 1 && count[f] > 0) {
    const float4 v0 = face_rec[kFaceRec * (size_t)f], v1 = face_rec[kFaceRec * (size_t)f + 1], v2 = face_rec[kFaceRec * (size_t)f + 2];
    uint32_t written = 0;
    float4 a, b;
    for (int i = 0; i < g.ka; ++i)
      for (int j = 0; j < g.kb; ++j)
        if (split_cell_box(v0, v1, v2, lo, hi, g, i, j, eps, a, b)) { ref_face[o] = f; ref_lo[o] = a; ref_hi[o] = b; ++o; ++written; }
    if (written) return;
  }
  ref_face[o] = f; ref_lo[o] = lo; ref_hi[o] = hi;
}

__device__ __forceinline__ unsigned long long expand21(unsigned long long v)
{
  v &= 0x1fffffull;
  v = (v | v << 32) & 0x1f00000000ffffull;
  v = (v | v << 16) & 0x1f0000ff0000ffull;
  v = (v | v << 8) & 0x100f00f00f00f00full;
  v = (v | v << 4) & 0x10c30c30c30c30c3ull;
  v = (v | v << 2) & 0x1249249249249249ull;
  return v;
}

__global__ void k_morton(const float4* lo, const float4* hi, uint32_t n, const int* bounds, unsigned long long* keys, uint32_t* vals)
{
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n) return;
  const float bl[3] = {order_float(bounds[0]), order_float(bounds[1]), order_float(bounds[2])};
  const float bh[3] = {order_float(bounds[3]), order_float(bounds[4]), order_float(bounds[5])};
  const float4 l = lo[f], h = hi[f];
  const float c[3] = {0.5f * (l.x + h.x), 0.5f * (l.y + h.y), 0.5f * (l.z + h.z)};
  unsigned long long q[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float ext = bh[k] - bl[k];
    float x = ext > 0.0f ? (c[k] - bl[k]) / ext : 0.0f;
    x = fminf(fmaxf(x * 2097152.0f, 0.0f), 2097151.0f);
    q[k] = (unsigned long long)x;
  }
  keys[f] = (expand21(q[0]) << 2) | (expand21(q[1]) << 1) | expand21(q[2]);
  vals[f] = f;
}

__device__ __forceinline__ int delta(const unsigned long long* keys, int n, int i, int j)
{
  if (j < 0 || j >= n) return -1;
  const unsigned long long x = keys[i] ^ keys[j];
  if (x == 0ull) return 64 + __clz((unsigned)(i ^ j));
  return __clzll((long long)x);
}

// child reference: >= 0 inner node, < 0 leaf (~ref = sorted position)
__global__ void k_hierarchy(const unsigned long long* keys, int n, int2* children, int2* ranges, int* node_parent, int* leaf_parent)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n - 1) return;
  const int d = (delta(keys, n, i, i + 1) - delta(keys, n, i, i - 1)) >= 0 ? 1 : -1;
  const int dmin = delta(keys, n, i, i - d);
  int lmax = 2;
  while (delta(keys, n, i, i + lmax * d) > dmin) lmax <<= 1;
  int l = 0;
  for (int t = lmax >> 1; t >= 1; t >>= 1)
    if (delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
  const int j = i + l * d;
  const int dnode = delta(keys, n, i, j);
  int s = 0;
  int t = l;
  do {
    t = (t + 1) >> 1;
    if (delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
  } while (t > 1);
  const int gamma = i + s * d + min(d, 0);
  const int first = min(i, j), last = max(i, j);
  const int left = (first == gamma) ? ~gamma : gamma;
  const int right = (last == gamma + 1) ? ~(gamma + 1) : gamma + 1;
  children[i] = make_int2(left, right);
  ranges[i] = make_int2(first, last);
  if (left >= 0) node_parent[left] = i; else leaf_parent[~left] = i;
  if (right >= 0) node_parent[right] = i; else leaf_parent[~right] = i;
  if (i == 0) node_parent[0] = -1;
}

__device__ __forceinline__ void child_box(int ref, const float4* node_lo, const float4* node_hi, const float4* leaf_lo, const float4* leaf_hi, float4& lo, float4& hi)
{
  if (ref >= 0) { lo = node_lo[ref]; hi = node_hi[ref]; }
  else { lo = leaf_lo[~ref]; hi = leaf_hi[~ref]; }
}

// bottom-up refit: the second thread to arrive at a node merges the two child boxes
__global__ void k_refit(const uint32_t* sorted_face, const float4* face_lo, const float4* face_hi, int n, const int2* children, const int* node_parent, const int* leaf_parent,
                        float4* node_lo, float4* node_hi, float4* leaf_lo, float4* leaf_hi, unsigned int* arrive)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t f = sorted_face[i];
  leaf_lo[i] = face_lo[f];
  leaf_hi[i] = face_hi[f];
  int cur = leaf_parent[i];
  while (cur >= 0) {
    __threadfence();  // publish this subtree's box before signalling
    const unsigned int prev = atomicAdd(&arrive[cur], 1u);
    if (prev == 0u) return;
    __threadfence();  // see the sibling's box
    const int2 ch = children[cur];
    float4 al, ah, bl, bh;
    child_box(ch.x, node_lo, node_hi, leaf_lo, leaf_hi, al, ah);
    child_box(ch.y, node_lo, node_hi, leaf_lo, leaf_hi, bl, bh);
    node_lo[cur] = make_float4(fminf(al.x, bl.x), fminf(al.y, bl.y), fminf(al.z, bl.z), 0.0f);
    node_hi[cur] = make_float4(fmaxf(ah.x, bh.x), fmaxf(ah.y, bh.y), fmaxf(ah.z, bh.z), 0.0f);
    cur = node_parent[cur];
  }
}

// traversal reference of a radix-tree child: small subtrees become leaves
__device__ __forceinline__ int emit_ref(int ref, const int2* ranges)
{
  if (ref < 0) return ~(int)(((uint32_t)(~ref) << 3) | 0u);
  const int2 r = ranges[ref];
  const uint32_t cnt = (uint32_t)(r.y - r.x + 1);
  if (cnt <= kLeafMax2) return ~(int)(((uint32_t)r.x << 3) | (cnt - 1u));
  return ref;
}

__global__ void k_emit2(int n_inner, const int2* children, const int2* ranges, const float4* node_lo, const float4* node_hi, const float4* leaf_lo, const float4* leaf_hi, float pad,
                        float4* out)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_inner) return;
  const int2 ch = children[i];
  float4 al, ah, bl, bh;
  child_box(ch.x, node_lo, node_hi, leaf_lo, leaf_hi, al, ah);
  child_box(ch.y, node_lo, node_hi, leaf_lo, leaf_hi, bl, bh);
  const int ra = emit_ref(ch.x, ranges), rb = emit_ref(ch.y, ranges);
  out[4 * i] = make_float4(al.x - pad, al.y - pad, al.z - pad, ah.x + pad);
  out[4 * i + 1] = make_float4(ah.y + pad, ah.z + pad, bl.x - pad, bl.y - pad);
  out[4 * i + 2] = make_float4(bl.z - pad, bh.x + pad, bh.y + pad, bh.z + pad);
  out[4 * i + 3] = make_float4(__int_as_float(ra), __int_as_float(rb), 0.0f, 0.0f);
}

// root for scenes with <= kLeafMax2 faces: child 0 is the only leaf, child 1 is an empty box
__global__ void k_emit2_tiny(int n, const float4* face_lo, const float4* face_hi, float pad, float4* out)
{
  float l[3] = {3e38f, 3e38f, 3e38f}, h[3] = {-3e38f, -3e38f, -3e38f};
  for (int f = 0; f < n; ++f) {
    l[0] = fminf(l[0], face_lo[f].x); l[1] = fminf(l[1], face_lo[f].y); l[2] = fminf(l[2], face_lo[f].z);
    h[0] = fmaxf(h[0], face_hi[f].x); h[1] = fmaxf(h[1], face_hi[f].y); h[2] = fmaxf(h[2], face_hi[f].z);
  }
  out[0] = make_float4(l[0] - pad, l[1] - pad, l[2] - pad, h[0] + pad);
  out[1] = make_float4(h[1] + pad, h[2] + pad, 3e38f, 3e38f);
  out[2] = make_float4(3e38f, 3e38f, 3e38f, 3e38f);  // unreachable point box: every slab test fails
  const int ra = ~(int)((0u << 3) | (uint32_t)(n - 1));
  out[3] = make_float4(__int_as_float(ra), __int_as_float(ra), 0.0f, 0.0f);
}

__global__ void k_emit_tris(const float4* face_rec, const uint8_t* face_cls, const uint32_t* sorted_face, uint32_t n, float4* tris, const uint32_t* ref_face)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t f = sorted_face[i];
  if (ref_face) f = ref_face[f];  // split faces: the leaf is a reference
  if (face_cls[f] & 0x20u) {  // a cut-out face whose any-hit test can never pass (scene_plan_host.h: footprint_class): a triangle no ray hits
    tris[3 * i] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xffffffffu));
    tris[3 * i + 1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    tris[3 * i + 2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  const float4 a = face_rec[kFaceRec * (size_t)f], b = face_rec[kFaceRec * (size_t)f + 1], c = face_rec[kFaceRec * (size_t)f + 2];
  tris[3 * i] = make_float4(a.x, a.y, a.z, __uint_as_float(f));
  tris[3 * i + 1] = make_float4(b.x, b.y, b.z, (face_cls[f] & 0x40u) ? 1.0f : 0.0f);  // .w != 0: candidate hits need the alpha test
  tris[3 * i + 2] = make_float4(c.x, c.y, c.z, 0.0f);
}


// ------------------------------------------------------------------------------------------------
// BVH8 collapse.  One thread per wide node: starting from the two children of a radix-tree node it
// repeatedly opens the child with the largest surface area (among those holding more than
// kLeafMax8 triangles) until eight children exist, assigns children to slots so that slot bits
// agree with the octant of (child centre - node centre), quantises the boxes and hands the inner
// children to the next level.  Levels are processed breadth first; node and triangle blocks are
// allocated with atomics (the traversal result does not depend on their order, fh_trace.h).
// ------------------------------------------------------------------------------------------------
constexpr uint32_t kLeafMax8 = 3;  // scenes with at most this many faces get a single root node (k_collapse8_tiny)

struct Work8 { int bnode; uint32_t wnode; };

__device__ __forceinline__ float box_area(const float4& lo, const float4& hi)
{
  const float ex = hi.x - lo.x, ey = hi.y - lo.y, ez = hi.z - lo.z;
  return ex * ey + ey * ez + ez * ex;
}

__device__ __forceinline__ uint32_t ref_count(int ref, const int2* ranges) { return ref < 0 ? 1u : (uint32_t)(ranges[ref].y - ranges[ref].x + 1); }
__device__ __forceinline__ uint32_t ref_first(int ref, const int2* ranges) { return ref < 0 ? (uint32_t)(~ref) : (uint32_t)ranges[ref].x; }

// smallest biased exponent E with 255 * 2^(E-127) >= extent
__device__ __forceinline__ uint32_t quant_exponent(float extent)
{
  if (!(extent > 0.0f)) return 1u;
  const float s = extent / 255.0f;
  uint32_t bits = __float_as_uint(s);
  uint32_t e = (bits >> 23) & 0xffu;
  if (bits & 0x7fffffu) e += 1u;  // round the scale up to a power of two
  if (e < 1u) e = 1u;
  if (e > 254u) e = 254u;
  // guard against rounding in the division above
  while (e < 254u && __uint_as_float(e << 23) * 255.0f < extent) e += 1u;
  return e;
}

// Origin and scale of one axis of a wide node share a word (fh_trace.h): the low mantissa byte of the origin holds the biased exponent of the
// scale, and the origin IS the float the word spells.  Returns the word for lower bound `lo` and upper bound `hi`: the largest such float that
// is <= lo, with the smallest exponent whose 255 steps still reach hi from there.
__device__ __forceinline__ uint32_t origin_word(float lo, uint32_t e)
{
  const uint32_t b = __float_as_uint(lo);
  if (!(b >> 31)) {                       // lo >= +0: clearing mantissa bits rounds down, the exponent byte may round up again
    uint32_t w = (b & ~0xffu) | e;
    if (w > b) w = w >= 0x100u ? w - 0x100u : (0x80000000u | e);  // (nothing below on the positive side: the negative number closest to zero)
    return w;
  }
  const uint32_t m = b & 0x7fffffffu;     // lo <= -0: the magnitude has to reach |lo|
  uint32_t wm = (m & ~0xffu) | e;
  if (wm < m) wm += 0x100u;
  return 0x80000000u | wm;
}
__device__ __forceinline__ uint32_t quant_axis(float lo, float hi, float& origin)
{
  uint32_t e = quant_exponent(hi - lo);
  for (;;) {
    const uint32_t w = origin_word(lo, e);
    origin = __uint_as_float(w);
    if (e >= 254u || __uint_as_float(e << 23) * 255.0f >= hi - origin) return w;
    e += 1u;
  }
}

// ---- which descendants of a binary node become the children of its wide node: the cut of least cost (Ylitie, Karras, Laine 2017, section 3).
// With one triangle per leaf child the triangles' share of the SAH cost is the same for every cut, so what is minimised is the summed surface area of the
// wide nodes, i.e. the expected number of 8-wide node tests per ray.  C(n, i) = least cost of the subtree of n when it may occupy at most i child slots
// of the wide node above it:
//   C(n, 1) = area(n) + D(n, 8)                n becomes a wide node itself and deals its eight slots to its two children
//   D(n, j) = min over k of C(left, k) + C(right, j - k)
//   C(n, i) = min(D(n, i), C(n, i - 1))        i = 2..7; a triangle costs nothing and takes one slot
// Tables are filled bottom up (arrival counters, like the box refit); per node 7 costs and the decisions: the k of D(n, j) for j = 2..8 (3 bits each in x)
// and the number of slots C(n, i) really uses for i = 1..7 (3 bits each in y).
__global__ void k_tree_parents(int n_inner, const int2* children, int* node_parent, int* leaf_parent)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_inner) return;
  const int2 ch = children[i];
  if (ch.x >= 0) node_parent[ch.x] = i; else leaf_parent[~ch.x] = i;
  if (ch.y >= 0) node_parent[ch.y] = i; else leaf_parent[~ch.y] = i;
}

__device__ __forceinline__ float cut_cost(int ref, int k, const float* cost) { return ref < 0 ? 0.0f : cost[7 * (size_t)ref + (k - 1)]; }

__global__ void k_cut_tables(int n_leaves, const int2* children, const int* node_parent, const int* leaf_parent, const float4* node_lo, const float4* node_hi, unsigned int* arrive,
                             float* cost, uint2* decision)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_leaves) return;
  int cur = leaf_parent[i];
  while (cur >= 0) {
    __threadfence();  // publish this subtree's table before signalling
    const unsigned int prev = atomicAdd(&arrive[cur], 1u);
    if (prev == 0u) return;
    __threadfence();  // see the sibling's table
    const int2 ch = children[cur];
    float D[9];
    uint32_t split = 0, use = 1u;
    for (int j = 2; j <= 8; ++j) {
      float best = 3e38f;
      int bk = 1;
      for (int k = (j - 7 > 1 ? j - 7 : 1); k <= (j - 1 < 7 ? j - 1 : 7); ++k) {
        const float c = cut_cost(ch.x, k, cost) + cut_cost(ch.y, j - k, cost);
        if (c < best) { best = c; bk = k; }
      }
      D[j] = best;
      split |= (uint32_t)bk << (3 * (j - 2));
    }
    float C = box_area(node_lo[cur], node_hi[cur]) + D[8];
    uint32_t u = 1u;
    cost[7 * (size_t)cur] = C;
    for (int k = 2; k <= 7; ++k) {
      if (D[k] < C) { C = D[k]; u = (uint32_t)k; }
      cost[7 * (size_t)cur + (k - 1)] = C;
      use |= u << (3 * (k - 1));
    }
    decision[cur] = make_uint2(split, use);
    cur = node_parent[cur];
  }
}

__global__ void k_collapse8(const Work8* items, uint32_t n_items, const int2* children, const int2* ranges, const float4* node_lo, const float4* node_hi, const float4* leaf_lo,
                            const float4* leaf_hi, float pad, uint32_t leaf_max, uint32_t absorb, uint4* nodes, uint32_t* node_counter, uint32_t* tri_counter, uint32_t* tri_slot, Work8* next_items, uint32_t* next_count,
                            const uint2* decision, uint32_t* wparent)
{
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n_items) return;
  const Work8 it = items[w];
  int ref[8];
  float4 lo[8], hi[8];
  int n = 0;
  {
    const int2 ch = children[it.bnode];
    ref[0] = ch.x; ref[1] = ch.y; n = 2;
    child_box(ch.x, node_lo, node_hi, leaf_lo, leaf_hi, lo[0], hi[0]);
    child_box(ch.y, node_lo, node_hi, leaf_lo, leaf_hi, lo[1], hi[1]);
  }
  // Which child to open next.  Plain rule: the largest one.  With `absorb` (default) small subtrees are treated as units: a child
  // with at most 8 leaves is opened only when ALL of its leaves fit into the free slots, and is then opened completely before
  // anything else, so it ends up either as direct leaf children of this node or as ONE full inner child below it, never as a few
  // 2-3 leaf fragments that each cost a node fetch (the plain rule left 4.5 of 8 slots used on average).
  if (decision) {  // the cut chosen by k_cut_tables: deal the eight slots down the binary tree
    int st_ref[8], st_slots[8], sp = 0;
    const int2 ch0 = children[it.bnode];
    const int k0 = (int)((decision[it.bnode].x >> 18) & 7u);
    st_ref[sp] = ch0.y; st_slots[sp++] = 8 - k0;
    st_ref[sp] = ch0.x; st_slots[sp++] = k0;
    n = 0;
    while (sp > 0) {
      --sp;
      const int m = st_ref[sp], j = st_slots[sp];
      if (m < 0) { ref[n++] = m; continue; }
      const uint2 d = decision[m];
      const int jj = (int)((d.y >> (3 * (j - 1))) & 7u);  // slots the subtree really uses of the j it was given
      if (jj <= 1) { ref[n++] = m; continue; }            // one slot: it becomes a wide node of its own
      const int k = (int)((d.x >> (3 * (jj - 2))) & 7u);
      const int2 ch = children[m];
      st_ref[sp] = ch.y; st_slots[sp++] = jj - k;
      st_ref[sp] = ch.x; st_slots[sp++] = k;
    }
    for (int i = 0; i < n; ++i) child_box(ref[i], node_lo, node_hi, leaf_lo, leaf_hi, lo[i], hi[i]);
  }
  uint32_t absorbing = 0;  // slots that belong to a subtree being absorbed
  while (!decision && n < 8) {
    int best = -1;
    float best_area = -1.0f;
    if (absorb) {
      for (int i = 0; i < n && best < 0; ++i)
        if ((absorbing >> i) & 1u) { if (ref[i] >= 0 && ref_count(ref[i], ranges) > leaf_max) best = i; else absorbing &= ~(1u << i); }
      if (best < 0) {
        for (int i = 0; i < n; ++i) {  // subtrees that cannot become one node: open the largest
          if (ref[i] < 0 || ref_count(ref[i], ranges) <= 8u * leaf_max) continue;
          const float a = box_area(lo[i], hi[i]);
          if (a > best_area) { best_area = a; best = i; }
        }
      }
      if (best < 0) {
        for (int i = 0; i < n; ++i) {  // small subtrees whose leaves all fit: absorb the largest
          if (ref[i] < 0) continue;
          const uint32_t c = ref_count(ref[i], ranges);
          if (c <= leaf_max || (uint32_t)n + (c + leaf_max - 1u) / leaf_max - 1u > 8u) continue;
          const float a = box_area(lo[i], hi[i]);
          if (a > best_area) { best_area = a; best = i; }
        }
        if (best >= 0) absorbing |= 1u << best;
      }
    } else {
      for (int i = 0; i < n; ++i) {
        if (ref[i] < 0 || ref_count(ref[i], ranges) <= leaf_max) continue;
        const float a = box_area(lo[i], hi[i]);
        if (a > best_area) { best_area = a; best = i; }
      }
    }
    if (best < 0) break;
    if ((absorbing >> best) & 1u) absorbing |= 1u << n;
    const int2 ch = children[ref[best]];
    ref[best] = ch.x;
    child_box(ch.x, node_lo, node_hi, leaf_lo, leaf_hi, lo[best], hi[best]);
    ref[n] = ch.y;
    child_box(ch.y, node_lo, node_hi, leaf_lo, leaf_hi, lo[n], hi[n]);
    ++n;
  }
  // node box = union of the padded child boxes
  float nlo[3] = {3e38f, 3e38f, 3e38f}, nhi[3] = {-3e38f, -3e38f, -3e38f};
  for (int i = 0; i < n; ++i) {
    lo[i].x -= pad; lo[i].y -= pad; lo[i].z -= pad; hi[i].x += pad; hi[i].y += pad; hi[i].z += pad;
    nlo[0] = fminf(nlo[0], lo[i].x); nlo[1] = fminf(nlo[1], lo[i].y); nlo[2] = fminf(nlo[2], lo[i].z);
    nhi[0] = fmaxf(nhi[0], hi[i].x); nhi[1] = fmaxf(nhi[1], hi[i].y); nhi[2] = fmaxf(nhi[2], hi[i].z);
  }
  const float cx = 0.5f * (nlo[0] + nhi[0]), cy = 0.5f * (nlo[1] + nhi[1]), cz = 0.5f * (nlo[2] + nhi[2]);
  // greedy octant assignment: repeatedly take the (child, slot) pair with the largest projection
  int slot_of[8], child_in[8];
  for (int i = 0; i < 8; ++i) { slot_of[i] = -1; child_in[i] = -1; }
  for (int round = 0; round < n; ++round) {
    float bestv = -3e38f;
    int bc = -1, bs = -1;
    for (int i = 0; i < n; ++i) {
      if (slot_of[i] >= 0) continue;
      const float dx = 0.5f * (lo[i].x + hi[i].x) - cx, dy = 0.5f * (lo[i].y + hi[i].y) - cy, dz = 0.5f * (lo[i].z + hi[i].z) - cz;
      for (int sl = 0; sl < 8; ++sl) {
        if (child_in[sl] >= 0) continue;
        const float v = ((sl & 4) ? dx : -dx) + ((sl & 2) ? dy : -dy) + ((sl & 1) ? dz : -dz);
        if (v > bestv) { bestv = v; bc = i; bs = sl; }
      }
    }
    slot_of[bc] = bs;
    child_in[bs] = bc;
  }
  // count inner children / triangles, allocate the block of inner children (triangles live in the node's own eight slots)
  uint32_t n_inner = 0, n_tris = 0;
  for (int sl = 0; sl < 8; ++sl) {
    const int c = child_in[sl];
    if (c < 0) continue;
    const uint32_t cnt = ref_count(ref[c], ranges);
    if (ref[c] >= 0 && cnt > leaf_max) n_inner++; else n_tris += cnt;
  }
  const uint32_t child_base = n_inner ? atomicAdd(node_counter, n_inner) : 0u;
  if (n_tris) atomicAdd(tri_counter, n_tris);
  float org[3];
  const uint32_t wx = quant_axis(nlo[0], nhi[0], org[0]), wy = quant_axis(nlo[1], nhi[1], org[1]), wz = quant_axis(nlo[2], nhi[2], org[2]);
  const float isx = 1.0f / __uint_as_float((wx & 0xffu) << 23), isy = 1.0f / __uint_as_float((wy & 0xffu) << 23), isz = 1.0f / __uint_as_float((wz & 0xffu) << 23);
  uint32_t imask = 0, q[6][2] = {{~0u, ~0u}, {~0u, ~0u}, {~0u, ~0u}, {0, 0}, {0, 0}, {0, 0}};  // empty slots keep the inverted box (lo 255, hi 0)
  uint32_t inner_seen = 0;
  uint32_t next_base = 0;
  if (n_inner) next_base = atomicAdd(next_count, n_inner);
  for (int sl = 0; sl < 8; ++sl) {
    const int c = child_in[sl];
    if (c < 0) continue;
    const uint32_t cnt = ref_count(ref[c], ranges);
    if (ref[c] >= 0 && cnt > leaf_max) {
      imask |= 1u << sl;
      next_items[next_base + inner_seen] = Work8{ref[c], child_base + inner_seen};
      wparent[child_base + inner_seen] = (it.wnode << 3) | (uint32_t)sl;  // the way up (fh_trace.h: bottom-up start of rays that leave a surface)
      inner_seen++;
    } else {
      tri_slot[ref_first(ref[c], ranges)] = 8u * it.wnode + (uint32_t)sl;  // (leaf_max is 1: one triangle per leaf child)
    }
    const float v[6] = {floorf((lo[c].x - org[0]) * isx), floorf((lo[c].y - org[1]) * isy), floorf((lo[c].z - org[2]) * isz),
                        ceilf((hi[c].x - org[0]) * isx), ceilf((hi[c].y - org[1]) * isy), ceilf((hi[c].z - org[2]) * isz)};
    for (int k = 0; k < 6; ++k) {
      const float cl = fminf(fmaxf(v[k], 0.0f), 255.0f);
      q[k][sl >> 2] = (q[k][sl >> 2] & ~(0xffu << (8 * (sl & 3)))) | (((uint32_t)cl) << (8 * (sl & 3)));
    }
  }
  uint4* out = nodes + kBvh8NodeVec * (size_t)it.wnode;
  out[0] = make_uint4(wx, wy, wz, (child_base << 8) | imask);
  out[1] = make_uint4(q[0][0], q[0][1], q[1][0], q[1][1]);
  out[2] = make_uint4(q[2][0], q[2][1], q[3][0], q[3][1]);
  out[3] = make_uint4(q[4][0], q[4][1], q[5][0], q[5][1]);
}

// scenes with <= kLeafMax8 faces: a root with one leaf child per face
__global__ void k_collapse8_tiny(int n, const float4* face_lo, const float4* face_hi, float pad, uint4* nodes, uint32_t* tri_slot)
{
  float l[3] = {3e38f, 3e38f, 3e38f}, h[3] = {-3e38f, -3e38f, -3e38f};
  for (int f = 0; f < n; ++f) {
    l[0] = fminf(l[0], face_lo[f].x - pad); l[1] = fminf(l[1], face_lo[f].y - pad); l[2] = fminf(l[2], face_lo[f].z - pad);
    h[0] = fmaxf(h[0], face_hi[f].x + pad); h[1] = fmaxf(h[1], face_hi[f].y + pad); h[2] = fmaxf(h[2], face_hi[f].z + pad);
    tri_slot[f] = (uint32_t)f;
  }
  float org[3];
  const uint32_t wx = quant_axis(l[0], h[0], org[0]), wy = quant_axis(l[1], h[1], org[1]), wz = quant_axis(l[2], h[2], org[2]);
  // every face gets the whole node box (0 .. 255 on every axis): with <= 3 triangles nothing is gained by tighter ones
  const uint32_t lo4 = n >= 4 ? 0u : (~0u << (8 * n)), hi4 = ~lo4;
  nodes[0] = make_uint4(wx, wy, wz, 0u);
  nodes[1] = make_uint4(lo4, ~0u, lo4, ~0u);
  nodes[2] = make_uint4(lo4, ~0u, hi4, 0u);
  nodes[3] = make_uint4(hi4, 0u, hi4, 0u);
}

// triangle slots of the wide tree: 8 per node, slot 8 * node + child slot; slots without a triangle hold a degenerate one (all zero, face id 0xffffffff)
__global__ void k_emit_tris8(const float4* face_rec, const uint8_t* face_cls, const uint32_t* sorted_face, const uint32_t* tri_slot, uint32_t n, float4* tris, const uint32_t* ref_face,
                             uint32_t* face_node, const uint32_t* split_count)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t f = sorted_face[i];
  if (ref_face) f = ref_face[f];
  if (face_node) face_node[f] = (split_count && split_count[f] > 1u) ? 0u : tri_slot[i] >> 3;  // the wide node that holds the face; a face that entered the build as several references: the root
  const size_t t = 3 * (size_t)tri_slot[i];
  if (face_cls[f] & 0x20u) return;  // never hit (above): the slot keeps the degenerate triangle k_clear_tris8 put there
  const float4 a = face_rec[kFaceRec * (size_t)f], b = face_rec[kFaceRec * (size_t)f + 1], c = face_rec[kFaceRec * (size_t)f + 2];
  tris[t] = make_float4(a.x, a.y, a.z, __uint_as_float(f));
  tris[t + 1] = make_float4(b.x, b.y, b.z, (face_cls[f] & 0x40u) ? 1.0f : 0.0f);
  tris[t + 2] = make_float4(c.x, c.y, c.z, 0.0f);
}
__global__ void k_clear_tris8(float4* tris, uint32_t n_slots)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_slots) return;
  tris[3 * (size_t)i] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xffffffffu));
  tris[3 * (size_t)i + 1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  tris[3 * (size_t)i + 2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// ------------------------------------------------------------------------------------------------
// PLOC: parallel locally-ordered clustering (Meister & Bittner, "Parallel Locally-Ordered Clustering for Bounding Volume
// Hierarchy Construction", TVCG 2018).  The radix tree above splits by Morton prefix only, which is what a uniform soup wants but
// wraps big and small triangles of a real scene into the same boxes.  PLOC builds the binary tree bottom up instead: the clusters
// (initially the Morton-sorted leaves) each look `kPlocRadius` neighbours to either side for the partner with the smallest
// merged surface area, mutual choices merge into a new node, the array is compacted, and the round repeats until one cluster is
// left.  The output has the radix tree's array layout (children, boxes, leaf counts in `ranges` as (0, count - 1)), so the
// 8-wide collapse consumes either.  Selected with FH_BVH_BUILDER=ploc.
// ------------------------------------------------------------------------------------------------
constexpr int kPlocRadius = 16;

__global__ void k_ploc_init(int n, const float4* leaf_lo, const float4* leaf_hi, int* cid, float4* clo, float4* chi)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  cid[i] = ~i;
  clo[i] = leaf_lo[i];
  chi[i] = leaf_hi[i];
}

__global__ void k_ploc_nearest(int n, const float4* clo, const float4* chi, int* nn, int radius)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 lo = clo[i], hi = chi[i];
  float best = __builtin_inff();
  int bj = -1;  // the first neighbour is taken unconditionally, so a cluster whose merged areas are all inf / NaN still gets a partner
  const int j0 = i - radius < 0 ? 0 : i - radius, j1 = i + radius > n - 1 ? n - 1 : i + radius;
  for (int j = j0; j <= j1; ++j) {
    if (j == i) continue;
    const float4 l2 = clo[j], h2 = chi[j];
    const float ex = fmaxf(hi.x, h2.x) - fminf(lo.x, l2.x), ey = fmaxf(hi.y, h2.y) - fminf(lo.y, l2.y), ez = fmaxf(hi.z, h2.z) - fminf(lo.z, l2.z);
    const float a = ex * ey + ey * ez + ez * ex;
    if (bj < 0 || a < best) { best = a; bj = j; }  // ties: the lower index (the loop ascends)
  }
  nn[i] = bj;
}

__global__ void k_ploc_merge(int n, const int* nn, int* cid, float4* clo, float4* chi, uint32_t* valid, int2* children, int2* ranges, float4* node_lo, float4* node_hi,
                             uint32_t* node_counter)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int j = nn[i];
  uint32_t keep = 1u;
  if (j >= 0 && nn[j] == i) {
    if (i < j) {
      const int a = cid[i], b = cid[j];
      const float4 lo = clo[i], hi = chi[i], l2 = clo[j], h2 = chi[j];
      const float4 ulo = make_float4(fminf(lo.x, l2.x), fminf(lo.y, l2.y), fminf(lo.z, l2.z), 0.0f);
      const float4 uhi = make_float4(fmaxf(hi.x, h2.x), fmaxf(hi.y, h2.y), fmaxf(hi.z, h2.z), 0.0f);
      const int id = (int)atomicAdd(node_counter, 1u);
      const int ca = a < 0 ? 1 : ranges[a].y + 1, cb = b < 0 ? 1 : ranges[b].y + 1;
      children[id] = make_int2(a, b);
      ranges[id] = make_int2(0, ca + cb - 1);
      node_lo[id] = ulo;
      node_hi[id] = uhi;
      cid[i] = id;
      clo[i] = ulo;
      chi[i] = uhi;
    } else keep = 0u;
  }
  valid[i] = keep;
}

__global__ void k_ploc_compact(int n, const uint32_t* valid, const uint32_t* offset, const int* cid, const float4* clo, const float4* chi, int* cid_out, float4* clo_out,
                               float4* chi_out)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !valid[i]) return;
  const uint32_t o = offset[i];
  cid_out[o] = cid[i];
  clo_out[o] = clo[i];
  chi_out[o] = chi[i];
}

// 1 + the wide node that holds a face into the free lane of the face's record (.z of its last vector; 0: unknown, rays start at the root): the shade kernels, which read that
// vector for the material id, find there where the rays that leave the face start their traversal (fh_trace.h: bottom-up start)
__global__ void k_face_node_to_rec(const uint32_t* face_node, uint32_t n, float4* face_rec)
{
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n) return;
  const uint32_t node = face_node[f];
  face_rec[kFaceRec * (size_t)f + 6].z = __uint_as_float(node == 0xffffffffu ? 0u : node + 1u);
}

// surface-area-heuristic cost of a binary tree: sum over inner nodes of area(node) (the leaves are the same triangles in both builders)
__global__ void k_sah_sum(int n_inner, const float4* node_lo, const float4* node_hi, double* sum)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double a = 0.0;
  if (i < n_inner) a = (double)box_area(node_lo[i], node_hi[i]);
  for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off);
  if ((threadIdx.x & 63) == 0 && a != 0.0) atomicAdd(sum, a);
}

// ------------------------------------------------------------------------------------------------
// Refit of the wide tree.  When only the instance transforms change (Renderer::set_time: the reference rebuilds its IAS and leaves
// the GAS alone, renderer.h:614-640) the topology of the flattened tree is kept: the triangle copies are refreshed from the moved
// face records and the boxes are recomputed bottom up, level by level (levels are contiguous node ranges because the collapse is
// breadth first), with the build's own padding and quantisation rules.  Hits do not depend on the shape of the tree (fh_trace.h), so a
// refitted tree returns the same bits as a rebuilt one; what degrades is its quality, which bvh_build_device watches.
__global__ void k_refresh_tris8(const float4* face_rec, uint32_t n_slots, float4* tris)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_slots) return;
  const uint32_t f = __float_as_uint(tris[3 * (size_t)i].w);
  if (f == 0xffffffffu) return;  // a slot without a triangle
  const float4 a = face_rec[kFaceRec * (size_t)f], b = face_rec[kFaceRec * (size_t)f + 1], c = face_rec[kFaceRec * (size_t)f + 2];
  tris[3 * (size_t)i] = make_float4(a.x, a.y, a.z, __uint_as_float(f));
  tris[3 * (size_t)i + 1].x = b.x; tris[3 * (size_t)i + 1].y = b.y; tris[3 * (size_t)i + 1].z = b.z;  // .w keeps the alpha flag
  tris[3 * (size_t)i + 2] = make_float4(c.x, c.y, c.z, 0.0f);
}

// full-precision box of every node of a freshly built tree, bottom up (the refit's starting state and its quality reference)
__global__ void k_refit8_level(uint4* nodes, const float4* tris, float4* box, uint32_t begin, uint32_t end, float pad, int requantise)
{
  const uint32_t ni = begin + blockIdx.x * blockDim.x + threadIdx.x;
  if (ni >= end) return;
  uint4* nd = nodes + kBvh8NodeVec * (size_t)ni;
  const uint4 n0 = nd[0];
  const uint32_t imask = n0.w & 0xffu, child_base = n0.w >> 8;
  float lo[8][3], hi[8][3];
  bool used[8];
  float nlo[3] = {3e38f, 3e38f, 3e38f}, nhi[3] = {-3e38f, -3e38f, -3e38f};
  for (int sl = 0; sl < 8; ++sl) {
    used[sl] = false;
    if ((imask >> sl) & 1u) {  // inner child: its own box, computed when its level was done (one padding already in it)
      const uint32_t c = child_base + (uint32_t)__popc(imask & ((1u << sl) - 1u));
      const float4 l = box[2 * (size_t)c], h = box[2 * (size_t)c + 1];
      lo[sl][0] = l.x; lo[sl][1] = l.y; lo[sl][2] = l.z; hi[sl][0] = h.x; hi[sl][1] = h.y; hi[sl][2] = h.z;
    } else {  // leaf child: bounds of its triangle, padded like the builder pads leaf boxes
      const size_t t = 3 * (size_t)(8u * ni + (uint32_t)sl);
      const float4 a = tris[t], b = tris[t + 1], c = tris[t + 2];
      if (__float_as_uint(a.w) == 0xffffffffu) continue;  // empty slot
      lo[sl][0] = fminf(a.x, fminf(b.x, c.x)) - pad; lo[sl][1] = fminf(a.y, fminf(b.y, c.y)) - pad; lo[sl][2] = fminf(a.z, fminf(b.z, c.z)) - pad;
      hi[sl][0] = fmaxf(a.x, fmaxf(b.x, c.x)) + pad; hi[sl][1] = fmaxf(a.y, fmaxf(b.y, c.y)) + pad; hi[sl][2] = fmaxf(a.z, fmaxf(b.z, c.z)) + pad;
    }
    used[sl] = true;
    for (int k = 0; k < 3; ++k) { nlo[k] = fminf(nlo[k], lo[sl][k]); nhi[k] = fmaxf(nhi[k], hi[sl][k]); }
  }
  box[2 * (size_t)ni] = make_float4(nlo[0], nlo[1], nlo[2], 0.0f);
  box[2 * (size_t)ni + 1] = make_float4(nhi[0], nhi[1], nhi[2], 0.0f);
  if (!requantise) return;
  float org[3];
  const uint32_t w[3] = {quant_axis(nlo[0], nhi[0], org[0]), quant_axis(nlo[1], nhi[1], org[1]), quant_axis(nlo[2], nhi[2], org[2])};
  const float is[3] = {1.0f / __uint_as_float((w[0] & 0xffu) << 23), 1.0f / __uint_as_float((w[1] & 0xffu) << 23), 1.0f / __uint_as_float((w[2] & 0xffu) << 23)};
  uint32_t q[6][2] = {{~0u, ~0u}, {~0u, ~0u}, {~0u, ~0u}, {0, 0}, {0, 0}, {0, 0}};
  for (int sl = 0; sl < 8; ++sl) {
    if (!used[sl]) continue;
    for (int k = 0; k < 3; ++k) {
      const float vl = fminf(fmaxf(floorf((lo[sl][k] - org[k]) * is[k]), 0.0f), 255.0f), vh = fminf(fmaxf(ceilf((hi[sl][k] - org[k]) * is[k]), 0.0f), 255.0f);
      q[k][sl >> 2] = (q[k][sl >> 2] & ~(0xffu << (8 * (sl & 3)))) | (((uint32_t)vl) << (8 * (sl & 3)));
      q[3 + k][sl >> 2] |= ((uint32_t)vh) << (8 * (sl & 3));
    }
  }
  nd[0] = make_uint4(w[0], w[1], w[2], n0.w);
  nd[1] = make_uint4(q[0][0], q[0][1], q[1][0], q[1][1]);
  nd[2] = make_uint4(q[2][0], q[2][1], q[3][0], q[3][1]);
  nd[3] = make_uint4(q[4][0], q[4][1], q[5][0], q[5][1]);
}

__global__ void k_box_area_sum(uint32_t n, const float4* box, double* sum)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  double a = 0.0;
  if (i < n) a = (double)box_area(box[2 * (size_t)i], box[2 * (size_t)i + 1]);
  for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off);
  if ((threadIdx.x & 63) == 0 && a != 0.0) atomicAdd(sum, a);
}

// ------------------------------------------------------------------------------------------------
// The build on the host.  bvh_build_device, at the bottom, is a sequence of the steps below; what they decide is decided by the pure functions of bvh_plan_host.h.
// A build assembles its tree in a NewTree; the context's tree fields are written by clear_tree and by the three commits (tiny, full, refit) only, so a failed
// build leaves the cleared state behind bvh_valid == false.
typedef std::chrono::steady_clock::time_point TimePoint;

BuildSwitches read_build_switches()  // (the only getenv calls of this file: at the top of every build, not at fh_ctx_create)
{
  return build_switches(getenv("FH_REFIT"), getenv("FH_SPLIT"), getenv("FH_BVH_BUILDER"), getenv("FH_ABSORB"), getenv("FH_COLLAPSE"), getenv("FH_BVH2"), getenv("FH_DEBUG_BVH"));
}

struct FaceBounds {  // per-face boxes, the scene's bounds as ordered ints (k_morton reads them), and the padding and scene box they give
  DeviceBuffer<float4> lo, hi;
  DeviceBuffer<int> bounds;
  ScenePad sp;
};
struct References {  // what the trees are built over: the faces' own boxes, or the clipped boxes of early split clipping (ref_face == nullptr: reference i is face i)
  uint32_t nr = 0;
  const float4 *box_lo = nullptr, *box_hi = nullptr;
  const uint32_t* ref_face = nullptr;
  DeviceBuffer<uint32_t> ref_face_buf, split_count, split_offset;  // (split_count: k_emit_tris8 finds a face's first reference with it)
  DeviceBuffer<float4> ref_lo, ref_hi;
};
struct SortedLeaves {  // the references in Morton order: order[i] is the reference of leaf i; the arrival counters are scratch of the bottom-up kernels
  DeviceBuffer<uint32_t> order;
  DeviceBuffer<float4> lo, hi;
  DeviceBuffer<unsigned int> arrive;
  // what the sort and the hierarchy worked in.  Kept with the leaves to the end of the build: a hipFree synchronises the device, and these are released after
  // the build has taken its time (fh_stats::bvh_build_ms), not inside it
  DeviceBuffer<unsigned long long> keys_a, keys_b;
  DeviceBuffer<uint32_t> vals_a;
  DeviceBuffer<int> node_parent, leaf_parent;
};
struct BinaryTree {  // nr - 1 inner nodes over the sorted leaves: the radix tree or the PLOC tree
  DeviceBuffer<int2> children, ranges;
  DeviceBuffer<float4> node_lo, node_hi;
  int root = 0;
};
struct NewTree {  // what a successful build hands to the context
  DeviceBuffer<float4> bvh2_nodes, bvh2_tris, bvh8_tris, bvh8_box;
  DeviceBuffer<uint4> bvh8_nodes;
  DeviceBuffer<uint32_t> bvh8_parent, face_node;
  uint32_t bvh2_n_nodes = 0, bvh2_n_tris = 0, bvh8_n_nodes = 0, bvh8_n_tris = 0, levels = 0;
  bool use_bvh8 = false, refit_ok = false;
  std::vector<uint32_t> level_start{0u};
  double area_built = 0.0;
};

// offset + count of the last element of an exclusive scan: the total
int scan_total(fh_ctx* ctx, const uint32_t* offset, const uint32_t* count, uint32_t n, uint32_t* total)
{
  uint32_t tail[2] = {0, 0};
  FH_HIP(hipMemcpyAsync(&tail[0], offset + (n - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
  FH_HIP(hipMemcpyAsync(&tail[1], count + (n - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
  FH_HIP(hipStreamSynchronize(ctx->stream));
  *total = tail[0] + tail[1];
  return FH_OK;
}

// boxes of all levels bottom up (requantise = 0: only the full-precision boxes of a freshly built tree), then the sum of the node areas
int refit_levels(fh_ctx* ctx, uint4* nodes, const float4* tris, float4* box, const std::vector<uint32_t>& ls, uint32_t n_nodes, float pad, int requantise, double* area)
{
  hipStream_t st = ctx->stream;
  for (size_t l = ls.size() - 1; l-- > 0;) {
    const uint32_t begin = ls[l], end = ls[l + 1];
    if (end > begin) hipLaunchKernelGGL(k_refit8_level, dim3((end - begin + 127) / 128), dim3(128), 0, st, nodes, tris, box, begin, end, pad, requantise);
  }
  DeviceBuffer<double> sum;
  FH_HIP(sum.alloc(1));
  FH_HIP(hipMemsetAsync(sum.get(), 0, 8, st));
  hipLaunchKernelGGL(k_box_area_sum, dim3((n_nodes + 255) / 256), dim3(256), 0, st, n_nodes, box, sum.get());
  FH_HIP(hipMemcpyAsync(area, sum.get(), 8, hipMemcpyDeviceToHost, st));
  FH_HIP(hipGetLastError());
  FH_HIP(hipStreamSynchronize(st));
  return FH_OK;
}

void publish_build_time(fh_ctx* ctx, TimePoint t_begin)
{
  ctx->bvh_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  ctx->stats.bvh_build_ms = ctx->bvh_build_ms;
}

void clear_tree(fh_ctx* ctx, uint32_t n)
{
  ctx->refit_ok = false;
  ctx->d_bvh8_box.reset();
  ctx->bvh8_level_start.clear();
  ctx->d_bvh2_nodes.reset(); ctx->d_bvh2_tris.reset();
  ctx->d_bvh8_nodes.reset(); ctx->d_bvh8_tris.reset(); ctx->d_bvh8_parent.reset(); ctx->d_face_node.reset();
  ctx->bvh2_n_nodes = ctx->bvh2_n_tris = ctx->bvh8_n_nodes = ctx->bvh8_n_tris = 0;
  ctx->use_bvh8 = false;
  ctx->bvh_valid = n == 0;  // (a scene without faces: the cleared state is its tree)
}

void commit_scene_box(fh_ctx* ctx, const ScenePad& sp)
{
  for (int k = 0; k < 3; ++k) { ctx->scene_lo[k] = sp.lo[k]; ctx->scene_hi[k] = sp.hi[k]; }
  ctx->bvh_valid = true;
}
void commit_refit(fh_ctx* ctx, const ScenePad& sp)
{
  commit_scene_box(ctx, sp);
  ctx->n_refits++;
}
// the binary root of up to kLeafMax2 faces and, up to kLeafMax8, the single wide node beside it (bvh8_depth keeps what the last full build left)
void commit_tiny(fh_ctx* ctx, const BuildSwitches& sw, const ScenePad& sp, NewTree& t)
{
  commit_scene_box(ctx, sp);
  ctx->d_bvh2_nodes = std::move(t.bvh2_nodes); ctx->d_bvh2_tris = std::move(t.bvh2_tris);
  ctx->d_bvh8_nodes = std::move(t.bvh8_nodes); ctx->d_bvh8_tris = std::move(t.bvh8_tris);
  ctx->bvh2_n_nodes = t.bvh2_n_nodes; ctx->bvh2_n_tris = t.bvh2_n_tris; ctx->bvh8_n_nodes = t.bvh8_n_nodes; ctx->bvh8_n_tris = t.bvh8_n_tris;
  ctx->use_bvh8 = traverse_wide(t.use_bvh8, sw);
}
void commit_full(fh_ctx* ctx, const BuildSwitches& sw, const ScenePad& sp, NewTree& t)
{
  commit_tiny(ctx, sw, sp, t);
  ctx->d_bvh8_parent = std::move(t.bvh8_parent); ctx->d_face_node = std::move(t.face_node);
  ctx->bvh8_depth = t.levels;
  if (!t.refit_ok) return;
  ctx->bvh8_level_start = std::move(t.level_start);
  ctx->d_bvh8_box = std::move(t.bvh8_box);
  ctx->bvh8_area_built = t.area_built;
  ctx->refit_ok = true;
  ctx->n_refits = 0;
}

void publish_stats(fh_ctx* ctx, TimePoint t_begin)
{
  publish_build_time(ctx, t_begin);
  const TreeStats s = tree_stats(ctx->use_bvh8, ctx->bvh8_n_nodes, ctx->bvh8_depth, ctx->bvh2_n_nodes, ctx->bvh2_n_tris, kBvh8NodeVec);
  ctx->stats.bvh_nodes = s.nodes;
  ctx->stats.bvh_node_bytes = s.node_bytes;
  ctx->stats.bvh_tri_bytes = s.tri_bytes;
  ctx->stats.bvh_depth = s.depth;
}

// Boxes of the faces, and the scene's bounds with the padding they give.  refit: the triangle copies of the wide tree are refreshed from the moved face records
// in the same submission.
int scene_bounds(fh_ctx* ctx, uint32_t n, bool refit, FaceBounds& fb)
{
  hipStream_t st = ctx->stream;
  FH_HIP(fb.lo.alloc(n)); FH_HIP(fb.hi.alloc(n)); FH_HIP(fb.bounds.alloc(6));
  const int init_bounds[6] = {0x7fffffff, 0x7fffffff, 0x7fffffff, (int)0x80000000, (int)0x80000000, (int)0x80000000};
  FH_HIP(hipMemcpyAsync(fb.bounds.get(), init_bounds, sizeof init_bounds, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_face_bounds, dim3((n + 255) / 256), dim3(256), 0, st, ctx->d_face_rec, n, fb.lo.get(), fb.hi.get(), fb.bounds.get());
  if (refit) hipLaunchKernelGGL(k_refresh_tris8, dim3((8u * ctx->bvh8_n_nodes + 255) / 256), dim3(256), 0, st, ctx->d_face_rec, 8u * ctx->bvh8_n_nodes, ctx->d_bvh8_tris);
  int hb[6];
  FH_HIP(hipMemcpyAsync(hb, fb.bounds.get(), sizeof hb, hipMemcpyDeviceToHost, st));
  FH_HIP(hipStreamSynchronize(st));
  const float b[6] = {order_float(hb[0]), order_float(hb[1]), order_float(hb[2]), order_float(hb[3]), order_float(hb[4]), order_float(hb[5])};
  fb.sp = scene_padding(b);
  return FH_OK;
}

// Instance transforms changed, topology did not: the wide tree is refitted in place.  *kept == false: not eligible, or the boxes have grown too far for the old
// topology and the caller rebuilds.
int try_refit(fh_ctx* ctx, uint32_t n, const BuildSwitches& sw, TimePoint t_begin, bool* kept)
{
  *kept = false;
  if (!refit_eligible(ctx->refit_ok, ctx->use_bvh8, ctx->d_bvh8_box.get() != nullptr, n, ctx->bvh8_n_tris, sw)) return FH_OK;
  FaceBounds fb;
  if (const int rc = scene_bounds(ctx, n, true, fb)) return rc;
  double area = 0.0;
  if (const int rc = refit_levels(ctx, ctx->d_bvh8_nodes, ctx->d_bvh8_tris, ctx->d_bvh8_box, ctx->bvh8_level_start, ctx->bvh8_n_nodes, fb.sp.pad, 1, &area)) return rc;
  if (!refit_accepted(area, ctx->bvh8_area_built)) {
    if (sw.debug) fprintf(stderr, "[bvh] refit discarded: node area %.4f > 1.5 x %.4f, rebuilding\n", area, ctx->bvh8_area_built);
    return FH_OK;
  }
  if (ctx->d_face_node) hipLaunchKernelGGL(k_face_node_to_rec, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_face_node, n, ctx->d_face_rec);  // (k_face_records has just rewritten the records)
  commit_refit(ctx, fb.sp);
  publish_build_time(ctx, t_begin);
  if (sw.debug) fprintf(stderr, "[bvh] refit %u: node area %.4f (built %.4f), %.3f ms\n", ctx->n_refits, area, ctx->bvh8_area_built, ctx->bvh_build_ms);
  *kept = true;
  return FH_OK;
}

// up to kLeafMax2 faces: the binary root with its one leaf; up to kLeafMax8 also a wide root with one leaf child per face
int build_tiny(fh_ctx* ctx, uint32_t n, bool wide, const FaceBounds& fb, NewTree& t)
{
  hipStream_t st = ctx->stream;
  const uint32_t blocks = (n + 255) / 256;
  const float pad = fb.sp.pad;
  DeviceBuffer<uint32_t> order, tri_slot;
  FH_HIP(t.bvh2_tris.alloc(3ull * n));
  FH_HIP(t.bvh2_nodes.alloc(4));
  FH_HIP(order.alloc(n));
  std::vector<uint32_t> ident(n);
  for (uint32_t i = 0; i < n; ++i) ident[i] = i;
  FH_HIP(hipMemcpyAsync(order.get(), ident.data(), 4ull * n, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_emit2_tiny, dim3(1), dim3(1), 0, st, (int)n, fb.lo.get(), fb.hi.get(), pad, t.bvh2_nodes.get());
  hipLaunchKernelGGL(k_emit_tris, dim3(blocks), dim3(256), 0, st, ctx->d_face_rec, ctx->d_face_cls, order.get(), n, t.bvh2_tris.get(), (const uint32_t*)nullptr);
  FH_HIP(hipStreamSynchronize(st));
  t.bvh2_n_tris = n;
  t.bvh2_n_nodes = 1;
  if (!wide) return FH_OK;
  FH_HIP(tri_slot.alloc(n));
  FH_HIP(t.bvh8_nodes.alloc(kBvh8NodeVec));
  FH_HIP(t.bvh8_tris.alloc(3ull * 8ull));
  hipLaunchKernelGGL(k_clear_tris8, dim3(1), dim3(64), 0, st, t.bvh8_tris.get(), 8u);
  hipLaunchKernelGGL(k_collapse8_tiny, dim3(1), dim3(1), 0, st, (int)n, fb.lo.get(), fb.hi.get(), pad, t.bvh8_nodes.get(), tri_slot.get());
  hipLaunchKernelGGL(k_emit_tris8, dim3(blocks), dim3(256), 0, st, ctx->d_face_rec, ctx->d_face_cls, order.get(), tri_slot.get(), n, t.bvh8_tris.get(), (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr);
  FH_HIP(hipStreamSynchronize(st));
  t.bvh8_n_nodes = 1;
  t.bvh8_n_tris = n;
  t.use_bvh8 = true;
  return FH_OK;
}

// references: large triangles enter the build as several clipped boxes (early split clipping, kernels above)
int split_references(fh_ctx* ctx, uint32_t n, const BuildSwitches& sw, const FaceBounds& fb, References& r)
{
  hipStream_t st = ctx->stream;
  const uint32_t blocks = (n + 255) / 256;
  r.nr = n;
  r.box_lo = fb.lo.get();
  r.box_hi = fb.hi.get();
  if (!split_enabled(n, sw)) return FH_OK;
  const SplitCells cells = split_cells(fb.sp.lo, fb.sp.hi);
  float thr = cells.thr;
  FH_HIP(r.split_count.alloc(n)); FH_HIP(r.split_offset.alloc(n));
  size_t scan_bytes = 0;
  FH_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, r.split_count.get(), r.split_offset.get(), 0u, (size_t)n, rocprim::plus<uint32_t>(), st));
  DeviceBuffer<char> scan_tmp;
  FH_HIP(scan_tmp.alloc(scan_bytes));
  uint32_t total = n;
  const int rc = split_search(n, &thr, &total, [&](float cell, uint32_t* found) {
    hipLaunchKernelGGL(k_split_count, dim3(blocks), dim3(256), 0, st, ctx->d_face_rec, fb.lo.get(), fb.hi.get(), n, cell, cells.eps, r.split_count.get());
    FH_HIP(rocprim::exclusive_scan(scan_tmp.get(), scan_bytes, r.split_count.get(), r.split_offset.get(), 0u, (size_t)n, rocprim::plus<uint32_t>(), st));
    return scan_total(ctx, r.split_offset.get(), r.split_count.get(), n, found);
  });
  if (rc || total <= n) return rc;
  r.nr = total;
  FH_HIP(r.ref_face_buf.alloc(r.nr)); FH_HIP(r.ref_lo.alloc(r.nr)); FH_HIP(r.ref_hi.alloc(r.nr));
  hipLaunchKernelGGL(k_split_emit, dim3(blocks), dim3(256), 0, st, ctx->d_face_rec, fb.lo.get(), fb.hi.get(), n, thr, cells.eps, r.split_count.get(), r.split_offset.get(), r.ref_face_buf.get(), r.ref_lo.get(),
                     r.ref_hi.get());
  r.box_lo = r.ref_lo.get(); r.box_hi = r.ref_hi.get(); r.ref_face = r.ref_face_buf.get();
  return FH_OK;
}

// Morton codes, sort, Karras hierarchy, bottom-up boxes; and the binary traversal layout (the fallback, which keeps the radix tree whatever the collapse takes)
int build_radix_tree(fh_ctx* ctx, const References& r, const FaceBounds& fb, SortedLeaves& leaves, BinaryTree& radix, NewTree& t)
{
  hipStream_t st = ctx->stream;
  const uint32_t nr = r.nr, n_inner = nr - 1, rblocks = (nr + 255) / 256, iblocks = (n_inner + 255) / 256;
  FH_HIP(t.bvh2_tris.alloc(3ull * nr));
  FH_HIP(leaves.keys_a.alloc(nr)); FH_HIP(leaves.keys_b.alloc(nr)); FH_HIP(leaves.vals_a.alloc(nr)); FH_HIP(leaves.order.alloc(nr));
  hipLaunchKernelGGL(k_morton, dim3(rblocks), dim3(256), 0, st, r.box_lo, r.box_hi, nr, fb.bounds.get(), leaves.keys_a.get(), leaves.vals_a.get());
  size_t temp_bytes = 0;
  FH_HIP(rocprim::radix_sort_pairs(nullptr, temp_bytes, leaves.keys_a.get(), leaves.keys_b.get(), leaves.vals_a.get(), leaves.order.get(), (size_t)nr, 0u, 63u, st));
  DeviceBuffer<char> temp;
  FH_HIP(temp.alloc(temp_bytes));
  FH_HIP(rocprim::radix_sort_pairs(temp.get(), temp_bytes, leaves.keys_a.get(), leaves.keys_b.get(), leaves.vals_a.get(), leaves.order.get(), (size_t)nr, 0u, 63u, st));
  FH_HIP(radix.children.alloc(n_inner)); FH_HIP(radix.ranges.alloc(n_inner)); FH_HIP(leaves.node_parent.alloc(n_inner)); FH_HIP(leaves.leaf_parent.alloc(nr));
  FH_HIP(radix.node_lo.alloc(n_inner)); FH_HIP(radix.node_hi.alloc(n_inner)); FH_HIP(leaves.lo.alloc(nr)); FH_HIP(leaves.hi.alloc(nr));
  FH_HIP(leaves.arrive.alloc(n_inner));
  FH_HIP(hipMemsetAsync(leaves.arrive.get(), 0, 4ull * n_inner, st));
  hipLaunchKernelGGL(k_hierarchy, dim3(iblocks), dim3(256), 0, st, leaves.keys_b.get(), (int)nr, radix.children.get(), radix.ranges.get(), leaves.node_parent.get(), leaves.leaf_parent.get());
  hipLaunchKernelGGL(k_refit, dim3(rblocks), dim3(256), 0, st, leaves.order.get(), r.box_lo, r.box_hi, (int)nr, radix.children.get(), leaves.node_parent.get(), leaves.leaf_parent.get(), radix.node_lo.get(), radix.node_hi.get(),
                     leaves.lo.get(), leaves.hi.get(), leaves.arrive.get());
  FH_HIP(t.bvh2_nodes.alloc(4ull * n_inner));
  hipLaunchKernelGGL(k_emit2, dim3(iblocks), dim3(256), 0, st, (int)n_inner, radix.children.get(), radix.ranges.get(), radix.node_lo.get(), radix.node_hi.get(), leaves.lo.get(), leaves.hi.get(), fb.sp.pad, t.bvh2_nodes.get());
  hipLaunchKernelGGL(k_emit_tris, dim3(rblocks), dim3(256), 0, st, ctx->d_face_rec, ctx->d_face_cls, leaves.order.get(), nr, t.bvh2_tris.get(), r.ref_face);
  FH_HIP(hipGetLastError());
  FH_HIP(hipStreamSynchronize(st));
  t.bvh2_n_tris = nr;
  t.bvh2_n_nodes = n_inner;
  radix.root = 0;  // the radix tree's root is node 0
  return FH_OK;
}

// PLOC over the sorted leaves: rounds of nearest-neighbour search, merge of the mutual pairs and compaction until one cluster is left.  *failed (auto mode
// only; an explicit FH_BVH_BUILDER=ploc reports the error): no mutual pair found (non-finite boxes), or the last cluster is no inner node.
int build_ploc_tree(fh_ctx* ctx, uint32_t nr, const BuilderPlan& plan, const SortedLeaves& leaves, BinaryTree& tree, bool* failed)
{
  hipStream_t st = ctx->stream;
  const uint32_t n_inner = nr - 1, rblocks = (nr + 255) / 256;
  DeviceBuffer<int> cid_a, cid_b, nn;
  DeviceBuffer<float4> clo_a, chi_a, clo_b, chi_b;
  DeviceBuffer<uint32_t> valid, offset, node_counter;
  FH_HIP(cid_a.alloc(nr)); FH_HIP(cid_b.alloc(nr)); FH_HIP(nn.alloc(nr)); FH_HIP(clo_a.alloc(nr)); FH_HIP(chi_a.alloc(nr)); FH_HIP(clo_b.alloc(nr)); FH_HIP(chi_b.alloc(nr));
  FH_HIP(valid.alloc(nr)); FH_HIP(offset.alloc(nr)); FH_HIP(node_counter.alloc(1));
  FH_HIP(tree.children.alloc(n_inner)); FH_HIP(tree.ranges.alloc(n_inner)); FH_HIP(tree.node_lo.alloc(n_inner)); FH_HIP(tree.node_hi.alloc(n_inner));
  FH_HIP(hipMemsetAsync(node_counter.get(), 0, 4, st));
  hipLaunchKernelGGL(k_ploc_init, dim3(rblocks), dim3(256), 0, st, (int)nr, leaves.lo.get(), leaves.hi.get(), cid_a.get(), clo_a.get(), chi_a.get());
  size_t scan_bytes = 0;
  FH_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, valid.get(), offset.get(), 0u, (size_t)nr, rocprim::plus<uint32_t>(), st));
  DeviceBuffer<char> scan_tmp;
  FH_HIP(scan_tmp.alloc(scan_bytes));
  const int ploc_radius = kPlocRadius;  // neighbours searched to either side
  int* cid = cid_a.get(); int* cid_o = cid_b.get();
  float4 *clo = clo_a.get(), *chi = chi_a.get(), *clo_o = clo_b.get(), *chi_o = chi_b.get();
  uint32_t count = nr;
  for (int round = 0; count > 1 && round < 4096; ++round) {
    const uint32_t b = (count + 255) / 256;
    hipLaunchKernelGGL(k_ploc_nearest, dim3(b), dim3(256), 0, st, (int)count, clo, chi, nn.get(), ploc_radius);
    hipLaunchKernelGGL(k_ploc_merge, dim3(b), dim3(256), 0, st, (int)count, nn.get(), cid, clo, chi, valid.get(), tree.children.get(), tree.ranges.get(), tree.node_lo.get(), tree.node_hi.get(), node_counter.get());
    FH_HIP(rocprim::exclusive_scan(scan_tmp.get(), scan_bytes, valid.get(), offset.get(), 0u, (size_t)count, rocprim::plus<uint32_t>(), st));
    hipLaunchKernelGGL(k_ploc_compact, dim3(b), dim3(256), 0, st, (int)count, valid.get(), offset.get(), cid, clo, chi, cid_o, clo_o, chi_o);
    uint32_t next = 0;  // offset and flag of the last cluster -> new count
    if (const int rc = scan_total(ctx, offset.get(), valid.get(), count, &next)) return rc;
    if (next >= count) {
      if (ploc_failure_is_error(plan)) return fail(ctx, FH_E_INVALID, "PLOC made no progress");
      *failed = true;
      return FH_OK;
    }
    count = next;
    std::swap(cid, cid_o); std::swap(clo, clo_o); std::swap(chi, chi_o);
  }
  FH_HIP(hipMemcpyAsync(&tree.root, cid, 4, hipMemcpyDeviceToHost, st));
  FH_HIP(hipStreamSynchronize(st));
  if (tree.root < 0 || (uint32_t)tree.root >= n_inner) {
    if (ploc_failure_is_error(plan)) return fail(ctx, FH_E_INVALID, "PLOC did not end in one inner node");
    *failed = true;
  }
  return FH_OK;
}

// The binary tree the collapse takes.  While deciding (and for the debug line) the sums of the inner-node areas of both trees are measured: -29 % for PLOC on
// tools' `city`, 9 % faster frames; -9 % on the Sponza-class glTF, 5 % faster frames; on a uniform soup the two are within 3 % and the radix tree traverses faster
// (closest-hit rays need the well separated children of a Morton split for the octant order to work), so it stays.
int choose_builder(fh_ctx* ctx, uint32_t n_inner, const BuildSwitches& sw, const BuilderPlan& plan, bool ploc_failed, const BinaryTree& radix, const BinaryTree& ploc, const BinaryTree** chosen)
{
  hipStream_t st = ctx->stream;
  double h[2] = {0.0, 0.0};
  if (plan.deciding || sw.debug) {
    const uint32_t iblocks = (n_inner + 255) / 256;
    DeviceBuffer<double> sums;
    FH_HIP(sums.alloc(2));
    FH_HIP(hipMemsetAsync(sums.get(), 0, 16, st));
    hipLaunchKernelGGL(k_sah_sum, dim3(iblocks), dim3(256), 0, st, (int)n_inner, radix.node_lo.get(), radix.node_hi.get(), sums.get());
    if (plan.ploc && !ploc_failed) hipLaunchKernelGGL(k_sah_sum, dim3(iblocks), dim3(256), 0, st, (int)n_inner, ploc.node_lo.get(), ploc.node_hi.get(), sums.get() + 1);
    FH_HIP(hipMemcpyAsync(h, sums.get(), 16, hipMemcpyDeviceToHost, st));
    FH_HIP(hipStreamSynchronize(st));
  }
  const BuilderVerdict v = builder_verdict(plan, ploc_failed, h);
  if (v.choice) ctx->builder_choice = v.choice;
  if (sw.debug) fprintf(stderr, "[bvh] sum of inner-node areas: radix tree %.4f, PLOC %.4f -> %s\n", h[0], h[1], v.ploc ? "PLOC" : "radix tree");
  *chosen = v.ploc ? &ploc : &radix;
  return FH_OK;
}

// the cut of least summed wide-node area below every node of the binary tree (k_cut_tables), bottom up with the tree's parents
int fill_cut_tables(fh_ctx* ctx, uint32_t nr, const BuildSwitches& sw, const BinaryTree& tree, const SortedLeaves& leaves, DeviceBuffer<float>& cost_tab, DeviceBuffer<uint2>& decision)
{
  hipStream_t st = ctx->stream;
  const uint32_t n_inner = nr - 1;
  DeviceBuffer<int> node_parent, leaf_parent;
  FH_HIP(node_parent.alloc(n_inner)); FH_HIP(leaf_parent.alloc(nr)); FH_HIP(cost_tab.alloc(7ull * n_inner)); FH_HIP(decision.alloc(n_inner));
  FH_HIP(hipMemsetAsync(node_parent.get(), 0xff, 4ull * n_inner, st));  // the root keeps -1
  FH_HIP(hipMemsetAsync(leaves.arrive.get(), 0, 4ull * n_inner, st));
  hipLaunchKernelGGL(k_tree_parents, dim3((n_inner + 255) / 256), dim3(256), 0, st, (int)n_inner, tree.children.get(), node_parent.get(), leaf_parent.get());
  hipLaunchKernelGGL(k_cut_tables, dim3((nr + 255) / 256), dim3(256), 0, st, (int)nr, tree.children.get(), node_parent.get(), leaf_parent.get(), tree.node_lo.get(), tree.node_hi.get(), leaves.arrive.get(), cost_tab.get(),
                     decision.get());
  FH_HIP(hipGetLastError());
  FH_HIP(hipStreamSynchronize(st));  // (the parent arrays go out of scope here)
  if (sw.debug) {
    float c_root = 0.0f;
    FH_HIP(hipMemcpy(&c_root, cost_tab.get() + 7ull * (size_t)tree.root, 4, hipMemcpyDeviceToHost));
    fprintf(stderr, "[bvh] least summed area of the wide nodes (cut tables, root): %.4f\n", c_root);
  }
  return FH_OK;
}

// Collapse of the chosen binary tree to BVH8, breadth first, one launch per level; then the limits the traversal sets.  tri_slot: triangle slot of every sorted leaf.
// (SAH refinement of the binary tree by parallel reinsertion, Meister & Bittner 2018, was built in round 5: the summed inner-node area falls by 2-7 %, the node visits per
// ray do not -- 15.28 -> 15.12 on configs[2], 11.73 -> 11.81 on configs[3].  profiles/README.md r5-1, tools/patches/r6_pruned_switches.patch)
int collapse_wide(fh_ctx* ctx, uint32_t n, uint32_t nr, const BuildSwitches& sw, float pad, const BinaryTree& tree, const SortedLeaves& leaves, DeviceBuffer<uint32_t>& tri_slot, NewTree& t)
{
  hipStream_t st = ctx->stream;
  const uint32_t n_inner = nr - 1;
  const CollapsePlan plan = collapse_plan(sw);
  DeviceBuffer<Work8> work_a, work_b;
  DeviceBuffer<uint32_t> counters;  // [0] node counter, [1] triangle counter, [2] next-level item count
  FH_HIP(work_a.alloc(n_inner)); FH_HIP(work_b.alloc(n_inner)); FH_HIP(counters.alloc(3)); FH_HIP(tri_slot.alloc(nr));
  FH_HIP(t.bvh8_nodes.alloc((size_t)kBvh8NodeVec * n_inner));
  FH_HIP(t.bvh8_parent.alloc(n_inner));
  FH_HIP(t.face_node.alloc(n));
  FH_HIP(hipMemsetAsync(t.bvh8_parent.get(), 0xff, 4ull * n_inner, st));  // (the root keeps 0xffffffff: no way up)
  FH_HIP(hipMemsetAsync(t.face_node.get(), 0xff, 4ull * n, st));
  DeviceBuffer<float> cut_cost_tab;
  DeviceBuffer<uint2> cut_decision;
  if (plan.optimal_cut)
    if (const int rc = fill_cut_tables(ctx, nr, sw, tree, leaves, cut_cost_tab, cut_decision)) return rc;
  const Work8 root{tree.root, 0u};
  const uint32_t init_counters[3] = {1u, 0u, 0u};
  FH_HIP(hipMemcpyAsync(work_a.get(), &root, sizeof root, hipMemcpyHostToDevice, st));
  FH_HIP(hipMemcpyAsync(counters.get(), init_counters, sizeof init_counters, hipMemcpyHostToDevice, st));
  uint32_t level_count = 1;
  Work8* cur = work_a.get();
  Work8* nxt = work_b.get();
  for (int level = 0; level < 64 && level_count > 0; ++level) {
    ++t.levels;
    t.level_start.push_back(t.level_start.back() + level_count);
    FH_HIP(hipMemsetAsync(counters.get() + 2, 0, 4, st));
    hipLaunchKernelGGL(k_collapse8, dim3((level_count + 63) / 64), dim3(64), 0, st, cur, level_count, tree.children.get(), tree.ranges.get(), tree.node_lo.get(), tree.node_hi.get(), leaves.lo.get(), leaves.hi.get(), pad,
                       plan.leaf_max8, plan.absorb8, t.bvh8_nodes.get(), counters.get(), counters.get() + 1, tri_slot.get(), nxt, counters.get() + 2, plan.optimal_cut ? cut_decision.get() : (const uint2*)nullptr, t.bvh8_parent.get());
    FH_HIP(hipMemcpyAsync(&level_count, counters.get() + 2, 4, hipMemcpyDeviceToHost, st));
    FH_HIP(hipStreamSynchronize(st));
    std::swap(cur, nxt);
  }
  uint32_t final_counters[2] = {0, 0};
  FH_HIP(hipMemcpyAsync(final_counters, counters.get(), 8, hipMemcpyDeviceToHost, st));
  FH_HIP(hipStreamSynchronize(st));
  const BuildError e = collapse_limits(final_counters[1], nr, t.levels, final_counters[0], (uint32_t)kBvh8Stack, kCoopMaxTris, FH_E_INVALID, FH_E_UNSUPPORTED);
  if (e.code) return fail(ctx, e.code, e.msg);
  t.bvh8_n_nodes = final_counters[0];
  return FH_OK;
}

// the triangle copies of the wide tree, one slot per child slot; the wide node of every face, also into the face's record
int emit_wide_triangles(fh_ctx* ctx, uint32_t n, const References& r, const SortedLeaves& leaves, const DeviceBuffer<uint32_t>& tri_slot, NewTree& t)
{
  hipStream_t st = ctx->stream;
  const uint32_t n_slots = 8u * t.bvh8_n_nodes;
  FH_HIP(t.bvh8_tris.alloc(3ull * n_slots));
  hipLaunchKernelGGL(k_clear_tris8, dim3((n_slots + 255) / 256), dim3(256), 0, st, t.bvh8_tris.get(), n_slots);
  hipLaunchKernelGGL(k_emit_tris8, dim3((r.nr + 255) / 256), dim3(256), 0, st, ctx->d_face_rec, ctx->d_face_cls, leaves.order.get(), tri_slot.get(), r.nr, t.bvh8_tris.get(), r.ref_face, t.face_node.get(),
                     r.ref_face ? r.split_count.get() : (const uint32_t*)nullptr);
  hipLaunchKernelGGL(k_face_node_to_rec, dim3((n + 255) / 256), dim3(256), 0, st, t.face_node.get(), n, ctx->d_face_rec);
  FH_HIP(hipGetLastError());
  FH_HIP(hipStreamSynchronize(st));
  t.bvh8_n_tris = r.nr;
  t.use_bvh8 = true;
  return FH_OK;
}

// what a later refit needs: the level ranges, the full-precision node boxes and the area the tree has now
int keep_for_refit(fh_ctx* ctx, uint32_t n, uint32_t nr, float pad, NewTree& t)
{
  if (!tree_refittable(nr, n, t.level_start.back(), t.bvh8_n_nodes)) return FH_OK;
  FH_HIP(t.bvh8_box.alloc(2ull * t.bvh8_n_nodes));
  if (const int rc = refit_levels(ctx, t.bvh8_nodes.get(), t.bvh8_tris.get(), t.bvh8_box.get(), t.level_start, t.bvh8_n_nodes, pad, 0, &t.area_built)) return rc;
  t.refit_ok = true;
  return FH_OK;
}

}  // namespace

void reset_tree_measurements(fh_ctx* ctx)
{
  // a new tree: where its rays should start is measured again (render.hip), and how long its paths live is not known yet.  (This also zeroes survival[], which nobody can
  // see: survival_n gates every read.)  Known gap, ADVICE.md finding 1: a counter snapshot recorded before the rebuild still refills the shares when it arrives afterwards
  ctx->tree = {};
}

int bvh_build_device(fh_ctx* ctx)
{
  const TimePoint t_begin = std::chrono::steady_clock::now();
  const uint32_t n = ctx->n_faces;
  const BuildSwitches sw = read_build_switches();
  bool refitted = false;
  if (const int rc = try_refit(ctx, n, sw, t_begin, &refitted)) return rc;
  if (refitted) return FH_OK;
  reset_tree_measurements(ctx);
  clear_tree(ctx, n);
  const TreeShape shape = tree_shape(n, kLeafMax8, kLeafMax2);
  if (shape == TreeShape::Empty) return FH_OK;

  FaceBounds fb;
  SortedLeaves leaves;  // (these three outlive the timed part of the build, like the boxes of the faces)
  BinaryTree radix;
  NewTree tree;
  if (const int rc = scene_bounds(ctx, n, false, fb)) return rc;
  if (shape != TreeShape::Full) {
    if (const int rc = build_tiny(ctx, n, shape == TreeShape::WideRoot, fb, tree)) return rc;
    commit_tiny(ctx, sw, fb.sp, tree);
  } else {
    References refs;
    BinaryTree ploc;
    const BinaryTree* chosen = nullptr;
    DeviceBuffer<uint32_t> tri_slot;
    bool ploc_failed = false;
    if (const int rc = split_references(ctx, n, sw, fb, refs)) return rc;
    if (const int rc = build_radix_tree(ctx, refs, fb, leaves, radix, tree)) return rc;
    const BuilderPlan plan = builder_plan(ctx->builder_choice, sw);
    if (plan.ploc)
      if (const int rc = build_ploc_tree(ctx, refs.nr, plan, leaves, ploc, &ploc_failed)) return rc;
    if (const int rc = choose_builder(ctx, refs.nr - 1, sw, plan, ploc_failed, radix, ploc, &chosen)) return rc;
    if (const int rc = collapse_wide(ctx, n, refs.nr, sw, fb.sp.pad, *chosen, leaves, tri_slot, tree)) return rc;
    if (const int rc = emit_wide_triangles(ctx, n, refs, leaves, tri_slot, tree)) return rc;
    if (const int rc = keep_for_refit(ctx, n, refs.nr, fb.sp.pad, tree)) return rc;
    commit_full(ctx, sw, fb.sp, tree);
  }
  publish_stats(ctx, t_begin);
  return FH_OK;
}

}  // namespace fh

