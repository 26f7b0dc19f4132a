// group.hip -- one frame on several GPUs from a single context (fh_ctx_create_group, include/fredholm_hip.h).
//
// A group owns n plain contexts, one per entry of devices[]; member i renders the tiles t with t % n == i (fh_set_tile_shard).  Member 0, the LEAD, renders straight into
// the caller's buffers; every other member accumulates in six full-size layers of its own, and after its passes ONE launch (k_pack_layers) packs the owned pixels of the
// selected layers into a staging buffer, ONE peer copy moves it to the lead's device, and ONE launch on the lead's stream (k_unpack_group) un-permutes all shards into the
// caller's buffers.  Streams wait on events; the host waits for nothing.  There is one code path: members on the same device go through staging, copy and unpack as well.
#include <hip/hip_runtime.h>

#include <cstring>

#include "context.h"

struct fh_group {
  uint32_t n = 0;
  std::vector<fh_ctx*> m;  // m[0]: the lead
  uint32_t mask = FH_LAYER_ALL;
  bool scene_in_doubt = false, frame_in_doubt = false;  // a broadcast failed half way: fh_render refuses until fh_scene_upload / fh_set_resolution succeeded again
  bool sized = false;
  struct Member {
    // (what lives on the member's device is released with that device current: free_frame_buffers, group_destroy)
    fh::DeviceBuffer<float> layers[6];      // full-size, on the member's device: its running means live here
    fh::DeviceBuffer<uint8_t> staging;      // packed shard, on the member's device
    size_t lead_offset = 0;                 // where the shard goes in the lead's staging area
    fh::Event ev_pack_begin, ev_packed;     // member's device
    fh::Event ev_copy_begin, ev_copied;     // lead's device
    bool copy_recorded = false, timed = false;
  };
  std::vector<Member> mem;
  fh::Stream copy_stream;                  // lead's device
  fh::DeviceBuffer<uint8_t> lead_staging;
  fh::Event ev_unpack_begin, ev_unpacked;  // lead's device
  bool unpack_recorded = false, unpack_timed = false;
};

namespace fh {
namespace {

constexpr uint32_t kLayerBytes[6] = {16u, 16u, 4u, 16u, 16u, 16u};  // beauty, position, depth, normal, texcoord, albedo (bit k of the gather mask)
constexpr uint32_t kGroupBlock = 256;

__host__ __device__ inline size_t round16(size_t b) { return (b + 15u) & ~(size_t)15u; }

// what one gather moves: up to six arrays of 4, 8 or 16 bytes per pixel
struct Slots { uint32_t n = 0; uint32_t bpp[6] = {0, 0, 0, 0, 0, 0}; };
size_t shard_bytes(const Slots& s, uint32_t n_owned)
{
  size_t b = 0;
  for (uint32_t k = 0; k < s.n; ++k) b += round16((size_t)n_owned * s.bpp[k]);
  return b;
}
Slots layer_slots(uint32_t mask)
{
  Slots s;
  for (uint32_t k = 0; k < 6u; ++k)
    if (mask & (1u << k)) s.bpp[s.n++] = kLayerBytes[k];
  return s;
}

// one member's shard: array after array (blockIdx.y), each in ownership-list order and padded to 16 bytes; every thread writes 16 bytes (1, 2 or 4 pixels)
struct PackArgs { const uint8_t* src[6]; uint32_t bpp[6]; const uint32_t* owned; uint32_t n; uint8_t* dst; };
__global__ void __launch_bounds__(kGroupBlock) k_pack_layers(PackArgs a)
{
  const uint32_t s = blockIdx.y, bpp = a.bpp[s];
  size_t off = 0;
  for (uint32_t t = 0; t < s; ++t) off += round16((size_t)a.n * a.bpp[t]);
  float4* dst = (float4*)(a.dst + off);
  const uint32_t per = 16u / bpp, units = (a.n + per - 1u) / per;
  for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < units; u += gridDim.x * blockDim.x) {
    if (bpp == 16u) {
      dst[u] = ((const float4*)a.src[s])[a.owned[u]];
    } else if (bpp == 8u) {
      const float2* src = (const float2*)a.src[s];
      const float2 lo = src[a.owned[2u * u]];
      const float2 hi = 2u * u + 1u < a.n ? src[a.owned[2u * u + 1u]] : make_float2(0.0f, 0.0f);
      dst[u] = make_float4(lo.x, lo.y, hi.x, hi.y);
    } else {
      const float* src = (const float*)a.src[s];  // (bits are moved, whatever the type)
      float v[4];
      for (uint32_t k = 0; k < 4u; ++k) v[k] = 4u * u + k < a.n ? src[a.owned[4u * u + k]] : 0.0f;
      dst[u] = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
}

// every non-lead member's shard of every selected array into the frame: `all_owned` is the ownership lists of members 0 .. world - 1 back to back (fh_ctx::FrameMap),
// start[r] where member r's begins, base[r] its packed shard on this device
struct UnpackArgs { const uint8_t* base[kMaxShardsPerLaunch]; uint32_t start[kMaxShardsPerLaunch + 1]; uint32_t world; uint32_t bpp[6]; uint8_t* dst[6]; const uint32_t* all_owned; };
__global__ void __launch_bounds__(kGroupBlock) k_unpack_group(UnpackArgs a)
{
  const uint32_t s = blockIdx.y, bpp = a.bpp[s];
  const uint32_t first = a.start[1], total = a.start[a.world] - first;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const uint32_t j = first + i;
    uint32_t r = 1;
    while (r + 1u < a.world && j >= a.start[r + 1u]) ++r;
    const uint32_t n_r = a.start[r + 1u] - a.start[r], k = j - a.start[r];
    size_t off = 0;
    for (uint32_t t = 0; t < s; ++t) off += round16((size_t)n_r * a.bpp[t]);
    const uint8_t* src = a.base[r] + off + (size_t)k * bpp;
    const uint32_t px = a.all_owned[j];
    if (bpp == 16u) ((float4*)a.dst[s])[px] = *(const float4*)src;
    else if (bpp == 8u) ((float2*)a.dst[s])[px] = *(const float2*)src;
    else ((float*)a.dst[s])[px] = *(const float*)src;
  }
}

uint32_t grid_for(uint32_t n) { return (n + kGroupBlock - 1u) / kGroupBlock; }

#define GROUP_HIP(g, call)                                                                                        \
  do {                                                                                                            \
    hipError_t e_ = (call);                                                                                       \
    if (e_ != hipSuccess) return fail(g, FH_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_));             \
  } while (0)

void free_frame_buffers(fh_group* G)
{
  if (G->m.empty()) return;
  for (uint32_t i = 1; i < (uint32_t)G->m.size(); ++i) {
    fh_group::Member& M = G->mem[i];
    (void)hipSetDevice(G->m[i]->device);
    (void)hipStreamSynchronize(G->m[i]->stream);
    for (auto& l : M.layers) l.reset();
    M.staging.reset();
    M.copy_recorded = false;
  }
  (void)hipSetDevice(G->m[0]->device);
  if (G->copy_stream) (void)hipStreamSynchronize(G->copy_stream);
  (void)hipStreamSynchronize(G->m[0]->stream);
  G->lead_staging.reset();
  G->unpack_recorded = false;
  G->sized = false;
}

// staging of every member for its ownership as it is now, and the lead's frame map; with_layers: the members' own layers too (a new resolution)
int size_frame_buffers(fh_ctx* g, bool with_layers)
{
  fh_group* G = g->group;
  fh_ctx* lead = G->m[0];
  const size_t px = (size_t)lead->width * lead->height;
  const Slots all = layer_slots(FH_LAYER_ALL);
  size_t lead_bytes = 0;
  for (uint32_t i = 1; i < G->n; ++i) {
    fh_group::Member& M = G->mem[i];
    fh_ctx* c = G->m[i];
    GROUP_HIP(g, hipSetDevice(c->device));
    GROUP_HIP(g, hipStreamSynchronize(c->stream));
    if (with_layers) {
      for (uint32_t k = 0; k < 6u; ++k) {
        GROUP_HIP(g, M.layers[k].alloc(px * kLayerBytes[k] / sizeof(float)));
        GROUP_HIP(g, hipMemsetAsync(M.layers[k], 0, px * kLayerBytes[k], c->stream));
      }
    }
    const size_t bytes = shard_bytes(all, c->n_owned);
    GROUP_HIP(g, M.staging.alloc(bytes));
    M.lead_offset = lead_bytes;
    M.copy_recorded = false;
    lead_bytes += bytes;
  }
  GROUP_HIP(g, hipSetDevice(lead->device));
  GROUP_HIP(g, hipStreamSynchronize(G->copy_stream));
  GROUP_HIP(g, hipStreamSynchronize(lead->stream));
  GROUP_HIP(g, G->lead_staging.alloc(lead_bytes));
  G->unpack_recorded = false;
  const int rc = frame_map_ensure(lead, G->n);
  if (rc) return rc;
  G->sized = true;
  return FH_OK;
}

// pack on every member's stream, copy on the lead's copy stream, one unpack on the lead's stream: src(i, k) = array k of member i, dst[k] = where it goes on the lead
int gather(fh_ctx* g, const Slots& slots, const std::function<const void*(uint32_t, uint32_t)>& src, void* const dst[6])
{
  fh_group* G = g->group;
  fh_ctx* lead = G->m[0];
  if (slots.n == 0) return FH_OK;
  const bool timed = (lead->flags & FH_FLAG_TIME_KERNELS) != 0;
  GROUP_HIP(g, hipSetDevice(lead->device));
  if (G->unpack_recorded) GROUP_HIP(g, hipStreamWaitEvent(G->copy_stream, G->ev_unpacked, 0));  // the previous unpack has read the lead's staging area
  UnpackArgs ua{};
  ua.world = G->n;
  uint32_t n_remote = 0;
  for (uint32_t i = 1; i < G->n; ++i) {
    fh_group::Member& M = G->mem[i];
    fh_ctx* c = G->m[i];
    ua.base[i] = G->lead_staging + M.lead_offset;
    M.timed = false;
    if (c->n_owned == 0) continue;
    n_remote += c->n_owned;
    const size_t bytes = shard_bytes(slots, c->n_owned);
    PackArgs pa{};
    for (uint32_t k = 0; k < slots.n; ++k) { pa.src[k] = (const uint8_t*)src(i, k); pa.bpp[k] = slots.bpp[k]; }
    pa.owned = c->d_owned; pa.n = c->n_owned; pa.dst = M.staging;
    GROUP_HIP(g, hipSetDevice(c->device));
    if (M.copy_recorded) GROUP_HIP(g, hipStreamWaitEvent(c->stream, M.ev_copied, 0));  // staging reuse: the previous call's copy has read it
    if (timed) GROUP_HIP(g, hipEventRecord(M.ev_pack_begin, c->stream));
    hipLaunchKernelGGL(k_pack_layers, dim3(grid_for(c->n_owned), slots.n), dim3(kGroupBlock), 0, c->stream, pa);
    GROUP_HIP(g, hipGetLastError());
    GROUP_HIP(g, hipEventRecord(M.ev_packed, c->stream));
    GROUP_HIP(g, hipSetDevice(lead->device));
    GROUP_HIP(g, hipStreamWaitEvent(G->copy_stream, M.ev_packed, 0));
    if (timed) GROUP_HIP(g, hipEventRecord(M.ev_copy_begin, G->copy_stream));
    if (c->device == lead->device) GROUP_HIP(g, hipMemcpyAsync(G->lead_staging + M.lead_offset, M.staging, bytes, hipMemcpyDeviceToDevice, G->copy_stream));
    else GROUP_HIP(g, hipMemcpyPeerAsync(G->lead_staging + M.lead_offset, lead->device, M.staging, c->device, bytes, G->copy_stream));
    GROUP_HIP(g, hipEventRecord(M.ev_copied, G->copy_stream));
    M.copy_recorded = true;
    M.timed = timed;
    GROUP_HIP(g, hipStreamWaitEvent(lead->stream, M.ev_copied, 0));
  }
  G->unpack_timed = false;
  if (n_remote == 0) return FH_OK;
  const fh_ctx::FrameMap& fm = lead->frame_map;
  for (uint32_t r = 0; r <= G->n; ++r) ua.start[r] = fm.start[r];
  for (uint32_t k = 0; k < slots.n; ++k) { ua.bpp[k] = slots.bpp[k]; ua.dst[k] = (uint8_t*)dst[k]; }
  ua.all_owned = fm.d_all;
  GROUP_HIP(g, hipSetDevice(lead->device));
  if (timed) GROUP_HIP(g, hipEventRecord(G->ev_unpack_begin, lead->stream));
  hipLaunchKernelGGL(k_unpack_group, dim3(grid_for(n_remote), slots.n), dim3(kGroupBlock), 0, lead->stream, ua);
  GROUP_HIP(g, hipGetLastError());
  GROUP_HIP(g, hipEventRecord(G->ev_unpacked, lead->stream));
  G->unpack_recorded = true;
  G->unpack_timed = timed;
  return FH_OK;
}

int check_frame(fh_ctx* g, const char* what)
{
  fh_group* G = g->group;
  if (G->scene_in_doubt) return fail(g, FH_E_INVALID, std::string(what) + ": an earlier call failed on some member of the group; call fh_scene_upload again");
  if (G->frame_in_doubt) return fail(g, FH_E_INVALID, std::string(what) + ": an earlier call failed on some member of the group; call fh_set_resolution again");
  if (!G->sized) return fail(g, FH_E_INVALID, std::string(what) + ": resolution not set");
  return FH_OK;
}

}  // namespace

fh_ctx* group_lead(fh_ctx* g) { return g->group->m[0]; }

int group_each(fh_ctx* g, int kind, const std::function<int(fh_ctx*, uint32_t)>& call)
{
  fh_group* G = g->group;
  for (uint32_t i = 0; i < G->n; ++i) {
    const int rc = call(G->m[i], i);
    if (rc) {
      g->err = "member " + std::to_string(i) + ": " + G->m[i]->err;
      // members before i took the call and member i may have taken part of it: they can disagree now, unless member 0 refused its arguments
      if (i > 0 || rc == FH_E_HIP) {
        if (kind == kGroupCallScene || kind == kGroupCallUpload) G->scene_in_doubt = true;
        if (kind == kGroupCallFrame) G->frame_in_doubt = true;
      }
      return rc;
    }
  }
  if (kind == kGroupCallUpload) G->scene_in_doubt = false;
  return FH_OK;
}

int group_destroy(fh_ctx* g)
{
  fh_group* G = g->group;
  if (!G->m.empty()) {
    free_frame_buffers(G);
    for (uint32_t i = 1; i < (uint32_t)G->m.size(); ++i) {
      (void)hipSetDevice(G->m[i]->device);
      G->mem[i].ev_pack_begin.reset(); G->mem[i].ev_packed.reset();
      (void)hipSetDevice(G->m[0]->device);
      G->mem[i].ev_copy_begin.reset(); G->mem[i].ev_copied.reset();
    }
    (void)hipSetDevice(G->m[0]->device);
    G->ev_unpack_begin.reset(); G->ev_unpacked.reset();
    G->copy_stream.reset();
  }
  int rc = FH_OK;
  for (fh_ctx* c : G->m) {
    c->owner = nullptr;
    const int r = fh_ctx_destroy(c);
    if (r && !rc) rc = r;
  }
  delete G;
  delete g;
  return rc;
}

int group_set_resolution(fh_ctx* g, uint32_t w, uint32_t h)
{
  fh_group* G = g->group;
  const int rc = group_each(g, kGroupCallFrame, [&](fh_ctx* c, uint32_t) { return fh_set_resolution(c, w, h); });
  if (rc) return rc;
  const int rs = size_frame_buffers(g, true);
  G->frame_in_doubt = rs != FH_OK;
  return rs;
}

int group_set_tile_shard(fh_ctx* g, uint32_t rank, uint32_t world, uint32_t tw, uint32_t th)
{
  fh_group* G = g->group;
  if (rank != 0 || world != 1) return fail(g, FH_E_INVALID, "fh_set_tile_shard: a group is the whole frame; only (0, 1, tile_w, tile_h) sets its tile size");
  if (tw == 0 || th == 0) return fail(g, FH_E_INVALID, "bad shard");
  const int rc = group_each(g, kGroupCallFrame, [&](fh_ctx* c, uint32_t i) { return fh_set_tile_shard(c, i, G->n, tw, th); });
  if (rc) return rc;
  if (G->m[0]->width == 0) return FH_OK;  // (no resolution yet: fh_set_resolution sizes the staging)
  const int rs = size_frame_buffers(g, false);
  if (rs) G->frame_in_doubt = true;
  return rs;
}

int group_init_render_states(fh_ctx* g)
{
  fh_group* G = g->group;
  const int rc = group_each(g, kGroupCallFrame, [&](fh_ctx* c, uint32_t) { return fh_init_render_states(c); });
  if (rc) return rc;
  const size_t px = (size_t)G->m[0]->width * G->m[0]->height;
  for (uint32_t i = 1; i < G->n && G->sized; ++i) {
    GROUP_HIP(g, hipSetDevice(G->m[i]->device));
    for (uint32_t k = 0; k < 6u; ++k) GROUP_HIP(g, hipMemsetAsync(G->mem[i].layers[k], 0, px * kLayerBytes[k], G->m[i]->stream));
  }
  return FH_OK;
}

int group_render(fh_ctx* g, const fh_camera* cam, const float* bg, const fh_render_layers* layers, uint32_t n_samples, uint32_t max_depth, uint32_t seed)
{
  fh_group* G = g->group;
  if (!cam || !bg || !layers || !layers->beauty || !layers->position || !layers->depth || !layers->normal || !layers->texcoord || !layers->albedo)
    return fail(g, FH_E_INVALID, "fh_render: null argument");
  int rc = check_frame(g, "fh_render");
  if (rc) return rc;
  // every member is submitted before anything waits: a plain context's fh_render does not synchronise with the host inside a frame (adaptive rounds do: DESIGN.md 6)
  rc = group_each(g, kGroupCallFrame, [&](fh_ctx* c, uint32_t i) {
    if (i == 0) return fh_render(c, cam, bg, layers, n_samples, max_depth, seed);
    const fh_group::Member& M = G->mem[i];
    const fh_render_layers own{M.layers[0], M.layers[1], M.layers[2], M.layers[3], M.layers[4], M.layers[5]};
    return fh_render(c, cam, bg, &own, n_samples, max_depth, seed);
  });
  if (rc) return rc;  // (group_each: unless the lead refused the arguments, the members' accumulations differ now and the next call is refused)
  if (n_samples == 0) return FH_OK;
  const Slots slots = layer_slots(G->mask);
  uint32_t which[6], n = 0;
  for (uint32_t k = 0; k < 6u; ++k)
    if (G->mask & (1u << k)) which[n++] = k;
  void* const caller[6] = {layers->beauty, layers->position, layers->depth, layers->normal, layers->texcoord, layers->albedo};
  void* dst[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  for (uint32_t k = 0; k < n; ++k) dst[k] = caller[which[k]];
  rc = gather(g, slots, [&](uint32_t i, uint32_t k) { return (const void*)G->mem[i].layers[which[k]]; }, dst);
  if (rc) G->frame_in_doubt = true;
  return rc;
}

int group_get_sample_counts(fh_ctx* g, uint32_t* counts)
{
  fh_group* G = g->group;
  if (!counts) return fail(g, FH_E_INVALID, "fh_get_sample_counts: null argument");
  int rc = check_frame(g, "fh_get_sample_counts");
  if (rc) return rc;
  rc = fh_get_sample_counts(G->m[0], counts);  // the lead's pixels (and zeros elsewhere) on the lead's stream; the unpack after it brings the others
  if (rc) return rc;
  Slots s;
  s.n = 1; s.bpp[0] = 4;
  void* dst[6] = {counts, nullptr, nullptr, nullptr, nullptr, nullptr};
  return gather(g, s, [&](uint32_t i, uint32_t) { return (const void*)G->m[i]->d_sample_count; }, dst);
}

int group_get_luminance_moments(fh_ctx* g, float* moments)
{
  fh_group* G = g->group;
  if (!moments) return fail(g, FH_E_INVALID, "fh_get_luminance_moments: null argument");
  int rc = check_frame(g, "fh_get_luminance_moments");
  if (rc) return rc;
  for (uint32_t i = 0; i < G->n; ++i)
    if (!G->m[i]->adaptive || !G->m[i]->d_moments) return fail(g, FH_E_INVALID, "fh_get_luminance_moments: adaptive sampling is off");
  rc = fh_get_luminance_moments(G->m[0], moments);
  if (rc) return rc;
  Slots s;
  s.n = 1; s.bpp[0] = 8;
  void* dst[6] = {moments, nullptr, nullptr, nullptr, nullptr, nullptr};
  return gather(g, s, [&](uint32_t i, uint32_t) { return (const void*)G->m[i]->d_moments; }, dst);
}

int group_active_pixel_count(fh_ctx* g, uint32_t* out)
{
  if (!out) return fail(g, FH_E_INVALID, "fh_active_pixel_count: null argument");
  uint32_t sum = 0;
  const int rc = group_each(g, kGroupCallPlain, [&](fh_ctx* c, uint32_t) { uint32_t v = 0; const int r = fh_active_pixel_count(c, &v); sum += v; return r; });
  if (rc) return rc;
  *out = sum;
  return FH_OK;
}

int group_owned_pixel_count(fh_ctx* g, uint32_t* out)
{
  if (!out) return FH_E_INVALID;
  *out = g->group->m[0]->width * g->group->m[0]->height;
  return FH_OK;
}

int group_path_pool_allocated(fh_ctx* g, uint64_t* bytes, uint64_t* paths)
{
  if (!bytes || !paths) return fail(g, FH_E_INVALID, "fh_path_pool_allocated: null argument");
  uint64_t b = 0, p = 0;
  const int rc = group_each(g, kGroupCallPlain, [&](fh_ctx* c, uint32_t) { uint64_t bb = 0, pp = 0; const int r = fh_path_pool_allocated(c, &bb, &pp); b += bb; p += pp; return r; });
  if (rc) return rc;
  *bytes = b; *paths = p;
  return FH_OK;
}

// counters and histograms are summed, every *_ms is the maximum over the members (they run side by side), bvh_* are the lead's
int group_get_stats(fh_ctx* g, fh_stats* out)
{
  fh_group* G = g->group;
  if (!out) return FH_E_INVALID;
  fh_stats a = G->m[0]->stats;
  for (uint32_t i = 1; i < G->n; ++i) {
    const fh_stats& s = G->m[i]->stats;
    double* const ams[] = {&a.render_ms, &a.trace_closest_ms, &a.trace_shadow_ms, &a.shade_ms, &a.tail_ms, &a.generate_ms, &a.accumulate_ms, &a.queue_ms, &a.post_ms};
    const double sms[] = {s.render_ms, s.trace_closest_ms, s.trace_shadow_ms, s.shade_ms, s.tail_ms, s.generate_ms, s.accumulate_ms, s.queue_ms, s.post_ms};
    for (int k = 0; k < 9; ++k)
      if (sms[k] > *ams[k]) *ams[k] = sms[k];
    a.n_closest_launches += s.n_closest_launches; a.n_shadow_launches += s.n_shadow_launches;
    a.rays_closest += s.rays_closest; a.rays_shadow += s.rays_shadow;
    a.nodes_closest += s.nodes_closest; a.tris_closest += s.tris_closest; a.nodes_shadow += s.nodes_shadow; a.tris_shadow += s.tris_shadow;
    a.paths += s.paths;
    a.wave_node_steps_closest += s.wave_node_steps_closest; a.wave_tri_steps_closest += s.wave_tri_steps_closest;
    a.wave_node_steps_shadow += s.wave_node_steps_shadow; a.wave_tri_steps_shadow += s.wave_tri_steps_shadow;
    for (int k = 0; k < 8; ++k) { a.hist_nodes_closest[k] += s.hist_nodes_closest[k]; a.hist_nodes_shadow[k] += s.hist_nodes_shadow[k]; }
    a.n_generate_launches += s.n_generate_launches; a.n_accumulate_launches += s.n_accumulate_launches; a.n_shade_launches += s.n_shade_launches; a.n_tail_launches += s.n_tail_launches;
    a.shaded_hits += s.shaded_hits; a.n_post_launches += s.n_post_launches;
    a.clk_cycles_closest += s.clk_cycles_closest; a.clk_ticks_closest += s.clk_ticks_closest; a.clk_cycles_shadow += s.clk_cycles_shadow; a.clk_ticks_shadow += s.clk_ticks_shadow;
    a.n_passes += s.n_passes; a.sky_pixel_samples += s.sky_pixel_samples; a.div_range_violations += s.div_range_violations;
  }
  *out = a;
  return FH_OK;
}

}  // namespace fh

using namespace fh;

extern "C" {

int fh_ctx_create_group(const int* devices, uint32_t n, fh_ctx** out)
{
  if (out) *out = nullptr;
  if (!devices || !out) return fail(nullptr, FH_E_INVALID, "fh_ctx_create_group: null argument");
  if (n == 0 || n > kMaxShardsPerLaunch) return fail(nullptr, FH_E_INVALID, "fh_ctx_create_group: a group has 1 to 16 members");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return fail(nullptr, FH_E_HIP, "no HIP device available: the fredholm HIP path has no CPU fallback");
  for (uint32_t i = 0; i < n; ++i)
    if (devices[i] < 0 || devices[i] >= n_dev) return fail(nullptr, FH_E_INVALID, "fh_ctx_create_group: device index out of range (entry " + std::to_string(i) + ")");
  if (n == 1) return fh_ctx_create(devices[0], out);
  fh_ctx* g = new fh_ctx;
  fh_group* G = new fh_group;
  g->group = G;
  g->device = devices[0];
  G->n = n;
  G->mem.resize(n);
  auto bail = [&](int code, const std::string& msg) {  // nothing is left behind: the members made so far, their streams and events go with the group
    for (fh_ctx* c : G->m) c->owner = nullptr;
    (void)group_destroy(g);
    return fail(nullptr, code, msg);
  };
  for (uint32_t i = 0; i < n; ++i) {
    fh_ctx* c = nullptr;
    const int rc = fh_ctx_create(devices[i], &c);
    if (rc) return bail(rc, "fh_ctx_create_group: member " + std::to_string(i) + ": " + fh_last_error(nullptr));
    G->m.push_back(c);
  }
  for (uint32_t i = 0; i < n; ++i) {
    fh_ctx* c = G->m[i];
    c->owner = g;
    c->member_index = i;
    c->pool_share = 0;
    for (uint32_t j = 0; j < n; ++j) c->pool_share += devices[j] == devices[i] ? 1u : 0u;
    const int rc = fh_set_tile_shard(c, i, n, c->tile_w, c->tile_h);
    if (rc) return bail(rc, "fh_ctx_create_group: " + std::string(c->err));
  }
  // peer access is tried once, in both directions; a refusal is not an error (the peer copy then goes through the host)
  for (uint32_t i = 1; i < n; ++i) {
    const int a = devices[0], b = devices[i];
    if (a == b) continue;
    int can = 0;
    if (hipSetDevice(a) == hipSuccess && hipDeviceCanAccessPeer(&can, a, b) == hipSuccess && can) (void)hipDeviceEnablePeerAccess(b, 0);
    can = 0;
    if (hipSetDevice(b) == hipSuccess && hipDeviceCanAccessPeer(&can, b, a) == hipSuccess && can) (void)hipDeviceEnablePeerAccess(a, 0);
    (void)hipGetLastError();  // (hipErrorPeerAccessAlreadyEnabled: a second group on the same devices)
  }
  bool ok = hipSetDevice(devices[0]) == hipSuccess && G->copy_stream.create(hipStreamNonBlocking) == hipSuccess;
  ok = ok && G->ev_unpack_begin.create() == hipSuccess && G->ev_unpacked.create() == hipSuccess;
  for (uint32_t i = 1; i < n && ok; ++i) {
    fh_group::Member& M = G->mem[i];
    ok = hipSetDevice(devices[i]) == hipSuccess && M.ev_pack_begin.create() == hipSuccess && M.ev_packed.create() == hipSuccess;
    ok = ok && hipSetDevice(devices[0]) == hipSuccess && M.ev_copy_begin.create() == hipSuccess && M.ev_copied.create() == hipSuccess;
  }
  if (!ok) return bail(FH_E_HIP, "fh_ctx_create_group: stream / event creation failed");
  *out = g;
  return FH_OK;
}

int fh_ctx_group_size(fh_ctx* ctx, uint32_t* n)
{
  if (!ctx) return FH_E_INVALID;
  if (!n) return fail(ctx, FH_E_INVALID, "fh_ctx_group_size: null argument");
  *n = ctx->group ? ctx->group->n : 1u;
  return FH_OK;
}

int fh_ctx_member(fh_ctx* ctx, uint32_t i, fh_ctx** member)
{
  if (!ctx) return FH_E_INVALID;
  if (!member) return fail(ctx, FH_E_INVALID, "fh_ctx_member: null argument");
  *member = nullptr;
  if (i >= (ctx->group ? ctx->group->n : 1u)) return fail(ctx, FH_E_INVALID, "fh_ctx_member: index beyond the group");
  *member = ctx->group ? ctx->group->m[i] : ctx;
  return FH_OK;
}

int fh_group_set_gather_layers(fh_ctx* ctx, uint32_t mask)
{
  if (!ctx) return FH_E_INVALID;
  if (mask & ~FH_LAYER_ALL) return fail(ctx, FH_E_INVALID, "fh_group_set_gather_layers: unknown layer bits");
  if (ctx->group) ctx->group->mask = mask;
  return FH_OK;
}

int fh_group_gather_times(fh_ctx* ctx, double ms[3])
{
  if (!ctx) return FH_E_INVALID;
  if (!ms) return fail(ctx, FH_E_INVALID, "fh_group_gather_times: null argument");
  ms[0] = ms[1] = ms[2] = 0.0;
  if (!ctx->group) return FH_OK;
  fh_group* G = ctx->group;
  const int rc = fh_sync(ctx);
  if (rc) return rc;
  float t = 0.0f;
  for (uint32_t i = 1; i < G->n; ++i) {
    fh_group::Member& M = G->mem[i];
    if (!M.timed) continue;
    (void)hipSetDevice(G->m[i]->device);
    if (hipEventElapsedTime(&t, M.ev_pack_begin, M.ev_packed) == hipSuccess) ms[0] += t;
    (void)hipSetDevice(G->m[0]->device);
    (void)hipEventSynchronize(M.ev_copied);
    if (hipEventElapsedTime(&t, M.ev_copy_begin, M.ev_copied) == hipSuccess) ms[1] += t;
  }
  (void)hipSetDevice(G->m[0]->device);
  if (G->unpack_timed && hipEventElapsedTime(&t, G->ev_unpack_begin, G->ev_unpacked) == hipSuccess) ms[2] = t;
  (void)hipGetLastError();
  return FH_OK;
}

int fh_group_shard_layout(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t n, uint32_t mask, uint64_t* offsets)
{
  if (!offsets || n == 0 || n > kMaxShardsPerLaunch || width == 0 || height == 0 || tile_w == 0 || tile_h == 0 || width > 65535u || height > 65535u || (mask & ~FH_LAYER_ALL))
    return fail(nullptr, FH_E_INVALID, "fh_group_shard_layout: bad argument");
  const Slots s = layer_slots(mask);
  offsets[0] = 0; offsets[1] = 0;  // (the lead packs nothing: it renders into the caller's buffers)
  for (uint32_t i = 1; i < n; ++i) offsets[i + 1u] = offsets[i] + shard_bytes(s, owned_count(width, height, tile_w, tile_h, i, n));
  return FH_OK;
}

}  // extern "C"
