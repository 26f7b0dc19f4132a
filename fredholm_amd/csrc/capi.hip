// capi.hip -- implementation of the C ABI declared in include/fredholm_hip.h (context, environment,
// frame state, stats, device-memory helpers, tile pack/unpack; the scene upload is scene.hip).
// Mirrors the host duties of fredholm::Renderer (fredholm/include/fredholm/renderer.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>

#include "../../include/fredholm/image_io.h"
#include <hip/hip_gl_interop.h>

#include "context.h"
#include "fh_bsdf.h"
#include "fh_local_exposure.h"
#include "fh_meter.h"
#include "fh_trace.h"

// generated at build time from fredholm_amd/data/*.{u32,f32} by tools/gen_tables_inc.py
#include "gen/tables.inc"

namespace fh {

// errors of calls that have no context (fh_ctx_create, fh_image_load_rgba8) are kept per thread: a failing call on one thread
// (e.g. a texture loader thread) never reallocates a string another thread is reading through fh_last_error(NULL)
static thread_local std::string g_create_error;

int fail(fh_ctx* ctx, int code, const std::string& msg)
{
  g_create_error = msg;
  if (ctx) ctx->err = msg;
  if (ctx && ctx->owner) ctx->owner->err = "member " + std::to_string(ctx->member_index) + ": " + msg;
  return code;
}

namespace {

// the pixels of rank `rank` of `world` in the order the library packs them: tiles t with t % world == rank, row-major tile order; inside a tile 8 x 8 blocks, row-major,
// and row-major inside a block -- so the 64 lanes of a wave of k_generate (64 consecutive list entries) hold a compact 8 x 8 patch of the image instead of two rows of 32:
// their camera rays share more nodes and their first hits more faces (r6-4: closest-hit -2 %, configs[2] / [3] +0.9 %; 4 x 4 blocks measure the same).  FH_PIXEL_BLOCK=0:
// rows of the whole tile, as before round 6.  fredholm_amd/distributed.py: tile_ownership is the same list; tests/test_gpu_parity.py compares the two.
constexpr uint32_t kPixelBlock = 8;
static void owned_list(uint32_t width, uint32_t height, uint32_t tw, uint32_t th, uint32_t rank, uint32_t world, std::vector<uint32_t>& owned, std::vector<uint32_t>* owned_xy)
{
  static const uint32_t blk = [] { const char* e = getenv("FH_PIXEL_BLOCK"); const int v = e ? atoi(e) : (int)kPixelBlock; return (uint32_t)(v > 0 && v <= 64 ? v : 65536); }();
  const uint32_t tx = (width + tw - 1) / tw, ty = (height + th - 1) / th;
  for (uint32_t t = rank; t < tx * ty; t += world) {
    const uint32_t x0 = (t % tx) * tw, y0 = (t / tx) * th;
    for (uint32_t by = y0; by < y0 + th && by < height; by += (blk < th ? blk : th))
      for (uint32_t bx = x0; bx < x0 + tw && bx < width; bx += (blk < tw ? blk : tw))
        for (uint32_t y = by; y < by + blk && y < y0 + th && y < height; ++y)
          for (uint32_t x = bx; x < bx + blk && x < x0 + tw && x < width; ++x) { owned.push_back(x + width * y); if (owned_xy) owned_xy->push_back(x | (y << 16)); }
  }
}

// the ownership list of (rank, world) at the context's resolution and tile size, on the device; xy: its x | y << 16 form as well, for who wants it.
// *n: its length; *e: what failed (the buffers are then empty).  A context without a resolution has no list.
DeviceBuffer<uint32_t> upload_owned(const fh_ctx* ctx, uint32_t rank, uint32_t world, uint32_t* n, hipError_t* e, DeviceBuffer<uint32_t>* xy = nullptr)
{
  DeviceBuffer<uint32_t> list;
  *n = 0; *e = hipSuccess;
  if (ctx->width == 0 || ctx->height == 0) return list;
  std::vector<uint32_t> owned, owned_xy;
  owned_list(ctx->width, ctx->height, ctx->tile_w, ctx->tile_h, rank, world, owned, xy ? &owned_xy : nullptr);
  const size_t bytes = owned.size() * 4;
  if ((*e = list.alloc(owned.size())) == hipSuccess && bytes) *e = hipMemcpy(list, owned.data(), bytes, hipMemcpyHostToDevice);
  if (xy && *e == hipSuccess && (*e = xy->alloc(owned.size())) == hipSuccess && bytes) *e = hipMemcpy(*xy, owned_xy.data(), bytes, hipMemcpyHostToDevice);
  if (*e != hipSuccess) { list.reset(); if (xy) xy->reset(); return list; }
  *n = (uint32_t)owned.size();
  return list;
}

int rebuild_ownership(fh_ctx* ctx)
{
  ctx->d_owned.reset();
  ctx->d_owned_xy.reset();
  ctx->n_owned = 0;
  if (ctx->width > 65535u || ctx->height > 65535u) return fail(ctx, FH_E_UNSUPPORTED, "frames wider or higher than 65535 pixels are not supported");
  hipError_t e = hipSuccess;
  ctx->d_owned = upload_owned(ctx, ctx->shard_rank, ctx->shard_world, &ctx->n_owned, &e, std::addressof(ctx->d_owned_xy));
  FH_HIP(e);
  return FH_OK;
}

}  // namespace

// the ownership lists of all `world` ranks one after the other (fh_unpack_shards, and the gather of a group: group.hip)
int frame_map_ensure(fh_ctx* ctx, uint32_t world)
{
  // built once per (world, resolution, tile size) and kept, so a presented frame is ONE asynchronous launch
  fh_ctx::FrameMap& fm = ctx->frame_map;
  if (!(fm.d_all.get() && fm.world == world && fm.width == ctx->width && fm.height == ctx->height && fm.tile_w == ctx->tile_w && fm.tile_h == ctx->tile_h)) {
    (void)hipStreamSynchronize(ctx->stream);
    fm = fh_ctx::FrameMap{};
    std::vector<uint32_t> all;
    fm.start.assign(world + 1u, 0u);
    for (uint32_t r = 0; r < world; ++r) { owned_list(ctx->width, ctx->height, ctx->tile_w, ctx->tile_h, r, world, all, nullptr); fm.start[r + 1u] = (uint32_t)all.size(); }
    FH_HIP(fm.d_all.alloc(all.size()));
    if (!all.empty()) FH_HIP(hipMemcpy(fm.d_all, all.data(), all.size() * 4, hipMemcpyHostToDevice));
    fm.world = world; fm.width = ctx->width; fm.height = ctx->height; fm.tile_w = ctx->tile_w; fm.tile_h = ctx->tile_h;
  }
  return FH_OK;
}

uint32_t owned_count(uint32_t width, uint32_t height, uint32_t tw, uint32_t th, uint32_t rank, uint32_t world)
{
  std::vector<uint32_t> owned;
  owned_list(width, height, tw, th, rank, world, owned, nullptr);
  return (uint32_t)owned.size();
}

namespace {

__global__ void k_pack(const float* layer, const uint32_t* owned, uint32_t n, uint32_t fpp, float* packed)
{
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n * fpp; i += gridDim.x * blockDim.x) packed[i] = layer[(size_t)owned[i / fpp] * fpp + i % fpp];
}
__global__ void k_unpack(const float* packed, const uint32_t* owned, uint32_t n, uint32_t fpp, float* layer)
{
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n * fpp; i += gridDim.x * blockDim.x) layer[(size_t)owned[i / fpp] * fpp + i % fpp] = packed[i];
}
// every rank's shard in ONE launch (fh_unpack_shards): `all_owned` is the ownership lists of ranks 0 .. world - 1 one after the other (a permutation of the frame's pixels),
// start[r] where rank r's list begins in it, packed[r] that rank's packed shard
struct ShardSources { const float* packed[kMaxShardsPerLaunch]; uint32_t start[kMaxShardsPerLaunch + 1]; uint32_t world; };
__global__ void k_unpack_all(ShardSources src, const uint32_t* all_owned, uint32_t n, uint32_t fpp, float* layer)
{
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n * fpp; i += gridDim.x * blockDim.x) {
    const uint32_t j = i / fpp, c = i % fpp;
    uint32_t r = 0;
    while (r + 1u < src.world && j >= src.start[r + 1u]) ++r;
    layer[(size_t)all_owned[j] * fpp + c] = src.packed[r][(size_t)(j - src.start[r]) * fpp + c];
  }
}

}  // namespace
}  // namespace fh

using namespace fh;

namespace fh {
// render.hip: pool_ensure -- path record 64, radiance 16, identity 8, flags 4, first-hit AOVs 64, a 48-byte place per kind of secondary ray, the pending
// light ray 32 (emitters only); queues: two radiance + one spare + secondary + its sorted copy 5 x 4, two 16-bit keys, one entry per shading class; the escape
// mask of the secondary queue's entries 1 (k_sky_resolve)
uint64_t pool_bytes_per_path(const fh_ctx* ctx)
{
  const uint32_t sec = 2u + (ctx->has_dir ? 1u : 0u) + (ctx->n_lights > 0 ? 1u : 0u);
  const uint32_t classes = ctx->n_classes < 1u ? 1u : ctx->n_classes;
  return 64u + 16u + 8u + 4u + 64u + 48u * sec + (ctx->n_lights > 0 ? 32u : 0u) + 20u + 4u + 4u + 4u * classes + 1u;  // (... + queue keys and sorted queues 20, q_sec 4, q_prim 4, class queues, escape masks)
}
}  // namespace fh

extern "C" {

int fh_ctx_create(int device, fh_ctx** out)
{
  if (!out) return FH_E_INVALID;
  *out = nullptr;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { g_create_error = "no HIP device available: the fredholm HIP path has no CPU fallback"; return FH_E_HIP; }
  if (device < 0 || device >= n_dev) { g_create_error = "device index out of range"; return FH_E_INVALID; }
  if (hipSetDevice(device) != hipSuccess) { g_create_error = "hipSetDevice failed"; return FH_E_HIP; }
  fh_ctx* ctx = new fh_ctx;
  ctx->device = device;
  auto bail = [&](const char* what) { g_create_error = what; delete ctx; return FH_E_HIP; };  // (the context releases what it has made so far)
  if (ctx->stream.create(hipStreamNonBlocking) != hipSuccess) return bail("stream creation failed");
  if (ctx->d_sobol.alloc(kSobolMatricesBytes / sizeof(uint32_t)) != hipSuccess) return bail("device allocation failed");
  if (ctx->d_lut_refl.alloc(kLutReflectionBytes / sizeof(float)) != hipSuccess) return bail("device allocation failed");
  if (ctx->d_lut_sheen.alloc(kLutSheenBytes / sizeof(float)) != hipSuccess) return bail("device allocation failed");
  if (ctx->d_trace_counters.alloc(32) != hipSuccess) return bail("device allocation failed");
  if (ctx->d_hosek.alloc(1) != hipSuccess || hipMemsetAsync(ctx->d_hosek, 0, sizeof(fh::HosekSky), ctx->stream) != hipSuccess) return bail("device allocation failed");
  if (hipMemcpy(ctx->d_sobol, kSobolMatrices, kSobolMatricesBytes, hipMemcpyHostToDevice) != hipSuccess) return bail("table upload failed");
  {
    // byte-indexed form of the generator matrices: entry [dim][k][b] = XOR of the columns 8k + j selected by the bits j of b, so that the XOR over the 32 index
    // bits (sobol.cu:10716-10727) becomes four table reads (fh_sampler.h: sobol_row_bytes); the integrator kernels stage the tables of their dimensions in LDS
    std::vector<uint32_t> bytes((size_t)1024 * 4 * 256);
    const uint32_t* mat = kSobolMatrices;
    for (uint32_t dim = 0; dim < 1024u; ++dim)
      for (uint32_t k = 0; k < 4u; ++k) {
        uint32_t* t = &bytes[((size_t)dim * 4 + k) * 256];
        t[0] = 0u;
        for (uint32_t b = 1; b < 256u; ++b) t[b] = t[b & (b - 1u)] ^ mat[dim * 52u + 8u * k + (uint32_t)__builtin_ctz(b)];
      }
    if (ctx->d_sobol_bytes.alloc(bytes.size()) != hipSuccess) return bail("device allocation failed");
    if (hipMemcpy(ctx->d_sobol_bytes, bytes.data(), bytes.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) return bail("table upload failed");
  }
  if (hipMemcpy(ctx->d_lut_refl, kLutReflection, kLutReflectionBytes, hipMemcpyHostToDevice) != hipSuccess) return bail("table upload failed");
  if (hipMemcpy(ctx->d_lut_sheen, kLutSheen, kLutSheenBytes, hipMemcpyHostToDevice) != hipSuccess) return bail("table upload failed");
  (void)hipMemsetAsync(ctx->d_trace_counters, 0, 32 * sizeof(unsigned long long), ctx->stream);  // (never hipMemset: it is asynchronous and ordered with nothing on a non-blocking stream)
  for (int k = 0; k < fh::kPassSlots - 1; ++k)
    if (ctx->aux_stream[k].create(hipStreamNonBlocking) != hipSuccess) return bail("stream creation failed");
  for (fh_ctx::PassSlot& s : ctx->slot) {
    if (s.snapshot.h.alloc((size_t)fh::kCounterStride * 66) != hipSuccess) return bail("pinned allocation failed");
    if (s.snapshot.ev.create() != hipSuccess || s.ev_gen.create(hipEventDisableTiming) != hipSuccess || s.ev_acc.create(hipEventDisableTiming) != hipSuccess) return bail("event creation failed");
  }
  if (ctx->ev_enter.create(hipEventDisableTiming) != hipSuccess) return bail("event creation failed");
  if (const char* e = getenv("FH_PIPELINE")) ctx->n_slots = e[0] == '0' ? 1 : (e[0] == '2' ? 2 : 3);
  {
    fh_ctx::Tunables& t = ctx->tun;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) t.n_cus = (uint32_t)prop.multiProcessorCount;
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, device) == hipSuccess && v >= 64 * 1024) t.lds_per_cu = (uint32_t)v;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeSharedMemPerBlockOptin, device) == hipSuccess && v >= 64 * 1024) t.lds_per_block = (uint32_t)v;
    if (t.lds_per_block > t.lds_per_cu) t.lds_per_block = t.lds_per_cu;
    auto env_uint = [](const char* name, int lo, int hi, uint32_t& dst) { if (const char* e = getenv(name)) { const int v = atoi(e); if (v >= lo && v <= hi) dst = (uint32_t)v; } };
    auto env_off = [](const char* name, bool& dst) { if (const char* e = getenv(name)) dst = e[0] != '0'; };
    env_uint("FH_COOP_T", 1, 64, t.coop_flush);
    t.coop_flush_fixed = getenv("FH_COOP_T") != nullptr;
    env_off("FH_COOP", t.coop);
    env_off("FH_STREAM", t.stream);
    t.stream_forced = t.stream && getenv("FH_STREAM") != nullptr;
    env_uint("FH_STREAM_REFILL", 1, 64, t.stream_refill);
    env_uint("FH_STREAM_MIN_RAYS", 0, 65535, t.stream_min_rays);
    env_off("FH_SORT_SMALL", t.sort_small);
    env_off("FH_OVERLAP", t.overlap_secondary);
    env_off("FH_MERGE", t.merge_trace);
    env_uint("FH_SKY_BLOCKS", 0, 64, t.sky_blocks_per_cu);
    env_uint("FH_SKY_FILLER_GRID", 0, 65535, t.sky_filler_grid);
    if (const char* e = getenv("FH_POISON")) t.poison_pools = e[0] == '1';
    env_off("FH_SKY_SPLIT", t.sky_split);
    env_uint("FH_SKY_SPLIT_MIN_LOG2", 0, 40, t.sky_split_min_log2);
    env_uint("FH_STACK_LDS", 1, 99, t.stack_lds_entries);
    env_uint("FH_SHADE_WGS", 2, 3, t.shade_wgs);
    env_uint("FH_STREAM_CHUNK", 16, 65535, t.stream_chunk);
    t.stream_chunk_fixed = getenv("FH_STREAM_CHUNK") != nullptr;
    if (t.stream_chunk_fixed) t.stream_chunk_closest = t.stream_chunk;  // (FH_STREAM_CHUNK alone sets both launches)
    env_uint("FH_STREAM_CHUNK_CLOSEST", 16, 65535, t.stream_chunk_closest);
    env_uint("FH_TAIL_DEPTH", 0, 64, t.tail_depth);
    env_uint("FH_TAIL_PATHS", 64, 1 << 30, t.tail_paths);
    env_off("FH_SORT", t.sort_queues);
    env_uint("FH_SORT_ONEPASS", 0, 2, t.sort_onepass);
    env_uint("FH_BOTTOM_UP", 0, 2, t.bottom_up);
    env_uint("FH_SKY_DEFER", 0, 1, t.sky_defer);
    env_uint("FH_DARK_SKY", 0, 1, t.dark_sky);
    t.debug_tail = getenv("FH_DEBUG_TAIL") != nullptr;
    if (const char* e = getenv("FH_FORCE_ALPHA")) t.force_alpha = e[0] == '1';
  }
  {  // the sky-pixel kernel's stream has the lowest priority: the workgroups of its filler launch -- pure arithmetic, 80 registers -- take what the passes leave instead of the
     // wave slots the traversal launches want (FH_SKY_PRIO=0: default priority; profiles/README.md r4-13)
    int least = 0, greatest = 0;
    const char* e = getenv("FH_SKY_PRIO");
    const bool low = !(e && e[0] == '0') && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess;
    if (ctx->sky_stream.create(hipStreamNonBlocking, low ? least : 0) != hipSuccess) return bail("stream creation failed");
  }
  if (ctx->ev_sky.create(hipEventDisableTiming) != hipSuccess || ctx->ev_sky_cursor.create(hipEventDisableTiming) != hipSuccess) return bail("event creation failed");
  if (ctx->d_split_counters.alloc(5) != hipSuccess) return bail("device allocation failed");
  (void)hipMemsetAsync(ctx->d_split_counters, 0, 20, ctx->stream);
  if (ctx->ev_render_begin.create() != hipSuccess || ctx->ev_render_end.create() != hipSuccess) return bail("event creation failed");
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return bail("hipStreamSynchronize failed");  // the fills above are done before any upload (synchronous copies, ordered with no stream) touches what they cleared
  *out = ctx;
  return FH_OK;
}

int fh_ctx_destroy(fh_ctx* ctx)
{
  FH_GROUP(ctx, group_destroy(ctx));
  if (!ctx) return FH_E_INVALID;
  (void)hipSetDevice(ctx->device);
  (void)drain_passes(ctx, true);
  delete ctx;  // (the members release themselves, the streams last: context.h)
  return FH_OK;
}

const char* fh_last_error(fh_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int fh_set_flags(fh_ctx* ctx, uint32_t flags)
{
  FH_GROUP_EACH(ctx, kGroupCallPlain, fh_set_flags(m_, flags));
  CTX_CHECK(ctx);
  ctx->flags = flags;
  return FH_OK;
}
int fh_get_flags(fh_ctx* ctx, uint32_t* flags)
{
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  if (!flags) return fail(ctx, FH_E_INVALID, "fh_get_flags: null argument");
  *flags = ctx->flags;
  return FH_OK;
}

int fh_set_path_pool(fh_ctx* ctx, uint32_t target)
{
  FH_GROUP_EACH(ctx, kGroupCallFrame, fh_set_path_pool(m_, target));
  CTX_CHECK(ctx);
  if (target == 0) return fail(ctx, FH_E_INVALID, "fh_set_path_pool: zero");
  (void)hipStreamSynchronize(ctx->stream);
  pool_release(ctx);
  ctx->pool_target = target;
  ctx->pool_target_by_caller = true;
  return FH_OK;
}

int fh_path_pool_bytes(fh_ctx* ctx, uint64_t* bytes_per_path, uint32_t* pools)
{
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  if (!bytes_per_path || !pools) return fail(ctx, FH_E_INVALID, "fh_path_pool_bytes: null argument");
  *bytes_per_path = pool_bytes_per_path(ctx);
  *pools = (uint32_t)ctx->n_slots;
  return FH_OK;
}

int fh_kat_face_classes(fh_ctx* ctx, uint8_t* out, uint32_t n)
{
  FH_GROUP_REFUSE(ctx, "fh_kat_face_classes");
  CTX_CHECK(ctx);
  if (!out || n != ctx->n_faces) return fail(ctx, FH_E_INVALID, "fh_kat_face_classes: one byte per face of the uploaded scene");
  if (n) FH_HIP(hipMemcpy(out, ctx->d_face_cls, n, hipMemcpyDeviceToHost));
  return FH_OK;
}

int fh_alpha_face_counts(fh_ctx* ctx, uint32_t counts[4])
{
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  if (!counts) return fail(ctx, FH_E_INVALID, "fh_alpha_face_counts: null argument");
  for (int k = 0; k < 4; ++k) counts[k] = ctx->alpha_face_counts[k];
  return FH_OK;
}

int fh_alpha_cell_counts(fh_ctx* ctx, uint64_t counts[3])
{
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  if (!counts) return fail(ctx, FH_E_INVALID, "fh_alpha_cell_counts: null argument");
  for (int k = 0; k < 3; ++k) counts[k] = ctx->alpha_cell_counts[k];
  return FH_OK;
}

int fh_kat_alpha_records(fh_ctx* ctx, uint32_t* out, uint32_t n_faces)
{
  FH_GROUP_REFUSE(ctx, "fh_kat_alpha_records");
  CTX_CHECK(ctx);
  if (!out || n_faces != ctx->n_faces) return fail(ctx, FH_E_INVALID, "fh_kat_alpha_records: 32 words per face of the uploaded scene");
  if (!ctx->d_alpha_rec) { std::memset(out, 0, 128ull * n_faces); return FH_OK; }
  FH_HIP(hipMemcpy(out, ctx->d_alpha_rec, 128ull * n_faces, hipMemcpyDeviceToHost));
  return FH_OK;
}

int fh_path_pool_allocated(fh_ctx* ctx, uint64_t* bytes, uint64_t* paths)
{
  FH_GROUP(ctx, group_path_pool_allocated(ctx, bytes, paths));
  CTX_CHECK(ctx);
  if (!bytes || !paths) return fail(ctx, FH_E_INVALID, "fh_path_pool_allocated: null argument");
  *bytes = 0; *paths = 0;
  for (const fh_ctx::PassSlot& s : ctx->slot) { *bytes += s.alloc_bytes; *paths += s.pool.capacity; }
  return FH_OK;
}

int fh_set_tail_depth(fh_ctx* ctx, uint32_t depth)
{
  FH_GROUP_EACH(ctx, kGroupCallPlain, fh_set_tail_depth(m_, depth));
  CTX_CHECK(ctx);
  ctx->tail_depth = depth;  // 0 = adaptive; bounce 0 always runs as wavefront kernels (it writes the first-hit AOVs)
  return FH_OK;
}

int fh_bvh_build(fh_ctx* ctx)
{
  FH_GROUP_EACH(ctx, kGroupCallScene, fh_bvh_build(m_));
  CTX_CHECK(ctx);
  if (!ctx->scene_loaded) return fail(ctx, FH_E_INVALID, "fh_bvh_build: no scene");
  if (ctx->bvh_valid) return FH_OK;  // geometry unchanged since the last build
  return bvh_build_device(ctx);
}

int fh_scene_n_lights(fh_ctx* ctx, uint32_t* out)
{
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  if (!out) return FH_E_INVALID;
  *out = ctx->n_lights;
  return FH_OK;
}

int fh_set_directional_light(fh_ctx* ctx, const float* le, const float* dir, float angle)
{
  FH_GROUP_EACH(ctx, kGroupCallScene, fh_set_directional_light(m_, le, dir, angle));
  CTX_CHECK(ctx);
  if (!le || !dir) return FH_E_INVALID;
  const f3 d = normalize(mk3(dir[0], dir[1], dir[2]));  // renderer.h:560
  ctx->has_dir = true;
  for (int k = 0; k < 3; ++k) ctx->dir_le[k] = le[k];
  ctx->dir_dir[0] = d.x; ctx->dir_dir[1] = d.y; ctx->dir_dir[2] = d.z;
  ctx->sun_dir[0] = d.x; ctx->sun_dir[1] = d.y; ctx->sun_dir[2] = d.z;  // renderer.h:563
  ctx->dir_angle = angle;
  return FH_OK;
}
int fh_clear_directional_light(fh_ctx* ctx)
{
  FH_GROUP_EACH(ctx, kGroupCallScene, fh_clear_directional_light(m_));
  CTX_CHECK(ctx);
  ctx->has_dir = false;
  return FH_OK;
}
int fh_set_sky_intensity(fh_ctx* ctx, float v)
{
  FH_GROUP_EACH(ctx, kGroupCallScene, fh_set_sky_intensity(m_, v));
  CTX_CHECK(ctx);
  ctx->sky_intensity = v;
  return FH_OK;
}
int fh_load_arhosek_sky(fh_ctx* ctx, float turbidity, float albedo)
{
  FH_GROUP_EACH(ctx, kGroupCallScene, fh_load_arhosek_sky(m_, turbidity, albedo));
  CTX_CHECK(ctx);
  if (!(turbidity >= 1.0f && turbidity <= 10.0f)) return fail(ctx, FH_E_INVALID, "turbidity must be in [1,10]");
  const float elevation = (float)(0.5f * 3.14159265358979323846 - fhe_acos(clampf(ctx->sun_dir[1], -1.0f, 1.0f)));  // renderer.h:592-601
  ctx->hosek = hosek_cook(kHosekRgb, turbidity, albedo, elevation);
  ctx->has_hosek = true;
  FH_HIP(hipMemcpyAsync(ctx->d_hosek, &ctx->hosek, sizeof ctx->hosek, hipMemcpyHostToDevice, ctx->stream));  // (ordered after the frames already submitted)
  FH_HIP(hipStreamSynchronize(ctx->stream));
  ctx->env_stale = true;
  return FH_OK;
}
int fh_clear_arhosek_sky(fh_ctx* ctx)
{
  FH_GROUP_EACH(ctx, kGroupCallScene, fh_clear_arhosek_sky(m_));
  CTX_CHECK(ctx);
  ctx->has_hosek = false;
  ctx->env_stale = true;
  return FH_OK;
}
int fh_load_ibl(fh_ctx* ctx, const float* rgba, uint32_t w, uint32_t h)
{
  FH_GROUP_EACH(ctx, kGroupCallScene, fh_load_ibl(m_, rgba, w, h));
  CTX_CHECK(ctx);
  if (!rgba || w == 0 || h == 0) return fail(ctx, FH_E_INVALID, "fh_load_ibl: empty image");
  (void)hipStreamSynchronize(ctx->stream);
  ctx->env_stale = true;
  FH_HIP(ctx->d_ibl.alloc(4ull * w * h));
  FH_HIP(hipMemcpy(ctx->d_ibl, rgba, sizeof(float) * 4ull * w * h, hipMemcpyHostToDevice));
  ctx->ibl_w = w;
  ctx->ibl_h = h;
  return FH_OK;
}
int fh_clear_ibl(fh_ctx* ctx)
{
  FH_GROUP_EACH(ctx, kGroupCallScene, fh_clear_ibl(m_));
  CTX_CHECK(ctx);
  (void)hipStreamSynchronize(ctx->stream);
  ctx->d_ibl.reset();
  ctx->env_stale = true;
  return FH_OK;
}

// importance sampling of the environment (envmap.hip, fh_envmap.h).  The refusal is decided before the context is looked at; a scene call, so every member of a group gets it
int fh_set_env_sampling(fh_ctx* ctx, const fh_env_sampling_params* params)
{
  if (const char* why = env_sampling_refusal(params)) return fail(ctx, FH_E_INVALID, std::string("fh_set_env_sampling: ") + why);
  FH_GROUP_EACH(ctx, kGroupCallScene, fh_set_env_sampling(m_, params));
  CTX_CHECK(ctx);
  return env_sampling_set(ctx, params);
}
int fh_get_env_sampling(fh_ctx* ctx, int* on, fh_env_sampling_params* params)
{
  FH_GROUP_LEAD(ctx);
  if (!ctx || !on) return FH_E_INVALID;
  *on = ctx->env_sampling;
  if (params) params->cosine_fraction = ctx->env_cosine_fraction;
  return FH_OK;
}

// sampling of area lights by power (lights.hip, fh_lights.h): refused from the arguments alone; a scene call
int fh_set_light_sampling(fh_ctx* ctx, const fh_light_sampling_params* params)
{
  if (const char* why = light_sampling_refusal(params)) return fail(ctx, FH_E_INVALID, std::string("fh_set_light_sampling: ") + why);
  FH_GROUP_EACH(ctx, kGroupCallScene, fh_set_light_sampling(m_, params));
  CTX_CHECK(ctx);
  return light_sampling_set(ctx, params);
}
int fh_get_light_sampling(fh_ctx* ctx, int* on, fh_light_sampling_params* params)
{
  FH_GROUP_LEAD(ctx);
  if (!ctx || !on) return FH_E_INVALID;
  *on = ctx->light_sampling;
  if (params) params->uniform_fraction = ctx->light_uniform_fraction;
  return FH_OK;
}
// resampling of the table's picks (fh_lights.h): refused from the arguments alone; a scene call.  Nothing is rebuilt and nothing waited for: the proxies exist whenever
// the table does, and M reaches the kernels by value
int fh_set_light_resampling(fh_ctx* ctx, const fh_light_resampling_params* params)
{
  if (const char* why = light_resampling_refusal(params)) return fail(ctx, FH_E_INVALID, std::string("fh_set_light_resampling: ") + why);
  FH_GROUP_EACH(ctx, kGroupCallScene, fh_set_light_resampling(m_, params));
  CTX_CHECK(ctx);
  ctx->light_resampling = params ? 1 : 0;
  if (params) ctx->light_candidates = params->candidates;
  return FH_OK;
}
int fh_get_light_resampling(fh_ctx* ctx, int* on, fh_light_resampling_params* params)
{
  FH_GROUP_LEAD(ctx);
  if (!ctx || !on) return FH_E_INVALID;
  *on = ctx->light_resampling;
  if (params) params->candidates = ctx->light_candidates;
  return FH_OK;
}

// the moments of adaptive sampling start at sample 0: allocated and cleared whenever the mode is on and the counters are reset (0 * inf would poison a reset's
// running means otherwise), and when the mode is turned on
static int adaptive_reset(fh_ctx* ctx)
{
  ctx->adapt_total = 0;
  if (!ctx->adaptive) return FH_OK;
  const size_t px = (size_t)ctx->width * ctx->height;
  if (!ctx->d_moments) FH_HIP(ctx->d_moments.alloc(px));
  if (!ctx->d_sky_taken) {
    FH_HIP(ctx->d_sky_taken.alloc(1));
    FH_HIP(hipMemsetAsync(ctx->d_sky_taken, 0, sizeof(unsigned long long), ctx->stream));
  }
  FH_HIP(hipMemsetAsync(ctx->d_moments, 0, 8ull * px, ctx->stream));
  return adaptive_upload(ctx);
}

int fh_init_render_states(fh_ctx* ctx)
{
  FH_GROUP(ctx, group_init_render_states(ctx));
  CTX_CHECK(ctx);
  if (!ctx->d_sample_count) return fail(ctx, FH_E_INVALID, "resolution not set");
  FH_HIP(hipMemsetAsync(ctx->d_sample_count, 0, 4ull * ctx->width * ctx->height, ctx->stream));
  FH_HIP(hipMemsetAsync(ctx->d_sample_issued, 0, 4ull * ctx->width * ctx->height, ctx->stream));
  ctx->accumulated = false;
  return adaptive_reset(ctx);
}

int fh_set_adaptive_sampling(fh_ctx* ctx, const fh_adaptive_params* p)
{
  FH_GROUP_EACH(ctx, kGroupCallFrame, fh_set_adaptive_sampling(m_, p));
  CTX_CHECK(ctx);
  if (!p) { ctx->adaptive = false; return FH_OK; }
  if (!(p->threshold >= 0.0f) || !std::isfinite(p->threshold)) return fail(ctx, FH_E_INVALID, "fh_set_adaptive_sampling: threshold must be finite and >= 0");
  if (!(p->floor > 0.0f) || !std::isfinite(p->floor)) return fail(ctx, FH_E_INVALID, "fh_set_adaptive_sampling: floor must be finite and > 0");
  if (p->min_samples < 2u) return fail(ctx, FH_E_INVALID, "fh_set_adaptive_sampling: min_samples must be >= 2");
  if (p->step < 1u) return fail(ctx, FH_E_INVALID, "fh_set_adaptive_sampling: step must be >= 1");
  if (ctx->adaptive && std::memcmp(&ctx->adapt, p, sizeof *p) == 0) return FH_OK;
  if (ctx->accumulated) return fail(ctx, FH_E_INVALID, "fh_set_adaptive_sampling: samples were accumulated since fh_init_render_states / fh_set_resolution (the moments must start at sample 0)");
  if (!ctx->d_sample_count) return fail(ctx, FH_E_INVALID, "fh_set_adaptive_sampling: resolution not set");
  ctx->adapt = *p;
  ctx->adaptive = true;
  return adaptive_reset(ctx);
}

int fh_get_adaptive_sampling(fh_ctx* ctx, int* enabled, fh_adaptive_params* p)
{
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  if (enabled) *enabled = ctx->adaptive ? 1 : 0;
  if (p) *p = ctx->adapt;
  return FH_OK;
}

int fh_set_adaptive_policy(fh_ctx* ctx, uint32_t block, uint32_t growth)
{
  FH_GROUP_EACH(ctx, kGroupCallFrame, fh_set_adaptive_policy(m_, block, growth));
  CTX_CHECK(ctx);
  if (block != 1u && block != 2u && block != 4u && block != 8u) return fail(ctx, FH_E_INVALID, "fh_set_adaptive_policy: block must be 1, 2, 4 or 8");
  if (growth != 1u && growth != 2u) return fail(ctx, FH_E_INVALID, "fh_set_adaptive_policy: growth must be 1 or 2");
  if (block == ctx->adapt_block && growth == ctx->adapt_growth) return FH_OK;
  if (ctx->accumulated) return fail(ctx, FH_E_INVALID, "fh_set_adaptive_policy: samples were accumulated since fh_init_render_states / fh_set_resolution (every stop so far followed the old policy)");
  if (ctx->tile_w % block != 0u || ctx->tile_h % block != 0u) return fail(ctx, FH_E_INVALID, "fh_set_adaptive_policy: tile width and height must be multiples of block (a guard block has one owner)");
  ctx->adapt_block = block;
  ctx->adapt_growth = growth;
  return ctx->adaptive ? adaptive_upload(ctx) : FH_OK;  // (the device copy of the parameters, the marks of the guard blocks)
}

int fh_get_adaptive_policy(fh_ctx* ctx, uint32_t* block, uint32_t* growth)
{
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  if (block) *block = ctx->adapt_block;
  if (growth) *growth = ctx->adapt_growth;
  return FH_OK;
}

int fh_adaptive_next_boundary(fh_ctx* ctx, uint32_t* samples)
{
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  if (!samples) return fail(ctx, FH_E_INVALID, "fh_adaptive_next_boundary: null argument");
  if (!ctx->adaptive) return fail(ctx, FH_E_INVALID, "fh_adaptive_next_boundary: adaptive sampling is off");
  *samples = adaptive_to_boundary(ctx);
  return FH_OK;
}

int fh_get_sample_counts(fh_ctx* ctx, uint32_t* counts)
{
  FH_GROUP(ctx, group_get_sample_counts(ctx, counts));
  CTX_CHECK(ctx);
  if (!counts) return fail(ctx, FH_E_INVALID, "fh_get_sample_counts: null argument");
  if (!ctx->d_sample_count) return fail(ctx, FH_E_INVALID, "fh_get_sample_counts: resolution not set");
  FH_HIP(hipMemcpyAsync(counts, ctx->d_sample_count, 4ull * ctx->width * ctx->height, hipMemcpyDeviceToDevice, ctx->stream));
  return FH_OK;
}

int fh_get_luminance_moments(fh_ctx* ctx, float* m)
{
  FH_GROUP(ctx, group_get_luminance_moments(ctx, m));
  CTX_CHECK(ctx);
  if (!m) return fail(ctx, FH_E_INVALID, "fh_get_luminance_moments: null argument");
  if (!ctx->adaptive || !ctx->d_moments) return fail(ctx, FH_E_INVALID, "fh_get_luminance_moments: adaptive sampling is off");
  FH_HIP(hipMemcpyAsync(m, ctx->d_moments, 8ull * ctx->width * ctx->height, hipMemcpyDeviceToDevice, ctx->stream));
  return FH_OK;
}

int fh_active_pixel_count(fh_ctx* ctx, uint32_t* out)
{
  FH_GROUP(ctx, group_active_pixel_count(ctx, out));
  CTX_CHECK(ctx);
  if (!out) return fail(ctx, FH_E_INVALID, "fh_active_pixel_count: null argument");
  if (!ctx->d_sample_count) return fail(ctx, FH_E_INVALID, "fh_active_pixel_count: resolution not set");
  if (!ctx->adaptive) { *out = ctx->n_owned; return FH_OK; }
  return adaptive_select(ctx, ctx->stream, ctx->d_owned, ctx->d_owned_xy, ctx->n_owned, out);
}

// known-answer hooks of the sample-index tests: both per-pixel counters at once, after everything queued on the context has finished (the passes of a call in flight
// read and write them)
int fh_kat_set_sample_counts(fh_ctx* ctx, const uint32_t* counts, uint32_t n_pixels)
{
  FH_GROUP_REFUSE(ctx, "fh_kat_set_sample_counts");
  CTX_CHECK(ctx);
  if (!ctx->d_sample_count) return fail(ctx, FH_E_INVALID, "fh_kat_set_sample_counts: resolution not set");
  if (!counts || (uint64_t)n_pixels != (uint64_t)ctx->width * ctx->height) return fail(ctx, FH_E_INVALID, "fh_kat_set_sample_counts: one count per pixel of the frame");
  const int rc = fh_sync(ctx);
  if (rc) return rc;
  FH_HIP(hipMemcpy(ctx->d_sample_count, counts, 4ull * n_pixels, hipMemcpyHostToDevice));
  FH_HIP(hipMemcpy(ctx->d_sample_issued, counts, 4ull * n_pixels, hipMemcpyHostToDevice));
  return FH_OK;
}

int fh_kat_set_issued(fh_ctx* ctx, const uint32_t* issued, uint32_t n_pixels)
{
  FH_GROUP_REFUSE(ctx, "fh_kat_set_issued");
  CTX_CHECK(ctx);
  if (!ctx->d_sample_issued) return fail(ctx, FH_E_INVALID, "fh_kat_set_issued: resolution not set");
  if (!issued || (uint64_t)n_pixels != (uint64_t)ctx->width * ctx->height) return fail(ctx, FH_E_INVALID, "fh_kat_set_issued: one count per pixel of the frame");
  const int rc = fh_sync(ctx);
  if (rc) return rc;
  FH_HIP(hipMemcpy(ctx->d_sample_issued, issued, 4ull * n_pixels, hipMemcpyHostToDevice));
  return FH_OK;
}

int fh_kat_sample_counts(fh_ctx* ctx, uint32_t* sample_count, uint32_t* issued, uint32_t n_pixels)
{
  FH_GROUP_REFUSE(ctx, "fh_kat_sample_counts");
  CTX_CHECK(ctx);
  if (!ctx->d_sample_count) return fail(ctx, FH_E_INVALID, "fh_kat_sample_counts: resolution not set");
  if ((uint64_t)n_pixels != (uint64_t)ctx->width * ctx->height) return fail(ctx, FH_E_INVALID, "fh_kat_sample_counts: one count per pixel of the frame");
  const int rc = fh_sync(ctx);
  if (rc) return rc;
  if (sample_count) FH_HIP(hipMemcpy(sample_count, ctx->d_sample_count, 4ull * n_pixels, hipMemcpyDeviceToHost));
  if (issued) FH_HIP(hipMemcpy(issued, ctx->d_sample_issued, 4ull * n_pixels, hipMemcpyDeviceToHost));
  return FH_OK;
}

int fh_set_resolution(fh_ctx* ctx, uint32_t w, uint32_t h)
{
  FH_GROUP(ctx, group_set_resolution(ctx, w, h));
  CTX_CHECK(ctx);
  if (w == 0 || h == 0) return fail(ctx, FH_E_INVALID, "zero resolution");
  if (w > 65535u || h > 65535u) return fail(ctx, FH_E_UNSUPPORTED, "frames wider or higher than 65535 pixels are not supported");  // (before anything is changed: the context keeps its resolution)
  (void)hipStreamSynchronize(ctx->stream);
  ctx->d_sample_count.reset();
  ctx->d_sample_issued.reset();
  ctx->d_moments.reset();  // (fh_init_render_states below makes it again at the new size if the mode is on)
  ctx->width = w; ctx->height = h;
  FH_HIP(ctx->d_sample_count.alloc((size_t)w * h));
  FH_HIP(ctx->d_sample_issued.alloc((size_t)w * h));
  const int rc = rebuild_ownership(ctx);
  if (rc) return rc;
  return fh_init_render_states(ctx);
}

int fh_set_tile_shard(fh_ctx* ctx, uint32_t rank, uint32_t world, uint32_t tw, uint32_t th)
{
  FH_GROUP(ctx, group_set_tile_shard(ctx, rank, world, tw, th));
  CTX_CHECK(ctx);
  if (world == 0 || rank >= world || tw == 0 || th == 0) return fail(ctx, FH_E_INVALID, "bad shard");
  if (tw % ctx->adapt_block != 0u || th % ctx->adapt_block != 0u) return fail(ctx, FH_E_INVALID, "fh_set_tile_shard: tile width and height must be multiples of the adaptive policy's block (a guard block has one owner)");
  (void)hipStreamSynchronize(ctx->stream);
  ctx->shard_rank = rank; ctx->shard_world = world; ctx->tile_w = tw; ctx->tile_h = th;
  return rebuild_ownership(ctx);
}

int fh_owned_pixel_count(fh_ctx* ctx, uint32_t* out)
{
  FH_GROUP(ctx, group_owned_pixel_count(ctx, out));
  CTX_CHECK(ctx);
  if (!out) return FH_E_INVALID;
  *out = ctx->n_owned;
  return FH_OK;
}

int fh_pack_owned(fh_ctx* ctx, const float* layer, uint32_t fpp, float* packed)
{
  FH_GROUP_REFUSE(ctx, "fh_pack_owned");
  CTX_CHECK(ctx);
  if (!layer || !packed || fpp == 0) return FH_E_INVALID;
  if (ctx->n_owned) hipLaunchKernelGGL(k_pack, dim3((ctx->n_owned * fpp + 255) / 256), dim3(256), 0, ctx->stream, layer, ctx->d_owned, ctx->n_owned, fpp, packed);
  FH_HIP(hipGetLastError());
  return FH_OK;
}

int fh_unpack_shard(fh_ctx* ctx, uint32_t rank, uint32_t world, const float* packed, uint32_t fpp, float* layer)
{
  FH_GROUP_REFUSE(ctx, "fh_unpack_shard");
  CTX_CHECK(ctx);
  if (!layer || !packed || fpp == 0 || world == 0 || rank >= world) return FH_E_INVALID;
  if (ctx->width > 65535u || ctx->height > 65535u) return fail(ctx, FH_E_UNSUPPORTED, "frames wider or higher than 65535 pixels are not supported");
  // ownership list of (rank, world) with this context's tile size and resolution: built once and kept (a presented frame unpacks every rank's shard), so that the call
  // is one asynchronous launch on the context stream -- no allocation, no host copy, no synchronisation per frame
  fh_ctx::ShardList* sl = nullptr;
  for (fh_ctx::ShardList& c : ctx->shard_lists)
    if (c.rank == rank && c.world == world && c.width == ctx->width && c.height == ctx->height && c.tile_w == ctx->tile_w && c.tile_h == ctx->tile_h) sl = &c;
  if (!sl) {
    uint32_t n = 0;
    hipError_t e = hipSuccess;
    DeviceBuffer<uint32_t> list = upload_owned(ctx, rank, world, &n, &e);
    FH_HIP(e);
    if (ctx->shard_lists.size() >= 64u) {  // (a caller cycling through many splits: drop the oldest)
      (void)hipStreamSynchronize(ctx->stream);
      ctx->shard_lists.erase(ctx->shard_lists.begin());
    }
    ctx->shard_lists.push_back(fh_ctx::ShardList{rank, world, ctx->width, ctx->height, ctx->tile_w, ctx->tile_h, std::move(list), n});
    sl = &ctx->shard_lists.back();
  }
  if (sl->n_owned) hipLaunchKernelGGL(k_unpack, dim3((sl->n_owned * fpp + 255) / 256), dim3(256), 0, ctx->stream, packed, sl->d_owned, sl->n_owned, fpp, layer);
  FH_HIP(hipGetLastError());
  return FH_OK;
}

int fh_unpack_shards(fh_ctx* ctx, uint32_t world, const float* const* packed, uint32_t fpp, float* layer)
{
  FH_GROUP_REFUSE(ctx, "fh_unpack_shards");
  CTX_CHECK(ctx);
  if (!layer || !packed || fpp == 0 || world == 0) return FH_E_INVALID;
  for (uint32_t r = 0; r < world; ++r)
    if (!packed[r]) return fail(ctx, FH_E_INVALID, "fh_unpack_shards: null shard pointer");
  if (world > kMaxShardsPerLaunch) {  // (more ranks than one launch's argument block holds: one launch per rank)
    for (uint32_t r = 0; r < world; ++r) { const int rc = fh_unpack_shard(ctx, r, world, packed[r], fpp, layer); if (rc) return rc; }
    return FH_OK;
  }
  if (ctx->width > 65535u || ctx->height > 65535u) return fail(ctx, FH_E_UNSUPPORTED, "frames wider or higher than 65535 pixels are not supported");
  const int rc_map = frame_map_ensure(ctx, world);
  if (rc_map) return rc_map;
  fh_ctx::FrameMap& fm = ctx->frame_map;
  ShardSources src{};
  src.world = world;
  for (uint32_t r = 0; r < world; ++r) { src.packed[r] = packed[r]; src.start[r] = fm.start[r]; }
  src.start[world] = fm.start[world];
  const uint32_t n = fm.start[world];
  if (n) hipLaunchKernelGGL(k_unpack_all, dim3((uint32_t)(((size_t)n * fpp + 255) / 256)), dim3(256), 0, ctx->stream, src, fm.d_all, n, fpp, layer);
  FH_HIP(hipGetLastError());
  return FH_OK;
}

int fh_render(fh_ctx* ctx, const fh_camera* cam, const float* bg, const fh_render_layers* layers, uint32_t n_samples, uint32_t max_depth, uint32_t seed)
{
  FH_GROUP(ctx, group_render(ctx, cam, bg, layers, n_samples, max_depth, seed));
  CTX_CHECK(ctx);
  if (!cam || !bg || !layers || !layers->beauty || !layers->position || !layers->depth || !layers->normal || !layers->texcoord || !layers->albedo)
    return fail(ctx, FH_E_INVALID, "fh_render: null argument");
  return render_submit(ctx, cam, bg, layers, n_samples, max_depth, seed);
}

int fh_sync(fh_ctx* ctx)
{
  FH_GROUP_EACH(ctx, kGroupCallPlain, fh_sync(m_));
  CTX_CHECK(ctx);
  if (ctx->render_pending) (void)hipEventRecord(ctx->ev_render_end, ctx->stream);
  FH_HIP(hipStreamSynchronize(ctx->stream));
  if (ctx->render_pending) {
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, ctx->ev_render_begin, ctx->ev_render_end) == hipSuccess) ctx->stats.render_ms += ms;
    ctx->render_pending = false;
  }
  for (auto& s : ctx->spans) {
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) {
      if (s.kind == 0) ctx->stats.trace_closest_ms += ms;
      else if (s.kind == 1) ctx->stats.trace_shadow_ms += ms;
      else if (s.kind == 3) ctx->stats.tail_ms += ms;
      else if (s.kind == 4) ctx->stats.generate_ms += ms;
      else if (s.kind == 5) ctx->stats.accumulate_ms += ms;
      else if (s.kind == 6) ctx->stats.queue_ms += ms;
      else if (s.kind == 7) ctx->stats.post_ms += ms;
      else ctx->stats.shade_ms += ms;
    }
    ctx->event_pool.push_back(std::move(s.a));
    ctx->event_pool.push_back(std::move(s.b));
  }
  ctx->spans.clear();
  if (ctx->sky_taken_pending) {  // samples the adaptive k_sky_pixels took (it stops pixels on the device)
    unsigned long long taken = 0;
    FH_HIP(hipMemcpy(&taken, ctx->d_sky_taken, sizeof taken, hipMemcpyDeviceToHost));
    FH_HIP(hipMemset(ctx->d_sky_taken, 0, sizeof taken));
    ctx->stats.paths += taken;
    ctx->stats.sky_pixel_samples += taken;
    ctx->sky_taken_pending = false;
  }
  if (ctx->stats.sky_pixel_samples && ctx->d_split_counters) {  // k_sky_pixels re-runs the scene-bounds test of every sample it renders: a hit there means the conservative split was wrong
    uint32_t violations = 0;
    FH_HIP(hipMemcpy(&violations, ctx->d_split_counters + 2, 4, hipMemcpyDeviceToHost));
    if (violations) {
      (void)hipMemsetAsync(ctx->d_split_counters + 2, 0, 4, ctx->stream);
      return fail(ctx, FH_E_HIP, "sky-pixel split: " + std::to_string(violations) + " pixels classified as sky have rays that reach the scene bounds (set FH_SKY_SPLIT=0 and report)");
    }
  }
#if defined(FH_CHECK_DIV_RANGES)
  {
    uint64_t n = 0;  // (every call on this device since the library was loaded, whichever context made it: the test reads it from a context of its own)
    if (const int rc = div_range_violations_read(ctx, &n)) return rc;
    ctx->stats.div_range_violations = n;
  }
#endif
  if (ctx->flags & FH_FLAG_TIME_KERNELS) {  // shader cycles and 100 MHz ticks the waves of the streaming traversal kernels have summed up (fh_device.h: ClockStamp)
    unsigned long long c[4];
    FH_HIP(hipMemcpy(c, ctx->d_trace_counters + 27, sizeof c, hipMemcpyDeviceToHost));
    ctx->stats.clk_cycles_closest = c[0]; ctx->stats.clk_ticks_closest = c[1]; ctx->stats.clk_cycles_shadow = c[2]; ctx->stats.clk_ticks_shadow = c[3];
  }
  if (ctx->flags & FH_FLAG_COUNT_TRAVERSAL) {
    unsigned long long c[32];
    FH_HIP(hipMemcpy(c, ctx->d_trace_counters, sizeof c, hipMemcpyDeviceToHost));
    ctx->stats.wave_node_steps_closest = c[6]; ctx->stats.wave_tri_steps_closest = c[7]; ctx->stats.wave_node_steps_shadow = c[8]; ctx->stats.wave_tri_steps_shadow = c[9];
    for (int k = 0; k < 8; ++k) { ctx->stats.hist_nodes_closest[k] = c[10 + k]; ctx->stats.hist_nodes_shadow[k] = c[18 + k]; }
    ctx->stats.nodes_closest = c[0]; ctx->stats.tris_closest = c[1]; ctx->stats.rays_closest = c[2];
    ctx->stats.nodes_shadow = c[3]; ctx->stats.tris_shadow = c[4]; ctx->stats.rays_shadow = c[5];
    ctx->stats.shaded_hits = c[26];
  }
  return FH_OK;
}

int fh_get_stats(fh_ctx* ctx, fh_stats* out)
{
  FH_GROUP(ctx, group_get_stats(ctx, out));
  CTX_CHECK(ctx);
  if (!out) return FH_E_INVALID;
  *out = ctx->stats;
  return FH_OK;
}
int fh_kernel_info(fh_ctx* ctx, int which, uint32_t out[6])
{
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  if (!out || which < 0 || which > 1 + (int)kMaxClasses) return fail(ctx, FH_E_INVALID, "fh_kernel_info: which must be 0 (closest hit), 1 (secondary rays) or 2 + a shading class of the scene");
  return kernel_info(ctx, which, out);
}
// test hook (fredholm_hip_test.h): where the scene's first-hit rays start, and what the probing passes have counted so far
int fh_kat_ray_start(fh_ctx* ctx, double out[5])
{
  FH_GROUP_REFUSE(ctx, "fh_kat_ray_start");
  CTX_CHECK(ctx);
  if (!out) return fail(ctx, FH_E_INVALID, "fh_kat_ray_start: null argument");
  out[0] = (double)ctx->tree.bu_choice; out[1] = ctx->tree.bu_items[0]; out[2] = ctx->tree.bu_items[1]; out[3] = ctx->tree.bu_cost[0]; out[4] = ctx->tree.bu_cost[1];
  return FH_OK;
}
int fh_reset_stats(fh_ctx* ctx)
{
  FH_GROUP_EACH(ctx, kGroupCallPlain, fh_reset_stats(m_));
  CTX_CHECK(ctx);
  const double build_ms = ctx->stats.bvh_build_ms;
  const uint64_t nodes = ctx->stats.bvh_nodes, nb = ctx->stats.bvh_node_bytes, tb = ctx->stats.bvh_tri_bytes, depth = ctx->stats.bvh_depth;
  ctx->stats = fh_stats{};
  ctx->stats.bvh_build_ms = build_ms; ctx->stats.bvh_nodes = nodes; ctx->stats.bvh_node_bytes = nb; ctx->stats.bvh_tri_bytes = tb; ctx->stats.bvh_depth = depth;
  FH_HIP(hipMemsetAsync(ctx->d_trace_counters, 0, 32 * sizeof(unsigned long long), ctx->stream));
  return FH_OK;
}

int fh_post_process(fh_ctx* ctx, const float* in, float* hi, float* tmp, int w, int h, const fh_post_params* pp, float* out)
{
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  if (!in || !hi || !tmp || !out || !pp || w <= 0 || h <= 0) return fail(ctx, FH_E_INVALID, "fh_post_process: bad argument");
  return post_process_submit(ctx, in, hi, tmp, w, h, pp, out);
}

// auto-exposure of the post chain (post.hip, fh_meter.h).  Every refusal of the parameters is decided before the context is looked at; on a group all of it lives
// and runs on the lead, as fh_post_process does
int fh_set_auto_exposure(fh_ctx* ctx, const fh_auto_exposure_params* params)
{
  if (const char* why = auto_exposure_refusal(params)) return fail(ctx, FH_E_INVALID, std::string("fh_set_auto_exposure: ") + why);
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  return auto_exposure_set(ctx, params);
}

int fh_get_auto_exposure(fh_ctx* ctx, int* on, fh_auto_exposure_params* params)
{
  FH_GROUP_LEAD(ctx);
  if (!ctx || !on) return FH_E_INVALID;
  *on = ctx->auto_exposure;
  if (params) *params = ctx->ae_params;
  return FH_OK;
}

int fh_auto_exposure_reset(fh_ctx* ctx)
{
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  if (!ctx->auto_exposure) return fail(ctx, FH_E_INVALID, "fh_auto_exposure_reset: auto-exposure is off (fh_set_auto_exposure)");
  return auto_exposure_reset(ctx);
}

int fh_meter_exposure(fh_ctx* ctx, const float* image_rgba, uint32_t width, uint32_t height)
{
  if (!image_rgba || width == 0 || height == 0 || width > 32768 || height > 32768) return fail(ctx, FH_E_INVALID, "fh_meter_exposure: needs an image of 1 .. 32768 pixels each way");
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  if (!ctx->auto_exposure) return fail(ctx, FH_E_INVALID, "fh_meter_exposure: auto-exposure is off (fh_set_auto_exposure)");
  return meter_submit(ctx, image_rgba, width, height);
}

int fh_get_auto_exposure_state(fh_ctx* ctx, fh_auto_exposure_state* state)
{
  if (!state) return fail(ctx, FH_E_INVALID, "fh_get_auto_exposure_state: null argument");
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  if (!ctx->auto_exposure) return fail(ctx, FH_E_INVALID, "fh_get_auto_exposure_state: auto-exposure is off (fh_set_auto_exposure)");
  return auto_exposure_read(ctx, state, nullptr);
}

int fh_get_luminance_histogram(fh_ctx* ctx, uint32_t hist[257])
{
  if (!hist) return fail(ctx, FH_E_INVALID, "fh_get_luminance_histogram: null argument");
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  if (!ctx->auto_exposure) return fail(ctx, FH_E_INVALID, "fh_get_luminance_histogram: auto-exposure is off (fh_set_auto_exposure)");
  return auto_exposure_read(ctx, nullptr, hist);
}

// local exposure of the post chain (post.hip, fh_local_exposure.h): the same rules as auto-exposure above
int fh_set_local_exposure(fh_ctx* ctx, const fh_local_exposure_params* params)
{
  if (const char* why = local_exposure_refusal(params)) return fail(ctx, FH_E_INVALID, std::string("fh_set_local_exposure: ") + why);
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  return local_exposure_set(ctx, params);
}

int fh_get_local_exposure(fh_ctx* ctx, int* on, fh_local_exposure_params* params)
{
  FH_GROUP_LEAD(ctx);
  if (!ctx || !on) return FH_E_INVALID;
  *on = ctx->local_exposure;
  if (params) *params = ctx->lx_params;
  return FH_OK;
}

int fh_local_exposure_analyse(fh_ctx* ctx, const float* image_rgba, uint32_t width, uint32_t height)
{
  if (!image_rgba || width == 0 || height == 0 || width > 32768 || height > 32768) return fail(ctx, FH_E_INVALID, "fh_local_exposure_analyse: needs an image of 1 .. 32768 pixels each way");
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  if (!ctx->local_exposure) return fail(ctx, FH_E_INVALID, "fh_local_exposure_analyse: local exposure is off (fh_set_local_exposure)");
  return local_exposure_submit(ctx, image_rgba, width, height);
}

int fh_get_local_exposure_base(fh_ctx* ctx, float* base, uint32_t* w4, uint32_t* h4)
{
  if (!w4 || !h4) return fail(ctx, FH_E_INVALID, "fh_get_local_exposure_base: null argument");
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  if (!ctx->local_exposure) return fail(ctx, FH_E_INVALID, "fh_get_local_exposure_base: local exposure is off (fh_set_local_exposure)");
  return local_exposure_read_base(ctx, base, w4, h4);
}

int fh_denoise(fh_ctx* ctx, uint32_t width, uint32_t height, const float* beauty, const float* normal, const float* albedo, float* denoised, int upscale2x)
{
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  if (!beauty || !normal || !albedo || !denoised || width == 0 || height == 0 || width > 32768 || height > 32768) return fail(ctx, FH_E_INVALID, "fh_denoise: bad argument");
  return denoise_submit(ctx, (int)width, (int)height, beauty, normal, albedo, denoised, upscale2x ? 1 : 0);
}

// fh_denoise_guided, fh_denoise_temporal, the history calls and their switches: denoise.hip

// OpenGL interop (cwl::CUDAGLBuffer, cwl/include/cwl/buffer.h:88-143: cuGraphicsGLRegisterBuffer + map + mapped pointer, unmapped and
// unregistered in the destructor).  Needs a current OpenGL context on the calling thread, like the reference.
int fh_gl_register_buffer(fh_ctx* ctx, unsigned int gl_buffer, void** resource, void** device_ptr, uint64_t* bytes)
{
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  if (!resource || !device_ptr) return fail(ctx, FH_E_INVALID, "fh_gl_register_buffer: null argument");
  *resource = nullptr; *device_ptr = nullptr;
  hipGraphicsResource_t res = nullptr;
  FH_HIP(hipGraphicsGLRegisterBuffer(&res, (GLuint)gl_buffer, hipGraphicsRegisterFlagsNone));
  hipError_t e = hipGraphicsMapResources(1, &res, ctx->stream);
  size_t size = 0;
  void* ptr = nullptr;
  if (e == hipSuccess) e = hipGraphicsResourceGetMappedPointer(&ptr, &size, res);
  if (e != hipSuccess) {
    (void)hipGraphicsUnregisterResource(res);
    return fail(ctx, FH_E_HIP, std::string("fh_gl_register_buffer: ") + hipGetErrorString(e));
  }
  *resource = (void*)res; *device_ptr = ptr;
  if (bytes) *bytes = (uint64_t)size;
  return FH_OK;
}
int fh_gl_unregister_buffer(fh_ctx* ctx, void* resource)
{
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  if (!resource) return FH_OK;
  hipGraphicsResource_t res = (hipGraphicsResource_t)resource;
  (void)hipStreamSynchronize(ctx->stream);
  FH_HIP(hipGraphicsUnmapResources(1, &res, ctx->stream));
  FH_HIP(hipGraphicsUnregisterResource(res));
  return FH_OK;
}

int fh_malloc(fh_ctx* ctx, uint64_t bytes, void** out)
{
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  if (!out) return FH_E_INVALID;
  FH_HIP(hipMalloc(out, bytes ? bytes : 16));
  return FH_OK;
}
int fh_free(fh_ctx* ctx, void* p)
{
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  FH_HIP(hipFree(p));
  return FH_OK;
}
int fh_memset(fh_ctx* ctx, void* p, int v, uint64_t bytes)
{
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  FH_HIP(hipMemsetAsync(p, v, bytes, ctx->stream));
  return FH_OK;
}
int fh_copy_to_device(fh_ctx* ctx, void* dst, const void* src, uint64_t bytes)
{
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  FH_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  FH_HIP(hipStreamSynchronize(ctx->stream));
  return FH_OK;
}
int fh_image_load_rgba8(const char* path, int flip_vertically, uint32_t* width, uint32_t* height, uint8_t** rgba8)
{
  if (!path || !width || !height || !rgba8) { g_create_error = "fh_image_load_rgba8: null argument"; return FH_E_INVALID; }
  try {
    const fredholm::image_io::Image8 img = fredholm::image_io::load_rgba8(path, flip_vertically != 0);
    uint8_t* out = (uint8_t*)std::malloc(img.rgba.size() ? img.rgba.size() : 1);
    if (!out) { g_create_error = "fh_image_load_rgba8: out of memory"; return FH_E_INVALID; }
    std::memcpy(out, img.rgba.data(), img.rgba.size());
    *width = (uint32_t)img.width; *height = (uint32_t)img.height; *rgba8 = out;
    return FH_OK;
  } catch (const std::exception& e) {
    g_create_error = e.what();
    return FH_E_INVALID;
  }
}
void fh_image_free(uint8_t* rgba8) { std::free(rgba8); }
int fh_copy_on_device(fh_ctx* ctx, void* dst, const void* src, uint64_t bytes)
{
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  FH_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  return FH_OK;
}
int fh_copy_to_host(fh_ctx* ctx, void* dst, const void* src, uint64_t bytes)
{
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  FH_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  FH_HIP(hipStreamSynchronize(ctx->stream));
  return FH_OK;
}
void* fh_stream(fh_ctx* ctx)
{
  FH_GROUP_LEAD(ctx);
  return ctx ? (void*)ctx->stream : nullptr;
}

}  // extern "C"
