/* fredholm_hip.h -- C ABI of libfredholm_hip.so, the MI355X (gfx950) replacement for the render
 * loop of yumcyaWiz/fredholm.
 *
 * The reference has no FFI: applications call the header-only C++ class fredholm::Renderer
 * (fredholm/include/fredholm/renderer.h) directly.  Each entry point below is what one of its
 * methods forwards to in the drop-in facade (include/fredholm/renderer.h in this repo); the
 * reference method it replaces is cited as file:line.  All arguments are plain pointers and
 * sizes; device pointers are HIP device addresses owned by the caller unless stated otherwise.
 *
 * Error convention: every function returns FH_OK (0) or a negative FH_E_* code and records a
 * message retrievable with fh_last_error(); the C++ facade turns non-zero into
 * std::runtime_error, matching the reference's CUDA_CHECK / OPTIX_CHECK behaviour
 * (cwl/include/cwl/util.h:11-34, optwl/include/optwl/optwl.h:11-35).
 * Threading: one host thread drives a context (reference: gui thread / rtcamp8 render thread);
 * fh_render is asynchronous on the context's private HIP stream, fh_sync blocks.
 */
#ifndef FREDHOLM_HIP_H
#define FREDHOLM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FH_OK 0
#define FH_E_INVALID -1      /* bad argument / state */
#define FH_E_HIP -2          /* a HIP runtime call failed */
#define FH_E_UNSUPPORTED -3  /* feature present in the reference but not in this build (glTF, image file decoding) */

typedef struct fh_ctx fh_ctx;

/* 180-byte material record, field-for-field the reference's Material (fredholm/include/fredholm/shared.h:100-142) */
typedef struct fh_material {
  float diffuse; float base_color[3]; int32_t base_color_texture_id; float diffuse_roughness;
  float specular; float specular_color[3]; int32_t specular_color_texture_id; float specular_roughness; int32_t specular_roughness_texture_id;
  float metalness; int32_t metalness_texture_id; int32_t metallic_roughness_texture_id;
  float coat; int32_t coat_texture_id; float coat_color[3]; float coat_roughness; int32_t coat_roughness_texture_id;
  float transmission; float transmission_color[3];
  float sheen; float sheen_color[3]; float sheen_roughness;
  float subsurface; float subsurface_color[3];
  float thin_walled;
  float emission; float emission_color[3]; int32_t emission_texture_id;
  int32_t heightmap_texture_id; int32_t normalmap_texture_id; int32_t alpha_texture_id;
} fh_material;

/* 8-bit RGBA texture as the reference's Texture holds it after stb_image load (fredholm/src/scene.cpp:7-37: 4 channels,
 * v-flipped on load) plus its TextureType: srgb = 1 for COLOR textures (hardware sRGB decode, cwl/texture.h:35-47) */
typedef struct fh_texture_desc {
  uint32_t width, height;
  const uint8_t* rgba8;
  int32_t srgb;
} fh_texture_desc;

/* Host-side flat scene, exactly the arrays Renderer::load_scene uploads (renderer.h:361-421; Scene members scene.h:103-135).
 * transforms are 3x4 row-major object_to_world / world_to_object per instance (renderer.h:404-421); NULL / 0 = one identity. */
typedef struct fh_scene_desc {
  uint32_t n_vertices;
  const float* vertices;  /* float3[n_vertices] */
  const float* normals;   /* float3[n_vertices] */
  const float* texcoords; /* float2[n_vertices] */
  uint32_t n_faces;
  const uint32_t* indices;      /* uint3[n_faces] */
  const uint32_t* material_ids; /* uint[n_faces]  */
  const uint32_t* instance_ids; /* uint[n_faces], may be NULL (all 0) */
  uint32_t n_materials;
  const fh_material* materials;
  uint32_t n_instances;
  const float* object_to_world; /* float[12] per instance, may be NULL */
  const float* world_to_object; /* float[12] per instance, may be NULL */
  uint32_t n_textures;           /* textures referenced by the materials' *_texture_id fields (renderer.h:372-386) */
  const fh_texture_desc* textures;
} fh_scene_desc;

/* CameraParams (shared.h:59-64): camera-to-world 3x4 rows, vertical fov in radians, F-number, focus distance */
typedef struct fh_camera {
  float transform[12];
  float fov, F, focus;
} fh_camera;

/* RenderLayer (shared.h:201-208): six caller-owned device buffers of width*height elements */
typedef struct fh_render_layers {
  float* beauty;   /* float4 */
  float* position; /* float4 */
  float* depth;    /* float  */
  float* normal;   /* float4 */
  float* texcoord; /* float4 */
  float* albedo;   /* float4 */
} fh_render_layers;

/* PostProcessParams (fredholm/kernels/include/kernels/post-process.h:4-10) */
typedef struct fh_post_params {
  int32_t use_bloom;
  float bloom_threshold, bloom_sigma, ISO, chromatic_aberration;
} fh_post_params;

/* counters / timers of the last fh_render .. fh_sync interval, see fh_get_stats */
typedef struct fh_stats {
  double render_ms;        /* HIP-event time of the whole fh_render submission on the context stream */
  double trace_closest_ms; /* summed HIP-event time of the closest-hit traversal kernel launches */
  double trace_shadow_ms;  /* summed time of the any-hit / secondary traversal kernel launches */
  double shade_ms;         /* summed time of the shade kernels */
  uint64_t n_closest_launches, n_shadow_launches;
  uint64_t rays_closest, rays_shadow;          /* rays traced by the two traversal kernels (only when FH_FLAG_COUNT_TRAVERSAL) */
  uint64_t nodes_closest, tris_closest;        /* node visits / triangle tests (only when FH_FLAG_COUNT_TRAVERSAL) */
  uint64_t nodes_shadow, tris_shadow;
  uint64_t paths;                              /* camera paths started */
  double bvh_build_ms;
  uint64_t bvh_nodes, bvh_node_bytes, bvh_tri_bytes;
  /* instrumented build only: wave-level executions of the node test / triangle test (SIMD efficiency =
   * nodes_* / (64 * wave_node_steps_*), likewise for triangles) */
  uint64_t wave_node_steps_closest, wave_tri_steps_closest, wave_node_steps_shadow, wave_tri_steps_shadow;
  /* instrumented build only: rays by number of node visits: <= 8, 16, 32, 64, 128, 256, 512, more */
  uint64_t hist_nodes_closest[8], hist_nodes_shadow[8];
  double tail_ms; /* summed HIP-event time of the k_tail launches */
  double generate_ms, accumulate_ms, queue_ms; /* k_generate + k_bump_issued ; k_accumulate ; k_route + the cell sorts of the bounce queues */
  uint64_t n_generate_launches, n_accumulate_launches, n_shade_launches, n_tail_launches;
  uint64_t shaded_hits; /* surface hits shaded by the k_shade kernels (only when FH_FLAG_COUNT_TRAVERSAL) */
  uint64_t bvh_depth;   /* node levels of the wide BVH; a traversal stack needs levels - 1 entries, of which the streaming kernels may keep only the first in LDS (fh_kernel_info) */
  double post_ms;       /* summed HIP-event time of the fh_post_process chains (threshold + blur + tone map) */
  uint64_t n_post_launches;
  /* FH_FLAG_TIME_KERNELS, streaming traversal kernels: shader cycles (s_memtime) and 100 MHz ticks (s_memrealtime) summed over their waves;
   * the clock the chip held while they ran = cycles / ticks x 100 MHz */
  uint64_t clk_cycles_closest, clk_ticks_closest, clk_cycles_shadow, clk_ticks_shadow;
  uint64_t n_passes;          /* passes of the path pools submitted */
  uint64_t sky_pixel_samples; /* camera samples (counted in `paths`) rendered by the sky-pixel kernel: samples of pixels no ray of which can reach the scene's bounds */
  uint64_t div_range_violations; /* libraries built with -DFH_CHECK_DIV_RANGES only (else 0): short divisions (fh_elementary.h: fhe_div) whose operands left the range their
                                    site claims, on this device since the library was loaded (by any context), as of the last fh_sync */
} fh_stats;

#define FH_FLAG_TIME_KERNELS 1u    /* bracket traversal/shade launches with HIP events (fh_stats *_ms) */
#define FH_FLAG_COUNT_TRAVERSAL 2u /* instrumented traversal kernels: count node visits / triangle tests */
/* bug-compatible multi-sample launches.  fh_render(n_samples = k) is by default k one-sample launches.  With this flag it reproduces
 * what ONE reference launch of k samples computes: the reference never resets payload.firsthit inside a launch (pt.cu:432-433), so only
 * the first sample of the launch that hits anything records AOVs / sees emitters directly (:745-760), primary misses after it add no sky
 * (:509) and every sample averages that first hit's AOVs again (:483-487).  rtcamp8 renders 16 samples per launch (rtcamp8.cpp:183-189). */
#define FH_FLAG_REFERENCE_FIRSTHIT 4u
/* run the passes of fh_render one after the other on the main stream instead of two in flight: slower, but every kernel then runs alone
 * on the GPU, so the HIP-event times of FH_FLAG_TIME_KERNELS are kernel times (with passes in flight they include the other stream's work) */
#define FH_FLAG_SERIAL_PASSES 8u
/* measurements: every ray starts its traversal at the root, whatever the library decided for the scene (render.hip: where a pass's first-hit rays start); results do not
 * depend on it -- bench.py counts with it what a walk from the root would have tested */
#define FH_FLAG_ROOT_START 16u

/* -- context: replaces optwl::Context + Renderer ctor/dtor (optwl.h:41-81, renderer.h:32-122) */
int fh_ctx_create(int device, fh_ctx** out);
int fh_ctx_destroy(fh_ctx* ctx);

/* -- one frame on several GPUs from a single context (an extension beyond the reference; DESIGN.md 6, INTEGRATION.md "multi-GPU").
 * n = 1 returns a plain context, exactly what fh_ctx_create(devices[0]) returns.
 * 2 <= n <= 16: a GROUP: one member context per entry of devices[] (an index may repeat: several members on one GPU).  Member i renders the tiles t with t % n == i.
 * Device pointers the caller passes (layers, fh_malloc results, post / denoise images) belong to devices[0], the LEAD.  The handle is used like any context:
 * state-setting calls reach every member, fh_render fans out and gathers on the device, memory / post / denoise / query calls go to the lead, and
 * fh_pack_owned, fh_unpack_shard, fh_unpack_shards and the known-answer hooks of fredholm_hip_test.h return FH_E_UNSUPPORTED (INTEGRATION.md has the table).
 * fh_set_tile_shard(group, 0, 1, tw, th) sets the tile size; any other rank / world is FH_E_INVALID, because a group is the whole frame.
 * When a call fails on member i, its code is returned and fh_last_error(group) gives its message prefixed with "member i: "; where the members could then disagree
 * (a scene or frame-state call that did not reach all of them) fh_render returns FH_E_INVALID until fh_scene_upload / fh_set_resolution succeeded again.
 * n = 0, n > 16, a null pointer (all refused before any HIP call) and a device index out of range are FH_E_INVALID; nothing is left behind.
 *
 * fh_render on a group: the lead renders its tiles straight into the caller's six buffers.  Every other member accumulates in six full-size layers of its own
 * (zero-filled by fh_set_resolution and fh_init_render_states), packs the owned pixels of the layers in the gather mask after its passes, and one asynchronous copy
 * per member and one un-permuting launch on the lead's stream (the one fh_stream returns) put them into the caller's buffers: work queued on that stream afterwards
 * sees the whole frame, and after fh_sync(group) so does the host.  What a caller may observe:
 *  - layers outside the gather mask receive only the lead's tiles;
 *  - swapping the layer buffers in the middle of an accumulation gives the lead's tiles accumulated in the new buffers and the other tiles copied in;
 *  - at the first sample after fh_init_render_states a pixel of a non-lead member starts from a zeroed mean, where a plain context starts from what the caller's
 *    buffer holds.  The update is coef * (fn * old + x) with fn = 0 at count 0 (k_accumulate and k_sky_pixels alike), so the two agree unless the caller's buffer held
 *    Inf or NaN there (0 * old is NaN), or a negative old value met x = -0.0 (-0.0 where a zeroed buffer gives +0.0). */
int fh_ctx_create_group(const int* devices, uint32_t n, fh_ctx** out);
int fh_ctx_group_size(fh_ctx* ctx, uint32_t* n);             /* 1 for a plain context */
int fh_ctx_member(fh_ctx* ctx, uint32_t i, fh_ctx** member); /* borrowed, for stats and diagnostics only; member 0 of a plain context is the context */
#define FH_LAYER_BEAUTY 1u
#define FH_LAYER_POSITION 2u
#define FH_LAYER_DEPTH 4u
#define FH_LAYER_NORMAL 8u
#define FH_LAYER_TEXCOORD 16u
#define FH_LAYER_ALBEDO 32u
#define FH_LAYER_ALL 63u
int fh_group_set_gather_layers(fh_ctx* ctx, uint32_t mask); /* default FH_LAYER_ALL; a plain context accepts and ignores it */
/* synchronising: HIP-event times (ms) of the last gather of a group whose flags had FH_FLAG_TIME_KERNELS: [0] k_pack_layers and [1] the copies, each summed over the
 * members, [2] k_unpack_group.  Zeros for a plain context. */
int fh_group_gather_times(fh_ctx* ctx, double ms[3]);
/* host only, no context: where each member's packed shard begins in the lead's staging area for a frame, a tile size, n members and a gather mask: n + 1 byte offsets
 * (a shard is layer after layer in ownership-list order, 16 or 4 bytes per pixel, each layer padded to 16 bytes; the lead packs nothing, so offsets[0] = offsets[1] = 0) */
int fh_group_shard_layout(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t n, uint32_t mask, uint64_t* offsets);
const char* fh_last_error(fh_ctx* ctx); /* ctx may be NULL for creation errors */
int fh_set_flags(fh_ctx* ctx, uint32_t flags);
int fh_get_flags(fh_ctx* ctx, uint32_t* flags); /* (a caller that wants to change one flag reads, edits and sets) */
/* target number of camera paths in flight per pass (path-pool slots); a pass starts floor(target / owned pixels) >= 1
 * samples per pixel.  Results do not depend on it.  Default 32 Mi paths per pool, three pools (one per pass in flight), 284-436 bytes per path.  Whenever a
 * default-sized pool has to be allocated (first frame, after fh_scene_upload changed what a path record holds) the default is lowered so that all pools together
 * stay within a quarter of the device memory that is free at that moment (memory the pools already hold counts as free); a size set here is taken as given.
 * The target is an upper bound: a pool is allocated for the paths its passes really start -- (owned pixels that can see the scene) x (samples per pass) -- and only grows. */
int fh_set_path_pool(fh_ctx* ctx, uint32_t target_paths);
/* device memory of the path pools with the scene and lights as they are now: bytes per path slot and the number of pools (one per pass in flight);
 * a caller that sizes the pools for a frame (bench.py) multiplies: pools x target_paths x bytes_per_path */
int fh_path_pool_bytes(fh_ctx* ctx, uint64_t* bytes_per_path, uint32_t* pools);
/* cut-out faces of the uploaded scene: [0] faces whose textures can discard a hit (pt.cu:545-678), [1] of them: the any-hit test passes wherever the face can be hit (no test
 * at run time), [2] it never passes (no ray can hit the face), [3] faces that keep their test.  Decided per face at fh_scene_upload from the texels the face can address. */
int fh_alpha_face_counts(fh_ctx* ctx, uint32_t counts[4]);
/* the opacity micromaps of the faces that keep their test (16 x 16 cells of a face's barycentrics, decided at upload like the faces themselves): [0] cells, [1] of them: the
 * test passes everywhere in the cell, [2] nowhere; candidates in such cells are decided by a two-bit look-up */
int fh_alpha_cell_counts(fh_ctx* ctx, uint64_t counts[3]);
/* what the path pools hold right now: device bytes of all pools together and path slots (summed over the pools) */
int fh_path_pool_allocated(fh_ctx* ctx, uint64_t* bytes, uint64_t* paths);
/* number of bounces run as bounce-synchronous wavefront kernels before the surviving paths are finished by one
 * fused launch (k_tail).  Results do not depend on it.  0 (default) = adaptive: the depth at which fewer than 64 Ki
 * paths survived in earlier passes; a value >= max_depth disables the fused tail. */
int fh_set_tail_depth(fh_ctx* ctx, uint32_t depth);

/* -- scene: Renderer::load_scene upload + AreaLight extraction (renderer.h:354-432).  FH_E_INVALID (missing arrays, a texture id outside the
 * textures, an empty texture, an instance id, material id or vertex index out of range) is found from the arguments alone, before anything is
 * changed: the context keeps the scene, the tree and the counters it had.  After FH_E_HIP the context has no scene until an upload succeeds. */
int fh_scene_upload(fh_ctx* ctx, const fh_scene_desc* scene);
/* Renderer::build_gas + build_ias (renderer.h:434-552): on-device LBVH build + wide-BVH collapse */
int fh_bvh_build(fh_ctx* ctx);
/* Renderer::set_time's transform re-upload + IAS rebuild (renderer.h:614-640); call fh_bvh_build afterwards */
int fh_set_transforms(fh_ctx* ctx, uint32_t n_instances, const float* object_to_world, const float* world_to_object);
int fh_scene_n_lights(fh_ctx* ctx, uint32_t* out);

/* -- skeletal skinning (an extension beyond the reference, whose glTF reader loads no skins): linear-blend skinning of the uploaded scene's vertices on the device,
 * one stage in front of the face records.  A skin gives every vertex four joint indices j[4] into ONE palette per scene and four weights w[4]; a pose is the palette:
 * n_joints row-major 3 x 4 matrices J in the object space of the skinned vertices.  fh_set_transforms composes on top (posed object space first, then the instance
 * transform); either order of the two calls gives the same bits.  Call fh_bvh_build afterwards, as after fh_set_transforms: the tree is refitted, or rebuilt when
 * its node area has grown past 1.5 x; the light table and the light proxies are rebuilt by the next fh_render.
 *
 * The arithmetic (csrc/fh_skin.h), per vertex with bind position p and bind normal n, in fp32 without contraction, / and sqrt correctly rounded, every product and
 * every sum rounded, sums taken left to right unless bracketed:
 *   - all four weights == 0: the posed position and normal are the bind ones, bit for bit.  Otherwise
 *   - B[e] = ((w0 * J[j0][e] + w1 * J[j1][e]) + w2 * J[j2][e]) + w3 * J[j3][e] for each of the 12 entries e.  Weights are used as given: no renormalisation.
 *   - position: p'[r] = B[r][0] * p.x + B[r][1] * p.y + B[r][2] * p.z + B[r][3] * 1 for the rows r = 0, 1, 2.
 *   - normal: with L0, L1, L2 the rows of B's 3 x 3 part, cross(a, b) = (a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x) and
 *     dot(a, b) = a.x * b.x + a.y * b.y + a.z * b.z: C0 = cross(L1, L2), C1 = cross(L2, L0), C2 = cross(L0, L1) (the cofactor matrix: the inverse transpose without
 *     its division by the determinant); m = (dot(C0, n), dot(C1, n), dot(C2, n)); m is negated when dot(L0, C0) < 0; ln = sqrtf(dot(n, n)), lm = sqrtf(dot(m, m));
 *     if lm is 0, infinite or NaN the posed normal is n; else s = ln / lm and the posed normal is (m.x * s, m.y * s, m.z * s): the bind normal's length is kept,
 *     because emitter normals are used un-normalised.
 * FH_E_INVALID, decided from the arguments and the context's counters before anything is changed (csrc/skin_plan_host.h): no scene loaded; n_vertices different from
 * the uploaded scene's; null arrays; n_joints 0 or above 65536; a weight that is not finite; a joint index >= n_joints on a vertex with a non-zero weight;
 * matrices before a skin was set; a matrix count different from n_joints; a matrix entry that is not finite.
 * The skin and the palette belong to the uploaded scene: fh_scene_upload drops them.  A group broadcasts both setters; the two queries go to the lead.
 * Not covered: morph targets, more than four influences per vertex, dual-quaternion blending, motion vectors for skinned pixels, per-sample motion blur. */
typedef struct fh_skin_desc {
  uint32_t n_vertices;    /* the uploaded scene's */
  uint32_t n_joints;      /* 1 .. 65536 */
  const uint16_t* joints; /* 4 per vertex */
  const float* weights;   /* 4 per vertex */
} fh_skin_desc;
/* NULL clears: geometry returns to the bind pose, bit for bit.  A skin alone changes no bit of any render: geometry stays in the bind pose until the first
 * fh_set_joint_matrices (setting a skin over a posed one returns to the bind pose as well). */
int fh_set_skin(fh_ctx* ctx, const fh_skin_desc* skin);
/* row-major 3 x 4 each, object space of the skinned vertices.  Matrices equal to the ones held return at once: geometry and tree stay. */
int fh_set_joint_matrices(fh_ctx* ctx, uint32_t n, const float* m3x4);
/* any pointer may be NULL.  n_joints 0: no skin; n_skinned_vertices: vertices with a non-zero weight */
int fh_get_skin_info(fh_ctx* ctx, uint32_t* n_joints, uint32_t* n_skinned_vertices, int* posed);
/* host arrays of 3 floats per vertex of the uploaded scene; the bind arrays when nothing is posed */
int fh_get_posed_geometry(fh_ctx* ctx, float* vertices3, float* normals3);

/* -- environment: renderer.h:554-612.  le/dir are float[3]; angle in degrees. */
int fh_set_directional_light(fh_ctx* ctx, const float* le, const float* dir, float angle);
int fh_clear_directional_light(fh_ctx* ctx);
int fh_set_sky_intensity(fh_ctx* ctx, float intensity);
int fh_load_arhosek_sky(fh_ctx* ctx, float turbidity, float albedo); /* renderer.h:588-607 */
int fh_clear_arhosek_sky(fh_ctx* ctx);                               /* renderer.h:609-612 */
int fh_load_ibl(fh_ctx* ctx, const float* rgba, uint32_t w, uint32_t h); /* renderer.h:574-581: float4 lat-long image, already decoded */
int fh_clear_ibl(fh_ctx* ctx);                                          /* renderer.h:583-586 */

/* -- frame state: renderer.h:642-655 */
int fh_set_resolution(fh_ctx* ctx, uint32_t width, uint32_t height); /* also resets the sample counters */
int fh_init_render_states(fh_ctx* ctx);                              /* sample_count = 0 */
/* pixel-tile sharding for multi-GPU rendering: this context renders only the tiles t with t % world == rank
 * (tiles of tile_w x tile_h pixels, row-major tile order).  world = 1 renders everything (default). */
int fh_set_tile_shard(fh_ctx* ctx, uint32_t rank, uint32_t world, uint32_t tile_w, uint32_t tile_h);
/* number of pixels this context owns, and pack/unpack of owned pixels for the framebuffer gather */
int fh_owned_pixel_count(fh_ctx* ctx, uint32_t* out);
int fh_pack_owned(fh_ctx* ctx, const float* layer, uint32_t floats_per_pixel, float* packed);
int fh_unpack_shard(fh_ctx* ctx, uint32_t rank, uint32_t world, const float* packed, uint32_t floats_per_pixel, float* layer);
/* the same for ALL ranks of a split in one asynchronous launch: packed[r] = rank r's packed shard (device pointers in a host array of `world` entries, read during the call).
 * What rank 0 calls once per presented frame after the gather (bench.py); world > 16 falls back to one launch per rank. */
int fh_unpack_shards(fh_ctx* ctx, uint32_t world, const float* const* packed, uint32_t floats_per_pixel, float* layer);

/* -- THE hot path: Renderer::render (renderer.h:657-734) -> __raygen__rg & friends (fredholm/modules/pt.cu:418-999).
 * Adds n_samples samples per owned pixel to the running means in `layers`; equivalent to n_samples consecutive
 * reference launches with n_samples = 1 (the reference's only well-defined mode). seed: reference uses 1. */
int fh_render(fh_ctx* ctx, const fh_camera* camera, const float* bg_color, const fh_render_layers* layers, uint32_t n_samples, uint32_t max_depth, uint32_t seed);
int fh_sync(fh_ctx* ctx); /* Renderer::wait_for_completion (renderer.h:736) */
int fh_get_stats(fh_ctx* ctx, fh_stats* out);
int fh_reset_stats(fh_ctx* ctx);

/* -- adaptive sampling (an extension beyond the reference).  While it is on, every accumulated sample also updates two running means per pixel, m1 of the
 * luminance y of the NaN-guarded radiance and m2 of y * y, with the beauty layer's coefficients.  At a pixel's sample count n with n >= min_samples and
 * n % step == 0 the pixel is converged when threshold > 0 and e2 <= (threshold * max(m1, floor))^2, e2 = max(m2 - m1^2, 0) * n / (n - 1) / n; a converged
 * pixel gets no further samples until fh_init_render_states / fh_set_resolution.  fh_render(n) then adds AT MOST n samples per owned pixel, and the bits of
 * every pixel are those of a plain render at its sample count, however the samples are split into calls.  threshold = 0 tracks the moments and stops nothing. */
typedef struct fh_adaptive_params {
  float threshold;       /* >= 0, finite */
  float floor;           /* > 0, finite: the smallest mean the relative error is taken of */
  uint32_t min_samples;  /* >= 2 */
  uint32_t step;         /* >= 1; 16 keeps every stop at the end of a CMJ 4x4 block */
} fh_adaptive_params;
/* NULL: off (the default).  Turning it on or changing its parameters is FH_E_INVALID once a sample has been accumulated since fh_init_render_states /
 * fh_set_resolution (the moments start at sample 0); turning it off is accepted at any time.  FH_FLAG_REFERENCE_FIRSTHIT calls of n_samples > 1 are
 * FH_E_INVALID while it is on. */
int fh_set_adaptive_sampling(fh_ctx* ctx, const fh_adaptive_params* params);
int fh_get_adaptive_sampling(fh_ctx* ctx, int* enabled, fh_adaptive_params* params);
/* how adaptive sampling decides (defaults 1, 1: exactly the per-pixel rule above).
 * block in {1, 2, 4, 8}: the guard block of pixel (x, y) is the set of frame pixels (x', y') with x' / block = x / block and y' / block = y / block, cut off by the
 * frame at its right and bottom edges.  A pixel gets no further samples exactly when EVERY pixel of its guard block satisfies the per-pixel predicate above at its
 * own current state.  So all pixels of a block always hold the same count and stop at the same boundary; a stopped block's states are frozen, so the rule keeps
 * holding (it is as stateless as the per-pixel rule); a pixel that passes alone keeps sampling and its moments keep updating; and each pixel still holds the bits
 * of a plain render at its count.  Tile width and height must be multiples of block, so that a block never spans two owners: whichever of this call and
 * fh_set_tile_shard would break that returns FH_E_INVALID.
 * growth in {1, 2}: with b0 the smallest multiple of step >= min_samples, growth 1 puts a boundary at every multiple of step >= min_samples (the rule above) and
 * growth 2 at b0 * 2^k only; a round of fh_render then runs to the next boundary in as many passes as that takes, and the rounds before b0 merge into one.
 * Values outside the sets are FH_E_INVALID and change nothing.  Changing a value once a sample has been accumulated since fh_init_render_states /
 * fh_set_resolution is FH_E_INVALID; setting the values it has is FH_OK.  The policy is accepted while the mode is off and survives turning the mode off and on
 * and fh_set_resolution. */
int fh_set_adaptive_policy(fh_ctx* ctx, uint32_t block, uint32_t growth);
int fh_get_adaptive_policy(fh_ctx* ctx, uint32_t* block, uint32_t* growth);
/* samples from the count requested since fh_init_render_states to the next boundary (>= 1); FH_E_INVALID while the mode is off */
int fh_adaptive_next_boundary(fh_ctx* ctx, uint32_t* samples);
/* device buffer of width * height sample counts, copied on the context stream (works with the mode off too) */
int fh_get_sample_counts(fh_ctx* ctx, uint32_t* counts);
/* device buffer of width * height float2 (m1, m2), copied on the context stream; FH_E_INVALID while the mode is off */
int fh_get_luminance_moments(fh_ctx* ctx, float* moments);
/* synchronising: the owned pixels the next fh_render would sample (all of them while the mode is off) */
int fh_active_pixel_count(fh_ctx* ctx, uint32_t* out);

/* -- post chain: post_process_kernel_launch (fredholm/kernels/src/post-process.cu:5-35); all device pointers, float4 images.
 * The tone map fetches r, g and b of an output pixel from three addresses of beauty_temp that chromatic_aberration moves apart (post-process.cu:122-136).  A fetch
 * address past the last pixel reads the last pixel; the reference leaves this undefined.  (It happens when a clamped coordinate is exactly 1: a negative
 * chromatic_aberration of about a quarter of the width, any value >= width * height, +-inf, NaN.)  Every address in range is the reference's. */
int fh_post_process(fh_ctx* ctx, const float* beauty_in, float* beauty_high_luminance, float* beauty_temp, int width, int height, const fh_post_params* params, float* beauty_out);

/* Denoiser slot (Denoiser::denoise, fredholm/include/fredholm/denoiser.h:87-95).  The reference invokes NVIDIA's OptiX AI denoiser (HDR model with
 * albedo + normal guide layers, optionally the 2x upscaling model), a proprietary network; the slot is filled by an edge-avoiding a-trous wavelet
 * filter (Dammertz et al. 2010) on albedo-demodulated radiance with the same inputs and output: float4 beauty / normal / albedo layers of
 * width x height pixels in, float4 denoised out (2*width x 2*height when upscale2x, by pixel replication).  Asynchronous on the context stream. */
int fh_denoise(fh_ctx* ctx, uint32_t width, uint32_t height, const float* beauty, const float* normal, const float* albedo, float* denoised, int upscale2x);

/* -- the variance-guided denoiser (an extension beyond the reference; opt-in, fh_denoise keeps its bits): the spatial filter of SVGF (Schied et al. 2017) on
 * albedo-demodulated radiance.  Its colour edge stop divides the luminance distance by the standard deviation each pixel is measured to have -- from the moments
 * adaptive sampling keeps, or without them from a 7x7 spatial estimate -- and the variance is filtered along with the colour.
 * All arithmetic is fp32 without contraction, exp is fhe_exp (fh_elementary.h), sqrt and / are correctly rounded, sums run over dy (outer) and dx (inner) ascending.
 * lum(r, g, b) = r * 0.2126729 + g * 0.7151522 + b * 0.0721750 (the luminance of the moments); finite(v) = 0 for NaN and |v| > 3e38, else v; B, N, A, P, Z, (m1, m2), n
 * are the inputs at a pixel; q is the tap position clamped to the frame.
 *   Preparation, per pixel p: a' = max(A.rgb, 0.01), c = finite(B.rgb) / a', l = lum(c).  Variance v of l
 *     with moments:    n >= 2: v = max(m2 - m1 * m1, 0) / (n - 1) * (r * r), r = l / max(m1, 1e-3);   n < 2: v = l * l
 *     without moments: over the 7 x 7 window, wn = max(0, N_p . N_q) squared normal_power_log2 times:  S = max(sum wn, 1e-6), S1 = (sum wn * l_q) / S,
 *                      S2 = (sum wn * (l_q * l_q)) / S, v = max(S2 - S1 * S1, 0)
 *   Pass i = 0 .. passes - 1, hole s = 2^i, on (c, v) of the pass before, l = lum(c):
 *     g = sum over the dense 3 x 3 neighbours of b * v_q, b = (1/4, 1/2, 1/4) x (1/4, 1/2, 1/4);  sd = sigma_l * sqrt(g) + 1e-6
 *     for (dx, dy) in [-2, 2]^2: q = p + s * (dx, dy), h = k[|dx|] * k[|dy|], k = (3/8, 1/4, 1/16); the centre tap has w = 9/64, every other tap
 *       w = h * wn * exp(-((e_z + e_a) + e_l)),  e_l = |l_q - l_p| / sd,  e_a = |A_q - A_p|^2 / (sigma_a * sigma_a),
 *       e_z = |N_p . (P_q - P_p)| / (sigma_z * 0.01 * max(Z_p, 1e-3) * s * sqrt(dx * dx + dy * dy) + 1e-6), or 0 without position
 *     c' = (sum w * c_q) / (sum w),  v' = (sum (w * w) * v_q) / ((sum w) * (sum w))
 *   Output: (c * a', 1) after the last pass; 2 * width x 2 * height by pixel replication when upscale2x.
 * A pixel whose normal is 0 (a miss) takes no neighbour and keeps its beauty up to the rounding of the demodulation; no other pixel takes from it either. */
typedef struct fh_denoise_inputs { /* device pointers, width * height elements each */
  const float* beauty;    /* float4, required */
  const float* normal;    /* float4, required */
  const float* albedo;    /* float4, required */
  const float* position;  /* float4, or NULL */
  const float* depth;     /* float, or NULL; position and depth are given together or not at all */
  const float* moments;   /* float2 (m1, m2) as fh_get_luminance_moments fills it, or NULL */
  const uint32_t* counts; /* as fh_get_sample_counts fills it; given together with moments or not at all */
} fh_denoise_inputs;
typedef struct fh_denoise_params {
  float sigma_l, sigma_z, sigma_a;
  uint32_t normal_power_log2, passes;
} fh_denoise_params;
/* params == NULL: sigma_l 2, sigma_z 1, sigma_a 0.2, normal_power_log2 7, passes 5.  FH_E_INVALID, decided from the arguments alone before anything is touched,
 * for a sigma that is not finite or <= 0, normal_power_log2 > 10, passes outside 1..6, a missing required pointer, or half a pair.  Asynchronous on the
 * context stream like fh_denoise; on a group it runs on the lead.  The scratch images live in the context and grow on demand. */
int fh_denoise_guided(fh_ctx* ctx, uint32_t width, uint32_t height, const fh_denoise_inputs* inputs, const fh_denoise_params* params, float* denoised, int upscale2x);

/* -- temporal accumulation in front of the variance-guided denoiser (opt-in; fh_denoise and fh_denoise_guided keep their bits): the reprojection and accumulation
 * stage of SVGF.  fh_denoise_temporal is fh_denoise_guided with ONE stage between its preparation and its passes, which blends (c, v) of the frame with the
 * context's history of the frames before it, found again through the world position (this call knows no motion vectors -- fh_denoise_temporal_motion and fh_set_denoise_motion below add them --: a surface that moved fails the plane stop at its
 * old place and gets no history).  `camera` is the camera the layers were rendered with; position and depth are required; moments and counts stay optional.
 * The context owns the history (on the lead of a group), double buffered: per pixel (c_acc.rgb, v_acc), (P, h) and N, and the camera of the call that wrote it.
 * A change of width x height, fh_denoise_history_reset and fh_ctx_destroy drop it; fh_set_resolution does not.  The first call after that gives fh_denoise_guided's bits.
 *
 * The stage, per pixel p, in fp32 without contraction, / correctly rounded, sums in the order written; c, v: the preparation's values; N, P, Z: the inputs at p;
 * primed values: the history; X != 0 for a normal: any of its three components is non-zero.
 *   N_p = 0 (a miss):      c_acc = c, v_acc = v, h = 0.
 *   no history (below):    c_acc = c, v_acc = v, h = 1.
 *   with history c_h, v_h, h_h:  h = min(h_h + 1, max_history),  a = max(1 / h, alpha_min),  b = 1 - a,
 *                          c_acc = b * c_h + a * c,   v_acc = (b * b) * v_h + (a * a) * v   (the variance of that combination of independent frames; a = 1 gives c, v exactly)
 *   The passes run on (c_acc, v_acc); the history keeps (c_acc, v_acc), (P_p, h), N_p: values from BEFORE the spatial filter, whose bias must not feed back.
 *   A tap q of the history is VALID when it lies inside the frame, N'_q != 0, (N_p.x * N'_q.x + N_p.y * N'_q.y) + N_p.z * N'_q.z >= normal_cos_min, and, with
 *   d = P'_q - P_p,  |(N_p.x * d.x + N_p.y * d.y) + N_p.z * d.z| <= plane_tol * max(Z_p, 1e-3).
 *   Still camera (all 15 floats of `camera` have the stored camera's bits): the only tap is p itself; valid: c_h, v_h, h_h are its values unchanged; else no history.
 *   Moved camera: with M' the stored camera's world-to-camera rows and f' = 1 / tanf(0.5 * fov') of it (fp32, as fh_render computes it):
 *     Q.i = ((M'[4i] * P.x + M'[4i+1] * P.y) + M'[4i+2] * P.z) + M'[4i+3];   t = (f' - Q.z) / f';   no history unless t > 0;
 *     x = (W + (H * Q.x) / t) * 0.5,  y = (H - (H * Q.y) / t) * 0.5   (W, H: width, height as floats; the inverse of the chief ray of pixel (x, y), pixel centres at + 0.5);
 *     xs = x - 0.5, ix = floor(xs), fx = xs - ix, likewise ys, iy, fy; taps (ix + i, iy + j) for j = 0, 1 (outer), i = 0, 1 (inner) with weights
 *     (i ? fx : 1 - fx) * (j ? fy : 1 - fy); over the valid taps in that order S = sum w, then c_h = (sum w * c'_q) / S, v_h = (sum w * v'_q) / S,
 *     h_h = (sum w * h'_q) / S; no history unless S >= 1e-3.
 *   M' is computed on the host, in double, and rounded once to float: with R the 3 x 3 of camera.transform (R[i][j] = transform[4i + j]) and T its fourth column,
 *     C00 = R11 R22 - R12 R21, C01 = R02 R21 - R01 R22, C02 = R01 R12 - R02 R11,   C10 = R12 R20 - R10 R22, C11 = R00 R22 - R02 R20, C12 = R02 R10 - R00 R12,
 *     C20 = R10 R21 - R11 R20, C21 = R01 R20 - R00 R21, C22 = R00 R11 - R01 R10,   det = (R00 C00 + R01 C10) + R02 C20,
 *     M'[4i + j] = Cij / det,   M'[4i + 3] = -(((Ci0 / det) * T0 + (Ci1 / det) * T1) + (Ci2 / det) * T2).
 * Defaults (temporal == NULL): alpha_min 0.2, max_history 32, normal_cos_min 0.5, plane_tol 0.02 -- chosen by the float64 replay of DESIGN.md 4a.  The normal layer
 * is the mean of the samples' normals, shorter than 1 wherever a pixel straddles an edge, so the usual 0.9 refuses a history to one hit pixel in eight, frame after
 * frame, on a still camera too; 0.5 still separates walls that meet at a right angle. */
typedef struct fh_temporal_params {
  float alpha_min;      /* lower bound of the blend weight of the new frame, in [0, 1] */
  float max_history;    /* cap of the history length, >= 1 */
  float normal_cos_min; /* a history tap is valid only if N_p . N'_q >= this, in (-1, 1] */
  float plane_tol;      /* ... and |N_p . (P'_q - P_p)| <= plane_tol * max(Z_p, 1e-3), > 0 */
} fh_temporal_params;
/* FH_E_INVALID, decided from the arguments alone before anything is touched (a refused call leaves history and output alone): a null camera; a camera whose
 * transform cannot be inverted (det is 0 or not finite) or whose 1 / tanf(0.5 * fov) is not finite and > 0; missing position or depth; a temporal parameter that
 * is not finite or outside its range; and everything fh_denoise_guided refuses.  Asynchronous on the context stream. */
int fh_denoise_temporal(fh_ctx* ctx, uint32_t width, uint32_t height, const fh_denoise_inputs* inputs, const fh_camera* camera, const fh_temporal_params* temporal,
                        const fh_denoise_params* params, float* denoised, int upscale2x);
int fh_denoise_history_reset(fh_ctx* ctx);
/* width and height of the history and the frames accumulated since the last reset (0, 0, 0 when there is none); any pointer may be NULL */
int fh_denoise_history_info(fh_ctx* ctx, uint32_t* width, uint32_t* height, uint32_t* frames);

/* -- per-instance motion vectors for the temporal stage (opt-in; every call above keeps its bits).  Motion here is rigid or affine PER INSTANCE
 * (fh_set_transforms), so where a pixel's surface was in the frame before is one affine map of the position layer, chosen by the instance the pixel sees.
 *
 * fh_primary_instances: per pixel of a width x height frame the instance id of the face the pixel's CHIEF RAY hits first, or 0xffffffff for a miss.  `ids` is a
 * device pointer to width * height words; asynchronous on the context stream; on a group it runs on the lead.  Needs a scene and a built BVH.
 *   The chief ray of pixel (px, py) is fh_render's camera ray at the pixel centre through the lens centre, in fp32 without contraction, sums in the order written:
 *     f = 1 / tanf(0.5 * fov);  a = 1 / ((1 + f) - 1 / focus);  ux = -((2 * (px + 0.5) - W) / H),  uy = (2 * (py + 0.5) - H) / H;
 *     s = normalize((0, 0, f) - (ux, uy, 0));  o = (ux, uy, 0) + ((a + focus) / s.z) * s;  d = normalize(o - (0, 0, f));  d.z = -d.z;
 *     origin = T * (0, 0, f, 1),  direction = T * (d, 0)   (T = camera.transform; normalize(v) = v * (1 / sqrt(v . v)); row . vector as ((r0 x + r1 y) + r2 z) + r3 w)
 *   -- the ray whose inverse the temporal stage above states.  It is traced to 1e9 for its closest hit (smaller t, then lower face id), with the any-hit rule for
 *   cut-outs that fh_render's primary rays follow. */
int fh_primary_instances(fh_ctx* ctx, const fh_camera* camera, uint32_t width, uint32_t height, uint32_t* ids);
/* where instance i's surface points and normals were: P' = point * (P, 1) (3 x 4, row major), N' = normal * N (3 x 3, row major) */
typedef struct fh_motion {
  float point[12];
  float normal[9];
  uint32_t moved; /* 0: all 24 floats of the instance's previous and current matrices have the same bits; the maps are then never applied */
} fh_motion;
/* Host only, no context, no GPU.  All four arrays hold n 3 x 4 row-major matrices (12 floats each) as fh_set_transforms takes them.  With L(M) the 3 x 3 of M:
 *   point  = o2w_prev * w2o_cur   as affine maps: point[4i + j] = (A[4i] * B[j] + A[4i+1] * B[4+j]) + A[4i+2] * B[8+j]  (+ A[4i+3] for j = 3), A = o2w_prev, B = w2o_cur;
 *   normal = (L(o2w_cur) * L(w2o_prev))^T: normal[3i + j] = (C[4j] * D[i] + C[4j+1] * D[4+i]) + C[4j+2] * D[8+i], C = o2w_cur, D = w2o_prev
 *            -- the inverse transpose of point's linear part when the w2o are the inverses of the o2w.
 * Both products are formed in double from the caller's floats and rounded once.  Normals are NOT renormalised: the normal layer is a mean of sample normals and not
 * of unit length anyway; under non-uniform scale the carried normal's length changes, so the normal stop (a bound on N_b . N'_q) is approximate there.
 * FH_E_INVALID for n > 0 with a null pointer. */
int fh_motion_from_transforms(uint32_t n, const float* o2w_prev, const float* w2o_prev, const float* o2w_cur, const float* w2o_cur, fh_motion* out);
/* fh_denoise_temporal with motion: instance_ids is a device pointer (width * height words, as fh_primary_instances writes them), motion a host array of n_instances
 * entries, read during the call (it goes to a context-owned device buffer that grows on demand).  The stage above with these changes, per hit pixel p, i = ids[p]:
 *   p is CARRIED when i < n_instances and motion[i].moved.  Then, with A = motion[i].point, G = motion[i].normal:
 *     Pb.k = ((A[4k] * P.x + A[4k+1] * P.y) + A[4k+2] * P.z) + A[4k+3],   Nb.k = (G[3k] * N.x + G[3k+1] * N.y) + G[3k+2] * N.z;   otherwise Pb = P, Nb = N, with their bits.
 *   Not carried and a still camera: the pixel's own tap with weight 1 (the still-camera rule above).
 *   Every other case (also a carried pixel under a still camera): Pb is projected with the stored camera's M' and f' as above, and the 2 x 2 taps are valid by the
 *     two stops with (Nb, Pb) in place of (N_p, P_p) and the limit plane_tol * max(Z_p, 1e-3); renormalised; no history unless S >= 1e-3.
 *   The blend is unchanged, and the history written is (c_acc, v_acc), (P_p, h), N_p: in the CURRENT frame's world space.
 * When no entry has `moved` set (and when instance_ids, motion are NULL and n_instances is 0) the call is fh_denoise_temporal launch for launch and bit for bit, and
 * the id plane is never read.  FH_E_INVALID, from the arguments alone, leaving history and output alone: ids without motion or motion without ids; n_instances 0
 * with either given; a motion entry with a non-finite float; everything fh_denoise_temporal refuses.
 * Not covered: motion that is not one affine map per instance (morph targets, which the glTF reader does not load; vertices moved by fh_set_joint_matrices: a skinned
 * instance whose matrix did not change counts as unmoved and the two stops decide whether its pixels keep a history); the id is the chief ray's, so a pixel most of whose samples see another instance
 * is carried with the wrong map and the two stops decide whether it keeps a history; the lighting change a moving light or occluder causes lags unless
 * fh_set_denoise_response (below) is on, which shortens the lag and does not remove it. */
int fh_denoise_temporal_motion(fh_ctx* ctx, uint32_t width, uint32_t height, const fh_denoise_inputs* inputs, const fh_camera* camera, const fh_temporal_params* temporal,
                               const fh_denoise_params* params, const uint32_t* instance_ids, uint32_t n_instances, const fh_motion* motion, float* denoised, int upscale2x);
/* The context does the bookkeeping (default off; on a group the switch is broadcast and the work runs on the lead).  While on, every fh_denoise_temporal call keeps,
 * on the host, a snapshot of the context's instance matrices with the history it writes.  If a snapshot exists, the history is alive, the instance count is the
 * snapshot's and any instance's matrices differ from it in bits, the call runs fh_primary_instances, fh_motion_from_transforms (previous: the snapshot, current: the
 * context's) and fh_denoise_temporal_motion itself -- it then needs a built BVH (FH_E_INVALID otherwise, nothing touched); in every other case (the first call, after
 * fh_denoise_history_reset, after fh_scene_upload, nothing moved) it is today's call launch for launch.  CONTRACT: the layers were rendered with the context's
 * current transforms.  Switching off drops the snapshot. */
int fh_set_denoise_motion(fh_ctx* ctx, int on);
int fh_get_denoise_motion(fh_ctx* ctx, int* on);

/* -- history clipping for the temporal stage (opt-in, default off; with it off every call above keeps its bits and its launches).  Nothing in the layers tells the
 * stage that the radiance of an unmoved surface changed: a history that passes the two stops is blended with weight 1 - alpha_min however wrong its colour has become,
 * so a moving light or occluder lags by 1 / alpha_min frames.  While this switch is on, fh_denoise_temporal and fh_denoise_temporal_motion (also the calls
 * fh_set_denoise_motion makes itself) clamp the history colour, before the blend, to the box mean +- gamma * standard deviation of the CURRENT frame's colour in a
 * fixed 5 x 5 window (the variance clipping of temporal anti-aliasing), and shorten the history by how far outside the box it lay.
 * A call without a history -- the first, after a reset, after a change of size -- is unchanged: fh_denoise_guided's bits.
 *
 * The changes to the stage, for a hit pixel p that HAS a history, after (c_h, v_h, h_h) are found exactly as above (the own tap, the 2 x 2 look-up or the carried
 * look-up); fp32 without contraction, / and sqrt correctly rounded, sums in the order written; c: the preparation's colour of the current frame.
 *   1 Window: for dy = -2 .. 2 (outer), dx = -2 .. 2 (inner), q = p + (dx, dy).  q COUNTS when it lies inside the frame (taps outside are skipped, not clamped),
 *     N_q != 0 and (N_p.x * N_q.x + N_p.y * N_q.y) + N_p.z * N_q.z >= normal_cos_min; the centre always counts (a mean normal can be shorter than
 *     sqrt(normal_cos_min)).  n = the count, as a float; per channel k: S1_k = sum c_q.k, S2_k = sum c_q.k * c_q.k over the counting taps in that order.
 *   2 Box: mu_k = S1_k / n,  var_k = fmax(S2_k / n - mu_k * mu_k, 0),  sd_k = sqrt(var_k),  lo_k = mu_k - gamma * sd_k,  hi_k = mu_k + gamma * sd_k.
 *   3 Too few taps: n < 2: cc = c_h, u = 0.
 *   4 Clip: otherwise cc_k = fmin(fmax(c_h.k, lo_k), hi_k),  u_k = |cc_k - c_h.k| / (gamma * sd_k + 1e-6),  u = fmax(fmax(u_r, u_g), u_b).
 *   5 Shortened history: k1 = 1 + u,  h_h' = h_h / k1,  v_h' = v_h * k1 (u = 0 gives both with their bits).  The blend is the one above with (cc, v_h', h_h') in
 *     place of (c_h, v_h, h_h).  What the history stores and what the passes read are as above.
 *   6 fmax and fmin are C's: a NaN operand loses (numpy's maximum / minimum return it instead).  finite() bounds the beauty, not c * c: for |c_q.k| above
 *     1.8e19 the square is + infinity and so is S2_k.  While mu_k * mu_k is finite, var_k = sd_k = + infinity, the box is (-inf, +inf), cc_k = c_h.k and
 *     u_k = 0 / inf = 0: such a window does not clip channel k.  When mu_k * mu_k overflows as well, inf - inf is NaN, fmax drops it, var_k = 0 and the box is
 *     the point mu_k: cc_k = mu_k, u is of the order 1e6 * |mu_k - c_h.k|, h_h' rounds to 0, so h = 1, a = 1, b = 0 and every pixel whose window counts that tap
 *     drops its history: c_acc = 0 * mu_k + c = c and v_acc = 0 * (v_h * k1) + v = v, both with their bits, as long as mu_k and v_h * k1 are finite.  They are not
 *     always: v_h * k1 overflows once u exceeds about 3e38 / v_h (a tap above about 1e32 / v_h), and then v_acc = 0 * inf = NaN; and a tap that is + infinity itself
 *     (finite() passes a beauty of 3e38, which the division by an albedo of 0.01 takes past FLT_MAX) gives mu_k = cc_k = + infinity and c_acc.k = 0 * inf = NaN.
 *     In both cases ALL pixels whose window counts the tap (up to 25) get the NaN, where the plain stage has a non-finite value in that one pixel only; the
 *     passes keep it out of no neighbour.  Not guarded: a frame with radiance above 1e30 is not one this filter is for.
 * Not covered by these six steps alone: where the window straddles an emitter and what surrounds it, its standard deviation is large, the box loose, and a moved
 * emitter still lags; fh_set_denoise_response_noise (below) closes most of that where the call has moments, and without moments it stays open (DESIGN.md 4a gives the
 * figures of both).  Window radius is not a parameter. */
typedef struct fh_response_params {
  float gamma; /* half-width of the clip box in standard deviations, finite and > 0; default 1 */
} fh_response_params;
/* params == NULL: off.  The switch lives on the context like fh_set_denoise_motion: broadcast on a group, the work runs on the lead.  FH_E_INVALID, decided from the
 * arguments alone, for a gamma that is not finite or <= 0; the switch then stays as it was.  Takes effect with the next call; the history is kept. */
int fh_set_denoise_response(fh_ctx* ctx, const fh_response_params* params);
/* *on = 0 or 1; params (may be NULL) receives the gamma last set (1 before any) */
int fh_get_denoise_response(fh_ctx* ctx, int* on, fh_response_params* params);

/* -- the noise box: one more step of the clipped stage (opt-in, default off).  The 5 x 5 box above is loose exactly where a window straddles an emitter and its
 * surroundings; the pixel's own MEASURED noise is not: a history consistent with the current frame lies within a few standard deviations of the pixel's colour, the
 * variance being the preparation's v (from the luminance moments) plus the history's v_h.  The step runs only when fh_set_denoise_response is on, this switch is on AND
 * the call has moments and counts; in every other call -- the response switch off, no moments -- the switch is stored and inert, and the call has the bits and the
 * launches it has without it.  (Without moments v is the 7 x 7 spatial estimate, which is large at those same edges: the step would gain nothing and cost the steady
 * state; it is not emulated.)  For a hit pixel p that has a history, fp32 without contraction, / and sqrt correctly rounded, sums in the order written:
 *   4b Noise box, after step 4 has produced cc and u (call that u_s; step 3's "too few taps" gives cc = c_h, u_s = 0, and this step still runs):
 *      s = kappa * sqrt(v + v_h),  v the preparation's variance at p, v_h the history variance as looked up (before step 5 scales it);
 *      per channel k: cd_k = fmin(fmax(cc_k, c.k - s), c.k + s),  w_k = |cd_k - cc_k| / (s + 1e-6);
 *      u = fmax(u_s, fmax(fmax(w_r, w_g), w_b)).
 *   5  then uses (cd, u) in place of (cc, u).
 *   The half-width s is the standard deviation of the LUMINANCE, used for all three channels of the demodulated colour: no per-channel scaling.
 *   6b fmax and fmin are C's.  A NaN s (a NaN v or v_h; kappa * sqrt cannot make one from finite operands) loses in both clamps, so cd = cc, and w_k = 0 / NaN = NaN
 *      loses in the fmax: u = u_s, the six steps' result.  An infinite s clips nothing: the box is (-inf, +inf), w_k = 0 / inf = 0 -- this is what v + v_h gives when
 *      it overflows (both are >= 0 or NaN, so the sum is never inf - inf), what an infinite v or v_h gives, and what kappa * sqrt(v + v_h) gives when the product
 *      overflows.  With c.k itself infinite and s infinite one bound is NaN and loses: still nothing is clipped.  s = 0 (v = v_h = 0: a pixel whose samples all
 *      agreed, in both) makes the box the point c: cd = c, and w_k = |c.k - cc_k| * 1e6 drops the history unless it equals the frame.  A NaN cc_k (a NaN history)
 *      loses against the lower bound and becomes c.k - s, with w_k = NaN, which loses. */
typedef struct fh_response_noise_params {
  float kappa; /* half-width of the noise box in standard deviations, finite and > 0; default 6 */
} fh_response_noise_params;
/* params == NULL: off.  Lives on the context and is broadcast on a group like fh_set_denoise_response; the work runs on the lead.  FH_E_INVALID, decided from the
 * arguments alone, for a kappa that is not finite or <= 0; the switch then stays as it was.  Takes effect with the next call; the history is kept. */
int fh_set_denoise_response_noise(fh_ctx* ctx, const fh_response_noise_params* params);
/* *on = 0 or 1; params (may be NULL) receives the kappa last set (6 before any) */
int fh_get_denoise_response_noise(fh_ctx* ctx, int* on, fh_response_noise_params* params);

/* -- temporal moments: the variance of a call WITHOUT luminance moments, from a history of moments (opt-in, default off; with it off every call above keeps its
 * bits, its launches and its memory).  The colour edge stop of the passes is steered by the per-pixel variance v.  Without sample moments and counts v is the 7 x 7
 * spatial estimate, which is large exactly at the edges the filter should keep; and at 1 sample per call sample moments cannot exist (n < 2 gives v = l * l).  While
 * this switch is on, EVERY fh_denoise_temporal and fh_denoise_temporal_motion call (also the calls fh_set_denoise_motion makes itself, and with or without sample
 * moments) keeps the first and second moment of the luminance, (mu1, mu2), in one more double-buffered history image of two floats per pixel, integrated through the
 * same look-up and with the same weights as the colour (SVGF's temporal variance); a call without sample moments takes its v from them once the pixel's history is
 * min_history long, and from the spatial estimate before that.
 *
 * The changes to the stage; fp32 without contraction, / correctly rounded, sums in the order written; c: the preparation's colour of the current frame:
 *   l = lum(c) = (c.r * 0.2126729 + c.g * 0.7151522) + c.b * 0.0721750, the preparation's luminance, for every pixel (a miss too).
 *   A pixel without a history -- a miss, the first call, a look-up that failed the stops -- stores mu_acc = (l, l * l).
 *   A pixel WITH a history finds mu_h exactly as it finds (c_h, v_h, h_h): the own tap gives the stored (mu1, mu2) with their bits; the 2 x 2 look-up sums
 *     wgt * mu'_q.k over the same valid taps in the same order and divides by the same S, per component k; a carried pixel of the motion form is looked up from where
 *     it is carried to.  The moments are NOT clipped: steps 1 to 5 of fh_set_denoise_response, where on, change (c_h, v_h, h_h) and leave mu_h alone.
 *   After those steps h = min(h_h + 1, max_history), a = max(1 / h, alpha_min), b = 1 - a as above, and mu_acc.k = b * mu_h.k + a * m.k with m = (l, l * l).
 *   Only in a call WITHOUT moments and counts: if the pixel has a history and h >= min_history, v := fmax(mu_acc.y - mu_acc.x * mu_acc.x, 0) takes the place of the
 *     preparation's v in v_acc = (b * b) * v_h + (a * a) * v; otherwise v stays the 7 x 7 estimate.  h is the length after the clip: a history that the clip shortened
 *     below min_history falls back on the spatial estimate.  fmax is C's: a NaN difference gives 0.
 *   In a call WITH moments and counts v is untouched: the output has the bits it has with the switch off (the moments are still kept), and step 4b, whose condition
 *     stays "the call has moments and counts", behaves as it does today.  This switch never enables step 4b.
 *   The history stores mu_acc next to (c_acc, v_acc), (P_p, h), N_p.  Nothing else changes: the preparation, the 7 x 7 estimate (the fallback needs it) and the passes
 *   are launched as they are.
 * Not covered: after a moved emitter a sharper variance blurs the lagging history less, and the call is worse than with the spatial estimate until the history has
 * caught up (DESIGN.md 4a gives the figures); the noise box is not fed from these moments (measured: it ruins the steady state or never binds). */
typedef struct fh_temporal_moments_params {
  float min_history; /* the history length from which the temporal variance replaces the spatial estimate, finite and >= 1; default 2 */
} fh_temporal_moments_params;
/* params == NULL: off.  Lives on the context and is broadcast on a group like fh_set_denoise_response; the work runs on the lead.  FH_E_INVALID, decided from the
 * arguments alone before the context is touched, for a min_history that is not finite or < 1 (any finite value >= 1 is accepted); the switch, the history and the next
 * output then stay as they were.  A successful call that turns the switch from off to on or from on to off drops the history exactly as fh_denoise_history_reset does
 * (the next call is fh_denoise_guided's bits); one that only changes min_history keeps it.  The moment images are allocated by the first call with the switch on,
 * grow and are freed with the rest of the history, and are freed when the switch goes off. */
int fh_set_denoise_temporal_moments(fh_ctx* ctx, const fh_temporal_moments_params* params);
/* *on = 0 or 1; params (may be NULL) receives the min_history last set (the default before any) */
int fh_get_denoise_temporal_moments(fh_ctx* ctx, int* on, fh_temporal_moments_params* params);

/* -- auto-exposure of the post chain: histogram metering and adaptation (opt-in, default off; with it off fh_post_process keeps its bits and its launches).
 * fh_post_params stays as it is: the feature is a switch on the context.  While it is on, every fh_post_process call first meters its input (fh_meter_exposure), and
 * its tone map multiplies by exposure = fhe_pow(2, ev) of the context's state in place of the exposure ISO gives; until a frame has been metered (frames == 0: an
 * input with no pixel of positive luminance) the ISO exposure is used.  Everything is queued on the context stream: no host synchronisation.
 * All of it is fp32 without contraction, / correctly rounded, sums in the order written, unless noted; finite() and lum() are fh_denoise_inputs' (above);
 * fhe_log2, fhe_exp, fhe_pow: include/fh_elementary.h.  On the host: scale = 256.0f / (log2_hi - log2_lo), log2key = fhe_log2(key),
 * a_up = 1 - fhe_exp(-frame_time * speed_up), a_down likewise with speed_down; both are exactly 1 for an infinite frame_time.
 *   Metering, over ALL width * height pixels of the input (not the floor-division grid of the tone map: the metering describes the scene):
 *     l = lum(finite(r), finite(g), finite(b)).  The pixel is UNMETERED when !(l > 0) and counts in word [256]; otherwise it counts in
 *     bin = clamp((int)floorf((fhe_log2(l) - log2_lo) * scale), 0, 255)  (the clamp is applied to the float, so every finite log2_lo is defined).
 *     The counts are integers: the histogram does not depend on the order the pixels are visited in.
 *   Resolve, once per metering call:
 *     N = sum of hist[0 .. 255].  N == 0: the state is left alone, whole.
 *     cut = (uint32)((double)N * (double)low),  end = (uint32)((double)N * (double)high);  if end <= cut: end = min(cut + 1, N), cut = end - 1.
 *     For b = 0 .. 255 in ascending order, c0 the count in the bins before b, h = hist[b]:  kept = max(0, min(c0 + h, end) - max(c0, cut)),
 *       centre_b = ((float)b + 0.5f) / scale + log2_lo,  S += (double)kept * (double)centre_b   (S a double, summed serially; the product and the sum rounded separately).
 *     mean_log2 = (float)(S / (double)(end - cut)).
 *     target = fmaxf(min_ev, fminf((log2key - mean_log2) + compensation_ev, max_ev)).
 *     frames == 0: ev = target.  Otherwise a = target > ev ? a_up : a_down and ev = ev + (target - ev) * a.
 *     target_ev = target, metered = N, unmetered = hist[256], frames += 1.
 *   Chain: the tone map is fh_post_process's with r, g, b multiplied by fhe_pow(2.0f, ev).  With FH_AE_BLOOM_RELATIVE the bloom threshold passes a pixel when
 *     l * exposure > bloom_threshold (l = r * 0.2126729 + g * 0.7151522 + b * 0.0721750 as that kernel computes it), with the ISO exposure while frames == 0;
 *     without the flag the threshold compares scene luminance as it always did.
 * Not covered: metering of tile shards before a gather (the input is a whole frame on one device), spatial (centre-weighted) metering.  Local tone mapping is
 * fh_set_local_exposure's, below. */
#define FH_AE_BLOOM_RELATIVE 1u
typedef struct fh_auto_exposure_params {
  float key;               /* 0.18: the value the metered mean luminance is mapped to */
  float compensation_ev;   /* 0 */
  float min_ev, max_ev;    /* -16, 16: clamp of ev = log2(exposure) */
  float low, high;         /* 0.10, 0.90: share of metered pixels below / up to which ranks are kept */
  float speed_up, speed_down; /* 3, 1 (1/s): rate while the exposure rises / falls */
  float frame_time;        /* 1/30 s per metering call; +inf = no adaptation (ev = target) */
  float log2_lo, log2_hi;  /* -16, 16: range of the 256 bins */
  uint32_t flags;          /* FH_AE_BLOOM_RELATIVE = 1 */
} fh_auto_exposure_params;
typedef struct fh_auto_exposure_state { float ev, target_ev, mean_log2; uint32_t metered, unmetered, frames; } fh_auto_exposure_state;
/* params == NULL: off, and the state is dropped.  A call that turns the switch on starts from frames = 0; one that changes the parameters of a switch that is on keeps
 * the state.  On a group the switch lives on the lead, where fh_post_process runs.  FH_E_INVALID, decided from the arguments alone before the context is looked at and
 * each with its own message: a key that is not finite or <= 0; a non-finite compensation_ev, min_ev, max_ev, log2_lo or log2_hi; min_ev > max_ev;
 * log2_hi - log2_lo not in (0, 64]; low or high outside [0, 1], or low >= high; a speed that is not finite or < 0; a frame_time that is NaN or < 0; unknown flag
 * bits.  A refused call leaves the switch, the parameters and the state alone. */
int fh_set_auto_exposure(fh_ctx* ctx, const fh_auto_exposure_params* params);
/* *on = 0 or 1; params (may be NULL) receives the parameters last set (the defaults above before any) */
int fh_get_auto_exposure(fh_ctx* ctx, int* on, fh_auto_exposure_params* params);
/* frames = 0: the next metered frame sets ev = target.  Asynchronous, on the context stream.  FH_E_INVALID while the switch is off */
int fh_auto_exposure_reset(fh_ctx* ctx);
/* meters image_rgba (a device pointer, width * height float4) and resolves: asynchronous, on the context stream; what fh_post_process runs first while the switch
 * is on.  FH_E_INVALID, from the arguments alone: a null image, width or height 0 or above 32768; and while the switch is off */
int fh_meter_exposure(fh_ctx* ctx, const float* image_rgba, uint32_t width, uint32_t height);
/* synchronising: the state after everything queued so far.  FH_E_INVALID while the switch is off */
int fh_get_auto_exposure_state(fh_ctx* ctx, fh_auto_exposure_state* state);
/* synchronising: the histogram of the last metering call (all zero before any); hist[256] = unmetered pixels.  FH_E_INVALID while the switch is off */
int fh_get_luminance_histogram(fh_ctx* ctx, uint32_t hist[257]);

/* -- local exposure of the post chain: an edge-aware base layer of log-luminance whose contrast is reduced, the detail on top of it left alone (opt-in, default off;
 * with it off fh_post_process keeps its bits, its launches and its kernels).  fh_post_params stays as it is: the feature is a switch on the context.  While it is on,
 * every fh_post_process call first analyses its input (fh_local_exposure_analyse: steps 1 - 3) and its tone map multiplies each output pixel by a gain of its own
 * (steps 4 - 5).  Everything is queued on the context stream: no host synchronisation.
 * All of it is fp32 without contraction, / correctly rounded, sums in the order written and starting from 0.0f unless noted; finite() and lum() are the metering's
 * (above); fhe_log2, fhe_exp, fhe_pow: include/fh_elementary.h; fmaxf / fminf are C's.  On the host: inv_sr = 1.0f / sigma_range, log2pivot = fhe_log2(pivot).
 *   1. Log image, per pixel of the input -- the image handed in as beauty_in, over ALL width * height pixels (not the floor-division grid of the tone map, and not
 *      beauty_temp, whose border is never written):  l = fhe_log2(fmaxf(lum(finite(r), finite(g), finite(b)), 0x1p-24f)).
 *   2. Quarter image, w4 = ceil(w / 4), h4 = ceil(h / 4):  for each in-frame row of the 4 x 4 block (X, Y) its in-frame l are added left to right (the first starts
 *      the sum), the row sums are added top to bottom (likewise), and D0[Y, X] = that sum / (float)(the number of pixels added).
 *   3. Base: `passes` a-trous passes, pass i = 0 .. passes - 1 with hole s = 2^i on the image of the pass before.  For pixel p = (X, Y), with dy = -2 .. 2 the outer
 *      and dx = -2 .. 2 the inner loop:  q = p + s * (dx, dy), each coordinate clamped to the quarter frame;  t = (D_q - D_p) * inv_sr;
 *      wt = (k[|dx|] * k[|dy|]) * fhe_exp(-(t * t)) with k = (3/8, 1/4, 1/16);  num += wt * D_q;  den += wt.  Then D'_p = num / den.
 *   4. Joint upsampling, per output pixel (i, j) with l_p its own value of the log image:  fx = ((float)i + 0.5f) * 0.25f - 0.5f, x0 = floorf(fx), tx = fx - x0, and
 *      the same for fy, y0, ty from j.  The taps (y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1) in this order, each index clamped to the quarter frame, with
 *      wx = 1.0f - tx for x0 and tx for x0 + 1 (wy likewise), Q the base there:  t = (Q - l_p) * inv_sr;  wt = (wy * wx) * fhe_exp(-(t * t));  num += wt * Q;
 *      den += wt.  B = den > 1e-6f ? num / den : l_p.
 *   5. Gain: `exposure` is what the tone map would multiply by -- the ISO exposure, or fhe_pow(2, ev) once a frame has been metered while auto-exposure is on.
 *      d = (B + fhe_log2(exposure)) - log2pivot;  g = -(d > 0 ? highlights : shadows) * d;  g = fmaxf(-max_stops, fminf(g, max_stops));
 *      x = exposure * fhe_pow(2.0f, g).  The tone map is fh_post_process's with r, g, b multiplied by x in place of exposure: chromatic aberration still fetches the
 *      three channels where it did, and the gain is the output pixel's.  Bloom and its threshold are untouched.  highlights = shadows = 0, or max_stops = 0, give
 *      g = +-0, fhe_pow(2, +-0) = 1 and so the bits of the call with the switch off.
 * The defaults are this library's own choice, made from a float64 prototype of the filter: at sigma_range = 1 and 4 passes an edge of 3 stops or more between two
 * noisy plateaus stays in the base (no halo), and 0.3 stops of noise stay out of it.  An edge of less than about 2 sigma_range is smoothed by design.
 * Not covered: analysis of tile shards before a gather (the input is a whole frame on one device), a resolution factor other than 4, per-channel gains, temporal
 * smoothing of the base (every frame is analysed anew), any change to bloom. */
typedef struct fh_local_exposure_params {
  float highlights;   /* 0.5: share of the base layer's distance ABOVE the pivot that is removed; [0, 1] */
  float shadows;      /* 0.5: the same BELOW the pivot; [0, 1] */
  float pivot;        /* 0.18: the exposed luminance that is left alone; finite, > 0 */
  float max_stops;    /* 4: clamp of the per-pixel correction, in stops; finite, >= 0 */
  float sigma_range;  /* 1.0: range sigma of the edge stop, in stops; finite, > 0 */
  uint32_t passes;    /* 4: a-trous passes on the quarter-resolution image; 1..6 */
} fh_local_exposure_params;
/* params == NULL: off.  On a group the switch lives on the lead, where fh_post_process runs.  FH_E_INVALID, decided from the arguments alone before the context is
 * looked at and each with its own message: highlights or shadows outside [0, 1]; a pivot that is not finite or <= 0; a max_stops that is not finite or < 0; a
 * sigma_range that is not finite or <= 0; passes outside 1 .. 6.  A refused call leaves the switch and the parameters alone. */
int fh_set_local_exposure(fh_ctx* ctx, const fh_local_exposure_params* params);
/* *on = 0 or 1; params (may be NULL) receives the parameters last set (the defaults above before any) */
int fh_get_local_exposure(fh_ctx* ctx, int* on, fh_local_exposure_params* params);
/* steps 1 - 3 on image_rgba (a device pointer, width * height float4): asynchronous, on the context stream; what fh_post_process runs first while the switch is
 * on.  FH_E_INVALID, from the arguments alone: a null image, width or height 0 or above 32768; and while the switch is off */
int fh_local_exposure_analyse(fh_ctx* ctx, const float* image_rgba, uint32_t width, uint32_t height);
/* synchronising: *w4 x *h4 and, when base is not NULL, the w4 * h4 floats (row-major) of the quarter-resolution base of the last analysis; 0 x 0 and nothing before
 * any.  FH_E_INVALID for a null w4 or h4, and while the switch is off */
int fh_get_local_exposure_base(fh_ctx* ctx, float* base, uint32_t* w4, uint32_t* h4);

/* -- importance sampling of the environment for sky lighting (opt-in, default off; with it off every render keeps its bits, its launches and its kernels).
 * The sky next-event ray of a shaded hit is drawn cosine-distributed round the shading normal whatever the environment is (pt.cu:796-815: "TODO: implement IBL
 * importance sampling").  While this switch is on it is drawn from a mixture of that cosine lobe (fraction cosine_fraction = B) and a table of the environment's
 * luminance, and the two BSDF-sampled light-ray weights that stand against it use the same density.  Nothing else of a frame changes: the draw is the 2-D draw of the
 * same sampler slot, and every other slot, dimension, kernel and layer is as it is with the switch off.
 * All of it is fp32 without contraction, / and sqrt correctly rounded, sums in the order written; fhe_sincos, fhe_acos, fhe_atan2: include/fh_elementary.h;
 * PI = 3.14159265358979323846f, TWO_PI = 2.0f * PI; fmax / fmin are C's (a NaN operand loses).
 *   The table: W x H = 512 x 256 cells over (phi, theta), cell (i, j) covering u = phi / TWO_PI in [i, i + 1) / 512 and v = theta / PI in [j, j + 1) / 256 --
 *     the mapping of the environment look-up: theta = fhe_acos(clamp(d.y, -1, 1)), phi = fhe_atan2(d.z, d.x), + TWO_PI when negative.
 *   Sub-samples: K = clamp(ceil(ibl_width / 512), 2, 16) with an image loaded, else 2.  For b = 0 .. K - 1 (outer), a = 0 .. K - 1 (inner):
 *     u = ((float)i + ((float)a + 0.5f) / (float)K) / 512,  v = ((float)j + ((float)b + 0.5f) / (float)K) / 256;
 *     (st, ct) = fhe_sincos(v * PI), (sp, cp) = fhe_sincos(u * TWO_PI), d = (st * cp, ct, st * sp);
 *     (r, g, b) = what the context shows along d at sky intensity 1: the image (its bilinear fetch at (phi / TWO_PI, theta / PI) of d), else the Hosek dome;
 *     l = (finite(r) * 0.2126729f + finite(g) * 0.7151522f) + finite(b) * 0.0721750f, finite(x) = 0 for a NaN or |x| > 3e38, else x; with neither image nor dome
 *       l = 1: a constant background weighs every direction alike, whatever its colour, so neither fh_set_sky_intensity nor the background changes the table;
 *     S += fmin(fmax(l, 0), 3e38) * fmax(st, 0)   (serially).   w = fmin(S / (float)(K * K), 3e38).
 *   Quantisation: w_max = the largest w of the table;  q = max(1, (uint32)((w / w_max) * 1048576.0f)), and q = 1 for every cell when w_max == 0.
 *     So a black image, NaN or infinite texels and texels below 2^-20 of the maximum all leave their cells the weight 1, never 0: every direction keeps a positive
 *     probability.  Row sums R_j = sum_i q (32 bits, at most 2^29), total T = sum_j R_j (64 bits): exact, independent of the order of summation.
 *   Stored: q;  cdf_row[j][i] = (float)((double)(q[j][0] + .. + q[j][i - 1]) / (double)R_j), i = 0 .. 512 (first 0, last 1);
 *     cdf_m[j] = (float)((double)(R_0 + .. + R_(j - 1)) / (double)T), j = 0 .. 256;  cell_p[j][i] = (float)((double)q[j][i] / (double)T).
 *   Search: the interval of u in a CDF of n + 1 entries is lo after  lo = 0, hi = n; while (hi - lo > 1) { mid = (lo + hi) >> 1; if (cdf[mid] <= u) lo = mid; else hi = mid; }
 *     and the position inside it is r = fmin((u - cdf[lo]) / (cdf[lo + 1] - cdf[lo]), 0.99999994f).
 *   The draw, from the sky slot's (ux, uy):  ux < B: the cosine branch with ux := ux / B: today's cosine_hemisphere(ux, uy) round the shading normal;
 *     otherwise ux := fmin((ux - B) / (1 - B), 0.99999994f): row j by cdf_m from ux, column i by cdf_row[j] from uy,
 *     v = ((float)j + r_j) / 256, u = ((float)i + r_i) / 512, d as for a sub-sample.  The drawn cell is (i, j).
 *   The density of a world direction d in cell c, for a shading normal n:
 *     st = fmax(sqrt(d.x * d.x + d.z * d.z), 2^-20),  cos = (d.x * n.x + d.y * n.y) + d.z * n.z,
 *     p = (1 - B) * ((cell_p[c] * 131072.0f) / ((2.0f * (PI * PI)) * st)) + B * (fmax(cos, 0) / PI).
 *     The table branch reports p with c = the drawn cell; the cosine branch and the BSDF-sampled rays take c from d: i = (int)((phi / TWO_PI) * 512), j = (int)((theta / PI)
 *     * 256), each held to its range.  This is the true mixture density: the cosine term lives on the upper hemisphere only (the reference's |cos| / pi on both is
 *     not carried into this mode).  A direction drawn from the table maps back to a neighbouring cell in well under 1e-3 of the draws (the position inside a cell is
 *     continuous, and u and v round); the reported density is then the drawn cell's.  Below 2^-24 a probability cannot be hit by a 24-bit draw: a row or cell whose
 *     CDF interval rounds to nothing is never drawn although its density is positive -- the same granularity every fp32 sampler here has.
 *   The three sites of the closest-hit program (pt.cu:817-857, :893-925), T the throughput, f the BSDF value, pdf_b the BSDF's density:
 *     sky ray: (d, p) from the draw; w = p / (p + pdf_b(d)); contribution clamp01(T * w * f * |cos| / p) * environment(d) -- and nothing when d lies at or below the
 *       shading horizon (d in the shading frame has y <= 0): the BSDF evaluation is not meant for there (today's draw never asks it; it answers the upper side's value
 *       with |cos|, which would light a surface through its back), and the ray leaves from the outer side of the surface, which stops it below the geometric horizon anyway.  Nor when T * w * f * |cos| / p has a
 *       NaN or infinite channel -- every hit on the back side of an opaque surface has one (all lobe weights 0, the lobe pmf 0 / 0, the BSDF's density NaN) --: clamp01
 *       would make it 1 (the reference's regularize_weight), and a draw weighed 1 has the expectation integral of p * L, which
 *       depends on the density -- under the table it is the sun's radiance times the sun's share.  The BSDF-sampled rays keep the clamp as it is.
 *     BSDF-sampled light ray, no emitters: pdf_light = p(d) in place of |cos| / pi.
 *     BSDF-sampled light ray, emitters: the secondary-ray kernels finish it with pdf_light = cos' / pi on a miss and T * w * f * cos' / pdf; they are handed
 *       cos' = PI * p(d) and f' = f * |cos| / cos', which makes the miss density p(d) and leaves the product T * w * f * |cos| / pdf in both branches.
 * The table is rebuilt, on the context stream and without a host synchronisation, by the first fh_render after fh_load_ibl, fh_clear_ibl, fh_load_arhosek_sky,
 * fh_clear_arhosek_sky or a call of this function that turns the switch on; a change of cosine_fraction alone keeps it.
 * Not covered: sampling the product of BSDF and environment, a table resolution parameter.  (Sampling area lights by power: fh_set_light_sampling, below.) */
#define FH_ENV_COSINE_FRACTION_DEFAULT 0.5f
typedef struct fh_env_sampling_params {
  float cosine_fraction; /* B: share of sky rays drawn cosine-distributed, in [0, 1); default FH_ENV_COSINE_FRACTION_DEFAULT (DESIGN.md 4 has the rule that chose it) */
} fh_env_sampling_params;
/* params == NULL: off.  A scene call: on a group it reaches every member.  FH_E_INVALID, decided from the arguments alone before the context is looked at, for a
 * cosine_fraction outside [0, 1) or NaN; the switch then stays as it was. */
int fh_set_env_sampling(fh_ctx* ctx, const fh_env_sampling_params* params);
/* *on = 0 or 1; params (may be NULL) receives the fraction last set (the default before any) */
int fh_get_env_sampling(fh_ctx* ctx, int* on, fh_env_sampling_params* params);

/* -- sampling of area lights by power for the area next-event ray (opt-in, default off; with it off every render keeps its bits, its launches and its kernels).
 * The emissive triangle of a shaded hit's area shadow ray is picked uniformly among the scene's n emitters (pt.cu:860-889), and the BSDF-sampled light ray that finds
 * an emitter is weighed against that density, 1 / (n * area).  While this switch is on the pick follows a table of the emitters' power, mixed with the uniform pick
 * (share uniform_fraction = U), and both sites use the pick's probability P: pdf_area = P / area.  Nothing else of a frame changes: the pick is made from the same
 * Sobol' dimension, and every other draw, slot, kernel and layer is as it is with the switch off.  A scene without emitters builds nothing and renders with the
 * plain kernels.
 * All of it is fp32 without contraction, / and sqrt correctly rounded, sums in the order written; fmax / fmin are C's (a NaN operand loses).
 *   Emitter k is the k-th emissive face in face order (f its face, m its material), as the uniform pick numbers them.
 *   area = 0.5f * length(cross(p1 - p0, p2 - p0)) of the world-space corners, the expression of the shadow ray's density.
 *   e = m's emission colour; when m has an emission texture, per channel the serial sum over s = 0 .. 15 of the texture's fetch at the texture coordinate of the
 *     barycentric point (bu, bv)_s, divided by 16.0f.  The points are the centroids of the 16 congruent triangles the face splits into:
 *       s = 0 .. 9:   rows j = 0 .. 3 of 4 - j points i = 0 .. 3 - j (j outer, i inner): bu = (float)(3 i + 1) / 12.0f, bv = (float)(3 j + 1) / 12.0f;
 *       s = 10 .. 15: rows j = 0 .. 2 of 3 - j points i = 0 .. 2 - j:                    bu = (float)(3 i + 2) / 12.0f, bv = (float)(3 j + 2) / 12.0f;
 *     bw = 1.0f - bu - bv and the coordinate is (bw * t0 + bu * t1) + bv * t2 per component, t0, t1, t2 the corners' -- what the shadow ray's sample forms.
 *   l = fmax((finite(e.r) * 0.2126729f + finite(e.g) * 0.7151522f) + finite(e.b) * 0.0721750f, 0), finite(x) = 0 for a NaN or |x| > 3e38, else x.
 *   w = fmin(area * l, 3e38f).  (The `emission` scalar of fh_material is not part of it: the emission the kernels add does not read it.)
 *   Quantisation: w_max = the largest w;  q_k = max(1, (uint32)((w_k / w_max) * 1048576.0f)), and q_k = 1 for every k when w_max == 0.  So black emitters,
 *     zero-area ones, NaN texels and those below 2^-20 of the maximum all keep a positive weight.  T = sum of q_k, 64 bits: exact, independent of the order.
 *   Stored: q[n];  cdf[k] = (float)((double)(q_0 + .. + q_(k - 1)) / (double)T), k = 0 .. n (first 0, last 1);
 *     P_k = (1 - U) * (float)((double)q_k / (double)T) + U / (float)n, kept per FACE: pick_p[f] = P_k for the emitter's face, 0 for a face that does not emit.
 *   The pick, from the draw u1 in [0, 1) of the area dimension:  u1 < U: u = u1 / U and k = min((uint32)(u * n), n - 1), today's pick;
 *     otherwise u = fmin((u1 - U) / (1 - U), 0.99999994f) and k = lo after  lo = 0, hi = n; while (hi - lo > 1) { mid = (lo + hi) >> 1; if (cdf[mid] <= u) lo = mid;
 *     else hi = mid; }.  The reported probability is P_k in both branches: the true mixture.
 *   The two sites: the area shadow ray uses pdf_area = P_k / area in place of 1 / (n * area); the BSDF-sampled light ray whose closest hit is an emitter uses
 *     pdf_area = pick_p[face hit] / area.  r^2 / |cos|, the facing test, the clamp and the order of additions are untouched, and so is what fh_set_env_sampling hands
 *     to that ray while both switches are on.
 *   U guards against a textured emitter whose 16 points misjudge it and against CDF intervals that round to nothing in fp32 among millions of emitters: whatever the
 *     table says, every emitter is picked with at least U / n.
 * The table is rebuilt, on the context stream, by the first fh_render after fh_scene_upload, fh_set_transforms (areas change) or a call of this function that turns
 * the switch on or changes uniform_fraction (everything is rebuilt, not pick_p alone).  The rebuild synchronises with the host only where it has to allocate: after an
 * upload that changed the number of emitters or faces.
 * Where the clamp binds (glossy lobes: T * w * f * |cos| / pdf above 1) the expectation depends on the pick distribution, as it depends on n today.
 * Not covered: a light hierarchy, product sampling with the BSDF.  (A pick that depends on the shaded point: fh_set_light_resampling, below.) */
#define FH_LIGHT_UNIFORM_FRACTION_DEFAULT 0.0625f
typedef struct fh_light_sampling_params {
  float uniform_fraction; /* U: share of picks that stay uniform, in (0, 1]; default FH_LIGHT_UNIFORM_FRACTION_DEFAULT (DESIGN.md 4 has the rule that chose it) */
} fh_light_sampling_params;
/* params == NULL: off.  A scene call: on a group it reaches every member.  FH_E_INVALID, decided from the arguments alone before the context is looked at, for a
 * uniform_fraction outside (0, 1] or NaN; the switch then stays as it was. */
int fh_set_light_sampling(fh_ctx* ctx, const fh_light_sampling_params* params);
/* *on = 0 or 1; params (may be NULL) receives the fraction last set (the default before any) */
int fh_get_light_sampling(fh_ctx* ctx, int* on, fh_light_sampling_params* params);

/* -- resampling of the table's picks by distance and facing (opt-in, default off; acts only while fh_set_light_sampling is on; with it off, or with candidates = 1,
 * every render keeps its bits, today's light-sampling mode included).  The table above knows nothing of the shaded point.  While this switch is on, the area shadow
 * ray draws M candidates from the table and chooses one of them in proportion to a geometric weight G of the emitter seen from the point (resampled importance
 * sampling).  No Sobol' dimension or CMJ slot is added: every other draw of the frame is where it was.
 * All of it is fp32 without contraction, / and sqrt correctly rounded, in the order written; fmax / fmin are C's (a NaN operand loses).
 *   Proxy of emitter i, two float4, built with the table (one more kernel, one thread per emitter, in emitter order) and rebuilt exactly when the table is:
 *     c = ((p0 + p1) + p2) / 3.0f per component, of the world-space corners;
 *     s = (n0 + n1) + n2 of the corners' world-space shading normals, len = sqrt((s.x * s.x + s.y * s.y) + s.z * s.z), m = s / len per component, and m = 0 where len
 *       is 0 or not finite;
 *     a = area, the table's expression.                                        Stored: (c.x, c.y, c.z, a), (m.x, m.y, m.z, 0).
 *   Geometric weight, from the shadow ray's origin so and the hit's shading normal ns (after the maps, turned to the side the ray came from):
 *     v = c - so;  r2 = (v.x * v.x + v.y * v.y) + v.z * v.z;  d = v / sqrt(r2) per component;  dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z;
 *     G = (fmax(dot(ns, d), 0) + 0.0625f) * (fmax(-dot(m, d), 0) + 0.0625f) / (r2 + a), then G = fmin(fmax(G, 1e-30f), 1e30f): a NaN becomes 1e-30f.
 *     The floors 1/16 keep every emitter's weight positive -- the choice may then never exclude an emitter the table can pick -- and a bounds G next to a large
 *     emitter.  The centroid may misjudge a triangle: a long emitter whose near end lights the point, one that faces the point only with part of its normals, one
 *     hidden behind an occluder.  G then prefers the wrong candidate more often than it should; the division below is by the density the choice really had, so this
 *     costs variance, never bias -- as a misjudged weight does under U.
 *   Candidates, from the one draw u1 of the area dimension, M = candidates:  t = u1 * (float)M;  j = min((uint32)t, M - 1);  v = t - (float)j;
 *     u_k = fmin(((float)k + v) / (float)M, 0.99999994f) and i_k = the table's pick from u_k, k = 0 .. M - 1.  Each u_k is uniform on its stratum.
 *   Selection:  S = G_(i_0) + .. + G_(i_(M - 1)), summed serially in k order;  thr = u_sel * S;  the chosen emitter y is the i_k of the smallest k whose running
 *     sum (the same serial sum) exceeds thr, the last i_k if none does.
 *     u_sel = (float)(xxhash32(image_idx, n_spp, dim_area, seed_hash ^ 0x9e3779b9) >> 8) * 2^-24: the pixel, the sample, the Sobol' dimension of the area draw and
 *     the frame's seed hash.  It is not derived from u1: a choice that is a function of the candidates' own draw is not a random choice.
 *   The two densities of the area shadow ray.  The point on y comes from the same CMJ slot as before.  pdf_area = pick_p[face] / area is unchanged and still enters
 *     the MIS weight w;  pdf_area_ris = pdf_area * (G_y / (S / (float)M)) takes its place only in the division of T * w * f * |cos| / pdf.  r^2 / |cos|, the facing
 *     test, the clamp and the order of operations stay.
 *   MIS.  The BSDF-sampled light ray is untouched: both sites weigh with the TABLE's density, which is the same function of the light point on both sides, so the
 *     two weights add to 1 and the sum stays unbiased.  The weights are deliberately those of the table and not of the resampled pick, whose marginal density has
 *     no closed form.
 * Changing candidates alone rebuilds nothing.  Where the clamp binds the expectation depends on M as it depends on the pick distribution.
 * Not covered: a light hierarchy, the BSDF in the target, reuse of picks across pixels or frames, resampled densities in the MIS weights. */
#define FH_LIGHT_CANDIDATES_DEFAULT 4
typedef struct fh_light_resampling_params {
  int candidates; /* M: 1, 2, 4, 8 or 16; default FH_LIGHT_CANDIDATES_DEFAULT (DESIGN.md 4 has the rule that chose it) */
} fh_light_resampling_params;
/* params == NULL: off.  A scene call: on a group it reaches every member.  FH_E_INVALID, decided from the arguments alone before the context is looked at, for
 * candidates outside {1, 2, 4, 8, 16}; the switch then stays as it was. */
int fh_set_light_resampling(fh_ctx* ctx, const fh_light_resampling_params* params);
/* *on = 0 or 1; params (may be NULL) receives the count last set (the default before any) */
int fh_get_light_resampling(fh_ctx* ctx, int* on, fh_light_resampling_params* params);

/* OpenGL interop for display (cwl::CUDAGLBuffer, cwl/include/cwl/buffer.h:88-143): register an OpenGL buffer object, map it and return the
 * device pointer the renderer can write AOVs to; unregister unmaps.  A current OpenGL context is required on the calling thread. */
int fh_gl_register_buffer(fh_ctx* ctx, unsigned int gl_buffer, void** resource, void** device_ptr, uint64_t* bytes);
int fh_gl_unregister_buffer(fh_ctx* ctx, void* resource);

/* -- device memory helpers (stand in for cwl::CUDABuffer, cwl/include/cwl/buffer.h:18-85) */
int fh_malloc(fh_ctx* ctx, uint64_t bytes, void** out);
int fh_free(fh_ctx* ctx, void* ptr);
int fh_memset(fh_ctx* ctx, void* ptr, int value, uint64_t bytes);
int fh_copy_to_device(fh_ctx* ctx, void* dst, const void* src, uint64_t bytes);
int fh_copy_to_host(fh_ctx* ctx, void* dst, const void* src, uint64_t bytes);
/* host-side image decoding for front ends without a decoder of their own (PNG, baseline JPEG, binary PPM/PGM through
 * include/fredholm/image_io.h; stb_image's role in fredholm/src/scene.cpp:7-37).  No context and no GPU needed.  *rgba8 holds
 * width*height*4 bytes, row 0 first (after the optional vertical flip), and is released with fh_image_free.  Returns FH_OK or
 * FH_E_INVALID; the message is available from fh_last_error(NULL). */
int fh_image_load_rgba8(const char* path, int flip_vertically, uint32_t* width, uint32_t* height, uint8_t** rgba8);
void fh_image_free(uint8_t* rgba8);
int fh_copy_on_device(fh_ctx* ctx, void* dst, const void* src, uint64_t bytes); /* asynchronous, ordered on the context stream (cwl::CUDABuffer device-to-device copies) */
void* fh_stream(fh_ctx* ctx); /* hipStream_t of the context */

/* -- batch ray queries over the built BVH (closest hit, or any hit): rays7 = o.xyz d.xyz tmax per ray (host memory); tuv: 3 floats, prim: face id or
 * 0xffffffff (host memory).  The same traversal code the render kernels run; what a caller without a renderer (picking, visibility probes) uses. */
int fh_trace_rays(fh_ctx* ctx, uint32_t n, const float* rays7, int any_hit, float* tuv, uint32_t* prim);
/* what the runtime reports for the streaming traversal kernel the current scene would be traced by (which = 0: closest hit, 1: secondary rays):
 * out[0] = vector registers per lane, out[1] = static LDS bytes per workgroup, out[2] = scratch bytes per lane, out[3] = workgroups per CU the kernel is
 * launched with, out[4] = stack levels it keeps in LDS (the deeper ones spill to global memory), out[5] = stack levels the BVH needs.  Valid after a
 * BVH build; out[3..4] after the first fh_render of the scene (0 before).  Lets a profile be tied to the code object that produced it (bench.py). */
/* which = 2 + c: the shade kernel of shading class c of the uploaded scene (FH_E_INVALID beyond the scene's classes): out[0..2] as above, out[3] = resident workgroups per
 * CU (of 4 waves: = waves per SIMD), out[4] = the lobe mask the kernel is compiled for, out[5] = the lobe mask of the class. */
int fh_kernel_info(fh_ctx* ctx, int which, uint32_t out[6]);
/* measured HBM bandwidth of this GPU (GB/s): a streaming float4 read and a float4 copy (read + written bytes) over `bytes`-sized buffers,
   `iters` launches each.  The "measured HBM roofline" SURVEY.md 8(d) asks for; use buffers well beyond the 256 MiB Infinity Cache. */
int fh_measure_bandwidth(fh_ctx* ctx, uint64_t bytes, uint32_t iters, double* read_gbs, double* copy_gbs);

#ifdef __cplusplus
}
#endif
#endif
