// context.h -- host-side state behind the opaque fh_ctx of include/fredholm_hip.h.
// Plays the role of the reference's Renderer members (fredholm/include/fredholm/renderer.h:739-828):
// scene buffers, acceleration structure, lights, environment state, sample-count buffer, stream.
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <string>
#include <vector>

#include "../../include/fredholm_hip.h"
#include "fh_device.h"
#include "fh_envmap.h"
#include "fh_lights.h"
#include "fh_memory.h"
#include "temporal_host.h"

struct fh_group;  // group.hip

namespace fh { constexpr int kPassSlots = 3; }  // passes of fh_render in flight at most: path pools, pass streams (the main stream and kPassSlots - 1 more), 2 * kPassSlots regions of d_stack_spill

struct fh_ctx {
  // a handle made by fh_ctx_create_group(n > 1) holds nothing but `group` and the lead's device; its members are plain contexts that name it as their `owner`
  fh_group* group = nullptr;
  fh_ctx* owner = nullptr;
  uint32_t member_index = 0;
  int device = 0;
  // the streams come first: members are destroyed in reverse order, so whatever may be in flight on a stream is released before the stream itself
  fh::Stream stream;   // main stream: everything the caller can observe is ordered on it
  fh::Stream aux_stream[fh::kPassSlots - 1];  // passes j % n_slots != 0 of fh_render run here, overlapping the latency-bound ends of the passes before
  fh::Stream sky_stream;
  std::string err;
  uint32_t flags = 0;

  // constant tables
  fh::DeviceBuffer<uint32_t> d_sobol;
  fh::DeviceBuffer<uint32_t> d_sobol_bytes;  // [1024 dims][4 index bytes][256]: byte-indexed generator matrices (capi.hip: fh_ctx_create)
  fh::DeviceBuffer<float> d_lut_refl;
  fh::DeviceBuffer<float> d_lut_sheen;

  // host copy of the flat scene (transforms can change: Renderer::set_time)
  std::vector<float> h_vertices, h_normals, h_texcoords;
  std::vector<uint32_t> h_indices, h_material_ids, h_instance_ids;
  std::vector<fh_material> h_materials;
  std::vector<float> h_o2w, h_w2o;  // 12 floats per instance
  bool scene_loaded = false, bvh_valid = false;

  // device scene
  fh::DeviceBuffer<float4> d_face_rec;
  fh::DeviceBuffer<uint8_t> d_face_cls;
  fh::DeviceBuffer<fh::MaterialDev> d_materials;
  fh::DeviceBuffer<fh::AreaLightDev> d_lights;
  // object-space geometry resident on the device: the face records above are recomputed from it when the instance transforms change
  fh::DeviceBuffer<float> d_obj_vertices;
  fh::DeviceBuffer<float> d_obj_normals;
  fh::DeviceBuffer<float> d_obj_texcoords;
  fh::DeviceBuffer<uint32_t> d_obj_indices;
  fh::DeviceBuffer<uint2> d_face_meta;  // (material id, instance id) per face
  fh::DeviceBuffer<float4> d_o2w;       // 3 rows per instance
  fh::DeviceBuffer<float4> d_w2o;
  // fh_set_skin / fh_set_joint_matrices (scene.hip: k_skin_vertices, fh_skin.h).  Belongs to the uploaded scene: an upload drops it.  While `posed`, the face
  // records are derived from d_vertices / d_normals (the layout of d_obj_vertices / d_obj_normals) instead of the bind arrays
  struct Skin {
    uint32_t n_joints = 0, n_skinned = 0;  // n_joints = 0: no skin
    bool posed = false;
    std::vector<float> h_palette;          // the matrices held (12 floats per joint); empty until the first fh_set_joint_matrices
    fh::DeviceBuffer<uint2> d_joints;      // four uint16 per vertex
    fh::DeviceBuffer<float4> d_weights;
    fh::DeviceBuffer<float4> d_palette;    // three rows per joint
    fh::DeviceBuffer<float> d_vertices, d_normals;
    // (the caller has made sure nothing still reads the buffers)
    void drop() { n_joints = 0; n_skinned = 0; posed = false; h_palette.clear(); d_joints.reset(); d_weights.reset(); d_palette.reset(); d_vertices.reset(); d_normals.reset(); }
  } skin;
  // textures (renderer.h:372-386): one device blob of texels + descriptors + the sRGB table
  // (which textures can cut, and the opacity classes and micromaps decided from their texels, are the upload's plan: scene_plan_host.h)
  unsigned long long alpha_cell_counts[3] = {0, 0, 0};  // micromap cells of the faces that keep their test; of them: always pass, never pass (fh_alpha_cell_counts)
  uint32_t alpha_face_counts[4] = {0, 0, 0, 0};  // faces whose textures can cut; of them: always pass, never pass, still tested (fh_alpha_face_counts)
  fh::DeviceBuffer<uint4> d_alpha_rec;         // 8 x 16 bytes per face when the scene has cut-outs: what the any-hit test of that face reads (4) and the face's opacity micromap (4) (fh_trace.h: alpha_pass)
  fh::DeviceBuffer<uint8_t> d_texels;
  fh::DeviceBuffer<fht_texture> d_textures;
  fh::DeviceBuffer<float> d_srgb_lut;
  uint32_t n_textures = 0;
  bool has_alpha = false;
  fh::DeviceBuffer<float> d_ibl;
  uint32_t ibl_w = 0, ibl_h = 0;
  uint32_t n_faces = 0, n_lights = 0, n_materials = 0;
  uint32_t n_classes = 0;
  uint32_t class_lobes[fh::kMaxClasses] = {};

  // BVH
  fh::DeviceBuffer<float4> d_bvh2_nodes;
  fh::DeviceBuffer<float4> d_bvh2_tris;
  uint32_t bvh2_n_nodes = 0, bvh2_n_tris = 0;
  fh::DeviceBuffer<uint4> d_bvh8_nodes;
  fh::DeviceBuffer<float4> d_bvh8_tris;
  uint32_t bvh8_n_nodes = 0, bvh8_n_tris = 0;
  fh::DeviceBuffer<uint32_t> d_bvh8_parent;  // per wide node: parent << 3 | child slot in the parent (root: 0xffffffff)
  fh::DeviceBuffer<uint32_t> d_face_node;    // per face: the wide node that holds it (bottom-up start of the rays that leave it, fh_trace.h)
  // kept after a full build so that a change of instance transforms refits the wide tree instead of rebuilding it (bvh_build.hip)
  fh::DeviceBuffer<float4> d_bvh8_box;             // full-precision (lo, hi) of every wide node
  std::vector<uint32_t> bvh8_level_start;   // node index range of every level (levels are contiguous: the collapse is breadth first)
  bool refit_ok = false;                    // topology unchanged since the last full build, no split references
  double bvh8_area_built = 0.0;             // sum of the node areas right after the full build (quality reference for refits)
  uint32_t n_refits = 0;
  uint32_t bvh8_depth = 0;            // node LEVELS of the wide tree; a traversal stack needs levels - 1 entries (fh_trace.h: stack_entries_for), of which the streaming kernels keep the first in LDS
  uint32_t occupancy_key = 0xffffffffu, occupancy_blocks = 0, occupancy_blocks_secondary = 0;  // resident workgroups per CU of the streaming kernels, as the runtime reports them (render.hip)
  uint32_t info_blocks[2] = {0, 0}, info_entries[2] = {0, 0};  // the same two facts for the uninstrumented closest-hit / secondary kernels as last launched (fh_kernel_info)
  uint32_t lds_configured_bytes = 0;  // dynamic-LDS size the traversal kernels were last configured for (render.hip)
  uint32_t stream_lds_entries = 0, stream_lds_entries_secondary = 0;    // stack levels the closest-hit / secondary streaming kernel keeps in LDS (the rest spills to d_stack_spill)
  fh::DeviceBuffer<uint2> d_stack_spill;  // [2 * kPassSlots launches in flight][entry beyond the LDS part][thread of the launch]
  uint32_t lds_static_max = 0;        // largest static LDS of a kernel that keeps its traversal stack in dynamic LDS (hipFuncGetAttributes; render.hip: configure_traversal_lds)
  bool use_bvh8 = false;
  int builder_choice = 0;  // 0 = not decided for this scene, 1 = radix tree (LBVH), 2 = PLOC; decided at the first build after an upload
  double bvh_build_ms = 0.0;
  float scene_lo[3] = {0, 0, 0}, scene_hi[3] = {0, 0, 0};  // padded world bounds of the geometry

  // frame state
  uint32_t width = 0, height = 0;
  fh::DeviceBuffer<uint32_t> d_sample_count;   // samples accumulated per pixel (written by k_accumulate)
  fh::DeviceBuffer<uint32_t> d_sample_issued;  // samples started per pixel (written after k_generate): the next pass does not wait for the accumulate
  uint32_t shard_rank = 0, shard_world = 1, tile_w = 32, tile_h = 32;
  fh::DeviceBuffer<uint32_t> d_owned;  // image indices of owned pixels, in tile order
  fh::DeviceBuffer<uint32_t> d_owned_xy;  // the same pixels as x | y << 16
  uint32_t n_owned = 0;
  // pixels that cannot see the scene (render.hip: k_split_pixels / k_sky_pixels): [0] / [1] image indices and x | y << 16 of the pixels the passes render, [2] / [3] of the sky pixels
  // k_sky_pixels renders, [4] / [5] of the dark sky pixels (k_dark_pixels; none unless the split was made under dark_sky_verdict, which is part of the key)
  fh::DeviceBuffer<uint32_t> d_split[6];
  uint32_t n_wave_px = 0, n_sky_px = 0, n_dark_px = 0;
  fh::DeviceBuffer<uint32_t> d_split_counters;  // wave pixels, sky pixels, bounds-test violations seen by k_sky_pixels, k_sky_pixels' cursor over the groups of its list, dark sky pixels
  bool split_valid = false;
  float split_key[32] = {};              // camera, scene bounds, resolution and ownership the lists were made for
  fh::Event ev_sky;
  fh::Event ev_sky_cursor;  // the cursor has been cleared on the main stream: the filler launch on the sky stream follows it
  struct ShardList { uint32_t rank, world, width, height, tile_w, tile_h; fh::DeviceBuffer<uint32_t> d_owned; uint32_t n_owned; };
  // fh_unpack_shards: the ownership lists of all ranks of a split one after the other (a permutation of the frame) and where each rank's begins
  struct FrameMap { uint32_t world = 0, width = 0, height = 0, tile_w = 0, tile_h = 0; fh::DeviceBuffer<uint32_t> d_all; std::vector<uint32_t> start; };
  FrameMap frame_map;
  std::vector<ShardList> shard_lists;  // ownership lists of other ranks' shards, built on first use by fh_unpack_shard and kept (freed with the context)
  // adaptive sampling (fh_set_adaptive_sampling; render.hip: k_adaptive_select and the round loop of render_submit)
  bool adaptive = false;
  fh_adaptive_params adapt{};
  fh::DeviceBuffer<float2> d_moments;         // (m1, m2) per pixel of the frame, cleared by fh_init_render_states
  bool accumulated = false;            // a call has submitted samples since fh_init_render_states / fh_set_resolution
  uint32_t adapt_total = 0;            // samples requested since then: the count every pixel still active shares (rounds end where it is a multiple of step)
  fh::DeviceBuffer<uint32_t> d_active[4];  // the active pixels of the round: image indices, x | y << 16 (a stable compaction of the call's base list); [2] / [3]: of its sky list (guard blocks only)
  fh::DeviceBuffer<uint32_t> d_active_blocks; // per-workgroup counts, then their exclusive scan; word [capacity blocks] = the active count (twice: the base list, the sky list)
  fh::PinnedBuffer<uint32_t> h_active_count;  // pinned: the counts read back at every boundary (base list, sky list)
  // fh_set_adaptive_policy: guard blocks of adapt_block x adapt_block pixels stop together, boundaries grow by adapt_growth (render.hip: k_adaptive_mark, adaptive_to_boundary)
  uint32_t adapt_block = 1, adapt_growth = 1;
  fh::DeviceBuffer<uint32_t> d_block_marks;   // one word per guard block of the frame: the sequence number of the last selection that found an unconverged pixel in it
  uint32_t mark_seq = 0;
  fh::DeviceBuffer<unsigned long long> d_sky_taken;  // samples the adaptive k_sky_pixels took since the last fh_sync (fh_stats.paths)
  bool sky_taken_pending = false;
  fh::DeviceBuffer<uint8_t> d_sky_adaptive;      // the adaptive k_sky_pixels' arguments beyond the plain form's (render.hip: SkyAdaptive)

  // environment (renderer.h:819-827)
  bool has_dir = false;
  float dir_le[3] = {0, 0, 0}, dir_dir[3] = {0, 1, 0}, dir_angle = 0;
  float sky_intensity = 1.0f;
  float sun_dir[3] = {0.0f, 1.0f, 0.0f};
  bool has_hosek = false;
  fh::HosekSky hosek{};
  fh::DeviceBuffer<fh::HosekSky> d_hosek;  // device copy (FrameDev::hosek)
  // fh_set_env_sampling (envmap.hip, fh_envmap.h): the table of the environment's luminance the sky rays are drawn from.  Allocated when the switch first goes on;
  // env_stale: the environment changed since it was built (the next fh_render rebuilds it on the context stream)
  int env_sampling = 0;
  float env_cosine_fraction = FH_ENV_COSINE_FRACTION_DEFAULT;
  bool env_stale = true;
  fh::DeviceBuffer<float> d_env_w;         // cell means, then one word: the bits of their maximum
  fh::DeviceBuffer<uint32_t> d_env_q;      // integer weights, then the 256 row sums
  fh::DeviceBuffer<unsigned long long> d_env_total;
  fh::DeviceBuffer<float> d_env_cdf_row, d_env_cdf_m, d_env_cell_p;
  // fh_set_light_sampling (lights.hip, fh_lights.h): the table of the emitters' power the area shadow rays pick from.  Sized for the scene by the rebuild;
  // light_stale: the scene, its transforms or the uniform share changed since it was built (the next fh_render of a scene with emitters rebuilds it on the context stream)
  int light_sampling = 0;
  float light_uniform_fraction = FH_LIGHT_UNIFORM_FRACTION_DEFAULT;
  bool light_stale = true;
  fh::DeviceBuffer<float> d_light_w;                    // weights, then one word: the bits of their maximum
  fh::DeviceBuffer<uint32_t> d_light_q;                 // integer weights, then the sums of the chunks of 256
  fh::DeviceBuffer<unsigned long long> d_light_offsets; // exclusive scan of the chunk sums, then the total
  fh::DeviceBuffer<float> d_light_cdf, d_light_pick_p;  // [n_lights + 1]; [n_faces]
  // fh_set_light_resampling: acts while light_sampling is on.  The proxies are built and rebuilt with the table, so the switch and M alone rebuild nothing
  int light_resampling = 0;
  int light_candidates = FH_LIGHT_CANDIDATES_DEFAULT;
  fh::DeviceBuffer<fh::LightProxy> d_light_proxy;       // [n_lights]

  // path pools: one per pass in flight (pass j uses slot j % n_slots and the stream of that slot: pass_stream); allocated on first use
  struct PoolShape { bool dir = false, lights = false; uint32_t classes = 0; };  // what the records of a pool have room for (render.hip: pool_ensure)
  struct PassSlot {  // everything a pass in flight owns
    fh::PoolDev pool{};
    uint8_t* esc = nullptr;  // one byte per ENTRY of the secondary queue: the slots whose shadow ray escaped (render.hip: k_sky_resolve).  Not a PoolDev member: that is a kernel argument of every pass kernel
    PoolShape shape;
    std::vector<fh::DeviceBuffer<uint8_t>> allocs;
    unsigned long long alloc_bytes = 0;  // device memory the allocations hold (fh_path_pool_allocated)
    // the per-bounce counters of a finished pass on their way to the host (render.hip: harvest_counters)
    struct Snapshot {
      fh::PinnedBuffer<uint32_t> h;
      fh::Event ev;
      bool in_flight = false;
      uint32_t wave_depth = 0, paths = 0;  // wave depth used by the pass the snapshot comes from, and the paths it started
      int bu = -1;              // ... and, while the scene is being probed, where its first-hit rays started (0: the root, 1: the node of their face; -1: not a probing pass)
    } snapshot;
    fh::Event ev_gen, ev_acc;  // the pass's k_generate / k_accumulate has been queued: what the pass after it, on another stream, orders its own after
    bool gen_valid = false, acc_valid = false;
    // the one place that empties the pool (the caller has made sure nothing runs out of it): the next pool_ensure starts from scratch
    void release() { allocs.clear(); alloc_bytes = 0; pool = fh::PoolDev{}; esc = nullptr; shape = PoolShape{}; snapshot.in_flight = false; }
  };
  PassSlot slot[fh::kPassSlots];
  fh::DeviceBuffer<unsigned long long> d_resolve_dbg;  // FH_DEBUG_TAIL: escaped sky and light rays, and the queue entries k_sky_resolve saw, of the call being submitted
  // 32 Mi path slots per pool: 16 samples per pixel per pass at 1080p.  Three pools (one per pass in flight) of 284-436 bytes per path are 27-42 GB when a call brings enough
  // samples to fill them; unless the caller chose the size (fh_set_path_pool), fh_render keeps all pools together within half of the device memory that is free when the first one is made
  uint32_t pool_target_default = 1u << 25, pool_target = 1u << 25;  // (pool_target: the default as capped by the free device memory whenever a pool is (re)allocated, or the caller's size)
  bool pool_target_by_caller = false;
  uint32_t pool_share = 1;          // contexts of one group on this device: each takes its share of the default cap (group.hip)
  uint32_t tail_depth = 0;          // bounces run as wavefront kernels before k_tail finishes the survivors; 0 = adaptive
  uint32_t auto_wave_depth = 2;     // adaptive choice of the pass submitted last (kept for the debug print)
  // what the render path has measured on the current tree; a new tree starts it again (bvh_build.hip: reset_tree_measurements)
  struct TreeMeasurements {
    // the adaptive choice is made per pass from the SHARE of a pass's paths still alive at each depth, taken from the newest snapshot of an earlier pass's counters: a share is a
    // property of the scene and the camera, not of the pass, so a call of another size (one final frame of 4096 spp after a session of 1-spp calls, or the other way round)
    // picks its depth right from its first pass.  (Up to round 5 the DEPTH picked for the earlier pass was carried over: the first 16-spp passes after small calls handed
    // millions of paths to the fused tail, 300 ms each on configs[3].)  survival_n = 0: nothing known yet; entries deeper than the newest snapshot's wavefront bounces are
    // an earlier pass's.
    double survival[66] = {};
    uint32_t survival_n = 0;
    int bu_choice = 0;  // 0: probing, 1: rays start at the root, 2: first-hit rays start at the node of the face they leave (render.hip)
    uint32_t bu_toggle = 0;
    double bu_cost[2] = {0.0, 0.0}, bu_items[2] = {0.0, 0.0};
  } tree;
  unsigned long long pass_seq = 0;           // passes submitted so far
  fh::Event ev_enter;
  int n_slots = fh::kPassSlots;  // passes in flight (FH_PIPELINE=0: 1, every pass on the main stream; =2: two).  Three against two: +2.3 % on configs[2], +0.3-0.9 % on the others, one more path pool
  int last_slot_used = 0;  // slot of the pass submitted last (what the next pass orders itself after)
  std::vector<fh::Event> ev_bounce;  // single-pass calls: (shade done, secondary done) per bounce, for the secondary launch on a second stream (render.hip)
  // FH_FLAG_REFERENCE_FIRSTHIT (render.hip: k_firsthit_scan): per-pixel "a sample of this launch has hit something" + the AOVs of that hit
  fh::DeviceBuffer<uint32_t> d_quirk_seen;
  fh::DeviceBuffer<float4> d_quirk_aov;

  // device facts and developer switches, read ONCE at fh_ctx_create (fh_render does no getenv / hipGetDeviceProperties)
  struct Tunables {
    uint32_t n_cus = 256;
    uint32_t lds_per_cu = 160u * 1024u, lds_per_block = 160u * 1024u;  // LDS of a CU / the most one workgroup may take, from the device attributes (gfx950: 160 KB both)
    uint32_t coop_flush = 48;       // FH_COOP_T: queued candidate triangles that trigger a cooperative test round (r5-12: 32 -> 48, configs[3] +1.6 %, configs[2] +0.5 %)
    bool coop_flush_fixed = false;  // FH_COOP_T was given: no per-call choice (render_submit)
    bool coop = true;               // FH_COOP=0: per-lane triangle loop
    bool stream = true;             // FH_STREAM=0: one fixed batch per wave; FH_STREAM=1: streaming whatever the size of the tree
    bool stream_forced = false;
    uint32_t stream_refill = 24;    // FH_STREAM_REFILL: idle lanes that trigger a refill
    uint32_t stream_min_rays = 64;  // FH_STREAM_MIN_RAYS: queue entries per wave below which workgroups of a streaming launch stay out (render.hip: stream_block_idle); 0 = all take part
    bool overlap_secondary = true;  // FH_OVERLAP=0: single-pass calls keep every launch on one stream
    bool sky_split = true;          // FH_SKY_SPLIT=0: every pixel goes through the passes (no k_sky_pixels)
    uint32_t sky_split_min_log2 = 27; // FH_SKY_SPLIT_MIN_LOG2: a call splits its pixels from 2^n camera paths on (27: 64 spp of a 1080p frame; tests lower it)
    uint32_t sky_blocks_per_cu = 1; // FH_SKY_BLOCKS: workgroups per CU of k_sky_pixels' filler launch, which runs beside the passes (render_submit); 0 = no filler, the drain launch renders everything
    uint32_t sky_filler_grid = 0;   // FH_SKY_FILLER_GRID: the filler's workgroups in total, whatever the number of CUs (tests: one workgroup, so that the drain does most groups); 0 = per CU, above
    bool poison_pools = false;      // FH_POISON=1: new path pools are filled with 0xa5 before their first use (tests: nothing may read what nobody wrote)
    bool merge_trace = true;        // FH_MERGE=0: single-pass calls trace secondary rays and the next bounce's closest-hit rays in two launches (two streams) instead of one
    uint32_t shade_wgs = 0;         // FH_SHADE_WGS=2|3: workgroups per CU the shade kernels are compiled for (0: three; until r5-12 for textured scenes that stream only)
    uint32_t stack_lds_entries = 0; // FH_STACK_LDS=n: stack levels the streaming kernels keep in LDS (0: as many as cost no workgroup; 99: all)
    bool sort_small = false;        // FH_SORT_SMALL=1: cell-order the bounce queues of trees the fixed-batch kernels trace as well
    uint32_t stream_chunk = 64;     // FH_STREAM_CHUNK: queue entries a wave takes per global atomic (setting it also switches the adaptive maximum off)
    bool stream_chunk_fixed = false;
    uint32_t stream_chunk_closest = 128; // FH_STREAM_CHUNK_CLOSEST: the same for the closest-hit launch (0 = stream_chunk).  Its queue is in cell order, so a longer run of it is a more coherent
                                         // wave: 64 / 96 / 128 / 192 / 256 / 512 entries measure 78.5 / 74.0 / 74.2 / 75.7 / 76.7 / 84.1 ms per configs[2] frame; configs[4] 2795 -> 2559 ms.  (The secondary launch,
                                         // whose items are whole paths with two to four rays each, loses with more than 64: 113.9 -> 115.7 ms at 128)
    uint32_t tail_depth = 0;        // FH_TAIL_DEPTH: fixed number of wavefront bounces before k_tail
    uint32_t tail_paths = 0;        // FH_TAIL_PATHS: survivors at which the adaptive mode switches to k_tail; 0 = 65536, 262144 for passes of at most 4 Mi paths
    uint32_t bottom_up = 2;         // FH_BOTTOM_UP=0: every ray starts its traversal at the root; =1: first-hit rays of scenes without cut-outs start at the wide node that holds the face
                                    // they leave and climb; default (2): the first passes after a build try both and the counted test rounds per shaded path decide (render.hip)
    bool sort_queues = true;        // FH_SORT=0: trace the bounce queues in emission order
    uint32_t sort_onepass = 2;      // FH_SORT_ONEPASS: cell sorts in calls of ONE pass -- 0 none, 1 all (as in multi-pass calls), 2 only the queue the fused tail takes over
    uint32_t sky_defer = 2;         // FH_SKY_DEFER=0|1: shadow rays of the sky and light slots carry weights and k_sky_resolve evaluates the environment for those that escape -- never / wherever
                                    // a pass is eligible (render_plan_host.h: sky_defer_verdict); default (2): the library's own choice
    uint32_t dark_sky = 2;          // FH_DARK_SKY=0|1: sky pixels below the Hosek sky's horizon skip k_sky_pixels -- never / wherever a call is eligible (dark_sky_verdict), which is the default too
    bool debug_tail = false;        // FH_DEBUG_TAIL
    bool force_alpha = false;       // FH_FORCE_ALPHA=1 (timing experiments): the kernels with the any-hit path compiled in, whatever the scene
  } tun;

  // bloom weights of the last sigma used (post.hip): no allocation, upload or host synchronisation per frame
  fh::DeviceBuffer<float> d_bloom_weights;
  float bloom_sigma_cached = -1.0f, bloom_wsum = 0.0f;

  // fh_set_auto_exposure (post.hip: k_meter_histogram, k_meter_resolve, k_tone_map_metered).  d_meter: the state, the exposure word and the summed histogram
  // (post.hip: MeterDev), allocated when the switch first goes on; d_meter_slabs: 257 words per workgroup of the metering launch, grown on demand
  int auto_exposure = 0;
  fh_auto_exposure_params ae_params = {0.18f, 0.0f, -16.0f, 16.0f, 0.10f, 0.90f, 3.0f, 1.0f, 1.0f / 30.0f, -16.0f, 16.0f, 0u};
  fh::DeviceBuffer<uint8_t> d_meter;
  fh::DeviceBuffer<uint32_t> d_meter_slabs;

  // fh_set_local_exposure (post.hip: k_lx_down, k_lx_atrous, k_tone_map_local).  d_lx_log: the log image of the last analysis, one float per pixel; d_lx_q: the two
  // quarter-resolution images the a-trous passes go back and forth between -- the base is d_lx_q[lx_passes_run & 1].  All three grow on demand and are kept
  int local_exposure = 0;
  fh_local_exposure_params lx_params = {0.5f, 0.5f, 0.18f, 4.0f, 1.0f, 4u};
  fh::DeviceBuffer<float> d_lx_log;
  fh::DeviceBuffer<float> d_lx_q[2];
  uint32_t lx_w4 = 0, lx_h4 = 0, lx_passes_run = 0;  // of the last analysis; 0 x 0: none since the switch went on

  // denoiser slot (post.hip): ping-pong buffers of the a-trous filter
  fh::DeviceBuffer<float4> d_denoise_tmp[2];
  // variance-guided denoiser (denoise.hip): ping-pong (colour, variance) images and dense variance planes
  fh::DeviceBuffer<float4> d_guided_cv[2];
  fh::DeviceBuffer<float> d_guided_var[2];
  // temporal accumulation (denoise.hip: fh_denoise_temporal): the history, double buffered -- per pixel (c_acc.rgb, v_acc), (P, h) and N, and while
  // fh_set_denoise_temporal_moments is on the luminance moments (mu1, mu2) -- with the camera of the call that wrote buffer `cur`, that camera's world-to-camera rows and
  // its cam_inv_tan.  frames = 0: there is no history.  o2w / w2o: the instance matrices the history was written under (fh_set_denoise_motion; empty: no snapshot).
  // Each member function is the only place that does its job; what a call decides from these facts is temporal_host.h's temporal_call_plan.
  struct TemporalHistory {
    fh::DeviceBuffer<float4> d_cv[2], d_ph[2], d_n[2];
    fh::DeviceBuffer<float2> d_mu[2];  // allocated by the first call with the switch on
    uint32_t w = 0, h = 0, frames = 0;
    int cur = 0;
    fh_camera camera{};
    float w2c[12] = {};
    float inv_tan = 0.0f;
    std::vector<float> o2w, w2o;
    // pixels the buffers have room for.  ensure() allocates in order, so the last buffer tells that all were made
    size_t capacity() const { return d_n[1].size(); }
    size_t moment_capacity() const { return d_mu[1].size(); }
    // the next call starts a new history.  Size and snapshot stay: fh_denoise_temporal has compared the snapshot before the call that restarts, and
    // fh_denoise_history_info reports the size until a call has written another (denoise_temporal_submit: a call at another size, a new moment image)
    void restart() { frames = 0; }
    void forget_instances() { o2w.clear(); w2o.clear(); }  // another scene's instances are not these (scene.hip); fh_set_denoise_motion(0)
    // fh_denoise_history_reset, and fh_set_denoise_temporal_moments when the switch changes.  The buffers stay: the next call overwrites them without reading
    void drop() { restart(); w = 0; h = 0; forget_instances(); }
    void release_moments() { for (int k = 0; k < 2; ++k) d_mu[k].reset(); }  // (the caller has made sure no call queued earlier still writes them)
    // room for a call of px pixels (temporal_host.h: temporal_grow).  A grow frees, marks the history dropped, then allocates: after a failed allocation there is no
    // history, the last buffer of the set is empty, so the capacity reads 0 and the next call makes the whole set again.  New main buffers forget the size as well but
    // not the snapshot -- that is not drop(): a context driven through fh_denoise_temporal_motion keeps the snapshot its next fh_denoise_temporal compares
    hipError_t ensure(size_t px, bool with_moments)
    {
      const fh::TemporalGrow grow = fh::temporal_grow(capacity(), moment_capacity(), px, with_moments);
      if (grow.main) {
        fh::DeviceBuffer<float4>* const bufs[3] = {d_cv, d_ph, d_n};
        for (auto b : bufs)
          for (int k = 0; k < 2; ++k) b[k].reset();
        restart(); w = 0; h = 0;
        for (auto b : bufs)
          for (int k = 0; k < 2; ++k)
            if (const hipError_t e = b[k].alloc(px)) return e;
      }
      if (grow.moments) {  // as large as the rest of the history
        release_moments();
        restart();
        for (int k = 0; k < 2; ++k)
          if (const hipError_t e = d_mu[k].alloc(capacity())) return e;
      }
      return hipSuccess;
    }
    // a call has written buffer cur ^ 1 under this camera
    void commit(const fh_camera& cam, const float cam_w2c[12], float cam_inv_tan, uint32_t cw, uint32_t ch)
    {
      cur ^= 1; camera = cam; inv_tan = cam_inv_tan;
      for (int k = 0; k < 12; ++k) w2c[k] = cam_w2c[k];
      w = cw; h = ch;
      if (frames != 0xffffffffu) ++frames;
    }
  } hist;
  // per-instance motion vectors (motion.hip, denoise.hip: k_temporal<kLookMotion, .>).  denoise_motion: fh_set_denoise_motion.  The motion table of a call goes through
  // the pinned h_motion (ev_motion: its copy has been taken) to d_motion; d_motion_ids is the id plane of the calls the context feeds itself.
  int denoise_motion = 0;
  fh::DeviceBuffer<fh_motion> d_motion;
  fh::PinnedBuffer<fh_motion> h_motion;
  fh::Event ev_motion;
  fh::DeviceBuffer<uint32_t> d_motion_ids;
  // fh_set_denoise_response (denoise.hip: k_temporal<., kClipColour>): while on, the temporal stage clips the history it found to the current frame's 5 x 5 colour box
  int denoise_response = 0;
  float response_gamma = 1.0f;
  // fh_set_denoise_response_noise (k_temporal<., kClipColourNoise>): the clipped history is clamped to the pixel's measured noise as well; inert while the switch above is off
  int denoise_response_noise = 0;
  float response_kappa = 6.0f;
  // fh_set_denoise_temporal_moments (k_temporal<., ., true>): while on, the history holds one more double-buffered image, the luminance moments (mu1, mu2), and a call
  // without sample moments takes its variance from them once a pixel's history is moments_min_history long (hist.d_mu).
  int denoise_temporal_moments = 0;
  float moments_min_history = 2.0f;

  // stats
  fh_stats stats{};
  fh::DeviceBuffer<unsigned long long> d_trace_counters;  // nodes, tris, rays of the closest-hit kernel, then of the secondary kernel
  struct TimedSpan { fh::Event a, b; int kind; };
  std::vector<TimedSpan> spans;
  std::vector<fh::Event> event_pool;
  fh::Event ev_render_begin, ev_render_end;
  bool render_pending = false;
};

namespace fh {
int fail(fh_ctx* ctx, int code, const std::string& msg);
#define FH_HIP(call)                                                                                                   \
  do {                                                                                                                 \
    hipError_t e_ = (call);                                                                                            \
    if (e_ != hipSuccess) return fh::fail(ctx, FH_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_));            \
  } while (0)
// the top of an entry point that takes a context: the context's device is the current one from here on
#define CTX_CHECK(ctx)                      \
  if (!(ctx)) return FH_E_INVALID;          \
  if (hipSetDevice((ctx)->device) != hipSuccess) return fh::fail(ctx, FH_E_HIP, "hipSetDevice failed")

// group dispatch at the top of the entry points (group.hip).  A plain context pays the one branch.
#define FH_GROUP(ctx, call) \
  if ((ctx) && (ctx)->group) return fh::call
#define FH_GROUP_EACH(ctx, kind, call) \
  if ((ctx) && (ctx)->group) return fh::group_each(ctx, kind, [&](fh_ctx* m_, uint32_t i_) { (void)i_; return call; })
#define FH_GROUP_LEAD(ctx) \
  if ((ctx) && (ctx)->group) ctx = fh::group_lead(ctx)
#define FH_GROUP_REFUSE(ctx, name) \
  if ((ctx) && (ctx)->group) return fh::fail(ctx, FH_E_UNSUPPORTED, name ": not available on a group (a plain context does hand-rolled gathers and known-answer runs)")
enum { kGroupCallPlain = 0, kGroupCallScene = 1, kGroupCallFrame = 2, kGroupCallUpload = 3 };  // what a broadcast that fails half way leaves in doubt: nothing, the scene, the frame state; fh_scene_upload itself
fh_ctx* group_lead(fh_ctx* g);
int group_each(fh_ctx* g, int kind, const std::function<int(fh_ctx*, uint32_t)>& call);
int group_destroy(fh_ctx* g);
int group_set_resolution(fh_ctx* g, uint32_t w, uint32_t h);
int group_set_tile_shard(fh_ctx* g, uint32_t rank, uint32_t world, uint32_t tw, uint32_t th);
int group_init_render_states(fh_ctx* g);
int group_render(fh_ctx* g, const fh_camera* cam, const float* bg, const fh_render_layers* layers, uint32_t n_samples, uint32_t max_depth, uint32_t seed);
int group_get_sample_counts(fh_ctx* g, uint32_t* counts);
int group_get_luminance_moments(fh_ctx* g, float* moments);
int group_active_pixel_count(fh_ctx* g, uint32_t* out);
int group_owned_pixel_count(fh_ctx* g, uint32_t* out);
int group_get_stats(fh_ctx* g, fh_stats* out);
int group_path_pool_allocated(fh_ctx* g, uint64_t* bytes, uint64_t* paths);
int frame_map_ensure(fh_ctx* ctx, uint32_t world);  // capi.hip: ctx->frame_map for `world` ranks at the context's resolution and tile size
uint32_t owned_count(uint32_t width, uint32_t height, uint32_t tw, uint32_t th, uint32_t rank, uint32_t world);  // capi.hip

Event take_event(fh_ctx* ctx);  // render.hip: a timing event from ctx->event_pool, or a new one
SceneDev scene_dev(const fh_ctx* ctx);
inline EnvTable env_table_dev(const fh_ctx* ctx) { return EnvTable{ctx->d_env_cdf_row, ctx->d_env_cdf_m, ctx->d_env_cell_p, ctx->env_cosine_fraction}; }
inline LightTable light_table_dev(const fh_ctx* ctx)
{
  return LightTable{ctx->d_light_cdf, ctx->d_light_pick_p, ctx->light_uniform_fraction, ctx->d_light_proxy, ctx->light_resampling ? (uint32_t)ctx->light_candidates : 1u};
}
int bvh_build_device(fh_ctx* ctx);                 // bvh_build.hip
void reset_tree_measurements(fh_ctx* ctx);         // bvh_build.hip: a new tree; what the render path has measured on the old one (bu_*, survival) starts again
int render_submit(fh_ctx* ctx, const fh_camera* cam, const float* bg, const fh_render_layers* layers, uint32_t n_samples, uint32_t max_depth, uint32_t seed);  // render.hip
int adaptive_upload(fh_ctx* ctx);  // render.hip
int adaptive_select(fh_ctx* ctx, hipStream_t st, const uint32_t* base_px, const uint32_t* base_xy, uint32_t n_base, uint32_t* n_active, const uint32_t* sky_px = nullptr,
                    const uint32_t* sky_xy = nullptr, uint32_t n_sky = 0, uint32_t* n_sky_active = nullptr);  // render.hip (synchronising)
uint32_t adaptive_to_boundary(const fh_ctx* ctx);  // render.hip: samples from adapt_total to the next boundary
int pool_ensure(fh_ctx* ctx, int slot, uint32_t capacity);   // render.hip
uint64_t pool_bytes_per_path(const fh_ctx* ctx);            // capi.hip
void pool_release(fh_ctx* ctx);
// the stream the passes of a pool slot run on: slot 0's is the main stream
inline hipStream_t pass_stream(const fh_ctx* ctx, int slot) { return slot ? ctx->aux_stream[slot - 1] : ctx->stream; }
// waits until no pass is running: the main stream, then every aux stream, then (with_sky) the sky stream if there is one.  The first error
inline hipError_t drain_passes(fh_ctx* ctx, bool with_sky)
{
  hipError_t first = hipStreamSynchronize(ctx->stream);
  for (int k = 0; k < kPassSlots - 1; ++k) { const hipError_t e = hipStreamSynchronize(ctx->aux_stream[k]); if (first == hipSuccess) first = e; }
  if (with_sky && ctx->sky_stream) { const hipError_t e = hipStreamSynchronize(ctx->sky_stream); if (first == hipSuccess) first = e; }
  return first;
}
int kernel_info(fh_ctx* ctx, int which, uint32_t out[6]);   // render.hip
#if defined(FH_CHECK_DIV_RANGES)
int div_range_violations_read(fh_ctx* ctx, uint64_t* n);  // render.hip: the counter of its kernels (fh_vec.h: div_r), which belongs to the device's code object, not to a context
#endif
int post_process_submit(fh_ctx* ctx, const float* in, float* hi, float* tmp, int w, int h, const fh_post_params* pp, float* out);  // post.hip
// post.hip, auto-exposure (arguments checked by the caller): the switch with its device state; metering + resolve of one image; frames = 0; synchronising read-backs
int auto_exposure_set(fh_ctx* ctx, const fh_auto_exposure_params* params);
int meter_submit(fh_ctx* ctx, const float* image, uint32_t w, uint32_t h);
int auto_exposure_reset(fh_ctx* ctx);
int auto_exposure_read(fh_ctx* ctx, fh_auto_exposure_state* state, uint32_t* hist);
// post.hip, local exposure (arguments checked by the caller): the switch; log image, quarter image and a-trous passes of one image; the synchronising read-back
int local_exposure_set(fh_ctx* ctx, const fh_local_exposure_params* params);
int local_exposure_submit(fh_ctx* ctx, const float* image, uint32_t w, uint32_t h);
int local_exposure_read_base(fh_ctx* ctx, float* base, uint32_t* w4, uint32_t* h4);
int denoise_submit(fh_ctx* ctx, int w, int h, const float* beauty, const float* normal, const float* albedo, float* out, int upscale);  // post.hip
int denoise_guided_submit(fh_ctx* ctx, int w, int h, const fh_denoise_inputs* in, const fh_denoise_params* params, float* out, int upscale);  // denoise.hip (arguments checked by the caller)
// denoise.hip (arguments checked by the caller); w2c, inv_tan: `cam` inverted and its cam_inv_tan, kept with the history this call writes
// ids == nullptr: no motion stage; else ids a device pointer and motion a host array of n_instances entries of which at least one has moved (k_temporal<kLookMotion, .>)
int denoise_temporal_submit(fh_ctx* ctx, int w, int h, const fh_denoise_inputs* in, const fh_camera* cam, const float w2c[12], float inv_tan, const fh_temporal_params* tp,
                            const fh_denoise_params* params, const uint32_t* ids, uint32_t n_instances, const fh_motion* motion, float* out, int upscale);
// envmap.hip: the switch with its device memory (arguments checked by the caller); the rebuild of a stale table, queued on the context stream
int env_sampling_set(fh_ctx* ctx, const fh_env_sampling_params* params);
int env_table_ensure(fh_ctx* ctx);
// lights.hip: the switch (arguments checked by the caller); the rebuild of a stale table, queued on the context stream (nothing for a scene without emitters)
int light_sampling_set(fh_ctx* ctx, const fh_light_sampling_params* params);
int light_table_ensure(fh_ctx* ctx);
FrameDev env_frame(const fh_ctx* ctx);  // the environment as the table weighs it: sky intensity 1, a white background
int primary_instances_submit(fh_ctx* ctx, const fh_camera* cam, uint32_t w, uint32_t h, uint32_t* ids);  // motion.hip (arguments checked by the caller)
}  // namespace fh
