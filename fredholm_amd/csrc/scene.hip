// scene.hip -- the device side of the scene: fh_scene_upload, fh_set_transforms and the skin (fh_set_skin, fh_set_joint_matrices).  An upload is a plan (scene_plan_host.h: everything decided on the host, from
// the caller's descriptor alone), then either a refusal that leaves the context as it was or the upload steps below, then the commit.  Mirrors
// Renderer::load_scene / set_time (fredholm/include/fredholm/renderer.h:361-432).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "context.h"
#include "fh_skin.h"
#include "fh_vec.h"
#include "scene_plan_host.h"
#include "skin_plan_host.h"

namespace fh {

namespace {

static_assert(sizeof(Word2) == sizeof(uint2) && offsetof(Word2, y) == offsetof(uint2, y), "Word2 is the device's uint2");
static_assert(sizeof(Word4) == sizeof(uint4) && offsetof(Word4, y) == offsetof(uint4, y) && offsetof(Word4, z) == offsetof(uint4, z) && offsetof(Word4, w) == offsetof(uint4, w),
              "Word4 is the device's uint4");
static_assert(sizeof(MaterialRecord) == sizeof(MaterialDev) && offsetof(MaterialRecord, lobes) == offsetof(MaterialDev, lobes) && offsetof(MaterialRecord, emissive) == offsetof(MaterialDev, emissive) &&
                  offsetof(MaterialRecord, alpha) == offsetof(MaterialDev, alpha) && offsetof(MaterialRecord, cls) == offsetof(MaterialDev, cls),
              "MaterialRecord is the device's MaterialDev");
static_assert(sizeof(LightRecord) == sizeof(AreaLightDev) && offsetof(LightRecord, material) == offsetof(AreaLightDev, material), "LightRecord is the device's AreaLightDev");

const float kIdentity12[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};

// world-space face record of every face (layout: fh_device.h) from the object-space arrays and the instance transforms:
// positions by object_to_world, normals by the transpose of world_to_object (shared.h:42-50), as pt.cu:141-179 does per hit
__global__ void __launch_bounds__(256) k_face_records(uint32_t nf, const float* vertices, const float* normals, const float* texcoords, const uint32_t* indices, const uint2* meta,
                                                      const float4* o2w, const float4* w2o, float4* rec)
{
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nf) return;
  const uint2 mi = meta[f];
  m34 a, b;
#pragma unroll
  for (int k = 0; k < 3; ++k) { a.r[k] = o2w[3 * (size_t)mi.y + k]; b.r[k] = w2o[3 * (size_t)mi.y + k]; }
  f3 p[3], n[3];
  float uv[3][2];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const size_t v = indices[3 * (size_t)f + k];
    p[k] = xform_point(a, mk3(vertices[3 * v], vertices[3 * v + 1], vertices[3 * v + 2]));
    n[k] = xform_normal(b, mk3(normals[3 * v], normals[3 * v + 1], normals[3 * v + 2]));
    uv[k][0] = texcoords[2 * v];
    uv[k][1] = texcoords[2 * v + 1];
  }
  float4* r = rec + kFaceRec * (size_t)f;
  r[0] = mk4(p[0], uv[0][0]); r[1] = mk4(p[1], uv[0][1]); r[2] = mk4(p[2], uv[1][0]);
  r[3] = mk4(n[0], uv[1][1]); r[4] = mk4(n[1], uv[2][0]); r[5] = mk4(n[2], uv[2][1]);
  r[6] = make_float4(__uint_as_float(mi.x), __uint_as_float(mi.y), 0.0f, 0.0f);
}

// Posed object-space position and normal of every vertex (fh_skin.h: skin_vertex) from the bind arrays, the vertex's four joints and weights and the palette of
// joint matrices, which is read with plain loads: 48 bytes per joint, shared by every thread that names the joint
__global__ void __launch_bounds__(256) k_skin_vertices(uint32_t nv, const float* vertices, const float* normals, const uint2* joints, const float4* weights, const float4* palette,
                                                       float* posed_vertices, float* posed_normals)
{
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nv) return;
  const float p[3] = {vertices[3 * (size_t)v], vertices[3 * (size_t)v + 1], vertices[3 * (size_t)v + 2]};
  const float n[3] = {normals[3 * (size_t)v], normals[3 * (size_t)v + 1], normals[3 * (size_t)v + 2]};
  const uint2 jj = joints[v];
  const float4 ww = weights[v];
  const uint32_t j[4] = {jj.x & 0xffffu, jj.x >> 16, jj.y & 0xffffu, jj.y >> 16};
  const float w[4] = {ww.x, ww.y, ww.z, ww.w};
  float po[3] = {p[0], p[1], p[2]}, no[3] = {n[0], n[1], n[2]};
  if (!skin_unskinned(w)) {
    float m[4][12];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const float4 row = palette[3 * (size_t)j[k] + r];
        m[k][4 * r] = row.x; m[k][4 * r + 1] = row.y; m[k][4 * r + 2] = row.z; m[k][4 * r + 3] = row.w;
      }
    float b[12];
    skin_blend(m[0], m[1], m[2], m[3], w, b);
    skin_point(b, p, po);
    skin_normal(b, n, no);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) { posed_vertices[3 * (size_t)v + k] = po[k]; posed_normals[3 * (size_t)v + k] = no[k]; }
}

// The world-space face records from the object-space arrays resident on the device (the posed ones while a skin is posed) and the context's transforms: a frame of an animation (fh_set_transforms)
// uploads 96 bytes per instance instead of recomputing and re-uploading 112 bytes per face
int transform_faces(fh_ctx* ctx)
{
  const uint32_t ni = (uint32_t)ctx->h_o2w.size() / 12;
  FH_HIP(ctx->d_o2w.ensure(3ull * ni));  // (three rows per instance)
  FH_HIP(ctx->d_w2o.ensure(3ull * ni));
  FH_HIP(hipMemcpyAsync(ctx->d_o2w, ctx->h_o2w.data(), 48ull * ni, hipMemcpyHostToDevice, ctx->stream));
  FH_HIP(hipMemcpyAsync(ctx->d_w2o, ctx->h_w2o.data(), 48ull * ni, hipMemcpyHostToDevice, ctx->stream));
  const float* const vertices = ctx->skin.posed ? ctx->skin.d_vertices.get() : ctx->d_obj_vertices.get();
  const float* const normals = ctx->skin.posed ? ctx->skin.d_normals.get() : ctx->d_obj_normals.get();
  if (ctx->n_faces)
    hipLaunchKernelGGL(k_face_records, dim3((ctx->n_faces + 255) / 256), dim3(256), 0, ctx->stream, ctx->n_faces, vertices, normals, ctx->d_obj_texcoords.get(), ctx->d_obj_indices.get(),
                       ctx->d_face_meta.get(), ctx->d_o2w.get(), ctx->d_w2o.get(), ctx->d_face_rec.get());
  FH_HIP(hipGetLastError());
  FH_HIP(hipStreamSynchronize(ctx->stream));  // the host copies of the transforms may change right after this call
  ctx->bvh_valid = false;
  ctx->light_stale = true;  // (fh_set_light_sampling: areas, and after an upload the emitters themselves, are new)
  return FH_OK;
}

// the only getenv calls of an upload
SceneSwitches read_scene_switches() { return scene_switches(getenv("FH_OPACITY_CLASSES"), getenv("FH_OPACITY_MICROMAP"), getenv("FH_DEBUG_BVH")); }

// n elements of the caller's (or the plan's) array into a buffer of exactly that size
template <typename T, typename U>
int upload_array(fh_ctx* ctx, DeviceBuffer<T>& d, const U* src, size_t n)
{
  static_assert(sizeof(T) == sizeof(U), "same layout on both sides");
  FH_HIP(d.alloc(n));
  if (n) FH_HIP(hipMemcpy(d, src, n * sizeof(T), hipMemcpyHostToDevice));
  return FH_OK;
}

// texels of all textures in one device blob + descriptors + the 256-entry sRGB table (cwl/texture.h:13-75 per texture)
int upload_textures(fh_ctx* ctx, const fh_scene_desc& s, const ScenePlan& plan)
{
  ctx->d_texels.reset();
  ctx->d_textures.reset();
  if (!ctx->d_srgb_lut) {
    float lut[256];
    srgb_decode_table(lut);
    FH_HIP(ctx->d_srgb_lut.alloc(256));
    FH_HIP(hipMemcpy(ctx->d_srgb_lut, lut, sizeof lut, hipMemcpyHostToDevice));
  }
  if (s.n_textures == 0) return FH_OK;
  FH_HIP(ctx->d_texels.alloc(plan.texel_bytes));
  std::vector<fht_texture> t(s.n_textures);
  for (uint32_t i = 0; i < s.n_textures; ++i) {
    const fh_texture_desc& d = s.textures[i];
    FH_HIP(hipMemcpy(ctx->d_texels + plan.tex_offset[i], d.rgba8, (size_t)d.width * d.height * 4, hipMemcpyHostToDevice));
    t[i] = fht_texture{ctx->d_texels + plan.tex_offset[i], nullptr, d.width, d.height, d.srgb ? 1u : 0u};
  }
  return upload_array(ctx, ctx->d_textures, t.data(), t.size());
}

// The host copy of the flat scene that the context keeps (the transforms can change: Renderer::set_time).  Made before the uploads, which read it instead of the
// caller's arrays, in the storage the context's arrays had: the first upload of a process measures a third slower from the caller's pages, and an upload over a
// loaded scene several times slower into fresh allocations (profiles/README.md).  The context's arrays are empty from here to the commit, which moves the copy in.
struct HostScene {
  std::vector<float> vertices, normals, texcoords, o2w, w2o;
  std::vector<uint32_t> indices, material_ids, instance_ids;
  std::vector<fh_material> materials;
};
HostScene copy_host_scene(fh_ctx* ctx, const fh_scene_desc& s)
{
  HostScene h{std::move(ctx->h_vertices), std::move(ctx->h_normals), std::move(ctx->h_texcoords), std::move(ctx->h_o2w), std::move(ctx->h_w2o),
              std::move(ctx->h_indices), std::move(ctx->h_material_ids), std::move(ctx->h_instance_ids), std::move(ctx->h_materials)};
  h.vertices.assign(s.vertices, s.vertices + 3ull * s.n_vertices);
  h.normals.assign(s.normals, s.normals + 3ull * s.n_vertices);
  h.texcoords.assign(s.texcoords, s.texcoords + 2ull * s.n_vertices);
  h.indices.assign(s.indices, s.indices + 3ull * s.n_faces);
  h.material_ids.assign(s.material_ids, s.material_ids + s.n_faces);
  if (s.instance_ids) h.instance_ids.assign(s.instance_ids, s.instance_ids + s.n_faces);
  else h.instance_ids.clear();
  h.materials.assign(s.materials, s.materials + s.n_materials);
  if (s.n_instances && s.object_to_world && s.world_to_object) {
    h.o2w.assign(s.object_to_world, s.object_to_world + 12ull * s.n_instances);
    h.w2o.assign(s.world_to_object, s.world_to_object + 12ull * s.n_instances);
  } else {
    h.o2w.assign(kIdentity12, kIdentity12 + 12);
    h.w2o.assign(kIdentity12, kIdentity12 + 12);
  }
  return h;
}

// the per-face and per-material tables of the plan, and the object-space geometry the face records are derived from on the device
int upload_geometry(fh_ctx* ctx, const HostScene& h, const ScenePlan& plan)
{
  FH_HIP(ctx->d_face_rec.alloc((size_t)kFaceRec * plan.face_cls.size()));
  if (const int rc = upload_array(ctx, ctx->d_face_cls, plan.face_cls.data(), plan.face_cls.size())) return rc;
  if (const int rc = upload_array(ctx, ctx->d_materials, plan.materials.data(), plan.materials.size())) return rc;
  if (const int rc = upload_array(ctx, ctx->d_lights, plan.lights.data(), plan.lights.size())) return rc;
  if (const int rc = upload_array(ctx, ctx->d_obj_vertices, h.vertices.data(), h.vertices.size())) return rc;
  if (const int rc = upload_array(ctx, ctx->d_obj_normals, h.normals.data(), h.normals.size())) return rc;
  if (const int rc = upload_array(ctx, ctx->d_obj_texcoords, h.texcoords.data(), h.texcoords.size())) return rc;
  if (const int rc = upload_array(ctx, ctx->d_obj_indices, h.indices.data(), h.indices.size())) return rc;
  return upload_array(ctx, ctx->d_face_meta, plan.face_meta.data(), plan.face_meta.size());
}

// the any-hit records, where a face keeps its test: the plan's, with the address of the texel blob added (in place) to the byte offsets in their two texture slots
int upload_alpha_records(fh_ctx* ctx, ScenePlan& plan)
{
  ctx->d_alpha_rec.reset();
  if (!plan.any_alpha) return FH_OK;
  std::vector<Word4>& rec = plan.alpha_rec;
  const unsigned long long base = (unsigned long long)(uintptr_t)ctx->d_texels.get();
  for (size_t f = 0; 8 * f < rec.size(); ++f)
    for (uint32_t slot = 0; slot < 2; ++slot)
      if (rec[8 * f + 1].z & (1u << slot)) {
        Word4& t = rec[8 * f + 2 + slot];
        const unsigned long long p = base + ((unsigned long long)t.x | (unsigned long long)t.y << 32);
        t.x = (uint32_t)p; t.y = (uint32_t)(p >> 32);
      }
  return upload_array(ctx, ctx->d_alpha_rec, rec.data(), rec.size());
}

// Every context field an upload writes, once everything is on the device: the host copy of the flat scene and the counters.
void commit_scene(fh_ctx* ctx, const fh_scene_desc& s, HostScene& h, const ScenePlan& plan)
{
  ctx->h_vertices = std::move(h.vertices);
  ctx->h_normals = std::move(h.normals);
  ctx->h_texcoords = std::move(h.texcoords);
  ctx->h_indices = std::move(h.indices);
  ctx->h_material_ids = std::move(h.material_ids);
  ctx->h_instance_ids = std::move(h.instance_ids);
  ctx->h_materials = std::move(h.materials);
  ctx->h_o2w = std::move(h.o2w);
  ctx->h_w2o = std::move(h.w2o);
  ctx->n_textures = s.n_textures;
  ctx->n_faces = s.n_faces;
  ctx->n_lights = (uint32_t)plan.lights.size();
  ctx->n_materials = s.n_materials;
  ctx->n_classes = plan.n_classes;
  for (uint32_t c = 0; c < plan.n_classes; ++c) ctx->class_lobes[c] = plan.class_lobes[c];
  ctx->has_alpha = plan.any_alpha;
  for (int k = 0; k < 4; ++k) ctx->alpha_face_counts[k] = plan.alpha_face_counts[k];
  for (int k = 0; k < 3; ++k) ctx->alpha_cell_counts[k] = plan.alpha_cell_counts[k];
  ctx->refit_ok = false;  // new topology: the next build is a full one
  ctx->builder_choice = 0;  // new geometry: let the next build choose its builder again
  ctx->hist.forget_instances();  // (fh_set_denoise_motion: another scene's instances are not these)
  if (plan.sw.debug && plan.alpha_face_counts[0])
    fprintf(stderr, "[alpha] %u faces whose textures can cut: %u always pass, %u never pass, %u keep their any-hit test\n", plan.alpha_face_counts[0], plan.alpha_face_counts[1], plan.alpha_face_counts[2],
            plan.alpha_face_counts[3]);
  if (plan.sw.debug && plan.alpha_cell_counts[0])
    fprintf(stderr, "[alpha] micromap: %llu cells of the faces that keep their test: %.1f %% always pass, %.1f %% never pass\n", plan.alpha_cell_counts[0], 100.0 * plan.alpha_cell_counts[1] / plan.alpha_cell_counts[0],
            100.0 * plan.alpha_cell_counts[2] / plan.alpha_cell_counts[0]);
}

// From the first step on the context has no scene; it has the new one when the last step has succeeded.  A HIP error half way leaves a context that refuses to
// render until an upload succeeds, not a mix of two scenes.
int upload_scene(fh_ctx* ctx, const fh_scene_desc& s, ScenePlan& plan)
{
  ctx->scene_loaded = false;
  ctx->bvh_valid = false;
  ctx->skin.drop();  // (a skin belongs to the scene it was set on)
  if (const int rc = upload_textures(ctx, s, plan)) return rc;
  HostScene host = copy_host_scene(ctx, s);
  if (const int rc = upload_geometry(ctx, host, plan)) return rc;
  if (const int rc = upload_alpha_records(ctx, plan)) return rc;
  commit_scene(ctx, s, host, plan);
  if (const int rc = transform_faces(ctx)) return rc;
  ctx->scene_loaded = true;
  return FH_OK;
}

SkinFacts skin_facts(const fh_ctx* ctx) { return SkinFacts{ctx->scene_loaded, (uint32_t)(ctx->h_vertices.size() / 3), ctx->skin.n_joints}; }

// the posed arrays from the bind arrays and the palette the context holds, then the face records from them
int pose_vertices(fh_ctx* ctx)
{
  const uint32_t nv = (uint32_t)(ctx->h_vertices.size() / 3);
  FH_HIP(hipMemcpyAsync(ctx->skin.d_palette, ctx->skin.h_palette.data(), 48ull * ctx->skin.n_joints, hipMemcpyHostToDevice, ctx->stream));
  if (nv)
    hipLaunchKernelGGL(k_skin_vertices, dim3((nv + 255) / 256), dim3(256), 0, ctx->stream, nv, ctx->d_obj_vertices.get(), ctx->d_obj_normals.get(), ctx->skin.d_joints.get(), ctx->skin.d_weights.get(),
                       ctx->skin.d_palette.get(), ctx->skin.d_vertices.get(), ctx->skin.d_normals.get());
  FH_HIP(hipGetLastError());
  ctx->skin.posed = true;
  return transform_faces(ctx);
}

}  // namespace
}  // namespace fh

using namespace fh;

extern "C" {

int fh_scene_upload(fh_ctx* ctx, const fh_scene_desc* s)
{
  FH_GROUP_EACH(ctx, kGroupCallUpload, fh_scene_upload(m_, s));
  if (!ctx) return FH_E_INVALID;
  // every refusal of the arguments comes from the plan, before the context or the device is touched: the context keeps its scene, its textures, its tree and its counters
  ScenePlan plan = plan_scene(s, read_scene_switches(), kMaxClasses);
  if (plan.error) return fail(ctx, FH_E_INVALID, plan.error);
  CTX_CHECK(ctx);
  return upload_scene(ctx, *s, plan);
}

int fh_set_transforms(fh_ctx* ctx, uint32_t n, const float* o2w, const float* w2o)
{
  FH_GROUP_EACH(ctx, kGroupCallScene, fh_set_transforms(m_, n, o2w, w2o));
  CTX_CHECK(ctx);
  if (!ctx->scene_loaded || !o2w || !w2o || n == 0) return fail(ctx, FH_E_INVALID, "fh_set_transforms: no scene / null arrays");
  // a frame of an animation that only moves the camera (rtcamp8's scene) leaves every instance where it was: keep the world-space
  // geometry and the acceleration structure (fh_bvh_build returns at once while bvh_valid holds)
  if (ctx->h_o2w.size() == 12ull * n && ctx->h_w2o.size() == 12ull * n && std::memcmp(ctx->h_o2w.data(), o2w, 48ull * n) == 0 &&
      std::memcmp(ctx->h_w2o.data(), w2o, 48ull * n) == 0)
    return FH_OK;
  (void)drain_passes(ctx, false);  // no pass may still be reading the face records
  uint32_t max_inst = 0;
  for (uint32_t i : ctx->h_instance_ids) max_inst = i > max_inst ? i : max_inst;
  if (max_inst >= n) return fail(ctx, FH_E_INVALID, "fh_set_transforms: fewer transforms than the scene has instances");
  ctx->h_o2w.assign(o2w, o2w + 12ull * n);
  ctx->h_w2o.assign(w2o, w2o + 12ull * n);
  return transform_faces(ctx);  // topology, classes and lights are unchanged: only the world-space records move (and the BVH is refitted)
}

int fh_set_skin(fh_ctx* ctx, const fh_skin_desc* d)
{
  FH_GROUP_EACH(ctx, kGroupCallScene, fh_set_skin(m_, d));
  if (!ctx) return FH_E_INVALID;
  if (const char* why = skin_refusal(skin_facts(ctx), d)) return fail(ctx, FH_E_INVALID, why);
  CTX_CHECK(ctx);
  (void)drain_passes(ctx, false);  // no pass may still be reading face records that are about to return to the bind pose
  const bool was_posed = ctx->skin.posed;
  ctx->skin.drop();
  // a skin alone moves nothing: the geometry is the bind pose until the first fh_set_joint_matrices, and returns to it when a posed skin goes
  if (was_posed)
    if (const int rc = transform_faces(ctx)) return rc;
  if (d) {
    fh_ctx::Skin& sk = ctx->skin;
    const size_t nv = d->n_vertices;
    FH_HIP(sk.d_joints.alloc(nv));
    FH_HIP(sk.d_weights.alloc(nv));
    FH_HIP(sk.d_palette.alloc(3ull * d->n_joints));
    FH_HIP(sk.d_vertices.alloc(3 * nv));
    FH_HIP(sk.d_normals.alloc(3 * nv));
    if (nv) {
      FH_HIP(hipMemcpy(sk.d_joints, d->joints, 8 * nv, hipMemcpyHostToDevice));
      FH_HIP(hipMemcpy(sk.d_weights, d->weights, 16 * nv, hipMemcpyHostToDevice));
    }
    sk.n_joints = d->n_joints;
    sk.n_skinned = skin_count_skinned(*d);
  }
  return FH_OK;
}

int fh_set_joint_matrices(fh_ctx* ctx, uint32_t n, const float* m3x4)
{
  FH_GROUP_EACH(ctx, kGroupCallScene, fh_set_joint_matrices(m_, n, m3x4));
  if (!ctx) return FH_E_INVALID;
  if (const char* why = joint_matrices_refusal(skin_facts(ctx), n, m3x4)) return fail(ctx, FH_E_INVALID, why);
  CTX_CHECK(ctx);
  // the pose the context already holds: keep the geometry and the acceleration structure, as fh_set_transforms does
  if (ctx->skin.posed && ctx->skin.h_palette.size() == 12ull * n && std::memcmp(ctx->skin.h_palette.data(), m3x4, 48ull * n) == 0) return FH_OK;
  (void)drain_passes(ctx, false);  // no pass may still be reading the face records
  ctx->skin.h_palette.assign(m3x4, m3x4 + 12ull * n);
  return pose_vertices(ctx);
}

int fh_get_skin_info(fh_ctx* ctx, uint32_t* n_joints, uint32_t* n_skinned_vertices, int* posed)
{
  FH_GROUP_LEAD(ctx);
  if (!ctx) return FH_E_INVALID;
  if (n_joints) *n_joints = ctx->skin.n_joints;
  if (n_skinned_vertices) *n_skinned_vertices = ctx->skin.n_skinned;
  if (posed) *posed = ctx->skin.posed ? 1 : 0;
  return FH_OK;
}

int fh_get_posed_geometry(fh_ctx* ctx, float* vertices3, float* normals3)
{
  FH_GROUP_LEAD(ctx);
  CTX_CHECK(ctx);
  if (!ctx->scene_loaded || !vertices3 || !normals3) return fail(ctx, FH_E_INVALID, "fh_get_posed_geometry: no scene / null arrays");
  const size_t bytes = ctx->h_vertices.size() * sizeof(float);
  if (!ctx->skin.posed) {
    std::memcpy(vertices3, ctx->h_vertices.data(), bytes);
    std::memcpy(normals3, ctx->h_normals.data(), bytes);
    return FH_OK;
  }
  if (bytes) {  // (the call that posed them has synchronised the stream)
    FH_HIP(hipMemcpy(vertices3, ctx->skin.d_vertices, bytes, hipMemcpyDeviceToHost));
    FH_HIP(hipMemcpy(normals3, ctx->skin.d_normals, bytes, hipMemcpyDeviceToHost));
  }
  return FH_OK;
}

}  // extern "C"
