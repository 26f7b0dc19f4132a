// fredholm/renderer.h -- drop-in facade with the method surface of the reference's header-only
// fredholm::Renderer (fredholm/include/fredholm/renderer.h:29-846).  Every method forwards to the C ABI of
// libfredholm_hip.so; a non-zero status becomes std::runtime_error like the reference's CUDA_CHECK /
// OPTIX_CHECK.  The OptiX pipeline-construction calls are kept as no-ops so application code
// (app/controller.cpp:60-68, app/rtcamp8.cpp:75-146) compiles unchanged.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <filesystem>
#include <stdexcept>

// the reference's header includes the application's logging library (renderer.h:12), and app/controller.cpp:311 relies on getting it from here
#if defined(__has_include)
#if __has_include("spdlog/spdlog.h")
#include "spdlog/spdlog.h"
#endif
#endif

#include "../cwl/buffer.h"
#include "../cwl/util.h"
#include "../optwl/optwl.h"
#include "camera.h"
#include "scene.h"
#include "shared.h"

namespace fredholm
{

class Renderer
{
 public:
  // FH_ENV_SAMPLING gives an application that is not edited importance sampling of the environment (fh_set_env_sampling): unset or 0: off; 1: on with the
  // library's cosine fraction; any other number: on with that fraction (one the library refuses throws here).  set_env_sampling / clear_env_sampling win.
  // FH_LIGHT_SAMPLING does the same for the sampling of area lights by power (fh_set_light_sampling): unset or 0: off; 1: on with the library's uniform fraction (a
  // fraction of 1 -- all picks uniform -- is spelt 1.0 like any other and means the library's all the same: ask for it with set_light_sampling(1.0f)); any other
  // number: on with that fraction.
  // FH_LIGHT_RESAMPLING turns on the resampling of those picks by distance and facing (fh_set_light_resampling): unset or 0: off; 1: on with the library's number of
  // candidates; 2, 4, 8 or 16: on with that many (another number is the library's refusal, thrown here).  It implies light sampling, with FH_LIGHT_SAMPLING's
  // fraction where that variable turns it on and the library's otherwise.
  explicit Renderer(const OptixDeviceContext& context) : m_ctx(context)
  {
    if (const char* e = std::getenv("FH_LIGHT_SAMPLING")) {
      char* end = nullptr;
      const float v = std::strtof(e, &end);
      if (end == e || *end != '\0') throw std::runtime_error("FH_LIGHT_SAMPLING: not a number");
      if (v == 1.0f) set_light_sampling();
      else if (v != 0.0f) set_light_sampling(v);
    }
    if (const char* e = std::getenv("FH_LIGHT_RESAMPLING")) {
      char* end = nullptr;
      const long v = std::strtol(e, &end, 10);
      if (end == e || *end != '\0') throw std::runtime_error("FH_LIGHT_RESAMPLING: not a number");
      if (v != 0) {
        int on = 0;
        cwl::check(m_ctx, fh_get_light_sampling(m_ctx, &on, nullptr), "fh_get_light_sampling");
        if (!on) set_light_sampling();
        if (v == 1) set_light_resampling();
        else set_light_resampling(int(v));
      }
    }
    if (const char* e = std::getenv("FH_ENV_SAMPLING")) {
      char* end = nullptr;
      const float v = std::strtof(e, &end);
      if (end == e || *end != '\0') throw std::runtime_error("FH_ENV_SAMPLING: not a number");
      if (v == 1.0f) set_env_sampling();
      else if (v != 0.0f) set_env_sampling(v);
    }
  }
  ~Renderer() noexcept(false) {}

  // OptiX plumbing of the reference (renderer.h:124-352): nothing to build, the kernels live in the library
  void create_module(const std::filesystem::path&) {}
  void create_program_group() {}
  void create_pipeline() {}
  void create_sbt() {}

  // renderer.h:354-432
  void load_scene(const std::filesystem::path& filepath, bool clear = true)
  {
    m_scene.load_model(filepath, clear);
    upload_scene();
  }
  // same upload for a scene assembled in memory
  void load_scene(const Scene& scene)
  {
    m_scene = scene;
    upload_scene();
  }

  void build_gas() {}                                                            // renderer.h:434-496: folded into build_ias
  void build_ias() { cwl::check(m_ctx, fh_bvh_build(m_ctx), "fh_bvh_build"); }  // renderer.h:498-552

  void set_directional_light(const float3& le, const float3& dir, float angle)  // renderer.h:554-567
  {
    const float l[3] = {le.x, le.y, le.z}, d[3] = {dir.x, dir.y, dir.z};
    cwl::check(m_ctx, fh_set_directional_light(m_ctx, l, d, angle), "fh_set_directional_light");
  }
  void set_sky_intensity(float v) { cwl::check(m_ctx, fh_set_sky_intensity(m_ctx, v), "fh_set_sky_intensity"); }
  void load_ibl(const std::filesystem::path& filepath)  // renderer.h:574-581
  {
    const FloatTexture ibl(filepath);
    cwl::check(m_ctx, fh_load_ibl(m_ctx, reinterpret_cast<const float*>(ibl.m_data.data()), ibl.m_width, ibl.m_height), "fh_load_ibl");
  }
  void clear_ibl() { cwl::check(m_ctx, fh_clear_ibl(m_ctx), "fh_clear_ibl"); }  // renderer.h:583-586
  void load_arhosek_sky(float turbidity, float albedo) { cwl::check(m_ctx, fh_load_arhosek_sky(m_ctx, turbidity, albedo), "fh_load_arhosek_sky"); }
  void clear_arhosek_sky() { cwl::check(m_ctx, fh_clear_arhosek_sky(m_ctx), "fh_clear_arhosek_sky"); }
  // importance sampling of the environment for the sky rays (no counterpart in the reference, pt.cu:796-815); without an argument: the library's cosine fraction
  void set_env_sampling() { set_env_sampling(FH_ENV_COSINE_FRACTION_DEFAULT); }
  void set_env_sampling(float cosine_fraction)
  {
    const fh_env_sampling_params p = {cosine_fraction};
    cwl::check(m_ctx, fh_set_env_sampling(m_ctx, &p), "fh_set_env_sampling");
  }
  void clear_env_sampling() { cwl::check(m_ctx, fh_set_env_sampling(m_ctx, nullptr), "fh_set_env_sampling"); }
  // sampling of area lights by power for the area shadow rays (no counterpart in the reference, pt.cu:860-889); without an argument: the library's uniform fraction
  void set_light_sampling() { set_light_sampling(FH_LIGHT_UNIFORM_FRACTION_DEFAULT); }
  void set_light_sampling(float uniform_fraction)
  {
    const fh_light_sampling_params p = {uniform_fraction};
    cwl::check(m_ctx, fh_set_light_sampling(m_ctx, &p), "fh_set_light_sampling");
  }
  void clear_light_sampling() { cwl::check(m_ctx, fh_set_light_sampling(m_ctx, nullptr), "fh_set_light_sampling"); }
  // resampling of those picks by distance and facing from the shaded point; acts while light sampling is on; without an argument: the library's number of candidates
  void set_light_resampling() { set_light_resampling(FH_LIGHT_CANDIDATES_DEFAULT); }
  void set_light_resampling(int candidates)
  {
    const fh_light_resampling_params p = {candidates};
    cwl::check(m_ctx, fh_set_light_resampling(m_ctx, &p), "fh_set_light_resampling");
  }
  void clear_light_resampling() { cwl::check(m_ctx, fh_set_light_resampling(m_ctx, nullptr), "fh_set_light_resampling"); }

  void set_time(float time)  // renderer.h:614-640: animation update, transform re-upload, acceleration-structure rebuild
  {
    m_scene.update_animation(time);
    std::vector<float> o2w, w2o;
    m_scene.transforms_3x4(o2w, w2o);
    if (!o2w.empty()) cwl::check(m_ctx, fh_set_transforms(m_ctx, uint32_t(o2w.size() / 12), o2w.data(), w2o.data()), "fh_set_transforms");
    if (!m_scene.m_skins.empty()) set_joint_matrices(m_scene.joint_matrices_3x4());
    build_ias();
  }
  // skeletal skinning (no counterpart in the reference, whose glTF reader loads no skins; include/fredholm_hip.h: fh_skin_desc).  load_scene and set_time do both for a
  // file with skins; joints / weights: four per vertex of the loaded scene, matrices: row-major 3 x 4 per joint.  Call build_ias after set_joint_matrices
  void set_skin(const std::vector<std::array<uint16_t, 4>>& joints, const std::vector<std::array<float, 4>>& weights, uint32_t n_joints)
  {
    if (joints.size() != weights.size()) throw std::runtime_error("set_skin: joints and weights hold four entries per vertex each");
    const fh_skin_desc d = {uint32_t(joints.size()), n_joints, reinterpret_cast<const uint16_t*>(joints.data()), reinterpret_cast<const float*>(weights.data())};
    cwl::check(m_ctx, fh_set_skin(m_ctx, &d), "fh_set_skin");
  }
  void clear_skin() { cwl::check(m_ctx, fh_set_skin(m_ctx, nullptr), "fh_set_skin"); }
  void set_joint_matrices(const std::vector<float>& m3x4) { cwl::check(m_ctx, fh_set_joint_matrices(m_ctx, uint32_t(m3x4.size() / 12), m3x4.data()), "fh_set_joint_matrices"); }
  void set_resolution(uint32_t width, uint32_t height)  // renderer.h:642-648
  {
    m_width = width;
    m_height = height;
    cwl::check(m_ctx, fh_set_resolution(m_ctx, width, height), "fh_set_resolution");
  }
  void init_render_states() { cwl::check(m_ctx, fh_init_render_states(m_ctx), "fh_init_render_states"); }  // renderer.h:650-655

  // renderer.h:657-734
  void render(const Camera& camera, const float3& bg_color, const RenderLayer& render_layer, uint32_t n_samples, uint32_t max_depth)
  {
    const fh_camera cam = m_scene.m_has_camera_transform ? camera_from(m_scene.m_camera_transform, camera) : camera.to_c();
    const float bg[3] = {bg_color.x, bg_color.y, bg_color.z};
    fh_render_layers layers{reinterpret_cast<float*>(render_layer.beauty), reinterpret_cast<float*>(render_layer.position), render_layer.depth,
                            reinterpret_cast<float*>(render_layer.normal), reinterpret_cast<float*>(render_layer.texcoord), reinterpret_cast<float*>(render_layer.albedo)};
    cwl::check(m_ctx, fh_render(m_ctx, &cam, bg, &layers, n_samples, max_depth, m_seed), "fh_render");
  }
  // not in the reference, which always renders with params.seed = 1 (renderer.h:664): the seed of the following render() calls.  The frames of a sequence whose
  // samples are accumulated over time (Denoiser::Temporal) need different ones; the default 1 keeps every bit.
  void set_seed(uint32_t seed) { m_seed = seed; }
  uint32_t seed() const { return m_seed; }
  // the camera render() hands to the library for `camera`: the scene's own camera transform where it has one (what Denoiser::set_camera wants)
  fh_camera camera_params(const Camera& camera) const { return m_scene.m_has_camera_transform ? camera_from(m_scene.m_camera_transform, camera) : camera.to_c(); }
  void wait_for_completion() { cwl::check(m_ctx, fh_sync(m_ctx), "fh_sync"); }  // renderer.h:736

  // not in the reference: render(n_samples = k) as ONE reference launch of k samples, payload.firsthit quirk included (pt.cu:432-433;
  // rtcamp8 renders 16 per launch, rtcamp8.cpp:183-189), instead of k one-sample launches
  void set_reference_launch_semantics(bool on)
  {
    uint32_t flags = 0;  // (only this bit changes: timing / counting / serial-pass flags set through the C ABI stay as they are)
    cwl::check(m_ctx, fh_get_flags(m_ctx, &flags), "fh_get_flags");
    cwl::check(m_ctx, fh_set_flags(m_ctx, on ? (flags | FH_FLAG_REFERENCE_FIRSTHIT) : (flags & ~FH_FLAG_REFERENCE_FIRSTHIT)), "fh_set_flags");
  }

  // not in the reference: a context over several GPUs (FH_DEVICES, include/fredholm_hip.h: fh_ctx_create_group).  group_size() is 1 for a plain context;
  // set_gather_layers(mask of FH_LAYER_*) names the layers a group brings back from its other members after every render (default: all six)
  uint32_t group_size()
  {
    uint32_t n = 1;
    cwl::check(m_ctx, fh_ctx_group_size(m_ctx, &n), "fh_ctx_group_size");
    return n;
  }
  void set_gather_layers(uint32_t mask) { cwl::check(m_ctx, fh_group_set_gather_layers(m_ctx, mask), "fh_group_set_gather_layers"); }
  // not in the reference: adaptive sampling (include/fredholm_hip.h: fh_set_adaptive_sampling).  A pixel stops at the first count n >= min_samples with
  // n % step == 0 where its relative error estimate is within `threshold`; render(n) then adds at most n samples per pixel.  Set it right after
  // init_render_states / set_resolution, before the first render of the frame.
  void set_adaptive_sampling(float threshold, uint32_t min_samples = 64, uint32_t step = 16, float floor = 0.01f)
  {
    const fh_adaptive_params p{threshold, floor, min_samples, step};
    cwl::check(m_ctx, fh_set_adaptive_sampling(m_ctx, &p), "fh_set_adaptive_sampling");
  }
  void clear_adaptive_sampling() { cwl::check(m_ctx, fh_set_adaptive_sampling(m_ctx, nullptr), "fh_set_adaptive_sampling"); }
  // how the mode decides (fh_set_adaptive_policy): block x block pixel blocks (1, 2, 4, 8) stop together, when all of their pixels are converged; growth 2 tests at
  // b0 * 2^k only (b0: the first multiple of step >= min_samples).  Accepted while the mode is off; like the mode itself, before the first render of the frame.
  void set_adaptive_policy(uint32_t block = 1, uint32_t growth = 1) { cwl::check(m_ctx, fh_set_adaptive_policy(m_ctx, block, growth), "fh_set_adaptive_policy"); }
  void adaptive_policy(uint32_t& block, uint32_t& growth) { cwl::check(m_ctx, fh_get_adaptive_policy(m_ctx, &block, &growth), "fh_get_adaptive_policy"); }
  uint32_t adaptive_next_boundary()  // samples from those requested so far to the next boundary: the call that ends a round (the mode must be on)
  {
    uint32_t n = 0;
    cwl::check(m_ctx, fh_adaptive_next_boundary(m_ctx, &n), "fh_adaptive_next_boundary");
    return n;
  }
  void get_sample_counts(cwl::CUDABuffer<uint32_t>& counts)  // width * height
  {
    cwl::check(m_ctx, fh_get_sample_counts(m_ctx, counts.get_device_ptr()), "fh_get_sample_counts");
  }
  void get_luminance_moments(cwl::CUDABuffer<float2>& moments)  // width * height (m1, m2); adaptive sampling must be on
  {
    cwl::check(m_ctx, fh_get_luminance_moments(m_ctx, reinterpret_cast<float*>(moments.get_device_ptr())), "fh_get_luminance_moments");
  }
  uint32_t active_pixel_count()  // synchronising: owned pixels the next render would sample
  {
    uint32_t n = 0;
    cwl::check(m_ctx, fh_active_pixel_count(m_ctx, &n), "fh_active_pixel_count");
    return n;
  }

 private:
  static fh_camera camera_from(const Mat4& m, const Camera& camera)
  {
    fh_camera c = camera.to_c();
    for (int r = 0; r < 3; ++r)
      for (int col = 0; col < 4; ++col) c.transform[4 * r + col] = m[col][r];
    return c;
  }
  void upload_scene()
  {
    if (!m_scene.is_valid()) throw std::runtime_error("invalid scene");
    std::vector<float> o2w, w2o;
    m_scene.transforms_3x4(o2w, w2o);
    fh_scene_desc d{};
    d.n_vertices = uint32_t(m_scene.m_vertices.size());
    d.vertices = reinterpret_cast<const float*>(m_scene.m_vertices.data());
    d.normals = reinterpret_cast<const float*>(m_scene.m_normals.data());
    d.texcoords = reinterpret_cast<const float*>(m_scene.m_texcoords.data());
    d.n_faces = uint32_t(m_scene.m_indices.size());
    d.indices = reinterpret_cast<const uint32_t*>(m_scene.m_indices.data());
    d.material_ids = m_scene.m_material_ids.data();
    d.instance_ids = m_scene.m_instance_ids.empty() ? nullptr : m_scene.m_instance_ids.data();
    d.n_materials = uint32_t(m_scene.m_materials.size());
    d.materials = reinterpret_cast<const fh_material*>(m_scene.m_materials.data());
    d.n_instances = uint32_t(m_scene.m_transforms.size());
    d.object_to_world = o2w.empty() ? nullptr : o2w.data();
    d.world_to_object = w2o.empty() ? nullptr : w2o.data();
    std::vector<fh_texture_desc> tex;  // renderer.h:414-424: COLOR textures are sRGB-decoded by the texture unit
    for (const Texture& t : m_scene.m_textures)
      tex.push_back(fh_texture_desc{t.m_width, t.m_height, reinterpret_cast<const uint8_t*>(t.m_data.data()), t.m_texture_type == TextureType::COLOR ? 1 : 0});
    d.n_textures = uint32_t(tex.size());
    d.textures = tex.empty() ? nullptr : tex.data();
    cwl::check(m_ctx, fh_scene_upload(m_ctx, &d), "fh_scene_upload");
    if (!m_scene.m_skins.empty()) {  // the skin, and the pose the nodes have now
      set_skin(m_scene.m_joints, m_scene.m_weights, m_scene.n_joints());
      set_joint_matrices(m_scene.joint_matrices_3x4());
    }
  }
  fh_ctx* m_ctx = nullptr;
  uint32_t m_width = 0, m_height = 0;
  uint32_t m_seed = 1;  // params.seed = 1, renderer.h:664
  Scene m_scene;
};

}  // namespace fredholm
