// rtcamp.cpp -- headless animation batch driver shaped like the reference's app/rtcamp8.cpp:47-303, against the drop-in headers
// of include/: for every frame { clear layers, init_render_states, set_time, render, (denoise: pass-through), post-process,
// copy to host } on a render thread, while a second thread converts finished frames to 8-bit and writes them as PNG files.
//
//   rtcamp --scene a.obj [--scene b.gltf ...] [--out DIR] [--width W --height H --spp N --depth D]
//          [--fps F --max-time T] [--bloom] [--sun] [--sky] [--ibl env.hdr] [--fov deg --F f --focus d]
//          [--noise-threshold T [--min-spp M --adaptive-step S]]   (adaptive sampling: --spp is the per-pixel cap, the frame renders in calls of S samples
//                                                                    until no pixel is active; prints the frame's mean spp)
//          [--adaptive-block G --adaptive-growth K]   (with --noise-threshold: G x G pixel blocks (1, 2, 4, 8) stop together; K = 2 tests at M, 2M, 4M ... only,
//                                                       and the frame renders in calls that end on those boundaries)
//          [--denoiser atrous|guided|temporal|temporal-motion|temporal-response|temporal-motion-response|temporal-response-noise|temporal-motion-response-noise] [--denoise-gamma G] [--denoise-kappa K] [--denoise-temporal-moments [--denoise-min-history H]]   (atrous, the default: fh_denoise; guided: the variance-guided filter on the position and depth layers too, and on the
//                                         luminance moments and sample counts whenever --noise-threshold is on; temporal: that filter behind temporal accumulation --
//                                         frame i renders with seed 1 + i and the denoiser is told the frame's camera; every other mode keeps seed 1; temporal-motion: temporal with
//                                         per-instance motion vectors, so that the key-framed objects keep their history too; -response: either of the two with
//                                         the history clipped to the frame's local colour box of +- G standard deviations (default 1), so that moving lights do not lag;
//                                         -response-noise: that with the history also clamped to the pixel's own colour +- K measured standard deviations (default 6) --
//                                         this step needs the luminance moments, so without --noise-threshold it does nothing;
//                                         --denoise-temporal-moments, with every temporal* denoiser: the history also keeps the luminance moments, and a frame without
//                                         --noise-threshold takes its per-pixel variance from them once a pixel's history is H frames long (default 2))
//          [--auto-exposure [--exposure-key K] [--exposure-comp EV] [--exposure-speed UP DOWN] [--bloom-relative]]   (the tone map's exposure is metered from every frame's
//                                         luminance histogram in place of ISO: the mean log2 luminance of the middle ranks is mapped to K (default 0.18), shifted by EV stops, and
//                                         followed at UP / DOWN per second (default 3 / 1) with a frame time of 1 / fps; --bloom-relative: the bloom threshold compares exposed luminance)
//          [--local-exposure [--local-highlights H] [--local-shadows S] [--local-sigma R] [--local-passes P]]   (the tone map's exposure varies over the frame: an
//                                         edge-aware base layer of log-luminance loses the share H of its distance above and S below mid-grey (default 0.5 / 0.5); R: the range
//                                         sigma of the edge stop in stops (default 1); P: a-trous passes on the quarter-resolution image, 1 .. 6 (default 4))
//          [--env-sampling [--env-cosine-fraction B]]   (the sky rays are drawn from a table of the environment's luminance -- the --ibl image, the --sky dome -- mixed with
//                                         the cosine lobe at share B in [0, 1) (default: the library's); without it they are cosine-distributed as in the reference)
//          [--light-sampling [--light-uniform-fraction U]]   (the emitter of every area shadow ray is picked by power -- area x luminance of its emission -- mixed with the
//                                         uniform pick at share U in (0, 1] (default: the library's); without it the pick is uniform as in the reference)
//          [--light-resampling [M]]   (with --light-sampling: M candidates of the table -- 1, 2, 4, 8 or 16, default: the library's -- are drawn for every area shadow ray
//                                         and one is chosen by its distance and facing from the shaded point)
//          [--devices 0,1,...]   (every frame split by pixel tile across these GPUs: the same meaning as the FH_DEVICES variable, and the flag wins; an index may repeat)
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <mutex>
#include <queue>
#include <string>
#include <thread>
#include <vector>

#include "cwl/buffer.h"
#include "cwl/util.h"
#include "fredholm/camera.h"
#include "fredholm/denoiser.h"
#include "fredholm/image_io.h"
#include "fredholm/renderer.h"
#include "kernels/post-process.h"
#include "optwl/optwl.h"

int main(int argc, char** argv)
{
  std::vector<std::string> scene_files;
  std::string out_dir = "output", ibl;
  int width = 1920, height = 1080, n_spp = 16, max_depth = 5;
  float fps = 24.0f, max_time = 9.5f, fov_deg = 60.0f, F = 100.0f, focus = 8.0f;
  bool bloom = false, sun = false, sky = false, reference_launches = false;
  float noise_threshold = -1.0f;  // --noise-threshold T: adaptive sampling, --spp becomes the per-pixel cap
  int min_spp = 64, adaptive_step = 16, adaptive_block = 1, adaptive_growth = 1;
  std::string denoiser_name = "atrous";  // --denoiser
  float denoise_gamma = 1.0f;            // --denoise-gamma (with a -response denoiser only)
  bool gamma_given = false;
  float denoise_kappa = 6.0f;            // --denoise-kappa (with a -response-noise denoiser only)
  bool kappa_given = false;
  bool temporal_moments = false;         // --denoise-temporal-moments (with a temporal* denoiser only)
  float denoise_min_history = 2.0f;      // --denoise-min-history (with --denoise-temporal-moments only)
  bool min_history_given = false;
  bool auto_exposure = false, bloom_relative = false;  // --auto-exposure, --bloom-relative
  AutoExposureParams exposure;                         // --exposure-key, --exposure-comp, --exposure-speed (with --auto-exposure only)
  const char* exposure_flag = nullptr;                 // the first of those flags that was given
  bool local_exposure = false;                         // --local-exposure
  LocalExposureParams local;                           // --local-highlights, --local-shadows, --local-sigma, --local-passes (with --local-exposure only)
  const char* local_flag = nullptr;                    // the first of those flags that was given
  bool env_sampling = false, env_fraction_given = false;  // --env-sampling, --env-cosine-fraction (with --env-sampling only)
  float env_fraction = FH_ENV_COSINE_FRACTION_DEFAULT;
  bool light_sampling = false, light_fraction_given = false;  // --light-sampling, --light-uniform-fraction (with --light-sampling only)
  float light_fraction = FH_LIGHT_UNIFORM_FRACTION_DEFAULT;
  bool light_resampling = false;  // --light-resampling [M] (with --light-sampling only)
  int light_candidates = FH_LIGHT_CANDIDATES_DEFAULT;
  std::vector<int> devices;  // --devices: empty = FH_DEVICES, or device 0
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    auto next = [&]() -> const char* { if (i + 1 >= argc) { std::fprintf(stderr, "missing value after %s\n", a.c_str()); std::exit(2); } return argv[++i]; };
    if (a == "--scene") scene_files.push_back(next());
    else if (a == "--out") out_dir = next();
    else if (a == "--width") width = std::atoi(next());
    else if (a == "--height") height = std::atoi(next());
    else if (a == "--spp") n_spp = std::atoi(next());
    else if (a == "--depth") max_depth = std::atoi(next());
    else if (a == "--fps") fps = float(std::atof(next()));
    else if (a == "--max-time") max_time = float(std::atof(next()));
    else if (a == "--fov") fov_deg = float(std::atof(next()));
    else if (a == "--F") F = float(std::atof(next()));
    else if (a == "--focus") focus = float(std::atof(next()));
    else if (a == "--ibl") ibl = next();
    else if (a == "--bloom") bloom = true;
    else if (a == "--sun") sun = true;
    else if (a == "--sky") sky = true;
    else if (a == "--reference-launches") reference_launches = true;  // one launch of --spp samples per frame exactly as the reference computes it (firsthit quirk)
    else if (a == "--noise-threshold") noise_threshold = float(std::atof(next()));
    else if (a == "--min-spp") min_spp = std::atoi(next());
    else if (a == "--adaptive-step") adaptive_step = std::atoi(next());
    else if (a == "--adaptive-block") adaptive_block = std::atoi(next());
    else if (a == "--adaptive-growth") adaptive_growth = std::atoi(next());
    else if (a == "--denoiser") denoiser_name = next();
    else if (a == "--denoise-gamma") { denoise_gamma = float(std::atof(next())); gamma_given = true; }
    else if (a == "--denoise-kappa") { denoise_kappa = float(std::atof(next())); kappa_given = true; }
    else if (a == "--denoise-temporal-moments") temporal_moments = true;
    else if (a == "--denoise-min-history") { denoise_min_history = float(std::atof(next())); min_history_given = true; }
    else if (a == "--auto-exposure") auto_exposure = true;
    else if (a == "--local-exposure") local_exposure = true;
    else if (a == "--local-highlights") { local.highlights = float(std::atof(next())); if (!local_flag) local_flag = "--local-highlights"; }
    else if (a == "--local-shadows") { local.shadows = float(std::atof(next())); if (!local_flag) local_flag = "--local-shadows"; }
    else if (a == "--local-sigma") { local.sigma_range = float(std::atof(next())); if (!local_flag) local_flag = "--local-sigma"; }
    else if (a == "--local-passes") { local.passes = uint32_t(std::atoi(next())); if (!local_flag) local_flag = "--local-passes"; }
    else if (a == "--env-sampling") env_sampling = true;
    else if (a == "--env-cosine-fraction") { env_fraction = float(std::atof(next())); env_fraction_given = true; }
    else if (a == "--light-sampling") light_sampling = true;
    else if (a == "--light-uniform-fraction") { light_fraction = float(std::atof(next())); light_fraction_given = true; }
    else if (a == "--light-resampling") {
      light_resampling = true;
      if (i + 1 < argc && argv[i + 1][0] != '-') {  // the count is optional
        char* end = nullptr;
        const long m = std::strtol(argv[++i], &end, 10);
        light_candidates = (*end == '\0' && end != argv[i] && m >= 0 && m <= 1000) ? int(m) : 0;
      }
    }
    else if (a == "--exposure-key") { exposure.key = float(std::atof(next())); if (!exposure_flag) exposure_flag = "--exposure-key"; }
    else if (a == "--exposure-comp") { exposure.compensation_ev = float(std::atof(next())); if (!exposure_flag) exposure_flag = "--exposure-comp"; }
    else if (a == "--exposure-speed") { exposure.speed_up = float(std::atof(next())); exposure.speed_down = float(std::atof(next())); if (!exposure_flag) exposure_flag = "--exposure-speed"; }
    else if (a == "--bloom-relative") { bloom_relative = true; if (!exposure_flag) exposure_flag = "--bloom-relative"; }
    else if (a == "--devices") {
      try { devices = cwl::parse_device_list(next(), "--devices"); } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 2; }
    }
    else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); return 2; }
  }
  if (scene_files.empty()) { std::fprintf(stderr, "usage: %s --scene file.obj|file.gltf [--scene ...] [--out DIR] [--width W --height H --spp N --depth D] [--fps F --max-time T] [--bloom] [--sun] [--sky] [--ibl env.hdr] [--noise-threshold T [--min-spp M --adaptive-step S --adaptive-block G --adaptive-growth K]] [--denoiser atrous|guided|temporal|temporal-motion|temporal-response|temporal-motion-response|temporal-response-noise|temporal-motion-response-noise] [--denoise-gamma G] [--denoise-kappa K] [--denoise-temporal-moments [--denoise-min-history H]] [--auto-exposure [--exposure-key K] [--exposure-comp EV] [--exposure-speed UP DOWN] [--bloom-relative]] [--local-exposure [--local-highlights H] [--local-shadows S] [--local-sigma R] [--local-passes P]] [--env-sampling [--env-cosine-fraction B]] [--light-sampling [--light-uniform-fraction U] [--light-resampling [M]]] [--devices 0,1,...]\n", argv[0]); return 2; }
  if (noise_threshold >= 0.0f && (min_spp < 2 || adaptive_step < 1)) { std::fprintf(stderr, "--min-spp must be >= 2 and --adaptive-step >= 1\n"); return 2; }
  if (adaptive_block != 1 && adaptive_block != 2 && adaptive_block != 4 && adaptive_block != 8) { std::fprintf(stderr, "--adaptive-block must be 1, 2, 4 or 8\n"); return 2; }
  if (adaptive_growth != 1 && adaptive_growth != 2) { std::fprintf(stderr, "--adaptive-growth must be 1 or 2\n"); return 2; }
  const bool temporal_noise = denoiser_name == "temporal-response-noise" || denoiser_name == "temporal-motion-response-noise";
  const bool temporal_response = denoiser_name == "temporal-response" || denoiser_name == "temporal-motion-response" || temporal_noise;
  const bool temporal_motion = denoiser_name == "temporal-motion" || denoiser_name == "temporal-motion-response" || denoiser_name == "temporal-motion-response-noise";
  const bool temporal = denoiser_name == "temporal" || temporal_motion || temporal_response;
  if (denoiser_name != "atrous" && denoiser_name != "guided" && denoiser_name != "temporal" && !temporal_motion && !temporal_response) { std::fprintf(stderr, "--denoiser must be atrous, guided, temporal, temporal-motion, temporal-response, temporal-motion-response, temporal-response-noise or temporal-motion-response-noise\n"); return 2; }
  if (!(denoise_gamma > 0.0f) || !std::isfinite(denoise_gamma)) { std::fprintf(stderr, "--denoise-gamma must be finite and > 0\n"); return 2; }
  if (!(denoise_kappa > 0.0f) || !std::isfinite(denoise_kappa)) { std::fprintf(stderr, "--denoise-kappa must be finite and > 0\n"); return 2; }
  if (kappa_given && !temporal_noise) { std::fprintf(stderr, "--denoise-kappa goes with --denoiser temporal-response-noise or temporal-motion-response-noise\n"); return 2; }
  if (gamma_given && !temporal_response) { std::fprintf(stderr, "--denoise-gamma goes with --denoiser temporal-response or temporal-motion-response\n"); return 2; }
  if (!(denoise_min_history >= 1.0f) || !std::isfinite(denoise_min_history)) { std::fprintf(stderr, "--denoise-min-history must be finite and >= 1\n"); return 2; }
  if (temporal_moments && !temporal) { std::fprintf(stderr, "--denoise-temporal-moments goes with a temporal --denoiser\n"); return 2; }
  if (min_history_given && !temporal_moments) { std::fprintf(stderr, "--denoise-min-history goes with --denoise-temporal-moments\n"); return 2; }
  if (exposure_flag && !auto_exposure) { std::fprintf(stderr, "%s goes with --auto-exposure\n", exposure_flag); return 2; }
  if (!(exposure.key > 0.0f) || !std::isfinite(exposure.key)) { std::fprintf(stderr, "--exposure-key must be finite and > 0\n"); return 2; }
  if (!std::isfinite(exposure.compensation_ev)) { std::fprintf(stderr, "--exposure-comp must be finite\n"); return 2; }
  if (!(exposure.speed_up >= 0.0f) || !std::isfinite(exposure.speed_up) || !(exposure.speed_down >= 0.0f) || !std::isfinite(exposure.speed_down)) { std::fprintf(stderr, "--exposure-speed takes two finite rates >= 0\n"); return 2; }
  if (local_flag && !local_exposure) { std::fprintf(stderr, "%s goes with --local-exposure\n", local_flag); return 2; }
  if (!(local.highlights >= 0.0f && local.highlights <= 1.0f)) { std::fprintf(stderr, "--local-highlights must be in [0, 1]\n"); return 2; }
  if (!(local.shadows >= 0.0f && local.shadows <= 1.0f)) { std::fprintf(stderr, "--local-shadows must be in [0, 1]\n"); return 2; }
  if (!(local.sigma_range > 0.0f) || !std::isfinite(local.sigma_range)) { std::fprintf(stderr, "--local-sigma must be finite and > 0\n"); return 2; }
  if (local.passes < 1u || local.passes > 6u) { std::fprintf(stderr, "--local-passes must be 1 .. 6\n"); return 2; }
  if (env_fraction_given && !env_sampling) { std::fprintf(stderr, "--env-cosine-fraction goes with --env-sampling\n"); return 2; }
  if (!(env_fraction >= 0.0f && env_fraction < 1.0f)) { std::fprintf(stderr, "--env-cosine-fraction must be in [0, 1)\n"); return 2; }
  if (light_fraction_given && !light_sampling) { std::fprintf(stderr, "--light-uniform-fraction goes with --light-sampling\n"); return 2; }
  if (!(light_fraction > 0.0f && light_fraction <= 1.0f)) { std::fprintf(stderr, "--light-uniform-fraction must be in (0, 1]\n"); return 2; }
  if (light_resampling && !light_sampling) { std::fprintf(stderr, "--light-resampling goes with --light-sampling\n"); return 2; }
  if (light_candidates != 1 && light_candidates != 2 && light_candidates != 4 && light_candidates != 8 && light_candidates != 16) { std::fprintf(stderr, "--light-resampling takes 1, 2, 4, 8 or 16\n"); return 2; }
  if (auto_exposure && !(fps > 0.0f)) { std::fprintf(stderr, "--auto-exposure needs --fps > 0\n"); return 2; }
  const bool guided = denoiser_name == "guided" || temporal;  // (temporal: the same guides)
  const float time_step = 1.0f / fps;
  try {
    std::filesystem::create_directories(out_dir);
    if (!devices.empty()) cwl::check(nullptr, cwl::create_context(devices, &cwl::default_context()), "--devices");  // (before anything asks for the process-wide context)
    optwl::Context context;
    fredholm::Renderer renderer(context.get_context());
    renderer.set_gather_layers(FH_LAYER_BEAUTY | FH_LAYER_NORMAL | FH_LAYER_ALBEDO | (guided ? FH_LAYER_POSITION | FH_LAYER_DEPTH : 0u));  // what the denoise / post / PNG chain below reads (a plain context ignores it)
    if (renderer.group_size() > 1) std::printf("rendering on a group of %u members\n", renderer.group_size());
    renderer.create_module("pt.ptx");
    renderer.create_program_group();
    renderer.create_pipeline();
    renderer.set_resolution(uint32_t(width), uint32_t(height));
    if (reference_launches) renderer.set_reference_launch_semantics(true);
    if (env_sampling) renderer.set_env_sampling(env_fraction);
    if (light_sampling) renderer.set_light_sampling(light_fraction);
    if (light_resampling) renderer.set_light_resampling(light_candidates);

    const size_t n_px = size_t(width) * size_t(height);
    cwl::CUDABuffer<float4> layer_beauty(n_px), layer_position(n_px), layer_normal(n_px), layer_texcoord(n_px), layer_albedo(n_px), layer_denoised(n_px);
    cwl::CUDABuffer<float> layer_depth(n_px);
    cwl::CUDABuffer<float4> layer_denoised_pp(n_px), denoised_high_luminance(n_px), denoised_temp(n_px);
    // the post-process grid is floor(w/16) x floor(h/16) tiles (post-process.cu:9-11): border pixels of these buffers are never written
    // but the bloom taps read them, so give them a defined value once
    layer_denoised.clear(); layer_denoised_pp.clear(); denoised_high_luminance.clear(); denoised_temp.clear();
    fredholm::Denoiser denoiser(context.get_context(), uint32_t(width), uint32_t(height), layer_beauty.get_device_ptr(), layer_normal.get_device_ptr(), layer_albedo.get_device_ptr(),
                                layer_denoised.get_device_ptr(), false);

    for (size_t k = 0; k < scene_files.size(); ++k) renderer.load_scene(scene_files[k], k == 0);  // rtcamp8.cpp:114-115
    renderer.build_gas();
    renderer.build_ias();
    renderer.create_sbt();

    fredholm::Camera camera;
    camera.m_fov = fov_deg / 180.0f * float(M_PI);
    camera.m_F = F;
    camera.m_focus = focus;
    cwl::CUDABuffer<uint32_t> sample_counts(n_px);  // (--noise-threshold: the per-pixel counts a frame ends with)
    cwl::CUDABuffer<float2> luminance_moments(guided && noise_threshold >= 0.0f ? n_px : 1);  // (and, for the guided denoiser, the moments they go with)
    if (guided) {
      denoiser.set_mode(temporal ? fredholm::Denoiser::Temporal : fredholm::Denoiser::Guided);
      if (temporal_motion) denoiser.set_motion(true);
      if (temporal_response) denoiser.set_response(true, denoise_gamma);
      if (temporal_noise) denoiser.set_response_noise(true, denoise_kappa);
      if (temporal_moments) denoiser.set_temporal_moments(true, denoise_min_history);
      if (noise_threshold >= 0.0f) denoiser.set_guides(layer_position.get_device_ptr(), layer_depth.get_device_ptr(), luminance_moments.get_device_ptr(), sample_counts.get_device_ptr());
      else denoiser.set_guides(layer_position.get_device_ptr(), layer_depth.get_device_ptr());
    }
    fredholm::RenderLayer render_layer{layer_beauty.get_device_ptr(), layer_position.get_device_ptr(), layer_depth.get_device_ptr(), layer_normal.get_device_ptr(),
                                       layer_texcoord.get_device_ptr(), layer_albedo.get_device_ptr()};
    if (auto_exposure) {
      exposure.frame_time = time_step;
      exposure.bloom_relative = bloom_relative;
      set_auto_exposure(&exposure);
    }
    if (local_exposure) set_local_exposure(&local);
    if (sun) renderer.set_directional_light(make_float3(20, 20, 20), make_float3(-0.1f, 1, 0.1f), 1.0f);  // rtcamp8.cpp:133-134
    if (sky) renderer.load_arhosek_sky(3.0f, 0.3f);                                                       // rtcamp8.cpp:137
    if (!ibl.empty()) renderer.load_ibl(ibl);

    std::queue<std::pair<int, std::vector<float4>>> queue;
    std::mutex queue_mutex;
    bool render_finished = false;
    std::string failure;

    std::thread render_thread([&] {
      try {
        int frame_idx = 0;
        float time = 0.0f;
        for (;;) {
          if (time > max_time) break;
          const auto t0 = std::chrono::steady_clock::now();
          layer_beauty.clear(); layer_position.clear(); layer_normal.clear(); layer_depth.clear(); layer_texcoord.clear(); layer_albedo.clear();
          renderer.init_render_states();
          renderer.set_time(time);
          if (temporal) {  // samples of its own for every frame, and the camera the history is reprojected with
            renderer.set_seed(1u + uint32_t(frame_idx));
            denoiser.set_camera(renderer.camera_params(camera));
          }
          if (noise_threshold < 0.0f) {
            renderer.render(camera, make_float3(0, 0, 0), render_layer, uint32_t(n_spp), uint32_t(max_depth));
          } else {  // calls of --adaptive-step samples until every pixel has stopped or reached --spp
            renderer.set_adaptive_policy(uint32_t(adaptive_block), uint32_t(adaptive_growth));
            renderer.set_adaptive_sampling(noise_threshold, uint32_t(min_spp), uint32_t(adaptive_step));
            for (int done = 0; done < n_spp;) {
              // (growth 2: a call that ended between two boundaries would end a round there, and the schedule would buy nothing)
              const uint32_t call = adaptive_growth == 2 ? renderer.adaptive_next_boundary() : uint32_t(adaptive_step);
              const int k = uint32_t(n_spp - done) < call ? n_spp - done : int(call);
              renderer.render(camera, make_float3(0, 0, 0), render_layer, uint32_t(k), uint32_t(max_depth));
              done += k;
              if (done < n_spp && renderer.active_pixel_count() == 0) break;
            }
            renderer.get_sample_counts(sample_counts);
            if (guided) renderer.get_luminance_moments(luminance_moments);
            std::vector<uint32_t> counts;
            sample_counts.copy_from_device_to_host(counts);
            double sum = 0.0;
            for (uint32_t c : counts) sum += c;
            std::printf("[Adaptive] frame %d: mean spp %.1f of at most %d\n", frame_idx, sum / double(counts.size()), n_spp);
          }
          CUDA_SYNC_CHECK();
          denoiser.denoise();
          PostProcessParams params{bloom, 2.0f, 5.0f, 80.0f, 1.0f};  // rtcamp8.cpp:57-60,207-212
          post_process_kernel_launch(layer_denoised.get_device_ptr(), denoised_high_luminance.get_device_ptr(), denoised_temp.get_device_ptr(), width, height, params,
                                     layer_denoised_pp.get_device_ptr());
          CUDA_SYNC_CHECK();
          std::vector<float4> image;
          layer_denoised_pp.copy_from_device_to_host(image);
          const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
          std::printf("[Render] frame %d, time %.4f: %.2f ms\n", frame_idx, double(time), ms);
          { std::lock_guard<std::mutex> lock(queue_mutex); queue.push({frame_idx, std::move(image)}); }
          frame_idx++;
          time += time_step;
        }
      } catch (const std::exception& e) {
        std::lock_guard<std::mutex> lock(queue_mutex);
        failure = e.what();
      }
      std::lock_guard<std::mutex> lock(queue_mutex);
      render_finished = true;
    });

    std::thread save_thread([&] {
      for (;;) {
        int frame_idx = -1;
        std::vector<float4> image;
        {
          std::lock_guard<std::mutex> lock(queue_mutex);
          if (queue.empty()) { if (render_finished) break; }
          else { frame_idx = queue.front().first; image = std::move(queue.front().second); queue.pop(); }
        }
        if (frame_idx < 0) { std::this_thread::sleep_for(std::chrono::milliseconds(1)); continue; }
        std::vector<uint8_t> rgba(image.size() * 4);
        for (size_t i = 0; i < image.size(); ++i) {  // rtcamp8.cpp:266-279
          const float4& v = image[i];
          rgba[4 * i] = static_cast<unsigned char>(std::fmin(std::fmax(255.0f * v.x, 0.0f), 255.0f));
          rgba[4 * i + 1] = static_cast<unsigned char>(std::fmin(std::fmax(255.0f * v.y, 0.0f), 255.0f));
          rgba[4 * i + 2] = static_cast<unsigned char>(std::fmin(std::fmax(255.0f * v.z, 0.0f), 255.0f));
          rgba[4 * i + 3] = 255;
        }
        const std::filesystem::path file = std::filesystem::path(out_dir) / (std::to_string(frame_idx) + ".png");
        fredholm::image_io::write_png_rgba8(file, width, height, rgba.data());
        std::printf("[Image Write] %s saved\n", file.generic_string().c_str());
      }
    });

    render_thread.join();
    save_thread.join();
    if (!failure.empty()) throw std::runtime_error(failure);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
