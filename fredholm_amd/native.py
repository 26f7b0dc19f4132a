"""ctypes binding of libfredholm_hip.so (C ABI: include/fredholm_hip.h)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FH_LIB") or os.path.join(_HERE, "libfredholm_hip.so")  # FH_LIB: developer override for A/B runs

FH_OK = 0
FLAG_TIME_KERNELS = 1
FLAG_COUNT_TRAVERSAL = 2
FLAG_SERIAL_PASSES = 8
FLAG_ROOT_START = 16  # (measurements) every ray starts its traversal at the root
# gather mask of a group (fh_group_set_gather_layers): bit k = layer k of RenderLayer.NAMES
LAYER_BEAUTY, LAYER_POSITION, LAYER_DEPTH, LAYER_NORMAL, LAYER_TEXCOORD, LAYER_ALBEDO, LAYER_ALL = 1, 2, 4, 8, 16, 32, 63
FLAG_REFERENCE_FIRSTHIT = 4  # one fh_render(n_samples = k) = ONE reference launch of k samples, firsthit quirk included (pt.cu:432-433)

MATERIAL_DTYPE = np.dtype([
    ("diffuse", "f4"), ("base_color", "f4", 3), ("base_color_texture_id", "i4"), ("diffuse_roughness", "f4"),
    ("specular", "f4"), ("specular_color", "f4", 3), ("specular_color_texture_id", "i4"), ("specular_roughness", "f4"),
    ("specular_roughness_texture_id", "i4"),
    ("metalness", "f4"), ("metalness_texture_id", "i4"), ("metallic_roughness_texture_id", "i4"),
    ("coat", "f4"), ("coat_texture_id", "i4"), ("coat_color", "f4", 3), ("coat_roughness", "f4"), ("coat_roughness_texture_id", "i4"),
    ("transmission", "f4"), ("transmission_color", "f4", 3),
    ("sheen", "f4"), ("sheen_color", "f4", 3), ("sheen_roughness", "f4"),
    ("subsurface", "f4"), ("subsurface_color", "f4", 3),
    ("thin_walled", "f4"),
    ("emission", "f4"), ("emission_color", "f4", 3), ("emission_texture_id", "i4"),
    ("heightmap_texture_id", "i4"), ("normalmap_texture_id", "i4"), ("alpha_texture_id", "i4"),
])
assert MATERIAL_DTYPE.itemsize == 180


def default_materials(n):
    """n materials with the reference's defaults (fredholm/include/fredholm/shared.h:100-142)."""
    m = np.zeros(n, dtype=MATERIAL_DTYPE)
    m["diffuse"] = 1.0
    m["base_color"] = 1.0
    m["specular"] = 1.0
    m["specular_color"] = 1.0
    m["specular_roughness"] = 0.2
    m["coat_color"] = 1.0
    m["coat_roughness"] = 0.1
    m["transmission_color"] = 1.0
    m["sheen_color"] = 1.0
    m["sheen_roughness"] = 0.3
    m["subsurface_color"] = 1.0
    for k in MATERIAL_DTYPE.names:
        if k.endswith("texture_id"):
            m[k] = -1
    return m


class TextureDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("rgba8", C.c_void_p), ("srgb", C.c_int32)]


class SceneDesc(C.Structure):
    _fields_ = [("n_vertices", C.c_uint32), ("vertices", C.c_void_p), ("normals", C.c_void_p), ("texcoords", C.c_void_p),
                ("n_faces", C.c_uint32), ("indices", C.c_void_p), ("material_ids", C.c_void_p), ("instance_ids", C.c_void_p),
                ("n_materials", C.c_uint32), ("materials", C.c_void_p),
                ("n_instances", C.c_uint32), ("object_to_world", C.c_void_p), ("world_to_object", C.c_void_p),
                ("n_textures", C.c_uint32), ("textures", C.c_void_p)]


class CameraC(C.Structure):
    _fields_ = [("transform", C.c_float * 12), ("fov", C.c_float), ("F", C.c_float), ("focus", C.c_float)]


class LayersC(C.Structure):
    _fields_ = [("beauty", C.c_void_p), ("position", C.c_void_p), ("depth", C.c_void_p), ("normal", C.c_void_p),
                ("texcoord", C.c_void_p), ("albedo", C.c_void_p)]


class PostParamsC(C.Structure):
    _fields_ = [("use_bloom", C.c_int32), ("bloom_threshold", C.c_float), ("bloom_sigma", C.c_float), ("ISO", C.c_float),
                ("chromatic_aberration", C.c_float)]


class StatsC(C.Structure):
    _fields_ = [("render_ms", C.c_double), ("trace_closest_ms", C.c_double), ("trace_shadow_ms", C.c_double), ("shade_ms", C.c_double),
                ("n_closest_launches", C.c_uint64), ("n_shadow_launches", C.c_uint64),
                ("rays_closest", C.c_uint64), ("rays_shadow", C.c_uint64),
                ("nodes_closest", C.c_uint64), ("tris_closest", C.c_uint64), ("nodes_shadow", C.c_uint64), ("tris_shadow", C.c_uint64),
                ("paths", C.c_uint64), ("bvh_build_ms", C.c_double), ("bvh_nodes", C.c_uint64), ("bvh_node_bytes", C.c_uint64),
                ("bvh_tri_bytes", C.c_uint64),
                ("wave_node_steps_closest", C.c_uint64), ("wave_tri_steps_closest", C.c_uint64), ("wave_node_steps_shadow", C.c_uint64),
                ("wave_tri_steps_shadow", C.c_uint64), ("hist_nodes_closest", C.c_uint64 * 8), ("hist_nodes_shadow", C.c_uint64 * 8), ("tail_ms", C.c_double),
                ("generate_ms", C.c_double), ("accumulate_ms", C.c_double), ("queue_ms", C.c_double),
                ("n_generate_launches", C.c_uint64), ("n_accumulate_launches", C.c_uint64), ("n_shade_launches", C.c_uint64), ("n_tail_launches", C.c_uint64),
                ("shaded_hits", C.c_uint64), ("bvh_depth", C.c_uint64), ("post_ms", C.c_double), ("n_post_launches", C.c_uint64),
                ("clk_cycles_closest", C.c_uint64), ("clk_ticks_closest", C.c_uint64), ("clk_cycles_shadow", C.c_uint64), ("clk_ticks_shadow", C.c_uint64),
                ("n_passes", C.c_uint64), ("sky_pixel_samples", C.c_uint64), ("div_range_violations", C.c_uint64)]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if hasattr(getattr(self, k), "__len__") else getattr(self, k)) for k, _ in self._fields_}


class FredholmError(RuntimeError):
    pass


# every symbol include/fredholm_hip.h and include/fredholm_hip_test.h (the known-answer hooks of the parity tests) declare (tests check the library exports all of them)
EXPORTS = [
    "fh_ctx_create", "fh_ctx_destroy", "fh_last_error", "fh_set_flags", "fh_get_flags", "fh_set_path_pool", "fh_path_pool_bytes", "fh_path_pool_allocated", "fh_alpha_face_counts", "fh_alpha_cell_counts", "fh_set_tail_depth", "fh_scene_upload", "fh_bvh_build", "fh_set_transforms",
    "fh_scene_n_lights", "fh_set_directional_light", "fh_clear_directional_light", "fh_set_sky_intensity", "fh_load_arhosek_sky",
    "fh_clear_arhosek_sky", "fh_load_ibl", "fh_clear_ibl", "fh_set_resolution", "fh_init_render_states", "fh_set_tile_shard", "fh_owned_pixel_count",
    "fh_pack_owned", "fh_unpack_shard", "fh_unpack_shards", "fh_render", "fh_sync", "fh_get_stats", "fh_reset_stats", "fh_post_process", "fh_denoise", "fh_gl_register_buffer", "fh_gl_unregister_buffer", "fh_malloc",
    "fh_free", "fh_memset", "fh_copy_to_device", "fh_copy_to_host", "fh_copy_on_device", "fh_image_load_rgba8", "fh_image_free", "fh_stream", "fh_trace_rays", "fh_kernel_info", "fh_kat_hash", "fh_kat_cmj",
    "fh_kat_sobol", "fh_kat_elementary", "fh_kat_warp", "fh_kat_bsdf", "fh_kat_bsdf_lobes", "fh_kat_bsdf_ior", "fh_kat_sky", "fh_kat_hosek_state", "fh_kat_camera",
    "fh_kat_offset_origin", "fh_kat_math", "fh_kat_sqrt", "fh_kat_div", "fh_kat_tex2d", "fh_kat_face_classes", "fh_kat_alpha_records", "fh_kat_ray_start", "fh_kat_set_sample_counts", "fh_kat_sample_counts", "fh_measure_bandwidth",
    "fh_set_adaptive_sampling", "fh_get_adaptive_sampling", "fh_get_sample_counts", "fh_get_luminance_moments", "fh_active_pixel_count", "fh_kat_set_issued", "fh_kat_live_allocations",
    "fh_set_adaptive_policy", "fh_get_adaptive_policy", "fh_adaptive_next_boundary",
    "fh_denoise_guided", "fh_denoise_temporal", "fh_denoise_history_reset", "fh_denoise_history_info",
    "fh_primary_instances", "fh_motion_from_transforms", "fh_denoise_temporal_motion", "fh_set_denoise_motion", "fh_get_denoise_motion", "fh_kat_chief_rays",
    "fh_set_denoise_response", "fh_get_denoise_response", "fh_set_denoise_response_noise", "fh_get_denoise_response_noise",
    "fh_set_denoise_temporal_moments", "fh_get_denoise_temporal_moments",
    "fh_set_auto_exposure", "fh_get_auto_exposure", "fh_auto_exposure_reset", "fh_meter_exposure", "fh_get_auto_exposure_state", "fh_get_luminance_histogram",
    "fh_set_local_exposure", "fh_get_local_exposure", "fh_local_exposure_analyse", "fh_get_local_exposure_base",
    "fh_set_env_sampling", "fh_get_env_sampling", "fh_kat_env_table", "fh_kat_env_sample", "fh_kat_env_pdf", "fh_kat_env_radiance",
    "fh_set_light_sampling", "fh_get_light_sampling", "fh_kat_light_table", "fh_kat_light_pick",
    "fh_set_light_resampling", "fh_get_light_resampling", "fh_kat_light_proxies", "fh_kat_light_resample", "fh_kat_light_usel",
    "fh_set_skin", "fh_set_joint_matrices", "fh_get_skin_info", "fh_get_posed_geometry",
    "fh_ctx_create_group", "fh_ctx_group_size", "fh_ctx_member", "fh_group_set_gather_layers", "fh_group_gather_times", "fh_group_shard_layout",
]


class AdaptiveParamsC(C.Structure):
    """fh_adaptive_params (include/fredholm_hip.h)"""
    _fields_ = [("threshold", C.c_float), ("floor", C.c_float), ("min_samples", C.c_uint32), ("step", C.c_uint32)]


class DenoiseInputsC(C.Structure):
    """fh_denoise_inputs (include/fredholm_hip.h): device pointers"""
    _fields_ = [("beauty", C.c_void_p), ("normal", C.c_void_p), ("albedo", C.c_void_p), ("position", C.c_void_p), ("depth", C.c_void_p), ("moments", C.c_void_p),
                ("counts", C.c_void_p)]


class DenoiseParamsC(C.Structure):
    """fh_denoise_params (include/fredholm_hip.h); the defaults are the library's (params == NULL)"""
    _fields_ = [("sigma_l", C.c_float), ("sigma_z", C.c_float), ("sigma_a", C.c_float), ("normal_power_log2", C.c_uint32), ("passes", C.c_uint32)]


class TemporalParamsC(C.Structure):
    """fh_temporal_params (include/fredholm_hip.h); the defaults are the library's (temporal == NULL)"""
    _fields_ = [("alpha_min", C.c_float), ("max_history", C.c_float), ("normal_cos_min", C.c_float), ("plane_tol", C.c_float)]


class MotionC(C.Structure):
    """fh_motion (include/fredholm_hip.h): where an instance's points and normals were in the frame before"""
    _fields_ = [("point", C.c_float * 12), ("normal", C.c_float * 9), ("moved", C.c_uint32)]


class ResponseParamsC(C.Structure):
    """fh_response_params (include/fredholm_hip.h)"""
    _fields_ = [("gamma", C.c_float)]


class ResponseNoiseParamsC(C.Structure):
    """fh_response_noise_params (include/fredholm_hip.h)"""
    _fields_ = [("kappa", C.c_float)]


class TemporalMomentsParamsC(C.Structure):
    """fh_temporal_moments_params (include/fredholm_hip.h)"""
    _fields_ = [("min_history", C.c_float)]


AE_BLOOM_RELATIVE = 1  # FH_AE_BLOOM_RELATIVE


class AutoExposureParamsC(C.Structure):
    """fh_auto_exposure_params (include/fredholm_hip.h)"""
    _fields_ = [("key", C.c_float), ("compensation_ev", C.c_float), ("min_ev", C.c_float), ("max_ev", C.c_float), ("low", C.c_float), ("high", C.c_float),
                ("speed_up", C.c_float), ("speed_down", C.c_float), ("frame_time", C.c_float), ("log2_lo", C.c_float), ("log2_hi", C.c_float), ("flags", C.c_uint32)]


class LocalExposureParamsC(C.Structure):
    """fh_local_exposure_params (include/fredholm_hip.h)"""
    _fields_ = [("highlights", C.c_float), ("shadows", C.c_float), ("pivot", C.c_float), ("max_stops", C.c_float), ("sigma_range", C.c_float), ("passes", C.c_uint32)]


class EnvSamplingParamsC(C.Structure):
    """fh_env_sampling_params (include/fredholm_hip.h)"""
    _fields_ = [("cosine_fraction", C.c_float)]


ENV_COSINE_FRACTION_DEFAULT = 0.5  # FH_ENV_COSINE_FRACTION_DEFAULT


class LightSamplingParamsC(C.Structure):
    """fh_light_sampling_params (include/fredholm_hip.h)"""
    _fields_ = [("uniform_fraction", C.c_float)]


LIGHT_UNIFORM_FRACTION_DEFAULT = 0.0625  # FH_LIGHT_UNIFORM_FRACTION_DEFAULT


class LightResamplingParamsC(C.Structure):
    """fh_light_resampling_params (include/fredholm_hip.h)"""
    _fields_ = [("candidates", C.c_int)]


LIGHT_CANDIDATES_DEFAULT = 4  # FH_LIGHT_CANDIDATES_DEFAULT
LIGHT_CANDIDATES = (1, 2, 4, 8, 16)


class SkinDescC(C.Structure):
    """fh_skin_desc (include/fredholm_hip.h)"""
    _fields_ = [("n_vertices", C.c_uint32), ("n_joints", C.c_uint32), ("joints", C.c_void_p), ("weights", C.c_void_p)]


class AutoExposureStateC(C.Structure):
    """fh_auto_exposure_state (include/fredholm_hip.h)"""
    _fields_ = [("ev", C.c_float), ("target_ev", C.c_float), ("mean_log2", C.c_float), ("metered", C.c_uint32), ("unmetered", C.c_uint32), ("frames", C.c_uint32)]


# argument types of the entry points declared with them (the adaptive-sampling ABI); every entry point returns int
SIGNATURES = {
    "fh_set_adaptive_sampling": [C.c_void_p, C.POINTER(AdaptiveParamsC)],
    "fh_get_adaptive_sampling": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(AdaptiveParamsC)],
    "fh_get_sample_counts": [C.c_void_p, C.c_void_p],
    "fh_get_luminance_moments": [C.c_void_p, C.c_void_p],
    "fh_active_pixel_count": [C.c_void_p, C.POINTER(C.c_uint32)],
    "fh_set_adaptive_policy": [C.c_void_p, C.c_uint32, C.c_uint32],
    "fh_get_adaptive_policy": [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
    "fh_adaptive_next_boundary": [C.c_void_p, C.POINTER(C.c_uint32)],
    "fh_kat_set_issued": [C.c_void_p, C.c_void_p, C.c_uint32],
    "fh_kat_live_allocations": [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
    "fh_denoise_guided": [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(DenoiseInputsC), C.POINTER(DenoiseParamsC), C.c_void_p, C.c_int],
    "fh_denoise_temporal": [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(DenoiseInputsC), C.POINTER(CameraC), C.POINTER(TemporalParamsC), C.POINTER(DenoiseParamsC), C.c_void_p, C.c_int],
    "fh_denoise_history_reset": [C.c_void_p],
    "fh_denoise_history_info": [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
    "fh_primary_instances": [C.c_void_p, C.POINTER(CameraC), C.c_uint32, C.c_uint32, C.c_void_p],
    "fh_motion_from_transforms": [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(MotionC)],
    "fh_denoise_temporal_motion": [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(DenoiseInputsC), C.POINTER(CameraC), C.POINTER(TemporalParamsC), C.POINTER(DenoiseParamsC), C.c_void_p,
                                   C.c_uint32, C.POINTER(MotionC), C.c_void_p, C.c_int],
    "fh_set_denoise_motion": [C.c_void_p, C.c_int],
    "fh_get_denoise_motion": [C.c_void_p, C.POINTER(C.c_int)],
    "fh_set_denoise_response": [C.c_void_p, C.POINTER(ResponseParamsC)],
    "fh_get_denoise_response": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(ResponseParamsC)],
    "fh_set_denoise_response_noise": [C.c_void_p, C.POINTER(ResponseNoiseParamsC)],
    "fh_get_denoise_response_noise": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(ResponseNoiseParamsC)],
    "fh_set_denoise_temporal_moments": [C.c_void_p, C.POINTER(TemporalMomentsParamsC)],
    "fh_get_denoise_temporal_moments": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(TemporalMomentsParamsC)],
    "fh_set_auto_exposure": [C.c_void_p, C.POINTER(AutoExposureParamsC)],
    "fh_get_auto_exposure": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(AutoExposureParamsC)],
    "fh_auto_exposure_reset": [C.c_void_p],
    "fh_meter_exposure": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32],
    "fh_get_auto_exposure_state": [C.c_void_p, C.POINTER(AutoExposureStateC)],
    "fh_get_luminance_histogram": [C.c_void_p, C.POINTER(C.c_uint32)],
    "fh_set_local_exposure": [C.c_void_p, C.POINTER(LocalExposureParamsC)],
    "fh_get_local_exposure": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(LocalExposureParamsC)],
    "fh_local_exposure_analyse": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32],
    "fh_get_local_exposure_base": [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
    "fh_set_env_sampling": [C.c_void_p, C.POINTER(EnvSamplingParamsC)],
    "fh_get_env_sampling": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(EnvSamplingParamsC)],
    "fh_kat_env_table": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "fh_kat_env_sample": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "fh_kat_env_pdf": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "fh_kat_env_radiance": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
    "fh_set_light_sampling": [C.c_void_p, C.POINTER(LightSamplingParamsC)],
    "fh_get_light_sampling": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(LightSamplingParamsC)],
    "fh_kat_light_table": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)],
    "fh_kat_light_pick": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p],
    "fh_set_light_resampling": [C.c_void_p, C.POINTER(LightResamplingParamsC)],
    "fh_get_light_resampling": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(LightResamplingParamsC)],
    "fh_kat_light_proxies": [C.c_void_p, C.c_void_p],
    "fh_kat_light_resample": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "fh_kat_light_usel": [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p],
    "fh_kat_chief_rays": [C.c_void_p, C.POINTER(CameraC), C.c_uint32, C.c_uint32, C.c_void_p],
    "fh_set_skin": [C.c_void_p, C.POINTER(SkinDescC)],
    "fh_set_joint_matrices": [C.c_void_p, C.c_uint32, C.c_void_p],
    "fh_get_skin_info": [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_int)],
    "fh_get_posed_geometry": [C.c_void_p, C.c_void_p, C.c_void_p],
    "fh_ctx_create_group": [C.POINTER(C.c_int), C.c_uint32, C.POINTER(C.c_void_p)],
    "fh_ctx_group_size": [C.c_void_p, C.POINTER(C.c_uint32)],
    "fh_ctx_member": [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)],
    "fh_group_set_gather_layers": [C.c_void_p, C.c_uint32],
    "fh_group_gather_times": [C.c_void_p, C.POINTER(C.c_double)],
    "fh_group_shard_layout": [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)],
}


def group_shard_layout(width, height, n, mask=LAYER_ALL, tile_w=32, tile_h=32):
    """fh_group_shard_layout: the n + 1 byte offsets of the members' packed shards in the lead's staging area (host only, no GPU)"""
    out = (C.c_uint64 * (int(n) + 1))()
    rc = lib().fh_group_shard_layout(int(width), int(height), int(tile_w), int(tile_h), int(n), int(mask), out)
    check(None, rc, "fh_group_shard_layout")
    return [int(v) for v in out]


def motion_from_transforms(o2w_prev, w2o_prev, o2w_cur, w2o_cur):
    """fh_motion_from_transforms (host only, no GPU): a ctypes array of MotionC, one per instance, from the previous and the current instance matrices (n x 12 floats each)"""
    arrs = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 12) for a in (o2w_prev, w2o_prev, o2w_cur, w2o_cur)]
    n = arrs[0].shape[0]
    if any(a.shape[0] != n for a in arrs):
        raise ValueError("motion_from_transforms: the four arrays hold one matrix per instance each")
    out = (MotionC * max(n, 1))()
    check(None, lib().fh_motion_from_transforms(n, *[ptr(a) for a in arrs], out), "fh_motion_from_transforms")
    return (MotionC * n).from_buffer(out) if n else (MotionC * 0)()


_lib = None


def load_library(path=None):
    """Load libfredholm_hip.so; raises FredholmError when it has not been built (no fallback)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise FredholmError(f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(make -C fredholm_amd/csrc); the HIP path has no CPU fallback")
    try:
        L = C.CDLL(p)
    except OSError as e:  # e.g. libamdhip64 missing
        raise FredholmError(f"cannot load {p}: {e}") from e
    L.fh_last_error.restype = C.c_char_p
    L.fh_last_error.argtypes = [C.c_void_p]
    L.fh_stream.restype = C.c_void_p
    L.fh_stream.argtypes = [C.c_void_p]
    for name in EXPORTS:
        fn = getattr(L, name)
        if name not in ("fh_last_error", "fh_stream"):
            fn.restype = C.c_int
        if name in SIGNATURES:
            fn.argtypes = SIGNATURES[name]
    _lib = L
    return L


def lib():
    return load_library()


def check(ctx, rc, what=""):
    if rc != FH_OK:
        msg = lib().fh_last_error(ctx)
        raise FredholmError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None
