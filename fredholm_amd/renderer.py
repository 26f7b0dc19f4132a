"""Python mirror of the reference's host interface for the render path.

`Renderer`, `Camera`, `RenderLayer` and `PostProcessParams` keep the names, argument meaning and
call order of fredholm::Renderer (fredholm/include/fredholm/renderer.h:29-846), fredholm::Camera
(fredholm/include/fredholm/camera.h:22-135), RenderLayer (fredholm/include/fredholm/shared.h:201-208)
and PostProcessParams (fredholm/kernels/include/kernels/post-process.h:4-10); every method forwards
to the C ABI of libfredholm_hip.so.  Errors surface as FredholmError, the analogue of the
std::runtime_error the reference throws from CUDA_CHECK / OPTIX_CHECK.
"""
import ctypes as C
import os
import math

import numpy as np

from . import native as N


def look_at_transform(origin, forward=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0)):
    """camera-to-world 3x4 rows = inverse(lookAt(origin, origin + 0.01 forward, up)) (camera.h:51-69)."""
    o = np.asarray(origin, dtype=np.float64)
    f = np.asarray(forward, dtype=np.float64)
    f = f / np.linalg.norm(f)
    r = np.cross(f, np.asarray(up, dtype=np.float64))
    r = r / np.linalg.norm(r)
    u = np.cross(r, f)
    m = np.zeros((3, 4), dtype=np.float32)
    m[:, 0] = r
    m[:, 1] = u
    m[:, 2] = -f
    m[:, 3] = o
    return m


class Camera:
    """fredholm::Camera: m_transform (camera-to-world), m_fov (radians), m_F, m_focus (camera.h:22-69)."""

    def __init__(self, origin=(0.0, 0.0, 0.0), fov=0.5 * math.pi, F=8.0, focus=10000.0, forward=(0.0, 0.0, -1.0)):
        self.m_origin = tuple(float(v) for v in origin)
        self.m_forward = tuple(float(v) for v in forward)
        self.m_fov = float(fov)
        self.m_F = float(F)
        self.m_focus = float(focus)
        self.m_transform = look_at_transform(self.m_origin, self.m_forward)

    def set_origin(self, origin):
        self.m_origin = tuple(float(v) for v in origin)
        self.m_transform = look_at_transform(self.m_origin, self.m_forward)

    def params(self):
        """the 15 floats of CameraParams (shared.h:59-64)"""
        return np.concatenate([np.asarray(self.m_transform, dtype=np.float32).reshape(12), np.asarray([self.m_fov, self.m_F, self.m_focus], dtype=np.float32)])

    def as_c(self):
        c = N.CameraC()
        flat = np.asarray(self.m_transform, dtype=np.float32).reshape(12)
        for i in range(12):
            c.transform[i] = float(flat[i])
        c.fov, c.F, c.focus = self.m_fov, self.m_F, self.m_focus
        return c


class PostProcessParams:
    def __init__(self, use_bloom=False, bloom_threshold=2.0, bloom_sigma=5.0, ISO=80.0, chromatic_aberration=1.0):
        self.use_bloom, self.bloom_threshold, self.bloom_sigma, self.ISO, self.chromatic_aberration = use_bloom, bloom_threshold, bloom_sigma, ISO, chromatic_aberration

    def as_c(self):
        return N.PostParamsC(int(bool(self.use_bloom)), self.bloom_threshold, self.bloom_sigma, self.ISO, self.chromatic_aberration)


class DeviceBuffer:
    """Owning device allocation (role of cwl::CUDABuffer, cwl/include/cwl/buffer.h:18-85)."""

    def __init__(self, renderer, nbytes):
        self._r = renderer
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        N.check(renderer._ctx, N.lib().fh_malloc(renderer._ctx, C.c_uint64(self.nbytes), C.byref(p)), "fh_malloc")
        self.ptr = p.value

    def clear(self, value=0):
        N.check(self._r._ctx, N.lib().fh_memset(self._r._ctx, C.c_void_p(self.ptr), int(value), C.c_uint64(self.nbytes)), "fh_memset")

    def upload(self, array):
        a = np.ascontiguousarray(array)
        assert a.nbytes <= self.nbytes
        N.check(self._r._ctx, N.lib().fh_copy_to_device(self._r._ctx, C.c_void_p(self.ptr), N.ptr(a), C.c_uint64(a.nbytes)), "fh_copy_to_device")

    def download(self, dtype=np.float32, shape=None):
        out = np.empty(self.nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        N.check(self._r._ctx, N.lib().fh_copy_to_host(self._r._ctx, N.ptr(out), C.c_void_p(self.ptr), C.c_uint64(self.nbytes)), "fh_copy_to_host")
        return out.reshape(shape) if shape is not None else out

    def free(self):
        if self.ptr and self._r._ctx:
            N.lib().fh_free(self._r._ctx, C.c_void_p(self.ptr))
        self.ptr = None


class RenderLayer:
    """Six AOV buffers owned by the caller (shared.h:201-208; allocated by the apps, controller.cpp:80-107).

    Either allocated here through the C ABI, or wrapping external device pointers (e.g. torch tensors)."""

    NAMES = ("beauty", "position", "depth", "normal", "texcoord", "albedo")

    def __init__(self, renderer, width, height, pointers=None):
        self.width, self.height = int(width), int(height)
        self._bufs = {}
        self.ptrs = {}
        for name in self.NAMES:
            comps = 1 if name == "depth" else 4
            if pointers is not None:
                self.ptrs[name] = int(pointers[name])
            else:
                b = DeviceBuffer(renderer, self.width * self.height * comps * 4)
                b.clear()
                self._bufs[name] = b
                self.ptrs[name] = b.ptr

    def clear(self):
        for b in self._bufs.values():
            b.clear()

    def download(self, name):
        comps = 1 if name == "depth" else 4
        shape = (self.height, self.width) if comps == 1 else (self.height, self.width, 4)
        return self._bufs[name].download(np.float32, shape)

    def as_c(self):
        return N.LayersC(*(C.c_void_p(self.ptrs[n]) for n in self.NAMES))

    def free(self):
        for b in self._bufs.values():
            b.free()
        self._bufs = {}


class Renderer:
    """Drop-in for the method surface of fredholm::Renderer that the apps use on the render path.

    The OptiX pipeline-construction calls of the reference (create_module / create_program_group /
    create_pipeline / create_sbt, renderer.h:124-352) are accepted and ignored: there is no OptiX
    pipeline, the HIP kernels are compiled into the library."""

    def __init__(self, device=0, devices=None):
        """device: one GPU (a plain context).  devices=[0, 1, 2, 3]: a group, one member per entry, that renders every frame split by pixel tile
        across them and is used like a plain renderer; buffers belong to devices[0] (include/fredholm_hip.h: fh_ctx_create_group)."""
        self._ctx = C.c_void_p()
        L = N.load_library()
        if devices is None:
            what = "fh_ctx_create"
            rc = L.fh_ctx_create(int(device), C.byref(self._ctx))
        else:
            what = "fh_ctx_create_group"
            devs = [int(d) for d in devices]
            rc = L.fh_ctx_create_group((C.c_int * max(len(devs), 1))(*devs), len(devs), C.byref(self._ctx))
        if rc != N.FH_OK:
            msg = L.fh_last_error(None)
            self._ctx = None
            raise N.FredholmError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
        self.m_width = self.m_height = 0
        self.seed = 1  # params.seed = 1 (renderer.h:664)
        self._keep = None
        self.m_scene = None

    # -- OptiX plumbing kept for call-compatibility
    def create_module(self, filepath=None):
        return None

    def create_program_group(self):
        return None

    def create_pipeline(self):
        return None

    def create_sbt(self):
        return None

    def close(self):
        if self._ctx:
            N.lib().fh_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        N.check(self._ctx, rc, what)

    # -- groups (fh_ctx_create_group)
    @property
    def group_size(self):
        """members of the group; 1 for a plain renderer"""
        n = C.c_uint32(0)
        self._ck(N.lib().fh_ctx_group_size(self._ctx, C.byref(n)), "fh_ctx_group_size")
        return int(n.value)

    def set_gather_layers(self, mask):
        """layers (native.LAYER_* bits) a group brings back from its other members after every render; the rest receive only the lead's tiles"""
        self._ck(N.lib().fh_group_set_gather_layers(self._ctx, C.c_uint32(int(mask))), "fh_group_set_gather_layers")

    def member_stats(self, i):
        """fh_get_stats of member i alone (stats() of a group aggregates them)"""
        m, s = C.c_void_p(), N.StatsC()
        self._ck(N.lib().fh_ctx_member(self._ctx, C.c_uint32(int(i)), C.byref(m)), "fh_ctx_member")
        N.check(m, N.lib().fh_get_stats(m, C.byref(s)), "fh_get_stats")
        return s.as_dict()

    def gather_times(self):
        """(k_pack_layers, copies, k_unpack_group) ms of the last gather, HIP events, with FLAG_TIME_KERNELS set; synchronising"""
        ms = (C.c_double * 3)()
        self._ck(N.lib().fh_group_gather_times(self._ctx, ms), "fh_group_gather_times")
        return tuple(float(v) for v in ms)

    def set_flags(self, flags):
        self._ck(N.lib().fh_set_flags(self._ctx, C.c_uint32(flags)), "fh_set_flags")

    def set_path_pool(self, target_paths):
        self._ck(N.lib().fh_set_path_pool(self._ctx, C.c_uint32(target_paths)), "fh_set_path_pool")

    def path_pool_bytes(self):
        """(bytes per path slot, pools) with the scene and lights as they are now: the pools take pools x target_paths x bytes of device memory"""
        b, n = C.c_uint64(0), C.c_uint32(0)
        self._ck(N.lib().fh_path_pool_bytes(self._ctx, C.byref(b), C.byref(n)), "fh_path_pool_bytes")
        return int(b.value), int(n.value)

    def alpha_face_counts(self):
        """(faces whose textures can cut, always pass, never pass, still tested) of the uploaded scene"""
        a = (C.c_uint32 * 4)()
        self._ck(N.lib().fh_alpha_face_counts(self._ctx, a), "fh_alpha_face_counts")
        return tuple(int(x) for x in a)

    def alpha_cell_counts(self):
        """(micromap cells of the faces that keep their any-hit test, always pass, never pass)"""
        a = (C.c_uint64 * 3)()
        self._ck(N.lib().fh_alpha_cell_counts(self._ctx, a), "fh_alpha_cell_counts")
        return tuple(int(x) for x in a)

    def path_pool_allocated(self):
        """(device bytes, path slots) the path pools hold right now, all pools together"""
        b, n = C.c_uint64(0), C.c_uint64(0)
        self._ck(N.lib().fh_path_pool_allocated(self._ctx, C.byref(b), C.byref(n)), "fh_path_pool_allocated")
        return int(b.value), int(n.value)

    def set_tail_depth(self, depth):
        self._ck(N.lib().fh_set_tail_depth(self._ctx, C.c_uint32(depth)), "fh_set_tail_depth")

    # -- scene (renderer.h:354-432)
    def load_scene(self, scene, clear=True):
        """scene: a .obj / .gltf path (renderer.h:354: load_scene(filepath, clear); clear=False appends, as rtcamp8.cpp:114-115 adds
        a camera .gltf to an .obj), a fredholm_amd.scene.Scene, or a dict of flat arrays as produced by fredholm_amd.scenes (the
        layout Scene exposes, scene.h:103-135)."""
        from .scene import Scene
        if isinstance(scene, (str, bytes)) or hasattr(scene, "__fspath__"):
            if self.m_scene is None:
                self.m_scene = Scene()
            self.m_scene.load_model(os.fspath(scene) if not isinstance(scene, bytes) else scene.decode(), clear)
            scene = self.m_scene.as_dict()
        elif isinstance(scene, Scene):
            self.m_scene = scene
            scene = scene.as_dict()
        else:
            self.m_scene = None  # flat arrays: no node hierarchy, no camera node
        v = np.ascontiguousarray(scene["vertices"], dtype=np.float32).reshape(-1, 3)
        n = np.ascontiguousarray(scene["normals"], dtype=np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(scene["texcoords"], dtype=np.float32).reshape(-1, 2)
        idx = np.ascontiguousarray(scene["indices"], dtype=np.uint32).reshape(-1, 3)
        mid = np.ascontiguousarray(scene["material_ids"], dtype=np.uint32)
        mats = np.ascontiguousarray(scene["materials"])
        assert mats.dtype.itemsize == 180
        inst = scene.get("instance_ids")
        inst = None if inst is None else np.ascontiguousarray(inst, dtype=np.uint32)
        o2w = scene.get("object_to_world")
        w2o = scene.get("world_to_object")
        d = N.SceneDesc()
        d.n_vertices = v.shape[0]
        d.vertices, d.normals, d.texcoords = N.ptr(v), N.ptr(n), N.ptr(t)
        d.n_faces = idx.shape[0]
        d.indices, d.material_ids, d.instance_ids = N.ptr(idx), N.ptr(mid), N.ptr(inst)
        d.n_materials = mats.shape[0]
        d.materials = N.ptr(mats)
        if o2w is not None:
            o2w = np.ascontiguousarray(o2w, dtype=np.float32).reshape(-1, 12)
            w2o = np.ascontiguousarray(w2o, dtype=np.float32).reshape(-1, 12)
            d.n_instances = o2w.shape[0]
            d.object_to_world, d.world_to_object = N.ptr(o2w), N.ptr(w2o)
        textures = scene.get("textures") or []
        tex_arr = (N.TextureDesc * max(len(textures), 1))()
        tex_keep = []
        for k, tex in enumerate(textures):
            img = np.ascontiguousarray(tex["rgba8"], dtype=np.uint8)
            assert img.ndim == 3 and img.shape[2] == 4
            tex_keep.append(img)
            tex_arr[k] = N.TextureDesc(img.shape[1], img.shape[0], img.ctypes.data, int(bool(tex.get("srgb", False))))
        d.n_textures = len(textures)
        d.textures = C.cast(tex_arr, C.c_void_p) if textures else None
        self._keep = (v, n, t, idx, mid, mats, inst, o2w, w2o, tex_arr, tex_keep)
        self._ck(N.lib().fh_scene_upload(self._ctx, C.byref(d)), "fh_scene_upload")
        if scene.get("joints") is not None:  # a skinned scene: the skin, and the pose where the scene brings one
            jm = scene.get("joint_matrices")
            n_joints = scene.get("n_joints")
            if n_joints is None:
                n_joints = np.asarray(jm).reshape(-1, 12).shape[0] if jm is not None else int(np.asarray(scene["joints"]).max()) + 1
            self.set_skin(scene["joints"], scene["weights"], n_joints)
            if jm is not None:
                self.set_joint_matrices(jm)

    def build_gas(self):
        """renderer.h:434-496; the whole acceleration structure is built by build_ias' counterpart"""
        return None

    def build_ias(self):
        """renderer.h:498-552 -> on-device BVH build"""
        self._ck(N.lib().fh_bvh_build(self._ctx), "fh_bvh_build")

    def build_accel(self):
        self.build_ias()

    def set_transforms(self, object_to_world, world_to_object):
        o = np.ascontiguousarray(object_to_world, dtype=np.float32).reshape(-1, 12)
        w = np.ascontiguousarray(world_to_object, dtype=np.float32).reshape(-1, 12)
        self._ck(N.lib().fh_set_transforms(self._ctx, C.c_uint32(o.shape[0]), N.ptr(o), N.ptr(w)), "fh_set_transforms")

    # -- skeletal skinning (an extension beyond the reference class; include/fredholm_hip.h: fh_skin_desc)
    def set_skin(self, joints, weights, n_joints):
        """four joint indices (into one palette of n_joints matrices) and four weights per vertex of the loaded scene; geometry stays in the bind pose until
        set_joint_matrices.  Vertices whose four weights are 0 are unskinned."""
        j = np.asarray(joints)
        if j.size and (j.min() < 0 or j.max() > 65535):
            raise N.FredholmError("set_skin: a joint index does not fit 16 bits")
        j = np.ascontiguousarray(j, dtype=np.uint16).reshape(-1, 4)
        w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1, 4)
        if j.shape[0] != w.shape[0]:
            raise N.FredholmError("set_skin: joints and weights hold four entries per vertex each")
        d = N.SkinDescC(j.shape[0], int(n_joints), N.ptr(j), N.ptr(w))
        self._ck(N.lib().fh_set_skin(self._ctx, C.byref(d)), "fh_set_skin")

    def clear_skin(self):
        """geometry returns to the bind pose, bit for bit"""
        self._ck(N.lib().fh_set_skin(self._ctx, None), "fh_set_skin")

    def set_joint_matrices(self, m):
        """the pose: one row-major 3 x 4 matrix per joint of the skin, in the object space of the skinned vertices; call build_ias afterwards"""
        m = np.ascontiguousarray(m, dtype=np.float32).reshape(-1, 12)
        self._ck(N.lib().fh_set_joint_matrices(self._ctx, C.c_uint32(m.shape[0]), N.ptr(m)), "fh_set_joint_matrices")

    def skin_info(self):
        """(n_joints, vertices with a non-zero weight, posed); n_joints 0: no skin"""
        nj, nv, posed = C.c_uint32(0), C.c_uint32(0), C.c_int(0)
        self._ck(N.lib().fh_get_skin_info(self._ctx, C.byref(nj), C.byref(nv), C.byref(posed)), "fh_get_skin_info")
        return int(nj.value), int(nv.value), bool(posed.value)

    def posed_geometry(self):
        """(vertices, normals) of the loaded scene as the face records are derived from them: [n_vertices, 3] float32 each, the bind arrays when nothing is posed"""
        nv = self._keep[0].shape[0]
        v, n = np.empty((nv, 3), np.float32), np.empty((nv, 3), np.float32)
        self._ck(N.lib().fh_get_posed_geometry(self._ctx, N.ptr(v), N.ptr(n)), "fh_get_posed_geometry")
        return v, n

    def n_lights(self):
        out = C.c_uint32()
        self._ck(N.lib().fh_scene_n_lights(self._ctx, C.byref(out)), "fh_scene_n_lights")
        return out.value

    # -- environment (renderer.h:554-612)
    def set_directional_light(self, le, direction, angle):
        le = np.asarray(le, dtype=np.float32)
        d = np.asarray(direction, dtype=np.float32)
        self._ck(N.lib().fh_set_directional_light(self._ctx, N.ptr(le), N.ptr(d), C.c_float(angle)), "fh_set_directional_light")

    def clear_directional_light(self):
        self._ck(N.lib().fh_clear_directional_light(self._ctx), "fh_clear_directional_light")

    def set_sky_intensity(self, v):
        self._ck(N.lib().fh_set_sky_intensity(self._ctx, C.c_float(v)), "fh_set_sky_intensity")

    def load_arhosek_sky(self, turbidity, albedo):
        self._ck(N.lib().fh_load_arhosek_sky(self._ctx, C.c_float(turbidity), C.c_float(albedo)), "fh_load_arhosek_sky")

    def clear_arhosek_sky(self):
        self._ck(N.lib().fh_clear_arhosek_sky(self._ctx), "fh_clear_arhosek_sky")

    def load_ibl(self, filepath_or_image):
        """renderer.h:574-581: a Radiance .hdr path (read like the reference's FloatTexture, scene.cpp:39-66) or the decoded
        lat-long image (H x W x 4 float32)"""
        if isinstance(filepath_or_image, (str, bytes)) or hasattr(filepath_or_image, "__fspath__"):
            from . import image_io
            filepath_or_image = image_io.load_hdr(filepath_or_image)
        img = np.ascontiguousarray(filepath_or_image, dtype=np.float32)
        assert img.ndim == 3 and img.shape[2] == 4
        self._ck(N.lib().fh_load_ibl(self._ctx, N.ptr(img), C.c_uint32(img.shape[1]), C.c_uint32(img.shape[0])), "fh_load_ibl")

    def clear_ibl(self):
        self._ck(N.lib().fh_clear_ibl(self._ctx), "fh_clear_ibl")

    # -- frame state (renderer.h:642-655)
    def set_resolution(self, width, height):
        self.m_width, self.m_height = int(width), int(height)
        self._ck(N.lib().fh_set_resolution(self._ctx, C.c_uint32(width), C.c_uint32(height)), "fh_set_resolution")

    def init_render_states(self):
        self._ck(N.lib().fh_init_render_states(self._ctx), "fh_init_render_states")

    def set_tile_shard(self, rank, world, tile_w=32, tile_h=32):
        self._ck(N.lib().fh_set_tile_shard(self._ctx, C.c_uint32(rank), C.c_uint32(world), C.c_uint32(tile_w), C.c_uint32(tile_h)), "fh_set_tile_shard")

    def owned_pixel_count(self):
        out = C.c_uint32()
        self._ck(N.lib().fh_owned_pixel_count(self._ctx, C.byref(out)), "fh_owned_pixel_count")
        return out.value

    def pack_owned(self, layer_ptr, floats_per_pixel, packed_ptr):
        self._ck(N.lib().fh_pack_owned(self._ctx, C.c_void_p(layer_ptr), C.c_uint32(floats_per_pixel), C.c_void_p(packed_ptr)), "fh_pack_owned")

    def unpack_shard(self, rank, world, packed_ptr, floats_per_pixel, layer_ptr):
        self._ck(N.lib().fh_unpack_shard(self._ctx, C.c_uint32(rank), C.c_uint32(world), C.c_void_p(packed_ptr), C.c_uint32(floats_per_pixel), C.c_void_p(layer_ptr)), "fh_unpack_shard")

    def unpack_shards(self, packed_ptrs, floats_per_pixel, layer_ptr):
        """fh_unpack_shards: every rank's packed shard (device pointers, rank order) into the frame in ONE launch"""
        arr = (C.c_void_p * len(packed_ptrs))(*[C.c_void_p(int(p)) for p in packed_ptrs])
        self._ck(N.lib().fh_unpack_shards(self._ctx, C.c_uint32(len(packed_ptrs)), arr, C.c_uint32(floats_per_pixel), C.c_void_p(layer_ptr)), "fh_unpack_shards")

    # -- the hot path (renderer.h:657-736)
    def set_time(self, time):
        """renderer.h:614-640: advance the animation, re-upload the instance transforms, rebuild the acceleration structure"""
        if self.m_scene is None:
            raise N.FredholmError("set_time: the scene was not loaded from a file or a Scene")
        self.m_scene.update_animation(time)
        o2w, w2o = self.m_scene.transforms_3x4()
        self.set_transforms(o2w, w2o)
        if getattr(self.m_scene, "m_skins", None):
            self.set_joint_matrices(self.m_scene.joint_matrices_3x4())
        self.build_ias()

    def render(self, camera, bg_color, render_layer, n_samples, max_depth):
        cam = camera.as_c()
        if self.m_scene is not None and self.m_scene.m_has_camera_transform:  # renderer.h:670-676: a camera node overrides the pose
            flat = self.m_scene.camera_transform_3x4().reshape(12)
            for i in range(12):
                cam.transform[i] = float(flat[i])
        bg = np.asarray(bg_color, dtype=np.float32)
        layers = render_layer.as_c()
        self._ck(N.lib().fh_render(self._ctx, C.byref(cam), N.ptr(bg), C.byref(layers), C.c_uint32(n_samples), C.c_uint32(max_depth), C.c_uint32(self.seed)), "fh_render")

    def wait_for_completion(self):
        self._ck(N.lib().fh_sync(self._ctx), "fh_sync")

    # -- adaptive sampling (an extension beyond the reference class; include/fredholm_hip.h: fh_set_adaptive_sampling)
    def set_adaptive_sampling(self, threshold, min_samples=64, step=16, floor=0.01):
        """stop a pixel at the first count n (n >= min_samples, n % step == 0) where its relative error estimate is within `threshold`; accepted only before the
        first sample after init_render_states / set_resolution.  render(n) then adds at most n samples per pixel."""
        p = N.AdaptiveParamsC(float(threshold), float(floor), int(min_samples), int(step))
        self._ck(N.lib().fh_set_adaptive_sampling(self._ctx, C.byref(p)), "fh_set_adaptive_sampling")

    def clear_adaptive_sampling(self):
        self._ck(N.lib().fh_set_adaptive_sampling(self._ctx, None), "fh_set_adaptive_sampling")

    def set_adaptive_policy(self, block=1, growth=1):
        """how the mode decides: block x block pixel blocks (1, 2, 4, 8) stop together, when all of their pixels are converged; growth 2 tests at b0 * 2^k only
        (b0: the first multiple of step >= min_samples).  Accepted while the mode is off, and like the mode only before the first sample of a frame."""
        self._ck(N.lib().fh_set_adaptive_policy(self._ctx, C.c_uint32(int(block)), C.c_uint32(int(growth))), "fh_set_adaptive_policy")

    def adaptive_policy(self):
        """(block, growth)"""
        b, g = C.c_uint32(0), C.c_uint32(0)
        self._ck(N.lib().fh_get_adaptive_policy(self._ctx, C.byref(b), C.byref(g)), "fh_get_adaptive_policy")
        return b.value, g.value

    def adaptive_next_boundary(self):
        """samples from those requested since init_render_states to the next boundary: a render() of that many ends a round (the mode must be on)"""
        out = C.c_uint32(0)
        self._ck(N.lib().fh_adaptive_next_boundary(self._ctx, C.byref(out)), "fh_adaptive_next_boundary")
        return out.value

    def adaptive_sampling(self):
        """None while off, else the parameters as a dict"""
        on, p = C.c_int(0), N.AdaptiveParamsC()
        self._ck(N.lib().fh_get_adaptive_sampling(self._ctx, C.byref(on), C.byref(p)), "fh_get_adaptive_sampling")
        return {"threshold": p.threshold, "floor": p.floor, "min_samples": p.min_samples, "step": p.step} if on.value else None

    def get_sample_counts(self, device_ptr):
        """width * height uint32 sample counts into a device buffer (ordered on the context stream)"""
        self._ck(N.lib().fh_get_sample_counts(self._ctx, C.c_void_p(int(device_ptr))), "fh_get_sample_counts")

    def get_luminance_moments(self, device_ptr):
        """width * height float2 (m1, m2) into a device buffer (adaptive sampling must be on)"""
        self._ck(N.lib().fh_get_luminance_moments(self._ctx, C.c_void_p(int(device_ptr))), "fh_get_luminance_moments")

    def active_pixel_count(self):
        """owned pixels the next render() would sample (synchronising)"""
        out = C.c_uint32(0)
        self._ck(N.lib().fh_active_pixel_count(self._ctx, C.byref(out)), "fh_active_pixel_count")
        return int(out.value)

    def sample_counts(self):
        """(height, width) uint32"""
        b = DeviceBuffer(self, 4 * self.m_width * self.m_height)
        try:
            self.get_sample_counts(b.ptr)
            return b.download(np.uint32, (self.m_height, self.m_width))
        finally:
            b.free()

    def luminance_moments(self):
        """(height, width, 2) float32: the running means of the luminance and of its square"""
        b = DeviceBuffer(self, 8 * self.m_width * self.m_height)
        try:
            self.get_luminance_moments(b.ptr)
            return b.download(np.float32, (self.m_height, self.m_width, 2))
        finally:
            b.free()

    def relative_error(self):
        """(height, width) float32 display map of the estimate the stop rule tests: sqrt(e2) / max(m1, floor), e2 = max(m2 - m1^2, 0) * n / (n - 1) / n (NaN below two samples)"""
        p = self.adaptive_sampling()
        if p is None:
            raise N.FredholmError("relative_error: adaptive sampling is off")
        m = self.luminance_moments().astype(np.float64)
        n = self.sample_counts().astype(np.float64)
        var = np.maximum(m[..., 1] - m[..., 0] ** 2, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            e2 = np.where(n >= 2, var * n / (n - 1) / n, np.nan)
            return (np.sqrt(e2) / np.maximum(m[..., 0], p["floor"])).astype(np.float32)

    def stats(self):
        s = N.StatsC()
        self._ck(N.lib().fh_get_stats(self._ctx, C.byref(s)), "fh_get_stats")
        return s.as_dict()

    def kernel_info(self, which):
        """fh_kernel_info: what the runtime reports for the streaming traversal kernel of the current scene (0: closest hit, 1: secondary rays)"""
        out = (C.c_uint32 * 6)()
        self._ck(N.lib().fh_kernel_info(self._ctx, int(which), out), "fh_kernel_info")
        return {"vgprs": int(out[0]), "static_lds_bytes": int(out[1]), "scratch_bytes": int(out[2]), "workgroups_per_cu": int(out[3]), "stack_levels_in_lds": int(out[4]),
                "stack_levels": int(out[5])}

    def shade_kernel_info(self):
        """fh_kernel_info(2 + c) for every shading class c of the scene: registers, LDS, scratch, waves per SIMD of the shade kernel each class runs"""
        out = []
        for c in range(8):
            o = (C.c_uint32 * 6)()
            if N.lib().fh_kernel_info(self._ctx, 2 + c, o) != 0:
                break
            out.append({"class": c, "lobes": int(o[5]), "compiled_for_lobes": int(o[4]), "vgprs": int(o[0]), "static_lds_bytes": int(o[1]), "scratch_bytes": int(o[2]), "waves_per_simd": int(o[3])})
        return out

    def reset_stats(self):
        self._ck(N.lib().fh_reset_stats(self._ctx), "fh_reset_stats")

    def stream(self):
        return N.lib().fh_stream(self._ctx)

    # -- post chain (kernels/post-process.h:126-128)
    def post_process(self, beauty_in_ptr, high_ptr, temp_ptr, width, height, params, beauty_out_ptr):
        pp = params.as_c()
        self._ck(N.lib().fh_post_process(self._ctx, C.c_void_p(beauty_in_ptr), C.c_void_p(high_ptr), C.c_void_p(temp_ptr), int(width), int(height), C.byref(pp), C.c_void_p(beauty_out_ptr)),
                 "fh_post_process")

    # -- importance sampling of the environment (fh_set_env_sampling)
    def set_env_sampling(self, cosine_fraction=N.ENV_COSINE_FRACTION_DEFAULT):
        """fh_set_env_sampling: while on, the sky next-event ray of every shaded hit is drawn from a mixture of the cosine lobe (share `cosine_fraction`, in [0, 1)) and a
        512 x 256 table of the environment's luminance (image, Hosek dome or constant), and the BSDF-sampled light ray is weighed against that density.  The table is
        rebuilt by the next render after the environment changes.  Nothing else of a frame changes; off (the default) keeps every bit"""
        p = N.EnvSamplingParamsC(float(cosine_fraction))
        self._ck(N.lib().fh_set_env_sampling(self._ctx, C.byref(p)), "fh_set_env_sampling")

    def clear_env_sampling(self):
        """off: the cosine-distributed sky ray of the reference"""
        self._ck(N.lib().fh_set_env_sampling(self._ctx, None), "fh_set_env_sampling")

    def get_env_sampling(self):
        """(on, cosine_fraction): the switch and the fraction last set (the default before any)"""
        on, p = C.c_int(0), N.EnvSamplingParamsC()
        self._ck(N.lib().fh_get_env_sampling(self._ctx, C.byref(on), C.byref(p)), "fh_get_env_sampling")
        return bool(on.value), float(p.cosine_fraction)

    # -- sampling of area lights by power (fh_set_light_sampling)
    def set_light_sampling(self, uniform_fraction=N.LIGHT_UNIFORM_FRACTION_DEFAULT):
        """fh_set_light_sampling: while on, the emitter of every area shadow ray is picked from a table of the emitters' power (area x luminance of the emission) mixed
        with the uniform pick (share `uniform_fraction`, in (0, 1]), and the BSDF-sampled light ray that finds an emitter is weighed against that pick.  The table is
        rebuilt by the next render after the scene or its transforms change.  Nothing else of a frame changes; off (the default) keeps every bit"""
        p = N.LightSamplingParamsC(float(uniform_fraction))
        self._ck(N.lib().fh_set_light_sampling(self._ctx, C.byref(p)), "fh_set_light_sampling")

    def clear_light_sampling(self):
        """off: the uniform pick of the reference"""
        self._ck(N.lib().fh_set_light_sampling(self._ctx, None), "fh_set_light_sampling")

    def get_light_sampling(self):
        """(on, uniform_fraction): the switch and the fraction last set (the default before any)"""
        on, p = C.c_int(0), N.LightSamplingParamsC()
        self._ck(N.lib().fh_get_light_sampling(self._ctx, C.byref(on), C.byref(p)), "fh_get_light_sampling")
        return bool(on.value), float(p.uniform_fraction)

    # -- resampling of the table's picks by distance and facing (fh_set_light_resampling)
    def set_light_resampling(self, candidates=N.LIGHT_CANDIDATES_DEFAULT):
        """fh_set_light_resampling: acts while light sampling is on.  The area shadow ray draws `candidates` (1, 2, 4, 8 or 16) emitters from the table and chooses
        one in proportion to a geometric weight of the emitter seen from the shaded point: facing at both ends over the squared distance.  No further random
        dimension is used and the MIS weights stay the table's; off (the default), or candidates = 1, keeps every bit"""
        p = N.LightResamplingParamsC(int(candidates))
        self._ck(N.lib().fh_set_light_resampling(self._ctx, C.byref(p)), "fh_set_light_resampling")

    def clear_light_resampling(self):
        """off: the table's pick as it is"""
        self._ck(N.lib().fh_set_light_resampling(self._ctx, None), "fh_set_light_resampling")

    def get_light_resampling(self):
        """(on, candidates): the switch and the count last set (the default before any)"""
        on, p = C.c_int(0), N.LightResamplingParamsC()
        self._ck(N.lib().fh_get_light_resampling(self._ctx, C.byref(on), C.byref(p)), "fh_get_light_resampling")
        return bool(on.value), int(p.candidates)

    # -- auto-exposure of the post chain (fh_set_auto_exposure)
    def set_auto_exposure(self, key=0.18, compensation_ev=0.0, min_ev=-16.0, max_ev=16.0, low=0.10, high=0.90, speed_up=3.0, speed_down=1.0, frame_time=1.0 / 30.0,
                          log2_lo=-16.0, log2_hi=16.0, bloom_relative=False):
        """fh_set_auto_exposure: while on, post_process meters its input into a 256-bin log2-luminance histogram, maps the mean of the ranks between `low` and `high`
        to `key`, moves ev = log2(exposure) towards that target at speed_up / speed_down per second (frame_time seconds per call; inf: no adaptation) and tone-maps
        with 2^ev in place of the ISO exposure.  bloom_relative: the bloom threshold compares exposed luminance.  Turning it on starts from frames = 0"""
        p = N.AutoExposureParamsC(float(key), float(compensation_ev), float(min_ev), float(max_ev), float(low), float(high), float(speed_up), float(speed_down), float(frame_time),
                                  float(log2_lo), float(log2_hi), N.AE_BLOOM_RELATIVE if bloom_relative else 0)
        self._ck(N.lib().fh_set_auto_exposure(self._ctx, C.byref(p)), "fh_set_auto_exposure")

    def clear_auto_exposure(self):
        """off; the state is dropped"""
        self._ck(N.lib().fh_set_auto_exposure(self._ctx, None), "fh_set_auto_exposure")

    def get_auto_exposure(self):
        """(on, parameters as a dict): the switch and the parameters last set (the defaults before any)"""
        on, p = C.c_int(0), N.AutoExposureParamsC()
        self._ck(N.lib().fh_get_auto_exposure(self._ctx, C.byref(on), C.byref(p)), "fh_get_auto_exposure")
        return bool(on.value), {k: getattr(p, k) for k, _ in p._fields_}

    def auto_exposure_state(self):
        """the state after everything queued so far (synchronising): ev, target_ev, mean_log2, metered, unmetered, frames"""
        s = N.AutoExposureStateC()
        self._ck(N.lib().fh_get_auto_exposure_state(self._ctx, C.byref(s)), "fh_get_auto_exposure_state")
        return {k: getattr(s, k) for k, _ in s._fields_}

    def auto_exposure_reset(self):
        """frames = 0: the next metered frame sets ev = target"""
        self._ck(N.lib().fh_auto_exposure_reset(self._ctx), "fh_auto_exposure_reset")

    def meter_exposure(self, image_ptr, width, height):
        """fh_meter_exposure: meter a device image of width * height float4 and update the state (asynchronous); what post_process does first while the switch is on"""
        self._ck(N.lib().fh_meter_exposure(self._ctx, C.c_void_p(image_ptr), C.c_uint32(int(width)), C.c_uint32(int(height))), "fh_meter_exposure")

    def luminance_histogram(self):
        """the 257 counts of the last metering call (synchronising); [256] = unmetered pixels"""
        h = (C.c_uint32 * 257)()
        self._ck(N.lib().fh_get_luminance_histogram(self._ctx, h), "fh_get_luminance_histogram")
        return np.frombuffer(h, dtype=np.uint32).copy()

    # -- local exposure of the post chain (fh_set_local_exposure)
    def set_local_exposure(self, highlights=0.5, shadows=0.5, pivot=0.18, max_stops=4.0, sigma_range=1.0, passes=4):
        """fh_set_local_exposure: while on, post_process builds an edge-aware base layer of its input's log2-luminance (4 x 4 means, `passes` a-trous passes with a
        range sigma of `sigma_range` stops, upsampled against each pixel's own value) and its tone map multiplies each pixel by a gain that removes the share
        `highlights` (above) or `shadows` (below) of the base's distance from `pivot`, by at most `max_stops` stops.  The detail on top of the base is left alone"""
        p = N.LocalExposureParamsC(float(highlights), float(shadows), float(pivot), float(max_stops), float(sigma_range), int(passes))
        self._ck(N.lib().fh_set_local_exposure(self._ctx, C.byref(p)), "fh_set_local_exposure")

    def clear_local_exposure(self):
        """off: one exposure for the frame"""
        self._ck(N.lib().fh_set_local_exposure(self._ctx, None), "fh_set_local_exposure")

    def get_local_exposure(self):
        """(on, parameters as a dict): the switch and the parameters last set (the defaults before any)"""
        on, p = C.c_int(0), N.LocalExposureParamsC()
        self._ck(N.lib().fh_get_local_exposure(self._ctx, C.byref(on), C.byref(p)), "fh_get_local_exposure")
        return bool(on.value), {k: getattr(p, k) for k, _ in p._fields_}

    def local_exposure_analyse(self, image_ptr, width, height):
        """fh_local_exposure_analyse: the base stage alone on a device image of width * height float4 (asynchronous); what post_process does first while the switch is on"""
        self._ck(N.lib().fh_local_exposure_analyse(self._ctx, C.c_void_p(image_ptr), C.c_uint32(int(width)), C.c_uint32(int(height))), "fh_local_exposure_analyse")

    def local_exposure_base(self):
        """the quarter-resolution base of the last analysis (synchronising): a float32 array of ceil(h / 4) x ceil(w / 4), empty before any"""
        w4, h4 = C.c_uint32(0), C.c_uint32(0)
        self._ck(N.lib().fh_get_local_exposure_base(self._ctx, None, C.byref(w4), C.byref(h4)), "fh_get_local_exposure_base")
        base = np.zeros((h4.value, w4.value), dtype=np.float32)
        if base.size:
            self._ck(N.lib().fh_get_local_exposure_base(self._ctx, base.ctypes.data_as(C.c_void_p), C.byref(w4), C.byref(h4)), "fh_get_local_exposure_base")
        return base

    def denoise(self, width, height, beauty_ptr, normal_ptr, albedo_ptr, denoised_ptr, upscale=False):
        """the denoiser slot (Denoiser::denoise, denoiser.h:87-95): edge-avoiding a-trous filter guided by the normal and albedo layers"""
        self._ck(N.lib().fh_denoise(self._ctx, C.c_uint32(int(width)), C.c_uint32(int(height)), C.c_void_p(beauty_ptr), C.c_void_p(normal_ptr), C.c_void_p(albedo_ptr),
                                    C.c_void_p(denoised_ptr), int(bool(upscale))), "fh_denoise")

    def denoise_guided(self, width, height, beauty_ptr, normal_ptr, albedo_ptr, denoised_ptr, position_ptr=None, depth_ptr=None, moments_ptr=None, counts_ptr=None,
                       sigma_l=2.0, sigma_z=1.0, sigma_a=0.2, normal_power_log2=7, passes=5, upscale=False):
        """the variance-guided denoiser (fh_denoise_guided): an a-trous filter whose colour edge stop is each pixel's own standard deviation, from the luminance
        moments and sample counts of adaptive sampling (moments_ptr, counts_ptr: device copies made with get_luminance_moments / get_sample_counts) or, without
        them, from a 7x7 spatial estimate.  position_ptr and depth_ptr add the plane edge stop.  All pointers are device pointers; pairs go together."""
        i = N.DenoiseInputsC(beauty_ptr, normal_ptr, albedo_ptr, position_ptr, depth_ptr, moments_ptr, counts_ptr)
        p = N.DenoiseParamsC(float(sigma_l), float(sigma_z), float(sigma_a), int(normal_power_log2), int(passes))
        self._ck(N.lib().fh_denoise_guided(self._ctx, int(width), int(height), C.byref(i), C.byref(p), C.c_void_p(denoised_ptr), int(bool(upscale))), "fh_denoise_guided")

    def denoise_temporal(self, width, height, beauty_ptr, normal_ptr, albedo_ptr, denoised_ptr, position_ptr, depth_ptr, camera, moments_ptr=None, counts_ptr=None,
                         alpha_min=0.2, max_history=32.0, normal_cos_min=0.5, plane_tol=0.02, sigma_l=2.0, sigma_z=1.0, sigma_a=0.2, normal_power_log2=7, passes=5, upscale=False):
        """temporal accumulation in front of the variance-guided denoiser (fh_denoise_temporal): the frame's demodulated radiance and variance are blended with the
        context's history of the frames before it, reprojected through the world position, and the guided filter's passes run on the result.  `camera` is the Camera
        the layers were rendered with; give every frame of a sequence samples of its own (Renderer.seed).  The first call after reset_denoise_history or a change of
        width x height is denoise_guided."""
        i = N.DenoiseInputsC(beauty_ptr, normal_ptr, albedo_ptr, position_ptr, depth_ptr, moments_ptr, counts_ptr)
        t = N.TemporalParamsC(float(alpha_min), float(max_history), float(normal_cos_min), float(plane_tol))
        p = N.DenoiseParamsC(float(sigma_l), float(sigma_z), float(sigma_a), int(normal_power_log2), int(passes))
        cam = camera.as_c()
        self._ck(N.lib().fh_denoise_temporal(self._ctx, int(width), int(height), C.byref(i), C.byref(cam), C.byref(t), C.byref(p), C.c_void_p(denoised_ptr), int(bool(upscale))),
                 "fh_denoise_temporal")

    def primary_instances(self, camera, width, height, ids_ptr):
        """fh_primary_instances: the instance id of the face each pixel's chief ray sees (0xffffffff: a miss), width * height uint32 at the device pointer ids_ptr"""
        cam = camera.as_c()
        self._ck(N.lib().fh_primary_instances(self._ctx, C.byref(cam), int(width), int(height), C.c_void_p(ids_ptr)), "fh_primary_instances")

    def denoise_temporal_motion(self, width, height, beauty_ptr, normal_ptr, albedo_ptr, denoised_ptr, position_ptr, depth_ptr, camera, instance_ids_ptr, motion,
                                moments_ptr=None, counts_ptr=None, alpha_min=0.2, max_history=32.0, normal_cos_min=0.5, plane_tol=0.02, sigma_l=2.0, sigma_z=1.0, sigma_a=0.2,
                                normal_power_log2=7, passes=5, upscale=False):
        """denoise_temporal with per-instance motion vectors (fh_denoise_temporal_motion): instance_ids_ptr is the device plane primary_instances fills, `motion` the
        table native.motion_from_transforms makes from the instance matrices of the frame before and of this frame (a ctypes array of native.MotionC).  Pixels of
        instances that moved look their history up where the surface was; everything else is denoise_temporal."""
        i = N.DenoiseInputsC(beauty_ptr, normal_ptr, albedo_ptr, position_ptr, depth_ptr, moments_ptr, counts_ptr)
        t = N.TemporalParamsC(float(alpha_min), float(max_history), float(normal_cos_min), float(plane_tol))
        p = N.DenoiseParamsC(float(sigma_l), float(sigma_z), float(sigma_a), int(normal_power_log2), int(passes))
        cam = camera.as_c()
        n = 0 if motion is None else len(motion)
        self._ck(N.lib().fh_denoise_temporal_motion(self._ctx, int(width), int(height), C.byref(i), C.byref(cam), C.byref(t), C.byref(p),
                                                    None if instance_ids_ptr is None else C.c_void_p(instance_ids_ptr), n, motion if n else None, C.c_void_p(denoised_ptr),
                                                    int(bool(upscale))), "fh_denoise_temporal_motion")

    def set_denoise_motion(self, on=True):
        """fh_set_denoise_motion: while on, denoise_temporal keeps the instance matrices with its history and carries the pixels of instances that set_transforms /
        set_time moved since (the layers must have been rendered with the current transforms)"""
        self._ck(N.lib().fh_set_denoise_motion(self._ctx, int(bool(on))), "fh_set_denoise_motion")

    def denoise_motion(self):
        on = C.c_int(0)
        self._ck(N.lib().fh_get_denoise_motion(self._ctx, C.byref(on)), "fh_get_denoise_motion")
        return bool(on.value)

    def set_denoise_response(self, gamma=1.0):
        """fh_set_denoise_response: while on, denoise_temporal and denoise_temporal_motion clamp the history they found to mean +- gamma standard deviations of the
        current frame's colour in a 5 x 5 window before blending, and shorten it by how far outside it lay: a change of lighting no longer lags by 1 / alpha_min frames"""
        p = N.ResponseParamsC(float(gamma))
        self._ck(N.lib().fh_set_denoise_response(self._ctx, C.byref(p)), "fh_set_denoise_response")

    def clear_denoise_response(self):
        self._ck(N.lib().fh_set_denoise_response(self._ctx, None), "fh_set_denoise_response")

    def get_denoise_response(self):
        """(on, gamma): the switch and the gamma last set (1 before any)"""
        on, p = C.c_int(0), N.ResponseParamsC(0.0)
        self._ck(N.lib().fh_get_denoise_response(self._ctx, C.byref(on), C.byref(p)), "fh_get_denoise_response")
        return bool(on.value), float(p.gamma)

    def set_denoise_response_noise(self, kappa=6.0):
        """fh_set_denoise_response_noise: while set_denoise_response is on and the call is given moments and counts, the clipped history is clamped once more, to the
        pixel's own colour +- kappa * sqrt(v + v_h) of the luminance variances it measured, and shortened by the larger excess: a moved emitter no longer lags next
        to where it was.  Stored but without effect while set_denoise_response is off, and in a call without moments (they exist while adaptive sampling is on)"""
        p = N.ResponseNoiseParamsC(float(kappa))
        self._ck(N.lib().fh_set_denoise_response_noise(self._ctx, C.byref(p)), "fh_set_denoise_response_noise")

    def clear_denoise_response_noise(self):
        self._ck(N.lib().fh_set_denoise_response_noise(self._ctx, None), "fh_set_denoise_response_noise")

    def get_denoise_response_noise(self):
        """(on, kappa): the switch and the kappa last set (6 before any)"""
        on, p = C.c_int(0), N.ResponseNoiseParamsC(0.0)
        self._ck(N.lib().fh_get_denoise_response_noise(self._ctx, C.byref(on), C.byref(p)), "fh_get_denoise_response_noise")
        return bool(on.value), float(p.kappa)

    def set_denoise_temporal_moments(self, min_history=2.0):
        """fh_set_denoise_temporal_moments: while on, denoise_temporal and denoise_temporal_motion keep the first and second moment of the luminance in the history,
        looked up and blended like the colour, and a call WITHOUT moments and counts takes its per-pixel variance from them once the pixel's history is min_history
        long (before that, from the 7 x 7 spatial estimate).  A call with moments keeps its bits.  Turning the switch on or off drops the history"""
        p = N.TemporalMomentsParamsC(float(min_history))
        self._ck(N.lib().fh_set_denoise_temporal_moments(self._ctx, C.byref(p)), "fh_set_denoise_temporal_moments")

    def clear_denoise_temporal_moments(self):
        self._ck(N.lib().fh_set_denoise_temporal_moments(self._ctx, None), "fh_set_denoise_temporal_moments")

    def get_denoise_temporal_moments(self):
        """(on, min_history): the switch and the min_history last set (the default before any)"""
        on, p = C.c_int(0), N.TemporalMomentsParamsC(0.0)
        self._ck(N.lib().fh_get_denoise_temporal_moments(self._ctx, C.byref(on), C.byref(p)), "fh_get_denoise_temporal_moments")
        return bool(on.value), float(p.min_history)

    def reset_denoise_history(self):
        """drop the history of denoise_temporal (fh_denoise_history_reset)"""
        self._ck(N.lib().fh_denoise_history_reset(self._ctx), "fh_denoise_history_reset")

    def denoise_history_info(self):
        """(width, height, frames accumulated since the last reset) of the history of denoise_temporal; (0, 0, 0) when there is none"""
        w, h, n = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self._ck(N.lib().fh_denoise_history_info(self._ctx, C.byref(w), C.byref(h), C.byref(n)), "fh_denoise_history_info")
        return w.value, h.value, n.value

    # -- parity-test hooks
    def measure_bandwidth(self, nbytes=1 << 30, iters=8):
        """(read GB/s, copy GB/s) of this GPU's HBM, measured with streaming kernels (fh_measure_bandwidth)"""
        r, c = C.c_double(0.0), C.c_double(0.0)
        self._ck(N.lib().fh_measure_bandwidth(self._ctx, C.c_uint64(nbytes), C.c_uint32(iters), C.byref(r), C.byref(c)), "fh_measure_bandwidth")
        return r.value, c.value

    def chief_rays(self, camera, width, height):
        """fh_kat_chief_rays: (height, width, 6) origin and direction of the chief rays primary_instances traces"""
        out = np.zeros((int(height), int(width), 6), dtype=np.float32)
        cam = camera.as_c()
        self._ck(N.lib().fh_kat_chief_rays(self._ctx, C.byref(cam), int(width), int(height), N.ptr(out)), "fh_kat_chief_rays")
        return out

    def trace_rays(self, rays7, any_hit=False):
        r = np.ascontiguousarray(rays7, dtype=np.float32).reshape(-1, 7)
        tuv = np.zeros((r.shape[0], 3), dtype=np.float32)
        prim = np.zeros(r.shape[0], dtype=np.uint32)
        self._ck(N.lib().fh_trace_rays(self._ctx, C.c_uint32(r.shape[0]), N.ptr(r), int(any_hit), N.ptr(tuv), N.ptr(prim)), "fh_trace_rays")
        return tuv, prim
