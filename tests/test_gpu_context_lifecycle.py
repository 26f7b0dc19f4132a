"""What a context and a group own on the device comes and goes with them (fredholm_amd/csrc/fh_memory.h, context.h): fh_kat_live_allocations counts the device
buffers, pinned buffers, events and streams the library holds and their bytes, and after fh_ctx_destroy both are back where they were before fh_ctx_create --
whatever was switched on in between.  The layers and scratch images of the tests themselves come from fh_malloc, which is the caller's memory and is not counted.
The last test is the one a stale capacity would fail: a context resized up and back down renders the bits of a fresh one."""
import ctypes as C

import numpy as np
import pytest

import fredholm_amd as F
from fredholm_amd import native as N
from fredholm_amd import scenes
from fredholm_amd.renderer import DeviceBuffer

pytestmark = pytest.mark.gpu

BG = (0.0, 0.0, 0.0)


def live():
    count, nbytes = C.c_uint64(0), C.c_uint64(0)
    assert N.lib().fh_kat_live_allocations(C.byref(count), C.byref(nbytes)) == N.FH_OK
    return int(count.value), int(nbytes.value)


def cornell_with_cutout():
    """cornell_box_instanced() plus one quad in front of the back wall whose base-colour texture cuts holes (alpha 0 / 255 checker): alpha records and textures exist"""
    sc = scenes.cornell_box_instanced()
    quad = np.asarray([(-0.6, 0.9, -0.5), (0.2, 0.9, -0.5), (0.2, 1.7, -0.5), (-0.6, 0.9, -0.5), (0.2, 1.7, -0.5), (-0.6, 1.7, -0.5)], np.float32)
    nv = sc["vertices"].shape[0]
    card = N.default_materials(1)
    card["base_color_texture_id"][0] = 0
    sc["vertices"] = np.concatenate([sc["vertices"], quad])
    sc["normals"] = np.concatenate([sc["normals"], np.tile(np.asarray([[0, 0, 1]], np.float32), (6, 1))])
    sc["texcoords"] = np.concatenate([sc["texcoords"], np.asarray([[0, 0], [1, 0], [1, 1], [0, 0], [1, 1], [0, 1]], np.float32)])
    sc["indices"] = np.concatenate([sc["indices"], np.arange(nv, nv + 6, dtype=np.uint32).reshape(2, 3)])
    sc["material_ids"] = np.concatenate([sc["material_ids"], np.full(2, len(sc["materials"]), np.uint32)])
    sc["instance_ids"] = np.concatenate([sc["instance_ids"], np.zeros(2, np.uint32)])
    sc["materials"] = np.concatenate([sc["materials"], card])
    sc["textures"] = [{"rgba8": scenes.checker_texture(32, 32, 4, (40, 200, 60), (0, 0, 0), alpha0=255, alpha1=0, seed=9), "srgb": True}]
    return sc


def test_a_context_with_everything_on_gives_back_all_it_took():
    before = live()
    r = F.Renderer(0)
    try:
        created = live()
        assert created[0] > before[0] and created[1] > before[1]
        r.load_scene(cornell_with_cutout())
        r.build_ias()
        assert r.alpha_face_counts()[0] == 2  # (the card's two faces can cut)
        w, h = 32, 24
        cam = F.Camera(**scenes.CORNELL_CAMERA)
        r.set_resolution(w, h)
        L = F.RenderLayer(r, w, h)
        r.set_flags(N.FLAG_REFERENCE_FIRSTHIT)
        r.render(cam, BG, L, 2, 4)
        r.set_flags(0)
        r.init_render_states()
        r.set_adaptive_policy(block=4, growth=1)
        r.set_adaptive_sampling(0.05, min_samples=2, step=2)
        L.clear()
        r.render(cam, BG, L, 4, 4)
        r.wait_for_completion()
        px = w * h
        moments, counts, out, tmp, hi = (DeviceBuffer(r, n) for n in (8 * px, 4 * px, 16 * px, 16 * px, 16 * px))
        r.get_luminance_moments(moments.ptr)
        r.get_sample_counts(counts.ptr)
        p = L.ptrs
        r.denoise(w, h, p["beauty"], p["normal"], p["albedo"], out.ptr)
        r.denoise_guided(w, h, p["beauty"], p["normal"], p["albedo"], out.ptr, p["position"], p["depth"], moments.ptr, counts.ptr)
        r.set_denoise_motion(True)
        r.set_denoise_response(1.0)
        r.set_denoise_response_noise(6.0)
        r.set_denoise_temporal_moments(2.0)
        r.denoise_temporal(w, h, p["beauty"], p["normal"], p["albedo"], out.ptr, p["position"], p["depth"], cam, moments.ptr, counts.ptr)
        r.set_transforms(*scenes.instanced_transforms((-0.19, 0.0, 0.0)))  # (the short block moves: the second call looks its history up through the motion table)
        r.build_ias()
        r.denoise_temporal(w, h, p["beauty"], p["normal"], p["albedo"], out.ptr, p["position"], p["depth"], cam, moments.ptr, counts.ptr)
        assert r.denoise_history_info()[2] == 2
        r.set_auto_exposure()
        r.post_process(p["beauty"], hi.ptr, tmp.ptr, w, h, F.PostProcessParams(use_bloom=True), out.ptr)
        packed = DeviceBuffer(r, 16 * px)
        packed.clear()  # (fh_malloc does not: without this the frame below is whatever a freed buffer held, 0xffffffff words included)
        for rank in (0, 1):
            r.unpack_shard(rank, 2, packed.ptr, 4, out.ptr)
        r.wait_for_completion()
        assert np.isfinite(out.download()).all()
        full = live()
        assert full[0] > created[0] and full[1] > created[1]
        for b in (moments, counts, out, tmp, hi, packed):
            b.free()
        L.free()
        r.set_resolution(40, 40)
        L = F.RenderLayer(r, 40, 40)
        r.render(cam, BG, L, 1, 4)
        r.set_path_pool(4096)
        r.render(cam, BG, L, 1, 4)
        r.set_transforms(*scenes.instanced_transforms((0.1, 0.0, 0.0)))
        r.build_ias()  # (a refit)
        r.wait_for_completion()
        assert np.isfinite(L.download("beauty")).all()
        L.free()
        assert live()[0] > before[0] and live()[1] > before[1]
    finally:
        r.close()
    assert live() == before


def test_a_group_of_two_on_one_device_gives_back_all_it_took():
    before = live()
    r = F.Renderer(devices=[0, 0])
    try:
        assert live()[0] > before[0]
        r.load_scene(scenes.cornell_box())
        r.build_ias()
        cam = F.Camera(**scenes.CORNELL_CAMERA)
        for w, h in ((64, 48), (40, 72)):  # (more than one 32 x 32 tile each way: both members own pixels)
            r.set_resolution(w, h)
            L = F.RenderLayer(r, w, h)
            r.render(cam, BG, L, 2, 4)
            r.wait_for_completion()
            assert np.isfinite(L.download("beauty")).all()
            L.free()
        assert live()[1] > before[1]
    finally:
        r.close()
    assert live() == before


def test_pools_that_grow_render_the_bits_of_pools_that_never_had_to(monkeypatch):
    """render.hip: pool_ensure.  A pool slot is re-made when a pass needs more paths than it holds or a kind of record it has no room for.  One context, its new pools
    full of 0xa5 (FH_POISON=1), meets every reason in turn -- more paths, the directional light's slot, the light record of a scene with emitters over one without --
    and renders the bits of a context whose pools had the largest shape and size before its first frame.  Pass j of a context runs in slot j % 3, so every step is
    three one-pass calls: each slot meets each reason.  fh_path_pool_allocated grows with every step, and fh_set_path_pool gives everything back."""
    w, h, depth = 64, 48, 4
    cam = F.Camera(**scenes.CORNELL_CAMERA)
    sky = (0.5, 0.6, 0.8)  # (the dark box is lit through its open front)
    lit = scenes.cornell_box()
    dark = dict(scenes.cornell_box())
    dark["materials"] = dark["materials"].copy()
    dark["materials"]["emission"][:] = 0.0
    dark["materials"]["emission_color"][:] = 0.0

    def steps(r, L):
        frames, held = [], []

        def calls(n_samples):
            for _ in range(3):
                r.render(cam, sky, L, n_samples, depth)
                r.wait_for_completion()
                frames.append({n: L.download(n).view(np.uint32) for n in F.RenderLayer.NAMES})
            held.append(r.path_pool_allocated())

        calls(1)
        calls(6)  # more paths
        r.set_directional_light((3.0, 3.0, 3.0), (0.2, 1.0, 0.9), 0.0)
        calls(6)  # the directional light's shadow ray
        r.load_scene(lit)
        r.build_ias()
        assert r.n_lights() == 2
        calls(6)  # the pending light-ray record
        return frames, held

    before = live()
    monkeypatch.setenv("FH_POISON", "1")
    r = F.Renderer(0)
    try:
        r.load_scene(dark)
        r.build_ias()
        assert r.n_lights() == 0
        r.set_resolution(w, h)
        L = F.RenderLayer(r, w, h)
        grown, held = steps(r, L)
        r.set_path_pool(4096)
        released = r.path_pool_allocated()
        L.free()
    finally:
        r.close()
    assert live() == before
    monkeypatch.delenv("FH_POISON")
    r = F.Renderer(0)
    try:
        r.load_scene(lit)
        r.build_ias()
        r.set_directional_light((3.0, 3.0, 3.0), (0.2, 1.0, 0.9), 0.0)
        r.set_resolution(w, h)
        L = F.RenderLayer(r, w, h)
        for _ in range(3):  # every slot: six samples of the largest shape
            r.render(cam, sky, L, 6, depth)
        r.wait_for_completion()
        roomy = r.path_pool_allocated()
        r.clear_directional_light()
        r.load_scene(dark)
        r.build_ias()
        r.init_render_states()
        L.clear()
        fitted, held_fitted = steps(r, L)
        L.free()
    finally:
        r.close()
    assert live() == before
    n_px = w * h
    assert [p for _, p in held] == [3 * n_px, 18 * n_px, 18 * n_px, 18 * n_px]
    assert all(a[0] < b[0] for a, b in zip(held, held[1:])), held
    assert released == (0, 0)
    assert held[-1] == roomy and held_fitted == [roomy] * 4  # (the second context never re-made a pool)
    assert len(grown) == len(fitted) == 12
    assert all(f["beauty"].view(np.float32)[..., :3].mean() > 0.01 for f in grown)  # (pictures, not cleared buffers)
    for k, (a, b) in enumerate(zip(grown, fitted)):
        for name in F.RenderLayer.NAMES:
            assert np.array_equal(a[name], b[name]), (k, name)


def _six_layers(r, cam, w, h):
    L = F.RenderLayer(r, w, h)
    r.render(cam, BG, L, 2, 4)
    r.wait_for_completion()
    out = {n: L.download(n) for n in F.RenderLayer.NAMES}
    L.free()
    return out


def test_a_resize_round_trip_renders_the_bits_of_a_fresh_context():
    cam = F.Camera(**scenes.CORNELL_CAMERA)

    def context():
        r = F.Renderer(0)
        r.load_scene(scenes.cornell_box())
        r.build_ias()
        return r

    fresh = context()
    try:
        fresh.set_resolution(32, 24)
        want = _six_layers(fresh, cam, 32, 24)
    finally:
        fresh.close()
    r = context()
    try:
        r.set_resolution(32, 24)
        first = _six_layers(r, cam, 32, 24)
        r.set_resolution(48, 40)
        _six_layers(r, cam, 48, 40)
        r.set_resolution(32, 24)
        r.init_render_states()
        again = _six_layers(r, cam, 32, 24)
    finally:
        r.close()
    assert want["beauty"][..., :3].mean() > 0.01  # (a picture, not a cleared buffer)
    for name in F.RenderLayer.NAMES:
        assert np.array_equal(first[name].view(np.uint32), want[name].view(np.uint32)), name
        assert np.array_equal(again[name].view(np.uint32), want[name].view(np.uint32)), name
