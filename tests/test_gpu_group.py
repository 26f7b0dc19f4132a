"""GPU tests (-m gpu): a group (fh_ctx_create_group) against a plain context of the same library, bit for bit.

Sampler keys are (pixel, per-pixel sample index, slot, seed) and every pixel's running means live in one place, so a frame split by tile across the members of a
group and gathered on the device must hold exactly the bits a plain context renders.  One visible device is enough: the groups [0, 0], [0, 0, 0] and [0, 0, 0, 0]
put several members on GPU 0 and take the same staging / copy / unpack path distinct devices take; [0] is the degenerate group (a plain context).  At most four
contexts exist at once: every plain render is finished, downloaded and its context destroyed before a group is made, and every test destroys what it made.
The tests zero-fill the caller's layers whenever they reset the render state, for the plain context and the group alike (include/fredholm_hip.h: what a caller may
observe at the first sample).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fredholm_amd as F
from fredholm_amd import distributed as D
from fredholm_amd import native as N
from fredholm_amd import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = F.RenderLayer.NAMES
GROUPS = ([0, 0], [0, 0, 0], [0, 0, 0, 0], [0])
SIZES = ((64, 48), (40, 24))  # 32 x 32 tiles: 48 is no multiple of the tile; 40 x 24 is two tiles, so members 2 and 3 own nothing
DEPTH = 8
CALLS = (1, 3, 16)
FH_E_INVALID, FH_E_UNSUPPORTED = -1, -3


def _device_count():
    import torch
    return torch.cuda.device_count()


def _scene(name):
    """(scene, camera, background, Hosek sky, environment of the context)"""
    if name == "cornell":
        return scenes.cornell_box(), F.Camera(**scenes.CORNELL_CAMERA), (0.0, 0.0, 0.0), False, {}
    if name == "textured":
        return scenes.textured_cornell_box(), F.Camera(**scenes.CORNELL_CAMERA), (0.1, 0.2, 0.4), False, {}
    if name == "soup_sky":  # the sky-pixel split forced on: k_sky_pixels and the passes both run
        cam = F.Camera(origin=(0.4, 0.2, 4.0), fov=1.2, F=16.0, focus=4.0, forward=(-0.15, -0.05, -1.0))
        return scenes.triangle_soup(3000, 0.1), cam, (0.05, 0.1, 0.2), True, {"FH_SKY_SPLIT_MIN_LOG2": "0"}
    raise KeyError(name)


_SC = {}


def _sc(name):
    if name not in _SC:
        _SC[name] = _scene(name)
    return _SC[name]


def _make(monkeypatch, devices, env=None):
    """devices None: a plain context; else the group over them (the environment is read at creation, by every member)"""
    for k in ("FH_SKY_SPLIT", "FH_PIPELINE", "FH_SKY_SPLIT_MIN_LOG2"):
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    r = F.Renderer(0) if devices is None else F.Renderer(devices=devices)
    for k in (env or {}):
        monkeypatch.delenv(k)
    assert r.group_size == (1 if devices is None else len(devices))
    return r


def _context(monkeypatch, name, devices, size, flags=0):
    sc, cam, bg, sky, env = _sc(name)
    r = _make(monkeypatch, devices, env)
    if flags:
        r.set_flags(flags)
    r.load_scene(sc)
    r.build_ias()
    if sky:
        r.set_directional_light((0.0, 0.0, 0.0), scenes.SOUP_SUN, 0.0)
        r.clear_directional_light()
        r.load_arhosek_sky(3.0, 0.3)
    r.set_resolution(*size)
    return r, F.RenderLayer(r, *size)


def _fresh(r, L):
    r.wait_for_completion()
    r.init_render_states()
    L.clear()


def _layers(r, L):
    r.wait_for_completion()
    return {n: L.download(n) for n in NAMES}


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.view(np.uint32) == b.view(np.uint32) if a.dtype == np.float32 else a == b


def _assert_same(got, want, what, keys=NAMES):
    for k in keys:
        assert got[k].shape == want[k].shape, (what, k)
        h, w = got[k].shape[:2]
        eq = _bits_equal(got[k], want[k]).reshape(h, w, -1).all(axis=2)  # (bytes: a NaN equals only the same NaN)
        bad = np.flatnonzero(~eq)
        assert bad.size == 0, f"{what}: {k} differs in {bad.size} of {h * w} pixels, the first at pixel {bad[0]}"


def _render_calls(r, L, name, calls=CALLS, depth=DEPTH):
    _, cam, bg, _, _ = _sc(name)
    for n in calls:
        r.render(cam, bg, L, n, depth)


_PLAIN = {}


def _plain_frame(monkeypatch, name, size, flags):
    key = (name, size, flags)
    if key not in _PLAIN:
        r, L = _context(monkeypatch, name, None, size, flags)
        _fresh(r, L)
        _render_calls(r, L, name)
        _PLAIN[key] = _layers(r, L)
        L.free()
        r.close()
    return _PLAIN[key]


# ------------------------------------------------------------------ 1. bit identity
@pytest.mark.parametrize("devices", GROUPS, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("firsthit", [False, True])
@pytest.mark.parametrize("name", ("cornell", "textured", "soup_sky"))
def test_group_renders_the_bits_of_a_plain_context(monkeypatch, name, firsthit, size, devices):
    flags = N.FLAG_REFERENCE_FIRSTHIT if firsthit else 0
    want = _plain_frame(monkeypatch, name, size, flags)
    r, L = _context(monkeypatch, name, devices, size, flags)
    try:
        _fresh(r, L)
        _render_calls(r, L, name)
        _assert_same(_layers(r, L), want, f"{name} {size} group {devices} firsthit={firsthit}")
        if name == "soup_sky" and not firsthit:
            assert r.stats()["sky_pixel_samples"] > 0  # the sky-pixel split was active
    finally:
        L.free()
        r.close()


def test_group_with_small_tiles_renders_the_same_bits(monkeypatch):
    """fh_set_tile_shard(group, 0, 1, 8, 8): 48 tiles of 8 x 8 dealt to three members"""
    size = SIZES[0]
    want = _plain_frame(monkeypatch, "cornell", size, 0)
    r, L = _context(monkeypatch, "cornell", [0, 0, 0], size)
    try:
        r.set_tile_shard(0, 1, 8, 8)
        _fresh(r, L)
        _render_calls(r, L, "cornell")
        _assert_same(_layers(r, L), want, "8 x 8 tiles")
    finally:
        L.free()
        r.close()


# ------------------------------------------------------------------ 2. gather mask
def test_gather_mask_brings_back_the_selected_layers_only(monkeypatch):
    size = SIZES[0]
    w, h = size
    want = _plain_frame(monkeypatch, "cornell", size, 0)
    devices = [0, 0, 0]
    r, L = _context(monkeypatch, "cornell", devices, size)
    try:
        r.set_gather_layers(N.LAYER_BEAUTY)
        r.wait_for_completion()
        r.init_render_states()
        for b in L._bufs.values():
            b.clear(0x7F)  # sentinel 0x7f7f7f7f: a finite positive float, so the lead's first sample (0 * old + x) is what it is over zeros
        _render_calls(r, L, "cornell")
        got = _layers(r, L)
        _assert_same(got, want, "beauty under the beauty mask", keys=("beauty",))
        lead = np.zeros(w * h, bool)
        lead[D.tile_ownership(w, h, 0, len(devices), 32, 32)] = True
        assert 0 < lead.sum() < w * h
        for k in NAMES[1:]:
            g = got[k].reshape(w * h, -1).view(np.uint32)
            p = want[k].reshape(w * h, -1).view(np.uint32)
            assert (g[lead] == p[lead]).all(), f"{k}: the lead's tiles"
            assert (g[~lead] == 0x7F7F7F7F).all(), f"{k}: tiles of the other members must stay untouched"
    finally:
        L.free()
        r.close()


# ------------------------------------------------------------------ 3. state changes reach every member
def _state_change_frames(r, gltf, tmp):
    """the same calls on a plain context and on a group: a frame after every state change"""
    frames = []
    size = [64, 48]
    cam = F.Camera(fov=0.5 * np.pi, F=100.0, focus=10000.0)
    L = [None]

    def frame(what):
        r.wait_for_completion()
        r.init_render_states()
        L[0].clear()
        r.render(cam, (0.02, 0.03, 0.05), L[0], 4, DEPTH)
        frames.append((what, _layers(r, L[0])))

    r.set_resolution(*size)
    L[0] = F.RenderLayer(r, *size)
    r.load_scene(gltf)
    r.build_ias()
    frame("animated glTF at t = 0")
    r.set_time(0.5)  # fh_set_transforms + fh_bvh_build: an instance moved
    frame("fh_set_transforms + fh_bvh_build")
    r.set_directional_light((5.0, 5.0, 4.0), scenes.SOUP_SUN, 1.0)
    frame("fh_set_directional_light")
    r.load_arhosek_sky(3.0, 0.3)
    frame("fh_load_arhosek_sky")
    r.load_scene(scenes.cornell_box())  # a second fh_scene_upload
    r.build_ias()
    frame("second fh_scene_upload")
    L[0].free()
    size[:] = [40, 24]
    r.set_resolution(*size)
    L[0] = F.RenderLayer(r, *size)
    frame("fh_set_resolution")
    r.set_path_pool(4096)
    frame("fh_set_path_pool")
    L[0].free()
    return frames


def test_state_changes_reach_every_member(monkeypatch, tmp_path):
    gltf = str(tmp_path / "anim.gltf")
    scenes.animated_cornell_gltf(gltf)
    r = _make(monkeypatch, None)
    want = _state_change_frames(r, gltf, tmp_path)
    r.close()
    assert not np.array_equal(want[0][1]["beauty"], want[1][1]["beauty"])  # the instance moved
    assert not np.array_equal(want[1][1]["beauty"], want[2][1]["beauty"])
    assert not np.array_equal(want[2][1]["beauty"], want[3][1]["beauty"])
    r = _make(monkeypatch, [0, 0, 0])
    try:
        got = _state_change_frames(r, gltf, tmp_path)
    finally:
        r.close()
    for (what, g), (_, p) in zip(got, want):
        _assert_same(g, p, f"after {what}")


# ------------------------------------------------------------------ 4. adaptive sampling on a group
def _adaptive_run(r, L, name, p, calls):
    _fresh(r, L)
    r.set_adaptive_sampling(p["threshold"], p["min_samples"], p["step"], p["floor"])
    _render_calls(r, L, name, calls)
    s = _layers(r, L)
    s["count"] = r.sample_counts()
    s["m"] = r.luminance_moments()
    return s, r.active_pixel_count(), r.stats()["paths"]


@pytest.mark.parametrize("devices", ([0, 0], [0, 0, 0, 0]), ids=lambda d: "x".join(map(str, d)))
def test_adaptive_sampling_on_a_group(monkeypatch, devices):
    name, size = "cornell", SIZES[0]
    cap, calls = 24, (8, 4, 4, 8)
    r, L = _context(monkeypatch, name, None, size)
    _fresh(r, L)
    r.set_adaptive_sampling(0.0, 8, 4, 0.01)  # threshold 0 tracks the moments and stops nothing: the error estimates after 8 samples give the threshold
    _render_calls(r, L, name, (8,))
    err = r.relative_error()
    t = float(np.median(err[np.isfinite(err)]))
    assert t > 0
    p = {"threshold": t, "min_samples": 8, "step": 4, "floor": 0.01}
    r.reset_stats()
    want, want_active, want_paths = _adaptive_run(r, L, name, p, calls)
    L.free()
    r.close()
    stopped = int((want["count"] < cap).sum())
    assert 0 < stopped < size[0] * size[1], "the threshold must stop part of the frame early"
    assert want_paths == int(want["count"].sum())
    r, L = _context(monkeypatch, name, devices, size)
    try:
        r.reset_stats()
        got, got_active, got_paths = _adaptive_run(r, L, name, p, calls)
        _assert_same(got, want, f"adaptive, group {devices}", keys=NAMES + ("count", "m"))
        assert got_active == want_active
        assert got_paths == int(got["count"].sum()) == want_paths
    finally:
        L.free()
        r.close()


# ------------------------------------------------------------------ 5. stats
def test_group_stats_add_up(monkeypatch):
    size = SIZES[0]
    n = 5
    r, L = _context(monkeypatch, "cornell", None, size)
    _fresh(r, L)
    r.reset_stats()
    _render_calls(r, L, "cornell", (n,))
    r.wait_for_completion()
    plain = r.stats()
    L.free()
    r.close()
    assert plain["paths"] == size[0] * size[1] * n
    devices = [0, 0, 0]
    r, L = _context(monkeypatch, "cornell", devices, size)
    try:
        _fresh(r, L)
        r.reset_stats()
        _render_calls(r, L, "cornell", (n,))
        r.wait_for_completion()
        s = r.stats()
        members = [r.member_stats(i) for i in range(len(devices))]
        assert s["paths"] == plain["paths"] == sum(m["paths"] for m in members)
        for i, m in enumerate(members):
            assert m["paths"] == n * D.tile_ownership(size[0], size[1], i, len(devices), 32, 32).size
        assert s["n_passes"] == sum(m["n_passes"] for m in members) >= len(devices)
        assert s["bvh_nodes"] == members[0]["bvh_nodes"] == plain["bvh_nodes"]
        assert s["render_ms"] == max(m["render_ms"] for m in members)
        assert r.owned_pixel_count() == size[0] * size[1]
        assert r.active_pixel_count() == size[0] * size[1]
    finally:
        L.free()
        r.close()


# ------------------------------------------------------------------ 6. refusals
def test_group_refusals(monkeypatch):
    size = SIZES[0]
    want = _plain_frame(monkeypatch, "cornell", size, 0)
    r, L = _context(monkeypatch, "cornell", [0, 0], size)
    lib = N.lib()
    try:
        buf = F.renderer.DeviceBuffer(r, size[0] * size[1] * 16)
        one = (C.c_void_p * 1)(buf.ptr)

        def refused(rc, code):
            msg = lib.fh_last_error(r._ctx)
            assert rc == code and msg, (rc, msg)

        refused(lib.fh_pack_owned(r._ctx, C.c_void_p(L.ptrs["beauty"]), C.c_uint32(4), C.c_void_p(buf.ptr)), FH_E_UNSUPPORTED)
        refused(lib.fh_unpack_shard(r._ctx, C.c_uint32(0), C.c_uint32(2), C.c_void_p(buf.ptr), C.c_uint32(4), C.c_void_p(L.ptrs["beauty"])), FH_E_UNSUPPORTED)
        refused(lib.fh_unpack_shards(r._ctx, C.c_uint32(1), one, C.c_uint32(4), C.c_void_p(L.ptrs["beauty"])), FH_E_UNSUPPORTED)
        counts = np.zeros(size[0] * size[1], np.uint32)
        refused(lib.fh_kat_sample_counts(r._ctx, N.ptr(counts), None, C.c_uint32(counts.size)), FH_E_UNSUPPORTED)
        refused(lib.fh_kat_set_sample_counts(r._ctx, N.ptr(counts), C.c_uint32(counts.size)), FH_E_UNSUPPORTED)
        out = np.zeros(30, np.float32)
        refused(lib.fh_kat_hosek_state(r._ctx, N.ptr(out)), FH_E_UNSUPPORTED)
        refused(lib.fh_set_tile_shard(r._ctx, C.c_uint32(1), C.c_uint32(2), C.c_uint32(32), C.c_uint32(32)), FH_E_INVALID)
        refused(lib.fh_set_tile_shard(r._ctx, C.c_uint32(0), C.c_uint32(2), C.c_uint32(32), C.c_uint32(32)), FH_E_INVALID)
        buf.free()
        # and the group still renders
        _fresh(r, L)
        _render_calls(r, L, "cornell")
        _assert_same(_layers(r, L), want, "after the refusals")
    finally:
        L.free()
        r.close()


def test_device_index_out_of_range_leaves_nothing_behind(monkeypatch):
    lib = N.lib()
    n_dev = _device_count()
    for devices in ([0, n_dev], [n_dev, 0], [0, 0, -1]):
        ctx = C.c_void_p(0xDEAD)
        rc = lib.fh_ctx_create_group((C.c_int * len(devices))(*devices), len(devices), C.byref(ctx))
        assert rc == FH_E_INVALID and ctx.value is None
        assert b"out of range" in lib.fh_last_error(None)
    size = SIZES[0]
    _PLAIN.pop(("cornell", size, 0), None)
    first = _plain_frame(monkeypatch, "cornell", size, 0)  # a plain context made afterwards renders what a group renders
    r, L = _context(monkeypatch, "cornell", [0, 0], size)
    try:
        _fresh(r, L)
        _render_calls(r, L, "cornell")
        _assert_same(_layers(r, L), first, "after the refused groups")
    finally:
        L.free()
        r.close()


# ------------------------------------------------------------------ 7. facade and driver
def _run_child(cmd, env=None, limit=300):
    """a fresh child process with its own time limit"""
    return subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=limit)


def test_batch_driver_writes_the_same_frames_on_a_group(tmp_path):
    exe = tmp_path / "rtcamp"
    cmd = ["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "rtcamp.cpp"), "-L" + os.path.join(ROOT, "fredholm_amd"), "-lfredholm_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "fredholm_amd"), "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", str(exe)]
    assert subprocess.run(cmd).returncode == 0
    gltf = str(tmp_path / "anim.gltf")
    scenes.animated_cornell_gltf(gltf, image_format="jpg")
    w, h, spp, depth, fps, n_frames = 80, 60, 3, 4, 2.0, 4
    base = ["--scene", gltf, "--width", str(w), "--height", str(h), "--spp", str(spp), "--depth", str(depth), "--fps", str(fps), "--max-time", str((n_frames - 1) / fps + 1e-3),
            "--fov", "90", "--F", "100", "--focus", "10000", "--bloom"]
    env = {k: v for k, v in os.environ.items() if k != "FH_DEVICES"}
    runs = {"plain": ([], env), "flag": (["--devices", "0,0,0"], env), "variable": ([], dict(env, FH_DEVICES="0,0")), "flag_wins": (["--devices", "0,0,0"], dict(env, FH_DEVICES="9,x"))}
    frames = {}
    for what, (extra, e) in runs.items():
        out = tmp_path / ("frames_" + what)
        run = _run_child([str(exe), *base, "--out", str(out), *extra], env=e)
        assert run.returncode == 0, what + ": " + run.stderr + run.stdout
        assert sorted(os.listdir(out)) == [f"{k}.png" for k in range(n_frames)]
        frames[what] = [open(out / f"{k}.png", "rb").read() for k in range(n_frames)]
        members = {"plain": None, "flag": 3, "variable": 2, "flag_wins": 3}[what]
        assert ("group of" in run.stdout) == (members is not None)
        if members:
            assert f"group of {members} members" in run.stdout
    assert frames["plain"][0] != frames["plain"][1]  # the blocks moved
    for what in ("flag", "variable", "flag_wins"):
        for k in range(n_frames):
            assert frames[what][k] == frames["plain"][k], f"{what}: frame {k}"


def test_python_group_properties(monkeypatch):
    r = _make(monkeypatch, [0, 0])
    try:
        assert r.group_size == 2
        r.set_gather_layers(N.LAYER_BEAUTY | N.LAYER_ALBEDO)
        with pytest.raises(F.FredholmError):
            r.set_gather_layers(64)
        with pytest.raises(F.FredholmError):
            r.member_stats(2)
        assert r.member_stats(1)["paths"] == 0
        assert r.gather_times() == (0.0, 0.0, 0.0)
    finally:
        r.close()
    r = _make(monkeypatch, [0])  # the degenerate group is a plain context
    try:
        assert r.group_size == 1
        r.set_gather_layers(N.LAYER_BEAUTY)  # accepted and ignored
        assert r.member_stats(0)["paths"] == 0
    finally:
        r.close()


# ------------------------------------------------------------------ 8. two real GPUs
@pytest.mark.skipif(_device_count() < 2, reason="needs two GPUs (peer copies between distinct devices)")
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("firsthit", [False, True])
def test_group_over_two_gpus_renders_the_bits_of_a_plain_context(monkeypatch, firsthit, size):
    flags = N.FLAG_REFERENCE_FIRSTHIT if firsthit else 0
    want = _plain_frame(monkeypatch, "cornell", size, flags)
    r, L = _context(monkeypatch, "cornell", [0, 1], size, flags)
    try:
        _fresh(r, L)
        _render_calls(r, L, "cornell")
        _assert_same(_layers(r, L), want, f"devices [0, 1] {size} firsthit={firsthit}")
    finally:
        L.free()
        r.close()
