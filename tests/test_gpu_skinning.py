"""GPU tests (-m gpu) of skeletal skinning (include/fredholm_hip.h: fh_skin_desc; scene.hip: k_skin_vertices).

  posed arrays   fh_get_posed_geometry equals the numpy restatement of the header's text (tests/skin_model.py) bit for bit, at the edges of the 256-thread workgroup
  renders        a context that sets a skin and a pose renders, in every bit of all six layers and of the sample counts, what a fresh context renders that uploaded
                 the restated posed arrays as a plain static scene -- through a kept refit, a rebuild, a discarded refit and successive poses, composed with
                 fh_set_transforms in either order, with the light table and the light proxies on, on a group, and through Renderer.set_time
  lifecycle      a skin alone and a cleared skin keep the bind pose's bits; an upload drops the skin; refusals change nothing; the context gives back all it took

Frames are 48 x 36 with 4 samples and depth 4 on fredholm_amd.scenes_skinned's arm in the Cornell box."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fredholm_amd as F
import skin_model as M
from fredholm_amd import native as N
from fredholm_amd import scenes
from fredholm_amd import scenes_skinned as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = F.RenderLayer.NAMES
W, H, SPP, DEPTH = 48, 36, 4, 4
FH_E_INVALID = -1
f32 = np.float32

ARM = S.arm_scene()
SKIN_KEYS = ("joints", "weights", "n_joints", "joint_matrices")
SMALL, LARGE = S.arm_joint_matrices(0.2, -0.3), S.arm_joint_matrices(0.9, 0.8, scale=8.0)
POSES = (S.arm_joint_matrices(-0.4, 0.5), SMALL, S.arm_joint_matrices(0.7, 0.6))


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _posed(pal, sc=ARM):
    return M.pose(pal, sc["joints"], sc["weights"], sc["vertices"], sc["normals"])


def _static_scene(pal, transforms=None, sc=ARM):
    """the scene with the restated posed arrays in place of the bind ones and no skin"""
    out = {k: v for k, v in sc.items() if k not in SKIN_KEYS}
    if pal is not None:
        out["vertices"], out["normals"] = _posed(pal, sc)
    if transforms is not None:
        out["object_to_world"], out["world_to_object"] = transforms
    return out


def _frame(r, setup=None, cam=None):
    """all six layers and the sample counts of one frame from a fresh render state"""
    r.set_resolution(W, H)
    L = F.RenderLayer(r, W, H)
    L.clear()
    if setup:
        setup(r)
    r.render(cam or F.Camera(**scenes.CORNELL_CAMERA), (0.0, 0.0, 0.0), L, SPP, DEPTH)
    r.wait_for_completion()
    out = {n: L.download(n) for n in NAMES}
    out["counts"] = r.sample_counts()
    return out


def _assert_same(got, want, what):
    for k in want:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape, (what, k)
        bad = np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)).reshape(H * W, -1).any(axis=1))
        assert bad.size == 0, f"{what}: {k} differs in {bad.size} of {H * W} pixels, the first at pixel {bad[0]}"
    assert (want["counts"] == SPP).all() and np.isfinite(want["beauty"]).all() and want["beauty"][..., :3].max() > 0


_STATIC = {}


def _static_frame(pal, transforms=None, setup=None, key=None):
    """the frame of a fresh context that uploaded the restated arrays as a plain static scene (computed once per key)"""
    if key is None or key not in _STATIC:
        r = F.Renderer(0)
        try:
            r.load_scene(_static_scene(pal, transforms))
            r.build_ias()
            out = _frame(r, setup)
            out["n_lights"] = r.n_lights()
        finally:
            r.close()
        if key is None:
            return out
        _STATIC[key] = out
    return _STATIC[key]


def _layers_only(frame):
    return {k: v for k, v in frame.items() if k != "n_lights"}


def _skinned_renderer(built=True):
    r = F.Renderer(0)
    r.load_scene(_static_scene(None))
    if built:
        r.build_ias()
    r.set_skin(ARM["joints"], ARM["weights"], ARM["n_joints"])
    return r


# ------------------------------------------------------------------ posed arrays
@pytest.mark.parametrize("nv", (1, 255, 256, 257, 1000))
def test_posed_geometry_equals_the_restatement_bit_for_bit(nv):
    rng = np.random.default_rng(100 + nv)
    nf = max(1, nv // 3)
    base = scenes.cornell_box()
    sc = {"indices": (np.arange(3 * nf, dtype=np.uint32) % nv).reshape(nf, 3), "material_ids": np.zeros(nf, np.uint32), "materials": base["materials"][:1],
          "texcoords": np.zeros((nv, 2), f32)}
    r = F.Renderer(0)
    try:
        for nj in (1, 2, 300):
            j, w, p, n = M.random_vertices(rng, nv, nj, unskinned_share=0.25 if nv > 1 else 0.0)
            n[::3] *= f32(2.5)
            r.load_scene(dict(sc, vertices=p, normals=n))
            assert r.skin_info() == (0, 0, False)
            r.set_skin(j, w, nj)
            got = r.posed_geometry()
            assert (_bits(got[0]) == _bits(p)).all() and (_bits(got[1]) == _bits(n)).all()  # a skin alone: the bind arrays
            zero = (w == 0).all(axis=1)
            assert r.skin_info() == (nj, int((~zero).sum()), False) and (nv == 1 or zero.any())
            assert int(j[~zero].max()) == nj - 1
            for scales in ((0.7, 1.4), (0.05, 20.0)):
                pal = M.random_palette(rng, nj, scales)
                r.set_joint_matrices(pal)
                got, want = r.posed_geometry(), M.pose(pal, j, w, p, n)
                assert (_bits(got[0]) == _bits(want[0])).all() and (_bits(got[1]) == _bits(want[1])).all(), (nv, nj, scales)
                assert (_bits(got[0][zero]) == _bits(p[zero])).all() and (_bits(got[1][zero]) == _bits(n[zero])).all()
            assert r.skin_info()[2] is True
    finally:
        r.close()


# ------------------------------------------------------------------ render equivalence
@pytest.mark.parametrize("case", ("small pose: refit kept", "FH_REFIT=0: rebuild", "large pose: refit discarded"))
def test_a_posed_render_equals_the_static_upload_of_the_restated_arrays(case, monkeypatch, capfd):
    pal = LARGE if case.startswith("large") else SMALL
    want = _static_frame(pal, key="large" if pal is LARGE else "small")
    monkeypatch.setenv("FH_DEBUG_BVH", "1")  # (read at every build: the [bvh] lines say which path ran)
    if case.startswith("FH_REFIT"):
        monkeypatch.setenv("FH_REFIT", "0")
    r = _skinned_renderer()
    try:
        capfd.readouterr()
        r.set_joint_matrices(pal)
        r.build_ias()
        err = capfd.readouterr().err
        print(case, "->", [ln for ln in err.splitlines() if ln.startswith("[bvh]")])
        if case.startswith("small"):
            assert "[bvh] refit 1:" in err and "refit discarded" not in err
        elif case.startswith("large"):
            assert "[bvh] refit discarded" in err
        else:
            assert "[bvh] refit" not in err
        got = r.posed_geometry()
        assert (_bits(got[0]) == _bits(_posed(pal)[0])).all() and (_bits(got[1]) == _bits(_posed(pal)[1])).all()
        _assert_same(_frame(r), _layers_only(want), case)
    finally:
        r.close()


def test_three_successive_poses_on_one_context():
    r = _skinned_renderer()
    try:
        for k, pal in enumerate(POSES):
            r.set_joint_matrices(pal)
            r.build_ias()
            _assert_same(_frame(r), _layers_only(_static_frame(pal, key="small" if pal is SMALL else "pose%d" % k)), "pose %d" % k)
    finally:
        r.close()


def _arm_transforms():
    """both instances moved: the room turned a little about y, the arm shifted and scaled"""
    c, s = np.cos(0.1), np.sin(0.1)
    m0 = np.array([[c, 0, s, 0.02], [0, 1, 0, 0.0], [-s, 0, c, -0.03], [0, 0, 0, 1]])
    m1 = np.array([[1.1, 0, 0, -0.3], [0, 0.9, 0, 0.3], [0, 0, 1.2, -0.1], [0, 0, 0, 1]])
    o2w = np.stack([m[:3].reshape(12) for m in (m0, m1)]).astype(f32)
    w2o = np.stack([np.linalg.inv(m)[:3].reshape(12) for m in (m0, m1)]).astype(f32)
    return o2w, w2o


@pytest.mark.parametrize("order", ("transforms first", "pose first"))
def test_set_transforms_composes_on_top_in_either_order(order):
    xf = _arm_transforms()
    want = _static_frame(SMALL, transforms=xf, key="composed")
    r = _skinned_renderer()
    try:
        if order == "pose first":
            r.set_joint_matrices(SMALL)
            r.set_transforms(*xf)
        else:
            r.set_transforms(*xf)
            r.set_joint_matrices(SMALL)
        r.build_ias()
        _assert_same(_frame(r), _layers_only(want), order)
    finally:
        r.close()


@pytest.mark.parametrize("resampling", (False, True))
def test_the_light_table_and_the_proxies_follow_the_pose(resampling):
    def setup(r):
        r.set_light_sampling()
        if resampling:
            r.set_light_resampling()
    want = _static_frame(SMALL, setup=setup, key="lights%d" % resampling)
    plain = _static_frame(SMALL, key="small")
    assert want["n_lights"] == 2 + 2 * S.ARM_SEGMENTS and not (_bits(want["beauty"]) == _bits(plain["beauty"])).all()  # (the switch does change the frame)
    r = _skinned_renderer()
    try:
        setup(r)
        _frame(r)  # the table and the proxies of the bind pose are built and used ...
        r.set_joint_matrices(SMALL)
        r.build_ias()
        _assert_same(_frame(r), _layers_only(want), "light sampling, resampling %s" % resampling)  # ... and rebuilt for the pose
        assert r.n_lights() == want["n_lights"]
    finally:
        r.close()


# ------------------------------------------------------------------ lifecycle
def test_skin_alone_clear_skin_and_a_repeated_pose():
    bind = _static_frame(None, key="bind")
    posed = _static_frame(SMALL, key="small")
    assert not (_bits(bind["beauty"]) == _bits(posed["beauty"])).all()
    r = _skinned_renderer()
    try:
        _assert_same(_frame(r), _layers_only(bind), "a skin alone")
        r.set_joint_matrices(SMALL)
        r.build_ias()
        first = r.posed_geometry()
        _assert_same(_frame(r), _layers_only(posed), "posed")
        builds = r.stats()["bvh_build_ms"]
        r.set_joint_matrices(SMALL.copy())  # the pose held: nothing moves, the tree stays valid
        r.build_ias()
        again = r.posed_geometry()
        assert (_bits(first[0]) == _bits(again[0])).all() and (_bits(first[1]) == _bits(again[1])).all() and r.stats()["bvh_build_ms"] == builds
        _assert_same(_frame(r), _layers_only(posed), "the same pose again")
        r.clear_skin()
        r.build_ias()
        assert r.skin_info() == (0, 0, False)
        got = r.posed_geometry()
        assert (_bits(got[0]) == _bits(ARM["vertices"])).all() and (_bits(got[1]) == _bits(ARM["normals"])).all()
        _assert_same(_frame(r), _layers_only(bind), "after clear_skin")
    finally:
        r.close()


def test_an_upload_drops_the_skin_and_refusals_change_nothing():
    lib = N.lib()
    r = _skinned_renderer(built=False)
    try:
        r.set_joint_matrices(SMALL)
        before = r.posed_geometry()
        nv = ARM["vertices"].shape[0]
        j, w = np.ascontiguousarray(ARM["joints"], np.uint16), np.ascontiguousarray(ARM["weights"], f32)

        def skin(nv_, nj, jj, ww):
            d = N.SkinDescC(nv_, nj, N.ptr(jj), N.ptr(ww))
            return lib.fh_set_skin(r._ctx, C.byref(d))

        def bad(a, v):
            a = a.copy()
            a[-1, 1] = v
            return a
        refused = [skin(nv - 1, 3, j, w), skin(nv, 3, None, w), skin(nv, 3, j, None), skin(nv, 0, j, w), skin(nv, 65537, j, w), skin(nv, 2, j, w), skin(nv, 3, bad(j, 3), w),
                   skin(nv, 3, j, bad(w, np.nan)), lib.fh_set_joint_matrices(r._ctx, 3, None), lib.fh_set_joint_matrices(r._ctx, 2, N.ptr(SMALL)),
                   lib.fh_set_joint_matrices(r._ctx, 4, N.ptr(np.tile(SMALL[:1], (4, 1)))), lib.fh_set_joint_matrices(r._ctx, 3, N.ptr(bad(SMALL, np.inf)))]
        assert refused == [FH_E_INVALID] * len(refused)
        assert b"not finite" in lib.fh_last_error(r._ctx)
        after = r.posed_geometry()
        assert r.skin_info() == (3, nv - 36, True) and (_bits(before[0]) == _bits(after[0])).all() and (_bits(before[1]) == _bits(after[1])).all()
        assert (_bits(after[0]) == _bits(_posed(SMALL)[0])).all()
        r.load_scene(_static_scene(None))  # fh_scene_upload drops the skin
        assert r.skin_info() == (0, 0, False)
        assert lib.fh_set_joint_matrices(r._ctx, 3, N.ptr(SMALL)) == FH_E_INVALID and b"no skin set" in lib.fh_last_error(r._ctx)
        got = r.posed_geometry()
        assert (_bits(got[0]) == _bits(ARM["vertices"])).all()
        r.build_ias()
        _assert_same(_frame(r), _layers_only(_static_frame(None, key="bind")), "after the upload")
    finally:
        r.close()
    fresh = F.Renderer(0)  # no scene: both setters refuse
    try:
        d = N.SkinDescC(nv, 3, N.ptr(j), N.ptr(w))
        assert lib.fh_set_skin(fresh._ctx, C.byref(d)) == FH_E_INVALID and lib.fh_set_skin(fresh._ctx, None) == FH_E_INVALID
        assert lib.fh_set_joint_matrices(fresh._ctx, 3, N.ptr(SMALL)) == FH_E_INVALID
    finally:
        fresh.close()


def _live():
    count, nbytes = C.c_uint64(0), C.c_uint64(0)
    assert N.lib().fh_kat_live_allocations(C.byref(count), C.byref(nbytes)) == N.FH_OK
    return int(count.value), int(nbytes.value)


def test_a_skinned_context_gives_back_all_it_took():
    before = _live()
    r = _skinned_renderer()
    try:
        assert _live()[0] >= before[0] + 5  # (the skin's five buffers)
        r.set_joint_matrices(POSES[0])
        r.build_ias()
        posed_once = _live()
        for pal in POSES[1:]:
            r.set_joint_matrices(pal)
            r.build_ias()
        assert _live() == posed_once  # further poses take nothing
        r.set_skin(ARM["joints"], ARM["weights"], ARM["n_joints"])  # a second skin replaces the first
        r.set_joint_matrices(SMALL)
        r.build_ias()
        assert _live() == posed_once
    finally:
        r.close()
    assert _live() == before


# ------------------------------------------------------------------ group
def test_a_group_gives_the_plain_contexts_bits_after_a_pose():
    want = _static_frame(SMALL, key="small")
    r = F.Renderer(devices=[0, 0])
    try:
        assert r.group_size == 2
        r.load_scene(_static_scene(None))
        r.build_ias()
        r.set_skin(ARM["joints"], ARM["weights"], ARM["n_joints"])
        r.set_joint_matrices(SMALL)
        r.build_ias()
        assert r.skin_info() == (3, ARM["vertices"].shape[0] - 36, True)
        got = r.posed_geometry()
        assert (_bits(got[0]) == _bits(_posed(SMALL)[0])).all()
        _assert_same(_frame(r), _layers_only(want), "group [0, 0]")
    finally:
        r.close()


# ------------------------------------------------------------------ facades
def test_a_dict_scene_with_a_skin_and_a_pose_loads_posed():
    r = F.Renderer(0)
    try:
        r.load_scene(dict(ARM, joint_matrices=SMALL))
        r.build_ias()
        assert r.skin_info()[2] is True
        _assert_same(_frame(r), _layers_only(_static_frame(SMALL, key="small")), "load_scene(dict with a pose)")
    finally:
        r.close()


LINK = ["-L" + os.path.join(ROOT, "fredholm_amd"), "-lfredholm_hip", "-Wl,-rpath," + os.path.join(ROOT, "fredholm_amd"), "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
FACADE_TIMES = (0.5, 1.75)


def test_set_time_poses_the_asset_in_python_and_in_the_cpp_facade(tmp_path):
    """Renderer.set_time(t) on the glTF asset: posed_geometry equals the restatement of the loader's matrices and the render the static upload of those arrays (with the
    camera node's pose); fredholm::Renderer::load_scene + set_time on the same file (tests/cpp/skin_facade.cpp) gives the same bytes"""
    from fredholm_amd.scene import Scene
    gltf = tmp_path / "arm.gltf"
    S.write_arm_gltf(str(gltf))
    python_bytes = b""
    r = F.Renderer(0)
    try:
        r.load_scene(str(gltf))
        r.build_ias()
        assert r.skin_info() == (3, ARM["vertices"].shape[0] - 36, True)
        got = r.posed_geometry()
        python_bytes += got[0].tobytes() + got[1].tobytes()
        for t in FACADE_TIMES:
            r.set_time(t)
            sc = Scene()
            sc.load_model(str(gltf))
            sc.update_animation(t)
            pal = sc.joint_matrices_3x4()
            assert not np.array_equal(pal, S.arm_joint_matrices(0.0, 0.0))
            got, want = r.posed_geometry(), _posed(pal)
            assert (_bits(got[0]) == _bits(want[0])).all() and (_bits(got[1]) == _bits(want[1])).all(), t
            python_bytes += got[0].tobytes() + got[1].tobytes()
            static = sc.as_dict()
            for k in SKIN_KEYS:
                static.pop(k)
            static["vertices"], static["normals"] = want
            q = F.Renderer(0)
            try:
                q.load_scene(static)
                q.build_ias()
                cam = F.Camera(**scenes.CORNELL_CAMERA)
                cam.m_transform = sc.camera_transform_3x4()  # (the pose the asset's camera node gives the renderer that loaded the file)
                ref = _frame(q, cam=cam)
            finally:
                q.close()
            _assert_same(_frame(r), ref, "set_time(%g)" % t)
    finally:
        r.close()
    exe = tmp_path / "skin_facade"
    c = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "skin_facade.cpp"), *LINK, "-lpthread", "-o", str(exe)],
                       capture_output=True, text=True)
    assert c.returncode == 0, c.stderr
    run = subprocess.run([str(exe), str(tmp_path / "facade.bin"), str(gltf), *[repr(float(t)) for t in FACADE_TIMES]], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert (tmp_path / "facade.bin").read_bytes() == python_bytes
