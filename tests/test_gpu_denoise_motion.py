"""Tests of the per-instance motion vectors of temporal accumulation (include/fredholm_hip.h: fh_primary_instances, fh_motion_from_transforms,
fh_denoise_temporal_motion, fh_set_denoise_motion; fredholm_amd/csrc/motion.hip and denoise.hip: k_temporal<kLookMotion, .>).  The restatement of
test_gpu_denoise_temporal.py is extended by the motion stage as the header states it, in float64 and in float32, and the device is held to that suite's bound:
4 x the largest float32-versus-float64 difference of the same case.  The tests marked gpu need the device; the host motion function, the chief-ray restatement's
own consistency and the share of carried pixels that find a history are checked on the CPU.

Observed on an MI355X: (device error) / (float32 error) = 1.000 in all 98 comparisons of this file (every device value has the float32 restatement's bits; float32
error 1.9e-7 ... 3.2e-6, so the device is held to 7.8e-7 ... 1.3e-5).  Chief rays: 0 ulp per component from the float32 numpy restatement in all six cases, the rotated
camera's included.  Quality: see test_quality_on_a_sequence_with_a_moving_box.
"""
import ctypes as C

import numpy as np
import pytest

import fredholm_amd as F
from fredholm_amd import native as N
from fredholm_amd import scenes
from fredholm_amd.renderer import DeviceBuffer

import test_gpu_denoise_temporal as T
from test_gpu_denoise_temporal import FAR, NAMES, NEAR, SIZES, STEP_X, TDEF, Dev, _bits, _compare, _dot3, _grow, _hit, _random_beauty, _relmse, _two_planes, inv_tan

gpu = pytest.mark.gpu
MISS = 0xFFFFFFFF
IDENT = np.asarray([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)


# ------------------------------------------------------------------ the motion table, restated
def motion_np(o2w_prev, w2o_prev, o2w_cur, w2o_cur):
    """the header's formulas: in float64 from the float32 inputs, sums in the order written, rounded once"""
    A, Dm, Cm, B = (np.asarray(a, np.float32).astype(np.float64).reshape(-1, 12) for a in (o2w_prev, w2o_prev, o2w_cur, w2o_cur))
    n = A.shape[0]
    point, normal = np.zeros((n, 12), np.float64), np.zeros((n, 9), np.float64)
    for i in range(3):
        for j in range(4):
            s = (A[:, 4 * i] * B[:, j] + A[:, 4 * i + 1] * B[:, 4 + j]) + A[:, 4 * i + 2] * B[:, 8 + j]
            point[:, 4 * i + j] = s + A[:, 4 * i + 3] if j == 3 else s
        for j in range(3):
            normal[:, 3 * i + j] = (Cm[:, 4 * j] * Dm[:, i] + Cm[:, 4 * j + 1] * Dm[:, 4 + i]) + Cm[:, 4 * j + 2] * Dm[:, 8 + i]
    prev = np.concatenate([np.asarray(o2w_prev, np.float32).reshape(-1, 12), np.asarray(w2o_prev, np.float32).reshape(-1, 12)], axis=1)
    cur = np.concatenate([np.asarray(o2w_cur, np.float32).reshape(-1, 12), np.asarray(w2o_cur, np.float32).reshape(-1, 12)], axis=1)
    moved = (prev.view(np.uint32) != cur.view(np.uint32)).any(axis=1)
    return point.astype(np.float32), normal.astype(np.float32), moved


def table_arrays(table):
    n = len(table)
    return (np.array([list(m.point) for m in table], np.float32).reshape(n, 12), np.array([list(m.normal) for m in table], np.float32).reshape(n, 9),
            np.array([m.moved for m in table], np.uint32))


def affine(rot=np.eye(3), t=(0.0, 0.0, 0.0)):
    """(o2w, w2o) of x -> rot x + t as 12 floats each; the inverse is formed in float64 and rounded once"""
    rot, t = np.asarray(rot, np.float64), np.asarray(t, np.float64)
    inv = np.linalg.inv(rot)
    return np.concatenate([rot, t[:, None]], axis=1).astype(np.float32).reshape(12), np.concatenate([inv, (-inv @ t)[:, None]], axis=1).astype(np.float32).reshape(12)


def rot_y(angle, pivot=(0.0, 0.0, 0.0)):
    """(rot, t) of the rotation by `angle` about the axis through `pivot` parallel to y"""
    c, s = np.cos(angle), np.sin(angle)
    r = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    p = np.asarray(pivot, np.float64)
    return r, p - r @ p


# ------------------------------------------------------------------ 1: the host motion function (CPU)
def test_motion_struct_has_the_header_layout_and_the_symbols_their_signatures():
    assert C.sizeof(N.MotionC) == 88 and N.MotionC.point.offset == 0 and N.MotionC.normal.offset == 48 and N.MotionC.moved.offset == 84
    L = N.load_library()
    for name in ("fh_primary_instances", "fh_motion_from_transforms", "fh_denoise_temporal_motion", "fh_set_denoise_motion", "fh_get_denoise_motion", "fh_kat_chief_rays"):
        assert name in N.EXPORTS and getattr(L, name).argtypes == N.SIGNATURES[name]


def test_motion_from_transforms_matches_the_float64_product_bit_for_bit():
    rng = np.random.default_rng(3)
    ident = affine()
    cases = {"equal bits": (ident, ident), "translation": (ident, affine(t=(0.25, -0.5, 0.125)))}
    r1, t1 = rot_y(0.7, (0.3, 0.0, -1.0))
    q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    cases["rotation and non-uniform scale"] = (affine(q @ np.diag([0.5, 1.7, 1.1]), (0.1, 0.2, -0.3)), affine(r1 @ q @ np.diag([0.8, 1.2, 2.0]), t1 + (0.4, 0.0, 0.1)))
    cases["random affine"] = (affine(rng.normal(size=(3, 3)), rng.normal(size=3)), affine(rng.normal(size=(3, 3)), rng.normal(size=3)))
    names = list(cases)
    prev_o, prev_w = np.stack([cases[k][0][0] for k in names]), np.stack([cases[k][0][1] for k in names])
    cur_o, cur_w = np.stack([cases[k][1][0] for k in names]), np.stack([cases[k][1][1] for k in names])
    got = table_arrays(N.motion_from_transforms(prev_o, prev_w, cur_o, cur_w))
    want = motion_np(prev_o, prev_w, cur_o, cur_w)
    assert _bits(got[0], want[0]) and _bits(got[1], want[1])
    assert list(got[2]) == [0, 1, 1, 1] and list(want[2]) == [False, True, True, True]
    # a pure translation by t: the points were at P - t, exactly; the normals were what they are
    assert _bits(got[0][1], np.asarray([1, 0, 0, -0.25, 0, 1, 0, 0.5, 0, 0, 1, -0.125], np.float32)) and _bits(got[1][1], np.eye(3, dtype=np.float32).reshape(9))
    # the stated formulas, independently of motion_np: point = o2w_prev * w2o_cur, normal = (L(o2w_cur) * L(w2o_prev))^T = inverse transpose of point's linear part
    for k in (2, 3):
        h = lambda m: np.vstack([m.astype(np.float64).reshape(3, 4), [0, 0, 0, 1]])
        P = (h(prev_o[k]) @ h(cur_w[k]))[:3]
        G = (h(cur_o[k])[:3, :3] @ h(prev_w[k])[:3, :3]).T
        assert np.abs(got[0][k].reshape(3, 4) - P).max() <= 4 * np.finfo(np.float32).eps * np.abs(P).max()
        assert np.abs(got[1][k].reshape(3, 3) - G).max() <= 4 * np.finfo(np.float32).eps * np.abs(G).max()
        assert np.abs(got[1][k].reshape(3, 3) - np.linalg.inv(P[:, :3]).T).max() <= 1e-5 * np.abs(G).max()  # (the float32 inverses are inverses to ~1e-7)
    # a moved bit anywhere in the 24 floats counts: -0.0 against 0.0 in one world_to_object entry
    w2 = prev_w.copy()
    w2[0, 3] = -0.0
    assert table_arrays(N.motion_from_transforms(prev_o, prev_w, prev_o, w2))[2][0] == 1
    assert len(N.motion_from_transforms(prev_o[:0], prev_w[:0], prev_o[:0], prev_w[:0])) == 0
    assert N.lib().fh_motion_from_transforms(1, None, None, None, None, None) == -1


def test_motion_host_check_program_passes(tmp_path):
    """the motion table and the refusals as a stand-alone host program (the one the host sanitizers are run on)"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "motion_host_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", os.path.join(root, "tools", "motion_host_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "ok" in run.stdout, run.stdout


OK_T, OK_P = (0.2, 32.0, 0.9, 0.02), (2.0, 1.0, 0.2, 7, 5)
FULL = [0x1000 * (k + 1) for k in range(7)]  # (made-up device addresses: never dereferenced)


def _host_call(ids=0x9000, n=2, motion="ok", ptrs=FULL, w=8, h=8, camera="default"):
    i = N.DenoiseInputsC(*ptrs)
    cam = F.Camera(origin=(0.0, 0.0, 1.0)).as_c() if camera == "default" else camera
    if motion == "ok":
        motion = N.motion_from_transforms([IDENT, IDENT], [IDENT, IDENT], [IDENT, affine(t=(0.1, 0, 0))[0]], [IDENT, affine(t=(0.1, 0, 0))[1]])
    rc = N.lib().fh_denoise_temporal_motion(None, w, h, C.byref(i), None if cam is None else C.byref(cam), C.byref(N.TemporalParamsC(*OK_T)), C.byref(N.DenoiseParamsC(*OK_P)), ids, n,
                                            motion, 1 << 20, 0)
    return rc, N.lib().fh_last_error(None).decode()


def _bad_table(where, value):
    t = N.motion_from_transforms([IDENT, IDENT], [IDENT, IDENT], [IDENT, affine(t=(0.1, 0, 0))[0]], [IDENT, affine(t=(0.1, 0, 0))[1]])
    getattr(t[1], where)[4] = value
    return t


def test_motion_refusals_are_decided_before_the_context_is_touched():
    """no GPU: with a NULL context an accepted call gets as far as the context check, a refused one does not"""
    for kw in (dict(), dict(ids=None, n=0, motion=None), dict(ids=None, n=2, motion=None)):
        rc, msg = _host_call(**kw)
        assert rc == -1 and msg == "fh_denoise_temporal_motion: null context", (kw, msg)
    refused = [(dict(motion=None), "together"), (dict(ids=None), "together"), (dict(n=0), "n_instances"), (dict(motion=_bad_table("point", float("nan"))), "finite"),
               (dict(motion=_bad_table("normal", float("inf"))), "finite"), (dict(camera=None), "null camera"), (dict(w=0), "width"),
               (dict(ptrs=FULL[:3] + [None, None] + FULL[5:]), "position and depth layers are required")]
    for kw, word in refused:
        rc, msg = _host_call(**kw)
        assert rc == -1 and msg.startswith("fh_denoise_temporal_motion: ") and word in msg and "null context" not in msg, (kw, msg)
    assert N.lib().fh_set_denoise_motion(None, 1) == -1 and N.lib().fh_get_denoise_motion(None, None) == -1 and N.lib().fh_primary_instances(None, None, 8, 8, None) == -1


# ------------------------------------------------------------------ the stage, restated
def stage_motion(dt, hist, cam15, c, v, normal, position, depth, ids, table, alpha_min, max_history, normal_cos_min, plane_tol):
    """fh_denoise_temporal_motion's stage as the header states it; table = (point[n, 12], normal[n, 9], moved[n]) in float32"""
    Nn, Pp, Z = normal[..., :3].astype(dt), position[..., :3].astype(dt), depth.astype(dt)
    hh, ww = v.shape
    hit = _hit(Nn)
    lim = dt(np.float32(plane_tol)) * np.maximum(Z, dt(np.float32(1e-3)))
    cos_min = dt(np.float32(normal_cos_min))
    n = table[2].shape[0]
    inside_table = ids < n
    safe = np.where(inside_table, ids, 0).astype(np.int64)
    carried = inside_table & (table[2][safe] != 0)
    A, G = table[0].astype(dt)[safe], table[1].astype(dt)[safe]
    with np.errstate(all="ignore"):
        Pc = np.stack([((A[..., 4 * k] * Pp[..., 0] + A[..., 4 * k + 1] * Pp[..., 1]) + A[..., 4 * k + 2] * Pp[..., 2]) + A[..., 4 * k + 3] for k in range(3)], axis=-1)
        Nc = np.stack([(G[..., 3 * k] * Nn[..., 0] + G[..., 3 * k + 1] * Nn[..., 1]) + G[..., 3 * k + 2] * Nn[..., 2] for k in range(3)], axis=-1)
    Pb, Nb = np.where(carried[..., None], Pc, Pp), np.where(carried[..., None], Nc, Nn)

    def valid(Nref, Pref, Nq, Pq):
        return _hit(Nq) & (_dot3(Nref, Nq) >= cos_min) & (np.abs(_dot3(Nref, Pq - Pref)) <= lim)
    still = np.array_equal(hist["cam"].view(np.uint32), np.asarray(cam15, np.float32).view(np.uint32))
    own = ~carried & still
    with np.errstate(all="ignore"):
        have_own = valid(Nn, Pp, hist["N"], hist["P"])
        x, y, t = T.reproject(dt, Pb, hist["m"], hist["f"], ww, hh)
        xs, ys = x - dt(0.5), y - dt(0.5)
        ix, iy = np.floor(xs), np.floor(ys)
        fx, fy = xs - ix, ys - iy
        S, sc, sv, sh = np.zeros(v.shape, dt), np.zeros(c.shape, dt), np.zeros(v.shape, dt), np.zeros(v.shape, dt)
        for j in (0, 1):
            for i in (0, 1):
                tx, ty = ix + dt(i), iy + dt(j)
                inside = (tx >= 0) & (tx <= dt(ww - 1)) & (ty >= 0) & (ty <= dt(hh - 1))
                qx, qy = np.where(inside, tx, 0).astype(np.int64), np.where(inside, ty, 0).astype(np.int64)
                wgt = (fx if i else dt(1) - fx) * (fy if j else dt(1) - fy)
                ok = (t > 0) & inside & valid(Nb, Pb, hist["N"][qy, qx], hist["P"][qy, qx])
                S = S + np.where(ok, wgt, dt(0))
                sc = sc + np.where(ok[..., None], wgt[..., None] * hist["c"][qy, qx], dt(0))
                sv = sv + np.where(ok, wgt * hist["v"][qy, qx], dt(0))
                sh = sh + np.where(ok, wgt * hist["h"][qy, qx], dt(0))
        have = np.where(own, have_own, (t > 0) & (S >= dt(np.float32(1e-3)))) & hit
        c_h = np.where(own[..., None], hist["c"], sc / S[..., None])
        v_h, h_h = np.where(own, hist["v"], sv / S), np.where(own, hist["h"], sh / S)
        hn = np.minimum(h_h + dt(1), dt(np.float32(max_history)))
        a = np.maximum(dt(1) / hn, dt(np.float32(alpha_min)))
        b = dt(1) - a
        c_acc = np.where(have[..., None], b[..., None] * c_h + a[..., None] * c, c)
        v_acc = np.where(have, (b * b) * v_h + (a * a) * v, v)
    h_out = np.where(hit, np.where(have, hn, dt(1)), dt(0))
    return c_acc.astype(dt), v_acc.astype(dt), h_out.astype(dt), have, carried & hit


class MotionRestatement(T.Restatement):
    """the restatement of the temporal suite with fh_denoise_temporal_motion's call beside fh_denoise_temporal's"""

    def call_motion(self, layers, cam15, ids, table, use_moments=True, upscale=False, temporal=None, sigma_l=2.0, sigma_z=1.0, sigma_a=0.2, normal_power_log2=7, passes=5):
        if self.hist is None or self.hist["v"].shape != layers["depth"].shape or not table[2].any():
            return self.call(layers, cam15, use_moments, upscale, temporal, sigma_l, sigma_z, sigma_a, normal_power_log2, passes)
        dt, tp, cam15 = self.dt, dict(TDEF, **(temporal or {})), np.asarray(cam15, np.float32)
        with np.errstate(all="ignore"):
            c, v, af = T.prepare(dt, layers["beauty"], layers["normal"], layers["albedo"], layers["moments"] if use_moments else None, layers["counts"] if use_moments else None,
                                 normal_power_log2)
            self.c_in, self.v_in = c, v
            c, v, h, self.have, self.carried = stage_motion(dt, self.hist, cam15, c, v, layers["normal"], layers["position"], layers["depth"], ids, table, **tp)
            self.hist = dict(c=c, v=v, h=h, P=layers["position"][..., :3].astype(dt), N=layers["normal"][..., :3].astype(dt), cam=cam15.copy(), m=T.world_to_camera(cam15[:12]),
                             f=inv_tan(cam15[12]))
            self.frames += 1
            out = T.passes_of(dt, self.exp, c, v, af, layers["normal"], layers["albedo"], layers["position"], layers["depth"], sigma_l, sigma_z, sigma_a, normal_power_log2, passes, upscale)
        assert out.dtype == dt
        return out


def motion_restatements(oracle):
    return MotionRestatement(np.float64, np.exp), MotionRestatement(np.float32, lambda x: oracle.elementary("exp", x).reshape(x.shape))


def dev_motion(r, layers, cam, ids, table, use_moments=True, upscale=False, temporal=None, **params):
    """one fh_denoise_temporal_motion call on the device: ids a (h, w) uint32 array or None, table a ctypes array of MotionC or None"""
    d = Dev(r, layers)
    idb = None
    try:
        if ids is not None:
            idb = DeviceBuffer(r, ids.nbytes)
            idb.upload(np.ascontiguousarray(ids, np.uint32))
        p, out = d.bufs, d._out(upscale)
        r.denoise_temporal_motion(d.w, d.h, p["beauty"].ptr, p["normal"].ptr, p["albedo"].ptr, out.ptr, p["position"].ptr, p["depth"].ptr, cam, None if idb is None else idb.ptr, table,
                                  p["moments"].ptr if use_moments else None, p["counts"].ptr if use_moments else None, upscale=upscale, **dict(TDEF, **(temporal or {})), **params)
        return d._get(out, upscale)
    finally:
        if idb is not None:
            idb.free()
        d.free()


def dev_plain(r, layers, cam, **kw):
    d = Dev(r, layers)
    try:
        return d.temporal(cam, **kw)
    finally:
        d.free()


class MotionSequence(T.Sequence):
    """the device and the two restatements fed the same calls, with and without motion"""

    def __init__(self, r, oracle):
        self.r, (self.r64, self.r32) = r, motion_restatements(oracle)
        r.reset_denoise_history()

    def call_motion(self, what, layers, cam, ids, table, **kw):
        got = dev_motion(self.r, layers, cam, ids, table, **kw)
        arrays = table_arrays(table)
        o64, o32 = self.r64.call_motion(layers, cam.params(), ids, arrays, **kw), self.r32.call_motion(layers, cam.params(), ids, arrays, **kw)
        return got, o32, _compare(what, got, o64, o32)


# ------------------------------------------------------------------ inputs: two planes, the near one an instance that moves rigidly
def planes_moved(w, h, cam, seed, rot=np.eye(3), t=(0.0, 0.0, 0.0)):
    """_two_planes with the near plane (instance 1: z = NEAR where x < STEP_X, in ITS OWN frame) carried by x -> rot x + t, seen along the chief rays of `cam`; the far plane
    z = FAR (instance 0) stays.  Returns the layers, the id plane (MISS where the normal is 0) and the near mask."""
    rot, t = np.asarray(rot, np.float64), np.asarray(t, np.float64)
    tc, f = np.asarray(cam.m_transform, np.float64), float(inv_tan(cam.m_fov))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    uvx, uvy = -(2.0 * (xx + 0.5) - w) / h, (2.0 * (yy + 0.5) - h) / h
    d = np.stack([-uvx, -uvy, np.full(uvx.shape, -f)], axis=2)
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    org = tc[:, :3] @ np.array([0.0, 0.0, f]) + tc[:, 3]
    dw = d @ tc[:, :3].T
    n_near = rot @ np.array([0.0, 0.0, 1.0])
    p0 = rot @ np.array([0.0, 0.0, NEAR]) + t
    s_near = ((p0 - org) @ n_near) / (dw @ n_near)
    hit_near = org + s_near[..., None] * dw
    obj = (hit_near - t) @ rot  # (rot^-1 = rot^T applied to row vectors)
    near = (obj[..., 0] < STEP_X) & (s_near > 0)
    s = np.where(near, s_near, (FAR - org[2]) / dw[..., 2])
    pos = np.zeros((h, w, 4), np.float32)
    pos[..., :3] = org + s[..., None] * dw
    pos[..., 2] = np.where(near, NEAR + t[2] if np.array_equal(rot, np.eye(3)) else pos[..., 2], FAR)  # exactly on the planes (a tilted one: as exactly as float32 has it)
    nrm = np.zeros((h, w, 4), np.float32)
    nrm[..., :3] = np.where(near[..., None], n_near, np.array([0.0, 0.0, 1.0]))
    nrm[h - 1, 0] = 0.0  # a miss
    pos[h - 1, 0] = 0.0
    rng = np.random.default_rng(seed)
    alb = np.zeros((h, w, 4), np.float32)
    alb[..., :3] = rng.uniform(0.2, 0.9, (h, w, 3)).astype(np.float32)
    layers = dict(normal=nrm, albedo=alb, position=pos, depth=s.astype(np.float32), **_random_beauty(alb, rng, np.where(near, 1.5, 0.6)))
    hit = _hit(nrm)
    ids = np.where(hit, np.where(near, 1, 0), MISS).astype(np.uint32)
    return layers, ids, near & hit


def pixel_on_near(h, pixels):
    """world units that are `pixels` pixels on the near plane for the cameras of _cameras (x = (W + H * Q.x / t) / 2: H / (2 t) pixels per unit, t = (f - (NEAR - 0.5)) / f)"""
    f = float(inv_tan(0.5 * np.pi))
    return pixels * 2.0 * ((f - (NEAR - 0.5)) / f) / h


def motion_cases(w, h):
    """the near plane's pose in the second frame: slid in its own plane by 2.3 pixels, moved along its normal by 10 x the plane tolerance, rotated about an in-plane axis"""
    depth_max = 0.5 - NEAR + 1.0  # (generous: the chief rays' distances to the near plane are 3.5 ... 4.5)
    return {"slide": (np.eye(3), (pixel_on_near(h, 2.3), 0.0, 0.0)), "normal": (np.eye(3), (0.0, 0.0, 10.0 * TDEF["plane_tol"] * depth_max)),
            "rotate": rot_y(0.12, (-0.4, 0.0, NEAR))}


def motion_case(size, case, moved_camera, seed=81):
    """[(camera, layers, ids, table)] of the two calls, and the near masks of both"""
    w, h = SIZES[size]
    a, b = T._cameras(w, h, T.SHIFT[size])
    rot, t = motion_cases(w, h)[case]
    first, ids1, near1 = planes_moved(w, h, a, seed)
    cam2 = b if moved_camera else a
    second, ids2, near2 = planes_moved(w, h, cam2, seed + 1, rot, t)
    ident, cur = affine(), affine(rot, t)
    table = N.motion_from_transforms([IDENT, ident[0]], [IDENT, ident[1]], [IDENT, cur[0]], [IDENT, cur[1]])
    return [(a, first, ids1, None), (cam2, second, ids2, table)], near1, near2


def _restated_shares(oracle, size, case, moved_camera):
    calls, near1, near2 = motion_case(size, case, moved_camera)
    r32 = motion_restatements(oracle)[1]
    r32.call(calls[0][1], calls[0][0].params(), passes=1)
    r32.call_motion(calls[1][1], calls[1][0].params(), calls[1][2], table_arrays(calls[1][3]), passes=1)
    plain = motion_restatements(oracle)[1]
    plain.call(calls[0][1], calls[0][0].params(), passes=1)
    plain.call(calls[1][1], calls[1][0].params(), passes=1)
    return r32, plain, near2


def test_motion_cases_carry_most_of_the_near_plane_to_a_history(oracle):
    """no GPU: in every case of the next test the carried pixels (the near plane) are the ones that take the new path, and at 37 x 29 more than 60 % of them find a history
    where the plain call finds one for fewer than half as many (slide: the plain call still finds the same plane, so it is exempt)"""
    for size in SIZES:
        for case in ("slide", "normal", "rotate"):
            for moved_camera in (False, True):
                r32, plain, near2 = _restated_shares(oracle, size, case, moved_camera)
                assert np.array_equal(r32.carried, near2) and near2.any()
                assert size == "5x3" or (~near2 & _hit(r32.hist["N"])).sum() > 100  # (5 x 3: 2.3 pixels are half the frame, the slid plane covers it)
                with_m, without = float(r32.have[near2].mean()), float(plain.have[near2].mean())
                print(f"motion case {size} {case} moved camera {moved_camera}: near pixels {int(near2.sum())}, with a history {with_m:.3f} (plain call {without:.3f})")
                if size == "37x29":
                    assert with_m > 0.6, (size, case, with_m)
                    assert case == "slide" or without < 0.5 * with_m, (size, case, with_m, without)
                assert np.array_equal(r32.have[~near2], plain.have[~near2])


# ------------------------------------------------------------------ 2: the id plane and the chief rays
def chief_rays_np(cam, w, h):
    """float32 restatement of the header's chief ray, operation by operation"""
    f32 = np.float32
    tr = np.asarray(cam.params()[:12], f32)
    f, focus = inv_tan(cam.m_fov), f32(cam.m_focus)
    apb = f32(f32(1) / f32(f32(f32(1) + f) - f32(f32(1) / focus))) + focus
    yy, xx = np.mgrid[0:h, 0:w]
    W, H = f32(w), f32(h)
    ux = -((f32(2) * (xx.astype(f32) + f32(0.5)) - W) / H)
    uy = (f32(2) * (yy.astype(f32) + f32(0.5)) - H) / H

    def normalize(v):
        inv = f32(1) / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        return [v[0] * inv, v[1] * inv, v[2] * inv]
    zero = np.zeros_like(ux)
    s = normalize([zero - ux, zero - uy, f - zero])
    k = apb / s[2]
    o = [ux + k * s[0], uy + k * s[1], zero + k * s[2]]
    d = normalize([o[0] - zero, o[1] - zero, o[2] - f])
    d[2] = d[2] * f32(-1)
    out = np.zeros((h, w, 6), f32)
    for i in range(3):
        out[..., i] = ((tr[4 * i] * zero + tr[4 * i + 1] * zero) + tr[4 * i + 2] * f) + tr[4 * i + 3] * f32(1)
        out[..., 3 + i] = ((tr[4 * i] * d[0] + tr[4 * i + 1] * d[1]) + tr[4 * i + 2] * d[2]) + tr[4 * i + 3] * f32(0)
    assert out.dtype == f32
    return out


ID_CAMERA = dict(origin=(0.0, 1.0, 3.0), fov=0.5 * np.pi, F=100.0, focus=10000.0)  # pulled back: the rays at the frame's sides pass the box by
ID_SCENES = [("instanced", 64, 48), ("instanced", 5, 3), ("textured", 64, 48)]


@gpu
@pytest.mark.parametrize("name,w,h", ID_SCENES)
def test_id_plane_is_the_traced_chief_rays_instance(name, w, h):
    sc = scenes.cornell_box_instanced() if name == "instanced" else scenes.textured_cornell_box()
    inst = np.asarray(sc.get("instance_ids", np.zeros(sc["indices"].shape[0], np.uint32)), np.uint32)
    r = F.Renderer(0)
    try:
        r.load_scene(sc)
        r.build_ias()
        if name == "textured":
            assert r.alpha_face_counts()[0] > 0  # (the ALPHA instantiation runs)
        for cam in (F.Camera(**ID_CAMERA), F.Camera(origin=(0.3, 1.2, 2.6), fov=0.4 * np.pi, F=8.0, focus=3.0, forward=(-0.2, -0.1, -1.0))):
            rays = r.chief_rays(cam, w, h)
            want6 = chief_rays_np(cam, w, h)
            rotated = cam.m_forward != (0.0, 0.0, -1.0)
            mag = np.abs(want6)  # per component, for the rotated camera too
            ulps = np.abs(rays.astype(np.float64) - want6.astype(np.float64)) / np.spacing(np.maximum(mag, np.float32(1e-30)))
            print(f"chief rays {name} {w}x{h} rotated={rotated}: largest difference from the float32 restatement {ulps.max():.2f} ulp")
            assert ulps.max() <= 4.0
            rays7 = np.concatenate([rays.reshape(-1, 6), np.full((w * h, 1), 1e9, np.float32)], axis=1)
            _, prim = r.trace_rays(rays7, any_hit=False)
            want = np.where(prim == MISS, MISS, inst[np.minimum(prim, len(inst) - 1)]).astype(np.uint32).reshape(h, w)
            buf = DeviceBuffer(r, 4 * w * h)
            buf.clear(0x5A)
            r.primary_instances(cam, w, h, buf.ptr)
            r.wait_for_completion()
            got = buf.download(np.uint32, (h, w))
            buf.free()
            assert np.array_equal(got, want)
            if not rotated:
                assert (want == MISS).any() and (want == 0).any() and (name != "instanced" or (w, h) != (64, 48) or (want == 1).sum() > 20)
    finally:
        r.close()


def _id_planes(save_to=None):
    """the id planes of ID_SCENES under ID_CAMERA by fh_primary_instances, and the same from fh_trace_rays on the hook's rays; optionally saved as an .npz"""
    out = {}
    for name, w, h in ID_SCENES:
        sc = scenes.cornell_box_instanced() if name == "instanced" else scenes.textured_cornell_box()
        inst = np.asarray(sc.get("instance_ids", np.zeros(sc["indices"].shape[0], np.uint32)), np.uint32)
        r = F.Renderer(0)
        try:
            r.load_scene(sc)
            r.build_ias()
            cam = F.Camera(**ID_CAMERA)
            rays7 = np.concatenate([r.chief_rays(cam, w, h).reshape(-1, 6), np.full((w * h, 1), 1e9, np.float32)], axis=1)
            _, prim = r.trace_rays(rays7, any_hit=False)
            buf = DeviceBuffer(r, 4 * w * h)
            r.primary_instances(cam, w, h, buf.ptr)
            r.wait_for_completion()
            out[f"{name}_{w}x{h}"] = buf.download(np.uint32, (h, w))
            out[f"{name}_{w}x{h}_traced"] = np.where(prim == MISS, MISS, inst[np.minimum(prim, len(inst) - 1)]).astype(np.uint32).reshape(h, w)
            buf.free()
        finally:
            r.close()
    if save_to:
        np.savez(save_to, **out)
    return out


@gpu
def test_id_plane_does_not_depend_on_the_traversal_entry_point(tmp_path):
    """FH_COOP=0 (read once when a context is created, so in a child process of its own) sends fh_primary_instances through k_primary_instances and `traverse`, and
    fh_trace_rays through its per-lane kernel; this process takes the wave-cooperative kernels.  All four id planes of a scene agree in every pixel."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    path = str(tmp_path / "ids.npz")
    code = f"import sys; sys.path[:0] = [{os.path.dirname(here)!r}, {here!r}]; import test_gpu_denoise_motion as M; M._id_planes({path!r})"
    run = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, FH_COOP="0"), capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    child, mine = np.load(path), _id_planes()
    assert sorted(child.files) == sorted(mine) and len(mine) == 2 * len(ID_SCENES)
    for k, v in mine.items():
        assert np.array_equal(child[k], v), k
        assert np.array_equal(v, mine[k.replace("_traced", "") + "_traced"]), k
    assert (mine["instanced_64x48"] == 1).sum() > 20 and (mine["instanced_64x48"] == MISS).any()


# ------------------------------------------------------------------ 3: the stage against the restatement
@gpu
@pytest.mark.parametrize("use_moments", [True, False])
@pytest.mark.parametrize("passes", [1, 5])
@pytest.mark.parametrize("moved_camera", [False, True])
@pytest.mark.parametrize("case", ["slide", "normal", "rotate"])
@pytest.mark.parametrize("size", list(SIZES))
def test_stage_matches_the_restatement(renderer, oracle, size, case, moved_camera, passes, use_moments):
    """device / float32 error ratio: 1.000 in every case (see the module docstring)"""
    calls, _, near2 = motion_case(size, case, moved_camera)
    seq = MotionSequence(renderer, oracle)
    what = f"motion {size} {case} moved camera={moved_camera} passes={passes} mom={use_moments}"
    seq.call(what + " first", calls[0][1], calls[0][0], use_moments=use_moments, passes=passes)
    seq.call_motion(what + " second", calls[1][1], calls[1][0], calls[1][2], calls[1][3], use_moments=use_moments, passes=passes)
    assert np.array_equal(seq.r32.carried, near2)
    if size == "37x29":
        assert seq.r32.have[near2].mean() > 0.6
    assert renderer.denoise_history_info() == SIZES[size] + (2,)


# ------------------------------------------------------------------ 4: the limit is gone
@gpu
def test_moved_geometry_keeps_its_history_with_motion(renderer, oracle):
    """test_moved_geometry_gets_no_history's scenario -- the near plane moves along its normal by 10 x the plane tolerance under a still camera -- through
    fh_denoise_temporal_motion: what the plain call loses (that test pins it) is kept"""
    w, h = SIZES["37x29"]
    cam, _ = T._cameras(w, h)
    first, near = _two_planes(w, h, cam, 71)
    move = 10.0 * 0.02 * float(first["depth"][near].max())
    second, near2 = _two_planes(w, h, cam, 72, near_z=NEAR + move)
    both, hitp = near & near2, _hit(first["normal"])
    ids = np.where(_hit(second["normal"]), np.where(near2, 1, 0), MISS).astype(np.uint32)
    cur = affine(t=(0.0, 0.0, move))
    table = N.motion_from_transforms([IDENT, IDENT], [IDENT, IDENT], [IDENT, cur[0]], [IDENT, cur[1]])
    seq = MotionSequence(renderer, oracle)
    seq.call("kept history, first", first, cam, passes=1)
    got, _, _ = seq.call_motion("kept history, second", second, cam, ids, table, passes=1)
    st = seq.r32
    assert both.sum() > 100 and st.have[both].all() and (st.hist["h"][both] == 2).all()
    assert near2.sum() > 100 and st.have[near2].all() and (st.hist["h"][near2] == 2).all()  # every pixel of the moved plane, the newly covered ones included
    far = hitp & ~near & ~near2
    assert far.sum() > 100 and st.have[far].all() and (st.hist["h"][far] == 2).all()
    d = Dev(renderer, second)
    try:
        spatial = d.guided(passes=1)
    finally:
        d.free()
    inner = ~_grow(~both, 2)
    assert inner.sum() > 50 and (got[inner] != spatial[inner]).any(axis=1).mean() > 0.9
    renderer.reset_denoise_history()
    dev_plain(renderer, first, cam, passes=1)
    plain = dev_plain(renderer, second, cam, passes=1)
    inner_far = ~_grow(~far, 2)
    assert inner_far.sum() > 50 and _bits(got[inner_far], plain[inner_far])
    assert _bits(plain[inner], spatial[inner])  # (the plain call: the limit the other test pins)


# ------------------------------------------------------------------ 5: nothing moved means the old bits
def _plain_sequence(r, frames, **kw):
    r.reset_denoise_history()
    return [dev_plain(r, layers, cam, **kw) for cam, layers in frames]


@gpu
def test_an_unmoved_table_gives_the_plain_calls_bits(renderer):
    frames = T._abc("37x29", 91)
    want = _plain_sequence(renderer, frames)
    o, wo = affine(np.diag([1.0, 2.0, 0.5]), (0.3, 0.1, 0.2))
    table = N.motion_from_transforms([IDENT, o], [IDENT, wo], [IDENT, o], [IDENT, wo])
    assert [m.moved for m in table] == [0, 0]
    renderer.reset_denoise_history()
    rng = np.random.default_rng(5)
    garbage = rng.integers(0, 3, (29, 37)).astype(np.uint32)  # (never read)
    got = [dev_motion(renderer, layers, cam, garbage, table) for cam, layers in frames]
    assert all(_bits(x, y) for x, y in zip(want, got))
    renderer.reset_denoise_history()
    got = [dev_motion(renderer, layers, cam, None, None) for cam, layers in frames]
    assert all(_bits(x, y) for x, y in zip(want, got))
    assert renderer.denoise_history_info() == (37, 29, 3)


@gpu
def test_carried_pixels_with_identity_maps_take_the_moved_cameras_look_up_bit_for_bit(renderer):
    """k_temporal<kLookMotion, .> takes the 2 x 2 look-up of k_temporal<kLookReproject, .>: with every pixel carried by maps that are the identity (a table marked moved by
    hand), Pb and Nb have P's and N's bits, so under a moved camera the whole call must equal the plain one in every pixel"""
    frames = T._abc("37x29", 94)  # cameras A, B, A: the second and third call reproject
    want = _plain_sequence(renderer, frames)
    table = (N.MotionC * 1)()
    for k in range(12):
        table[0].point[k] = float(IDENT[k])
    for k in range(9):
        table[0].normal[k] = 1.0 if k % 4 == 0 else 0.0
    table[0].moved = 1
    ids = np.zeros((29, 37), np.uint32)
    renderer.reset_denoise_history()
    got = [dev_motion(renderer, layers, cam, ids, table) for cam, layers in frames]
    assert all(_bits(x, y) for x, y in zip(want, got))
    small = T._abc("5x3", 95)
    want = _plain_sequence(renderer, small)
    renderer.reset_denoise_history()
    assert all(_bits(x, y) for x, y in zip(want, [dev_motion(renderer, layers, cam, np.zeros((3, 5), np.uint32), table) for cam, layers in small]))


@gpu
def test_the_switch_changes_nothing_until_an_instance_moves():
    frames = T._abc("37x29", 92)
    r = F.Renderer(0)
    try:
        r.load_scene(scenes.cornell_box_instanced())
        r.build_ias()
        assert r.denoise_motion() is False
        want = _plain_sequence(r, frames)
        r.set_denoise_motion(True)
        assert r.denoise_motion() is True
        assert all(_bits(x, y) for x, y in zip(want, _plain_sequence(r, frames)))  # on, the transforms never changed
        r.set_transforms(*scenes.instanced_transforms((0.0, 0.0, 0.0)))           # the bits they have: still nothing moved
        assert all(_bits(x, y) for x, y in zip(want, _plain_sequence(r, frames)))
        # off after fh_set_transforms: today's call
        r.set_denoise_motion(False)
        r.reset_denoise_history()
        outs = [dev_plain(r, frames[0][1], frames[0][0])]
        r.set_transforms(*scenes.instanced_transforms((-0.19, 0.0, 0.0)))
        r.build_ias()
        outs += [dev_plain(r, layers, cam) for cam, layers in frames[1:]]
        assert all(_bits(x, y) for x, y in zip(want, outs))
        # on again: no snapshot was kept while it was off, so the next call is the plain one and only the one after could see a move
        r.set_denoise_motion(True)
        assert all(_bits(x, y) for x, y in zip(want, _plain_sequence(r, frames)))
        # a new scene drops the snapshot
        r.load_scene(scenes.cornell_box_instanced())
        r.build_ias()
        r.reset_denoise_history()
        outs = [dev_plain(r, frames[0][1], frames[0][0])]
        r.load_scene(scenes.cornell_box_instanced())
        r.set_transforms(*scenes.instanced_transforms((-0.19, 0.0, 0.0)))
        r.build_ias()
        outs += [dev_plain(r, layers, cam) for cam, layers in frames[1:]]
        assert all(_bits(x, y) for x, y in zip(want, outs))
    finally:
        r.close()


# ------------------------------------------------------------------ 6: end to end
E2E = dict(w=64, h=48, spp=4, depth=3, offset=(-0.19, 0.0, 0.0))  # 48 / (2 t) = 16 pixels per unit at the block's depth (t = 1 + 0.5): 0.19 is about 3 pixels


def _render_two_frames(r):
    """frame 1 with the block at home (seed 1), frame 2 with it moved (seed 2): the layers of both on the host"""
    q = E2E
    w, h = q["w"], q["h"]
    cam = F.Camera(**scenes.CORNELL_CAMERA)
    r.set_resolution(w, h)
    r.set_adaptive_sampling(0.0)
    L = F.RenderLayer(r, w, h)
    frames = []
    for k, off in enumerate(((0.0, 0.0, 0.0), q["offset"])):
        r.set_transforms(*scenes.instanced_transforms(off))
        r.build_ias()
        L.clear()
        r.init_render_states()
        r.seed = 1 + k
        r.render(cam, (0.0, 0.0, 0.0), L, q["spp"], q["depth"])
        r.wait_for_completion()
        layers = {n: L.download(n) for n in ("beauty", "normal", "albedo", "position", "depth")}
        layers["moments"], layers["counts"] = r.luminance_moments(), r.sample_counts()
        frames.append(layers)
    L.free()
    return cam, frames


def _implicit(r, cam, frames):
    r.set_denoise_motion(True)
    r.reset_denoise_history()
    outs = []
    for layers, off in zip(frames, ((0.0, 0.0, 0.0), E2E["offset"])):
        r.set_transforms(*scenes.instanced_transforms(off))
        r.build_ias()
        outs.append(dev_plain(r, layers, cam))
    r.set_denoise_motion(False)
    return outs


@gpu
def test_the_context_feeds_itself_what_the_explicit_call_is_fed():
    q = E2E
    w, h = q["w"], q["h"]
    r = F.Renderer(0)
    g = None
    try:
        r.load_scene(scenes.cornell_box_instanced())
        r.build_ias()
        cam, frames = _render_two_frames(r)
        implicit = _implicit(r, cam, frames)
        # the explicit call: the BVH stands at the moved pose, as when frame 2 was rendered
        r.reset_denoise_history()
        first = dev_plain(r, frames[0], cam)
        ids_buf = DeviceBuffer(r, 4 * w * h)
        r.primary_instances(cam, w, h, ids_buf.ptr)
        r.wait_for_completion()
        ids = ids_buf.download(np.uint32, (h, w))
        ids_buf.free()
        table = N.motion_from_transforms(*scenes.instanced_transforms((0.0, 0.0, 0.0)), *scenes.instanced_transforms(q["offset"]))
        assert [m.moved for m in table] == [0, 1]
        explicit = dev_motion(r, frames[1], cam, ids, table)
        assert _bits(first, implicit[0]) and _bits(explicit, implicit[1])
        box = ids == 1
        assert box.sum() > 100 and (ids == 0).sum() > 1000
        r.reset_denoise_history()
        plain = [dev_plain(r, layers, cam) for layers in frames]
        assert _bits(plain[0], implicit[0])
        inner = ~_grow(~box, 1)
        assert inner.sum() > 50 and (plain[1][inner] != implicit[1][inner]).any(axis=1).mean() > 0.5  # (the block's pixels now have a history)
        g = F.Renderer(devices=[0, 0])
        g.load_scene(scenes.cornell_box_instanced())
        g.build_ias()
        assert all(_bits(x, y) for x, y in zip(implicit, _implicit(g, cam, frames)))
        assert g.denoise_history_info() == (w, h, 2)
    finally:
        if g is not None:
            g.close()
        r.close()


# ------------------------------------------------------------------ 7: refusals
@gpu
def test_refused_motion_calls_leave_output_and_history_alone(renderer):
    calls, _, _ = motion_case("37x29", "rotate", True, seed=61)
    (cam1, first, _, _), (cam2, second, ids2, table) = calls
    renderer.reset_denoise_history()
    want = [dev_plain(renderer, first, cam1), dev_motion(renderer, second, cam2, ids2, table)]
    renderer.reset_denoise_history()
    outs = []
    L, ctx = N.lib(), renderer._ctx
    for k, (cam, layers) in enumerate(((cam1, first), (cam2, second))):
        d = Dev(renderer, layers)
        out, idb = DeviceBuffer(renderer, d.w * d.h * 16), DeviceBuffer(renderer, ids2.nbytes)
        out.clear(0x5A)
        idb.upload(ids2)
        try:
            ptrs = [d.bufs[n].ptr for n in NAMES]

            def call(ptrs=ptrs, camera=cam.as_c(), temporal=(0.2, 32.0, 0.9, 0.02), params=(2.0, 1.0, 0.2, 7, 5), w=d.w, h=d.h, dst=out.ptr, ids=idb.ptr, n=2, motion=table):
                i = N.DenoiseInputsC(*ptrs)
                return L.fh_denoise_temporal_motion(ctx, w, h, C.byref(i), None if camera is None else C.byref(camera), C.byref(N.TemporalParamsC(*temporal)),
                                                    C.byref(N.DenoiseParamsC(*params)), ids, n, motion, dst, 0)
            bad = [dict(motion=None), dict(ids=None), dict(n=0), dict(motion=_bad_table("point", float("nan"))), dict(motion=_bad_table("normal", float("inf"))),
                   dict(motion=_bad_table("point", float("-inf"))), dict(camera=None), dict(ptrs=ptrs[:3] + [None, None] + ptrs[5:]), dict(ptrs=ptrs[:6] + [None]),
                   dict(temporal=(0.2, 32.0, 0.9, 0.0)), dict(params=(2.0, 1.0, 0.2, 7, 7)), dict(w=0), dict(dst=None)]
            for kw in bad:
                assert call(**kw) == -1, kw
                assert b"fh_denoise_temporal_motion" in L.fh_last_error(ctx)
            renderer.wait_for_completion()
            assert (out.download(np.uint8) == 0x5A).all()
            assert renderer.denoise_history_info() == ((37, 29, k) if k else (0, 0, 0))
            outs.append(dev_plain(renderer, layers, cam) if k == 0 else dev_motion(renderer, layers, cam, ids2, table))
        finally:
            out.free()
            idb.free()
            d.free()
    assert all(_bits(x, y) for x, y in zip(want, outs))


@gpu
def test_the_switch_refuses_a_moved_scene_without_a_built_tree():
    frames = T._abc("37x29", 93)
    r = F.Renderer(0)
    try:
        r.load_scene(scenes.cornell_box_instanced())
        r.build_ias()
        r.set_denoise_motion(True)
        want = dev_plain(r, frames[0][1], frames[0][0])
        r.set_transforms(*scenes.instanced_transforms((-0.19, 0.0, 0.0)))  # (and no build)
        with pytest.raises(N.FredholmError, match="BVH"):
            dev_plain(r, frames[1][1], frames[1][0])
        assert r.denoise_history_info() == (37, 29, 1)
        r.set_transforms(*scenes.instanced_transforms((0.0, 0.0, 0.0)))
        r.build_ias()
        r.reset_denoise_history()
        assert _bits(want, dev_plain(r, frames[0][1], frames[0][0]))
    finally:
        r.close()


# ------------------------------------------------------------------ 8: quality
MOTION_QUALITY = dict(w=96, h=72, depth=5, frames=8, spp=16, step=0.05, truth_spp=1024)
REPLAY_R_MOTION = 0.325  # tools/denoise_temporal_replay.py --motion: profiles/denoise_motion_replay.json


def motion_quality_offset(k):
    """the short block's translation in frame k: 0.05 per frame towards -x, centred on its place in cornell_box() (it stays clear of the walls and of the tall block)"""
    return (0.175 - MOTION_QUALITY["step"] * k, 0.0, 0.0)


@gpu
def test_quality_on_a_sequence_with_a_moving_box():
    """cornell_box_instanced() at 96 x 72, depth 5, 8 frames of 16 spp with seeds 1..8 under a still camera, the short block moving 0.05 per frame (1.2 pixels); truth
    1024 spp at the last pose; relMSE as the temporal suite defines it, last frame, with moments, over the pixels whose id is the block in the last frame.  The float64
    replay on checker-rendered frames (tools/denoise_temporal_replay.py --motion) gives relMSE 0.01482 for plain temporal accumulation -- WORSE than the guided filter
    alone, 0.01415: the block's top slides in its own plane, so the plain call passes both stops there and blends in what another point of the block looked like -- and
    0.00482 with motion: R = REPLAY_R_MOTION = 0.325.  The device, which renders other samples than the checker, must reach (R + 1) / 2 = 0.663 on those pixels, and
    over the whole frame must not be worse than the plain call (replay: 0.983 x).  Observed on the device: block 0.01482 -> 0.00482 (0.325 x), frame 0.02576 -> 0.02533 (0.983 x)."""
    q = MOTION_QUALITY
    w, h = q["w"], q["h"]
    cam = F.Camera(**scenes.CORNELL_CAMERA)
    r = F.Renderer(0)
    try:
        r.load_scene(scenes.cornell_box_instanced())
        r.build_ias()
        r.set_resolution(w, h)
        L = F.RenderLayer(r, w, h)
        moments, counts, out, idb = DeviceBuffer(r, 8 * w * h), DeviceBuffer(r, 4 * w * h), DeviceBuffer(r, 16 * w * h), DeviceBuffer(r, 4 * w * h)
        p = L.ptrs
        r.set_adaptive_sampling(0.0)  # (threshold 0: the moments exist and nothing stops)
        r.set_denoise_motion(True)
        r.reset_denoise_history()
        frames = []
        for k in range(q["frames"]):
            r.set_transforms(*scenes.instanced_transforms(motion_quality_offset(k)))
            r.build_ias()
            L.clear()
            r.init_render_states()
            r.seed = 1 + k
            for _ in range(q["spp"]):
                r.render(cam, (0.0, 0.0, 0.0), L, 1, q["depth"])
            r.get_luminance_moments(moments.ptr)
            r.get_sample_counts(counts.ptr)
            r.denoise_temporal(w, h, p["beauty"], p["normal"], p["albedo"], out.ptr, p["position"], p["depth"], cam, moments.ptr, counts.ptr)
            r.wait_for_completion()
            layers = {n: L.download(n) for n in ("beauty", "normal", "albedo", "position", "depth")}
            layers["moments"], layers["counts"] = moments.download(np.float32, (h, w, 2)), counts.download(np.uint32, (h, w))
            frames.append(layers)
        motion = out.download(np.float32, (h, w, 4))
        r.primary_instances(cam, w, h, idb.ptr)
        r.wait_for_completion()
        box = idb.download(np.uint32, (h, w)) == 1
        r.set_denoise_motion(False)
        r.reset_denoise_history()
        for layers in frames:
            plain = dev_plain(r, layers, cam)
        L.clear()
        r.init_render_states()
        r.clear_adaptive_sampling()
        r.seed = 1000
        r.render(cam, (0.0, 0.0, 0.0), L, q["truth_spp"], q["depth"])
        r.wait_for_completion()
        truth = L.download("beauty")
        for b in (moments, counts, out, idb):
            b.free()
    finally:
        r.close()
    em, ep = _relmse(motion[box][None], truth[box][None]), _relmse(plain[box][None], truth[box][None])
    fm, fp = _relmse(motion, truth), _relmse(plain, truth)
    print(f"relMSE of frame 8 over the block's {int(box.sum())} pixels: plain temporal {ep:.5f}, motion {em:.5f} ({em / ep:.3f} x; replay R = {REPLAY_R_MOTION}); "
          f"whole frame: plain {fp:.5f}, motion {fm:.5f} ({fm / fp:.3f} x)")
    assert box.sum() > 200
    assert em <= (REPLAY_R_MOTION + 1.0) / 2.0 * ep, (em, ep)
    assert fm <= fp, (fm, fp)
