"""Tests of temporal accumulation (fh_denoise_temporal, fredholm_amd/csrc/denoise.hip: k_temporal<LOOK, kClipOff>) against a numpy restatement of the whole call as
include/fredholm_hip.h states it: the guided filter's preparation, the temporal stage, the passes.  The tests marked gpu need the device (-m gpu); two run on the CPU
alone: the reprojection formula against the checker's camera, and the with-history share of the moving-camera cases.

The restatement runs once in float64 and once in float32 (exp through the checker's fp32 routine, tanf from the C library the device library uses, sums in the header's
order), each with a history of its own.  As in test_gpu_denoise_guided.py the device may differ from the float64 result by at most 4 x the largest float32-versus-float64
difference of the same case, per value, relative to max(|value|, image mean).  Where the header promises bits -- the first call, alpha_min 1 and max_history 1 against
fh_denoise_guided, the still camera's running mean against the float32 restatement -- the comparison is bit for bit.
Observed on an MI355X: (device error) / (float32 error) = 1.000 in all 78 comparisons below -- every device value has the float32 restatement's bits, in every call of
every sequence -- with the float32 error between 2.0e-7 (5 x 3, one pass) and 6.8e-6 (the rendered 64 x 48 frame reprojected onto itself), so the bound the device
is held to is 8.0e-7 ... 2.7e-5.  With-history share of the moving-camera cases (asserted to lie in 20 % ... 95 %): 37 x 29: 92 % and 89 % in the second and third
call; 5 x 3: 79 % and 71 %.  The reprojection formula returns the pixel a checker-rendered position came from for 99.70 % (GUI camera) and 99.57 % (rotated and
translated camera) of the hit pixels of a 64 x 48 Cornell frame, in float32 and in float64 alike.

Quality (Cornell box, 96 x 72, depth 5, 8 frames of 16 spp with seeds 1..8, the camera moving 0.05 sideways per frame -- about one pixel of parallax on the nearest
wall --, truth 1024 spp at the last camera, relMSE as the guided suite defines it, last frame, with moments): the float64 replay on checker-rendered frames
(tools/denoise_temporal_replay.py) gives R = relMSE(temporal) / relMSE(guided alone) = REPLAY_R = 0.552; the device must reach (R + 1) / 2 = 0.776 and stay below the
unfiltered frame.  Observed on the device: unfiltered 0.07883, guided alone 0.02619, temporal 0.01445 (0.552 x).
"""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

import fredholm_amd as F
from fredholm_amd import native as N
from fredholm_amd import scenes
from fredholm_amd.renderer import DeviceBuffer

gpu = pytest.mark.gpu

LUM = (np.float32(0.2126729), np.float32(0.7151522), np.float32(0.0721750))
KERN = (3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
TDEF = dict(alpha_min=0.2, max_history=32.0, normal_cos_min=0.5, plane_tol=0.02)  # the library's defaults
REPLAY_R = 0.552  # tools/denoise_temporal_replay.py: moving_16spp, see DESIGN.md 4a


# ------------------------------------------------------------------ the restatement
def _shift(a, dx, dy):
    h, w = a.shape[:2]
    return a[np.clip(np.arange(h) + dy, 0, h - 1)][:, np.clip(np.arange(w) + dx, 0, w - 1)]


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _lum(c, dt):
    return c[..., 0] * dt(LUM[0]) + c[..., 1] * dt(LUM[1]) + c[..., 2] * dt(LUM[2])


def _wn(Nn, Nq, dt, power):
    wn = np.maximum(dt(0), Nn[..., 0] * Nq[..., 0] + Nn[..., 1] * Nq[..., 1] + Nn[..., 2] * Nq[..., 2])
    for _ in range(power):
        wn = wn * wn
    return wn


def prepare(dt, beauty, normal, albedo, moments, counts, normal_power_log2):
    """(c, v, a') of the guided filter's preparation"""
    b32 = beauty[..., :3]
    b32 = np.where(np.isnan(b32) | (np.abs(b32) > np.float32(3.0e38)), np.float32(0), b32)
    Bm, Nn, A = b32.astype(dt), normal[..., :3].astype(dt), albedo[..., :3].astype(dt)
    af = np.maximum(A, dt(np.float32(0.01)))
    c = Bm / af
    l = _lum(c, dt)
    if moments is not None:
        m1, m2, n = moments[..., 0].astype(dt), moments[..., 1].astype(dt), counts
        r = l / np.maximum(m1, dt(np.float32(1e-3)))
        v = np.where(n >= 2, np.maximum(m2 - m1 * m1, dt(0)) / np.maximum(n.astype(np.int64) - 1, 1).astype(dt) * (r * r), l * l)
    else:
        s0, s1, s2 = (np.zeros(l.shape, dt) for _ in range(3))
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                wn, lq = _wn(Nn, _shift(Nn, dx, dy), dt, normal_power_log2), _shift(l, dx, dy)
                s0 = s0 + wn
                s1 = s1 + wn * lq
                s2 = s2 + wn * (lq * lq)
        S = np.maximum(s0, dt(np.float32(1e-6)))
        S1, S2 = s1 / S, s2 / S
        v = np.maximum(S2 - S1 * S1, dt(0))
    return c, v, af


def passes_of(dt, exp, c, v, af, normal, albedo, position, depth, sigma_l, sigma_z, sigma_a, normal_power_log2, passes, upscale):
    Nn, A, Pp, Z = normal[..., :3].astype(dt), albedo[..., :3].astype(dt), position[..., :3].astype(dt), depth.astype(dt)
    sl, sz, sa = dt(np.float32(sigma_l)), dt(np.float32(sigma_z)), dt(np.float32(sigma_a))
    for it in range(passes):
        s = 1 << it
        g = np.zeros(v.shape, dt)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                g = g + dt((0.5 if dx == 0 else 0.25) * (0.5 if dy == 0 else 0.25)) * _shift(v, dx, dy)
        sd = sl * np.sqrt(g) + dt(np.float32(1e-6))
        lp = _lum(c, dt)
        kz = sz * dt(np.float32(0.01)) * np.maximum(Z, dt(np.float32(1e-3))) * dt(s)
        sc, sw, sv = np.zeros(c.shape, dt), np.zeros(v.shape, dt), np.zeros(v.shape, dt)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                cq, vq = _shift(c, s * dx, s * dy), _shift(v, s * dx, s * dy)
                if dx == 0 and dy == 0:
                    wgt = np.full(v.shape, dt(9.0 / 64.0))
                else:
                    wn = _wn(Nn, _shift(Nn, s * dx, s * dy), dt, normal_power_log2)
                    d = _shift(Pp, s * dx, s * dy) - Pp
                    ez = np.abs(Nn[..., 0] * d[..., 0] + Nn[..., 1] * d[..., 1] + Nn[..., 2] * d[..., 2]) / (kz * np.sqrt(dt(dx * dx + dy * dy)) + dt(np.float32(1e-6)))
                    da = _shift(A, s * dx, s * dy) - A
                    ea = (da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1] + da[..., 2] * da[..., 2]) / (sa * sa)
                    el = np.abs(_lum(cq, dt) - lp) / sd
                    wgt = dt(KERN[abs(dx)] * KERN[abs(dy)]) * wn * exp(-((ez + ea) + el))
                sc = sc + wgt[..., None] * cq
                sw = sw + wgt
                sv = sv + wgt * wgt * vq
        c, v = sc / sw[..., None], sv / (sw * sw)
    out = np.concatenate([c * af, np.ones(v.shape + (1,), dt)], axis=2)
    return out.repeat(2, axis=0).repeat(2, axis=1) if upscale else out


_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.tanf.restype, _libm.tanf.argtypes = C.c_float, [C.c_float]


def inv_tan(fov):
    """cam_inv_tan as render.hip computes it: 1.0f / tanf(0.5f * fov), with the C library's tanf"""
    return np.float32(1) / np.float32(_libm.tanf(float(np.float32(0.5) * np.float32(fov))))


def world_to_camera(t12):
    """the header's cofactor formula: in double, rounded once to float"""
    t = np.asarray(t12, np.float32).astype(np.float64).reshape(3, 4)
    R, T = t[:, :3], t[:, 3]
    Cf = [[R[1, 1] * R[2, 2] - R[1, 2] * R[2, 1], R[0, 2] * R[2, 1] - R[0, 1] * R[2, 2], R[0, 1] * R[1, 2] - R[0, 2] * R[1, 1]],
          [R[1, 2] * R[2, 0] - R[1, 0] * R[2, 2], R[0, 0] * R[2, 2] - R[0, 2] * R[2, 0], R[0, 2] * R[1, 0] - R[0, 0] * R[1, 2]],
          [R[1, 0] * R[2, 1] - R[1, 1] * R[2, 0], R[0, 1] * R[2, 0] - R[0, 0] * R[2, 1], R[0, 0] * R[1, 1] - R[0, 1] * R[1, 0]]]
    det = (R[0, 0] * Cf[0][0] + R[0, 1] * Cf[1][0]) + R[0, 2] * Cf[2][0]
    out = np.zeros(12, np.float64)
    for i in range(3):
        m0, m1, m2 = Cf[i][0] / det, Cf[i][1] / det, Cf[i][2] / det
        out[4 * i:4 * i + 4] = m0, m1, m2, -((m0 * T[0] + m1 * T[1]) + m2 * T[2])
    return out.astype(np.float32)


def reproject(dt, P, m12, f, w, h):
    """(x, y, t) of the header: where the camera (m12, f) saw the world points P; pixel centres at + 0.5"""
    m, f, W, H = m12.astype(dt), dt(f), dt(w), dt(h)
    q = [((m[4 * i] * P[..., 0] + m[4 * i + 1] * P[..., 1]) + m[4 * i + 2] * P[..., 2]) + m[4 * i + 3] for i in range(3)]
    with np.errstate(all="ignore"):
        t = (f - q[2]) / f
        return (W + (H * q[0]) / t) * dt(0.5), (H - (H * q[1]) / t) * dt(0.5), t


def _hit(n):
    return (n[..., 0] != 0) | (n[..., 1] != 0) | (n[..., 2] != 0)


def stage(dt, hist, cam15, c, v, normal, position, depth, alpha_min, max_history, normal_cos_min, plane_tol):
    """the temporal stage: (c_acc, v_acc, h) and which pixels took the with-history branch"""
    Nn, Pp, Z = normal[..., :3].astype(dt), position[..., :3].astype(dt), depth.astype(dt)
    hh, ww = v.shape
    hit = _hit(Nn)
    lim = dt(np.float32(plane_tol)) * np.maximum(Z, dt(np.float32(1e-3)))
    cos_min = dt(np.float32(normal_cos_min))

    def valid(Nq, Pq):
        d = Pq - Pp
        return _hit(Nq) & (_dot3(Nn, Nq) >= cos_min) & (np.abs(_dot3(Nn, d)) <= lim)
    have = np.zeros(v.shape, bool)
    c_h, v_h, h_h = np.zeros(c.shape, dt), np.zeros(v.shape, dt), np.zeros(v.shape, dt)
    with np.errstate(all="ignore"):
        if hist is not None and np.array_equal(hist["cam"].view(np.uint32), cam15.view(np.uint32)):
            have = valid(hist["N"], hist["P"])
            c_h, v_h, h_h = hist["c"], hist["v"], hist["h"]
        elif hist is not None:
            x, y, t = reproject(dt, Pp, hist["m"], hist["f"], ww, hh)
            xs, ys = x - dt(0.5), y - dt(0.5)
            ix, iy = np.floor(xs), np.floor(ys)
            fx, fy = xs - ix, ys - iy
            S, sc, sv, sh = np.zeros(v.shape, dt), np.zeros(c.shape, dt), np.zeros(v.shape, dt), np.zeros(v.shape, dt)
            for j in (0, 1):
                for i in (0, 1):
                    tx, ty = ix + dt(i), iy + dt(j)
                    inside = (tx >= 0) & (tx <= dt(ww - 1)) & (ty >= 0) & (ty <= dt(hh - 1))
                    qx = np.where(inside, tx, 0).astype(np.int64)
                    qy = np.where(inside, ty, 0).astype(np.int64)
                    wgt = (fx if i else dt(1) - fx) * (fy if j else dt(1) - fy)
                    ok = (t > 0) & inside & valid(hist["N"][qy, qx], hist["P"][qy, qx])
                    S = S + np.where(ok, wgt, dt(0))
                    sc = sc + np.where(ok[..., None], wgt[..., None] * hist["c"][qy, qx], dt(0))
                    sv = sv + np.where(ok, wgt * hist["v"][qy, qx], dt(0))
                    sh = sh + np.where(ok, wgt * hist["h"][qy, qx], dt(0))
            have = (t > 0) & (S >= dt(np.float32(1e-3)))
            c_h, v_h, h_h = sc / S[..., None], sv / S, sh / S
        have = have & hit
        hn = np.minimum(h_h + dt(1), dt(np.float32(max_history)))
        a = np.maximum(dt(1) / hn, dt(np.float32(alpha_min)))
        b = dt(1) - a
        c_acc = np.where(have[..., None], b[..., None] * c_h + a[..., None] * c, c)
        v_acc = np.where(have, (b * b) * v_h + (a * a) * v, v)
    h_out = np.where(hit, np.where(have, hn, dt(1)), dt(0))
    return c_acc.astype(dt), v_acc.astype(dt), h_out.astype(dt), have


class Restatement:
    """fh_denoise_temporal with a history of its own, in the arithmetic `dt`"""

    def __init__(self, dt, exp):
        self.dt, self.exp, self.hist, self.frames, self.have = dt, exp, None, 0, None

    def reset(self):
        self.hist, self.frames = None, 0

    def call(self, layers, cam15, use_moments=True, upscale=False, temporal=None, sigma_l=2.0, sigma_z=1.0, sigma_a=0.2, normal_power_log2=7, passes=5, spatial_only=False):
        dt = self.dt
        tp = dict(TDEF, **(temporal or {}))
        cam15 = np.asarray(cam15, np.float32)
        with np.errstate(all="ignore"):
            c, v, af = prepare(dt, layers["beauty"], layers["normal"], layers["albedo"], layers["moments"] if use_moments else None, layers["counts"] if use_moments else None,
                               normal_power_log2)
            if not spatial_only:
                if self.hist is not None and self.hist["v"].shape != v.shape:
                    self.reset()
                self.c_in, self.v_in = c, v
                c, v, h, self.have = stage(dt, self.hist, cam15, c, v, layers["normal"], layers["position"], layers["depth"], **tp)
                self.hist = dict(c=c, v=v, h=h, P=layers["position"][..., :3].astype(dt), N=layers["normal"][..., :3].astype(dt), cam=cam15.copy(),
                                 m=world_to_camera(cam15[:12]), f=inv_tan(cam15[12]))
                self.frames += 1
            out = passes_of(dt, self.exp, c, v, af, layers["normal"], layers["albedo"], layers["position"], layers["depth"], sigma_l, sigma_z, sigma_a, normal_power_log2, passes,
                            upscale)
        assert out.dtype == dt
        return out


def restatements(oracle):
    return Restatement(np.float64, np.exp), Restatement(np.float32, lambda x: oracle.elementary("exp", x).reshape(x.shape))


# ------------------------------------------------------------------ device side
NAMES = ("beauty", "normal", "albedo", "position", "depth", "moments", "counts")


class Dev:
    """the layers of one frame in device memory of renderer `r`"""

    def __init__(self, r, layers):
        self.r, self.bufs = r, {}
        for k in NAMES:
            self.bufs[k] = DeviceBuffer(r, layers[k].nbytes)
            self.bufs[k].upload(layers[k])
        self.h, self.w = layers["beauty"].shape[:2]

    def _out(self, upscale):
        out = DeviceBuffer(self.r, (4 if upscale else 1) * self.w * self.h * 16)
        out.clear(0xFF)
        return out

    def _get(self, out, upscale):
        self.r.wait_for_completion()
        got = out.download(np.float32, ((2 if upscale else 1) * self.h, (2 if upscale else 1) * self.w, 4))
        out.free()
        return got

    def temporal(self, cam, use_moments=True, upscale=False, temporal=None, **params):
        p, out = self.bufs, self._out(upscale)
        self.r.denoise_temporal(self.w, self.h, p["beauty"].ptr, p["normal"].ptr, p["albedo"].ptr, out.ptr, p["position"].ptr, p["depth"].ptr, cam,
                                p["moments"].ptr if use_moments else None, p["counts"].ptr if use_moments else None, upscale=upscale, **dict(TDEF, **(temporal or {})), **params)
        return self._get(out, upscale)

    def guided(self, use_moments=True, upscale=False, **params):
        p, out = self.bufs, self._out(upscale)
        self.r.denoise_guided(self.w, self.h, p["beauty"].ptr, p["normal"].ptr, p["albedo"].ptr, out.ptr, p["position"].ptr, p["depth"].ptr,
                              p["moments"].ptr if use_moments else None, p["counts"].ptr if use_moments else None, upscale=upscale, **params)
        return self._get(out, upscale)

    def free(self):
        for b in self.bufs.values():
            b.free()


def _bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _compare(what, got, r64, r32):
    """the guided suite's bound; returns the share of values bit-identical to the float32 restatement"""
    assert got.shape == r64.shape and np.isfinite(got).all() and (got[..., 3] == 1).all()
    scale = np.maximum(np.abs(r64), np.abs(r64[..., :3]).mean())
    e32, edev = float((np.abs(r32 - r64) / scale).max()), float((np.abs(got - r64) / scale).max())
    same = float((got.view(np.uint32) == r32.view(np.uint32)).mean())
    print(f"temporal {what}: float32 error {e32:.3e}, device error {edev:.3e}, ratio {edev / e32:.3f}, values bit-identical to float32 {same:.4f}")
    assert e32 > 0 and edev <= 4.0 * e32, (what, e32, edev)
    return same


class Sequence:
    """the device and the two restatements fed the same calls"""

    def __init__(self, r, oracle):
        self.r, (self.r64, self.r32) = r, restatements(oracle)
        r.reset_denoise_history()

    def call(self, what, layers, cam, check=True, **kw):
        d = Dev(self.r, layers)
        try:
            got = d.temporal(cam, **kw)
        finally:
            d.free()
        o64, o32 = self.r64.call(layers, cam.params(), **kw), self.r32.call(layers, cam.params(), **kw)
        same = _compare(what, got, o64, o32) if check else None
        return got, o32, same


# ------------------------------------------------------------------ inputs
def _random_layers(w, h, seed):
    """the guided suite's layers: piecewise-smooth guides, noisy radiance with a NaN and an Inf, counts with 0 and 1, a missed pixel, an albedo below the floor"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    side = (xx + 0.5 * yy > 0.55 * w)
    nrm = np.zeros((h, w, 4), np.float32)
    nrm[..., :3] = np.where(side[..., None], np.float32([0.6, 0.0, 0.8]), np.float32([0.0, 0.28, 0.96])) + rng.normal(0, 0.02, (h, w, 3)).astype(np.float32)
    nrm[..., :3] /= np.linalg.norm(nrm[..., :3], axis=2, keepdims=True)
    nrm[0, 0] = 0.0
    alb = np.zeros((h, w, 4), np.float32)
    alb[..., :3] = np.where((yy > 0.4 * h)[..., None], np.float32([0.7, 0.3, 0.2]), np.float32([0.25, 0.6, 0.7])) + rng.uniform(0, 0.03, (h, w, 3)).astype(np.float32)
    alb[h - 1, w - 1, :3] = 0.0
    depth = (2.0 + 0.05 * xx + np.where(side, 0.8, 0.0) + rng.normal(0, 0.002, (h, w))).astype(np.float32)
    pos = np.zeros((h, w, 4), np.float32)
    pos[..., 0], pos[..., 1], pos[..., 2] = (xx - w / 2) * 0.03 * depth, (yy - h / 2) * 0.03 * depth, -depth
    return dict(normal=nrm, albedo=alb, position=pos, depth=depth, **_random_beauty(alb, rng, 0.3 + 0.02 * xx + np.where(side, 1.5, 0.0), bad=True))


def _random_beauty(alb, rng, level, bad=False):
    """independent noisy radiance over the albedo `alb`, with moments and counts that go with it"""
    h, w = alb.shape[:2]
    beauty = np.ones((h, w, 4), np.float32)
    beauty[..., :3] = np.asarray(level, np.float32)[..., None] * rng.gamma(2.0, 0.5, (h, w, 3)).astype(np.float32) * alb[..., :3]
    counts = rng.integers(2, 40, (h, w)).astype(np.uint32)
    y = beauty[..., 0] * LUM[0] + beauty[..., 1] * LUM[1] + beauty[..., 2] * LUM[2]
    rel = rng.uniform(0.2, 1.2, (h, w)).astype(np.float32)
    mom = np.stack([y, y * y * (1 + rel * rel)], axis=2).astype(np.float32)
    if bad:
        counts[0, w - 1], counts[h - 1, 0], counts[h // 2, w // 2] = 0, 1, 1
        beauty[h // 2, 1, 0] = np.nan
        beauty[1, w // 2, 1] = np.inf
    return dict(beauty=beauty, moments=mom, counts=counts)


def _new_beauty(layers, seed, level=1.0):
    rng = np.random.default_rng(seed)
    return dict(layers, **_random_beauty(layers["albedo"], rng, np.full(layers["depth"].shape, level, np.float32)))


NEAR, FAR, STEP_X = -3.0, -5.0, 0.35


def _two_planes(w, h, cam, seed, near_z=NEAR):
    """two planes z = near_z (where x < STEP_X) and z = FAR, normal (0, 0, 1), seen along the chief rays of `cam` (render.hip: camera_ray with the lens centre)"""
    t, f = np.asarray(cam.m_transform, np.float64), float(inv_tan(cam.m_fov))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    uvx, uvy = -(2.0 * (xx + 0.5) - w) / h, (2.0 * (yy + 0.5) - h) / h
    d = np.stack([-uvx, -uvy, np.full(uvx.shape, -f)], axis=2)
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    org = t[:, :3] @ np.array([0.0, 0.0, f]) + t[:, 3]
    dw = d @ t[:, :3].T
    s_near = (near_z - org[2]) / dw[..., 2]
    near = (org[0] + s_near * dw[..., 0]) < STEP_X
    s = np.where(near, s_near, (FAR - org[2]) / dw[..., 2])
    pos = np.zeros((h, w, 4), np.float32)
    pos[..., :3] = org + s[..., None] * dw
    pos[..., 2] = np.where(near, near_z, FAR)  # exactly on the planes
    nrm = np.zeros((h, w, 4), np.float32)
    nrm[..., 2] = 1.0
    nrm[h - 1, 0] = 0.0  # a miss
    pos[h - 1, 0] = 0.0
    rng = np.random.default_rng(seed)
    alb = np.zeros((h, w, 4), np.float32)
    alb[..., :3] = rng.uniform(0.2, 0.9, (h, w, 3)).astype(np.float32)
    layers = dict(normal=nrm, albedo=alb, position=pos, depth=s.astype(np.float32), **_random_beauty(alb, rng, np.where(near, 1.5, 0.6)))
    return layers, near & _hit(nrm)


def _cameras(w, h, pixels=1.4):
    """camera A and camera B = A moved sideways by `pixels` of parallax on the near plane: x = (W + H * Q.x / t) / 2 moves by H / (2 t) per unit, t = (f - NEAR) / f"""
    a = F.Camera(origin=(0.1, -0.2, 0.5), fov=0.5 * np.pi, F=8.0, focus=100.0)
    f = float(inv_tan(a.m_fov))
    t = (f - (NEAR - 0.5)) / f
    b = F.Camera(origin=(0.1 + pixels * 2.0 * t / h, -0.2, 0.5), fov=0.5 * np.pi, F=8.0, focus=100.0)
    return a, b


SIZES = {"37x29": (37, 29), "5x3": (5, 3)}


# ------------------------------------------------------------------ 3 (CPU part): the reprojection formula against the checker's camera
def _own_pixel_share(oracle, cam, w=64, h=48):
    ref = oracle.Scene(scenes.cornell_box())
    lo = ref.render(cam.params(), w, h, ref.new_layers(w, h), 1, 1, n_threads=4)
    hit = _hit(lo["normal"])
    shares = []
    for dt in (np.float32, np.float64):
        x, y, t = reproject(dt, lo["position"][..., :3].astype(dt), world_to_camera(cam.params()[:12]), inv_tan(cam.m_fov), w, h)
        yy, xx = np.mgrid[0:h, 0:w]
        own = (np.floor(x) == xx) & (np.floor(y) == yy) & (t > 0)
        shares.append(float(own[hit].mean()))
    return shares, int(hit.sum())


def test_reprojection_formula_lands_on_the_pixel_of_the_checker(oracle):
    """no GPU: the header's formula inverts the checker's camera (1 spp: the position layer is the hit of the pixel's one jittered ray, F-number 1e4: nearly a pinhole)"""
    for cam in (F.Camera(**dict(scenes.CORNELL_CAMERA, F=1e4)), F.Camera(origin=(0.25, 1.2, 0.9), fov=0.4 * np.pi, F=1e4, focus=10000.0, forward=(-0.3, -0.15, -1.0))):
        shares, n = _own_pixel_share(oracle, cam)
        print(f"reprojection: {n} hit pixels, own pixel for {shares[0]:.4f} (float32) and {shares[1]:.4f} (float64)")
        assert n > 0.5 * 64 * 48 and min(shares) >= 0.99, shares


# ------------------------------------------------------------------ 1: the first call is fh_denoise_guided
@gpu
@pytest.mark.parametrize("use_moments,upscale", [(True, False), (False, False), (True, True)])
def test_first_call_equals_the_guided_filter(renderer, use_moments, upscale):
    cam = F.Camera(origin=(0.0, 0.0, 1.0))
    devs = {k: Dev(renderer, _random_layers(*wh, seed)) for (k, wh), seed in zip(SIZES.items(), (5, 6))}
    try:
        renderer.reset_denoise_history()
        assert renderer.denoise_history_info() == (0, 0, 0)
        want = {k: d.guided(use_moments, upscale) for k, d in devs.items()}
        assert _bits(devs["37x29"].temporal(cam, use_moments, upscale), want["37x29"])
        assert renderer.denoise_history_info() == (37, 29, 1)
        assert _bits(devs["5x3"].temporal(cam, use_moments, upscale), want["5x3"])  # a change of width x height drops the history
        assert renderer.denoise_history_info() == (5, 3, 1)
        assert not _bits(devs["5x3"].temporal(cam, use_moments, upscale, temporal=dict(normal_cos_min=0.5, plane_tol=0.5)), want["5x3"])  # (now there is one)
        assert renderer.denoise_history_info() == (5, 3, 2)
        renderer.reset_denoise_history()
        assert renderer.denoise_history_info() == (0, 0, 0)
        assert _bits(devs["5x3"].temporal(cam, use_moments, upscale), want["5x3"])
        assert _bits(devs["37x29"].temporal(cam, use_moments, upscale), want["37x29"])
    finally:
        for d in devs.values():
            d.free()


@gpu
@pytest.mark.parametrize("moments", [False, True])
def test_history_life_cycle_on_a_fresh_context(moments):
    """What becomes of the history from call to call, on a context that has never denoised: a larger frame makes the buffers grow (with fh_set_denoise_temporal_moments
    on from the start, the moment image and the main buffers in one call), a frame of the same pixel count and other dimensions fits the buffers and still starts a new
    history.  A call that starts a history gives fh_denoise_guided's bits (with sample moments also while the temporal moments are on); one that uses its history does not."""
    r = F.Renderer(0)
    devs = {}
    try:
        if moments:
            r.set_denoise_temporal_moments()
        cam = F.Camera(origin=(0.0, 0.0, 1.0))
        devs = {wh: Dev(r, _random_layers(*wh, seed)) for wh, seed in (((5, 3), 6), ((8, 5), 7), ((5, 8), 8))}
        want = {wh: d.guided() for wh, d in devs.items()}
        assert r.denoise_history_info() == (0, 0, 0)

        def call(wh, starts, frames):
            got = devs[wh].temporal(cam)
            assert _bits(got, want[wh]) == starts, (wh, frames)
            assert r.denoise_history_info() == wh + (frames,)

        call((5, 3), True, 1)
        call((5, 3), False, 2)
        call((8, 5), True, 1)   # a: the buffers grow
        call((8, 5), False, 2)  # b: ... and hold a history after it
        call((5, 8), True, 1)   # the same 40 pixels: no grow, another size
        call((5, 8), False, 2)
        call((5, 3), True, 1)   # a smaller frame within the buffers
        call((5, 3), False, 2)
    finally:
        for d in devs.values():
            d.free()
        r.close()


# ------------------------------------------------------------------ 2: a still camera accumulates a running mean
@gpu
def test_still_camera_keeps_a_running_mean(renderer, oracle):
    base = _random_layers(37, 29, 5)
    cam = F.Camera(origin=(0.0, 0.0, 1.0))
    seq = Sequence(renderer, oracle)
    tp = dict(alpha_min=0.0, max_history=64.0, normal_cos_min=0.9, plane_tol=0.02)
    hit = _hit(base["normal"])
    mean32, cs = None, []
    for k in range(1, 5):
        layers = base if k == 1 else _new_beauty(base, 100 + k)
        got, o32, same = seq.call(f"still frame {k}", layers, cam, temporal=tp, passes=1)
        assert _bits(got, o32), same  # the whole call, bit for bit
        assert renderer.denoise_history_info() == (37, 29, k) and seq.r32.frames == k
        c = seq.r32.c_in
        cs.append(c.astype(np.float64))
        a = np.float32(1) / np.float32(k)
        mean32 = c if k == 1 else (np.float32(1) - a) * mean32 + a * c  # the running mean, written out independently of stage()
        assert _bits(np.where(hit[..., None], seq.r32.hist["c"], 0), np.where(hit[..., None], mean32, 0))
        assert (seq.r32.hist["h"][hit] == k).all() and (seq.r32.hist["h"][~hit] == 0).all() and (seq.r32.have[hit].all() if k > 1 else True)
        m64 = np.mean(cs, axis=0)
        assert np.abs(seq.r32.hist["c"] - m64)[hit].max() <= 8 * k * np.finfo(np.float32).eps * np.abs(m64[hit]).max()
        assert _bits(seq.r32.hist["c"][~hit], c[~hit])  # a miss passes through


# ------------------------------------------------------------------ 3 (device part): real layers through the reprojecting kernel
@gpu
def test_reprojection_of_a_rendered_frame_onto_itself():
    """the frame of the CPU test rendered on the device, accumulated twice; the second camera differs in its F-number alone, so the kernel reprojects and must find
    every pixel's history around the pixel itself"""
    from oracle import pyoracle
    w, h = 64, 48
    r = F.Renderer(0)
    try:
        r.load_scene(scenes.cornell_box())
        r.build_ias()
        r.set_resolution(w, h)
        r.set_adaptive_sampling(0.0)
        cam = F.Camera(origin=(0.25, 1.2, 0.9), fov=0.4 * np.pi, F=1e4, focus=10000.0, forward=(-0.3, -0.15, -1.0))
        L = F.RenderLayer(r, w, h)
        r.render(cam, (0.0, 0.0, 0.0), L, 1, 3)
        r.wait_for_completion()
        layers = {k: L.download(k) for k in ("beauty", "normal", "albedo", "position", "depth")}
        layers["moments"], layers["counts"] = r.luminance_moments(), r.sample_counts()
        cam2 = F.Camera(origin=(0.25, 1.2, 0.9), fov=0.4 * np.pi, F=2e4, focus=10000.0, forward=(-0.3, -0.15, -1.0))
        seq = Sequence(r, pyoracle)
        tp = dict(alpha_min=0.0, max_history=8.0, normal_cos_min=0.9, plane_tol=0.05)
        seq.call("rendered frame, first", layers, cam, temporal=tp)
        seq.call("rendered frame, reprojected", layers, cam2, temporal=tp)
        hit = _hit(layers["normal"])
        assert seq.r32.have[hit].mean() >= 0.95, seq.r32.have[hit].mean()
    finally:
        r.close()


# ------------------------------------------------------------------ 4: a moving camera
# Parallax of B on the near plane, in pixels.  A shift of s pixels leaves floor(s) of the W columns without any tap inside the old frame, and the strip the step
# uncovers is s * (1 - 4.5 / 6.5) wide: at 37 x 29 the 1.4 pixels that do for 5 x 3 (3 of its 14 hit pixels lose their history) would leave 100 % of the hit pixels
# with a history, so that size moves by 4.7 (92 % and 89 % in the second and third call); neither puts the far plane's shift (x 4.5 / 6.5) near a whole pixel.
SHIFT = {"37x29": 4.7, "5x3": 1.4}


def _abc(size, seed=11):
    w, h = SIZES[size]
    a, b = _cameras(w, h, SHIFT[size])
    (la, _), (lb, _), (lc, _) = _two_planes(w, h, a, seed), _two_planes(w, h, b, seed + 1), _two_planes(w, h, a, seed + 2)
    return [(a, la), (b, lb), (a, lc)]


def test_moving_camera_cases_run_both_branches(oracle):
    """no GPU: the cases of the next test put between 20 % and 95 % of the hit pixels on the with-history branch, in the second and in the third call"""
    for size in SIZES:
        r32 = restatements(oracle)[1]
        for k, (cam, layers) in enumerate(_abc(size)):
            r32.call(layers, cam.params(), passes=1)
            if k:
                share = float(r32.have[_hit(layers["normal"])].mean())
                print(f"moving camera {size}, call {k + 1}: with history {share:.3f}")
                assert 0.20 <= share <= 0.95, (size, k, share)


@gpu
@pytest.mark.parametrize("passes", [1, 5])
@pytest.mark.parametrize("use_moments,upscale", [(True, False), (False, False), (True, True), (False, True)])
@pytest.mark.parametrize("size", list(SIZES))
def test_moving_camera_matches_the_restatement(renderer, oracle, size, use_moments, upscale, passes):
    seq = Sequence(renderer, oracle)
    for k, (cam, layers) in enumerate(_abc(size)):
        seq.call(f"moving {size} mom={use_moments} up={upscale} passes={passes} call {k + 1}", layers, cam, use_moments=use_moments, upscale=upscale, passes=passes)
        if k:
            assert 0.20 <= seq.r32.have[_hit(layers["normal"])].mean() <= 0.95


# ------------------------------------------------------------------ 5: every stop and every parameter reaches the kernel
@gpu
@pytest.mark.parametrize("moved", [False, True])
def test_stops_reach_the_kernel(renderer, oracle, moved):
    w, h = SIZES["37x29"]
    a, b = _cameras(w, h)
    first, _ = _two_planes(w, h, a, 21)
    second, _ = _two_planes(w, h, b if moved else a, 22)
    block = np.zeros((h, w), bool)
    block[8:20, 20:34] = True
    for what in ("normals", "positions"):
        damaged = {k: v.copy() for k, v in first.items()}
        if what == "normals":
            damaged["normal"][block] *= -1.0
        else:
            damaged["position"][block, 2] += 0.5  # off the plane: 0.02 * depth is at most 0.2
        shares = {}
        for name, lay in (("intact", first), ("damaged", damaged)):
            seq = Sequence(renderer, oracle)
            seq.call(f"stop {what} moved={moved} {name}, first", lay, a)
            seq.call(f"stop {what} moved={moved} {name}, second", second, b if moved else a)
            shares[name] = seq.r32.have.copy()
        x, y, _ = reproject(np.float64, second["position"][..., :3].astype(np.float64), world_to_camera(a.params()[:12]), inv_tan(a.m_fov), w, h)
        inner = (x - 0.5 >= 21) & (x - 0.5 < 32) & (y - 0.5 >= 9) & (y - 0.5 < 18) & _hit(second["normal"])  # all four taps (or the pixel itself) in the block
        assert inner.sum() >= 20 and shares["intact"][inner].mean() > 0.5 and not shares["damaged"][inner].any()
        assert np.array_equal(shares["intact"][~_grow(block, 2 if moved else 0)], shares["damaged"][~_grow(block, 2 if moved else 0)])


def _grow(mask, n):
    out = mask.copy()
    for dy in range(-n, n + 1):
        for dx in range(-n, n + 1):
            out |= _shift(mask, dx, dy)
    return out


@gpu
@pytest.mark.parametrize("temporal", [dict(alpha_min=1.0), dict(max_history=1.0)])
def test_alpha_min_one_and_max_history_one_give_the_guided_filter(renderer, oracle, temporal):
    """the blend weight of the new frame is 1: b = 0, c_acc = 0 * c_h + 1 * c, exactly c"""
    seq = Sequence(renderer, oracle)
    for k, (cam, layers) in enumerate(_abc("37x29", 31)):
        got, _, _ = seq.call(f"{temporal} call {k + 1}", layers, cam, temporal=temporal)
        d = Dev(renderer, layers)
        try:
            assert _bits(got, d.guided())
        finally:
            d.free()
        if k:
            assert seq.r32.have.any() and ("alpha_min" in temporal or (seq.r32.hist["h"][seq.r32.have] == 1).all())


# ------------------------------------------------------------------ 6: surrounding behaviour
def _run_sequence(r, frames, **kw):
    r.reset_denoise_history()
    outs = []
    for cam, layers in frames:
        d = Dev(r, layers)
        try:
            outs.append(d.temporal(cam, **kw))
        finally:
            d.free()
    return outs


@gpu
def test_repeated_sequences_and_a_group_give_the_same_bits(renderer):
    frames = _abc("37x29", 41) + [(_abc("37x29", 41)[0][0], _two_planes(37, 29, _cameras(37, 29)[0], 44)[0])]  # A, B, A, A: the last one on the still branch
    first = _run_sequence(renderer, frames)
    again = _run_sequence(renderer, frames)
    assert all(_bits(x, y) for x, y in zip(first, again))
    assert not _bits(first[1], _run_sequence(renderer, frames[1:2])[0])  # (the history does something)
    g = F.Renderer(devices=[0, 0])
    try:
        assert all(_bits(x, y) for x, y in zip(first, _run_sequence(g, frames)))
        assert g.denoise_history_info() == (37, 29, 4)
    finally:
        g.close()


@gpu
def test_the_other_denoisers_keep_their_bits_around_temporal_calls(renderer, oracle):
    frames = _abc("37x29", 51)
    d = Dev(renderer, frames[0][1])
    out = DeviceBuffer(renderer, d.w * d.h * 16)

    def atrous():
        renderer.denoise(d.w, d.h, d.bufs["beauty"].ptr, d.bufs["normal"].ptr, d.bufs["albedo"].ptr, out.ptr)
        renderer.wait_for_completion()
        return out.download(np.float32, (d.h, d.w, 4))
    try:
        before = atrous(), d.guided(True), d.guided(False, upscale=True)
        _run_sequence(renderer, frames)
        _run_sequence(renderer, frames, use_moments=False, upscale=True)
        after = atrous(), d.guided(True), d.guided(False, upscale=True)
        assert all(_bits(x, y) for x, y in zip(before, after))
        lay = frames[0][1]
        assert _bits(before[0], oracle.denoise(lay["beauty"], lay["normal"], lay["albedo"]))
    finally:
        out.free()
        d.free()


@gpu
def test_refused_calls_leave_output_and_history_alone(renderer):
    frames = _abc("37x29", 61)
    want = _run_sequence(renderer, frames)
    renderer.reset_denoise_history()
    outs = []
    L, ctx = N.lib(), renderer._ctx
    for k, (cam, layers) in enumerate(frames):
        d = Dev(renderer, layers)
        out = DeviceBuffer(renderer, d.w * d.h * 16)
        out.clear(0x5A)
        try:
            ptrs = [d.bufs[n].ptr for n in NAMES]

            def call(ptrs=ptrs, camera=cam.as_c(), temporal=(0.2, 32.0, 0.9, 0.02), params=(2.0, 1.0, 0.2, 7, 5), w=d.w, h=d.h, dst=out.ptr):
                i = N.DenoiseInputsC(*ptrs)
                return L.fh_denoise_temporal(ctx, w, h, C.byref(i), None if camera is None else C.byref(camera), C.byref(N.TemporalParamsC(*temporal)),
                                             C.byref(N.DenoiseParamsC(*params)), dst, 0)
            flat = cam.as_c()
            flat.transform[0] = flat.transform[1] = flat.transform[2] = 0.0
            bad = [dict(camera=None), dict(ptrs=ptrs[:3] + [None, None] + ptrs[5:]), dict(ptrs=ptrs[:3] + [None] + ptrs[4:]), dict(ptrs=ptrs[:6] + [None]), dict(camera=flat),
                   dict(temporal=(-0.5, 32.0, 0.9, 0.02)), dict(temporal=(0.2, 0.5, 0.9, 0.02)), dict(temporal=(0.2, 32.0, -1.0, 0.02)), dict(temporal=(0.2, 32.0, 0.9, 0.0)),
                   dict(temporal=(float("nan"), 32.0, 0.9, 0.02)), dict(params=(0.0, 1.0, 0.2, 7, 5)), dict(params=(2.0, 1.0, 0.2, 7, 7)), dict(w=0), dict(dst=None)]
            for kw in bad:
                assert call(**kw) == -1, kw
                assert b"fh_denoise_temporal" in L.fh_last_error(ctx)
            renderer.wait_for_completion()
            assert (out.download(np.uint8) == 0x5A).all()
            assert renderer.denoise_history_info() == ((37, 29, k) if k else (0, 0, 0))
            outs.append(d.temporal(cam))
        finally:
            out.free()
            d.free()
    assert all(_bits(x, y) for x, y in zip(want, outs))


# ------------------------------------------------------------------ 8: moved geometry gets no history, and leaves no ghost
@gpu
def test_moved_geometry_gets_no_history(renderer, oracle):
    """no motion vectors: the near plane moves along its normal by 10 x the plane tolerance between two calls of a still camera"""
    w, h = SIZES["37x29"]
    cam, _ = _cameras(w, h)
    first, near = _two_planes(w, h, cam, 71)
    move = 10.0 * 0.02 * float(first["depth"][near].max())
    second, near2 = _two_planes(w, h, cam, 72, near_z=NEAR + move)
    both = near & near2
    hitp = _hit(first["normal"])
    seq = Sequence(renderer, oracle)
    seq.call("moved geometry, first", first, cam, passes=1)
    got, _, _ = seq.call("moved geometry, second", second, cam, passes=1)
    st = seq.r32
    assert both.sum() > 100 and not st.have[both].any() and (st.hist["h"][both] == 1).all()
    assert _bits(st.hist["c"][both], st.c_in[both]) and _bits(st.hist["v"][both], st.v_in[both])
    far = hitp & ~near & ~near2
    assert far.sum() > 100 and st.have[far].all() and (st.hist["h"][far] == 2).all()
    d = Dev(renderer, second)
    try:
        spatial = d.guided(passes=1)
    finally:
        d.free()
    alone = ~_grow(~both, 2)  # every tap of the pass, and of its 3 x 3 variance prefilter, is a near-plane pixel: none of them has a history
    assert alone.sum() > 50 and _bits(got[alone], spatial[alone])
    inner_far = ~_grow(~far, 2)
    assert inner_far.sum() > 50 and (got[inner_far] != spatial[inner_far]).any(axis=1).mean() > 0.9


# ------------------------------------------------------------------ 7: quality
def _relmse(x, t):
    x, t = x[..., :3].astype(np.float64), t[..., :3].astype(np.float64)
    return float(np.mean((x - t) ** 2 / (t ** 2 + 1e-2)))


QUALITY = dict(w=96, h=72, depth=5, frames=8, spp=16, step=0.05, truth_spp=1024)


def quality_camera(k):
    o = scenes.CORNELL_CAMERA["origin"]
    return F.Camera(**dict(scenes.CORNELL_CAMERA, origin=(o[0] - 0.175 + QUALITY["step"] * k, o[1], o[2])))


@gpu
def test_quality_on_a_moving_cornell_sequence():
    q = QUALITY
    w, h = q["w"], q["h"]
    r = F.Renderer(0)
    try:
        r.load_scene(scenes.cornell_box())
        r.build_ias()
        r.set_resolution(w, h)
        L = F.RenderLayer(r, w, h)
        moments, counts, out = DeviceBuffer(r, 8 * w * h), DeviceBuffer(r, 4 * w * h), DeviceBuffer(r, 16 * w * h)
        p = L.ptrs
        r.reset_denoise_history()
        r.set_adaptive_sampling(0.0)  # (threshold 0: the moments exist and nothing stops)
        for k in range(q["frames"]):
            cam = quality_camera(k)
            L.clear()
            r.init_render_states()
            r.seed = 1 + k
            for _ in range(q["spp"]):
                r.render(cam, (0.0, 0.0, 0.0), L, 1, q["depth"])
            r.get_luminance_moments(moments.ptr)
            r.get_sample_counts(counts.ptr)
            r.denoise_temporal(w, h, p["beauty"], p["normal"], p["albedo"], out.ptr, p["position"], p["depth"], cam, moments.ptr, counts.ptr)
            r.wait_for_completion()
        temporal = out.download(np.float32, (h, w, 4))
        r.denoise_guided(w, h, p["beauty"], p["normal"], p["albedo"], out.ptr, p["position"], p["depth"], moments.ptr, counts.ptr)
        r.wait_for_completion()
        guided, unfiltered = out.download(np.float32, (h, w, 4)), L.download("beauty")
        L.clear()
        r.init_render_states()
        r.clear_adaptive_sampling()
        r.seed = 1000
        r.render(cam, (0.0, 0.0, 0.0), L, q["truth_spp"], q["depth"])
        r.wait_for_completion()
        truth = L.download("beauty")
        for b in (moments, counts, out):
            b.free()
    finally:
        r.close()
    et, eg, eu = _relmse(temporal, truth), _relmse(guided, truth), _relmse(unfiltered, truth)
    print(f"relMSE of frame 8: unfiltered {eu:.5f}, guided alone {eg:.5f}, temporal {et:.5f} ({et / eg:.3f} x guided; replay R = {REPLAY_R})")
    assert et <= (REPLAY_R + 1.0) / 2.0 * eg, (et, eg)
    assert et < eu, (et, eu)
