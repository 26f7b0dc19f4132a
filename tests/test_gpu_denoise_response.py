"""Tests of the clipped form of the temporal stage (include/fredholm_hip.h: fh_set_denoise_response; fredholm_amd/csrc/denoise.hip: k_temporal<., kClipColour>).  The
restatements of test_gpu_denoise_temporal.py and test_gpu_denoise_motion.py are extended by the header's six steps -- the 5 x 5 window of the current frame's colour,
the box, the clip, the shortened history -- in float64 and in float32, and the device is held to those suites' bound: 4 x the largest float32-versus-float64
difference of the same case.  Where the header promises bits the comparison is bit for bit.  The tests marked gpu need the device; that the look-up restated here is the
one of the two suites and that every case clips, keeps and isolates pixels are checked on the CPU; test_denoise_response_host.py holds the other CPU tests, the
hand-computed window among them.

Observed on an MI355X: (device error) / (float32 error) = 1.000 in all 96 comparisons of the restatement test -- every device value has the float32 restatement's
bits, in each of the three calls of each case -- with the float32 error between 2.6e-7 and 2.8e-6, so the bound the device is held to is 1.0e-6 ... 1.1e-5.
Quality: see test_quality_after_a_change_of_lighting.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import fredholm_amd as F
from fredholm_amd import native as N
from fredholm_amd import scenes
from fredholm_amd.renderer import DeviceBuffer

import test_gpu_denoise_motion as M
import test_gpu_denoise_temporal as T
from test_gpu_denoise_temporal import SIZES, TDEF, Dev, _bits, _compare, _dot3, _hit, _relmse, inv_tan

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the restatement
def lookup(dt, hist, cam15, normal, position, depth, ids, table, normal_cos_min, plane_tol):
    """(have, c_h, v_h, h_h, carried): the history of every pixel as the header's stage finds it -- the own tap, the 2 x 2 look-up, or (table given) the carried look-up"""
    Nn, Pp, Z = normal[..., :3].astype(dt), position[..., :3].astype(dt), depth.astype(dt)
    hh, ww = Z.shape
    hit = _hit(Nn)
    lim = dt(np.float32(plane_tol)) * np.maximum(Z, dt(np.float32(1e-3)))
    cos_min = dt(np.float32(normal_cos_min))
    carried = np.zeros(Z.shape, bool)
    Pb, Nb = Pp, Nn
    if table is not None:
        inside_table = ids < table[2].shape[0]
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
        S, sc, sv, sh = np.zeros(Z.shape, dt), np.zeros(Z.shape + (3,), dt), np.zeros(Z.shape, dt), np.zeros(Z.shape, dt)
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
    return have, c_h, v_h, h_h, carried & hit


def window_box(dt, c, normal, gamma, normal_cos_min):
    """steps 1 and 2 of the header: (n, lo, hi, gamma * sd) of every pixel's 5 x 5 window of the current frame's colour c; fmax with C semantics (a NaN operand loses)"""
    Nn = normal[..., :3].astype(dt)
    hh, ww = c.shape[:2]
    yy, xx = np.mgrid[0:hh, 0:ww]
    cos_min, g = dt(np.float32(normal_cos_min)), dt(np.float32(gamma))
    n, S1, S2 = np.zeros((hh, ww), dt), np.zeros(c.shape, dt), np.zeros(c.shape, dt)
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                inside = (xx + dx >= 0) & (xx + dx < ww) & (yy + dy >= 0) & (yy + dy < hh)
                cq, Nq = T._shift(c, dx, dy), T._shift(Nn, dx, dy)
                counts = inside & _hit(Nq) & (_dot3(Nn, Nq) >= cos_min) if (dx or dy) else np.ones((hh, ww), bool)
                n = n + np.where(counts, dt(1), dt(0))
                S1 = S1 + np.where(counts[..., None], cq, dt(0))
                S2 = S2 + np.where(counts[..., None], cq * cq, dt(0))
        mu = S1 / n[..., None]
        var = np.fmax(S2 / n[..., None] - mu * mu, dt(0))
        gsd = g * np.sqrt(var)
        return n, mu - gsd, mu + gsd, gsd


def clip_history(dt, c, normal, c_h, v_h, h_h, gamma, normal_cos_min):
    """steps 1 to 5: (cc, v_h', h_h', u, n)"""
    n, lo, hi, gsd = window_box(dt, c, normal, gamma, normal_cos_min)
    with np.errstate(all="ignore"):
        cc = np.fmin(np.fmax(c_h, lo), hi)
        uk = np.abs(cc - c_h) / (gsd + dt(np.float32(1e-6)))
        u = np.fmax(np.fmax(uk[..., 0], uk[..., 1]), uk[..., 2])
        few = n < 2
        cc, u = np.where(few[..., None], c_h, cc), np.where(few, dt(0), u)
        k1 = dt(1) + u
        return cc.astype(dt), (v_h * k1).astype(dt), (h_h / k1).astype(dt), u.astype(dt), n


def blend(dt, have, hit, c, v, c_h, v_h, h_h, alpha_min, max_history):
    with np.errstate(all="ignore"):
        hn = np.minimum(h_h + dt(1), dt(np.float32(max_history)))
        a = np.maximum(dt(1) / hn, dt(np.float32(alpha_min)))
        b = dt(1) - a
        c_acc = np.where(have[..., None], b[..., None] * c_h + a[..., None] * c, c)
        v_acc = np.where(have, (b * b) * v_h + (a * a) * v, v)
    h_out = np.where(hit, np.where(have, hn, dt(1)), dt(0))
    return c_acc.astype(dt), v_acc.astype(dt), h_out.astype(dt)


class ResponseRestatement(M.MotionRestatement):
    """the two restatements above it with the context's switch: gamma None is off (the parent's calls), else fh_set_denoise_response's clipped stage"""

    gamma = u = n = None

    def call_r(self, layers, cam15, ids=None, table=None, use_moments=True, upscale=False, temporal=None, sigma_l=2.0, sigma_z=1.0, sigma_a=0.2, normal_power_log2=7, passes=5):
        moved = table is not None and bool(table[2].any())
        if self.gamma is None or self.hist is None or self.hist["v"].shape != layers["depth"].shape:
            self.u = self.n = None
            if moved:
                return self.call_motion(layers, cam15, ids, table, use_moments, upscale, temporal, sigma_l, sigma_z, sigma_a, normal_power_log2, passes)
            return self.call(layers, cam15, use_moments, upscale, temporal, sigma_l, sigma_z, sigma_a, normal_power_log2, passes)
        dt, tp, cam15 = self.dt, dict(TDEF, **(temporal or {})), np.asarray(cam15, np.float32)
        with np.errstate(all="ignore"):
            c, v, af = T.prepare(dt, layers["beauty"], layers["normal"], layers["albedo"], layers["moments"] if use_moments else None, layers["counts"] if use_moments else None,
                                 normal_power_log2)
            self.c_in, self.v_in = c, v
            self.have, c_h, v_h, h_h, self.carried = lookup(dt, self.hist, cam15, layers["normal"], layers["position"], layers["depth"], ids, table if moved else None,
                                                            tp["normal_cos_min"], tp["plane_tol"])
            cc, v_h, h_h, self.u, self.n = clip_history(dt, c, layers["normal"], c_h, v_h, h_h, self.gamma, tp["normal_cos_min"])
            c, v, h = blend(dt, self.have, _hit(layers["normal"][..., :3]), c, v, cc, v_h, h_h, tp["alpha_min"], tp["max_history"])
            self.hist = dict(c=c, v=v, h=h, P=layers["position"][..., :3].astype(dt), N=layers["normal"][..., :3].astype(dt), cam=cam15.copy(), m=T.world_to_camera(cam15[:12]),
                             f=inv_tan(cam15[12]))
            self.frames += 1
            out = T.passes_of(dt, self.exp, c, v, af, layers["normal"], layers["albedo"], layers["position"], layers["depth"], sigma_l, sigma_z, sigma_a, normal_power_log2, passes, upscale)
        assert out.dtype == dt
        return out


def response_restatements(oracle, gamma):
    r64, r32 = ResponseRestatement(np.float64, np.exp), ResponseRestatement(np.float32, lambda x: oracle.elementary("exp", x).reshape(x.shape))
    r64.gamma = r32.gamma = gamma
    return r64, r32


# ------------------------------------------------------------------ the sequences with a change of lighting (tools/denoise_temporal_replay.py --response replays them)
RESPONSE_QUALITY = dict(w=96, h=72, depth=5, spp=16, frames_before=8, frames_after=4, truth_spp=1024)
LIGHT_FACES = (10, 11)  # of scenes.cornell_box(): the ceiling light's two triangles


def changed_scene(tag):
    """cornell_box() after the change: "L": the light's emission x 0.25; "S": the light quad moved + 0.5 in x"""
    sc = scenes.cornell_box()
    if tag == "L":
        em = sc["materials"]["emission_color"].copy()
        em[3] = em[3] * np.float32(0.25)
        sc["materials"]["emission_color"] = em
    else:
        v = sc["vertices"].copy()
        corners = np.asarray(sc["indices"])[list(LIGHT_FACES)].reshape(-1)
        assert (sc["material_ids"][list(LIGHT_FACES)] == 3).all()
        v[corners, 0] += np.float32(0.5)
        sc["vertices"] = v
    return sc


# ------------------------------------------------------------------ the cases of the restatement test
KINDS = ("still", "moved", "carried-still", "carried-moved")
GAMMA = 1.0
# the pixel of each call's frame that is left alone in its window: its 24 neighbours are made misses (so the layers have misses inside windows too)
ALONE = {"37x29": ((8, 6), (20, 14), (30, 22)), "5x3": ((0, 0), (0, 0), (4, 2))}


def _alone(layers, x, y):
    """`layers` with misses all around pixel (x, y): its window then holds the pixel alone (n = 1), and its neighbours' windows hold misses"""
    lay = {k: v.copy() for k, v in layers.items()}
    h, w = lay["depth"].shape
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if (dx or dy) and 0 <= x + dx < w and 0 <= y + dy < h:
                lay["normal"][y + dy, x + dx] = 0.0
                lay["position"][y + dy, x + dx] = 0.0
    return lay


def _relit(layers, seed, k):
    """new radiance over the layers' albedo, with the suite's bad pixels (a NaN, an Inf, counts of 0 and 1): frame k lights the left half of the frame differently"""
    h, w = layers["depth"].shape
    rng = np.random.default_rng(seed)
    level = np.where(np.arange(w)[None, :] < w // 2, (1.0, 0.3, 2.0)[k], 0.8) * np.ones((h, 1))
    return dict(layers, **T._random_beauty(layers["albedo"], rng, level.astype(np.float32), bad=True))


def response_case(size, kind, seed=301):
    """[(camera, layers, ids, table)] of three consecutive calls: a still camera; cameras A, B, A; the near plane an instance that turns a little further in every
    frame (the motion suite's "rotate"), under a still camera and under A, B, A"""
    w, h = SIZES[size]
    a, b = T._cameras(w, h, T.SHIFT[size])
    cams = (a, a, a) if kind in ("still", "carried-still") else (a, b, a)
    calls = []
    for k, cam in enumerate(cams):
        ids = table = None
        if kind.startswith("carried"):
            pivot = (-0.4, 0.0, T.NEAR)
            lay, ids, _ = M.planes_moved(w, h, cam, seed + k, *M.rot_y(0.12 * k, pivot))
            if k:
                prev, cur = M.affine(*M.rot_y(0.12 * (k - 1), pivot)), M.affine(*M.rot_y(0.12 * k, pivot))
                table = N.motion_from_transforms([M.IDENT, prev[0]], [M.IDENT, prev[1]], [M.IDENT, cur[0]], [M.IDENT, cur[1]])
        else:
            lay, _ = T._two_planes(w, h, cam, seed + k)
        lay = _alone(_relit(lay, seed + 10 + k, k), *ALONE[size][k])
        if ids is not None:
            ids = np.where(_hit(lay["normal"]), ids, M.MISS).astype(np.uint32)
        calls.append((cam, lay, ids, table))
    return calls


def case_counts(st):
    """(pixels with u > 0, with u = 0, with n < 2) among the pixels of the restatement's last call that have a history"""
    if st.u is None:
        return 0, 0, 0
    have = st.have
    return int((st.u[have] > 0).sum()), int(((st.u[have] == 0) & (st.n[have] >= 2)).sum()), int((st.n[have] < 2).sum())


def _restate(st, call, **kw):
    cam, lay, ids, table = call
    return st.call_r(lay, cam.params(), ids, None if table is None else M.table_arrays(table), **kw)


def test_cases_clip_keep_and_leave_alone(oracle):
    """no GPU: by the float32 restatement's own count every case of the restatement test has, over its second and third call, pixels with a history that are clipped
    (u > 0), that are not (u = 0, n >= 2) and whose window holds them alone (n < 2); and the carried cases carry"""
    for size in SIZES:
        for kind in KINDS:
            st = response_restatements(oracle, GAMMA)[1]
            total = np.zeros(3, int)
            for k, call in enumerate(response_case(size, kind)):
                _restate(st, call, passes=1)
                total += case_counts(st)
                if k and kind.startswith("carried"):
                    assert st.carried.any()
            print(f"response case {size} {kind}: u > 0: {total[0]}, u = 0: {total[1]}, n < 2: {total[2]}")
            assert (total > 0).all(), (size, kind, total)


def test_the_restated_look_up_is_the_one_of_the_two_suites(oracle):
    """no GPU: with the switch off the restatement is its parents'; and lookup() + blend() without the clip have the bits of T.stage and M.stage_motion"""
    for kind in KINDS:
        plain, mine = M.motion_restatements(oracle)[1], response_restatements(oracle, None)[1]
        for k, (cam, lay, ids, table) in enumerate(response_case("37x29", kind)):
            arrays = None if table is None else M.table_arrays(table)
            want = plain.call(lay, cam.params(), passes=1) if arrays is None else plain.call_motion(lay, cam.params(), ids, arrays, passes=1)
            if k:
                have, c_h, v_h, h_h, _ = lookup(np.float32, mine.hist, cam.params(), lay["normal"], lay["position"], lay["depth"], ids, arrays, TDEF["normal_cos_min"], TDEF["plane_tol"])
                c, v, _ = T.prepare(np.float32, lay["beauty"], lay["normal"], lay["albedo"], lay["moments"], lay["counts"], 7)
                c_acc, v_acc, h = blend(np.float32, have, _hit(lay["normal"]), c, v, c_h, v_h, h_h, TDEF["alpha_min"], TDEF["max_history"])
                assert np.array_equal(have, plain.have) and _bits(h, plain.hist["h"])
                assert _bits(np.nan_to_num(c_acc), np.nan_to_num(plain.hist["c"])) and _bits(np.nan_to_num(v_acc), np.nan_to_num(plain.hist["v"]))
            assert _bits(_restate(mine, (cam, lay, ids, table), passes=1), want)


# ------------------------------------------------------------------ device side
def dev_call(r, call, **kw):
    cam, lay, ids, table = call
    return T_dev_plain(r, lay, cam, **kw) if table is None else M.dev_motion(r, lay, cam, ids, table, **kw)


T_dev_plain = M.dev_plain


class switched:
    """the context's switch on (gamma) or off (None) for a block, and off again after it: the session's renderer is shared with the other suites"""

    def __init__(self, r, gamma):
        self.r, self.gamma = r, gamma

    def __enter__(self):
        if self.gamma is None:
            self.r.clear_denoise_response()
        else:
            self.r.set_denoise_response(self.gamma)
        return self.r

    def __exit__(self, *exc):
        self.r.clear_denoise_response()


def run_calls(r, calls, gamma, **kw):
    """the outputs of consecutive calls from an empty history, the switch at `gamma`"""
    with switched(r, gamma):
        r.reset_denoise_history()
        return [dev_call(r, c, **kw) for c in calls]


# ------------------------------------------------------------------ 1: the stage against the restatement
@gpu
@pytest.mark.parametrize("use_moments,upscale", [(True, False), (False, False), (True, True), (False, True)])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", list(SIZES))
def test_clipped_stage_matches_the_restatement(renderer, oracle, size, kind, use_moments, upscale):
    """three consecutive calls, so that a clipped history is itself looked up (and clipped) again.  The device must have the float32 restatement's bits and, as in
    the temporal and motion suites, lie within 4 x the float32 restatement's own distance from the float64 one (_compare).
    Observed on an MI355X: ratio 1.000 in all 96 comparisons (the module's docstring)."""
    r64, r32 = response_restatements(oracle, GAMMA)
    total = np.zeros(3, int)
    with switched(renderer, GAMMA):
        renderer.reset_denoise_history()
        for k, call in enumerate(response_case(size, kind)):
            got = dev_call(renderer, call, use_moments=use_moments, upscale=upscale)
            o64, o32 = _restate(r64, call, use_moments=use_moments, upscale=upscale), _restate(r32, call, use_moments=use_moments, upscale=upscale)
            total += case_counts(r32)
            same = _compare(f"response {size} {kind} mom={use_moments} up={upscale} call {k + 1}", got, o64, o32)
            assert _bits(got, o32), (k, same)
        assert renderer.denoise_history_info() == SIZES[size] + (3,)
    assert (total > 0).all(), total  # (u > 0, u = 0, n < 2: a case that clips nothing proves nothing)


@gpu
def test_windows_whose_squares_overflow(renderer, oracle):
    """step 6 of the header, pinned on two pixels of the second frame.  float32 only: in float64 nothing overflows.  With moments, whose variance of the two pixels is
    made 0 (m1 = 1e31: m2 - m1 * m1 = -inf, max 0): without them the 7 x 7 estimate of the preparation would hold inf - inf, where numpy's maximum and fmaxf part.
    (10, 10): c = 3e19 in red.  c * c is + infinity, so S2 of every window that counts the pixel is; mu = 3e19 / n with n >= 2 squares to at most 2.3e38, finite;
    var = sd = + infinity, the box is everything: the red channel of those windows' pixels is not clipped and their u comes from green and blue alone.
    (25, 20): c = 1e30 in green.  mu * mu overflows as well, inf - inf is NaN, fmax drops it: var = 0, the box is the point mu = 1e30 / n, u is about 1e34 and
    every pixel whose window counts the tap drops its history: h = 1, and (c_acc, v_acc) = (c, v) with their bits, all finite."""
    calls = response_case("37x29", "still", seed=311)[:2]
    lay = {k: v.copy() for k, v in calls[1][1].items()}
    for (x, y), ch, value in (((10, 10), 0, 3e19), ((25, 20), 1, 1e30)):
        lay["beauty"][y, x, ch] = np.float32(value) * max(lay["albedo"][y, x, ch], np.float32(0.01))
        lay["moments"][y, x] = (1e31, 1.0)
        lay["counts"][y, x] = 10
    calls[1] = (calls[1][0], lay, None, None)
    r32 = response_restatements(oracle, GAMMA)[1]
    want = [_restate(r32, c) for c in calls]
    c = r32.c_in
    with np.errstate(over="ignore"):
        assert c[10, 10, 0] > 1.9e19 and np.isinf(c[10, 10, 0] * c[10, 10, 0]) and c[20, 25, 1] > 0.9e30
    n, lo, hi, gsd = window_box(np.float32, c, lay["normal"], GAMMA, TDEF["normal_cos_min"])
    first = np.zeros((29, 37), bool)
    first[8:13, 8:13] = True
    first &= r32.have & (n >= 2)
    assert first.sum() >= 20 and np.isinf(gsd[first][:, 0]).all() and (lo[first][:, 0] == -np.inf).all() and (hi[first][:, 0] == np.inf).all()
    assert np.isfinite(gsd[first][:, 1:]).all() and (r32.u[first] > 0).any() and np.isfinite(r32.u[first]).all()
    second = np.zeros((29, 37), bool)
    second[18:23, 23:28] = True
    second &= r32.have & (n >= 2)
    assert second.sum() >= 20 and (gsd[second][:, 1] == 0).all() and (lo[second][:, 1] == hi[second][:, 1]).all() and (lo[second][:, 1] > 3e28).all()
    assert (r32.u[second] > 1e33).all() and np.isfinite(r32.u[second]).all() and (r32.hist["h"][second] == 1).all()
    assert _bits(r32.hist["c"][second], c[second]) and _bits(r32.hist["v"][second], r32.v_in[second])
    got = run_calls(renderer, calls, GAMMA)
    assert _bits(got[0], want[0]) and _bits(got[1], want[1])
    assert np.isfinite(got[1]).all()


# ------------------------------------------------------------------ 2: identities, bit for bit
@gpu
def test_set_then_cleared_is_the_plain_call(renderer):
    frames = [(cam, lay, None, None) for cam, lay in T._abc("37x29", 321)]
    want = run_calls(renderer, frames, None)
    renderer.set_denoise_response(0.75)
    assert renderer.get_denoise_response() == (True, 0.75)
    renderer.clear_denoise_response()
    assert renderer.get_denoise_response() == (False, 0.75)
    renderer.reset_denoise_history()
    got = [dev_call(renderer, c) for c in frames]
    assert all(_bits(x, y) for x, y in zip(want, got))
    assert not _bits(run_calls(renderer, frames, GAMMA)[1], want[1])  # (the switch does something)


@gpu
@pytest.mark.parametrize("use_moments,upscale", [(True, False), (False, True)])
def test_first_call_with_the_switch_on_is_the_guided_filter(renderer, use_moments, upscale):
    cam = F.Camera(origin=(0.0, 0.0, 1.0))
    devs = {k: Dev(renderer, T._random_layers(*wh, seed)) for (k, wh), seed in zip(SIZES.items(), (5, 6))}
    try:
        with switched(renderer, GAMMA):
            renderer.reset_denoise_history()
            want = {k: d.guided(use_moments, upscale) for k, d in devs.items()}
            assert _bits(devs["37x29"].temporal(cam, use_moments, upscale), want["37x29"])
            assert _bits(devs["5x3"].temporal(cam, use_moments, upscale), want["5x3"])  # a change of width x height drops the history
            assert not _bits(devs["5x3"].temporal(cam, use_moments, upscale, temporal=dict(normal_cos_min=0.5, plane_tol=0.5)), want["5x3"])  # (now there is one)
            renderer.reset_denoise_history()
            assert _bits(devs["5x3"].temporal(cam, use_moments, upscale), want["5x3"])
    finally:
        for d in devs.values():
            d.free()


@gpu
def test_a_huge_gamma_clips_nothing_and_gives_the_plain_call(renderer, oracle):
    """gamma = 1e6 on the noisy two-plane sequence: the box is a million standard deviations wide, the float32 restatement reports no pixel with u > 0 (asserted
    first), so cc = c_h, k1 = 1 and every pixel has the plain call's bits -- the still kernel's (A, A) and the moved kernel's (A, B, A) look-ups are the plain ones"""
    abc = T._abc("37x29", 331)
    frames = [(c, l, None, None) for c, l in abc] + [(abc[0][0], T._two_planes(37, 29, abc[0][0], 334)[0], None, None)]  # A, B, A, A: the last call on the still branch
    r32 = response_restatements(oracle, 1e6)[1]
    clipped = []
    for call in frames:
        _restate(r32, call, passes=1)
        if r32.u is not None:
            assert r32.have.any()
            clipped.append(int((r32.u[r32.have] > 0).sum()))
    assert clipped == [0, 0, 0], clipped
    want = run_calls(renderer, frames, None)
    got = run_calls(renderer, frames, 1e6)
    assert all(_bits(x, y) for x, y in zip(want, got))


@gpu
def test_identity_maps_under_a_moved_camera_give_the_switched_on_plain_call(renderer):
    """the motion form of the clipped kernel with every pixel carried by identity maps must equal its moved-camera form: both go through the same look-up"""
    frames = T._abc("37x29", 341)
    table = (N.MotionC * 1)()
    for k in range(12):
        table[0].point[k] = float(M.IDENT[k])
    for k in range(9):
        table[0].normal[k] = 1.0 if k % 4 == 0 else 0.0
    table[0].moved = 1
    ids = np.zeros((29, 37), np.uint32)
    want = run_calls(renderer, [(c, l, None, None) for c, l in frames], GAMMA)
    got = run_calls(renderer, [(c, l, ids, table) for c, l in frames], GAMMA)
    assert all(_bits(x, y) for x, y in zip(want, got))
    assert not _bits(want[1], run_calls(renderer, [(c, l, None, None) for c, l in frames], None)[1])


@gpu
def test_a_group_gives_the_plain_contexts_bits(renderer):
    calls = response_case("37x29", "moved", seed=351) + response_case("37x29", "still", seed=352)[2:]
    want = run_calls(renderer, calls, GAMMA)
    g = F.Renderer(devices=[0, 0])
    try:
        assert g.get_denoise_response() == (False, 1.0)
        assert all(_bits(x, y) for x, y in zip(want, run_calls(g, calls, GAMMA)))
        g.set_denoise_response(2.0)
        assert g.get_denoise_response() == (True, 2.0)
        with pytest.raises(N.FredholmError, match="gamma"):
            g.set_denoise_response(0.0)
        assert g.get_denoise_response() == (True, 2.0)
        assert g.denoise_history_info() == (37, 29, 4)
    finally:
        g.close()


@gpu
def test_other_calls_keep_their_bits_beside_a_switched_on_context(renderer, oracle):
    """fh_denoise, fh_denoise_guided and switch-off temporal calls on the session's context, interleaved with switch-on calls on a second context"""
    frames = [(cam, lay, None, None) for cam, lay in T._abc("37x29", 361)]
    d = Dev(renderer, frames[0][1])
    out = DeviceBuffer(renderer, d.w * d.h * 16)
    other = F.Renderer(0)

    def atrous():
        renderer.denoise(d.w, d.h, d.bufs["beauty"].ptr, d.bufs["normal"].ptr, d.bufs["albedo"].ptr, out.ptr)
        renderer.wait_for_completion()
        return out.download(np.float32, (d.h, d.w, 4))
    try:
        before = [atrous(), d.guided(True), d.guided(False, upscale=True)] + run_calls(renderer, frames, None)
        other.set_denoise_response(GAMMA)
        other.reset_denoise_history()
        renderer.reset_denoise_history()
        after = []
        for call in frames:
            switched_on = dev_call(other, call)
            after.append(dev_call(renderer, call))
        assert not _bits(switched_on, after[-1])
        after = [atrous(), d.guided(True), d.guided(False, upscale=True)] + after
        assert all(_bits(x, y) for x, y in zip(before, after))
        lay = frames[0][1]
        assert _bits(before[0], oracle.denoise(lay["beauty"], lay["normal"], lay["albedo"]))
    finally:
        other.close()
        out.free()
        d.free()


@gpu
def test_the_bookkeeping_path_runs_the_clipped_stage_too():
    """fh_set_denoise_motion and fh_set_denoise_response both on: fh_denoise_temporal, which then traces the id plane and builds the table itself, has the bits of the
    explicit fh_denoise_temporal_motion call under the same switch (the motion suite's two rendered frames, the block moved by 3 pixels between them)"""
    q = M.E2E
    w, h = q["w"], q["h"]
    r = F.Renderer(0)
    try:
        r.load_scene(scenes.cornell_box_instanced())
        r.build_ias()
        cam, frames = M._render_two_frames(r)
        plain = M._implicit(r, cam, frames)
        r.set_denoise_response(GAMMA)
        implicit = M._implicit(r, cam, frames)
        r.reset_denoise_history()  # the explicit call: the BVH stands at the moved pose, as when frame 2 was rendered
        first = M.dev_plain(r, frames[0], cam)
        ids_buf = DeviceBuffer(r, 4 * w * h)
        r.primary_instances(cam, w, h, ids_buf.ptr)
        r.wait_for_completion()
        ids = ids_buf.download(np.uint32, (h, w))
        ids_buf.free()
        table = N.motion_from_transforms(*scenes.instanced_transforms((0.0, 0.0, 0.0)), *scenes.instanced_transforms(q["offset"]))
        explicit = M.dev_motion(r, frames[1], cam, ids, table)
        assert r.get_denoise_response() == (True, GAMMA) and (ids == 1).sum() > 100
        assert _bits(first, implicit[0]) and _bits(explicit, implicit[1])
        assert _bits(plain[0], implicit[0]) and not _bits(plain[1], implicit[1])  # (the first call has no history to clip; the second is clipped)
    finally:
        r.close()


# ------------------------------------------------------------------ 3: refusals
@gpu
def test_a_bad_gamma_leaves_switch_history_and_output_alone(renderer):
    calls = response_case("37x29", "moved", seed=371)
    want = run_calls(renderer, calls, 1.5)
    L, ctx = N.lib(), renderer._ctx
    try:
        renderer.reset_denoise_history()
        renderer.set_denoise_response(1.5)
        outs = []
        for k, call in enumerate(calls):
            for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
                assert L.fh_set_denoise_response(ctx, C.byref(N.ResponseParamsC(bad))) == -1
                assert b"fh_set_denoise_response" in L.fh_last_error(ctx) and b"gamma" in L.fh_last_error(ctx)
                assert renderer.get_denoise_response() == (True, 1.5)
            assert renderer.denoise_history_info() == ((37, 29, k) if k else (0, 0, 0))
            outs.append(dev_call(renderer, call))
        assert all(_bits(x, y) for x, y in zip(want, outs))
        renderer.clear_denoise_response()
        assert L.fh_set_denoise_response(ctx, C.byref(N.ResponseParamsC(float("nan")))) == -1
        assert renderer.get_denoise_response() == (False, 1.5)
        on = C.c_int(7)
        assert L.fh_get_denoise_response(ctx, C.byref(on), None) == 0 and on.value == 0
    finally:
        renderer.clear_denoise_response()
        renderer.set_denoise_response(1.0)  # (the gamma a later get reports: back to the default)
        renderer.clear_denoise_response()


# ------------------------------------------------------------------ 4: quality on the device
def replay_record():
    with open(os.path.join(ROOT, "profiles", "denoise_response_replay.json")) as f:
        return json.loads(f.readline())


def replay_ratio(rec, tag, frame, gamma=GAMMA):
    """rho: relMSE(clipped) / relMSE(plain) of the float64 replay (tools/denoise_temporal_replay.py --response) for `frame` of sequence `tag`"""
    seq = rec["sequences"][tag]
    clipped = {f["frame"]: f["relmse"] for f in seq[f"gamma={gamma}"]}
    plain = {f["frame"]: f["relmse"] for f in seq["plain"]}
    return clipped[frame] / plain[frame]


def _render_frame(r, L, cam, seed, spp, depth, moments, counts):
    L.clear()
    r.init_render_states()
    r.seed = seed
    for _ in range(spp):
        r.render(cam, (0.0, 0.0, 0.0), L, 1, depth)
    r.get_luminance_moments(moments.ptr)
    r.get_sample_counts(counts.ptr)


def _truth(r, L, cam, spp, depth):
    L.clear()
    r.init_render_states()
    r.clear_adaptive_sampling()
    r.seed = 1000
    r.render(cam, (0.0, 0.0, 0.0), L, spp, depth)
    r.wait_for_completion()
    return L.download("beauty")


def device_sequence(plan, gamma, score_from, with_guided=False):
    """plan: [(scene or None, camera)] per frame -- a scene that is not None is loaded (load_scene + build_ias) before that frame is rendered; every frame is rendered
    with 16 one-sample calls and seed 1 + k and denoised at once by fh_denoise_temporal on the same context, the switch at `gamma`.  Returns the outputs of the
    frames from `score_from` on (1-based) and, with_guided, fh_denoise_guided's of the same layers."""
    q = RESPONSE_QUALITY
    w, h = q["w"], q["h"]
    r = F.Renderer(0)
    outs, guided = {}, {}
    try:
        L = moments = None
        for k, (scene, cam) in enumerate(plan):
            if scene is not None:
                r.load_scene(scene)
                r.build_ias()
                if L is None:
                    r.set_resolution(w, h)
                    L = F.RenderLayer(r, w, h)
                    moments, counts, out = DeviceBuffer(r, 8 * w * h), DeviceBuffer(r, 4 * w * h), DeviceBuffer(r, 16 * w * h)
                    if gamma is not None:
                        r.set_denoise_response(gamma)
                    r.reset_denoise_history()
            r.set_adaptive_sampling(0.0)  # (threshold 0: the moments exist and nothing stops)
            _render_frame(r, L, cam, 1 + k, q["spp"], q["depth"], moments, counts)
            p = L.ptrs
            r.denoise_temporal(w, h, p["beauty"], p["normal"], p["albedo"], out.ptr, p["position"], p["depth"], cam, moments.ptr, counts.ptr)
            r.wait_for_completion()
            if k + 1 >= score_from:
                outs[k + 1] = out.download(np.float32, (h, w, 4))
                if with_guided:
                    r.denoise_guided(w, h, p["beauty"], p["normal"], p["albedo"], out.ptr, p["position"], p["depth"], moments.ptr, counts.ptr)
                    r.wait_for_completion()
                    guided[k + 1] = out.download(np.float32, (h, w, 4))
        assert r.denoise_history_info() == (w, h, len(plan))
    finally:
        r.close()
    return outs, guided


def device_truth(scene, cam):
    q = RESPONSE_QUALITY
    r = F.Renderer(0)
    try:
        r.load_scene(scene)
        r.build_ias()
        r.set_resolution(q["w"], q["h"])
        return _truth(r, F.RenderLayer(r, q["w"], q["h"]), cam, q["truth_spp"], q["depth"])
    finally:
        r.close()


_TRUTH_A = []


def truth_before():
    if not _TRUTH_A:
        _TRUTH_A.append(device_truth(scenes.cornell_box(), F.Camera(**scenes.CORNELL_CAMERA)))
    return _TRUTH_A[0]


@gpu
@pytest.mark.parametrize("tag", ["L", "S"])
def test_quality_after_a_change_of_lighting(tag):
    """Cornell box, 96 x 72, depth 5, 16 spp per frame with seeds 1 + k, a still camera: 8 frames, then the light's emission x 0.25 (L) or the light quad moved by
    + 0.5 in x (S) by a new load_scene + build_ias, then 4 more; truths of 1024 spp with seed 1000.  First the condition: the PLAIN call lags -- its relMSE of frame 9
    is more than 10 x the guided filter's (replay: 90 x and 330 x), so a history that the upload dropped could not pass for responsiveness.  Then the clipped call at
    frames 9 and 12 is at most (rho + 1) / 2 x the plain call, rho the replay's ratio of that frame, and at frame 8 -- nothing has changed yet -- at most 1.05 x.
    Observed on the device (guided alone / plain temporal / clipped, frames 8, 9, 12), the replay's figures to the digits shown, since the device renders the checker's samples:
      (L) 0.02943 / 0.01510 / 0.01433 (0.949 x);  0.00651 / 0.58449 / 0.02774 (0.0475 x, asserted 0.524 x);  0.00655 / 0.15234 / 0.00820 (0.0538 x, asserted 0.527 x)
      (S) 0.02943 / 0.01510 / 0.01433 (0.949 x);  0.03113 / 10.38136 / 0.38772 (0.0373 x, asserted 0.519 x);  0.03393 / 2.73111 / 0.10950 (0.0401 x, asserted 0.520 x)
    The plain call's frame 9 is 90 x (L) and 333 x (S) the guided filter's."""
    q = RESPONSE_QUALITY
    cam = F.Camera(**scenes.CORNELL_CAMERA)
    nb, na = q["frames_before"], q["frames_after"]
    plan = [(scenes.cornell_box() if k == 0 else changed_scene(tag) if k == nb else None, cam) for k in range(nb + na)]
    plain, guided = device_sequence(plan, None, nb, with_guided=True)
    clipped, _ = device_sequence(plan, GAMMA, nb)
    truth = {k: truth_before() if k <= nb else None for k in plain}
    after = device_truth(changed_scene(tag), cam)
    rec = replay_record()
    err = {}
    for k in sorted(plain):
        t = truth[k] if truth[k] is not None else after
        err[k] = (_relmse(guided[k], t), _relmse(plain[k], t), _relmse(clipped[k], t))
        rho = replay_ratio(rec, tag, k)
        print(f"response quality ({tag}) frame {k}: guided {err[k][0]:.5f}, plain temporal {err[k][1]:.5f}, clipped {err[k][2]:.5f} ({err[k][2] / err[k][1]:.4f} x plain; replay rho {rho:.4f})")
    assert err[nb + 1][1] > 10.0 * err[nb + 1][0], err[nb + 1]
    for k in (nb + 1, nb + na):
        assert err[k][2] <= (replay_ratio(rec, tag, k) + 1.0) / 2.0 * err[k][1], (k, err[k])
    assert err[nb][2] <= 1.05 * err[nb][1], err[nb]


@gpu
def test_quality_of_the_steady_moving_camera_sequence_is_kept():
    """the temporal suite's QUALITY sequence (a moving camera, nothing else changes): the clipped call's last frame is at most 1.05 x the plain call's.
    Observed on the device: plain 0.01445, clipped 0.01364 (0.944 x; the replay's 0.944)."""
    q = T.QUALITY
    assert (q["w"], q["h"], q["spp"], q["depth"], q["truth_spp"]) == tuple(RESPONSE_QUALITY[k] for k in ("w", "h", "spp", "depth", "truth_spp"))
    plan = [(scenes.cornell_box() if k == 0 else None, T.quality_camera(k)) for k in range(q["frames"])]
    plain, _ = device_sequence(plan, None, q["frames"])
    clipped, _ = device_sequence(plan, GAMMA, q["frames"])
    truth = device_truth(scenes.cornell_box(), T.quality_camera(q["frames"] - 1))
    ep, ec = _relmse(plain[q["frames"]], truth), _relmse(clipped[q["frames"]], truth)
    print(f"response quality (M) frame {q['frames']}: plain temporal {ep:.5f}, clipped {ec:.5f} ({ec / ep:.4f} x; replay {replay_ratio(replay_record(), 'M', q['frames']):.4f})")
    assert ec <= 1.05 * ep, (ec, ep)
