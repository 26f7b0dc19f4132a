"""GPU tests (-m gpu) of the variance-guided denoiser (fh_denoise_guided, fredholm_amd/csrc/denoise.hip) against a numpy restatement of the filter as
include/fredholm_hip.h states it.

The restatement below runs once in float64 and once in float32 (exp through the checker's fp32 routine, taps in the header's order).  The device may differ from
the float64 result by at most 4 x the largest float32-versus-float64 difference of the same case, per value, relative to max(|value|, image mean): the tolerance is
measured per case, and the factor 4 covers the summation-order freedom of the 25 taps.  Observed on an MI355X: (device error) / (float32 error) = 1.000 in all
20 comparisons below -- the device's values are bit-identical to the float32 restatement in every one of them -- with the float32 error between 4.5e-7 (two passes,
wide stops) and 2.9e-6 (37 x 29 random layers without guides), so the bound the device is held to is 1.8e-6 ... 1.2e-5.

Quality (Cornell box, 96 x 72, depth 5, 16 spp against 1024 spp, relMSE = mean((x - T)^2 / (T^2 + 1e-2)) over RGB): the guided filter must reach 0.5 x the
unfiltered frame's relMSE with moments and 0.6 x without (the float64 replay gives 0.35 x and 0.43 x), and both below fh_denoise on the same input.  Observed:
unfiltered 0.08945, fh_denoise 0.13786, guided 0.03173 with moments (0.355 x) and 0.03893 without (0.435 x); textured box (background (0.1, 0.2, 0.4)): unfiltered
0.01060, fh_denoise 0.23692, guided 0.00824 / 0.01081.
"""
import ctypes as C

import numpy as np
import pytest

import fredholm_amd as F
from fredholm_amd import native as N
from fredholm_amd import scenes
from fredholm_amd.renderer import DeviceBuffer

pytestmark = pytest.mark.gpu

LUM = (np.float32(0.2126729), np.float32(0.7151522), np.float32(0.0721750))
KERN = (3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
DEFAULTS = dict(sigma_l=2.0, sigma_z=1.0, sigma_a=0.2, normal_power_log2=7, passes=5)


# ------------------------------------------------------------------ the restatement
def _shift(a, dx, dy):
    """a at the tap position clamped to the frame"""
    h, w = a.shape[:2]
    return a[np.clip(np.arange(h) + dy, 0, h - 1)][:, np.clip(np.arange(w) + dx, 0, w - 1)]


def _dot3(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _lum(c, dt):
    return c[..., 0] * dt(LUM[0]) + c[..., 1] * dt(LUM[1]) + c[..., 2] * dt(LUM[2])


def restate(dt, exp, beauty, normal, albedo, position=None, depth=None, moments=None, counts=None, sigma_l=2.0, sigma_z=1.0, sigma_a=0.2, normal_power_log2=7, passes=5,
            upscale=False):
    """the filter of include/fredholm_hip.h in the arithmetic `dt`, `exp` being its exponential"""
    b32 = beauty[..., :3]
    b32 = np.where(np.isnan(b32) | (np.abs(b32) > np.float32(3.0e38)), np.float32(0), b32)  # finite(): decided on the fp32 input
    Bm, Nn, A = b32.astype(dt), normal[..., :3].astype(dt), albedo[..., :3].astype(dt)
    sl, sz, sa = dt(np.float32(sigma_l)), dt(np.float32(sigma_z)), dt(np.float32(sigma_a))

    def wn_of(Nq):
        wn = np.maximum(dt(0), _dot3(Nn, Nq))
        for _ in range(normal_power_log2):
            wn = wn * wn
        return wn

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
                wn, lq = wn_of(_shift(Nn, dx, dy)), _shift(l, dx, dy)
                s0 = s0 + wn
                s1 = s1 + wn * lq
                s2 = s2 + wn * (lq * lq)
        S = np.maximum(s0, dt(np.float32(1e-6)))
        S1, S2 = s1 / S, s2 / S
        v = np.maximum(S2 - S1 * S1, dt(0))
    if position is not None:
        Pp, Z = position[..., :3].astype(dt), depth.astype(dt)
    for it in range(passes):
        s = 1 << it
        g = np.zeros(l.shape, dt)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                g = g + dt((0.5 if dx == 0 else 0.25) * (0.5 if dy == 0 else 0.25)) * _shift(v, dx, dy)
        sd = sl * np.sqrt(g) + dt(np.float32(1e-6))
        lp = _lum(c, dt)
        if position is not None:
            kz = sz * dt(np.float32(0.01)) * np.maximum(Z, dt(np.float32(1e-3))) * dt(s)
        sc, sw, sv = np.zeros(c.shape, dt), np.zeros(l.shape, dt), np.zeros(l.shape, dt)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                cq, vq = _shift(c, s * dx, s * dy), _shift(v, s * dx, s * dy)
                if dx == 0 and dy == 0:
                    wgt = np.full(l.shape, dt(9.0 / 64.0))
                else:
                    wn = wn_of(_shift(Nn, s * dx, s * dy))
                    ez = dt(0)
                    if position is not None:
                        ez = np.abs(_dot3(Nn, _shift(Pp, s * dx, s * dy) - Pp)) / (kz * np.sqrt(dt(dx * dx + dy * dy)) + dt(np.float32(1e-6)))
                    da = _shift(A, s * dx, s * dy) - A
                    ea = _dot3(da, da) / (sa * sa)
                    el = np.abs(_lum(cq, dt) - lp) / sd
                    wgt = dt(KERN[abs(dx)] * KERN[abs(dy)]) * wn * exp(-((ez + ea) + el))
                sc = sc + wgt[..., None] * cq
                sw = sw + wgt
                sv = sv + wgt * wgt * vq
        c, v = sc / sw[..., None], sv / (sw * sw)
    out = np.concatenate([c * af, np.ones(l.shape + (1,), dt)], axis=2)
    return out.repeat(2, axis=0).repeat(2, axis=1) if upscale else out


def restate64(**kw):
    with np.errstate(all="ignore"):
        return restate(np.float64, np.exp, **kw)


def restate32(oracle, **kw):
    with np.errstate(all="ignore"):
        out = restate(np.float32, lambda x: oracle.elementary("exp", x).reshape(x.shape), **kw)
    assert out.dtype == np.float32
    return out


# ------------------------------------------------------------------ device side
class Dev:
    """the layers of one case in device memory of renderer `r`"""

    def __init__(self, r, layers):
        self.r, self.bufs = r, {}
        for k, a in layers.items():
            if a is not None:
                self.bufs[k] = DeviceBuffer(r, a.nbytes)
                self.bufs[k].upload(a)
        self.h, self.w = layers["beauty"].shape[:2]

    def run(self, use_position=True, use_moments=True, upscale=False, **params):
        p = lambda k: self.bufs[k].ptr if k in self.bufs else None
        k = 4 if upscale else 1
        out = DeviceBuffer(self.r, k * self.w * self.h * 16)
        out.clear(0xFF)
        self.r.denoise_guided(self.w, self.h, p("beauty"), p("normal"), p("albedo"), out.ptr, p("position") if use_position else None, p("depth") if use_position else None,
                              p("moments") if use_moments else None, p("counts") if use_moments else None, upscale=upscale, **params)
        self.r.wait_for_completion()
        got = out.download(np.float32, ((2 if upscale else 1) * self.h, (2 if upscale else 1) * self.w, 4))
        out.free()
        return got

    def free(self):
        for b in self.bufs.values():
            b.free()


def _random_layers(w, h, seed):
    """piecewise-smooth guides (so that the edge stops neither pass nor block everything), noisy radiance with a NaN and an Inf, counts with 0 and 1"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    side = (xx + 0.5 * yy > 0.55 * w)
    nrm = np.zeros((h, w, 4), np.float32)
    nrm[..., :3] = np.where(side[..., None], np.float32([0.6, 0.0, 0.8]), np.float32([0.0, 0.28, 0.96])) + rng.normal(0, 0.02, (h, w, 3)).astype(np.float32)
    nrm[..., :3] /= np.linalg.norm(nrm[..., :3], axis=2, keepdims=True)
    nrm[0, 0] = 0.0  # a miss
    alb = np.zeros((h, w, 4), np.float32)
    alb[..., :3] = np.where((yy > 0.4 * h)[..., None], np.float32([0.7, 0.3, 0.2]), np.float32([0.25, 0.6, 0.7])) + rng.uniform(0, 0.03, (h, w, 3)).astype(np.float32)
    alb[h - 1, w - 1, :3] = 0.0  # below the floor
    depth = (2.0 + 0.05 * xx + np.where(side, 0.8, 0.0) + rng.normal(0, 0.002, (h, w))).astype(np.float32)
    pos = np.zeros((h, w, 4), np.float32)
    pos[..., 0], pos[..., 1], pos[..., 2] = (xx - w / 2) * 0.03 * depth, (yy - h / 2) * 0.03 * depth, -depth
    level = (0.3 + 0.02 * xx + np.where(side, 1.5, 0.0)).astype(np.float32)
    noise = rng.gamma(2.0, 0.5, (h, w, 3)).astype(np.float32)
    beauty = np.ones((h, w, 4), np.float32)
    beauty[..., :3] = level[..., None] * noise * alb[..., :3]
    counts = rng.integers(2, 40, (h, w)).astype(np.uint32)
    counts[0, w - 1], counts[h - 1, 0], counts[h // 2, w // 2] = 0, 1, 1
    y = beauty[..., 0] * LUM[0] + beauty[..., 1] * LUM[1] + beauty[..., 2] * LUM[2]
    rel = rng.uniform(0.2, 1.2, (h, w)).astype(np.float32)
    mom = np.stack([y, y * y * (1 + rel * rel)], axis=2).astype(np.float32)
    beauty[h // 2, 1, 0] = np.nan
    beauty[1, w // 2, 1] = np.inf
    return dict(beauty=beauty, normal=nrm, albedo=alb, position=pos, depth=depth, moments=mom, counts=counts)


def _relmse(x, t):
    x, t = x[..., :3].astype(np.float64), t[..., :3].astype(np.float64)
    return float(np.mean((x - t) ** 2 / (t ** 2 + 1e-2)))


class Frames:
    """a 96 x 72 scene at 16 spp (single-sample calls, adaptive sampling on at threshold 0 so that the moments exist) and its 1024-spp truth"""

    def __init__(self, scene, bg, depth):
        w, h = 96, 72
        r = F.Renderer(0)
        r.load_scene(scene)
        r.build_ias()
        r.set_resolution(w, h)
        r.set_adaptive_sampling(0.0)
        cam = F.Camera(**scenes.CORNELL_CAMERA)
        L = F.RenderLayer(r, w, h)
        for _ in range(16):
            r.render(cam, bg, L, 1, depth)
        r.wait_for_completion()
        self.layers = {k: L.download(k) for k in ("beauty", "normal", "albedo", "position", "depth")}
        self.layers["moments"], self.layers["counts"] = r.luminance_moments(), r.sample_counts()
        old = DeviceBuffer(r, w * h * 16)
        r.denoise(w, h, L.ptrs["beauty"], L.ptrs["normal"], L.ptrs["albedo"], old.ptr)
        r.wait_for_completion()
        self.atrous = old.download(np.float32, (h, w, 4))
        r.render(cam, bg, L, 1008, depth)  # (= 1008 single-sample calls: include/fredholm_hip.h, fh_render)
        r.wait_for_completion()
        self.truth = L.download("beauty")
        self.r, self.w, self.h = r, w, h
        self.dev = Dev(r, self.layers)

    def close(self):
        self.dev.free()
        self.r.close()


@pytest.fixture(scope="module")
def cornell():
    f = Frames(scenes.cornell_box(), (0.0, 0.0, 0.0), 5)
    yield f
    f.close()


@pytest.fixture(scope="module")
def random_cases(renderer):
    cases = {"37x29": _random_layers(37, 29, 5), "5x3": _random_layers(5, 3, 6)}
    devs = {k: Dev(renderer, v) for k, v in cases.items()}
    yield cases, devs
    for d in devs.values():
        d.free()


def _check(oracle, layers, dev, use_position, use_moments, upscale=False, **params):
    kw = dict(beauty=layers["beauty"], normal=layers["normal"], albedo=layers["albedo"], upscale=upscale, **params)
    if use_position:
        kw.update(position=layers["position"], depth=layers["depth"])
    if use_moments:
        kw.update(moments=layers["moments"], counts=layers["counts"])
    r64, r32 = restate64(**kw), restate32(oracle, **kw)
    got = dev.run(use_position, use_moments, upscale, **params)
    assert got.shape == r64.shape and np.isfinite(got).all() and (got[..., 3] == 1).all()
    scale = np.maximum(np.abs(r64), np.abs(r64[..., :3]).mean())
    e32, edev = float((np.abs(r32 - r64) / scale).max()), float((np.abs(got - r64) / scale).max())
    same = float((got.view(np.uint32) == r32.view(np.uint32)).mean())
    print(f"guided {layers['beauty'].shape[1]}x{layers['beauty'].shape[0]} pos={use_position} mom={use_moments} up={upscale} {params}: float32 error {e32:.3e}, device error {edev:.3e}, "
          f"ratio {edev / e32:.3f}, values bit-identical to float32 {same:.4f}")
    assert e32 > 0 and edev <= 4.0 * e32, (e32, edev)
    return got


VARIANTS = [(True, True), (True, False), (False, True), (False, False)]


@pytest.mark.parametrize("use_position,use_moments", VARIANTS)
@pytest.mark.parametrize("case", ["37x29", "5x3"])
def test_random_layers_match_the_restatement(random_cases, oracle, case, use_position, use_moments):
    """every tap clamps somewhere (5 x 3: everywhere); counts 0 and 1, a NaN and an Inf in the beauty, a missed pixel and an albedo below the floor"""
    cases, devs = random_cases
    _check(oracle, cases[case], devs[case], use_position, use_moments)


@pytest.mark.parametrize("use_position,use_moments", VARIANTS)
def test_cornell_frame_matches_the_restatement(cornell, oracle, use_position, use_moments):
    _check(oracle, cornell.layers, cornell.dev, use_position, use_moments)


@pytest.mark.parametrize("passes", [1, 6])
@pytest.mark.parametrize("use_position,use_moments", [(True, True), (False, False)])
def test_one_and_six_passes(random_cases, oracle, passes, use_position, use_moments):
    """six passes: hole 32 on a 37 x 29 frame, most workgroups of the last pass hold a single pixel"""
    cases, devs = random_cases
    _check(oracle, cases["37x29"], devs["37x29"], use_position, use_moments, passes=passes)


def test_parameters_reach_the_kernels(random_cases, oracle):
    cases, devs = random_cases
    _check(oracle, cases["37x29"], devs["37x29"], True, True, sigma_l=0.7, sigma_z=3.0, sigma_a=0.5, normal_power_log2=3, passes=3)
    _check(oracle, cases["37x29"], devs["37x29"], True, False, sigma_l=4.0, sigma_z=0.25, sigma_a=0.05, normal_power_log2=0, passes=2)


@pytest.mark.parametrize("use_moments", [True, False])
def test_upscale_replicates_pixels(random_cases, oracle, use_moments):
    cases, devs = random_cases
    up = _check(oracle, cases["37x29"], devs["37x29"], True, use_moments, upscale=True)
    one = devs["37x29"].run(True, use_moments)
    for oy in (0, 1):
        for ox in (0, 1):
            assert np.array_equal(up[oy::2, ox::2].view(np.uint32), one.view(np.uint32))


def test_defaults_are_the_documented_parameters(random_cases):
    cases, devs = random_cases
    d = devs["37x29"]
    out = DeviceBuffer(d.r, d.w * d.h * 16)
    i = N.DenoiseInputsC(*(d.bufs[k].ptr for k in ("beauty", "normal", "albedo", "position", "depth", "moments", "counts")))
    N.check(d.r._ctx, N.lib().fh_denoise_guided(d.r._ctx, d.w, d.h, C.byref(i), None, out.ptr, 0), "fh_denoise_guided")
    d.r.wait_for_completion()
    got = out.download(np.float32, (d.h, d.w, 4))
    out.free()
    assert np.array_equal(got.view(np.uint32), d.run(**DEFAULTS).view(np.uint32))


def test_missed_pixel_keeps_its_beauty_up_to_the_demodulation(random_cases):
    cases, devs = random_cases
    b = cases["37x29"]["beauty"][0, 0, :3]
    for variant in VARIANTS:
        got = devs["37x29"].run(*variant)[0, 0, :3]
        assert np.abs(got - b).max() <= 8 * np.finfo(np.float32).eps * np.abs(b).max()  # b / a', five passes of * (9/64) / (9/64), * a': twelve roundings of eps / 2


def test_flat_image_is_a_fixed_point(renderer):
    w, h = 70, 45
    layers = dict(beauty=np.full((h, w, 4), 0.37, np.float32), normal=np.tile(np.float32([0, 0, 1, 0]), (h, w, 1)), albedo=np.full((h, w, 4), 0.37, np.float32),
                  position=np.full((h, w, 4), 0.37, np.float32), depth=np.full((h, w), 0.37, np.float32), moments=np.full((h, w, 2), 0.37, np.float32),
                  counts=np.full((h, w), 16, np.uint32))
    d = Dev(renderer, layers)
    for variant in VARIANTS:
        assert np.allclose(d.run(*variant)[..., :3], 0.37, rtol=2e-6, atol=0)
    d.free()


def test_repeated_calls_and_a_group_give_the_same_bits(random_cases):
    cases, devs = random_cases
    first = {v: devs["37x29"].run(*v, passes=6) for v in VARIANTS}
    for v in VARIANTS:
        assert np.array_equal(first[v].view(np.uint32), devs["37x29"].run(*v, passes=6).view(np.uint32))
    g = F.Renderer(devices=[0, 0])
    d = Dev(g, cases["37x29"])
    for v in VARIANTS:
        assert np.array_equal(first[v].view(np.uint32), d.run(*v, passes=6).view(np.uint32))
    d.free()
    g.close()


def test_fh_denoise_keeps_its_bits_around_guided_calls(cornell, oracle):
    d = cornell.dev
    out = DeviceBuffer(d.r, d.w * d.h * 16)

    def atrous():
        d.r.denoise(d.w, d.h, d.bufs["beauty"].ptr, d.bufs["normal"].ptr, d.bufs["albedo"].ptr, out.ptr)
        d.r.wait_for_completion()
        return out.download(np.float32, (d.h, d.w, 4))
    before = atrous()
    d.run(True, True)
    d.run(False, False, upscale=True)
    after = atrous()
    out.free()
    want = oracle.denoise(cornell.layers["beauty"], cornell.layers["normal"], cornell.layers["albedo"])
    assert np.array_equal(before.view(np.uint32), want.view(np.uint32)) and np.array_equal(after.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(cornell.atrous.view(np.uint32), want.view(np.uint32))


def test_refused_calls_leave_the_output_and_the_context_alone(random_cases):
    cases, devs = random_cases
    d = devs["37x29"]
    good = d.run()
    out = DeviceBuffer(d.r, d.w * d.h * 16)
    out.clear(0x5A)
    names = ("beauty", "normal", "albedo", "position", "depth", "moments", "counts")
    full = {k: d.bufs[k].ptr for k in names}
    L, ctx = N.lib(), d.r._ctx

    def call(ptrs, params, w=d.w, h=d.h, dst=out.ptr):
        i = N.DenoiseInputsC(*(ptrs[k] for k in names))
        return L.fh_denoise_guided(ctx, w, h, C.byref(i), None if params is None else C.byref(N.DenoiseParamsC(*params)), dst, 0)
    ok = (2.0, 1.0, 0.2, 7, 5)
    bad = [(dict(full, **{k: None}), ok) for k in names]  # a missing required pointer, or half a pair
    for k in range(3):
        for v in (0.0, -1.0, float("nan"), float("inf")):
            bad.append((full, ok[:k] + (v,) + ok[k + 1:]))
    bad += [(full, (2.0, 1.0, 0.2, 11, 5)), (full, (2.0, 1.0, 0.2, 7, 0)), (full, (2.0, 1.0, 0.2, 7, 7))]
    for ptrs, params in bad:
        assert call(ptrs, params) == -1, (ptrs, params)
        assert b"fh_denoise_guided" in L.fh_last_error(ctx)
    assert call(full, ok, dst=None) == -1 and call(full, ok, w=0) == -1 and L.fh_denoise_guided(ctx, d.w, d.h, None, None, out.ptr, 0) == -1
    d.r.wait_for_completion()
    assert (out.download(np.uint8) == 0x5A).all()
    out.free()
    assert np.array_equal(d.run().view(np.uint32), good.view(np.uint32))


# ------------------------------------------------------------------ quality
def _quality(f):
    un = _relmse(f.layers["beauty"], f.truth)
    with_m, without_m = _relmse(f.dev.run(True, True), f.truth), _relmse(f.dev.run(True, False), f.truth)
    old = _relmse(f.atrous, f.truth)
    print(f"relMSE at 16 spp: unfiltered {un:.5f}, fh_denoise {old:.5f}, guided with moments {with_m:.5f} ({with_m / un:.3f} x), without {without_m:.5f} ({without_m / un:.3f} x)")
    return un, old, with_m, without_m


def test_quality_on_the_cornell_box(cornell):
    un, old, with_m, without_m = _quality(cornell)
    assert with_m <= 0.5 * un, (with_m, un)
    assert without_m <= 0.6 * un, (without_m, un)
    assert with_m < old and without_m < old, (with_m, without_m, old)


def test_quality_on_the_textured_box_beats_the_slot_filter():
    """texture features about one pixel wide: the guided filter is only required to do better than fh_denoise here (it does not beat the unfiltered frame)"""
    f = Frames(scenes.textured_cornell_box(), (0.1, 0.2, 0.4), 5)
    try:
        un, old, with_m, without_m = _quality(f)
        assert with_m < old and without_m < old, (with_m, without_m, old)
    finally:
        f.close()
