"""GPU tests (-m gpu) of the post chain's own kernels (fredholm_amd/csrc/post.hip: k_bloom_threshold, k_bloom_blur, k_copy, the three tone maps, k_atrous) away
from the one operating point the parity tests run them at: aberrations that really displace the fetch, fetch addresses past the last pixel, the three tone maps
against each other, bloom over sigmas, thresholds and special values, the weight cache, images smaller than a block, refusals, and the denoiser slot on small, odd
and non-finite layers.

Comparisons are bit for bit unless stated; where both sides are NaN the position must agree and the payload need not (x86 and gfx950 sign their default NaN
differently).  The three buffers of the chain start from distinct finite sentinels (HI, TMP, OUT), the checker (oracle.post_process) is handed the same contents,
and the assertions cover the whole of out, tmp and hi: the border outside the floor-division grid is never written, and the blur and an aberrated fetch READ it.

The fetch addresses come from tests/test_post_chain_host.py: fetch_model, the numpy model of the reference's tone_mapping_kernel, limited to the last pixel
(include/fredholm_hip.h, fh_post_process).  In the past-the-end tests beauty_temp is the front of a larger allocation, so that even an unlimited address would read
allocated memory; the guard behind it holds GUARD, which tone-maps to exactly 1.0, a value no pixel of the test images reaches.

FLOAT64.  The blur (post-process.cu:76-109) and the a-trous filter (post.hip: k_atrous) are restated below once and run in float64 and in float32 (exp from the
checker, taps in the kernels' order).  The device may differ from the float64 result by at most 4 x the largest float32-versus-float64 difference of the same case,
relative to max(|value|, image mean): the convention and the factor of tests/test_gpu_denoise_guided.py.  The tap order is fixed here, so the factor covers fp32
rounding alone.  These comparisons run on finite inputs -- the same images with the specials NaN, +-inf and 3e38 left out: a blur spreads one inf over its 33 x 33
window (and 0 * inf = NaN where the weights underflow), and sums of 3e38 overflow in float32 and not in float64.
MEASURED on an MI355X (printed by the tests): (device error) / (float32 error) = 1.000 in all 55 comparisons, and the device's values are bit-identical to the
float32 restatement in every one.  float32 error, smallest .. largest over the three thresholds:
  bloom, sigma 0.25:  16x16 1.47e-7 .. 2.28e-7;  16x40 2.21e-7 .. 2.35e-7;  33x17 2.40e-7 .. 2.47e-7;  70x50 2.11e-7 .. 2.82e-7;  48x130 2.20e-7 .. 2.60e-7
  bloom, sigma 5:     16x16 6.55e-7 .. 1.02e-6;  16x40 8.27e-7 .. 1.05e-6;  33x17 1.02e-6 .. 1.23e-6;  70x50 1.15e-6 .. 1.25e-6;  48x130 1.03e-6 .. 1.18e-6
  bloom, sigma 200:   16x16 4.32e-7 .. 9.06e-7;  16x40 1.20e-6 .. 1.30e-6;  33x17 1.16e-6 .. 1.25e-6;  70x50 1.35e-6 .. 1.39e-6;  48x130 1.34e-6 .. 1.46e-6
  a-trous (the same with and without upscaling):  1x1 6.03e-10;  5x3 3.66e-7;  19x17 3.53e-7;  33x64 4.72e-7;  70x45 5.37e-7
so the bound the device is held to is 5.9e-7 .. 5.8e-6 for the blur and 2.4e-9 .. 2.1e-6 for the filter.
"""
import numpy as np
import pytest

import test_gpu_auto_exposure as A
import test_gpu_local_exposure as X
import test_post_chain_host as H

pytestmark = pytest.mark.gpu

f32 = np.float32
HI, TMP, OUT, GUARD = 3.0, 0.625, 0.25, 1.0e6  # what hi / tmp / out hold before a call; what lies behind tmp (and behind the denoiser's output)
ISO = 80.0
inf, nan = float("inf"), float("nan")


def same(a, b):
    ok = X.same_bits(a, b)
    assert ok.all(), (np.argwhere(~ok)[:4], np.asarray(a)[~ok][:4], np.asarray(b)[~ok][:4])
    return True


def written(w, h):
    """(gh, gw): the floor-division grid, post-process.cu:9-11"""
    return min(max(h // 16, 1) * 16, h), min(max(w // 16, 1) * 16, w)


def params(bloom=False, ca=0.0, threshold=2.0, sigma=5.0, iso=ISO):
    import fredholm_amd as F
    return F.PostProcessParams(use_bloom=bloom, bloom_threshold=threshold, bloom_sigma=sigma, ISO=iso, chromatic_aberration=ca)


def run_chain(r, img, pp):
    """fh_post_process with hi, tmp and out at their sentinels and w + 16 pixels of GUARD behind tmp: dict(out, tmp, hi, guard, error)"""
    from fredholm_amd.native import FredholmError
    from fredholm_amd.renderer import DeviceBuffer
    h, w = img.shape[:2]
    n, guard = w * h, w + 16
    bufs = [DeviceBuffer(r, n * 16), DeviceBuffer(r, n * 16), DeviceBuffer(r, (n + guard) * 16), DeviceBuffer(r, n * 16)]
    try:
        bufs[0].upload(img)
        bufs[1].upload(np.full((n, 4), HI, np.float32))
        bufs[2].upload(np.concatenate([np.full((n, 4), TMP, np.float32), np.full((guard, 4), GUARD, np.float32)]))
        bufs[3].upload(np.full((n, 4), OUT, np.float32))
        error = None
        try:
            r.post_process(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, w, h, pp, bufs[3].ptr)
        except FredholmError as e:
            error = e
        r.wait_for_completion()
        tmp = bufs[2].download(np.float32, (n + guard, 4))
        return dict(out=bufs[3].download(np.float32, (h, w, 4)), tmp=tmp[:n].reshape(h, w, 4), hi=bufs[1].download(np.float32, (h, w, 4)), guard=tmp[n:], error=error)
    finally:
        for b in bufs:
            b.free()


def checker(oracle, img, pp):
    out, tmp, hi = oracle.post_process(img, pp.use_bloom, pp.bloom_threshold, pp.bloom_sigma, pp.ISO, pp.chromatic_aberration, hi=np.full_like(img, HI), tmp=np.full_like(img, TMP),
                                       out=np.full_like(img, OUT), full=True)
    return dict(out=out, tmp=tmp, hi=hi)


def equals_checker(got, want):
    assert (got["guard"] == f32(GUARD)).all()  # nothing is ever written behind beauty_temp
    return all(same(got[k], want[k]) for k in ("out", "tmp", "hi"))


def copied(img):
    """beauty_temp after the chain without bloom: the input on the grid, the sentinel outside it"""
    gh, gw = written(img.shape[1], img.shape[0])
    tmp = np.full_like(img, TMP)
    tmp[:gh, :gw] = img[:gh, :gw]
    return tmp


def model_out(oracle, tmp, x, ca):
    """the whole output buffer by the index model: tmp gathered at fetch_model's addresses limited to the last pixel, times x, through the checker's uchimura and sRGB"""
    h, w = tmp.shape[:2]
    gh, gw = written(w, h)
    idx = np.minimum(H.fetch_model(w, h, ca), w * h - 1)
    flat = tmp.reshape(-1, 4)
    with np.errstate(all="ignore"):
        rgb = np.stack([flat[idx[k].reshape(-1), k] for k in range(3)], axis=1) * f32(x)
    out = np.full((h, w, 4), OUT, np.float32)
    out[:gh, :gw, :3] = oracle.math("linear_to_srgb", oracle.math("uchimura", rgb)).reshape(h, w, 3)[:gh, :gw]
    out[:gh, :gw, 3] = 1.0
    return out


def distinct_image(w, h):
    """a different value in every pixel and channel, 0.01 .. 5"""
    n = 4 * w * h
    img = (0.01 + 4.99 * np.random.default_rng(w * 1000 + h).permutation(n) / n).astype(np.float32).reshape(h, w, 4)
    assert np.unique(img).size == n
    return img


@pytest.fixture()
def chain(renderer):
    """the session's renderer with auto-exposure and local exposure off, before and after"""
    renderer.clear_local_exposure()
    renderer.clear_auto_exposure()
    yield renderer
    renderer.clear_local_exposure()
    renderer.clear_auto_exposure()


# ------------------------------------------------------------------ a. aberration that really displaces
@pytest.mark.parametrize("w,h", [(16, 16), (33, 17), (64, 48), (70, 50), (48, 130)])
def test_displacing_aberration_equals_the_checker_and_the_index_model(chain, oracle, w, h):
    img = distinct_image(w, h)
    gh, gw = written(w, h)
    for ca in (0.02 * w * h, 0.1 * w * h, 0.45 * w * h, -0.2 * w):
        model = H.fetch_model(w, h, ca)
        # the reference is defined at the positive values: nothing is limited there.  The reversed fringe moves the last row down by a fraction of a row, and since
        # the row is not floored before it is multiplied by w, that fraction alone carries the address up to 13 pixels past the image: limited
        assert (model.max() <= w * h - 1) == (ca > 0), (w, h, ca, model.max())
        rows = model // w
        moved = (rows[2] != np.arange(h)[:, None])[:gh, :gw]
        if ca == 0.1 * w * h:
            assert 2 * int(moved.sum()) >= gh * gw, (w, h, int(moved.sum()))  # at least half of the written pixels take blue from another row
            assert (w, h) != (70, 50) or int((rows[2] != np.arange(h)[:, None]).sum()) == 3150
        assert (model[1] != model[2]).any() and (model[0] == np.arange(w * h).reshape(h, w)).all()
        pp = params(ca=ca)
        got = run_chain(chain, img, pp)
        assert got["error"] is None
        equals_checker(got, checker(oracle, img, pp))
        same(got["tmp"], copied(img))
        same(got["out"], model_out(oracle, copied(img), X.iso_exposure(oracle, ISO), ca))
        same(got["hi"], np.full_like(img, HI))


# ------------------------------------------------------------------ b. fetch addresses past the end
@pytest.mark.parametrize("w,h", [(16, 16), (64, 48)])
def test_a_fetch_address_past_the_last_pixel_reads_the_last_pixel(chain, oracle, w, h):
    img = distinct_image(w, h)
    guard = w + 16
    assert (oracle.math("linear_to_srgb", oracle.math("uchimura", np.full((1, 3), GUARD, np.float32) * X.iso_exposure(oracle, ISO))) == 1.0).all()
    for ca in H.overrunning(w, h):
        assert H.fetch_model(w, h, ca).max() > w * h - 1 and H.fetch_model(w, h, ca).max() < w * h + guard  # needed, and inside the allocation even if unlimited
        pp = params(ca=ca)
        got = run_chain(chain, img, pp)
        assert got["error"] is None
        want = model_out(oracle, copied(img), X.iso_exposure(oracle, ISO), ca)
        assert (want[..., :3] < 1.0).all()  # what a read of the guard would give is not among the expected values
        same(got["out"], want)
        assert got["guard"].shape == (guard, 4) and (got["guard"] == f32(GUARD)).all()
        equals_checker(got, checker(oracle, img, pp))


# ------------------------------------------------------------------ c. the three tone maps are one
@pytest.mark.parametrize("which", ["one", "tenth", "reversed"])
@pytest.mark.parametrize("w,h", [(70, 50), (33, 17)])
def test_the_metered_and_the_local_tone_map_are_the_plain_one(chain, oracle, w, h, which):
    ca = {"one": 1.0, "tenth": 0.1 * w * h, "reversed": -1.0 * w}[which]
    img = X.image(w, h, seed=5)
    # metered at a pinned exposure = plain at the matching ISO (ISO = 120 * 2^k is an exposure of exactly 2^k, and fhe_pow(2, k) is exact)
    for k in (-3, 2):
        chain.clear_auto_exposure()
        off = A._post(chain, img, params(ca=ca, iso=120.0 * 2.0 ** k))
        chain.set_auto_exposure(min_ev=float(k), max_ev=float(k))
        on = A._post(chain, img, params(ca=ca))
        assert chain.auto_exposure_state()["ev"] == k
        same(on, off)
    chain.clear_auto_exposure()
    # local exposure with zero shares = switched off
    off, _ = X._post(chain, img, params(ca=ca))
    chain.set_local_exposure(**X.params(highlights=0.0, shadows=0.0))
    on, _ = X._post(chain, img, params(ca=ca))
    same(on, off)
    # local exposure with the defaults = the restatement (whose tone map fetches where the plain one does)
    chain.set_local_exposure(**X.DEFAULTS)
    out, tmp = X._post(chain, img, params(ca=ca))
    X._check(oracle, out, tmp, img, X.DEFAULTS, X.iso_exposure(oracle, ISO), ca, chain.local_exposure_base())
    gh, gw = X._written(w, h)
    assert not X.same_bits(out[:gh, :gw], off[:gh, :gw]).all()


# ------------------------------------------------------------------ d. bloom
BLOOM_SPECIALS = [0.0, -1.0, 1e-40, 3e38, inf, nan]
FINITE_SPECIALS = [0.0, -1.0, 1e-40]


def bloom_image(w, h, specials):
    """the parity test's distribution (values to 8, most of them small); every 7th pixel has one channel special"""
    img = (np.random.default_rng(31 * w + h).uniform(0, 1, (h, w, 4)) ** 3 * 8).astype(np.float32)
    flat = img.reshape(-1, 4)
    idx = np.arange(3, w * h, 7)
    flat[idx, np.arange(idx.size) % 3] = np.array(specials, np.float32)[(np.arange(idx.size) // 3) % len(specials)]
    return img


def luminance32(img):
    with np.errstate(all="ignore"):
        return (img[..., 0] * f32(0.2126729) + img[..., 1] * f32(0.7151522)) + img[..., 2] * f32(0.0721750)


def thresholded(img, threshold):
    """beauty_high_luminance after bloom_kernel_0 (post-process.cu:60-74): the pixel where its luminance is above the threshold, 0 elsewhere; the sentinel off the grid"""
    gh, gw = written(img.shape[1], img.shape[0])
    hi = np.full_like(img, HI)
    with np.errstate(all="ignore"):
        hi[:gh, :gw] = np.where((luminance32(img) > f32(threshold))[..., None], img, f32(0))[:gh, :gw]
    return hi


def blurred(dt, exp, img, hi, sigma):
    """beauty_temp on the grid after bloom_kernel_1 (post-process.cu:76-109) in the arithmetic dt: v outer, u inner, taps clamped to the WHOLE image, b0 + sum * (1 / w_sum)"""
    h, w = img.shape[:2]
    gh, gw = written(w, h)
    Hh = hi.astype(dt)
    acc, wsum = np.zeros((gh, gw, 4), dt), dt(0)
    d2 = np.array([[u * u + v * v for u in range(-16, 17)] for v in range(-16, 17)], np.float32).astype(dt)
    wt = exp(-d2 / (dt(2) * dt(f32(sigma)))).astype(dt)
    for v in range(-16, 17):
        rows = Hh[np.clip(np.arange(gh) + v, 0, h - 1)]
        for u in range(-16, 17):
            hh = wt[v + 16, u + 16]
            acc = acc + hh * rows[:, np.clip(np.arange(gw) + u, 0, w - 1)]
            wsum = wsum + hh
    return img[:gh, :gw].astype(dt) + acc * (dt(1) / wsum)


def held_to_float64(case, got, r32, r64):
    assert r32.dtype == np.float32 and r64.dtype == np.float64 and got.shape == r64.shape
    scale = np.maximum(np.abs(r64), np.abs(r64[..., :3]).mean())
    e32, edev = float((np.abs(r32 - r64) / scale).max()), float((np.abs(got - r64) / scale).max())
    print(f"{case}: float32 error {e32:.3e}, device error {edev:.3e}, ratio {edev / e32 if e32 else float(edev != 0):.3f}, "
          f"values bit-identical to float32 {float((got.view(np.uint32) == r32.view(np.uint32)).mean()):.4f}")
    assert edev <= 4.0 * e32, (case, e32, edev)


@pytest.mark.parametrize("sigma", [0.25, 5.0, 200.0])
@pytest.mark.parametrize("w,h", [(16, 16), (16, 40), (33, 17), (70, 50), (48, 130)])
def test_bloom_equals_the_checker_and_the_float64_blur(chain, oracle, w, h, sigma):
    gh, gw = written(w, h)
    exp32 = lambda x: oracle.elementary("exp", x).reshape(x.shape)
    plain = bloom_image(w, h, FINITE_SPECIALS)
    lum = luminance32(plain)[:gh, :gw]
    pick = np.unravel_index(np.argsort(lum, axis=None)[(3 * lum.size) // 5], lum.shape)  # a pixel three fifths up the ranks: some pass, it must not
    for name, threshold in (("2", 2.0), ("negative", -1.0), ("a pixel's own", float(lum[pick]))):
        # every special value, against the checker
        img = bloom_image(w, h, BLOOM_SPECIALS)
        pp = params(True, 1.0, threshold, sigma)
        got = run_chain(chain, img, pp)
        assert got["error"] is None
        equals_checker(got, checker(oracle, img, pp))
        same(got["hi"], thresholded(img, threshold))
        assert np.isnan(got["tmp"]).any() and np.isfinite(got["tmp"]).any()
        # finite input: the checker again, and the float64 blur
        got = run_chain(chain, plain, pp)
        equals_checker(got, checker(oracle, plain, pp))
        hi = thresholded(plain, threshold)
        same(got["hi"], hi)
        passed = (got["hi"][:gh, :gw] != 0).any(axis=2)
        if name == "negative":
            same(got["hi"][:gh, :gw], plain[:gh, :gw])  # every pixel passes, zeros included
        if name == "a pixel's own":
            assert not passed[pick] and plain[pick][:3].min() > 0 and passed.any() and (lum[passed] > lum[pick]).all()  # the comparison is strict
            assert passed.sum() == (lum > lum[pick]).sum()
        with np.errstate(all="ignore"):
            r32, r64 = blurred(np.float32, exp32, plain, hi, sigma), blurred(np.float64, np.exp, plain, hi, sigma)
        assert np.isfinite(got["tmp"]).all()
        held_to_float64(f"bloom {w}x{h} sigma {sigma} threshold {name}", got["tmp"][:gh, :gw], r32, r64)
    if sigma == 0.25:
        assert oracle.elementary("exp", [-f32(200.0) / (f32(2) * f32(sigma))])[0] == 0  # the far weights underflow
    if (w, h) == (16, 16):
        assert gh == h and gw == w  # one block: every tap of its rim is clamped


# ------------------------------------------------------------------ e. the weight cache
def test_the_blur_weights_follow_sigma_there_and_back(oracle):
    import fredholm_amd as F
    w, h = 33, 17
    img = bloom_image(w, h, FINITE_SPECIALS)
    r = F.Renderer(0)
    try:
        first, second, third = (run_chain(r, img, params(True, 1.0, 2.0, s)) for s in (5.0, 0.25, 5.0))
    finally:
        r.close()
    fresh = F.Renderer(0)
    try:
        alone = run_chain(fresh, img, params(True, 1.0, 2.0, 0.25))
    finally:
        fresh.close()
    for k in ("out", "tmp", "hi"):
        same(third[k], first[k])
        same(second[k], alone[k])
    assert not X.same_bits(second["tmp"], first["tmp"]).all()
    equals_checker(second, checker(oracle, img, params(True, 1.0, 2.0, 0.25)))


# ------------------------------------------------------------------ f. small and refused
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (16, 7), (7, 40)])
def test_an_image_smaller_than_a_block_equals_the_checker(chain, oracle, w, h):
    img = distinct_image(w, h)
    gh, gw = written(w, h)
    assert gw == min(16, w) and gh == (h if h < 16 else (h // 16) * 16)
    for ca in (0.0, 1.0, 0.1 * w * h, -1.0 * w):
        pp = params(ca=ca)
        got = run_chain(chain, img, pp)
        assert got["error"] is None
        equals_checker(got, checker(oracle, img, pp))
        same(got["out"], model_out(oracle, copied(img), X.iso_exposure(oracle, ISO), ca))


@pytest.mark.parametrize("w,h", [(15, 40), (40, 15)])
def test_bloom_below_16_pixels_is_refused_and_leaves_the_buffers_and_the_context_alone(chain, oracle, w, h):
    img = bloom_image(w, h, FINITE_SPECIALS)
    got = run_chain(chain, img, params(True, 1.0))
    assert got["error"] is not None and "fh_post_process failed (-3)" in str(got["error"]) and "at least 16x16" in str(got["error"])  # -3: FH_E_UNSUPPORTED
    for k, v in (("out", OUT), ("tmp", TMP), ("hi", HI)):
        assert (got[k] == f32(v)).all(), k
    big = bloom_image(33, 17, FINITE_SPECIALS)
    pp = params(True, 1.0)
    equals_checker(run_chain(chain, big, pp), checker(oracle, big, pp))
    pp = params(False, 1.0)
    equals_checker(run_chain(chain, img, pp), checker(oracle, img, pp))  # without bloom the same size is served


# ------------------------------------------------------------------ g. the denoiser slot
DENOISE_SPECIALS = [nan, inf, -inf, 3.1e38, -2.0]


def denoise_layers(w, h, specials):
    rng = np.random.default_rng(7 * w + h)
    beauty = np.ones((h, w, 4), np.float32)
    beauty[..., :3] = np.exp2(rng.uniform(-8.0, 8.0, (h, w, 3)))
    if specials:
        b3 = beauty[..., :3].reshape(-1).copy()
        b3[::9] = np.array(specials, np.float32)[np.arange(b3[::9].size) % len(specials)]
        beauty[..., :3] = b3.reshape(h, w, 3)
    normal = np.zeros((h, w, 4), np.float32)
    n3 = rng.normal(0.0, 1.0, (h, w, 3))
    normal[..., :3] = n3 / np.linalg.norm(n3, axis=2, keepdims=True)
    albedo = np.ones((h, w, 4), np.float32)
    albedo[..., :3] = rng.uniform(0.0, 1.0, (h, w, 3))
    nf, af = normal.reshape(-1, 4), albedo.reshape(-1, 4)
    nf[1::11, :3] = 0.0   # misses
    af[2::5, 1] = 0.0     # exact zeros and negatives: the 0.01 floor
    af[4::13, 2] = -0.25
    af[0, 0] = 0.005
    return beauty, normal, albedo


def atrous(dt, exp, beauty, normal, albedo, upscale):
    """fh_denoise as post.hip's k_atrous defines it, in the arithmetic dt"""
    K = [dt(3.0 / 8.0), dt(1.0 / 4.0), dt(1.0 / 16.0)]
    b = beauty[..., :3]
    b = np.where(np.isnan(b) | (np.abs(b) > f32(3.0e38)), f32(0), b).astype(dt)
    A, Nn = albedo[..., :3].astype(dt), normal[..., :3].astype(dt)
    floor = np.maximum(A, dt(f32(0.01)))
    c = b / floor
    h, w = c.shape[:2]
    sq = lambda d: d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    inv_sn, inv_sa = dt(1) / (dt(f32(0.35)) * dt(f32(0.35))), dt(1) / (dt(f32(0.2)) * dt(f32(0.2)))
    for it in range(5):
        s = 1 << it
        inv_sc = dt(1) / (dt(2) * dt(2) * (dt(1) / dt(1 << (2 * it))))
        acc, sw = np.zeros_like(c), np.zeros((h, w), dt)
        for dy in range(-2, 3):
            qy = np.clip(np.arange(h) + dy * s, 0, h - 1)
            for dx in range(-2, 3):
                qx = np.clip(np.arange(w) + dx * s, 0, w - 1)
                cq, nq, aq = c[qy][:, qx], Nn[qy][:, qx], A[qy][:, qx]
                m = (cq[..., 0] + cq[..., 1] + cq[..., 2]) + (c[..., 0] + c[..., 1] + c[..., 2])
                den = m * m * (dt(1) / dt(9)) + dt(f32(1e-4))
                e = (sq(cq - c) / den) * inv_sc + sq(nq - Nn) * inv_sn + sq(aq - A) * inv_sa
                wgt = K[abs(dx)] * K[abs(dy)] * exp(-e)
                acc = acc + wgt[..., None] * cq
                sw = sw + wgt
        c = acc * (dt(1) / sw)[..., None]
    out = np.concatenate([c * floor, np.ones((h, w, 1), dt)], axis=2)
    return out.repeat(2, axis=0).repeat(2, axis=1) if upscale else out


def run_denoise(r, beauty, normal, albedo, upscale):
    """fh_denoise into an allocation with one more row of GUARD behind the image: (output, guard row)"""
    from fredholm_amd.renderer import DeviceBuffer
    h, w = beauty.shape[:2]
    k = 2 if upscale else 1
    H2, W2 = k * h, k * w
    bufs = [DeviceBuffer(r, w * h * 16) for _ in range(3)] + [DeviceBuffer(r, (H2 + 1) * W2 * 16)]
    try:
        for b, a in zip(bufs, (beauty, normal, albedo)):
            b.upload(a)
        bufs[3].upload(np.concatenate([np.full((H2, W2, 4), OUT, np.float32), np.full((1, W2, 4), GUARD, np.float32)]))
        r.denoise(w, h, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, upscale=upscale)
        r.wait_for_completion()
        got = bufs[3].download(np.float32, (H2 + 1, W2, 4))
        return got[:H2], got[H2]
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("upscale", [False, True])
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (19, 17), (33, 64), (70, 45)])
def test_denoiser_slot_on_small_odd_and_non_finite_layers(renderer, oracle, w, h, upscale):
    exp32 = lambda x: oracle.elementary("exp", x).reshape(x.shape)
    plain = None
    for specials in (DENOISE_SPECIALS, None):
        lay = denoise_layers(w, h, specials)
        assert specials is None or not np.isfinite(lay[0]).all()
        got, guard = run_denoise(renderer, *lay, upscale)
        same(got, oracle.denoise(*lay, upscale=upscale))
        assert np.array_equal(X._bits(guard), X._bits(np.full_like(guard, GUARD)))
        assert np.isfinite(got).all() and (got[..., 3] == 1).all()
        if upscale:
            assert got.shape == (2 * h, 2 * w, 4)
            plain, _ = run_denoise(renderer, *lay, False)
            for a in (got[::2, ::2], got[1::2, ::2], got[::2, 1::2], got[1::2, 1::2]):  # the four replicated pixels
                same(a, plain)
    with np.errstate(all="ignore"):
        r32, r64 = atrous(np.float32, exp32, *lay, upscale), atrous(np.float64, np.exp, *lay, upscale)
    held_to_float64(f"a-trous {w}x{h} upscale {int(upscale)}", got, r32, r64)
    assert (lay[2][..., :3] < 0.01).any()  # the floor is taken, at 1 x 1 too
    assert w * h < 15 or ((lay[2][..., :3] < 0).any() and (lay[2][..., :3] == 0).any() and (np.abs(lay[1][..., :3]).sum(axis=2) == 0).any())


def test_denoiser_slot_leaves_a_flat_image_alone(renderer):
    w, h = 19, 17
    flat = np.full((h, w, 4), 0.37, np.float32)
    got, guard = run_denoise(renderer, flat, flat, flat, False)
    assert np.allclose(got[..., :3], 0.37, rtol=2e-6) and (got[..., 3] == 1).all() and (guard == f32(GUARD)).all()
