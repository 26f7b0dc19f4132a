"""Local exposure of the post chain on the device (include/fredholm_hip.h: fh_set_local_exposure ... fh_get_local_exposure_base; post.hip: k_lx_down, k_lx_atrous,
k_tone_map_local) against the numpy restatement of the header's five steps below, which tests/test_local_exposure_host.py pins, bit for bit, to
csrc/fh_local_exposure.h compiled for the host.  The restatement is written once and runs in two number formats: Ops32 (numpy float32, one rounding per operation,
log2 / exp / pow from the checker: oracle.elementary) and Ops64 (every float a double, numpy's log2 / exp / exp2), the float64 twin whose distance from the float32
one the host test bounds and whose operator properties it asserts.

Compared as bits: the quarter-resolution base (fh_get_local_exposure_base) and every written pixel of the tone-mapped output; the never-written border outside the
floor-division grid must stay as the caller left it.  "Same bits" treats two NaNs as the same: a NaN, +-inf or > 3e38 channel reaches the tone map unchanged (only the
log image sanitises it) and comes out as a NaN whose sign bit is the processor's choice (inf * 0 is -NaN on x86 and +NaN on the device).
The tone map's own input (beauty_temp: the copy, or the bloom's output) is read back from the device and, with bloom, checked against the switched-off call's: bloom
is not this feature's.  With bloom on the special pixels are 0, negative and NaN only -- none passes the threshold -- so that the blur does not spread them."""
import ctypes as C

import numpy as np
import pytest

f32 = np.float32
DEFAULTS = dict(highlights=0.5, shadows=0.5, pivot=0.18, max_stops=4.0, sigma_range=1.0, passes=4)
LUM = (0.2126729, 0.7151522, 0.0721750)
KERN = (3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
SPECIALS = [0.0, -0.0, -1.0, -3.5e4, np.nan, np.inf, -np.inf, 3.2e38, -3.2e38]
MILD_SPECIALS = [0.0, -0.0, -1.0, -3.5e4, np.nan]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    """elementwise: the same bits, or both NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


# ------------------------------------------------------------------ the restatement, once, in two number formats
class Ops32:
    """float32, one rounding per operation; the elementary functions are the checker's"""
    t = np.float32

    def __init__(self, oracle):
        self.o = oracle

    def log2(self, x):
        return self.o.elementary("log2", np.asarray(x, np.float32))

    def exp(self, x):
        return self.o.elementary("exp", np.asarray(x, np.float32))

    def pow2(self, y):
        y = np.asarray(y, np.float32)
        return self.o.elementary("pow", np.full_like(y, 2.0), y)


class Ops64:
    """the float64 twin"""
    t = np.float64
    log2 = staticmethod(np.log2)
    exp = staticmethod(np.exp)
    pow2 = staticmethod(np.exp2)


def log_image(ops, img):
    """step 1: (h, w) from an (h, w, 4) float32 image"""
    t = ops.t
    with np.errstate(all="ignore"):
        ch = [np.where(np.isnan(img[..., k]) | (np.abs(img[..., k]) > f32(3.0e38)), f32(0), img[..., k]).astype(t) for k in range(3)]
        c = [t(f32(v)) for v in LUM]
        l = (ch[0] * c[0] + ch[1] * c[1]) + ch[2] * c[2]
        return ops.log2(np.maximum(l, t(2.0 ** -24)))


def quarter_image(ops, L):
    """step 2: row sums left to right, then top to bottom, over the in-frame pixels of each 4 x 4 block"""
    t = ops.t
    h, w = L.shape
    h4, w4 = (h + 3) // 4, (w + 3) // 4
    pad = np.zeros((4 * h4, 4 * w4), t)
    pad[:h, :w] = L
    blk = pad.reshape(h4, 4, w4, 4)
    n_cols = np.minimum(4, w - 4 * np.arange(w4))
    n_rows = np.minimum(4, h - 4 * np.arange(h4))
    rows = blk[..., 0].copy()
    for k in range(1, 4):
        rows = np.where((n_cols > k)[None, None, :], rows + blk[..., k], rows)
    s = rows[:, 0, :].copy()
    for k in range(1, 4):
        s = np.where((n_rows > k)[:, None], s + rows[:, k, :], s)
    return s / (n_rows[:, None] * n_cols[None, :]).astype(t)


def atrous_pass(ops, D, step, inv_sr):
    """step 3, one pass"""
    t = ops.t
    h4, w4 = D.shape
    Y, X = np.arange(h4), np.arange(w4)
    num, den = np.zeros_like(D), np.zeros_like(D)
    for dy in range(-2, 3):
        qy = np.clip(Y + step * dy, 0, h4 - 1)
        for dx in range(-2, 3):
            qx = np.clip(X + step * dx, 0, w4 - 1)
            Dq = D[qy][:, qx]
            d = (Dq - D) * inv_sr
            wt = (t(f32(KERN[abs(dx)])) * t(f32(KERN[abs(dy)]))) * ops.exp(-(d * d))
            num = num + wt * Dq
            den = den + wt
    return num / den


def base_layer(ops, img, p):
    """steps 1 - 3: (log image, quarter image, base)"""
    t = ops.t
    inv_sr = t(1) / t(f32(p["sigma_range"]))
    L = log_image(ops, img)
    D0 = quarter_image(ops, L)
    D = D0
    for i in range(p["passes"]):
        D = atrous_pass(ops, D, 1 << i, inv_sr)
    return L, D0, D


def upsample(ops, base, L, p):
    """step 4: B per pixel, and where the fall-back B = l_p was taken"""
    t = ops.t
    inv_sr = t(1) / t(f32(p["sigma_range"]))
    h, w = L.shape
    h4, w4 = base.shape

    def axis(n, n4):
        f = (np.arange(n).astype(t) + t(0.5)) * t(0.25) - t(0.5)
        f0 = np.floor(f)
        tt = f - f0
        i0 = f0.astype(np.int64)
        return (np.clip(i0, 0, n4 - 1), np.clip(i0 + 1, 0, n4 - 1)), (t(1) - tt, tt)
    xi, wx = axis(w, w4)
    yi, wy = axis(h, h4)
    num, den = np.zeros_like(L), np.zeros_like(L)
    for b in range(2):
        for a in range(2):
            Q = base[yi[b]][:, xi[a]]
            d = (Q - L) * inv_sr
            wt = (wy[b][:, None] * wx[a][None, :]) * ops.exp(-(d * d))
            num = num + wt * Q
            den = den + wt
    ok = den > t(f32(1e-6))
    with np.errstate(all="ignore"):
        return np.where(ok, num / np.where(ok, den, t(1)), L), ~ok


def gain(ops, B, exposure, p):
    """step 5: (x, the correction g in stops before its clamp)"""
    t = ops.t
    exposure = t(exposure)
    log2pivot = ops.log2(np.array([p["pivot"]], f32).astype(t))[0]
    le = ops.log2(np.array([exposure], t))[0]
    d = (B + le) - log2pivot
    raw = -np.where(d > 0, t(f32(p["highlights"])), t(f32(p["shadows"]))) * d
    ms = t(f32(p["max_stops"]))
    g = np.fmax(-ms, np.fmin(raw, ms))
    return exposure * ops.pow2(g), raw


def local_gain(ops, img, p, exposure):
    """steps 1 - 5: (base, x per pixel, diagnostics)"""
    L, D0, base = base_layer(ops, img, p)
    B, fell_back = upsample(ops, base, L, p)
    x, raw = gain(ops, B, exposure, p)
    return base, x, dict(L=L, D0=D0, B=B, fell_back=fell_back, raw=raw)


def iso_exposure(oracle, iso):
    return oracle.math("exposure", [[1.0, 1.0, iso]])[0, 1]


def tone_map(oracle, tmp, x, ca):
    """fh_post_process's tone map of the (h, w, 4) image tmp with r, g, b multiplied by x (a scalar or (h, w)): float pixel addressing as the kernel computes it"""
    h, w = tmp.shape[:2]
    i, j = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    uvx, uvy = i / f32(w), j / f32(h)
    inv = f32(1) / f32(w * h)
    dx, dy = (uvx - f32(0.5)) * inv * f32(ca), (uvy - f32(0.5)) * inv * f32(ca)
    c01 = lambda v: np.fmax(f32(0), np.fmin(v, f32(1)))
    flat = tmp.reshape(-1, 4)
    cols = []
    for k in range(3):
        cx, cy = c01(uvx - f32(k) * dx), c01(uvy - f32(k) * dy)
        idx = np.minimum((cx * f32(w) + f32(w) * (cy * f32(h))).astype(np.int32), w * h - 1)  # an address past the last pixel reads the last pixel (fredholm_hip.h)
        with np.errstate(all="ignore"):
            cols.append(flat[idx.reshape(-1), k].reshape(h, w) * np.asarray(x, np.float32))
    rgb = np.stack(cols, axis=-1).reshape(-1, 3)
    return oracle.math("linear_to_srgb", oracle.math("uchimura", rgb)).reshape(h, w, 3)


# ------------------------------------------------------------------ images
FRAMES = [(70, 45), (64, 48), (16, 16), (19, 17)]  # partial blocks on both edges; whole blocks; one tile; a quarter image smaller than the hole from pass 2 on
PARAMS = {"defaults": params(),
          "one-pass": params(passes=1, sigma_range=0.25, highlights=0.8, shadows=0.3),
          "six-pass": params(passes=6, sigma_range=4.0, highlights=0.2, shadows=1.0, max_stops=1.5, pivot=0.5)}  # (max_stops binds: test 1 asserts it)


def image(w, h, specials=SPECIALS, seed=0):
    """luminance log-uniform over 2^-10 .. 2^12 with tinted colours on the left two thirds -- neighbours many sigma apart: the edge stop closes, the fall-back of
    step 4 is taken --, two plateaus six stops apart with 0.3 stops of noise on the right third, and every 5th pixel with one channel special"""
    rng = np.random.default_rng(100 * w + h + seed)
    lum = np.exp2(rng.uniform(-10.0, 12.0, (h, w)))
    x0 = (2 * w) // 3
    lum[:, x0:] = np.exp2(np.where(np.arange(h)[:, None] < h // 2, -2.0, 4.0) + rng.normal(0.0, 0.3, (h, w - x0)))
    img = np.ones((h, w, 4), np.float32)
    img[..., :3] = (lum[..., None] * rng.uniform(0.5, 1.5, (h, w, 3))).astype(np.float32)
    flat = img.reshape(-1, 4)
    idx = np.arange(2, w * h, 5)
    flat[idx, rng.integers(0, 3, idx.size)] = np.array(specials, np.float32)[np.arange(idx.size) % len(specials)]
    return img


# ------------------------------------------------------------------ device plumbing
@pytest.fixture()
def lx(renderer):
    """the session's renderer, handed back with both switches off"""
    renderer.clear_local_exposure()
    renderer.clear_auto_exposure()
    yield renderer
    renderer.clear_local_exposure()
    renderer.clear_auto_exposure()


FILL = 0.25  # what the output buffer holds before the call: the never-written border must keep it


def _post(r, img, pp):
    """fh_post_process on an output buffer filled with FILL: (output, beauty_temp)"""
    from fredholm_amd.renderer import DeviceBuffer
    h, w = img.shape[:2]
    bufs = [DeviceBuffer(r, w * h * 16) for _ in range(4)]
    bufs[0].upload(img)
    bufs[1].clear()
    bufs[2].clear()
    bufs[3].upload(np.full((h, w, 4), FILL, np.float32))
    r.post_process(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, w, h, pp, bufs[3].ptr)
    r.wait_for_completion()
    out, tmp = bufs[3].download(np.float32, (h, w, 4)), bufs[2].download(np.float32, (h, w, 4))
    for b in bufs:
        b.free()
    return out, tmp


def _written(w, h):
    return (h // 16) * 16, (w // 16) * 16


def _check(oracle, out, tmp, img, p, exposure, ca, base_got):
    """the device's base and output against the float32 restatement; returns the restatement's diagnostics"""
    h, w = img.shape[:2]
    base, x, diag = local_gain(Ops32(oracle), img, p, exposure)
    assert base_got.shape == base.shape == ((h + 3) // 4, (w + 3) // 4)
    assert np.array_equal(_bits(base_got), _bits(base)), np.argwhere(_bits(base_got) != _bits(base))[:4]
    gh, gw = _written(w, h)
    want = tone_map(oracle, tmp, x, ca)
    ok = same_bits(out[:gh, :gw, :3], want[:gh, :gw])
    assert ok.all(), (np.argwhere(~ok)[:4], out[:gh, :gw, :3][~ok][:4], want[:gh, :gw][~ok][:4])
    assert (out[:gh, :gw, 3] == 1).all()
    assert (out[gh:] == FILL).all() and (out[:, gw:] == FILL).all()  # the never-written border
    return diag


def _pp(use_bloom=False, ca=0.0, iso=80.0):
    import fredholm_amd as F
    return F.PostProcessParams(use_bloom=use_bloom, bloom_threshold=2.0, bloom_sigma=5.0, ISO=iso, chromatic_aberration=ca)


# ------------------------------------------------------------------ 1. bit for bit against the float32 restatement
@pytest.mark.gpu
@pytest.mark.parametrize("which", list(PARAMS))
@pytest.mark.parametrize("w,h", FRAMES)
def test_base_and_output_equal_the_restatement_bit_for_bit(lx, oracle, w, h, which):
    p = PARAMS[which]
    img = image(w, h)
    lx.set_local_exposure(**p)
    out, tmp = _post(lx, img, _pp())
    gh, gw = _written(w, h)
    assert same_bits(tmp[:gh, :gw], img[:gh, :gw]).all()  # (no bloom: the tone map's input is the copy)
    diag = _check(oracle, out, tmp, img, p, iso_exposure(oracle, 80.0), 0.0, lx.local_exposure_base())
    if (w, h) == (70, 45):
        assert which == "six-pass" or diag["fell_back"].any()  # both branches of step 4 (at sigma_range = 4 no pixel is far enough from its four taps)
        assert not diag["fell_back"].all()
        assert (diag["raw"] > 0).any() and (diag["raw"] < 0).any()      # both shares of step 5
        if which == "six-pass":
            assert (np.abs(diag["raw"]) > f32(p["max_stops"])).any() and (np.abs(diag["raw"]) < f32(p["max_stops"])).any()  # max_stops binds, and not everywhere
    if (w, h) == (19, 17) and p["passes"] >= 3:
        assert 2 * (1 << (p["passes"] - 1)) >= max((w + 3) // 4, (h + 3) // 4)  # the outer taps of the last pass are all clamped


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["bloom", "bloom-ca", "ca", "auto", "auto-bloom-ca", "auto-black"])
def test_chain_variants_equal_the_restatement_bit_for_bit(lx, oracle, variant):
    import math
    import test_gpu_auto_exposure as A
    w, h = 70, 45
    bloom, ca, auto = "bloom" in variant, (1.5 if "ca" in variant else 0.0), "auto" in variant
    img = np.zeros((h, w, 4), np.float32) if variant == "auto-black" else image(w, h, MILD_SPECIALS if bloom else SPECIALS, seed=1)
    p = PARAMS["six-pass"] if variant in ("bloom-ca", "auto") else PARAMS["defaults"]
    pp = _pp(bloom, ca)
    exposure = iso_exposure(oracle, 80.0)
    if auto:
        ap = A.params(frame_time=math.inf)
        lx.set_auto_exposure(**ap)
    off, tmp_off = _post(lx, img, pp)
    if auto:
        lx.auto_exposure_reset()
    lx.set_local_exposure(**p)
    out, tmp = _post(lx, img, pp)
    assert same_bits(tmp, tmp_off).all()  # bloom, its threshold and the copy are untouched
    if auto:
        state = lx.auto_exposure_state()
        if variant == "auto-black":
            assert state["frames"] == 0  # nothing metered: the ISO exposure is used
        else:
            assert A._same_state(state, A.resolve(oracle, A.histogram(oracle, img, ap), ap, None)) and abs(state["ev"]) > 0.5
            exposure = A.exposure_of(oracle, state["ev"])
    _check(oracle, out, tmp, img, p, exposure, ca, lx.local_exposure_base())
    gh, gw = _written(w, h)
    if variant != "auto-black":
        assert not same_bits(out[:gh, :gw], off[:gh, :gw]).all()  # (the switch does something on this image)


# ------------------------------------------------------------------ 2. the chain against itself
@pytest.mark.gpu
@pytest.mark.parametrize("auto", [False, True])
def test_zero_shares_or_zero_max_stops_give_the_bits_of_the_switched_off_call(lx, auto):
    import math
    w, h = 70, 45
    img = image(w, h, seed=2)
    pp = _pp(False, 1.0)
    if auto:
        lx.set_auto_exposure(frame_time=math.inf)
    off, _ = _post(lx, img, pp)
    for kw in (dict(highlights=0.0, shadows=0.0), dict(max_stops=0.0), dict(highlights=0.0, shadows=0.0, max_stops=0.0, passes=1, sigma_range=0.25)):
        lx.set_local_exposure(**params(**kw))
        on, _ = _post(lx, img, pp)
        assert same_bits(on, off).all(), kw
    lx.set_local_exposure()
    on, _ = _post(lx, img, pp)
    gh, gw = _written(w, h)
    assert not same_bits(on[:gh, :gw], off[:gh, :gw]).all()


# ------------------------------------------------------------------ 3. a constant image
@pytest.mark.gpu
def test_a_constant_image_gets_one_gain_and_the_plain_bits_return_with_the_switch_off(lx, oracle):
    w, h = 64, 48
    img = np.tile(np.array([1.6, 1.0, 0.6, 1.0], np.float32), (h, w, 1))
    pp = _pp()
    plain, _ = _post(lx, img, pp)
    lx.set_local_exposure()
    out, tmp = _post(lx, img, pp)
    diag = _check(oracle, out, tmp, img, DEFAULTS, iso_exposure(oracle, 80.0), 0.0, lx.local_exposure_base())
    base = lx.local_exposure_base()
    assert np.unique(_bits(base)).size == 1 and abs(float(base[0, 0]) - float(diag["L"][0, 0])) <= 4 * 2.0 ** -24  # whole blocks: every pixel runs the same sums
    gh, gw = _written(w, h)
    # one gain up to the roundings of step 4, whose bilinear weights differ between the 16 phases of a pixel in its block: a few ulp
    assert all(np.ptp(out[:gh, :gw, k]) <= 8 * 2.0 ** -24 for k in range(3)) and np.ptp(diag["B"]) <= 4 * 2.0 ** -24
    assert (out[:gh, :gw, :3] < plain[:gh, :gw, :3]).all()  # brighter than the pivot: pulled down
    lx.clear_local_exposure()
    again, _ = _post(lx, img, pp)
    assert np.array_equal(_bits(again), _bits(plain))


# ------------------------------------------------------------------ 4. refusals on a live context
@pytest.mark.gpu
def test_refusals_leave_the_switch_and_the_parameters_alone(lx):
    import fredholm_amd as F
    from fredholm_amd import native as N
    from fredholm_amd.renderer import DeviceBuffer
    E = F.native.FredholmError
    assert lx.get_local_exposure()[0] is False
    buf = DeviceBuffer(lx, 16 * 16 * 16)
    buf.clear()
    with pytest.raises(E, match="local exposure is off"):
        lx.local_exposure_analyse(buf.ptr, 16, 16)
    with pytest.raises(E, match="local exposure is off"):
        lx.local_exposure_base()
    lx.set_local_exposure(highlights=0.75, passes=2)
    par = lx.get_local_exposure()
    assert par[0] is True and par[1]["highlights"] == 0.75 and par[1]["passes"] == 2
    assert lx.local_exposure_base().size == 0  # nothing analysed yet
    for bad in (dict(highlights=1.5), dict(shadows=-0.1), dict(pivot=0.0), dict(max_stops=float("nan")), dict(sigma_range=0.0), dict(passes=0), dict(passes=7)):
        with pytest.raises(E):
            lx.set_local_exposure(**bad)
    assert lx.get_local_exposure() == par
    for args in ((0, 16, 16), (buf.ptr, 0, 16), (buf.ptr, 16, 0), (buf.ptr, 32769, 1), (buf.ptr, 1, 32769)):
        with pytest.raises(E, match="1 .. 32768"):
            lx.local_exposure_analyse(*args)
    lx.local_exposure_analyse(buf.ptr, 16, 16)
    assert lx.local_exposure_base().shape == (4, 4)
    w4, h4 = C.c_uint32(9), C.c_uint32(9)
    assert N.lib().fh_get_local_exposure_base(lx._ctx, None, C.byref(w4), C.byref(h4)) == N.FH_OK and (w4.value, h4.value) == (4, 4)  # NULL: the size alone
    buf.free()
    lx.clear_local_exposure()
    assert lx.get_local_exposure() == (False, par[1])


# ------------------------------------------------------------------ 5. size changes, a group, allocations
@pytest.mark.gpu
def test_calls_at_changing_sizes_each_equal_the_restatement(lx, oracle):
    p = PARAMS["defaults"]
    lx.set_local_exposure(**p)
    for w, h in ((16, 16), (70, 45), (19, 17), (64, 48), (70, 45)):  # grows, shrinks, grows again: the images are kept and re-used
        img = image(w, h, seed=3)
        out, tmp = _post(lx, img, _pp())
        _check(oracle, out, tmp, img, p, iso_exposure(oracle, 80.0), 0.0, lx.local_exposure_base())


@pytest.mark.gpu
def test_a_group_of_two_members_on_one_device_gives_the_plain_contexts_bits(lx):
    import fredholm_amd as F
    w, h = 70, 45
    img = image(w, h, seed=4)
    pp = _pp(False, 1.0)
    lx.set_local_exposure(**PARAMS["one-pass"])
    plain, _ = _post(lx, img, pp)
    plain_base = lx.local_exposure_base()
    g = F.Renderer(devices=[0, 0])
    try:
        assert g.group_size == 2 and g.get_local_exposure()[0] is False
        g.set_local_exposure(**PARAMS["one-pass"])
        assert g.get_local_exposure()[0] is True
        out, _ = _post(g, img, pp)
        assert same_bits(out, plain).all() and np.array_equal(_bits(g.local_exposure_base()), _bits(plain_base))
    finally:
        g.close()


@pytest.mark.gpu
def test_what_the_feature_allocates_goes_with_the_context():
    import fredholm_amd as F
    from fredholm_amd import native as N

    def live():
        count, nbytes = C.c_uint64(0), C.c_uint64(0)
        assert N.lib().fh_kat_live_allocations(C.byref(count), C.byref(nbytes)) == N.FH_OK
        return int(count.value), int(nbytes.value)
    before = live()
    r = F.Renderer(0)
    try:
        created = live()
        assert r.get_local_exposure() == (False, {k: pytest.approx(v) for k, v in DEFAULTS.items()})  # the defaults before any set
        r.set_local_exposure()
        for w, h in ((64, 48), (70, 45)):
            _post(r, image(w, h), _pp())
        used = live()
        assert used[0] >= created[0] + 3 and used[1] >= created[1] + 4 * (70 * 45 + 2 * 18 * 12)  # the log image and the two quarter images
        r.clear_local_exposure()
        assert live() == used  # kept for the next switch-on
    finally:
        r.close()
    assert live() == before
