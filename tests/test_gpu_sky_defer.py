"""The deferred mode of the sky and light slots (render.hip: shade_hit<..., DEFER>, SecondaryStream<..., DEFER>, k_sky_resolve; render_plan_host.h: sky_defer_verdict).

Shadow rays of the sky-NEE slot and of the BSDF-sampled light slot carry their WEIGHT, the secondary-ray kernel leaves one byte per queue entry that says which slots
escaped, and k_sky_resolve evaluates the environment for those alone and adds their contributions in slot order.  Same functions, same operands, same order of additions:
FH_SKY_DEFER=1 against =0 has to match bit for bit on every layer and on the sample counts, and the beauty layer has to match the CPU checker by the parity rule of
tests/test_gpu_parity.py (99.9 % of the pixels bit-identical, per-pixel L2 <= 1e-5 of the image mean).

Every GPU case: FH_STREAM=1 (a small tree runs the streaming kernels), 80 x 60, depth 5 with every bounce a wavefront bounce, a pool of two samples per pixel and two
launches of four samples, so that every call has two passes (no merged launch)."""
import os
import subprocess

import numpy as np
import pytest

import fredholm_amd as F
from fredholm_amd import scenes
from test_gpu_parity import _fence_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, DEPTH, LAUNCHES, SPP = 80, 60, 5, 2, 4
BELOW = dict(origin=(0.0, -2.6, 1.5), forward=(0.0, 0.866, -0.5), fov=np.radians(60.0), F=100.0, focus=10000.0)  # (the below-horizon camera of test_gpu_parity.py)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _hosek(x):
    x.load_arhosek_sky(3.0, 0.3)


def _hosek_and_directional(x):
    x.load_arhosek_sky(3.0, 0.3)
    x.set_directional_light((3.0, 2.5, 2.0), (0.3, 1.0, 0.8), 2.0)


def _small_ibl(x):
    x.load_ibl(scenes.gradient_ibl(8, 4))


def _soup():
    return scenes.triangle_soup(20000, 0.1)


def _dark_fence():
    sc = dict(_fence_scene())
    sc["materials"] = sc["materials"].copy()
    sc["materials"]["emission"][:] = 0.0
    sc["materials"]["emission_color"][:] = 0.0
    sc["materials"]["emission_texture_id"][:] = -1  # (a material with an emission texture is an emitter whatever its constants say: scene_plan_host.h, material_emissive)
    return sc


def _half_black_soup():
    sc = dict(_soup())
    m = sc["materials"] = sc["materials"].copy()
    for i in range(m.shape[0]):
        if i % 2 == 0:  # black and non-specular: every weight out of such a surface is exactly zero
            m["base_color"][i] = (0.0, 0.0, 0.0)
            m["specular"][i] = 0.0
        else:
            m["base_color"][i] = (1.0, 1.0, 1.0)
    return sc


CASES = {
    "hosek": (_soup, scenes.SOUP_CAMERA, _hosek),
    "hosek_below_horizon": (_soup, BELOW, _hosek),
    "hosek_directional": (_soup, scenes.SOUP_CAMERA, _hosek_and_directional),
    "ibl_8x4": (_soup, scenes.SOUP_CAMERA, _small_ibl),
    "cut_outs_dark": (_dark_fence, scenes.CORNELL_CAMERA, _hosek),
    "half_black_below_horizon": (_half_black_soup, BELOW, _hosek),
}


def _render(monkeypatch, defer, sc, cam, setup, bg=(0.0, 0.0, 0.0), flags=0, env=None, eligible=None):
    """all layers, the sample counts and the stats of LAUNCHES calls in a fresh context created under FH_SKY_DEFER=defer (and `env`).
    FH_DEBUG_TAIL=1 makes every call that launched k_sky_resolve print the resolve's list lengths to stderr (a [sky-resolve] line; the switch only adds a wait at the
    end of the call): the callers read it with capfd, so that a comparison of a path with itself cannot pass for one of the two modes.
    eligible: whether the scene is one the mode applies to -- such a scene has no emitter."""
    env = dict(env or {}, FH_STREAM="1", FH_SKY_DEFER=defer, FH_DEBUG_TAIL="1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = F.Renderer(0)
    for k in env:
        monkeypatch.delenv(k)
    r.set_path_pool(W * H * 2)
    r.load_scene(sc)
    r.build_ias()
    if setup:
        setup(r)
    if eligible is not None:
        assert (r.n_lights() == 0) == eligible, r.n_lights()
    r.set_resolution(W, H)
    r.set_tail_depth(DEPTH)
    if flags:
        r.set_flags(flags)
    L = F.RenderLayer(r, W, H)
    for _ in range(LAUNCHES):
        r.render(F.Camera(**cam), bg, L, SPP, DEPTH)
    r.wait_for_completion()
    out = {n: L.download(n) for n in F.RenderLayer.NAMES}
    out["sample_count"] = np.asarray(r.sample_counts())
    st = r.stats()
    r.close()
    return out, st


def _resolve_calls(capfd):
    """calls since the last look whose passes launched k_sky_resolve over a non-empty queue"""
    return capfd.readouterr().err.count("[sky-resolve]")


def _assert_same_bits(a, b):
    assert len(F.RenderLayer.NAMES) == 6
    for name in list(F.RenderLayer.NAMES):
        same = (_bits(a[name]) == _bits(b[name])) | (np.isnan(a[name]) & np.isnan(b[name]))
        assert same.all(), f"{name}: {int((~same).sum())} values differ"
    assert np.array_equal(a["sample_count"], b["sample_count"])


def _assert_image_parity(gpu, ref):
    same = ((_bits(gpu) == _bits(ref)) | (np.isnan(gpu) & np.isnan(ref))).reshape(-1, gpu.shape[-1]).all(axis=1).mean()
    assert same >= 0.999, f"only {same:.5f} of the pixels are bit-identical"
    l2 = np.sqrt(((gpu[..., :3].astype(np.float64) - ref[..., :3]) ** 2).mean(axis=2))
    assert l2.max() <= 1e-5 * max(float(ref[..., :3].mean()), 1e-6) or same == 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_deferred_sky_radiance_keeps_every_bit(oracle, monkeypatch, capfd, case):
    make, cam, setup = CASES[case]
    sc = make()
    _resolve_calls(capfd)
    on, st_on = _render(monkeypatch, "1", sc, cam, setup, eligible=True)
    assert _resolve_calls(capfd) == LAUNCHES  # the deferred kernels ran, in every call
    off, st_off = _render(monkeypatch, "0", sc, cam, setup, eligible=True)
    assert _resolve_calls(capfd) == 0
    assert st_on["n_passes"] == st_off["n_passes"] == 2 * LAUNCHES  # (several passes per call: the secondary launches are the streaming kernel's own)
    _assert_same_bits(on, off)
    S = oracle.Scene(sc)
    setup(S)
    Lo = S.new_layers(W, H)
    for _ in range(LAUNCHES * SPP):
        S.render(F.Camera(**cam).params(), W, H, Lo, 1, DEPTH, bg=(0.0, 0.0, 0.0), n_threads=8)
    _assert_image_parity(on["beauty"], Lo["beauty"])
    assert np.isfinite(on["beauty"]).all()
    if case == "half_black_below_horizon":  # weights of exactly zero on paths that carry radiance already, NaN radiance below the horizon: the frame is not all black
        assert on["beauty"][..., :3].max() > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["constant_grey", "emitters"])
def test_switch_changes_nothing_where_the_mode_does_not_apply(monkeypatch, capfd, scene):
    """a constant background keeps its zero-contribution pruning and a scene with emitters its own light-ray kernels: same bits, same shadow rays, same shade launches"""
    sc, cam, bg = (_soup(), scenes.SOUP_CAMERA, (0.5, 0.5, 0.5)) if scene == "constant_grey" else (scenes.cornell_box(), scenes.CORNELL_CAMERA, (0.0, 0.0, 0.0))
    _resolve_calls(capfd)
    on, st_on = _render(monkeypatch, "1", sc, cam, None, bg=bg, flags=2, eligible=scene == "constant_grey")  # FH_FLAG_COUNT_TRAVERSAL
    off, st_off = _render(monkeypatch, "0", sc, cam, None, bg=bg, flags=2)
    assert _resolve_calls(capfd) == 0  # (no resolve launch in either)
    _assert_same_bits(on, off)
    assert st_on["rays_shadow"] == st_off["rays_shadow"] and st_on["rays_shadow"] > 0
    assert st_on["n_shade_launches"] == st_off["n_shade_launches"]


@pytest.mark.gpu
def test_counting_kernels_count_the_same_rays(monkeypatch, capfd):
    """FH_FLAG_COUNT_TRAVERSAL on the plain Hosek soup: the deferred forms of the counting kernels trace the same rays through the same nodes and triangles.

    FH_COOP_T=1 (a cooperative test round as soon as one candidate is queued) makes the two sums functions of the rays.  At the default threshold a first-hit ray walks
    on until its WAVE has queued enough candidates, so how many nodes it visits depends on the rays beside it -- on the order the shade kernels' atomics gave the queue
    and on which wave drew which chunk -- and the sums differ from run to run of the SAME kernel: measured with this setup on one MI355X, nodes_shadow / tris_shadow of
    three FH_SKY_DEFER=0 runs 172197 / 96518, 172105 / 96428, 172065 / 96476 and of three =1 runs 172144 / 96450, 172087 / 96460, 172018 / 96372 (rays_shadow 14636 in
    all six).  With the threshold at one, all six runs gave 14636 / 162647 / 87984.  rays_shadow, which is a function of the rays at any threshold, is compared at the
    default one as well."""
    sc = _soup()
    _resolve_calls(capfd)
    on, st_on = _render(monkeypatch, "1", sc, scenes.SOUP_CAMERA, _hosek, flags=2, env={"FH_COOP_T": "1"}, eligible=True)
    assert _resolve_calls(capfd) == LAUNCHES
    off, st_off = _render(monkeypatch, "0", sc, scenes.SOUP_CAMERA, _hosek, flags=2, env={"FH_COOP_T": "1"}, eligible=True)
    _assert_same_bits(on, off)
    on_d, st_on_d = _render(monkeypatch, "1", sc, scenes.SOUP_CAMERA, _hosek, flags=2, eligible=True)
    off_d, st_off_d = _render(monkeypatch, "0", sc, scenes.SOUP_CAMERA, _hosek, flags=2, eligible=True)
    _assert_same_bits(on_d, off_d)
    _assert_same_bits(on_d, on)
    assert st_on_d["rays_shadow"] == st_off_d["rays_shadow"] == st_on["rays_shadow"]
    print("FH_SKY_DEFER=1 / =0:", {k: (st_on[k], st_off[k]) for k in ("rays_shadow", "nodes_shadow", "tris_shadow")})
    for key in ("rays_shadow", "nodes_shadow", "tris_shadow"):
        assert st_on[key] == st_off[key] and st_on[key] > 0, (key, st_on[key], st_off[key])


def test_host_verdict_truth_table(tmp_path):
    """render_plan_host.h: sky_defer_verdict, compiled into tools/sky_defer_check.cpp and run over every input (no GPU)"""
    exe = tmp_path / "sky_defer_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tools", "sky_defer_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "sky_defer_check: ok (2048 cases)" in run.stdout, run.stdout
