#!/usr/bin/env python3
"""tools/denoise_bench.py [--out profiles/denoise_guided_bench.json] [--config 3] [--spp 16] [--calls 20] [--temporal] -- what a call of the denoisers costs.

The layers of a BASELINE.json configs[c] frame at 1920x1080 (`--spp` samples, adaptive sampling on at threshold 0 so that the luminance moments exist), then, in this
one process, the median of `--calls` calls of fh_denoise and of fh_denoise_guided, each followed by one fh_sync and timed from before the call to after the sync:
the guided filter with every guide (position, depth, moments, counts), without the moments (the 7x7 spatial variance estimate runs instead) and without position
and depth.  Prints one JSON line (and writes it to --out).

--temporal (-> profiles/denoise_temporal_bench.json): instead, two such frames with seeds 1 and 2 from cameras a small step apart (--step, as a fraction of the camera's
distance from the origin), and the median of `--calls` calls of fh_denoise_temporal that alternate between the two frames -- every call reprojects the other frame's
history --, of calls that repeat one frame (the still-camera kernel), and of fh_denoise_guided on the same layers in the same process.  The stage's share is the
difference of the medians; the kernel's own time comes from running this under `rocprofv3 --kernel-trace --stats` (k_temporal)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(r, call, calls):
    for _ in range(4):  # (warm-up: scratch allocation, code objects; an even number, so that alternating calls go on alternating)
        call()
        r.wait_for_completion()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        call()
        r.wait_for_completion()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def temporal(a, bench, F, DeviceBuffer, r, w):
    W, H = w["width"], w["height"]
    o = np.asarray(w["camera"]["origin"], np.float64)
    step = a.step * max(float(np.linalg.norm(o)), 1.0)
    cams = [F.Camera(**w["camera"]), F.Camera(**dict(w["camera"], origin=tuple(o + np.array([step, 0.0, 0.0]))))]
    frames = []
    for k, cam in enumerate(cams):
        L = F.RenderLayer(r, W, H)
        r.init_render_states()
        r.seed = 1 + k
        r.render(cam, w["bg"], L, a.spp, w["depth"])
        m, c = DeviceBuffer(r, 8 * W * H), DeviceBuffer(r, 4 * W * H)
        r.get_luminance_moments(m.ptr)
        r.get_sample_counts(c.ptr)
        r.wait_for_completion()
        frames.append((cam, L.ptrs, m, c))
    out = DeviceBuffer(r, 16 * W * H)
    turn = [0]

    def call_temporal(alternate):
        cam, p, m, c = frames[turn[0] & 1 if alternate else 0]
        turn[0] += 1
        r.denoise_temporal(W, H, p["beauty"], p["normal"], p["albedo"], out.ptr, p["position"], p["depth"], cam, m.ptr, c.ptr)

    def call_guided():
        cam, p, m, c = frames[0]
        r.denoise_guided(W, H, p["beauty"], p["normal"], p["albedo"], out.ptr, p["position"], p["depth"], m.ptr, c.ptr)
    rec = {"workload": w["name"], "width": W, "height": H, "spp": a.spp, "calls": a.calls, "camera_step": step, "source_fingerprint": bench.source_fingerprint(),
           "fh_denoise_guided_ms": median_ms(r, call_guided, a.calls),
           "fh_denoise_temporal_moving_ms": median_ms(r, lambda: call_temporal(True), a.calls),
           "fh_denoise_temporal_still_ms": median_ms(r, lambda: call_temporal(False), a.calls),
           "fh_denoise_guided_again_ms": median_ms(r, call_guided, a.calls)}
    rec["stage_moving_ms_by_difference"] = rec["fh_denoise_temporal_moving_ms"] - rec["fh_denoise_guided_ms"]
    rec["stage_still_ms_by_difference"] = rec["fh_denoise_temporal_still_ms"] - rec["fh_denoise_guided_ms"]
    w_, h_, n_ = r.denoise_history_info()
    rec["history"] = [w_, h_, n_]
    r.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--temporal", action="store_true")
    ap.add_argument("--step", type=float, default=0.002)
    a = ap.parse_args()

    import bench
    import fredholm_amd as F
    from fredholm_amd.renderer import DeviceBuffer

    w = bench.workload(a.config, tempfile.mkdtemp())
    W, H = w["width"], w["height"]
    r = F.Renderer(0)
    r.load_scene(w["scene"])
    r.build_ias()
    bench.apply_environment(r, w)
    r.set_resolution(W, H)
    r.set_adaptive_sampling(0.0)
    if a.temporal:
        return temporal(a, bench, F, DeviceBuffer, r, w)
    L = F.RenderLayer(r, W, H)
    r.render(F.Camera(**w["camera"]), w["bg"], L, a.spp, w["depth"])
    moments, counts, out = DeviceBuffer(r, 8 * W * H), DeviceBuffer(r, 4 * W * H), DeviceBuffer(r, 16 * W * H)
    r.get_luminance_moments(moments.ptr)
    r.get_sample_counts(counts.ptr)
    r.wait_for_completion()
    p = L.ptrs

    def median_ms(call):
        for _ in range(3):  # (warm-up: scratch allocation, code objects)
            call()
            r.wait_for_completion()
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            call()
            r.wait_for_completion()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3

    rec = {"workload": w["name"], "width": W, "height": H, "spp": a.spp, "calls": a.calls, "source_fingerprint": bench.source_fingerprint(),
           "fh_denoise_ms": median_ms(lambda: r.denoise(W, H, p["beauty"], p["normal"], p["albedo"], out.ptr)),
           "fh_denoise_guided_ms": median_ms(lambda: r.denoise_guided(W, H, p["beauty"], p["normal"], p["albedo"], out.ptr, p["position"], p["depth"], moments.ptr, counts.ptr)),
           "fh_denoise_guided_no_moments_ms": median_ms(lambda: r.denoise_guided(W, H, p["beauty"], p["normal"], p["albedo"], out.ptr, p["position"], p["depth"])),
           "fh_denoise_guided_no_position_ms": median_ms(lambda: r.denoise_guided(W, H, p["beauty"], p["normal"], p["albedo"], out.ptr, None, None, moments.ptr, counts.ptr))}
    rec["guided_over_atrous"] = rec["fh_denoise_guided_ms"] / rec["fh_denoise_ms"]
    r.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
