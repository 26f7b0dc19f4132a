#!/usr/bin/env python3
"""tools/denoise_bench.py [--out profiles/denoise_guided_bench.json] [--config 3] [--spp 16] [--calls 20] -- what a call of the two denoisers costs.

The layers of a BASELINE.json configs[c] frame at 1920x1080 (`--spp` samples, adaptive sampling on at threshold 0 so that the luminance moments exist), then, in this
one process, the median of `--calls` calls of fh_denoise and of fh_denoise_guided, each followed by one fh_sync and timed from before the call to after the sync:
the guided filter with every guide (position, depth, moments, counts), without the moments (the 7x7 spatial variance estimate runs instead) and without position
and depth.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default="")
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
