#!/usr/bin/env python3
"""tools/adaptive_bench.py [--out profiles/X.json] [--configs 2 3] [--spp 1024] [--threshold 0.05] [--truth-spp 4096] [--block 1 2 4 8] [--growth 1 2] -- what adaptive
sampling costs and what it buys.

Overhead: the same frame (BASELINE.json configs[c] scene at 1920x1080, `--spp` samples per frame, init_render_states before each) rendered plain and in adaptive
mode at threshold 0, where every pixel stays active to the cap: the difference is the machinery (a selection per round of `step` samples, the moments in the
accumulate, the rounds' host read-back).  Also the latency of 1-sample calls, the GUI's pattern (median of fh_render(1) + fh_sync).  The path pools are sized
as bench.py sizes them.

Benefit (configs[3] only): adaptive at `--threshold` (min_samples 64, step 16, cap `--spp`) against a plain render at the adaptive run's mean spp, both timed,
and the error of both against a `--truth-spp` plain render: mean over pixels of ((y - y_truth) / max(y_truth, floor))^2 of the beauty luminance.

`--block` / `--growth` (fh_set_adaptive_policy; default 1 / 1, the per-pixel rule with a boundary at every step): with more than the default given, the record also
holds `overhead_by_policy` (the threshold-0 frame for blocks 1 and 4 of those given x every growth: time, overhead against the plain frame of the same run, the
rounds of the schedule and the passes the library ran) and, for configs[3], `benefit_by_policy` (the benefit figures for every block x growth; "b1_g1" is the
per-pixel rule and the yardstick of the others).
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lum(b):
    b = b.astype(np.float64)
    return b[..., 0] * 0.2126729 + b[..., 1] * 0.7151522 + b[..., 2] * 0.0721750


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--floor", type=float, default=0.01)
    ap.add_argument("--truth-spp", type=int, default=4096)
    ap.add_argument("--latency-calls", type=int, default=100)
    ap.add_argument("--block", type=int, nargs="+", default=[1])
    ap.add_argument("--growth", type=int, nargs="+", default=[1])
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch

    import bench
    import fredholm_amd as F

    rec = {"spp": a.spp, "frames": a.frames, "source_fingerprint": bench.source_fingerprint(), "configs": {}}
    tmp = tempfile.mkdtemp()
    for cfg in a.configs:
        w = bench.workload(cfg, tmp)
        W, H, D = w["width"], w["height"], w["depth"]
        r = F.Renderer(0)
        r.load_scene(w["scene"])
        r.build_ias()
        bench.apply_environment(r, w)
        r.set_resolution(W, H)
        cam = F.Camera(**w["camera"])
        layers = F.RenderLayer(r, W, H)
        n_owned = r.owned_pixel_count()
        pool_spp, _, _ = bench.pass_size(r, torch, 0, n_owned, a.spp)
        r.set_path_pool(max(int(n_owned * pool_spp), 1))

        def frame(calls, adaptive=None, policy=(1, 1)):
            r.wait_for_completion()
            r.init_render_states()
            layers.clear()
            r.set_adaptive_policy(*policy)
            if adaptive is None:
                r.clear_adaptive_sampling()
            else:
                r.set_adaptive_sampling(*adaptive)
            r.wait_for_completion()
            t0 = time.perf_counter()
            for n in calls:
                r.render(cam, w["bg"], layers, n, D)
            r.wait_for_completion()
            return time.perf_counter() - t0

        def timed(calls, adaptive=None, policy=(1, 1)):
            frame(calls, adaptive, policy)  # (warm-up: pools, lists)
            return sorted(frame(calls, adaptive, policy) for _ in range(a.frames))[a.frames // 2] * 1e3

        def rounds(growth, min_samples=64, step=16):
            """the rounds of one call of --spp samples: growth 1 ends one at every multiple of step, growth 2 at b0 * 2^k"""
            if growth == 1:
                return -(-a.spp // step)
            n, t, b = 0, 0, -(-min_samples // step) * step
            while t < a.spp:
                t, b, n = b, 2 * b, n + 1
            return n

        def benefit(truth, policy):
            t_ad = frame([a.spp], (a.threshold, 64, 16, a.floor), policy) * 1e3
            y_ad = lum(layers.download("beauty"))
            counts = r.sample_counts()
            mean_spp = float(counts.mean())
            n_u = max(1, int(round(mean_spp)))
            t_u = frame([n_u]) * 1e3
            y_u = lum(layers.download("beauty"))
            ref = np.maximum(truth, a.floor)
            return {"threshold": a.threshold, "floor": a.floor, "min_samples": 64, "step": 16, "cap": a.spp, "truth_spp": a.truth_spp, "block": policy[0], "growth": policy[1],
                    "adaptive_ms": t_ad, "adaptive_mean_spp": mean_spp, "stopped_before_cap": float((counts < a.spp).mean()),
                    "plain_ms_at_mean_spp": t_u, "plain_spp": n_u,
                    "rel_sq_error_adaptive": float(np.mean(((y_ad - truth) / ref) ** 2)), "rel_sq_error_plain": float(np.mean(((y_u - truth) / ref) ** 2))}

        def latency(adaptive=None):
            frame([1] * 20, adaptive)
            ts = []
            for _ in range(a.latency_calls):
                t0 = time.perf_counter()
                r.render(cam, w["bg"], layers, 1, D)
                r.wait_for_completion()
                ts.append(time.perf_counter() - t0)
            return float(np.median(ts)) * 1e3

        c = {"workload": w["name"], "frame_ms_plain": timed([a.spp])}
        c["frame_ms_adaptive_threshold0"] = timed([a.spp], (0.0, 64, 16, a.floor))
        c["overhead"] = c["frame_ms_adaptive_threshold0"] / c["frame_ms_plain"] - 1.0
        c["spp1_ms_plain"] = latency()
        c["spp1_ms_adaptive_threshold0"] = latency((0.0, 64, 16, a.floor))
        c["spp1_delta_ms"] = c["spp1_ms_adaptive_threshold0"] - c["spp1_ms_plain"]
        policies = [(b, g) for b in a.block for g in a.growth]
        if policies != [(1, 1)]:
            c["overhead_by_policy"] = {}
            for b, g in policies:
                if b not in (1, 4):
                    continue
                r.reset_stats()
                ms = timed([a.spp], (0.0, 64, 16, a.floor), (b, g))
                c["overhead_by_policy"][f"b{b}_g{g}"] = {"frame_ms": ms, "overhead": ms / c["frame_ms_plain"] - 1.0, "rounds": rounds(g),
                                                         "passes_per_frame": r.stats()["n_passes"] // (a.frames + 1)}
        if cfg == 3:
            frame([a.truth_spp])
            truth = lum(layers.download("beauty"))
            c["benefit"] = benefit(truth, (1, 1))
            if policies != [(1, 1)]:
                c["benefit_by_policy"] = {f"b{b}_g{g}": (c["benefit"] if (b, g) == (1, 1) else benefit(truth, (b, g))) for b, g in policies}
        rec["configs"][str(cfg)] = c
        r.close()
        print(json.dumps({cfg: c}), file=sys.stderr, flush=True)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
