#!/usr/bin/env python3
"""tools/group_bench.py [--out profiles/X.json] [--configs 1 3] [--spp 1 16 256] [--leg-timeout 600] -- what a group (fh_ctx_create_group) costs on ONE device.

Legs, each in a fresh process under a time limit: a plain context, the degenerate group [0] (a plain context through fh_ctx_create_group), and the group [0, 0] with
the gather mask at all six layers and at beauty only.  Scenes: BASELINE.json configs[1] and configs[3] at 1920x1080.  Per leg and samples per call: the median ms of
fh_render(n) + fh_sync over an accumulating frame, and, from HIP events in a second short run with FH_FLAG_TIME_KERNELS, the time of k_pack_layers, of the copy and
of k_unpack_group.  On one GPU a group cannot be faster than a plain context: the legs price the gather (174 MB of layers per call at 1080p with all six, 33 MB with
beauty) and the fixed per-pass cost each member pays.  Speed-up over distinct devices is not measured here.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = {"plain": (None, 63), "group_0": ([0], 63), "group_0_0_all": ([0, 0], 63), "group_0_0_beauty": ([0, 0], 1)}
CALLS = {1: 40, 16: 12, 256: 3}


def leg(cfg, name, spps):
    import numpy as np
    import torch

    import bench
    import fredholm_amd as F
    from fredholm_amd import native as N

    devices, mask = LEGS[name]
    w = bench.workload(cfg, tempfile.mkdtemp())
    W, H, D = w["width"], w["height"], w["depth"]
    r = F.Renderer(0) if devices is None else F.Renderer(devices=devices)
    r.set_gather_layers(mask)
    r.load_scene(w["scene"])
    r.build_ias()
    bench.apply_environment(r, w)
    r.set_resolution(W, H)
    cam = F.Camera(**w["camera"])
    layers = F.RenderLayer(r, W, H)
    pool_spp, _, _ = bench.pass_size(r, torch, 0, W * H, max(spps))
    r.set_path_pool(max(int(W * H * pool_spp) // r.group_size, 1))  # (the target is per member: the members of one device share the budget)
    out = {"members": r.group_size, "gather_mask": mask, "spp": {}}
    for n in spps:
        def frame(calls, flags):
            r.wait_for_completion()
            r.set_flags(flags)
            r.init_render_states()
            layers.clear()
            r.wait_for_completion()
            ts, gather = [], []
            for _ in range(calls):
                t0 = time.perf_counter()
                r.render(cam, w["bg"], layers, n, D)
                r.wait_for_completion()
                ts.append((time.perf_counter() - t0) * 1e3)
                if flags:
                    gather.append(r.gather_times())
            return ts, gather

        frame(min(CALLS.get(n, 3), 4), 0)  # (warm-up: pools, lists)
        ts, _ = frame(CALLS.get(n, 3), 0)
        _, g = frame(min(CALLS.get(n, 3), 5), N.FLAG_TIME_KERNELS)
        g = np.median(np.asarray(g), axis=0)
        out["spp"][str(n)] = {"ms_per_call": float(np.median(ts)), "ms_per_call_min": float(np.min(ts)), "calls": len(ts),
                              "k_pack_layers_ms": float(g[0]), "copy_ms": float(g[1]), "k_unpack_group_ms": float(g[2])}
    out["n_passes_total"] = r.stats()["n_passes"]  # (all frames of the leg: a group of two submits twice the passes)
    layers.free()
    r.close()
    print("LEG " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--spp", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--leg-timeout", type=float, default=600.0)
    ap.add_argument("--leg", nargs=2, metavar=("CONFIG", "NAME"), default=None, help="(internal) run one leg in this process")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.leg:
        leg(int(a.leg[0]), a.leg[1], a.spp)
        return
    import bench
    rec = {"width": 1920, "height": 1080, "devices_used": 1, "source_fingerprint": bench.source_fingerprint(), "configs": {}}
    for cfg in a.configs:
        rec["configs"][str(cfg)] = {}
        for name in LEGS:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", str(cfg), name, "--spp", *map(str, a.spp)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.leg_timeout)  # a fresh process per leg, under its own time limit
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("LEG ")]
            if p.returncode != 0 or not lines:  # nothing more is started on the GPU after a leg that failed
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"leg {name} of configs[{cfg}] failed with exit status {p.returncode}")
            rec["configs"][str(cfg)][name] = json.loads(lines[-1][4:])
            print(json.dumps({str(cfg): {name: rec["configs"][str(cfg)][name]}}), file=sys.stderr, flush=True)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
