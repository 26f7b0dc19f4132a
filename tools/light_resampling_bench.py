#!/usr/bin/env python3
"""tools/light_resampling_bench.py -- what resampling of the light table's picks (fh_set_light_resampling) costs and gains.

  leg    python3 tools/light_resampling_bench.py leg [--width 240 --height 135 --spp 16 --ref-spp 4096] --out FILE.json
         One process.  relMSE at equal samples on the lamp-lit interior (scenes_sponza with lamps=True: four lamps, 32 emitters of one emission, no sky, no sun) and on
         the model scene with the lamp 15 aside, for the modes off / table / resampled among 4, 8 and 16, against TWO references of `ref_spp` samples -- one rendered
         off and one with resampling (default M) on -- and of the two references against each other.  relMSE as tools/light_sampling_bench.py has it.  Frame times
         are wall clock of a synchronised call, median of five.
  trace  python3 tools/light_resampling_bench.py trace [--width 240 --height 135 --spp 16 --frames 8]
         One process: `frames` frames of the interior per mode, the modes separated by one launch of the pick hook (k_light_pick), the off frames last.  Run it under
             rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python3 tools/light_resampling_bench.py trace ...
         (no counters): NAME_kernel_trace.csv then holds every dispatch with its start and end.
  merge  python3 tools/light_resampling_bench.py merge --legs FILE.json --trace TRACE.csv --frames 8 [--resources FILE.json] [--bench FILE.json]
             --out profiles/light_resampling_bench.json   (no GPU)
         k_shade_lt (the k_shade<..., fh::LightTable> launches: kernel_families.py), k_tail_lt and all kernels together per frame and mode from the trace, cut at the separators.
"""
import argparse
import csv
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import light_sampling_bench as LB  # noqa: E402
from kernel_families import family  # noqa: E402

MS = (4, 8, 16)
MODES = ["table"] + ["resampled_%d" % m for m in MS] + ["off"]


def set_mode(r, mode):
    if mode == "off":
        r.clear_light_resampling()
        r.clear_light_sampling()
        return
    r.set_light_sampling()
    if mode == "table":
        r.clear_light_resampling()
    else:
        r.set_light_resampling(int(mode.split("_")[1]))


def measure(F, N, np, sc, cam, w, h, depth, spp, ref_spp):
    import statistics
    import time
    r = F.Renderer(0)
    r.load_scene(sc)
    r.build_ias()
    r.set_resolution(w, h)
    L = F.RenderLayer(r, w, h)

    def frame(n):
        r.init_render_states()
        t0 = time.perf_counter()
        r.render(cam, (0.0, 0.0, 0.0), L, n, depth)
        r.wait_for_completion()
        dt = time.perf_counter() - t0
        return L.download("beauty")[..., :3].astype(np.float64), dt
    rec = {"emitters": int(r.n_lights()), "width": w, "height": h, "max_depth": depth, "spp": spp,
           "references": f"{ref_spp} spp, one with the switches off, one with resampling among {N.LIGHT_CANDIDATES_DEFAULT} on", "modes": {}}
    set_mode(r, "off")
    ref_off = frame(ref_spp)[0]
    set_mode(r, "resampled_%d" % N.LIGHT_CANDIDATES_DEFAULT)
    ref_on = frame(ref_spp)[0]
    for mode in ["off", "table"] + ["resampled_%d" % m for m in MS]:
        set_mode(r, mode)
        frame(spp)
        runs = [frame(spp) for _ in range(5)]
        img = runs[-1][0]
        rec["modes"][mode] = {"relmse_against_reference_off": LB.relmse(img, ref_off), "relmse_against_reference_resampled": LB.relmse(img, ref_on),
                              "frame_ms": round(statistics.median(t for _, t in runs) * 1e3, 3)}
    r.close()
    rec["relmse_reference_off_against_reference_resampled"] = LB.relmse(ref_off, ref_on)
    rec["mean_reference_off"], rec["mean_reference_resampled"] = float(ref_off.mean()), float(ref_on.mean())
    off = rec["modes"]["off"]["relmse_against_reference_off"]
    rec["resampling_beats_off"] = {m: bool(v["relmse_against_reference_off"] < off) for m, v in rec["modes"].items() if m.startswith("resampled")}
    return rec


def leg(args):
    import numpy as np
    import fredholm_amd as F
    from fredholm_amd import native as N
    import light_resampling_scenes as RS
    import light_sampling_scenes as S
    from test_estimator_expectation import lens_at
    tmp = tempfile.mkdtemp(prefix="light_bench_")
    sc, camera, info = LB.interior(tmp)
    rec = {"frame_ms_source": "wall clock of fh_render + fh_sync, median of five", "default_candidates": N.LIGHT_CANDIDATES_DEFAULT}
    rec["interior"] = measure(F, N, np, sc, F.Camera(**camera), args.width, args.height, 8, args.spp, args.ref_spp)
    rec["interior"]["scene"] = f"scenes_sponza with lamps=True ({info['triangles']} triangles), lit by its four lamps alone"
    rec["model_scene_lamp_aside"] = measure(F, N, np, S.model_scene(quads=S.model_quads(RS.ASIDE)), lens_at((0.0, 4.0, 0.0)), 64, 48, 1, args.spp, args.ref_spp)
    rec["model_scene_lamp_aside"]["scene"] = "tests/light_sampling_scenes.py: model_scene(quads=model_quads(15))"
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def trace(args):
    import numpy as np
    import fredholm_amd as F
    from fredholm_amd import native as N
    tmp = tempfile.mkdtemp(prefix="light_bench_")
    sc, camera, _ = LB.interior(tmp)
    r = F.Renderer(0)
    r.load_scene(sc)
    r.build_ias()
    r.set_resolution(args.width, args.height)
    L = F.RenderLayer(r, args.width, args.height)
    cam = F.Camera(**camera)
    u1, k, p = np.full(1, 0.5, np.float32), np.zeros(1, np.uint32), np.zeros(1, np.float32)
    set_mode(r, "table")
    r.init_render_states()
    r.render(cam, (0.0, 0.0, 0.0), L, args.spp, 8)  # (warm-up: the table build, the pools)
    r.wait_for_completion()
    for mode in MODES:
        if mode == "off":  # the separator needs the table: launched before the switch goes off
            N.check(r._ctx, N.lib().fh_kat_light_pick(r._ctx, 1, N.ptr(u1), N.ptr(k), N.ptr(p)), "fh_kat_light_pick")
        set_mode(r, mode)
        if mode != "off":
            N.check(r._ctx, N.lib().fh_kat_light_pick(r._ctx, 1, N.ptr(u1), N.ptr(k), N.ptr(p)), "fh_kat_light_pick")
        for _ in range(args.frames):
            r.init_render_states()
            r.render(cam, (0.0, 0.0, 0.0), L, args.spp, 8)
            r.wait_for_completion()
    r.close()
    print(json.dumps({"frames_per_mode": args.frames, "modes": MODES, "spp": args.spp, "width": args.width, "height": args.height}))


def trace_segments(path, frames):
    rows = []
    for row in csv.DictReader(open(path)):
        rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"]), row["Kernel_Name"]))
    rows.sort()
    seg, out = -1, {}
    for _, dur, name in rows:
        if "k_light_pick" in name:
            seg += 1
            continue
        if seg < 0 or seg >= len(MODES):
            continue
        c = out.setdefault(MODES[seg], {"k_shade_lt_us_per_frame": 0.0, "k_tail_lt_us_per_frame": 0.0, "k_shade_us_per_frame": 0.0, "k_tail_us_per_frame": 0.0, "all_kernels_us_per_frame": 0.0})
        c["all_kernels_us_per_frame"] += dur / 1e3 / frames
        fam = family(name)  # (the forms with the light table count as k_shade_lt, k_tail_lt: kernel_families.py)
        if fam in ("k_shade_lt", "k_tail_lt", "k_shade", "k_tail"):
            c[fam + "_us_per_frame"] += dur / 1e3 / frames
    return {m: {k: round(v, 2) for k, v in c.items()} for m, c in out.items()}


def merge(args):
    rec = json.loads(open(args.legs).read())
    rec["kernels"] = trace_segments(args.trace, args.frames)
    rec["kernels_source"] = f"rocprofv3 --kernel-trace, no counters, one run of `trace`: {args.frames} frames of the interior per mode, cut at the separator launches; sums of the dispatches' durations per frame"
    if args.resources:
        rec["lt_twins_resources_parent_and_this"] = json.load(open(args.resources))
    if args.bench:
        rec["bench_switches_off"] = json.load(open(args.bench))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec)[:3000])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["leg", "trace", "merge"])
    ap.add_argument("--width", type=int, default=240)
    ap.add_argument("--height", type=int, default=135)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--legs", default="")
    ap.add_argument("--trace", default="")
    ap.add_argument("--resources", default="")
    ap.add_argument("--bench", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    {"leg": leg, "trace": trace, "merge": merge}[args.mode](args)


if __name__ == "__main__":
    main()
