#!/usr/bin/env python3
"""tools/light_sampling_bench.py -- what sampling of area lights by power (fh_set_light_sampling) costs and gains.

  leg    python3 tools/light_sampling_bench.py leg [--width 240 --height 135 --spp 16 --ref-spp 4096] --out FILE.json
         One process.  (a) The table build at 2, 1025 and 10^6 emitters (strips of emissive triangles): wall clock of the first fh_kat_light_table (build + read-back)
         less a second one that finds the table current (read-back alone).  (d) relMSE at equal samples, off and on, on two scenes -- the lamp-lit interior
         (scenes_sponza with lamps=True: four lamps of textured emission, no sky, no sun) and the model scene of the tests -- against TWO references of `ref_spp` samples,
         one rendered with the switch on and one with it off, and of the two references against each other: the one the frames of both modes are nearer to has
         converged further.  relMSE = mean over pixels and channels of (frame - ref)^2 / (ref^2 + 1e-2).  Frame times are wall clock of a synchronised call, median of five.
  trace  python3 tools/light_sampling_bench.py trace [--width 240 --height 135 --spp 16 --frames 8]
         One process: the three table builds, then `frames` frames of the interior with the switch off and `frames` with it on.  Run it under
             rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python3 tools/light_sampling_bench.py trace ...
         (no counters): NAME_kernel_stats.csv then has the plain kernels of the off frames and, of the on frames, the forms that take the light table or pick_p
         (kernel_families.py: counted under the record's keys k_shade_lt, k_trace_secondary_stream_lt ...) in one trace.
  merge  python3 tools/light_sampling_bench.py merge --legs FILE.json --stats STATS.csv --frames 8 [--listing render.s] --out profiles/light_sampling_bench.json   (no GPU)
         (b) summed time of the shade, tail and secondary-ray kernels per shaded hit, plain against _lt; (a) the build kernels one by one;
         (c) registers, scratch and LDS of the new instantiations from the metadata of a device listing (hipcc -S --cuda-device-only render.hip).
"""
import argparse
import csv
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from kernel_families import family, template_id  # noqa: E402

STRIPS = (2, 1025, 1000000)


def interior(tmp):
    from fredholm_amd import scenes_sponza as SS
    from fredholm_amd.scene import Scene
    path = os.path.join(tmp, "sponza_lamps.gltf")
    info = SS.write_sponza_gltf(path, lamps=True)
    s = Scene()
    s.load_model(path)
    return s.as_dict(), SS.SPONZA_CAMERA, info


def build_times(F, N, np):
    import ctypes as C
    import light_sampling_scenes as S
    out = {}
    for n in STRIPS:
        sc = S.strip(n, seed=n)[0]
        r = F.Renderer(0)
        r.load_scene(sc)
        r.build_ias()
        r.set_light_sampling()
        q, total = np.zeros(n, np.uint32), C.c_uint64(0)
        t = []
        for _ in range(2):
            t0 = time.perf_counter()
            N.check(r._ctx, N.lib().fh_kat_light_table(r._ctx, N.ptr(q), None, None, C.byref(total)), "fh_kat_light_table")
            t.append(time.perf_counter() - t0)
        r.close()
        out[str(n)] = {"build_and_read_back_ms": round(t[0] * 1e3, 3), "read_back_ms": round(t[1] * 1e3, 3)}
    return out


def relmse(img, ref):
    return float(((img - ref) ** 2 / (ref ** 2 + 1e-2)).mean())


def measure(F, N, np, sc, cam, bg, w, h, depth, spp, ref_spp, count_hits):
    r = F.Renderer(0)
    r.load_scene(sc)
    r.build_ias()
    r.set_resolution(w, h)
    L = F.RenderLayer(r, w, h)

    def frame(n, timed=False):
        r.init_render_states()
        t0 = time.perf_counter()
        r.render(cam, bg, L, n, depth)
        r.wait_for_completion()
        dt = time.perf_counter() - t0
        img = L.download("beauty")[..., :3].astype(np.float64)
        return (img, dt) if timed else img

    def timed(n):
        frame(n)
        runs = [frame(n, True) for _ in range(5)]
        return runs[-1][0], statistics.median(t for _, t in runs)
    rec = {"emitters": int(r.n_lights()), "width": w, "height": h, "max_depth": depth, "spp": spp, "references": f"{ref_spp} spp, one with the switch on, one with it off"}
    ref_off = frame(ref_spp)
    off, t_off = timed(spp)
    if count_hits:
        r.set_flags(N.FLAG_COUNT_TRAVERSAL)
        r.reset_stats()
        frame(spp)
        rec["shaded_hits_per_frame_off"] = int(r.stats()["shaded_hits"])
        r.set_flags(0)
    r.set_light_sampling()
    rec["uniform_fraction"] = r.get_light_sampling()[1]
    ref_on = frame(ref_spp)
    on, t_on = timed(spp)
    r.close()
    both = lambda img: {"against_reference_on": relmse(img, ref_on), "against_reference_off": relmse(img, ref_off)}
    rec.update({"frame_ms_off": round(t_off * 1e3, 3), "frame_ms_on": round(t_on * 1e3, 3), "relmse_off": both(off), "relmse_on_equal_samples": both(on),
                "relmse_reference_off_against_reference_on": relmse(ref_off, ref_on), "mean_reference_on": float(ref_on.mean()), "mean_reference_off": float(ref_off.mean())})
    return rec


def leg(args):
    import numpy as np
    import fredholm_amd as F
    from fredholm_amd import native as N
    import light_sampling_scenes as S
    from test_estimator_expectation import lens_at
    tmp = tempfile.mkdtemp(prefix="light_bench_")
    sc, camera, info = interior(tmp)
    rec = {"table_build": build_times(F, N, np), "table_build_source": "wall clock of the first fh_kat_light_table (build + read-back) and of a second one (read-back alone)",
           "frame_ms_source": "wall clock of fh_render + fh_sync, median of five"}
    rec["interior"] = measure(F, N, np, sc, F.Camera(**camera), (0.0, 0.0, 0.0), args.width, args.height, 8, args.spp, args.ref_spp, True)
    rec["interior"]["scene"] = f"scenes_sponza with lamps=True ({info['triangles']} triangles), lit by its four lamps alone"
    rec["model_scene"] = measure(F, N, np, S.model_scene(), lens_at((0.0, 4.0, 0.0)), (0.0, 0.0, 0.0), 64, 48, 1, args.spp, args.ref_spp, False)
    rec["model_scene"]["scene"] = "tests/light_sampling_scenes.py: model_scene()"
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
    build_times(F, N, np)
    tmp = tempfile.mkdtemp(prefix="light_bench_")
    sc, camera, _ = interior(tmp)
    r = F.Renderer(0)
    r.load_scene(sc)
    r.build_ias()
    r.set_resolution(args.width, args.height)
    L = F.RenderLayer(r, args.width, args.height)
    cam = F.Camera(**camera)
    for on in (False, True):
        if on:
            r.set_light_sampling()
        for _ in range(args.frames):
            r.init_render_states()
            r.render(cam, (0.0, 0.0, 0.0), L, args.spp, 8)
            r.wait_for_completion()
    r.close()
    print(json.dumps({"frames_per_mode": args.frames, "spp": args.spp, "width": args.width, "height": args.height}))


FAMILIES = ("k_shade_lt", "k_shade_env", "k_shade", "k_tail_lt", "k_tail_env", "k_tail", "k_trace_secondary_static_lt", "k_trace_secondary_coop_lt", "k_trace_secondary_stream_lt",
            "k_trace_merged_stream_lt", "k_trace_secondary_static", "k_trace_secondary_coop", "k_trace_secondary_stream", "k_trace_merged_stream", "k_light_weights", "k_light_chunks",
            "k_light_offsets", "k_light_write")


def kernel_rows(path):
    rows = {}
    pat = re.compile(r"\b(k_light_\w+)\b")
    for row in csv.DictReader(open(path)):
        m = pat.search(row["Name"])
        fam = m.group(1) if m else family(row["Name"])  # (the forms with a table: kernel_families.py)
        if fam not in FAMILIES:
            continue
        c = rows.setdefault(fam, {"calls": 0, "total_ns": 0})
        c["calls"] += int(row["Calls"])
        c["total_ns"] += int(row["TotalDurationNs"])
    return rows


def listing_metadata(path):
    s = open(path).read()
    out = {}
    for m in re.finditer(r"\.group_segment_fixed_size: (\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size: (\d+).*?\.vgpr_count:\s+(\d+)", s, re.S):
        lds, name, scratch, vgpr = m.groups()
        if (family(name) or "").endswith("_lt"):
            out[template_id(name)[1]] = {"vgprs": int(vgpr), "scratch_bytes": int(scratch), "lds_bytes": int(lds)}
    return out


def merge(args):
    rec = json.loads(open(args.legs).read())
    rows = kernel_rows(args.stats)
    rec["kernels"] = rows
    rec["kernels_source"] = f"rocprofv3 --kernel-trace --stats, no counters, one run of `trace`: the three table builds, {args.frames} frames of the interior with the switch off, then {args.frames} with it on"
    rec["table_build_kernels_us"] = {k: round(v["total_ns"] / max(v["calls"], 1) / 1e3, 2) for k, v in rows.items() if k.startswith("k_light_")}
    rec["table_build_kernels_note"] = "mean over the three builds (2, 1025 and 10^6 emitters) and the interior's; the per-size wall clock is table_build"
    hits = rec["interior"].get("shaded_hits_per_frame_off", 0) * args.frames
    if hits:
        rec["ns_per_shaded_hit"] = {k: round(v["total_ns"] / hits, 4) for k, v in rows.items() if not k.startswith("k_light_")}
    if args.listing:
        rec["new_instantiations"] = listing_metadata(args.listing)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec)[:2000])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["leg", "trace", "merge"])
    ap.add_argument("--width", type=int, default=240)
    ap.add_argument("--height", type=int, default=135)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--legs", default="")
    ap.add_argument("--stats", default="")
    ap.add_argument("--listing", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    {"leg": leg, "trace": trace, "merge": merge}[args.mode](args)


if __name__ == "__main__":
    main()
