#!/usr/bin/env python3
"""tools/env_sampling_bench.py -- what importance sampling of the environment (fh_set_env_sampling) costs and gains on BASELINE.json configs[3], the textured
interior, lit by a generated 2048 x 1024 sun-and-sky image in place of its Hosek dome and directional light.

  leg    python3 tools/env_sampling_bench.py leg [--width 960 --height 540 --spp 16 --ref-spp 4096] --out FILE.json
         One process: the time of the table build (the first fh_kat_env_table after the switch goes on, less a second one that finds the table current); frames of
         `spp` samples with the switch off and on (wall clock of a synchronised call, median of five); TWO references of `ref_spp` samples, one with the switch off
         and one with it on.  Neither is a common truth: the two estimators agree in expectation where the tests hold them to it (single-lobe floors), and differ
         where the reference's clamp binds, in its multi-lobe MIS weights and in the NaN -> 1 glow the mode drops -- on this scene the two reference means
         differ by 19 %; and under a sun a few texels wide the off reference has not converged at 4096 samples (it finds the sun in 2e-5 of its sky rays), so errors
         against it measure the reference.  Both are reported;
         relMSE = mean over pixels and channels of (frame - ref)^2 / (ref^2 + 1e-2) of the off frame, of the on frame at equal samples, and of an on frame whose
         sample count is scaled by t_off / t_on (equal time), against either reference, and of the two references against each other; the shaded hits of one off
         frame, counted by an instrumented frame of its own.
  trace  python3 tools/env_sampling_bench.py trace [--width 960 --height 540 --spp 16 --frames 8]
         One process that renders nothing but `frames` frames with the switch off and then `frames` with it on.  Run it under
             rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python3 tools/env_sampling_bench.py trace ...
         (no counters): DIR/.../NAME_kernel_stats.csv then has the k_shade launches of the off frames and the k_shade<..., fh::EnvTable> launches of the on frames, in one trace.
  merge  python3 tools/env_sampling_bench.py merge --legs FILE.json --stats STATS.csv --frames 8 --out profiles/env_sampling_bench.json   (no GPU)
         The leg's record with the summed time of the k_shade and of the k_shade_env launches of the trace per shaded hit (the two modes shade the same hits: the
         next direction of a path does not depend on how its sky ray was drawn), and the table's build kernels.  The launches with the table count under the record's
         key k_shade_env (kernel_families.py), as when they were a kernel of that name.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from kernel_families import family  # noqa: E402


def sun_and_sky(w=2048, h=1024):
    """a clear-sky gradient (brighter towards the horizon, a dim ground) and a sun of radiance 20000 about three texels across at 40 degrees elevation"""
    import numpy as np
    y, x = np.meshgrid((np.arange(h) + 0.5) / h * np.pi, (np.arange(w) + 0.5) / w * 2 * np.pi, indexing="ij")
    up = np.cos(y)
    sky = np.where(up > 0, 0.25 + 0.9 * (1.0 - up) ** 3, 0.05)
    img = np.ones((h, w, 4), np.float32)
    img[..., 0], img[..., 1], img[..., 2] = 0.55 * sky, 0.75 * sky, 1.0 * sky
    d = np.stack([np.sin(y) * np.cos(x), np.cos(y), np.sin(y) * np.sin(x)], axis=-1)
    el, az = np.radians(40.0), np.radians(250.0)
    s = np.array([np.cos(el) * np.cos(az), np.sin(el), np.cos(el) * np.sin(az)])
    img[(d @ s) > np.cos(np.radians(0.27)), :3] = 20000.0
    return img


def leg(args):
    import numpy as np
    import bench
    import fredholm_amd as F
    from fredholm_amd import native as N
    tmp = tempfile.mkdtemp(prefix="env_bench_")
    wl = bench.workload(3, tmp)
    w, h, depth = args.width, args.height, wl["depth"]
    r = F.Renderer(0)
    r.load_scene(wl["scene"])
    r.build_ias()
    r.load_ibl(sun_and_sky())
    r.set_resolution(w, h)
    L = F.RenderLayer(r, w, h)
    cam = F.Camera(**wl["camera"])

    def frame(spp, timed=False):
        r.init_render_states()
        t0 = time.perf_counter()
        r.render(cam, wl["bg"], L, spp, depth)
        r.wait_for_completion()
        dt = time.perf_counter() - t0
        img = L.download("beauty")[..., :3].astype(np.float64)
        return (img, dt) if timed else img

    def timed(spp):
        frame(spp)  # warm-up: pools, lists, the table
        runs = [frame(spp, True) for _ in range(5)]
        return runs[-1][0], statistics.median(t for _, t in runs)

    ref_off = frame(args.ref_spp)
    off, t_off = timed(args.spp)
    r.set_flags(N.FLAG_COUNT_TRAVERSAL)
    r.reset_stats()
    frame(args.spp)
    hits = int(r.stats()["shaded_hits"])
    r.set_flags(0)
    r.set_env_sampling()
    bufs = [np.zeros((256, 512), np.uint32), np.zeros((256, 513), np.float32), np.zeros(257, np.float32), np.zeros((256, 512), np.float32)]
    t = []
    for _ in range(2):
        t0 = time.perf_counter()
        N.check(r._ctx, N.lib().fh_kat_env_table(r._ctx, *[N.ptr(b) for b in bufs]), "fh_kat_env_table")
        t.append(time.perf_counter() - t0)
    ref_on = frame(args.ref_spp)
    on, t_on = timed(args.spp)
    spp_time = max(1, int(round(args.spp * t_off / t_on)))
    on_time = frame(spp_time)

    def relmse(img, ref):
        return float(((img - ref) ** 2 / (ref ** 2 + 1e-2)).mean())

    def both(img):
        return {"against_reference_on": relmse(img, ref_on), "against_reference_off": relmse(img, ref_off)}
    rec = {"scene": wl["name"], "environment": "generated 2048 x 1024 sun-and-sky image (tools/env_sampling_bench.py: sun_and_sky), no Hosek dome, no directional light",
           "width": w, "height": h, "max_depth": depth, "spp": args.spp, "references": f"{args.ref_spp} spp, one with the switch on, one with it off",
           "relmse_reference_off_against_reference_on": relmse(ref_off, ref_on), "mean_reference_on": float(ref_on.mean()), "mean_reference_off": float(ref_off.mean()),
           "cosine_fraction": r.get_env_sampling()[1], "table_sub_samples": max(2, min(16, -(-sun_and_sky().shape[1] // 512))),
           "table_build_ms": round((t[0] - t[1]) * 1e3, 3), "table_build_source": "wall clock of the first fh_kat_env_table (build + read-back) less a second one (read-back alone)",
           "frame_ms_off": round(t_off * 1e3, 3), "frame_ms_on": round(t_on * 1e3, 3), "frame_ms_source": "wall clock of fh_render + fh_sync, median of five",
           "shaded_hits_per_frame_off": hits, "relmse_off": both(off), "relmse_on_equal_samples": both(on), "spp_on_equal_time": spp_time,
           "relmse_on_equal_time": both(on_time), "max_weight_share_of_table": float(bufs[3].max())}
    r.close()
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def trace(args):
    import bench
    import fredholm_amd as F
    tmp = tempfile.mkdtemp(prefix="env_bench_")
    wl = bench.workload(3, tmp)
    r = F.Renderer(0)
    r.load_scene(wl["scene"])
    r.build_ias()
    r.load_ibl(sun_and_sky())
    r.set_resolution(args.width, args.height)
    L = F.RenderLayer(r, args.width, args.height)
    cam = F.Camera(**wl["camera"])
    for on in (False, True):
        if on:
            r.set_env_sampling()
        for _ in range(args.frames):
            r.init_render_states()
            r.render(cam, wl["bg"], L, args.spp, wl["depth"])
            r.wait_for_completion()
    r.close()
    print(json.dumps({"frames_per_mode": args.frames, "spp": args.spp, "width": args.width, "height": args.height}))


def kernel_rows(path):
    """summed over the instantiations: (calls, total ns) of k_shade and of k_shade_env; the table's build kernels one by one"""
    rows = {}
    for row in csv.DictReader(open(path)):
        m = re.search(r"(k_env_weights|k_env_rows|k_env_marginal|k_env_cells)", row["Name"])
        fam = m.group(1) if m else family(row["Name"])  # (the forms with the table: kernel_families.py)
        if fam not in ("k_shade_env", "k_shade", "k_tail_env", "k_tail", "k_env_weights", "k_env_rows", "k_env_marginal", "k_env_cells"):
            continue
        c = rows.setdefault(fam, {"calls": 0, "total_ns": 0})
        c["calls"] += int(row["Calls"])
        c["total_ns"] += int(row["TotalDurationNs"])
    return rows


def merge(args):
    rec = json.loads(open(args.legs).read())
    rows = kernel_rows(args.stats)
    rec["kernels"] = rows
    rec["kernels_source"] = f"rocprofv3 --kernel-trace --stats, no counters, one run of `trace`: {args.frames} frames with the switch off, then {args.frames} with it on"
    if "k_env_weights" in rows:
        rec["table_build_kernels_us"] = {k: round(v["total_ns"] / max(v["calls"], 1) / 1e3, 2) for k, v in rows.items() if k.startswith("k_env_")}
    if "k_shade" in rows and "k_shade_env" in rows:
        hits = rec["shaded_hits_per_frame_off"] * args.frames
        rec["shade_ns_per_hit"] = {k: round(rows[k]["total_ns"] / hits, 4) for k in ("k_shade", "k_shade_env")}
        rec["shade_ns_per_hit_note"] = "hits of the wavefront bounces and of the fused tail together; the tail's own rows (k_tail, k_tail_env) hold its shading and its traversal"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["leg", "trace", "merge"])
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--legs", default="")
    ap.add_argument("--stats", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    {"leg": leg, "trace": trace, "merge": merge}[args.mode](args)


if __name__ == "__main__":
    main()
