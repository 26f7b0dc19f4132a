#!/usr/bin/env python3
"""tools/local_exposure_bench.py -- what local exposure (fh_set_local_exposure) costs: its kernels beside the chain's own, and the added cost of a call.

  leg    python3 tools/local_exposure_bench.py leg --size 1080p|4k [--calls 40] [--passes 4] --out FILE.json
         One process, one image on the device: `calls` fh_post_process calls with the switch off (k_copy + k_tone_map) and `calls` with it on (k_lx_down + `passes` x
         k_lx_atrous + k_copy + k_tone_map_local).  Writes the wall-clock cost of a synchronised call, off and on (medians; their difference is the added cost of a
         call).  Run it under
             rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python3 tools/local_exposure_bench.py leg ...
         (no counters) and the kernels' own times are in DIR/.../NAME_kernel_stats.csv: all of one trace, so k_copy and k_tone_map stand beside the new kernels.
  merge  python3 tools/local_exposure_bench.py merge --legs FILE.json[,...] --stats STATS.csv[,...] [--asm post.s] --out profiles/local_exposure_bench.json   (no GPU)
         The records of the legs with the rows of k_lx_down, k_lx_atrous, k_tone_map_local, k_copy and k_tone_map of their kernel_stats.csv (calls, mean, min, max in
         microseconds), the stage's added kernel time in units of that trace's k_copy, and -- from a `hipcc -S --cuda-device-only` listing of post.hip -- the
         registers, LDS and scratch of the new kernels.
"""
import argparse
import csv
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = {"1080p": (1920, 1080), "4k": (3840, 2160)}
KERNELS = ("k_lx_down", "k_lx_atrous", "k_tone_map_local", "k_copy", "k_tone_map")
NEW = ("k_lx_down", "k_lx_atrous", "k_tone_map_local")


def make_image(w, h):
    """a smooth field with a bright rectangle and 0.3 stops of noise: edges the stop keeps, noise it removes"""
    import numpy as np
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:h, 0:w]
    logl = -3.0 + 1.5 * np.sin(x / 97.0) * np.cos(y / 61.0) + rng.normal(0.0, 0.3, (h, w))
    logl[h // 5: h // 2, w // 2: (4 * w) // 5] += 10.0
    img = np.ones((h, w, 4), np.float32)
    img[..., :3] = (np.exp2(logl)[..., None] * rng.uniform(0.8, 1.2, (h, w, 3))).astype(np.float32)
    return img


def leg(args):
    import fredholm_amd as F
    from fredholm_amd.renderer import DeviceBuffer
    w, h = SIZES[args.size]
    img = make_image(w, h)
    r = F.Renderer(0)
    bufs = [DeviceBuffer(r, w * h * 16) for _ in range(4)]
    bufs[0].upload(img)
    for b in bufs[1:]:
        b.clear()
    pp = F.PostProcessParams(use_bloom=False, ISO=80.0, chromatic_aberration=1.0)

    def timed_post():
        t = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            r.post_process(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, w, h, pp, bufs[3].ptr)
            r.wait_for_completion()
            t.append((time.perf_counter() - t0) * 1e6)
        return t

    off = timed_post()
    r.set_local_exposure(passes=args.passes)
    on = timed_post()
    base = r.local_exposure_base()
    rec = {"size": args.size, "width": w, "height": h, "calls": args.calls, "passes": args.passes, "quarter": [int(base.shape[1]), int(base.shape[0])],
           "post_call_us_off_median": round(statistics.median(off[2:]), 2), "post_call_us_on_median": round(statistics.median(on[2:]), 2),
           "post_call_us_added": round(statistics.median(on[2:]) - statistics.median(off[2:]), 2),
           "call_cost_source": "wall clock of fh_post_process + fh_sync (no bloom), medians without the first two calls, one process",
           "base_min_max_stops": [round(float(base.min()), 3), round(float(base.max()), 3)]}
    for b in bufs:
        b.free()
    r.close()
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def kernel_rows(path):
    rows = {}
    for row in csv.DictReader(open(path)):
        for k in KERNELS:  # (k_tone_map_local before k_tone_map: the longer name first)
            if re.search(r"\b" + k + r"\b", row["Name"]) or re.search(k + r"E", row["Name"]):
                if k not in rows:
                    rows[k] = {"calls": int(row["Calls"]), "mean": round(float(row["AverageNs"]) / 1e3, 3), "min": round(float(row["MinNs"]) / 1e3, 3), "max": round(float(row["MaxNs"]) / 1e3, 3)}
                break
    return rows


def resources(asm_path):
    """vgpr, sgpr, LDS and scratch bytes of the new kernels from the metadata of a device listing"""
    text = open(asm_path).read()
    out = {}
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name:
            continue
        for k in NEW:
            if k + "E" in name.group(1):
                get = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", block).group(1))
                out[k] = {"vgpr": get("vgpr_count"), "sgpr": get("sgpr_count"), "lds_bytes": get("group_segment_fixed_size"), "scratch_bytes": get("private_segment_fixed_size")}
    return out


def merge(args):
    legs = [json.loads(open(p).read()) for p in args.legs.split(",")]
    stats = args.stats.split(",")
    assert len(legs) == len(stats), "one kernel_stats.csv per leg"
    for rec, path in zip(legs, stats):
        k = rec["kernel_us"] = kernel_rows(path)
        if all(n in k for n in KERNELS):
            # what a call with the switch on runs beyond one with it off: the analysis, and the dearer tone map
            added = k["k_lx_down"]["mean"] + rec["passes"] * k["k_lx_atrous"]["mean"] + k["k_tone_map_local"]["mean"] - k["k_tone_map"]["mean"]
            rec["stage_added_kernel_us"] = round(added, 3)
            rec["stage_added_in_k_copy"] = round(added / k["k_copy"]["mean"], 3)
            rec["k_lx_down_in_k_copy"] = round(k["k_lx_down"]["mean"] / k["k_copy"]["mean"], 3)
            rec["k_tone_map_local_to_k_tone_map"] = round(k["k_tone_map_local"]["mean"] / k["k_tone_map"]["mean"], 3)
    out = {"what": "local exposure: its kernels beside the chain's own, and the added cost of a call (tools/local_exposure_bench.py)",
           "kernel_us_source": "rocprofv3 --kernel-trace --stats, no counters, one run per leg (warm-up calls included)", "legs": legs}
    if args.asm:
        out["resources"] = resources(args.asm)
        out["resources_source"] = "metadata of hipcc -S --cuda-device-only of post.hip with the Makefile's flags (gfx950)"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["leg", "merge"])
    ap.add_argument("--size", choices=sorted(SIZES), default="1080p")
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--legs", default="")
    ap.add_argument("--stats", default="")
    ap.add_argument("--asm", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    (leg if args.mode == "leg" else merge)(args)


if __name__ == "__main__":
    main()
