#!/usr/bin/env python3
"""tools/auto_exposure_bench.py -- what auto-exposure (fh_set_auto_exposure) costs: the metering kernels beside the chain's own, and the added cost of a call.

  leg    python3 tools/auto_exposure_bench.py leg --size 1080p|4k --image constant|noise [--calls 40] --out FILE.json
         One process, one image on the device: `calls` fh_meter_exposure calls (k_meter_histogram + k_meter_resolve), `calls` fh_post_process calls with the switch
         off (k_copy + k_tone_map) and `calls` with it on (metering + k_copy + k_tone_map_metered).  Writes the wall-clock cost of a synchronised call, off and on
         (medians; their difference is the added cost of a call), and the state the metering ended in.  Run it under
             rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python3 tools/auto_exposure_bench.py leg ...
         (no counters) and the kernels' own times are in DIR/.../NAME_kernel_stats.csv.
  merge  python3 tools/auto_exposure_bench.py merge --legs FILE.json[,...] --stats STATS.csv[,...] [--asm post.s] --out profiles/auto_exposure_bench.json   (no GPU)
         The records of the legs with the rows of k_meter_histogram, k_meter_resolve, k_copy, k_tone_map and k_tone_map_metered of their kernel_stats.csv (calls, mean, min,
         max in microseconds), the ratio of the constant to the noise image per size, and -- from a `hipcc -S --cuda-device-only` listing of post.hip -- the registers,
         LDS and scratch of the new kernels.
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
KERNELS = ("k_meter_histogram", "k_meter_resolve", "k_copy", "k_tone_map_metered", "k_tone_map")


def make_image(kind, w, h):
    import numpy as np
    if kind == "constant":
        return np.tile(np.array([0.8, 0.5, 0.3, 1.0], np.float32), (h, w, 1))
    rng = np.random.default_rng(5)
    img = np.ones((h, w, 4), np.float32)
    img[..., :3] = (np.exp2(rng.uniform(-20.0, 20.0, (h, w, 1))) * rng.uniform(0.2, 1.8, (h, w, 3))).astype(np.float32)  # log-uniform: every lane of a wave in another bin
    return img


def leg(args):
    import numpy as np
    import fredholm_amd as F
    from fredholm_amd.renderer import DeviceBuffer
    w, h = SIZES[args.size]
    img = make_image(args.image, w, h)
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
    r.set_auto_exposure()
    for _ in range(args.calls):
        r.meter_exposure(bufs[0].ptr, w, h)
    r.wait_for_completion()
    on = timed_post()
    state, hist = r.auto_exposure_state(), r.luminance_histogram()
    rec = {"size": args.size, "width": w, "height": h, "image": args.image, "calls": args.calls,
           "post_call_us_off_median": round(statistics.median(off[2:]), 2), "post_call_us_on_median": round(statistics.median(on[2:]), 2),
           "post_call_us_added": round(statistics.median(on[2:]) - statistics.median(off[2:]), 2),
           "call_cost_source": "wall clock of fh_post_process + fh_sync (no bloom), medians without the first two calls, one process",
           "state": {k: float(v) for k, v in state.items()}, "bins_in_use": int((hist[:256] != 0).sum()), "unmetered": int(hist[256])}
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
        for k in KERNELS:  # (k_tone_map_metered before k_tone_map: the longer name first)
            if re.search(r"\b" + k + r"\b", row["Name"]) or re.search(k + r"E", row["Name"]):
                if k not in rows:
                    rows[k] = {"calls": int(row["Calls"]), "mean": round(float(row["AverageNs"]) / 1e3, 3), "min": round(float(row["MinNs"]) / 1e3, 3), "max": round(float(row["MaxNs"]) / 1e3, 3)}
                break
    return rows


def resources(asm_path):
    """vgpr, sgpr, LDS and scratch bytes of the metering kernels from the metadata of a device listing"""
    text = open(asm_path).read()
    out = {}
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name:
            continue
        for k in ("k_meter_histogram", "k_meter_resolve", "k_tone_map_metered", "k_bloom_threshold_metered"):
            if k + "E" in name.group(1):
                get = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", block).group(1))
                out[k] = {"vgpr": get("vgpr_count"), "sgpr": get("sgpr_count"), "lds_bytes": get("group_segment_fixed_size"), "scratch_bytes": get("private_segment_fixed_size")}
    return out


def merge(args):
    legs = [json.loads(open(p).read()) for p in args.legs.split(",")]
    stats = args.stats.split(",")
    assert len(legs) == len(stats), "one kernel_stats.csv per leg"
    for rec, path in zip(legs, stats):
        rec["kernel_us"] = kernel_rows(path)
    out = {"what": "auto-exposure: metering kernels beside the chain's own, and the added cost of a call (tools/auto_exposure_bench.py)",
           "kernel_us_source": "rocprofv3 --kernel-trace --stats, no counters, one run per leg (warm-up calls included)", "legs": legs, "constant_to_noise": {}}
    for size in SIZES:
        by = {rec["image"]: rec for rec in legs if rec["size"] == size}
        if "constant" in by and "noise" in by and "k_meter_histogram" in by["constant"]["kernel_us"] and "k_meter_histogram" in by["noise"]["kernel_us"]:
            c, n = by["constant"]["kernel_us"]["k_meter_histogram"]["mean"], by["noise"]["kernel_us"]["k_meter_histogram"]["mean"]
            out["constant_to_noise"][size] = round(c / n, 3)
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
    ap.add_argument("--image", choices=["constant", "noise"], default="noise")
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--legs", default="")
    ap.add_argument("--stats", default="")
    ap.add_argument("--asm", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    (leg if args.mode == "leg" else merge)(args)


if __name__ == "__main__":
    main()
