#!/usr/bin/env python3
"""tools/denoise_bench.py [--out profiles/denoise_guided_bench.json] [--config 3] [--spp 16] [--calls 20] [--temporal | --motion | --response [--noise]] -- what a call of the denoisers costs.

The layers of a BASELINE.json configs[c] frame at 1920x1080 (`--spp` samples, adaptive sampling on at threshold 0 so that the luminance moments exist), then, in this
one process, the median of `--calls` calls of fh_denoise and of fh_denoise_guided, each followed by one fh_sync and timed from before the call to after the sync:
the guided filter with every guide (position, depth, moments, counts), without the moments (the 7x7 spatial variance estimate runs instead) and without position
and depth.  Prints one JSON line (and writes it to --out).

--temporal (-> profiles/denoise_temporal_bench.json): instead, two such frames with seeds 1 and 2 from cameras a small step apart (--step, as a fraction of the camera's
distance from the origin), and the median of `--calls` calls of fh_denoise_temporal that alternate between the two frames -- every call reprojects the other frame's
history --, of calls that repeat one frame (the still-camera kernel), and of fh_denoise_guided on the same layers in the same process.  The stage's share is the
difference of the medians; the kernel's own time comes from running this under `rocprofv3 --kernel-trace --stats` (k_temporal).

--motion (-> profiles/denoise_motion_bench.json): one such frame, and the median of `--calls` calls of fh_primary_instances and of fh_denoise_temporal_motion under a still
camera with a motion table that alternates between two small translations (--step) of the scene's largest instance, so that every call carries that instance's pixels;
beside them fh_denoise_temporal with the camera alternating as in --temporal, and fh_denoise_guided.  The two new kernels' own times come from a
`rocprofv3 --kernel-trace --stats` run of this leg (k_primary_instances*, k_temporal<3, 0>: the motion look-up): `--merge-kernel-stats STATS.csv --out FILE` (no GPU) writes those rows of the
profiler's kernel_stats.csv into FILE's record as "kernel_us".

--response (-> profiles/denoise_response_bench.json): the two frames of --temporal and the id plane and alternating tables of --motion, and the median of `--calls` calls of
fh_denoise_temporal (cameras alternating; one frame repeated) and of fh_denoise_temporal_motion with fh_set_denoise_response off and then on (--gamma), in one process, beside
fh_denoise_guided.  The kernels' own times come from a `rocprofv3 --kernel-trace --stats` run of this leg, in which the instances of k_temporal<LOOK, CLIP> -- LOOK 1, 2, 3: own tap,
reprojection, motion; CLIP 0, 1: plain, colour box -- and the k_guided_pass instances all run: `--merge-kernel-stats STATS.csv --out FILE` adds them (with the passes' rows), and
`--resource-usage LOG` the registers, LDS, scratch and occupancy hipcc's -Rpass-analysis=kernel-resource-usage printed for those kernels when denoise.hip was built.

--response --noise (-> profiles/denoise_noise_box_bench.json): the --response leg (every call has moments) with a third round, fh_set_denoise_response_noise on (--kappa) as well:
plain, clipped, clipped with the noise box, in one process.  In a `rocprofv3 --kernel-trace --stats` run of this leg the three k_temporal<., 1> and the three
k_temporal<., 2> (colour box + noise box) run side by side: the former are the reference point for the latter.

--moments (-> profiles/denoise_temporal_moments_bench.json): the calls of --response WITHOUT sample moments (the 7 x 7 estimate runs in all of them) with
fh_set_denoise_temporal_moments off and then on (--min-history), each with the clip off and on, in one process.  In a `rocprofv3 --kernel-trace --stats` run of this leg the six
instances k_temporal<LOOK, CLIP, true> run beside the six k_temporal<LOOK, CLIP, false> they are measured against (LOOK 1, 2, 3; CLIP 0, 1); the record also holds the bytes
per pixel both move, whose ratio is what the moments may cost."""
import argparse
import json
import os
import re
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


def moving_instance(a, F, w):
    """what the --motion and --response legs share: the scene's instance with the most faces, `step` (--step x the camera's distance from the origin), the two motion tables
    that carry that instance by + step and - step along x in world space (o2w' = T o2w, w2o' = w2o T^-1), and the workload's camera with a second one `step` to its side"""
    from fredholm_amd import native as N
    sc = w["scene"] if isinstance(w["scene"], dict) else None
    inst = None if sc is None else sc.get("instance_ids")
    o2w = None if sc is None or sc.get("object_to_world") is None else np.asarray(sc["object_to_world"], np.float32).reshape(-1, 12)
    n_inst = 1 if o2w is None else o2w.shape[0]
    ident = np.tile(np.asarray([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), (n_inst, 1))
    base_o = ident if o2w is None else o2w
    base_w = ident if o2w is None else np.asarray(sc["world_to_object"], np.float32).reshape(-1, 12)
    target = 0 if inst is None else int(np.bincount(np.asarray(inst, np.int64), minlength=n_inst).argmax())
    o = np.asarray(w["camera"]["origin"], np.float64)
    step = a.step * max(float(np.linalg.norm(o)), 1.0)
    tables = []
    for sign in (1.0, -1.0):
        cur_o, cur_w = base_o.copy(), base_w.copy()
        cur_o[target, 3] += np.float32(sign * step)
        cur_w[target, 3::4] -= cur_w[target, 0::4][:3] * np.float32(sign * step)
        tables.append(N.motion_from_transforms(base_o, base_w, cur_o, cur_w))
    cams = [F.Camera(**w["camera"]), F.Camera(**dict(w["camera"], origin=tuple(o + np.array([step, 0.0, 0.0]))))]
    return n_inst, target, step, tables, cams


def motion(a, bench, F, DeviceBuffer, r, w):
    W, H = w["width"], w["height"]
    n_inst, target, step, tables, cams = moving_instance(a, F, w)
    L = F.RenderLayer(r, W, H)
    r.render(cams[0], w["bg"], L, a.spp, w["depth"])
    m, c, out, ids = DeviceBuffer(r, 8 * W * H), DeviceBuffer(r, 4 * W * H), DeviceBuffer(r, 16 * W * H), DeviceBuffer(r, 4 * W * H)
    r.get_luminance_moments(m.ptr)
    r.get_sample_counts(c.ptr)
    r.primary_instances(cams[0], W, H, ids.ptr)
    r.wait_for_completion()
    id_plane = ids.download(np.uint32, (H, W))
    p = L.ptrs
    turn = [0]

    def call_motion():
        turn[0] += 1
        r.denoise_temporal_motion(W, H, p["beauty"], p["normal"], p["albedo"], out.ptr, p["position"], p["depth"], cams[0], ids.ptr, tables[turn[0] & 1], m.ptr, c.ptr)

    def call_temporal():
        turn[0] += 1
        r.denoise_temporal(W, H, p["beauty"], p["normal"], p["albedo"], out.ptr, p["position"], p["depth"], cams[turn[0] & 1], m.ptr, c.ptr)

    def call_guided():
        r.denoise_guided(W, H, p["beauty"], p["normal"], p["albedo"], out.ptr, p["position"], p["depth"], m.ptr, c.ptr)
    rec = {"workload": w["name"], "width": W, "height": H, "spp": a.spp, "calls": a.calls, "instance_step": step, "instances": n_inst, "moved_instance": target,
           "carried_pixel_share": float((id_plane == target).mean()), "missed_pixel_share": float((id_plane == 0xFFFFFFFF).mean()), "source_fingerprint": bench.source_fingerprint(),
           "fh_denoise_guided_ms": median_ms(r, call_guided, a.calls),
           "fh_primary_instances_ms": median_ms(r, lambda: r.primary_instances(cams[0], W, H, ids.ptr), a.calls),
           "fh_denoise_temporal_motion_ms": median_ms(r, call_motion, a.calls),
           "fh_denoise_temporal_moving_ms": median_ms(r, call_temporal, a.calls),
           "fh_denoise_guided_again_ms": median_ms(r, call_guided, a.calls)}
    rec["stage_motion_ms_by_difference"] = rec["fh_denoise_temporal_motion_ms"] - rec["fh_denoise_guided_ms"]
    rec["stage_moving_ms_by_difference"] = rec["fh_denoise_temporal_moving_ms"] - rec["fh_denoise_guided_ms"]
    r.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def response(a, bench, F, DeviceBuffer, r, w):
    W, H = w["width"], w["height"]
    n_inst, target, step, tables, cams = moving_instance(a, F, w)
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
    out, ids = DeviceBuffer(r, 16 * W * H), DeviceBuffer(r, 4 * W * H)
    r.primary_instances(cams[0], W, H, ids.ptr)
    r.wait_for_completion()
    turn = [0]

    def call_temporal(alternate):
        cam, p, m, c = frames[turn[0] & 1 if alternate else 0]
        turn[0] += 1
        r.denoise_temporal(W, H, p["beauty"], p["normal"], p["albedo"], out.ptr, p["position"], p["depth"], cam, m.ptr, c.ptr)

    def call_motion():
        cam, p, m, c = frames[0]
        turn[0] += 1
        r.denoise_temporal_motion(W, H, p["beauty"], p["normal"], p["albedo"], out.ptr, p["position"], p["depth"], cam, ids.ptr, tables[turn[0] & 1], m.ptr, c.ptr)

    def call_guided():
        cam, p, m, c = frames[0]
        r.denoise_guided(W, H, p["beauty"], p["normal"], p["albedo"], out.ptr, p["position"], p["depth"], m.ptr, c.ptr)
    rec = {"workload": w["name"], "width": W, "height": H, "spp": a.spp, "calls": a.calls, "camera_step": step, "gamma": a.gamma, "source_fingerprint": bench.source_fingerprint(),
           "fh_denoise_guided_ms": median_ms(r, call_guided, a.calls)}
    rounds = [("", None, None), ("response_", a.gamma, None)]
    if a.noise:
        rec["kappa"] = a.kappa
        rounds.append(("response_noise_", a.gamma, a.kappa))
    for name, gamma, kappa in rounds:
        if gamma is None:
            r.clear_denoise_response()
        else:
            r.set_denoise_response(gamma)
        if kappa is not None:
            r.set_denoise_response_noise(kappa)
        rec[f"fh_denoise_temporal_{name}moving_ms"] = median_ms(r, lambda: call_temporal(True), a.calls)
        rec[f"fh_denoise_temporal_{name}still_ms"] = median_ms(r, lambda: call_temporal(False), a.calls)
        rec[f"fh_denoise_temporal_motion_{name}ms"] = median_ms(r, call_motion, a.calls)
    r.clear_denoise_response()
    if a.noise:
        r.clear_denoise_response_noise()
        for leg in ("moving", "still"):
            rec[f"noise_{leg}_ms_by_difference"] = rec[f"fh_denoise_temporal_response_noise_{leg}_ms"] - rec[f"fh_denoise_temporal_response_{leg}_ms"]
        rec["noise_motion_ms_by_difference"] = rec["fh_denoise_temporal_motion_response_noise_ms"] - rec["fh_denoise_temporal_motion_response_ms"]
    rec["fh_denoise_guided_again_ms"] = median_ms(r, call_guided, a.calls)
    for leg in ("moving", "still"):
        rec[f"response_{leg}_ms_by_difference"] = rec[f"fh_denoise_temporal_response_{leg}_ms"] - rec[f"fh_denoise_temporal_{leg}_ms"]
    rec["response_motion_ms_by_difference"] = rec["fh_denoise_temporal_motion_response_ms"] - rec["fh_denoise_temporal_motion_ms"]
    r.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def temporal_moments(a, bench, F, DeviceBuffer, r, w):
    """the --response leg's calls WITHOUT sample moments (the calls fh_set_denoise_temporal_moments is for), in four rounds: the moments switch off and on, each with the
    clip off and on.  Turning the switch drops the history; the warm-up calls of every median build it again"""
    W, H = w["width"], w["height"]
    n_inst, target, step, tables, cams = moving_instance(a, F, w)
    frames = []
    for k, cam in enumerate(cams):
        L = F.RenderLayer(r, W, H)
        r.init_render_states()
        r.seed = 1 + k
        r.render(cam, w["bg"], L, a.spp, w["depth"])
        r.wait_for_completion()
        frames.append((cam, L.ptrs))
    out, ids = DeviceBuffer(r, 16 * W * H), DeviceBuffer(r, 4 * W * H)
    r.primary_instances(cams[0], W, H, ids.ptr)
    r.wait_for_completion()
    turn = [0]

    def call_temporal(alternate):
        cam, p = frames[turn[0] & 1 if alternate else 0]
        turn[0] += 1
        r.denoise_temporal(W, H, p["beauty"], p["normal"], p["albedo"], out.ptr, p["position"], p["depth"], cam)

    def call_motion():
        cam, p = frames[0]
        turn[0] += 1
        r.denoise_temporal_motion(W, H, p["beauty"], p["normal"], p["albedo"], out.ptr, p["position"], p["depth"], cam, ids.ptr, tables[turn[0] & 1])

    def call_guided():
        cam, p = frames[0]
        r.denoise_guided(W, H, p["beauty"], p["normal"], p["albedo"], out.ptr, p["position"], p["depth"])
    rec = {"workload": w["name"], "width": W, "height": H, "spp": a.spp, "calls": a.calls, "camera_step": step, "gamma": a.gamma, "min_history": a.min_history, "sample_moments": False,
           "source_fingerprint": bench.source_fingerprint(), "fh_denoise_guided_ms": median_ms(r, call_guided, a.calls)}
    for mom in (False, True):
        if mom:
            r.set_denoise_temporal_moments(a.min_history)
        else:
            r.clear_denoise_temporal_moments()
        for gamma in (None, a.gamma):
            if gamma is None:
                r.clear_denoise_response()
            else:
                r.set_denoise_response(gamma)
            name = ("moments_" if mom else "") + ("response_" if gamma is not None else "")
            rec[f"fh_denoise_temporal_{name}moving_ms"] = median_ms(r, lambda: call_temporal(True), a.calls)
            rec[f"fh_denoise_temporal_{name}still_ms"] = median_ms(r, lambda: call_temporal(False), a.calls)
            rec[f"fh_denoise_temporal_motion_{name}ms"] = median_ms(r, call_motion, a.calls)
    r.clear_denoise_response()
    r.clear_denoise_temporal_moments()
    rec["fh_denoise_guided_again_ms"] = median_ms(r, call_guided, a.calls)
    for clip in ("", "response_"):
        for leg in ("moving", "still"):
            rec[f"moments_{clip}{leg}_ms_by_difference"] = rec[f"fh_denoise_temporal_moments_{clip}{leg}_ms"] - rec[f"fh_denoise_temporal_{clip}{leg}_ms"]
        rec[f"moments_{clip}motion_ms_by_difference"] = rec[f"fh_denoise_temporal_motion_moments_{clip}ms"] - rec[f"fh_denoise_temporal_motion_{clip}ms"]
    # bytes a pixel moves in the stage, as DESIGN.md 4a counts them: (c, v), N, P, Z read, every history element fetched once (48), three images and the plane written (52): 152,
    # and 4 more for the id with motion.  The moments: 8 per tap fetched (one tap still, four otherwise) and 8 written
    base = {"still": 152, "moving": 152, "motion": 156}
    rec["bytes_per_pixel"] = {k: {"plain": v, "moments": v + 8 * (1 if k == "still" else 4) + 8} for k, v in base.items()}
    r.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def merge_resource_usage(log_path, json_path):
    """what hipcc -Rpass-analysis=kernel-resource-usage printed for the temporal kernels and the passes, into the record of json_path"""
    rec = json.loads(open(json_path).read())
    rows, name = {}, None
    for line in open(log_path):
        m = re.search(r"remark: +(Function Name|[A-Za-z ]+(?: \[[^\]]*\])?): +(\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = m.group(2) if ("k_temporal" in m.group(2) or "k_guided_pass" in m.group(2)) else None
            if name:
                rows[name] = {}
        elif name and m.group(1).split(" [")[0] in ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "Occupancy", "LDS Size"):
            rows[name][m.group(1).split(" [")[0]] = int(m.group(2))
    rec["resource_usage"] = rows
    rec["resource_usage_source"] = "hipcc -Rpass-analysis=kernel-resource-usage on denoise.hip with the Makefile's flags (mangled names)"
    line = json.dumps(rec)
    print(line)
    with open(json_path, "w") as f:
        f.write(line + "\n")


def merge_kernel_stats(csv_path, json_path):
    """the k_primary_instances* and k_temporal* rows of a rocprofv3 kernel_stats.csv into the record of json_path: calls, mean, min and max in microseconds"""
    import csv
    rec = json.loads(open(json_path).read())
    rows = {}
    for row in csv.DictReader(open(csv_path)):
        name = row["Name"]
        if "k_primary_instances" in name or "k_temporal" in name or ("k_guided_pass" in name and rec.get("gamma") is not None):
            short = re.search(r"k_(primary_instances|temporal|guided_pass)\w*(<[^>]*>)?", name).group(0)
            rows[short] = {"calls": int(row["Calls"]), "mean": float(row["AverageNs"]) / 1e3, "min": float(row["MinNs"]) / 1e3, "max": float(row["MaxNs"]) / 1e3}
    rec["kernel_us"] = rows
    rec["kernel_us_source"] = "rocprofv3 --kernel-trace --stats of a run of this leg of its own (warm-up calls included)"
    line = json.dumps(rec)
    print(line)
    with open(json_path, "w") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--temporal", action="store_true")
    ap.add_argument("--motion", action="store_true")
    ap.add_argument("--response", action="store_true")
    ap.add_argument("--gamma", type=float, default=1.0, help="--response: the gamma of fh_set_denoise_response")
    ap.add_argument("--noise", action="store_true", help="--response: a third round with fh_set_denoise_response_noise on")
    ap.add_argument("--kappa", type=float, default=6.0, help="--response --noise: the kappa of fh_set_denoise_response_noise")
    ap.add_argument("--moments", action="store_true", help="the --response leg without sample moments, with fh_set_denoise_temporal_moments off and on")
    ap.add_argument("--min-history", type=float, default=2.0, help="--moments: the min_history of fh_set_denoise_temporal_moments")
    ap.add_argument("--step", type=float, default=0.002)
    ap.add_argument("--resource-usage", default="", help="a log of hipcc -Rpass-analysis=kernel-resource-usage on denoise.hip: add its figures to the record in --out and exit (no GPU)")
    ap.add_argument("--merge-kernel-stats", default="", help="a rocprofv3 kernel_stats.csv of the --motion leg: add its rows to the record in --out and exit (no GPU)")
    a = ap.parse_args()
    if a.merge_kernel_stats:
        return merge_kernel_stats(a.merge_kernel_stats, a.out)
    if a.resource_usage:
        return merge_resource_usage(a.resource_usage, a.out)

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
    if a.motion:
        return motion(a, bench, F, DeviceBuffer, r, w)
    if a.moments:
        return temporal_moments(a, bench, F, DeviceBuffer, r, w)
    if a.response:
        return response(a, bench, F, DeviceBuffer, r, w)
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
