#!/usr/bin/env python3
"""tools/denoise_temporal_replay.py [--out FILE] -- what temporal accumulation buys, replayed on the CPU (no GPU needed).

The sequence of the device's quality test (tests/test_gpu_denoise_temporal.py: QUALITY, quality_camera) rendered by the CPU checker -- Cornell box, 96 x 72, depth 5,
8 frames with seeds 1..8 -- and denoised by that file's float64 restatement of fh_denoise_temporal and of fh_denoise_guided.  The luminance moments are rebuilt
from the running means the checker leaves after every sample (x_s = s * mean_s - (s - 1) * mean_(s-1)).  Prints, for the last frame with moments against the
1024-spp truth at the last camera, relMSE of the unfiltered frame, of the guided filter alone and of temporal accumulation, and their ratio R, at 16 spp per frame
with the moving camera, at 4 spp per frame, and for a still camera; then R of the first sequence for other parameter values.  One JSON line at the end."""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build():
    """(the test module, the three sequences, ratio(frames, **temporal parameters))"""
    spec = importlib.util.spec_from_file_location("temporal_tests", os.path.join(ROOT, "tests", "test_gpu_denoise_temporal.py"))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    from fredholm_amd import scenes
    from oracle import pyoracle as O

    q = T.QUALITY
    w, h, depth = q["w"], q["h"], q["depth"]
    ref = O.Scene(scenes.cornell_box())
    threads = O.hardware_threads()

    def frame(cam, spp, seed):
        lo = ref.new_layers(w, h)
        s1, s2, prev = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w, 3))
        for s in range(1, spp + 1):
            ref.render(cam.params(), w, h, lo, 1, depth, seed=seed, n_threads=threads)
            mean = lo["beauty"][..., :3].astype(np.float64)
            x = s * mean - (s - 1) * prev
            prev = mean
            y = x[..., 0] * float(T.LUM[0]) + x[..., 1] * float(T.LUM[1]) + x[..., 2] * float(T.LUM[2])
            s1 += y
            s2 += y * y
        out = {k: lo[k].copy() for k in ("beauty", "normal", "albedo", "position", "depth")}
        out["moments"] = np.stack([s1 / spp, s2 / spp], axis=2).astype(np.float32)
        out["counts"] = np.full((h, w), spp, np.uint32)
        return out

    last = T.quality_camera(q["frames"] - 1)
    lo = ref.new_layers(w, h)
    for _ in range(q["truth_spp"]):  # (single-sample calls: a checker call of n samples is ONE reference launch, first-hit quirk included)
        ref.render(last.params(), w, h, lo, 1, depth, seed=1000, n_threads=threads)
    truth = lo["beauty"]
    sequences = {"moving_16spp": [(T.quality_camera(k), frame(T.quality_camera(k), 16, 1 + k)) for k in range(q["frames"])]}
    sequences["moving_4spp"] = [(T.quality_camera(k), frame(T.quality_camera(k), 4, 1 + k)) for k in range(q["frames"])]
    sequences["still_16spp"] = [(last, frame(last, 16, 1 + k)) for k in range(q["frames"])]

    def ratio(frames, **temporal):
        st = T.Restatement(np.float64, np.exp)
        for cam, layers in frames:
            out = st.call(layers, cam.params(), temporal=temporal)
        guided = T.Restatement(np.float64, np.exp).call(frames[-1][1], frames[-1][0].params(), spatial_only=True)
        hit = T._hit(frames[-1][1]["normal"])
        return dict(unfiltered=T._relmse(frames[-1][1]["beauty"], truth), guided=T._relmse(guided, truth), temporal=T._relmse(out, truth),
                    R=T._relmse(out, truth) / T._relmse(guided, truth), with_history=float(st.have[hit].mean()), mean_history=float(st.hist["h"][hit].mean()))

    return T, sequences, ratio


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    T, sequences, ratio = build()
    rec = {"replay": True, "quality": T.QUALITY, "defaults": T.TDEF}
    for name, frames in sequences.items():
        rec[name] = ratio(frames)
        print(name, json.dumps(rec[name]))
    sweep = {}
    for key, values in (("alpha_min", (0.05, 0.1, 0.2, 0.4)), ("max_history", (4.0, 8.0, 32.0)), ("normal_cos_min", (0.5, 0.9, 0.99)), ("plane_tol", (0.005, 0.02, 0.1))):
        for v in values:
            sweep[f"{key}={v}"] = {n: ratio(sequences[n], **{key: v})["R"] for n in ("moving_16spp", "moving_4spp")}
            print(f"{key}={v}", json.dumps(sweep[f"{key}={v}"]))
    rec["sweep_R"] = sweep
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
