#!/usr/bin/env python3
"""tools/auto_exposure_replay.py [--out profiles/auto_exposure_replay.json] [--fps 24] [--frames-after 96]   (no GPU)

What auto-exposure (fh_set_auto_exposure) does to a sequence with a change of lighting, replayed on the CPU: frames rendered by the checker (oracle/), metered with
the restatement of tests/test_gpu_auto_exposure.py and resolved by its float64 form (resolve64).  The sequence is the one of the response tests: the Cornell box at
96 x 72, 16 samples per frame with seeds 1 + k, a still camera; 4 frames, then the light's emission x 0.25.  The frames after the change are one render each of the
dimmed scene with a new seed (the exposure sees the histogram only, so the tail repeats the last rendered frames rather than rendering all of them).
Writes the ev and target trajectory with the library's default speeds (3 / 1 per second) at the given frame rate, the frames needed to come within 0.1 stop of the new
target, the same figure from the closed form ceil(ln(|step| / 0.1) / (speed * frame_time)), and the tone-mapped mean luminance with the switch off, held (frame_time = inf)
and adapting."""
import argparse
import importlib.util
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "auto_exposure_replay.json"))
    ap.add_argument("--fps", type=float, default=24.0)
    ap.add_argument("--frames-after", type=int, default=96)
    ap.add_argument("--rendered-after", type=int, default=4)
    args = ap.parse_args()
    A = _load("test_gpu_auto_exposure")
    R = _load("test_gpu_denoise_response")
    import fredholm_amd as F
    from fredholm_amd import scenes
    from oracle import pyoracle as O

    q = A.E2E
    w, h, spp, depth, nb = q["w"], q["h"], q["spp"], q["depth"], q["frames_before"]
    cam, threads = F.Camera(**scenes.CORNELL_CAMERA), O.hardware_threads()

    def frame(ref, seed):
        lo = ref.new_layers(w, h)
        for _ in range(spp):
            ref.render(cam.params(), w, h, lo, 1, depth, seed=seed, n_threads=threads)
        return lo["beauty"].copy()

    before, after = O.Scene(scenes.cornell_box()), O.Scene(R.changed_scene("L"))
    rendered = [frame(before, 1 + k) for k in range(nb)] + [frame(after, 1 + nb + k) for k in range(args.rendered_after)]
    frames = rendered + [rendered[nb + k % args.rendered_after] for k in range(args.rendered_after, args.frames_after)]

    def tone_mapped_mean(img, exposure):
        x = (img[: (h // 16) * 16, : (w // 16) * 16, :3] * np.float32(exposure)).reshape(-1, 3)
        y = O.math("linear_to_srgb", O.math("uchimura", x)).astype(np.float64)
        return float((y @ np.array([0.2126729, 0.7151522, 0.0721750])).mean())

    iso_exposure = 80.0 / 120.0
    runs = {}
    for name, p in (("held", A.params(frame_time=math.inf)), ("adapting", A.params(frame_time=1.0 / args.fps))):
        st, rows = None, []
        for k, f in enumerate(frames):
            st = A.resolve64(A.histogram(O, f, p), p, st)
            rows.append({"frame": k + 1, "ev": round(st["ev"], 5), "target_ev": round(st["target_ev"], 5), "mean_log2": round(st["mean_log2"], 5),
                         "tone_mapped_mean": round(tone_mapped_mean(f, 2.0 ** st["ev"]), 5)})
        runs[name] = rows
    off = [round(tone_mapped_mean(f, iso_exposure), 5) for f in frames[: nb + args.rendered_after]]
    rows = runs["adapting"]
    new_target = float(np.mean([r["target_ev"] for r in rows[nb:]]))
    step = new_target - rows[nb - 1]["ev"]
    within = next((r["frame"] - nb for r in rows[nb:] if abs(r["ev"] - r["target_ev"]) <= 0.1), None)
    speed = A.DEFAULTS["speed_up"] if step > 0 else A.DEFAULTS["speed_down"]
    closed = math.ceil(math.log(abs(step) / 0.1) / (speed / args.fps)) if abs(step) > 0.1 else 0
    out = {"what": "auto-exposure replayed on checker-rendered frames in float64 (tools/auto_exposure_replay.py): Cornell box, then its light's emission x 0.25",
           "width": w, "height": h, "spp": spp, "depth": depth, "fps": args.fps, "frames_before": nb, "frames_after": args.frames_after, "rendered_after": args.rendered_after,
           "params": {k: (v if math.isfinite(v) else "inf") for k, v in A.params(frame_time=1.0 / args.fps).items()},
           "step_ev": round(step, 4), "new_target_ev": round(new_target, 4), "frames_to_within_0.1_stop": within, "frames_to_within_0.1_stop_closed_form": closed,
           "tone_mapped_mean_off": off, "held": runs["held"][: nb + args.rendered_after], "adapting": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps({k: out[k] for k in ("step_ev", "new_target_ev", "frames_to_within_0.1_stop", "frames_to_within_0.1_stop_closed_form", "tone_mapped_mean_off")}))
    print("held", [(r["ev"], r["tone_mapped_mean"]) for r in out["held"]])


if __name__ == "__main__":
    main()
