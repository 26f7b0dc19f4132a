#!/usr/bin/env python3
"""tools/local_exposure_replay.py [--out profiles/local_exposure_replay.json]   (no GPU)

What local exposure (fh_set_local_exposure) does to a picture, replayed on the CPU with the float64 twin of the restatement in tests/test_gpu_local_exposure.py, at the
library's defaults, on two synthetic images:
  step    128 x 96, two plateaus E stops apart (E = 2, 3, 6, 10) round the pivot, the step in the middle column, Gaussian log-noise of 0.3 stops
  room    320 x 240, "a room with a window": a log-normal field (sigma 0.8 stops, smoothed over 8 pixels, mean 2^-4) with a rectangle 10 stops brighter and noise of
          0.2 stops on both; the exposure maps the mean log-luminance of the frame to 0.18, as auto-exposure would
For each, with the switch off and on: the share of pixels whose tone-mapped value (the checker's uchimura + sRGB) is above 0.99 in every channel, the share whose
tone-mapped luminance is below 0.02; for the steps the halo (worst |B - plateau|), the detail ratio std(l - B) / 0.3 and the contrast left between the plateau
means; for the room the same shares inside and outside the window, and once more with highlights = 0.9 and max_stops = 8."""
import argparse
import importlib.util
import json
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


def room(w=320, h=240, seed=11):
    rng = np.random.default_rng(seed)
    field = rng.normal(0.0, 1.0, (h, w))
    for axis in (0, 1):  # a box blur of 8 pixels each way, twice: a smooth field
        for _ in range(2):
            field = sum(np.roll(field, k, axis) for k in range(-4, 4)) / 8.0
    field = 0.8 * field / field.std() - 4.0
    window = np.zeros((h, w), bool)
    window[h // 5: h // 2, w // 2: (4 * w) // 5] = True
    logl = np.where(window, field + 10.0, field) + rng.normal(0.0, 0.2, (h, w))
    img = np.ones((h, w, 4), np.float32)
    img[..., :3] = np.exp2(logl)[..., None].astype(np.float32)
    return img, window


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_exposure_replay.json"))
    args = ap.parse_args()
    X = _load("test_gpu_local_exposure")
    H = _load("test_local_exposure_host")
    from oracle import pyoracle as O

    def shares(img, x, mask=None):
        rgb = (img[..., :3].astype(np.float64) * np.asarray(x, np.float64)[..., None]).astype(np.float32).reshape(-1, 3)
        y = O.math("linear_to_srgb", O.math("uchimura", rgb)).astype(np.float64).reshape(img.shape[0], img.shape[1], 3)
        lum = y @ np.array(X.LUM)
        m = np.ones(lum.shape, bool) if mask is None else mask
        return {"above_0.99": round(float((y.min(axis=2) > 0.99)[m].mean()), 4), "below_0.02": round(float((lum < 0.02)[m].mean()), 4)}

    out = {"what": "local exposure replayed in float64 on synthetic images (tools/local_exposure_replay.py), library defaults", "params": X.DEFAULTS, "steps": [], "room": {}}
    for e in (2, 3, 6, 10):
        img, plateau = H.step_image(e)
        halo, detail, contrast = H.operator_figures(e)
        _, x, _ = X.local_gain(X.Ops64, img, X.DEFAULTS, 1.0)
        out["steps"].append({"edge_stops": e, "halo_stops": round(halo, 4), "detail_ratio": round(detail, 4), "contrast_left": round(contrast, 4),
                             "off": shares(img, np.ones(img.shape[:2])), "on": shares(img, x)})
    img, window = room()
    L = X.log_image(X.Ops64, img)
    exposure = float(2.0 ** (np.log2(0.18) - L.mean()))
    _, x, diag = X.local_gain(X.Ops64, img, X.DEFAULTS, exposure)
    out["room"] = {"width": img.shape[1], "height": img.shape[0], "window_share": round(float(window.mean()), 4), "exposure": round(exposure, 4),
                   "gain_stops_window_mean": round(float(np.log2(x / exposure)[window].mean()), 3), "gain_stops_room_mean": round(float(np.log2(x / exposure)[~window].mean()), 3),
                   "off": {"frame": shares(img, np.full(img.shape[:2], exposure)), "window": shares(img, np.full(img.shape[:2], exposure), window), "room": shares(img, np.full(img.shape[:2], exposure), ~window)},
                   "on": {"frame": shares(img, x), "window": shares(img, x, window), "room": shares(img, x, ~window)}}
    strong = X.params(highlights=0.9, max_stops=8.0)  # the defaults remove half of the window's ten stops, and max_stops = 4 caps that: what a stronger setting does
    _, xs, _ = X.local_gain(X.Ops64, img, strong, exposure)
    out["room"]["strong"] = {"params": strong, "gain_stops_window_mean": round(float(np.log2(xs / exposure)[window].mean()), 3),
                             "on": {"frame": shares(img, xs), "window": shares(img, xs, window), "room": shares(img, xs, ~window)}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
