#!/usr/bin/env python3
"""tools/light_sampling_model.py -- the float64 model of fh_set_light_sampling on the model scene (tests/light_sampling_scenes.py), CPU only: the predicted first-vertex
variance for the candidate uniform shares and the default the rule picks, and where the mode loses -- emitters of equal power, and a textured emitter whose 16 points
misjudge its mean.  Writes profiles/light_sampling_model.json.

The rule: the largest share among 1/2, 1/4, 1/8, 1/16 whose predicted variance (summed over rgb, averaged over the model's floor points) is within 1.25 x of the best
of them."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import light_sampling_scenes as S  # noqa: E402
from test_estimator_expectation import LIGHT_QUADS  # noqa: E402

SHARES = [0.5, 0.25, 0.125, 0.0625]


def main():
    pred = {u: S.model_prediction(u) for u in SHARES}
    var = {u: pred[u]["variance_on"] for u in SHARES}
    best = min(var.values())
    default = max(u for u in SHARES if var[u] <= 1.25 * best)
    off = pred[SHARES[0]]["variance_off"]
    out = {
        "scene": "Lambertian floor (albedo 0.8, 0.6, 0.4) under the two quads of tests/test_estimator_expectation.py, the first's radiance x %g, the second shrunk by %g with radiance x %g: "
                 "emitter powers %.1f : 1; %d floor points" % (S.DIM, S.SHRINK, S.BRIGHT, S.model_power_ratio(), len(S.MODEL_GRID)),
        "rule": "the largest share among 1/2, 1/4, 1/8, 1/16 whose predicted variance is within 1.25 x of the best of them",
        "variance_off": off,
        "variance_on": {repr(u): var[u] for u in SHARES},
        "ratio_on_off": {repr(u): var[u] / off for u in SHARES},
        "pick_p": {repr(u): [float(x) for x in S.model_table(u).p] for u in SHARES},
        "default_uniform_fraction": default,
    }
    # where it loses.  (1) emitters of (nearly) equal power: the quads as the estimator test has them
    eq = S.model_prediction(default, quads=LIGHT_QUADS)
    out["equal_power"] = {"scene": "the same quads unscaled (powers within 1.3 x of each other)", "variance_on": eq["variance_on"], "variance_off": eq["variance_off"],
                          "ratio_on_off": eq["variance_on"] / eq["variance_off"]}
    # (1b) a powerful emitter far from everything it lights: the lamp moved 15 aside keeps its power and its pick probability and gives the floor a fraction of what it gave
    far = S.model_prediction(default, quads=S.model_quads(15.0))
    out["far_lamp"] = {"scene": "the model scene with the bright lamp moved 15 along +x", "variance_on": far["variance_on"], "variance_off": far["variance_off"],
                       "ratio_on_off": far["variance_on"] / far["variance_off"]}
    # (2) a textured emitter misjudged by its 16 points: the bright lamp's weight under- and over-estimated
    out["misjudged"] = {}
    for k in (0.01, 0.1, 10.0, 100.0):
        m = S.model_prediction(default, misjudge=[1.0, 1.0, k, k])
        out["misjudged"][repr(k)] = {"variance_on": m["variance_on"], "ratio_on_off": m["variance_on"] / off}
    path = os.path.join(ROOT, "profiles", "light_sampling_model.json")
    json.dump(out, open(path, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
