#!/usr/bin/env python3
"""tools/light_resampling_model.py -- the float64 model of fh_set_light_resampling on the model scene (tests/light_resampling_scenes.py), CPU only: the predicted
first-vertex variance with the lamp overhead and with the lamp 15 aside, for M = 2, 4, 8, 16 candidates beside the table alone and the uniform pick; the default the
rule picks; the exact marginal of the chosen emitter at the model's floor point; whether the clamp binds in the quadrature; and the two mistakes the unbiasedness
tests must catch.  Writes profiles/light_resampling_model.json.

The rule: the smallest M among 2, 4, 8, 16 whose predicted variance on the lamp-aside scene (summed over rgb, averaged over the model's floor points) is within
1.25 x the best of the four."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import light_resampling_model as R  # noqa: E402
import light_resampling_scenes as RS  # noqa: E402
import light_sampling_scenes as S  # noqa: E402
from fredholm_amd import native as N  # noqa: E402

MS = [2, 4, 8, 16]
U = N.LIGHT_UNIFORM_FRACTION_DEFAULT


def main():
    out = {"scene": "tests/light_sampling_scenes.py: the model scene (Lambertian floor, large dim panel, small bright lamp), %d floor points, uniform share %g" % (len(S.MODEL_GRID), U),
           "rule": "the smallest M among 2, 4, 8, 16 whose predicted variance on the lamp-aside scene is within 1.25 x the best of the four"}
    for name, aside in (("lamp_overhead", 0.0), ("lamp_aside", RS.ASIDE)):
        quads = S.model_quads(aside)
        base = S.model_prediction(U, quads=quads)
        var = {m: RS.model_prediction(m, quads=quads)["variance"] for m in MS}
        info = {}
        tris, les = S.model_lights(quads)
        table, prox = S.model_table(U, quads), RS.model_proxies(quads)
        for m in MS:
            for x in S.MODEL_GRID:
                R.floor_moments(x, RS.UP, S.MODEL_RHO, tris, les, table, prox, m, info=info)
        g = R.geom64(prox, S.MODEL_X, np.array(RS.UP))
        out[name] = {"aside": aside, "variance_uniform": base["variance_off"], "variance_table": base["variance_on"], "variance_resampled": {str(m): var[m] for m in MS},
                     "ratio_to_uniform": {str(m): var[m] / base["variance_off"] for m in MS}, "ratio_to_table": {str(m): var[m] / base["variance_on"] for m in MS},
                     "table_to_uniform": base["variance_on"] / base["variance_off"],
                     "largest_unclamped_term": info["clamp_max"], "clamped_probability": info["clamped_probability"],
                     "pick_p_table": [float(p) for p in table.p], "geometric_weight_at_model_x": [float(v) for v in g],
                     "marginal_at_model_x": {str(m): [float(v) for v in R.marginal(table, g, m)] for m in MS}}
    aside = {m: out["lamp_aside"]["variance_resampled"][str(m)] for m in MS}
    default = RS.default_candidates(aside)
    out["default_candidates"] = default
    out["lamp_aside_below_uniform"] = {str(m): bool(aside[m] < out["lamp_aside"]["variance_uniform"]) for m in MS}
    # the two mistakes, as bias of the frame mean relative to the mean, on the lamp-aside scene at the default
    quads = S.model_quads(RS.ASIDE)
    tris, les = S.model_lights(quads)
    table, prox = S.model_table(U, quads), RS.model_proxies(quads)
    out["mistakes"] = {}
    for mistake in ("pdf_area", "one_site"):
        good = np.array([sum(R.floor_moments(x, RS.UP, S.MODEL_RHO, tris, les, table, prox, default)[k][0] for k in (0, 1)) for x in S.MODEL_GRID]).mean(axis=0)
        bad = np.array([sum(R.floor_moments(x, RS.UP, S.MODEL_RHO, tris, les, table, prox, default, mistake=mistake)[k][0] for k in (0, 1)) for x in S.MODEL_GRID]).mean(axis=0)
        out["mistakes"][mistake] = {"relative_bias_rgb": [float(v) for v in (bad - good) / good]}
    path = os.path.join(ROOT, "profiles", "light_resampling_model.json")
    json.dump(out, open(path, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
