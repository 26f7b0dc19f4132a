#!/usr/bin/env python3
"""tools/env_sampling_model.py [OUT.json] -- the default cosine fraction of fh_set_env_sampling, chosen on the CPU from the float64 variance model of the tests.

For B in {0.125, 0.25, 0.5} and for today's cosine-distributed sky ray: the predicted variance of one first-vertex sample at a Lambertian floor (albedo 0.8) that
sees the whole upper hemisphere -- the sky ray plus the BSDF-sampled light ray, tests/env_sampling_model.py: lambert_floor_variance -- under two environments: the
64 x 32 sun image of the tests and a constant background.  The rule: among the fractions whose variance under the constant is within 1.1 x today's, the one with the
smallest variance under the sun image.  Under a constant a Lambertian floor is sampled perfectly today (variance 0 but for rounding), so no fraction can meet
that bound and the rule has no answer.  What is then taken is this tool's own choice, not part of the rule: the fraction with the smallest variance under the
constant (0.5), i.e. the rule's concern for the cosine-friendly case kept and its bound given up.  Its price is written beside it: under the sun image 0.5 predicts about
four times the variance of 0.125 (12.8 against 3.0; today's sampler: 632).  Both outcomes are written.
Variances are summed over the three channels.  Writes profiles/env_sampling_model.json (or OUT.json) and prints it."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import env_sampling_model as M  # noqa: E402
from oracle import pyoracle as oracle  # noqa: E402

CANDIDATES = (0.125, 0.25, 0.5)
RHO = (0.8, 0.8, 0.8)
CONSTANT_BOUND = 1.1


def predicted(env):
    t = M.Table(M.weights_of(env, oracle))
    dirs, wq = M.cell_quadrature(range(M.H // 2))
    L = M.radiance(env, dirs.astype(np.float32), oracle).astype(np.float64)
    out = {}
    for beta in (None,) + CANDIDATES:
        mean, var, _ = M.lambert_floor_variance(t, beta, dirs, wq, L, RHO)
        out["cosine" if beta is None else repr(beta)] = {"mean": float(mean.sum()), "variance": float(var.sum())}
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "env_sampling_model.json")
    sun, const = predicted(("ibl", M.sun_image())), predicted(("constant",))
    ok = [b for b in CANDIDATES if const[repr(b)]["variance"] <= CONSTANT_BOUND * const["cosine"]["variance"]]
    by_rule = min(ok, key=lambda b: sun[repr(b)]["variance"]) if ok else None
    fallback = min(CANDIDATES, key=lambda b: const[repr(b)]["variance"])
    choice = by_rule if by_rule is not None else fallback
    doc = {"what": "predicted first-vertex variance (sum over rgb) of a Lambertian floor, albedo 0.8, per cosine fraction; 'cosine' is the sampler with the switch off",
           "sun_image": sun, "constant": const, "constant_bound": CONSTANT_BOUND, "within_bound": ok, "choice_by_rule": by_rule,
           "own_choice_when_the_rule_has_no_answer_smallest_variance_under_the_constant": fallback, "choice": choice,
           "price_of_the_choice": "sun-image variance of the choice over that of the best candidate: %.2f" % (sun[repr(choice)]["variance"] / min(sun[repr(b)]["variance"] for b in CANDIDATES))}
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
