"""What the light-resampling tests share (CPU only), on top of light_sampling_scenes.py: the proxies of the model scene's and the strips' emitters as the
restatement builds them, and the float64 prediction of the first-vertex variance with resampling among M candidates (light_resampling_model.py)."""
import numpy as np

import light_resampling_model as R
import light_sampling_model as M
import light_sampling_scenes as S
from fredholm_amd import native as N

f32 = np.float32
ASIDE = 15.0   # the scene the table loses on: the bright lamp 15 to the side (light_sampling_scenes.model_quads)
UP = (0.0, 1.0, 0.0)


def face_normals(corners):
    """the shading normals scenes._finish gives a flat face: its unit normal at all three corners, (n, 3, 3) float32"""
    c = np.asarray(corners, np.float64)
    n = np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)
    return np.repeat(n.astype(f32)[:, None, :], 3, axis=1)


def proxies_of(corners):
    c = np.asarray(corners, f32)
    return R.proxies(c, face_normals(c), M.area(c[:, 0], c[:, 1], c[:, 2]))


def model_proxies(quads=None):
    return proxies_of(np.array(S.model_lights(quads)[0], f32))


def model_moments(m, points, level=4, quads=None, uniform=N.LIGHT_UNIFORM_FRACTION_DEFAULT):
    """per point and channel: (mean, variance, fourth central moment), arrays (n_points, 3), with resampling among m candidates"""
    tris, les = S.model_lights(quads)
    table, prox = S.model_table(uniform, quads), model_proxies(quads)
    out = [R.floor_variance(x, UP, S.MODEL_RHO, tris, les, table, prox, m, level) for x in points]
    return tuple(np.array([o[k] for o in out]) for k in range(3))


def model_prediction(m, points=None, level=4, quads=None, uniform=N.LIGHT_UNIFORM_FRACTION_DEFAULT):
    """as light_sampling_scenes.model_prediction: the variance summed over the channels and averaged over the points, the term that bounds the relative standard
    error of its estimate, and the mean"""
    points = S.MODEL_GRID if points is None else points
    mean, var, mu4 = model_moments(m, points, level, quads, uniform)
    return {"variance": float(var.sum(axis=1).mean()), "se_term": float(np.sqrt((mu4 - var ** 2).sum(axis=0)).sum() / var.sum()), "mean": mean}


def default_candidates(variance_aside):
    """the rule: the smallest M among 2, 4, 8, 16 whose predicted variance on the lamp-aside scene is within 1.25 x the best of the four"""
    best = min(variance_aside[m] for m in (2, 4, 8, 16))
    return min(m for m in (2, 4, 8, 16) if variance_aside[m] <= 1.25 * best)
