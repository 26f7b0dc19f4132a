#!/usr/bin/env python3
"""tools/denoise_temporal_replay.py [--out FILE] -- what temporal accumulation buys, replayed on the CPU (no GPU needed).

The sequence of the device's quality test (tests/test_gpu_denoise_temporal.py: QUALITY, quality_camera) rendered by the CPU checker -- Cornell box, 96 x 72, depth 5,
8 frames with seeds 1..8 -- and denoised by that file's float64 restatement of fh_denoise_temporal and of fh_denoise_guided.  The luminance moments are rebuilt
from the running means the checker leaves after every sample (x_s = s * mean_s - (s - 1) * mean_(s-1)).  Prints, for the last frame with moments against the
1024-spp truth at the last camera, relMSE of the unfiltered frame, of the guided filter alone and of temporal accumulation, and their ratio R, at 16 spp per frame
with the moving camera, at 4 spp per frame, and for a still camera; then R of the first sequence for other parameter values.  One JSON line at the end.

--motion replays the sequence of tests/test_gpu_denoise_motion.py instead (MOTION_QUALITY: a still camera, the short block of cornell_box_instanced() moving 0.05 per
frame) through that file's float64 restatement of fh_denoise_temporal_motion and through the plain one, and prints relMSE over the pixels whose chief ray sees the block
in the last frame and over the whole frame: R = relMSE(motion) / relMSE(plain temporal) is what the device test's margin is taken from.  The checker renders the block
where the instance transform puts it (a translation: the baked vertices are the device's world-space vertices bit for bit); the id plane is the chief rays' closest
hit, by brute force in float64.

--response replays four sequences -- (L) the light's emission x 0.25 after 8 frames, (S) the light quad moved, (M) the moving camera, (B) the moving block -- through the
float64 restatement of fh_set_denoise_response for several gamma and chooses the default by a stated rule.  --noise-box replays the same four with gamma = 1 fixed
through the restatement of fh_set_denoise_response_noise (tests/test_denoise_noise_box_host.py) for kappa in KAPPAS, chooses the default kappa by the same rule, and also
records what the step would do WITHOUT moments (on the 7 x 7 spatial variance), which is why the library leaves that path alone.

--temporal-moments (-> profiles/denoise_temporal_moments_replay.json) replays calls WITHOUT sample moments through the float64 restatement of
fh_set_denoise_temporal_moments (tests/test_denoise_temporal_moments_host.py): the QUALITY sequence at 16, 4 and 1 spp, a still camera at 1 spp, and (L), (S), (M) of
--response (shared with its --cache), for min_history in MIN_HISTORIES, clip off and gamma = 1, beside the spatial-estimate and the sample-moment calls, and chooses the
default min_history by a stated rule."""
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


def _load(name, filename):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", filename))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def chief_ids(scene, cam, w, h):
    """instance of the closest triangle along every pixel's chief ray (float64 Moeller-Trumbore over all faces; 0xffffffff: a miss)"""
    t = np.asarray(cam.params()[:12], np.float64).reshape(3, 4)
    f = 1.0 / np.tan(0.5 * cam.m_fov)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    d = np.stack([(2.0 * (xx + 0.5) - w) / h, -(2.0 * (yy + 0.5) - h) / h, np.full(xx.shape, -f)], axis=2)  # (ux = -(...), the lens centre minus the sensor point, z flipped)
    d = (d / np.linalg.norm(d, axis=2, keepdims=True)) @ t[:, :3].T
    o = t[:, :3] @ np.array([0.0, 0.0, f]) + t[:, 3]
    v = np.asarray(scene["vertices"], np.float64)[np.asarray(scene["indices"])]
    best, ids = np.full((h, w), np.inf), np.full((h, w), 0xFFFFFFFF, np.uint32)
    for k in range(v.shape[0]):
        e1, e2 = v[k, 1] - v[k, 0], v[k, 2] - v[k, 0]
        pv = np.cross(d, e2)
        det = pv @ e1
        with np.errstate(all="ignore"):
            inv = 1.0 / det
            tv = o - v[k, 0]
            u = (pv @ tv) * inv
            qv = np.cross(tv, e1)
            vv = (d @ qv) * inv
            tt = (qv @ e2) * inv
        ok = (np.abs(det) > 1e-12) & (u >= 0) & (vv >= 0) & (u + vv <= 1) & (tt > 0) & (tt < best)
        best = np.where(ok, tt, best)
        ids = np.where(ok, np.uint32(scene["instance_ids"][k]), ids)
    return ids


def motion_replay(out):
    """the moving-block sequence: relMSE of plain temporal accumulation and of the motion call, over the block's pixels and over the frame"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    M = _load("test_gpu_denoise_motion", "test_gpu_denoise_motion.py")
    T = M.T
    from fredholm_amd import native as N
    from fredholm_amd import scenes
    from oracle import pyoracle as O
    import fredholm_amd as F

    q = M.MOTION_QUALITY
    w, h, depth, spp = q["w"], q["h"], q["depth"], q["spp"]
    threads = O.hardware_threads()
    cam = F.Camera(**scenes.CORNELL_CAMERA)

    def baked(offset):
        sc = scenes.cornell_box_instanced()
        v = sc["vertices"].copy()
        block = np.asarray(sc["indices"])[sc["instance_ids"] == 1].reshape(-1)
        v[block] = v[block] + np.asarray(offset, np.float32)  # (o2w is the identity plus a translation: 1 * x + t in float32, the device's world-space vertex)
        sc["vertices"] = v
        return sc

    def frame(ref, n, seed):
        lo = ref.new_layers(w, h)
        s1, s2, prev = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w, 3))
        for s in range(1, n + 1):
            ref.render(cam.params(), w, h, lo, 1, depth, seed=seed, n_threads=threads)
            mean = lo["beauty"][..., :3].astype(np.float64)
            x = s * mean - (s - 1) * prev
            prev = mean
            y = x[..., 0] * float(T.LUM[0]) + x[..., 1] * float(T.LUM[1]) + x[..., 2] * float(T.LUM[2])
            s1 += y
            s2 += y * y
        res = {k: lo[k].copy() for k in ("beauty", "normal", "albedo", "position", "depth")}
        res["moments"] = np.stack([s1 / n, s2 / n], axis=2).astype(np.float32)
        res["counts"] = np.full((h, w), n, np.uint32)
        return res

    offsets = [M.motion_quality_offset(k) for k in range(q["frames"])]
    frames, ids = [], None
    for k, off in enumerate(offsets):
        sc = baked(off)
        plain_scene = {key: val for key, val in sc.items() if key not in ("instance_ids", "object_to_world", "world_to_object")}
        frames.append(frame(O.Scene(plain_scene), spp, 1 + k))
        ids = chief_ids(sc, cam, w, h)
        frames[-1]["ids"] = ids
        print(f"frame {k}: block at {off}, {int((ids == 1).sum())} pixels see it")
    ref = O.Scene({key: val for key, val in baked(offsets[-1]).items() if key not in ("instance_ids", "object_to_world", "world_to_object")})
    lo = ref.new_layers(w, h)
    for _ in range(q["truth_spp"]):
        ref.render(cam.params(), w, h, lo, 1, depth, seed=1000, n_threads=threads)
    truth = lo["beauty"]
    plain, motion = M.MotionRestatement(np.float64, np.exp), M.MotionRestatement(np.float64, np.exp)
    for k, layers in enumerate(frames):
        out_plain = plain.call(layers, cam.params())
        if k == 0:
            out_motion = motion.call(layers, cam.params())
        else:
            table = N.motion_from_transforms(*scenes.instanced_transforms(offsets[k - 1]), *scenes.instanced_transforms(offsets[k]))
            out_motion = motion.call_motion(layers, cam.params(), layers["ids"], M.table_arrays(table))
    guided = T.Restatement(np.float64, np.exp).call(frames[-1], cam.params(), spatial_only=True)
    box = ids == 1

    def err(x, mask=None):
        return T._relmse(x, truth) if mask is None else T._relmse(x[mask][None], truth[mask][None])
    rec = {"replay": True, "motion": True, "quality": q, "defaults": T.TDEF, "block_pixels": int(box.sum()),
           "block": dict(unfiltered=err(frames[-1]["beauty"], box), guided=err(guided, box), temporal=err(out_plain, box), motion=err(out_motion, box)),
           "frame": dict(unfiltered=err(frames[-1]["beauty"]), guided=err(guided), temporal=err(out_plain), motion=err(out_motion)),
           "block_with_history": dict(temporal=float(plain.have[box].mean()), motion=float(motion.have[box].mean())),
           "block_mean_history": dict(temporal=float(plain.hist["h"][box].mean()), motion=float(motion.hist["h"][box].mean()))}
    rec["R"] = rec["block"]["motion"] / rec["block"]["temporal"]
    rec["R_frame"] = rec["frame"]["motion"] / rec["frame"]["temporal"]
    line = json.dumps(rec)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


GAMMAS = (0.5, 0.75, 1.0, 1.5, 2.0, 3.0)
KAPPAS = (3.0, 4.0, 5.0, 6.0, 8.0)


def response_replay(out, cache, noise_box=False):
    """what fh_set_denoise_response buys and costs: four sequences through the float64 restatement of tests/test_gpu_denoise_response.py, for every gamma of GAMMAS;
    noise_box: what fh_set_denoise_response_noise adds at gamma = 1, for every kappa of KAPPAS, through the restatement of tests/test_denoise_noise_box_host.py"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    R = _load("test_gpu_denoise_response", "test_gpu_denoise_response.py")
    H = _load("test_denoise_noise_box_host", "test_denoise_noise_box_host.py") if noise_box else None
    M, T = R.M, R.T
    from fredholm_amd import native as N
    from fredholm_amd import scenes
    from oracle import pyoracle as O
    import fredholm_amd as F

    q = R.RESPONSE_QUALITY
    w, h, depth, spp, n_before, n_after = q["w"], q["h"], q["depth"], q["spp"], q["frames_before"], q["frames_after"]
    threads = O.hardware_threads()
    still = F.Camera(**scenes.CORNELL_CAMERA)

    def frame(ref, cam, seed):
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
        res = {k: lo[k].copy() for k in ("beauty", "normal", "albedo", "position", "depth")}
        res["moments"] = np.stack([s1 / spp, s2 / spp], axis=2).astype(np.float32)
        res["counts"] = np.full((h, w), spp, np.uint32)
        return res

    def truth(ref, cam):
        lo = ref.new_layers(w, h)
        for _ in range(q["truth_spp"]):
            ref.render(cam.params(), w, h, lo, 1, depth, seed=1000, n_threads=threads)
        return lo["beauty"].copy()

    def rendered():
        """every frame and truth of the four sequences, as one flat dict of arrays"""
        d = {}

        def put(name, layers):
            for k, v in layers.items():
                d[f"{name}/{k}"] = v
        base = O.Scene(scenes.cornell_box())
        for k in range(n_before):
            put(f"A{k}", frame(base, still, 1 + k))
        d["truth/A"] = truth(base, still)
        for tag in ("L", "S"):
            ref = O.Scene(R.changed_scene(tag))
            for k in range(n_before, n_before + n_after):
                put(f"{tag}{k}", frame(ref, still, 1 + k))
            d[f"truth/{tag}"] = truth(ref, still)
            print(f"rendered ({tag})", flush=True)
        for k in range(T.QUALITY["frames"]):
            put(f"M{k}", frame(base, T.quality_camera(k), 1 + k))
        d["truth/M"] = truth(base, T.quality_camera(T.QUALITY["frames"] - 1))
        print("rendered (M)", flush=True)
        plain = lambda sc: {key: val for key, val in sc.items() if key not in ("instance_ids", "object_to_world", "world_to_object")}
        for k in range(M.MOTION_QUALITY["frames"]):
            sc = scenes.cornell_box_instanced()
            v = sc["vertices"].copy()
            block = np.asarray(sc["indices"])[sc["instance_ids"] == 1].reshape(-1)
            v[block] = v[block] + np.asarray(M.motion_quality_offset(k), np.float32)
            sc["vertices"] = v
            ref = O.Scene(plain(sc))
            put(f"B{k}", dict(frame(ref, still, 1 + k), ids=chief_ids(sc, still, w, h)))
        d["truth/B"] = truth(ref, still)
        print("rendered (B)", flush=True)
        return d

    if cache and os.path.exists(cache):
        d = dict(np.load(cache))
    else:
        d = rendered()
        if cache:
            np.savez_compressed(cache, **d)
    layers_of = lambda name: {k.split("/")[1]: v for k, v in d.items() if k.startswith(name + "/")}
    assert (T.QUALITY["w"], T.QUALITY["h"], T.QUALITY["spp"]) == (w, h, spp) == (M.MOTION_QUALITY["w"], M.MOTION_QUALITY["h"], M.MOTION_QUALITY["spp"])

    def clipped_share(st):
        return None if st.u is None else float((st.u[st.have] > 0).mean())

    def run(gamma, frames, first_scored, truth_of, extra=None, kappa=None, use_moments=True):
        """the scored frames of a sequence for one call: gamma None is the plain call, a number the clipped one, "guided" the spatial filter alone on each scored frame.
        frames: [(camera, layers, motion table or None)]; the frames from `first_scored` on (1-based) are scored against truth_of(frame); extra(output, truth) adds fields.
        kappa: the noise box on top (use_moments False: on the spatial variance, which the library does not do)"""
        st = R.ResponseRestatement(np.float64, np.exp) if kappa is None else H.NoiseBoxRestatement(np.float64, np.exp)
        st.gamma = None if gamma == "guided" else gamma
        if kappa is not None:
            st.kappa, st.without_moments = kappa, not use_moments
        res = []
        for k, (cam, layers, table) in enumerate(frames):
            scored = k + 1 >= first_scored
            if gamma == "guided":
                if not scored:
                    continue
                o = T.Restatement(np.float64, np.exp).call(layers, cam.params(), use_moments, spatial_only=True)
            else:
                o = st.call_r(layers, cam.params(), layers.get("ids"), table, use_moments)
            if scored:
                truth_k = truth_of(k + 1)
                res.append(dict(frame=k + 1, relmse=T._relmse(o, truth_k), clipped=None if gamma == "guided" else clipped_share(st), **(extra(o, truth_k) if extra else {})))
        return res

    def all_calls(frames, first_scored, truth_of, extra=None):
        if noise_box:
            res = {}
            for tail, mom in (("", True), (" no moments", False)):
                res["guided" + tail] = run("guided", frames, first_scored, truth_of, extra, use_moments=mom)
                res["plain" + tail] = run(None, frames, first_scored, truth_of, extra, use_moments=mom)
                res["clipped" + tail] = run(1.0, frames, first_scored, truth_of, extra, use_moments=mom)
                res.update({f"kappa={k}{tail}": run(1.0, frames, first_scored, truth_of, extra, kappa=k, use_moments=mom) for k in KAPPAS})
            return res
        return {"guided": run("guided", frames, first_scored, truth_of, extra), "plain": run(None, frames, first_scored, truth_of, extra),
                **{f"gamma={g}": run(g, frames, first_scored, truth_of, extra) for g in GAMMAS}}

    rec = {"replay": True, "response": True, "quality": q, "defaults": T.TDEF, "gammas": list(GAMMAS), "sequences": {}}
    if noise_box:
        rec = {"replay": True, "noise_box": True, "quality": q, "defaults": T.TDEF, "gamma": 1.0, "kappas": list(KAPPAS), "sequences": {}}
    for tag in ("L", "S"):
        frames = [(still, layers_of(f"A{k}"), None) for k in range(n_before)] + [(still, layers_of(f"{tag}{k}"), None) for k in range(n_before, n_before + n_after)]
        rec["sequences"][tag] = all_calls(frames, n_before, lambda f, tag=tag: d["truth/A"] if f <= n_before else d[f"truth/{tag}"])
        print(tag, json.dumps(rec["sequences"][tag]), flush=True)
    nm = T.QUALITY["frames"]
    rec["sequences"]["M"] = all_calls([(T.quality_camera(k), layers_of(f"M{k}"), None) for k in range(nm)], nm, lambda f: d["truth/M"])
    print("M", json.dumps(rec["sequences"]["M"]), flush=True)
    nb = M.MOTION_QUALITY["frames"]
    tables = [None] + [M.table_arrays(N.motion_from_transforms(*scenes.instanced_transforms(M.motion_quality_offset(k - 1)), *scenes.instanced_transforms(M.motion_quality_offset(k))))
                       for k in range(1, nb)]
    box = d[f"B{nb - 1}/ids"] == 1
    rec["sequences"]["B"] = all_calls([(still, layers_of(f"B{k}"), tables[k]) for k in range(nb)], nb, lambda f: d["truth/B"],
                                      lambda o, t: dict(relmse_block=T._relmse(o[box][None], t[box][None])))
    print("B", json.dumps(rec["sequences"]["B"]), flush=True)

    seq = rec["sequences"]
    if noise_box:
        # the default, by the rule that chose gamma: the smallest sum of relMSE over the four frames after the change on (L) + (S), among the kappas whose steady state
        # costs at most 5 % of the plain call; the rows without moments are scored against the plain call without moments
        for tail in ("", " no moments"):
            choice = {}
            for key in ["clipped" + tail] + [f"kappa={k}{tail}" for k in KAPPAS]:
                plain = "plain" + tail
                steady = {"L frame 8": seq["L"][key][0]["relmse"] / seq["L"][plain][0]["relmse"], "M last": seq["M"][key][0]["relmse"] / seq["M"][plain][0]["relmse"],
                          "B frame": seq["B"][key][0]["relmse"] / seq["B"][plain][0]["relmse"], "B block": seq["B"][key][0]["relmse_block"] / seq["B"][plain][0]["relmse_block"]}
                after = sum(f["relmse"] for tag in ("L", "S") for f in seq[tag][key][1:])
                choice[key] = dict(steady=steady, after_change=after, qualifies=max(steady.values()) <= 1.05)
                print(key, json.dumps(choice[key]))
            rec["choice" + tail.replace(" ", "_")] = choice
        rec["guided_after_change"] = sum(f["relmse"] for tag in ("L", "S") for f in seq[tag]["guided"][1:])
        ok = [k for k in KAPPAS if rec["choice"][f"kappa={k}"]["qualifies"]]
        rec["default_kappa"] = min(ok, key=lambda k: rec["choice"][f"kappa={k}"]["after_change"]) if ok else None
        print("default kappa:", rec["default_kappa"])
        line = json.dumps(rec)
        print(line)
        if out:
            with open(out, "w") as f:
                f.write(line + "\n")
        return
    # the default: the smallest sum of the clipped call's relMSE over the frames after the change on (L) + (S), among the gammas whose steady state costs at most 5 %
    choice = {}
    for g in GAMMAS:
        key = f"gamma={g}"
        steady = {"L frame 8": seq["L"][key][0]["relmse"] / seq["L"]["plain"][0]["relmse"], "M last": seq["M"][key][0]["relmse"] / seq["M"]["plain"][0]["relmse"],
                  "B frame": seq["B"][key][0]["relmse"] / seq["B"]["plain"][0]["relmse"], "B block": seq["B"][key][0]["relmse_block"] / seq["B"]["plain"][0]["relmse_block"]}
        after = sum(f["relmse"] for tag in ("L", "S") for f in seq[tag][key][1:])
        choice[key] = dict(steady=steady, after_change=after, qualifies=max(steady.values()) <= 1.05)
        print(key, json.dumps(choice[key]))
    ok = [g for g in GAMMAS if choice[f"gamma={g}"]["qualifies"]]
    rec["choice"] = choice
    rec["default_gamma"] = min(ok, key=lambda g: choice[f"gamma={g}"]["after_change"]) if ok else None
    rec["nearest_gamma"] = min(GAMMAS, key=lambda g: max(choice[f"gamma={g}"]["steady"].values()))
    print("default gamma:", rec["default_gamma"], "(nearest to the steady-state condition:", rec["nearest_gamma"], ")")
    line = json.dumps(rec)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


MIN_HISTORIES = (2.0, 3.0, 4.0, 6.0)
STEADY = ("moving_16spp", "moving_4spp", "moving_1spp", "still_1spp")


def moments_replay(out, cache):
    """what fh_set_denoise_temporal_moments buys in calls WITHOUT sample moments: the QUALITY sequence at 16, 4 and 1 spp per frame, a still camera at 1 spp, and (L), (S),
    (M) of --response (read from its --cache where the file holds them, rendered and added to it otherwise), through the float64 restatement of
    tests/test_denoise_temporal_moments_host.py for min_history in MIN_HISTORIES, clip off and gamma = 1, beside the call with the 7 x 7 spatial estimate (the switch off)
    and the call WITH sample moments; and the default min_history by the stated rule"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    H = _load("test_denoise_temporal_moments_host", "test_denoise_temporal_moments_host.py")
    R, T = H.R, H.T
    from fredholm_amd import scenes
    from oracle import pyoracle as O
    import fredholm_amd as F

    q = R.RESPONSE_QUALITY
    w, h, depth, n_before, n_after, nm = q["w"], q["h"], q["depth"], q["frames_before"], q["frames_after"], T.QUALITY["frames"]
    assert (T.QUALITY["w"], T.QUALITY["h"], T.QUALITY["spp"], T.QUALITY["depth"]) == (w, h, q["spp"], depth) and q["spp"] == 16
    threads = O.hardware_threads()
    still = F.Camera(**scenes.CORNELL_CAMERA)
    d = dict(np.load(cache)) if cache and os.path.exists(cache) else {}
    n_cached = len(d)

    def frames_at(ref, cam, seed, names):
        """one frame rendered sample by sample; names: {spp: name}: the layers after 1, 4 or 16 samples are a frame of that many samples per pixel with the same seed"""
        if all(f"{n}/beauty" in d for n in names.values()):
            return
        lo = ref.new_layers(w, h)
        s1, s2, prev = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w, 3))
        for s in range(1, max(names) + 1):
            ref.render(cam.params(), w, h, lo, 1, depth, seed=seed, n_threads=threads)
            mean = lo["beauty"][..., :3].astype(np.float64)
            x = s * mean - (s - 1) * prev
            prev = mean
            y = x[..., 0] * float(T.LUM[0]) + x[..., 1] * float(T.LUM[1]) + x[..., 2] * float(T.LUM[2])
            s1 += y
            s2 += y * y
            if s in names:
                for k in ("beauty", "normal", "albedo", "position", "depth"):
                    d[f"{names[s]}/{k}"] = lo[k].copy()
                d[f"{names[s]}/moments"] = np.stack([s1 / s, s2 / s], axis=2).astype(np.float32)
                d[f"{names[s]}/counts"] = np.full((h, w), s, np.uint32)

    def truth(ref, cam, name):
        if name not in d:
            lo = ref.new_layers(w, h)
            for _ in range(q["truth_spp"]):
                ref.render(cam.params(), w, h, lo, 1, depth, seed=1000, n_threads=threads)
            d[name] = lo["beauty"].copy()

    base = O.Scene(scenes.cornell_box())
    for k in range(n_before):
        frames_at(base, still, 1 + k, {16: f"A{k}", 1: f"A1_{k}"})
    truth(base, still, "truth/A")
    for tag in ("L", "S"):
        ref = O.Scene(R.changed_scene(tag))
        for k in range(n_before, n_before + n_after):
            frames_at(ref, still, 1 + k, {16: f"{tag}{k}"})
        truth(ref, still, f"truth/{tag}")
    for k in range(nm):
        frames_at(base, T.quality_camera(k), 1 + k, {16: f"M{k}", 4: f"M4_{k}", 1: f"M1_{k}"})
    truth(base, T.quality_camera(nm - 1), "truth/M")
    print("rendered", flush=True)
    if cache and len(d) != n_cached:
        np.savez_compressed(cache, **d)
    layers_of = lambda name: {k.split("/")[1]: v for k, v in d.items() if k.startswith(name + "/")}

    def run(frames, first_scored, truth_of, gamma, min_history, use_moments):
        """relMSE of the frames from `first_scored` on (1-based): gamma None is the clip off; min_history None the switch off"""
        st = H.MomentsRestatement(np.float64, np.exp)
        st.gamma, st.min_history = gamma, min_history
        res = []
        for k, (cam, layers) in enumerate(frames):
            o = st.call_r(layers, cam.params(), use_moments=use_moments)
            if k + 1 >= first_scored:
                res.append(T._relmse(o, truth_of(k + 1)))
        return res

    def rows(frames, first_scored, truth_of, gamma):
        r = {"spatial": run(frames, first_scored, truth_of, gamma, None, False), "sample moments": run(frames, first_scored, truth_of, gamma, None, True)}
        r.update({f"min_history={m:g}": run(frames, first_scored, truth_of, gamma, m, False) for m in MIN_HISTORIES})
        return r

    sequences = {"moving_16spp": [(T.quality_camera(k), layers_of(f"M{k}")) for k in range(nm)], "moving_4spp": [(T.quality_camera(k), layers_of(f"M4_{k}")) for k in range(nm)],
                 "moving_1spp": [(T.quality_camera(k), layers_of(f"M1_{k}")) for k in range(nm)], "still_1spp": [(still, layers_of(f"A1_{k}")) for k in range(n_before)],
                 "still_16spp": [(still, layers_of(f"A{k}")) for k in range(n_before)]}
    rec = {"replay": True, "temporal_moments": True, "quality": q, "defaults": T.TDEF, "min_histories": [f"{m:g}" for m in MIN_HISTORIES], "steady": {}, "steady_clipped": {}, "change": {}}
    for name, frames in sequences.items():
        truth_of = (lambda f: d["truth/M"]) if name.startswith("moving") else (lambda f: d["truth/A"])
        rec["steady"][name] = {k: v[0] for k, v in rows(frames, len(frames), truth_of, None).items()}
        rec["steady_clipped"][name] = {k: v[0] for k, v in rows(frames, len(frames), truth_of, 1.0).items()}
        print(name, "clip off", json.dumps(rec["steady"][name]), "gamma 1", json.dumps(rec["steady_clipped"][name]), flush=True)
    for tag in ("L", "S"):  # the change of lighting after 8 frames: the sum of relMSE over the 4 frames after it (and each of them)
        frames = [(still, layers_of(f"A{k}")) for k in range(n_before)] + [(still, layers_of(f"{tag}{k}")) for k in range(n_before, n_before + n_after)]
        rec["change"][tag] = {}
        for gname, gamma in (("clip off", None), ("gamma=1", 1.0)):
            r = rows(frames, n_before + 1, lambda f, tag=tag: d[f"truth/{tag}"], gamma)
            rec["change"][tag][gname] = {k: dict(frames=v, sum=sum(v)) for k, v in r.items()}
        print(tag, json.dumps(rec["change"][tag]), flush=True)
    # the default: the smallest sum over the four clip-off steady sequences of relMSE / the spatial-estimate call's relMSE; ties go to the smaller value
    sums = {f"{m:g}": sum(rec["steady"][n][f"min_history={m:g}"] / rec["steady"][n]["spatial"] for n in STEADY) for m in MIN_HISTORIES}
    rec["rule_sums"] = sums
    rec["default_min_history"] = min(MIN_HISTORIES, key=lambda m: (sums[f"{m:g}"], m))
    key = f"min_history={rec['default_min_history']:g}"
    rec["R"] = {n: rec["steady"][n][key] / rec["steady"][n]["spatial"] for n in sequences}  # what the device's quality test takes its margin from
    print("rule sums:", json.dumps(sums), "default min_history:", rec["default_min_history"], "R:", json.dumps(rec["R"]))
    line = json.dumps(rec)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--motion", action="store_true", help="replay the moving-block sequence of tests/test_gpu_denoise_motion.py instead")
    ap.add_argument("--response", action="store_true", help="replay the lighting-change and steady-state sequences of tests/test_gpu_denoise_response.py through the clipped stage")
    ap.add_argument("--noise-box", action="store_true", help="replay the same four sequences at gamma = 1 through the noise box of fh_set_denoise_response_noise, for kappa in KAPPAS")
    ap.add_argument("--cache", default="", help="--response, --noise-box, --temporal-moments: an .npz the rendered frames are kept in (read when it exists): the rendering is most of the run")
    ap.add_argument("--temporal-moments", action="store_true", help="replay steady and lighting-change sequences WITHOUT sample moments through fh_set_denoise_temporal_moments, for min_history in MIN_HISTORIES")
    a = ap.parse_args()
    if a.temporal_moments:
        return moments_replay(a.out or os.path.join(ROOT, "profiles", "denoise_temporal_moments_replay.json"), a.cache)
    if a.motion:
        return motion_replay(a.out)
    if a.response or a.noise_box:
        return response_replay(a.out, a.cache, a.noise_box)
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
