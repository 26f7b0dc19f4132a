#!/usr/bin/env python3
"""tools/skinning_bench.py -- what posing a skinned scene costs (fh_set_skin / fh_set_joint_matrices; scene.hip: k_skin_vertices).

The scene is the configs[3] asset (fredholm_amd/scenes_sponza.py through the glTF reader) with synthetic two-joint weights on EVERY vertex and a palette of 64 joints.

  trace  python3 tools/skinning_bench.py trace [--poses 8]
         One process: the scene, the skin, `poses` poses, each followed by fh_bvh_build.  Run it under
             rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python3 tools/skinning_bench.py trace
         (a kernel trace on its own, no counters): NAME_kernel_trace.csv then holds every dispatch with its start and end.
  calls  python3 tools/skinning_bench.py calls [--poses 8] --out FILE.json
         One process, one context: the synchronised fh_set_joint_matrices + fh_bvh_build beside fh_set_transforms + fh_bvh_build, wall clock, `poses` calls each,
         alternating; every call moves something (neither takes its early return).
  merge  python3 tools/skinning_bench.py merge --calls FILE.json --trace TRACE.csv [--bench FILE.json] --out profiles/skinning_bench.json   (no GPU)
         k_skin_vertices and k_face_records per dispatch from the trace, the call times, and the bench lines of this tree and its parent where given.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_JOINTS = 64


def scene():
    from fredholm_amd import scenes_sponza as SS
    from fredholm_amd.scene import Scene
    d = tempfile.mkdtemp(prefix="skinning_bench_")
    SS.write_sponza_gltf(os.path.join(d, "sponza_like.gltf"))
    S = Scene()
    S.load_model(os.path.join(d, "sponza_like.gltf"))
    return S.as_dict()


def skin(np, nv):
    """two joints and two weights that sum to 1 on every vertex; neighbouring vertices share joints, as the vertices of a limb do"""
    v = np.arange(nv, dtype=np.int64)
    j0 = (v // 1024) % N_JOINTS
    joints = np.stack([j0, (j0 + 1) % N_JOINTS, np.zeros_like(v), np.zeros_like(v)], axis=1).astype(np.uint16)
    a = ((v % 1024).astype(np.float32) + np.float32(0.5)) / np.float32(1024.0)
    weights = np.stack([a, np.float32(1.0) - a, np.zeros_like(a), np.zeros_like(a)], axis=1).astype(np.float32)
    return joints, weights


def pose(np, k):
    """64 joint matrices near the identity: a turn about y and a shift, both small (the tree is refitted, as for a frame of an animation), different for every k"""
    m = np.zeros((N_JOINTS, 3, 4))
    for j in range(N_JOINTS):
        a = 0.004 * (k + 1) * np.sin(1.0 + j)
        c, s = np.cos(a), np.sin(a)
        m[j, :, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
        m[j, :, 3] = 0.002 * (k + 1) * np.array([np.cos(j), 0.0, np.sin(2.0 * j)])
    return m.astype(np.float32).reshape(N_JOINTS, 12)


def moved_transforms(np, sc, k):
    o2w, w2o = np.array(sc["object_to_world"], np.float32).reshape(-1, 12), np.array(sc["world_to_object"], np.float32).reshape(-1, 12)
    if k:  # every instance a little along x (world_to_object to first order: timing only)
        o2w[:, 3] += np.float32(0.002 * k)
        w2o[:, 3] -= np.float32(0.002 * k) * w2o[:, 0]
    return o2w, w2o


def setup(np):
    import fredholm_amd as F
    sc = scene()
    r = F.Renderer(0)
    r.load_scene({k: v for k, v in sc.items() if k not in ("joints", "weights", "n_joints", "joint_matrices")})
    r.build_ias()
    nv = np.asarray(sc["vertices"]).reshape(-1, 3).shape[0]
    r.set_skin(*skin(np, nv), N_JOINTS)
    return r, sc, nv


def trace(args):
    import numpy as np
    r, sc, nv = setup(np)
    for k in range(args.poses):
        r.set_joint_matrices(pose(np, k))
        r.build_ias()
    r.wait_for_completion()
    print(json.dumps({"vertices": nv, "faces": int(np.asarray(sc["indices"]).reshape(-1, 3).shape[0]), "poses": args.poses}))
    r.close()


def calls(args):
    import numpy as np
    r, sc, nv = setup(np)
    r.set_joint_matrices(pose(np, 100))  # warm-up of both paths
    r.build_ias()
    r.set_transforms(*moved_transforms(np, sc, 100))
    r.build_ias()
    t_pose, t_xform = [], []
    for k in range(args.poses):
        pal = pose(np, k)
        t0 = time.perf_counter()
        r.set_joint_matrices(pal)
        r.build_ias()
        t_pose.append(1e3 * (time.perf_counter() - t0))
        xf = moved_transforms(np, sc, k)
        t0 = time.perf_counter()
        r.set_transforms(*xf)
        r.build_ias()
        t_xform.append(1e3 * (time.perf_counter() - t0))
    rec = {"scene": "configs[3] asset, two-joint weights on every vertex, %d joints" % N_JOINTS, "vertices": nv, "faces": int(np.asarray(sc["indices"]).reshape(-1, 3).shape[0]),
           "poses": args.poses, "set_joint_matrices_plus_bvh_build_ms": {"median": statistics.median(t_pose), "all": t_pose},
           "set_transforms_plus_bvh_build_ms": {"median": statistics.median(t_xform), "all": t_xform},
           "calls_source": "wall clock of the two synchronised calls, alternating on one context; both calls end in transform_faces and a refit of the tree"}
    r.close()
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in rec.items() if k.endswith("_ms")}))


def merge(args):
    rec = json.load(open(args.calls))
    per = {"k_skin_vertices": [], "k_face_records": []}
    for row in csv.DictReader(open(args.trace)):
        for name in per:
            if name in row["Kernel_Name"]:
                per[name].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    # the dispatches of the poses: the last `poses` of each kernel (k_face_records also runs at the upload)
    n = rec["poses"]
    rec["kernels_us"] = {name: {"dispatches": len(v), "median_of_the_poses": statistics.median(v[-n:]), "of_the_poses": v[-n:]} for name, v in per.items() if v}
    rec["kernels_source"] = "rocprofv3 --kernel-trace, no counters, one run of `trace`"
    if "k_skin_vertices" in rec["kernels_us"] and "k_face_records" in rec["kernels_us"]:
        a, b = rec["kernels_us"]["k_skin_vertices"]["median_of_the_poses"], rec["kernels_us"]["k_face_records"]["median_of_the_poses"]
        rec["verdict"] = "k_skin_vertices %s k_face_records on this asset (%.1f us against %.1f us)" % ("at or below" if a <= b else "above", a, b)
    if args.bench:
        rec["bench_against_parent"] = json.load(open(args.bench))
    json.dump(rec, open(args.out, "w"), indent=1)
    print(rec.get("verdict", "no kernels found in the trace"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("trace", "calls", "merge"))
    ap.add_argument("--poses", type=int, default=8)
    ap.add_argument("--calls", default="")
    ap.add_argument("--trace", default="")
    ap.add_argument("--bench", default="")
    ap.add_argument("--out", default="skinning_bench.json")
    args = ap.parse_args()
    {"trace": trace, "calls": calls, "merge": merge}[args.mode](args)


if __name__ == "__main__":
    main()
