"""Skeletal skinning without a GPU: csrc/fh_skin.h compiled for the host (with -fsanitize=address,undefined) into a stand-alone program (tests/cpp/skin_host.cpp)
whose posed positions and normals must equal, bit for bit, the numpy float32 restatement of what include/fredholm_hip.h states under fh_skin_desc
(tests/skin_model.py); the direction of the posed normals against float64; and every refusal of csrc/skin_plan_host.h with its message."""
import os
import struct
import subprocess

import numpy as np
import pytest

import skin_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def _compile(d, name, extra=()):
    exe = d / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", *SAN, *extra, "-I" + os.path.join(ROOT, "fredholm_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def skin_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("skin_host")
    exe = _compile(d, "skin_host")

    def run(palette, joints, weights, p, n):
        palette = np.ascontiguousarray(palette, f32).reshape(-1, 12)
        nv = len(p)
        blob = struct.pack("<I", len(palette)) + palette.tobytes() + struct.pack("<I", nv) + np.ascontiguousarray(joints, np.uint16).tobytes() + \
            np.ascontiguousarray(weights, f32).tobytes() + np.ascontiguousarray(p, f32).tobytes() + np.ascontiguousarray(n, f32).tobytes()
        (d / "in.bin").write_bytes(blob)
        r = subprocess.run([str(exe), str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        raw = np.frombuffer((d / "out.bin").read_bytes(), dtype=f32)
        assert raw.size == 6 * nv
        return raw[:3 * nv].reshape(nv, 3), raw[3 * nv:].reshape(nv, 3)
    return run


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _cases():
    """(name, palette, joints, weights, positions, normals, well conditioned)"""
    rng = np.random.default_rng(2024)
    out = []
    for nj in (1, 2, 300):
        out.append(("random affine palette of %d joints" % nj, M.random_palette(rng, nj), *M.random_vertices(rng, 400, nj), True))
    pal = M.random_palette(rng, 5)
    j, w, p, n = M.random_vertices(rng, 300, 5, unskinned_share=0.0)
    out.append(("weights that do not sum to 1", pal, j, (w * rng.uniform(0.2, 1.9, (300, 1))).astype(f32), p, n, True))
    mirror = pal.copy().reshape(5, 3, 4)
    mirror[:, :, 0] = -mirror[:, :, 0]  # every joint mirrors; one joint per vertex, so every blend does
    one = np.zeros_like(w)
    one[:, 0] = 1.0
    out.append(("mirroring joint matrices (det < 0)", mirror.reshape(5, 12), j, one, p, n, True))
    singular = pal.copy().reshape(5, 3, 4)
    singular[0, :, :3] = np.outer([1.0, 2.0, -1.0], [0.5, 0.25, 2.0])  # rank 1: the cofactor matrix is zero
    singular[1, :, :3] = 0.0
    singular[2, 2, :3] = singular[2, 1, :3]                             # rank 2: a cofactor matrix of rank 1
    out.append(("singular joint matrices (normal fallback)", singular.reshape(5, 12), (j % 3).astype(np.uint16), one, p, n, False))
    out.append(("a strongly non-uniform scale", M.random_palette(rng, 4, scales=(1e-3, 1e3)), *M.random_vertices(rng, 300, 4), False))
    j, w, p, n = M.random_vertices(rng, 300, 5)
    n[::2] = 0.0
    n[1::2] *= f32(3.0)
    out.append(("bind normals of length 0 and 3", pal, j, w, p, n, True))
    return out


CASES = _cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_header_on_the_host_equals_the_restatement_bit_for_bit(skin_host, case):
    name, pal, j, w, p, n, _ = case
    got_p, got_n = skin_host(pal, j, w, p, n)
    want_p, want_n = M.pose(pal, j, w, p, n)
    assert (_bits(got_p) == _bits(want_p)).all() and (_bits(got_n) == _bits(want_n)).all(), name
    zero = (w == 0).all(axis=1)
    assert (_bits(got_p[zero]) == _bits(p[zero])).all() and (_bits(got_n[zero]) == _bits(n[zero])).all()  # the bind bits
    if name.startswith("singular"):
        dead = ~zero & (j[:, 0] < 2)
        assert dead.any() and (_bits(got_n[dead]) == _bits(n[dead])).all()  # the cofactor matrix is zero: the bind normal is kept
    if name.startswith("bind normals"):
        assert (got_n[::2] == 0).all()
    if not name.startswith(("singular", "a strongly")):  # the bind normal's length is kept: three roundings of a value near it
        ln, lg = np.linalg.norm(n.astype(np.float64), axis=1), np.linalg.norm(got_n.astype(np.float64), axis=1)
        assert np.abs(lg - ln).max() <= 4e-7 * 3.0


COND_CAP = 8.0         # condition number (2-norm) of the blended 3 x 3 up to which a case counts as well conditioned
MEASURED_ANGLE = 3.6e-7  # radians: the restatement's largest angle to the float64 inverse transpose over the well-conditioned inputs below


def _angle(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), (a * b).sum(axis=1))


def test_the_posed_normals_point_where_float64_says(skin_host):
    """Well-conditioned cases only: vertices whose blended 3 x 3 has a condition number of at most COND_CAP = 8.  The numpy restatement's largest angle to a float64
    evaluation of the inverse transpose on these inputs was measured here as 3.59e-7 rad (1570 normals); the program's normals (which the test above holds to the restatement's
    bits) must stay within 4 x that -- the rounding of a handful of float32 products and nothing else.  A mirrored joint agrees in sign: its angle is near 0, not pi."""
    worst, worst_model, seen_mirror, n_checked = 0.0, 0.0, False, 0
    for name, pal, j, w, p, n, well in CASES:
        if not well:
            continue
        k = np.flatnonzero(~(w == 0).all(axis=1) & (np.abs(n).sum(axis=1) > 0))
        ref, cond = M.normal_float64(pal, j[k], w[k], n[k])
        k, ref = k[cond <= COND_CAP], ref[cond <= COND_CAP]
        got = skin_host(pal, j, w, p, n)[1][k]
        model = M.pose(pal, j, w, p, n)[1][k]
        ang = _angle(got, ref)
        worst, worst_model, n_checked = max(worst, float(ang.max())), max(worst_model, float(_angle(model, ref).max())), n_checked + len(k)
        if name.startswith("mirroring"):
            seen_mirror = True
            assert len(k) > 100 and ang.max() < 1e-5
    print("largest angle to float64: program %.3e rad, restatement %.3e rad, over %d normals" % (worst, worst_model, n_checked))
    assert seen_mirror and n_checked > 1000
    assert worst <= 4.0 * MEASURED_ANGLE


# ------------------------------------------------------------------ skin_plan_host.h
def _skin_case(facts, desc):
    """desc: None (clear) or (n_vertices, n_joints, joints or None, weights or None)"""
    blob = struct.pack("<4I", 0, *facts)
    if desc is None:
        return blob + struct.pack("<6I", 0, 0, 0, 0, 0, 0)
    nv, nj, joints, weights = desc
    k = max(len(joints) if joints is not None else 0, len(weights) if weights is not None else 0)
    jd = np.zeros((k, 4), np.uint16) if joints is None else np.ascontiguousarray(joints, np.uint16)
    wd = np.zeros((k, 4), f32) if weights is None else np.ascontiguousarray(weights, f32)
    return blob + struct.pack("<6I", 1, nv, nj, int(joints is not None), int(weights is not None), k) + jd.tobytes() + wd.tobytes()


def _matrix_case(facts, n, m):
    k = 0 if m is None else len(m)
    return struct.pack("<4I", 1, *facts) + struct.pack("<3I", n, int(m is not None), k) + (b"" if m is None else np.ascontiguousarray(m, f32).tobytes())


def test_every_refusal_of_the_skin_plan_with_its_message(tmp_path):
    exe = _compile(tmp_path, "skin_plan_check")
    j = np.array([[0, 1, 2, 2], [2, 0, 0, 0], [9, 9, 9, 9], [1, 1, 1, 1]], np.uint16)
    w = np.array([[0.5, 0.5, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0], [0.2, 0.2, 0.2, 0.2]], f32)
    m = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], f32), (3, 1))
    loaded, skinned = (1, 4, 0), (1, 4, 3)

    def bad(a, at, v):
        a = a.copy()
        a[at] = v
        return a
    cases = [
        (_skin_case((0, 0, 0), (4, 3, j, w)), "fh_set_skin: no scene loaded"),
        (_skin_case((0, 0, 0), None), "fh_set_skin: no scene loaded"),
        (_skin_case(loaded, None), "ok"),
        (_skin_case(loaded, (3, 3, j[:3], w[:3])), "fh_set_skin: n_vertices differs from the uploaded scene's"),
        (_skin_case(loaded, (5, 3, np.tile(j[:1], (5, 1)), np.tile(w[:1], (5, 1)))), "fh_set_skin: n_vertices differs from the uploaded scene's"),
        (_skin_case(loaded, (4, 3, None, w)), "fh_set_skin: null arrays"),
        (_skin_case(loaded, (4, 3, j, None)), "fh_set_skin: null arrays"),
        (_skin_case(loaded, (4, 0, j, w)), "fh_set_skin: n_joints must be in [1, 65536]"),
        (_skin_case(loaded, (4, 65537, j, w)), "fh_set_skin: n_joints must be in [1, 65536]"),
        (_skin_case(loaded, (4, 65536, j, w)), "ok 3"),
        (_skin_case(loaded, (4, 2, j, w)), "fh_set_skin: a joint index of a weighted vertex is outside the palette"),
        (_skin_case(loaded, (4, 3, bad(j, (1, 3), 3), w)), "fh_set_skin: a joint index of a weighted vertex is outside the palette"),  # (its own weight is 0, the vertex's are not)
        (_skin_case(loaded, (4, 3, j, bad(w, (2, 1), np.nan))), "fh_set_skin: a weight is not finite"),
        (_skin_case(loaded, (4, 3, j, bad(w, (0, 0), np.inf))), "fh_set_skin: a weight is not finite"),
        (_skin_case(loaded, (4, 3, j, w)), "ok 3"),            # (vertex 2: indices outside the palette, all weights 0)
        (_skin_case(skinned, (4, 3, j, bad(w, (2, 0), -0.0))), "ok 3"),
        (_skin_case(loaded, (4, 3, j, w * f32(0))), "ok 0"),
        (_matrix_case((0, 0, 0), 3, m), "fh_set_joint_matrices: no scene loaded"),
        (_matrix_case(loaded, 3, m), "fh_set_joint_matrices: no skin set"),
        (_matrix_case(skinned, 3, None), "fh_set_joint_matrices: null arrays"),
        (_matrix_case(skinned, 2, m[:2]), "fh_set_joint_matrices: the matrix count differs from the skin's n_joints"),
        (_matrix_case(skinned, 4, np.tile(m[:1], (4, 1))), "fh_set_joint_matrices: the matrix count differs from the skin's n_joints"),
        (_matrix_case(skinned, 3, bad(m, (2, 11), np.nan)), "fh_set_joint_matrices: a matrix entry is not finite"),
        (_matrix_case(skinned, 3, bad(m, (0, 0), -np.inf)), "fh_set_joint_matrices: a matrix entry is not finite"),
        (_matrix_case(skinned, 3, m), "ok"),
    ]
    (tmp_path / "cases.bin").write_bytes(b"".join(c[0] for c in cases))
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == [c[1] for c in cases]
    # the header is plain C++: no HIP in it
    src = open(os.path.join(ROOT, "fredholm_amd", "csrc", "skin_plan_host.h")).read()
    assert "hip_runtime" not in src and "__global__" not in src


# ------------------------------------------------------------------ the two glTF loaders on the skinned asset
TIMES = (0.0, 0.5, 1.0, 1.75)


@pytest.fixture(scope="module")
def skin_dump(tmp_path_factory):
    """tests/cpp/skin_dump.cpp against include/: the chunks it writes, or ValueError with the loader's message"""
    d = tmp_path_factory.mktemp("skin_dump")
    exe = d / "skin_dump"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "skin_dump.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(gltf, times=TIMES):
        p = subprocess.run([str(exe), str(d / "dump.bin"), str(gltf), *[repr(float(t)) for t in times]], capture_output=True, text=True, timeout=120)
        if p.returncode == 1:
            raise ValueError(p.stderr.strip())
        assert p.returncode == 0, f"skin_dump crashed on {gltf}: {p.returncode}"
        data = (d / "dump.bin").read_bytes()
        chunks, pos = [], 0
        while pos < len(data):
            n = int(np.frombuffer(data, dtype=np.uint64, count=1, offset=pos)[0])
            chunks.append(data[pos + 8:pos + 8 + n])
            pos += 8 + n
        return chunks
    return run


def _python_chunks(gltf, times=TIMES):
    from fredholm_amd.scene import Scene
    S = Scene()
    S.load_model(str(gltf))
    out = [S.m_joints.tobytes(), S.m_weights.tobytes(), np.asarray([v for sk in S.m_skins for v in (sk.base, len(sk.joints))], np.uint32).tobytes()]
    for t in times:
        S.update_animation(t)
        o2w, w2o = S.transforms_3x4()
        out += [S.joint_matrices_3x4().tobytes(), o2w.tobytes(), w2o.tobytes()]
    return out


def test_the_two_loaders_agree_byte_for_byte_on_the_skinned_asset(tmp_path, skin_dump):
    from fredholm_amd import scenes_skinned as S
    from fredholm_amd.scene import Scene
    gltf = tmp_path / "arm.gltf"
    wrote = S.write_arm_gltf(str(gltf))
    got, want = skin_dump(gltf), _python_chunks(gltf)
    names = ["joints", "weights", "palette bases"] + ["%s at t = %g" % (what, t) for t in TIMES for what in ("joint matrices", "o2w", "w2o")]
    assert len(got) == len(want) == len(names)
    for name, a, b in zip(names, got, want):
        assert a == b and len(a) > 0, name
    # ... and with what the generator wrote
    sc = Scene()
    sc.load_model(str(gltf))
    d = sc.as_dict()
    for k in ("vertices", "normals", "texcoords", "indices", "material_ids", "instance_ids", "object_to_world", "world_to_object", "joints", "weights"):
        assert np.asarray(d[k]).dtype == np.asarray(wrote[k]).dtype and np.array_equal(d[k], wrote[k]), k
    assert d["materials"].tobytes() == wrote["materials"].tobytes() and d["n_joints"] == S.ARM_N_JOINTS == sc.n_joints()
    assert [(sk.base, [n.idx for n in sk.joints], sk.mesh_node.idx) for sk in sc.m_skins] == [(0, [2, 3, 4], 1)]
    assert len(sc.m_animations) == 2 and [a.node.idx for a in sc.m_animations] == [3, 4] and sc.m_has_camera_transform  # one record per animated joint
    assert (d["weights"][:36] == 0).all() and (d["weights"][36:].sum(axis=1) == 1).all()
    # the palette against the generator's own float64 matrices.  The keys are float32 quaternions (relative error 6e-8 per component, about 2.4e-7 on an entry of the
    # rotation), the joints sit at most 0.75 from the base, and the palette is rounded to float32 once: 1e-6 bounds it with room
    for t, key in ((0.0, 0), (1.0, 1)):
        sc.update_animation(t)
        ref = S.arm_joint_matrices_float64(S.ARM_KEY_ANGLES[0][key], S.ARM_KEY_ANGLES[1][key]).reshape(-1, 12)
        assert np.abs(sc.joint_matrices_3x4().astype(np.float64) - ref).max() <= 1e-6
        assert not np.array_equal(sc.joint_matrices_3x4()[1], sc.joint_matrices_3x4()[0])
    o2w, _ = sc.transforms_3x4()
    assert np.array_equal(o2w[1, 3::4], np.asarray(S.ARM_BASE, f32))  # the instance's own transform stays the mesh node's


def _edited(tmp_path, name, edit):
    import json
    from fredholm_amd import scenes_skinned as S
    src = tmp_path / "arm_src.gltf"
    if not src.exists():
        S.write_arm_gltf(str(src))
    doc = json.load(open(src))
    edit(doc)
    out = tmp_path / (name + ".gltf")
    json.dump(doc, open(out, "w"))
    return out


def _arm_prim(doc, k=0):
    return doc["meshes"][1]["primitives"][k]["attributes"]


def _set(obj, key, value):
    obj[key] = value


def _two_joint_skin_nobody_uses(doc):
    doc["skins"][0]["joints"] = [2, 3]
    doc["skins"][0].pop("inverseBindMatrices")
    doc["nodes"][1].pop("skin")


REFUSALS = [
    ("joints_only", lambda d: _arm_prim(d).pop("WEIGHTS_0"), "JOINTS_0 and WEIGHTS_0 must come together"),
    ("weights_only", lambda d: _arm_prim(d, 1).pop("JOINTS_0"), "JOINTS_0 and WEIGHTS_0 must come together"),
    ("normalised_weights", lambda d: _set(d["accessors"][_arm_prim(d)["WEIGHTS_0"]], "componentType", 5123), "normalised-integer WEIGHTS_0 is not supported"),
    ("joint_index", lambda d: (_set(d["skins"][0], "joints", [2, 3]), d["skins"][0].pop("inverseBindMatrices")), "joint index outside the skin's joints"),
    ("no_attributes", lambda d: (_arm_prim(d).pop("WEIGHTS_0"), _arm_prim(d).pop("JOINTS_0")), "a primitive of a skinned node has no JOINTS_0 / WEIGHTS_0"),
    ("ibm_count", lambda d: _set(d["accessors"][d["skins"][0]["inverseBindMatrices"]], "count", 2), "inverseBindMatrices must be tightly packed float MAT4, one per joint"),
    ("ibm_type", lambda d: _set(d["accessors"][d["skins"][0]["inverseBindMatrices"]], "type", "VEC4"), "inverseBindMatrices must be tightly packed float MAT4, one per joint"),
    ("ibm_stride", lambda d: _set(d["bufferViews"][d["accessors"][d["skins"][0]["inverseBindMatrices"]]["bufferView"]], "byteStride", 80),
     "inverseBindMatrices must be tightly packed float MAT4, one per joint"),
    ("animated_non_joint", lambda d: _two_joint_skin_nobody_uses(d), "invalid target node"),  # (node 4 is still animated: neither a root nor a joint now)
]


@pytest.mark.parametrize("name,edit,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_each_loader_refusal_is_raised_by_both_loaders(tmp_path, skin_dump, name, edit, message):
    from fredholm_amd.scene import Scene
    gltf = _edited(tmp_path, name, edit)
    with pytest.raises(ValueError, match=message.replace("/", ".")):
        Scene().load_model(str(gltf))
    with pytest.raises(ValueError, match=message.replace("/", ".")):
        skin_dump(gltf)


def test_absent_inverse_bind_matrices_mean_identities_and_no_skins_means_todays_loader(tmp_path, skin_dump):
    from fredholm_amd import scenes_skinned as S
    from fredholm_amd.scene import Scene
    gltf = _edited(tmp_path, "no_ibm", lambda d: d["skins"][0].pop("inverseBindMatrices"))
    assert skin_dump(gltf) == _python_chunks(gltf)
    sc = Scene()
    sc.load_model(str(gltf))
    pal = sc.joint_matrices_3x4().reshape(3, 3, 4)
    assert np.array_equal(pal[:, :, :3], np.tile(np.eye(3, dtype=f32), (3, 1, 1))) and np.array_equal(pal[:, 1, 3], np.asarray([0, 1, 2], f32) * f32(S.ARM_JOINT_SPACING))
    # the asset with `skins` removed and its joint animation kept: the pinned refusal, in both
    plain = tmp_path / "arm_noskins.gltf"
    S.write_arm_gltf(str(plain), skins=False)
    with pytest.raises(ValueError, match="invalid target node"):
        Scene().load_model(str(plain))
    with pytest.raises(ValueError, match="invalid target node"):
        skin_dump(plain)
    # ... and without the animation it loads with no skin and no joints in its dict
    import json
    doc = json.load(open(plain))
    doc.pop("animations")
    json.dump(doc, open(plain, "w"))
    sc = Scene()
    sc.load_model(str(plain))
    assert not sc.m_skins and "joints" not in sc.as_dict() and (sc.m_weights == 0).all() and len(sc.m_weights) == len(sc.m_vertices)
    assert skin_dump(plain, ())[2] == b""
