"""Test asset for skeletal skinning (include/fredholm_hip.h: fh_skin_desc): a bending arm inside the Cornell box.

The arm is a tube of 8 x 12 quads along +y with a chain of three joints -- the root at the tube's base, two children up the tube -- and smooth two-joint weights; one
ring of it emits.  The room (floor, ceiling, three walls, the ceiling light) is a second, unskinned mesh.  arm_scene() gives the flat arrays Renderer.load_scene
takes, with the skin; arm_joint_matrices() the palette of a pose; write_arm_gltf() the same scene as a glTF file with a `skins` array, one animation that turns both
child joints, a camera node and its buffer embedded as base64, and returns the arrays it wrote."""
import base64
import json
import math

import numpy as np

from .native import default_materials
from .scenes import _quad

ARM_SEGMENTS, ARM_RINGS = 8, 12          # quads around, quads along
ARM_RADIUS, ARM_LENGTH = 0.09375, 1.125  # (ring spacing 0.09375: exact in binary)
ARM_JOINT_SPACING = 0.375                # joints at y = 0, 0.375, 0.75 of the tube's object space
ARM_BASE = (0.25, 0.25, -0.25)           # where the mesh node (and the root joint) puts the tube's base
ARM_EMISSIVE_RING = 7
ARM_N_JOINTS = 3
ARM_CAMERA = (0.0, 1.0, 1.0)
# rotation keys of the two child joints about z (radians) at 0, 1, 2 s; keys are 1 s apart because the loaders' interpolation does not divide by the key interval
ARM_KEY_TIMES = (0.0, 1.0, 2.0)
ARM_KEY_ANGLES = ((0.2, -0.5, 0.2), (-0.3, -0.6, -0.3))


def _arm_weights(y):
    """(joints[4], weights[4]) of a vertex at height y: one joint away from the joints' heights, a smoothstep blend of two across each child joint"""
    u = y / ARM_JOINT_SPACING
    for k in (1, 2):
        if u <= k + 0.5:
            x = min(max(u - (k - 0.5), 0.0), 1.0)
            s = x * x * (3.0 - 2.0 * x)
            return (k - 1, k, 0, 0), (1.0 - s, s, 0.0, 0.0)
    return (1, 2, 0, 0), (0.0, 1.0, 0.0, 0.0)


def _arm_mesh():
    """unshared triangles of the tube in its object space: (vertices, normals, ring of each face)"""
    verts, norms, rings = [], [], []

    def corner(i, s):
        a = 2.0 * math.pi * (s % ARM_SEGMENTS) / ARM_SEGMENTS
        return (ARM_RADIUS * math.cos(a), ARM_LENGTH * i / ARM_RINGS, ARM_RADIUS * math.sin(a)), (math.cos(a), 0.0, math.sin(a))
    for i in range(ARM_RINGS):
        for s in range(ARM_SEGMENTS):
            for tri in (((i, s), (i + 1, s), (i + 1, s + 1)), ((i, s), (i + 1, s + 1), (i, s + 1))):  # outward
                for c in tri:
                    p, n = corner(*c)
                    verts.append(p)
                    norms.append(n)
                rings.append(i)
    return np.asarray(verts, np.float32), np.asarray(norms, np.float32), np.asarray(rings)


def arm_scene():
    """The flat scene with its skin: the keys of scenes.cornell_box_instanced() plus joints [n_vertices, 4] uint16, weights [n_vertices, 4] float32 and n_joints.
    Instance 0 is the room (unskinned: zero weights), instance 1 the arm, whose vertices are in the tube's object space."""
    tris, mats = [], []

    def add(q, m):
        tris.extend(q)
        mats.extend([m] * (len(q) // 3))
    # per instance, faces sorted by material (the order a glTF file's primitives give them)
    add(_quad((-1, 0, 1), (1, 0, 1), (1, 0, -1), (-1, 0, -1)), 0)      # floor
    add(_quad((-1, 2, -1), (1, 2, -1), (1, 2, 1), (-1, 2, 1)), 0)      # ceiling
    add(_quad((-1, 0, -1), (1, 0, -1), (1, 2, -1), (-1, 2, -1)), 0)    # back wall
    add(_quad((-1, 0, 1), (-1, 0, -1), (-1, 2, -1), (-1, 2, 1)), 1)    # left wall (red)
    add(_quad((1, 0, -1), (1, 0, 1), (1, 2, 1), (1, 2, -1)), 2)        # right wall (green)
    add(_quad((-0.35, 1.995, -0.3), (0.35, 1.995, -0.3), (0.35, 1.995, 0.3), (-0.35, 1.995, 0.3)), 3)  # light
    room_v = np.asarray(tris, np.float32).reshape(-1, 3)
    p0, p1, p2 = (room_v[k::3].astype(np.float64) for k in range(3))
    fn = np.cross(p1 - p0, p2 - p0)
    fn /= np.linalg.norm(fn, axis=1, keepdims=True)
    room_n = np.repeat(fn.astype(np.float32), 3, axis=0)
    av, an, ring = _arm_mesh()
    order = np.argsort(ring == ARM_EMISSIVE_RING, kind="stable")  # material 4 (the body) first, then 5 (the ring that emits)
    arm_mats = np.where(ring[order] == ARM_EMISSIVE_RING, 5, 4)
    vsel = (3 * order[:, None] + np.arange(3)[None, :]).reshape(-1)
    av, an = av[vsel], an[vsel]
    m = default_materials(6)
    m["metalness"] = 0.0
    m["specular_roughness"] = 0.5
    m["emission"] = 1.0  # (what the glTF readers give every material)
    for k, c in enumerate(((0.73, 0.73, 0.73), (0.65, 0.05, 0.05), (0.12, 0.45, 0.15), (0.78, 0.78, 0.78), (0.25, 0.35, 0.75), (0.8, 0.8, 0.8))):
        m["base_color"][k] = c
    m["emission_color"][3] = (17.0, 12.0, 4.0)
    m["emission_color"][5] = (3.0, 4.0, 6.0)
    v = np.concatenate([room_v, av])
    nv, n_room = v.shape[0], room_v.shape[0]
    joints, weights = np.zeros((nv, 4), np.uint16), np.zeros((nv, 4), np.float32)
    for k in range(n_room, nv):
        joints[k], weights[k] = _arm_weights(float(v[k, 1]))
    nf = nv // 3
    o2w = np.tile(np.asarray([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), (2, 1))
    w2o = o2w.copy()
    o2w[1, 3::4] = ARM_BASE
    w2o[1, 3::4] = -np.asarray(ARM_BASE, np.float32)
    return {"vertices": v, "normals": np.concatenate([room_n, an]), "texcoords": np.tile(np.asarray([[0, 1]], np.float32), (nv, 1)),
            "indices": np.arange(nv, dtype=np.uint32).reshape(nf, 3), "material_ids": np.concatenate([np.asarray(mats), arm_mats]).astype(np.uint32), "materials": m,
            "instance_ids": np.concatenate([np.zeros(n_room // 3), np.ones((nv - n_room) // 3)]).astype(np.uint32), "object_to_world": o2w, "world_to_object": w2o,
            "joints": joints, "weights": weights, "n_joints": ARM_N_JOINTS}


def _rot_z(a):
    m = np.eye(4)
    m[0, 0], m[0, 1], m[1, 0], m[1, 1] = math.cos(a), -math.sin(a), math.sin(a), math.cos(a)
    return m


def _translate(t):
    m = np.eye(4)
    m[:3, 3] = t
    return m


def arm_joint_matrices_float64(a1, a2, scale=1.0):
    """the palette [3, 3, 4] in float64, in the arm's object space, with the child joints turned by a1 and a2 about z (and the whole arm scaled about its base):
    global(joint) * inverseBind per joint, the mesh node's own transform taken off"""
    step = _translate((0.0, ARM_JOINT_SPACING, 0.0))
    g0 = np.diag([scale, scale, scale, 1.0])
    g1 = g0 @ step @ _rot_z(a1)
    g2 = g1 @ step @ _rot_z(a2)
    inv_bind = [_translate((0.0, -ARM_JOINT_SPACING * k, 0.0)) for k in range(3)]
    return np.stack([(g @ ib)[:3] for g, ib in zip((g0, g1, g2), inv_bind)])


def arm_joint_matrices(a1, a2, scale=1.0):
    """... rounded to float32 once: [3, 12]"""
    return arm_joint_matrices_float64(a1, a2, scale).astype(np.float32).reshape(-1, 12)


def write_arm_gltf(path, skins=True):
    """arm_scene() as a glTF file: node 0 the room, node 1 the arm (mesh + skin), nodes 2, 3, 4 the joint chain (2 a root of the scene), node 5 the camera; one
    animation with a rotation and a (constant) translation channel on each child joint -- an animated node's transform is REPLACED by its interpolated keys.
    skins=False leaves the `skins` array and the nodes' `skin` out and keeps the animation.  Returns arm_scene()'s arrays plus the rotation keys as quaternions
    (x, y, z, w) per child joint."""
    sc = arm_scene()
    blob = bytearray()
    views, accessors = [], []

    def add(arr, target, ctype, typ, minmax=False):
        while len(blob) % 4:
            blob.append(0)
        raw = np.ascontiguousarray(arr)
        views.append({"buffer": 0, "byteOffset": len(blob), "byteLength": raw.nbytes, **({"target": target} if target else {})})
        blob.extend(raw.tobytes())
        acc = {"bufferView": len(views) - 1, "componentType": ctype, "count": int(raw.shape[0]), "type": typ}
        if minmax:
            acc["min"], acc["max"] = [float(x) for x in np.atleast_1d(raw.min(axis=0))], [float(x) for x in np.atleast_1d(raw.max(axis=0))]
        accessors.append(acc)
        return len(accessors) - 1

    meshes = []
    for inst in (0, 1):
        prims = []
        faces = np.flatnonzero(sc["instance_ids"] == inst)
        for m in sorted(set(int(x) for x in sc["material_ids"][faces])):
            vid = sc["indices"][faces[sc["material_ids"][faces] == m]].reshape(-1)
            uv = sc["texcoords"][vid].copy()
            uv[:, 1] = np.float32(1.0) - uv[:, 1]  # undone by the loaders
            attrs = {"POSITION": add(sc["vertices"][vid], 34962, 5126, "VEC3", True), "NORMAL": add(sc["normals"][vid], 34962, 5126, "VEC3"), "TEXCOORD_0": add(uv, 34962, 5126, "VEC2")}
            if inst == 1 and skins:
                # local joint indices, as unsigned bytes in the first primitive and unsigned shorts in the second: both forms the loaders read
                attrs["JOINTS_0"] = add(sc["joints"][vid].astype(np.uint8 if m == 4 else np.uint16), 34962, 5121 if m == 4 else 5123, "VEC4")
                attrs["WEIGHTS_0"] = add(sc["weights"][vid], 34962, 5126, "VEC4")
            prims.append({"attributes": attrs, "indices": add(np.arange(len(vid), dtype=np.uint16), 34963, 5123, "SCALAR"), "material": m})
        meshes.append({"primitives": prims})
    step = [0.0, ARM_JOINT_SPACING, 0.0]
    nodes = [{"mesh": 0, "name": "room"}, {"mesh": 1, "name": "arm", "translation": list(ARM_BASE)},
             {"name": "joint0", "translation": list(ARM_BASE), "children": [3]}, {"name": "joint1", "translation": step, "children": [4]}, {"name": "joint2", "translation": step},
             {"camera": 0, "name": "cam", "translation": list(ARM_CAMERA)}]
    samplers, channels, quats = [], [], []
    times = add(np.asarray(ARM_KEY_TIMES, np.float32), None, 5126, "SCALAR", True)
    for node, angles in zip((3, 4), ARM_KEY_ANGLES):
        q = np.asarray([[0.0, 0.0, math.sin(0.5 * a), math.cos(0.5 * a)] for a in angles], np.float32)
        quats.append(q)
        samplers.append({"input": times, "output": add(q, None, 5126, "VEC4"), "interpolation": "LINEAR"})
        channels.append({"sampler": len(samplers) - 1, "target": {"node": node, "path": "rotation"}})
        samplers.append({"input": times, "output": add(np.tile(np.asarray(step, np.float32), (3, 1)), None, 5126, "VEC3"), "interpolation": "LINEAR"})
        channels.append({"sampler": len(samplers) - 1, "target": {"node": node, "path": "translation"}})
    mats = [{"pbrMetallicRoughness": {"baseColorFactor": [float(x) for x in m["base_color"]] + [1.0], "roughnessFactor": float(m["specular_roughness"]), "metallicFactor": float(m["metalness"])},
             "emissiveFactor": [float(x) for x in m["emission_color"]]} for m in sc["materials"]]
    doc = {"asset": {"version": "2.0", "generator": "fredholm_amd.scenes_skinned.write_arm_gltf"}, "scene": 0, "scenes": [{"nodes": [0, 1, 2, 5]}], "nodes": nodes, "meshes": meshes,
           "materials": mats, "animations": [{"samplers": samplers, "channels": channels}], "cameras": [{"type": "perspective", "perspective": {"yfov": 1.0, "znear": 0.01}}]}
    if skins:
        nodes[1]["skin"] = 0
        ibm = np.stack([_translate((0.0, -ARM_JOINT_SPACING * k, 0.0)).T for k in range(3)]).astype(np.float32).reshape(3, 16)  # column-major
        doc["skins"] = [{"joints": [2, 3, 4], "inverseBindMatrices": add(ibm, None, 5126, "MAT4"), "skeleton": 2}]
    doc["accessors"], doc["bufferViews"] = accessors, views
    doc["buffers"] = [{"byteLength": len(blob), "uri": "data:application/octet-stream;base64," + base64.b64encode(bytes(blob)).decode()}]
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
    return dict(sc, rotation_keys=quats)
