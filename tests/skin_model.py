"""The skinning arithmetic of include/fredholm_hip.h (under fh_skin_desc) restated in numpy float32 from the header's text: every product and every sum is one
float32 operation, in the order the header writes them.  What tests/test_skinning_host.py and tests/test_gpu_skinning.py hold csrc/fh_skin.h and k_skin_vertices to,
bit for bit."""
import numpy as np

f32 = np.float32


def _dot(a, b):
    """a.x * b.x + a.y * b.y + a.z * b.z, left to right; a, b [n, 3]"""
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def blend(palette, joints, weights):
    """B [n, 12] of the vertices given (all of them weighted)"""
    J = np.ascontiguousarray(palette, f32).reshape(-1, 12)[joints.astype(np.int64)]  # [n, 4, 12]
    w = np.ascontiguousarray(weights, f32)[:, :, None]
    return ((w[:, 0] * J[:, 0] + w[:, 1] * J[:, 1]) + w[:, 2] * J[:, 2]) + w[:, 3] * J[:, 3]


def pose(palette, joints, weights, vertices, normals):
    """(posed vertices, posed normals), [n, 3] float32 each"""
    joints = np.asarray(joints).reshape(-1, 4)
    weights = np.ascontiguousarray(weights, f32).reshape(-1, 4)
    p = np.ascontiguousarray(vertices, f32).reshape(-1, 3)
    n = np.ascontiguousarray(normals, f32).reshape(-1, 3)
    out_p, out_n = p.copy(), n.copy()
    k = np.flatnonzero(~(weights == 0).all(axis=1))  # all four weights exactly 0: the bind bits
    if k.size == 0:
        return out_p, out_n
    with np.errstate(all="ignore"):
        B = blend(palette, joints[k], weights[k]).reshape(-1, 3, 4)
        pk, nk = p[k], n[k]
        out_p[k] = np.stack([((B[:, r, 0] * pk[:, 0] + B[:, r, 1] * pk[:, 1]) + B[:, r, 2] * pk[:, 2]) + B[:, r, 3] * f32(1.0) for r in range(3)], axis=1)
        L0, L1, L2 = B[:, 0, :3], B[:, 1, :3], B[:, 2, :3]
        C0, C1, C2 = _cross(L1, L2), _cross(L2, L0), _cross(L0, L1)
        m = np.stack([_dot(C0, nk), _dot(C1, nk), _dot(C2, nk)], axis=1)
        m = np.where((_dot(L0, C0) < 0)[:, None], -m, m)
        ln, lm = np.sqrt(_dot(nk, nk)), np.sqrt(_dot(m, m))
        s = ln / lm
        posed = m * s[:, None]
        keep = ~((lm > 0) & np.isfinite(lm))
        out_n[k] = np.where(keep[:, None], nk, posed)
    return out_p, out_n


def normal_float64(palette, joints, weights, normals):
    """the direction of the posed normal from a float64 evaluation of the inverse transpose of the float64 blend of the same float32 inputs (weighted vertices only)"""
    J = np.asarray(palette, np.float64).reshape(-1, 12)[np.asarray(joints).reshape(-1, 4).astype(np.int64)]
    w = np.asarray(weights, np.float64).reshape(-1, 4)[:, :, None]
    B = (w * J).sum(axis=1).reshape(-1, 3, 4)
    L = B[:, :, :3]
    m = np.einsum("nij,nj->ni", np.linalg.inv(L).transpose(0, 2, 1), np.asarray(normals, np.float64).reshape(-1, 3))
    return m / np.linalg.norm(m, axis=1, keepdims=True), np.linalg.cond(L)


def random_rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def random_palette(rng, n_joints, scales=(0.7, 1.4)):
    """n_joints affine 3 x 4 matrices, float32 [n_joints, 12]: a rotation times a diagonal scale drawn from `scales` per axis, and a translation"""
    out = np.zeros((n_joints, 3, 4))
    for k in range(n_joints):
        out[k, :, :3] = random_rotation(rng) @ np.diag(rng.uniform(scales[0], scales[1], 3)) @ random_rotation(rng)
        out[k, :, 3] = rng.uniform(-1.0, 1.0, 3)
    return out.astype(f32).reshape(n_joints, 12)


def random_vertices(rng, n, n_joints, unskinned_share=0.2):
    """joints [n, 4] uint16 (n_joints - 1 in use), weights [n, 4] float32 (two to four influences that sum to 1; a share of the vertices with four zero weights and
    arbitrary joint indices), positions and unit normals [n, 3] float32"""
    joints = rng.integers(0, n_joints, (n, 4)).astype(np.uint16)
    w = rng.uniform(0.0, 1.0, (n, 4)) * (rng.uniform(size=(n, 4)) < 0.7)
    w[:, 0] += 0.05
    w = (w / w.sum(axis=1, keepdims=True)).astype(f32)
    zero = rng.uniform(size=n) < unskinned_share
    w[zero] = 0.0
    joints[zero] = rng.integers(0, 65536, (int(zero.sum()), 4)).astype(np.uint16)  # never read
    joints[np.flatnonzero(~zero)[-1], rng.integers(0, 4)] = n_joints - 1
    p = rng.uniform(-2.0, 2.0, (n, 3)).astype(f32)
    nr = rng.normal(size=(n, 3))
    nr = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(f32)
    return joints, w, p, nr
