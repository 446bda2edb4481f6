"""numpy restatement of the mesh surface sampler (pings_amd/csrc/mesh_sample.hip): the contract that
`mesh_ops.sample_surface` and `eval_ops.eval_mesh` are bit-equal to.  Every fp64 operation is written out in the order
the kernel performs it (numpy evaluates one operation at a time, so nothing is contracted).  Plain on purpose;
test_mesh_sample_ref.py checks it against properties worked out by hand."""
from __future__ import annotations

import numpy as np

import eval_ref

UNIT_BITS, SUM_BITS = 32, 62                   # area quantum 2^-32 m^2; F * cap <= 2^62
ST_INDEX, ST_NONFINITE, ST_AREA_CAP = 16, 32, 64
GOLDEN, MIX1, MIX2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def area_cap(F: int) -> int:
    """The largest quantised area of one triangle among F, in quanta."""
    return (1 << SUM_BITS) // F


def _inside(v, box):
    """[..., 3] fp32 vertices against an inclusive fp64 box (lo, hi)."""
    v = np.asarray(v, np.float32).astype(np.float64)
    return ((v >= np.asarray(box[0], np.float64)) & (v <= np.asarray(box[1], np.float64))).all(-1)


def areas_q(verts, faces, box=None):
    """-> (q int64 [F], status): the quantised area of every triangle, 0 for one that is cropped, names a vertex outside
    [0, V), has a non-finite vertex or exceeds the cap (the last three set their status bit)."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    V, F = len(verts), len(faces)
    q = np.zeros(F, np.int64)
    if F == 0:
        return q, 0
    status = 0
    named = ((faces >= 0) & (faces < V)).all(1)
    if not named.all():
        status |= ST_INDEX
    tri = verts[np.where(named[:, None], faces, 0)] if V else np.zeros((F, 3, 3), np.float32)     # [F, 3, 3]
    finite = np.isfinite(tri).all((1, 2))
    if (named & ~finite).any():
        status |= ST_NONFINITE
    live = named & finite
    if box is not None:
        live &= _inside(tri, box).all(1)
    v = tri.astype(np.float64)
    with np.errstate(all="ignore"):
        e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        scaled = 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz) * float(1 << UNIT_BITS)
        fits = scaled <= float(area_cap(F))
    if (live & ~fits).any():
        status |= ST_AREA_CAP
    live &= fits
    q[live] = np.rint(scaled[live]).astype(np.int64)
    return q, status


def bounds(q, n: int):
    """llrint(Q_t * n / Q) per triangle: the number of points owned by triangles 0..t.  Q > 0."""
    Q = np.cumsum(np.asarray(q, np.int64))
    return np.rint(Q.astype(np.float64) * float(n) / float(Q[-1])).astype(np.int64)


def owners(q, n: int):
    """-> int32 [n]: the triangle of every point, the first t with bounds[t] > i; empty when no triangle has area."""
    q = np.asarray(q, np.int64)
    if len(q) == 0 or int(q.sum()) == 0 or n == 0:
        return np.zeros(0, np.int32)
    return np.searchsorted(bounds(q, n), np.arange(n, dtype=np.int64), side="right").astype(np.int32)


def uniforms(seed: int, idx):
    """splitmix64 keyed on (seed, i) -> (u1, u2), both exact multiples of 2^-32 in [0, 1)."""
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) % (1 << 64)) + (np.asarray(idx).astype(np.uint64) + np.uint64(1)) * GOLDEN
        z = (z ^ (z >> np.uint64(30))) * MIX1
        z = (z ^ (z >> np.uint64(27))) * MIX2
        z = z ^ (z >> np.uint64(31))
    u1 = (z >> np.uint64(32)).astype(np.float64) * 2.0 ** -32
    u2 = (z & np.uint64(0xFFFFFFFF)).astype(np.float64) * 2.0 ** -32
    return u1, u2


def sample(verts, faces, n: int, seed: int = 0, box=None):
    """-> (points fp32 [count, 3], tri int32 [count], count, status) with count = n, or 0 when no triangle has area."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    q, status = areas_q(verts, faces, box)
    tri = owners(q, n)
    if len(tri) == 0:
        return np.zeros((0, 3), np.float32), tri, 0, status
    u1, u2 = uniforms(seed, np.arange(n, dtype=np.int64))
    s = np.sqrt(u1)
    a, b, c = (1.0 - s)[:, None], (s * (1.0 - u2))[:, None], (s * u2)[:, None]
    v = verts[faces[tri]].astype(np.float64)                              # [n, 3, 3]
    p = (a * v[:, 0] + b * v[:, 1]) + c * v[:, 2]
    return p.astype(np.float32), tri, n, status


def crop_faces(verts, faces, lo, hi):
    """Open3D's crop on the face list: the faces whose three vertices lie in the inclusive box, in order."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    return faces[_inside(verts, (lo, hi))[faces].all(1)]


def target_box(trgt, down_sample_res):
    """The target's bounding box, z widened by down_sample_res at both ends, in fp64 from the fp32 cloud."""
    t = np.asarray(trgt, np.float32).astype(np.float64).reshape(-1, 3)
    lo, hi = t.min(0), t.max(0)
    lo[2] -= down_sample_res
    hi[2] += down_sample_res
    return lo, hi


def eval_mesh_ref(verts, faces, trgt, down_sample_res=0.02, threshold=0.05, truncation_acc=0.5, truncation_com=0.5,
                  gt_bbx_mask_on=True, mesh_sample_point=20000000, seed=0):
    """eval_mesh: box, sample, then the fp64 restatement of eval_pair (tests/eval_ref.py)."""
    box = target_box(trgt, down_sample_res) if gt_bbx_mask_on else None
    pts, _, _, _ = sample(verts, faces, mesh_sample_point, seed, box)
    return eval_ref.eval_pair(pts, np.asarray(trgt, np.float32), down_sample_res, threshold, truncation_acc,
                              truncation_com)
