"""Numpy restatement of the mesh-finishing contracts (pings_amd/csrc/mesh.hip): the oracle of
tests/test_mesh_ops.py.  Plain loops, `np.unique` and `np.add.at`; the normals in fp64 (or any dtype, for the test's
own fp32 error estimate).

The device code stands in for Open3D's `remove_duplicated_vertices`, `cluster_connected_triangles`,
`remove_triangles_by_mask` and `compute_vertex_normals`.  Open3D cannot be imported where these tests run, so what is
compared against is a reading of its source, which comes down to four points, each in ONE function here so that each
can be changed if the reading proves wrong:
  * a weld keeps the first occurrence of every group                     -> `weld`
  * cluster adjacency is by shared edge, ids in BFS order from the lowest unvisited face -> `cluster_triangles`
  * vertex normals are area-weighted (unnormalised face cross products)  -> `face_normals`
  * the normal of a vertex with a zero sum is (0, 0, 1)                  -> `vertex_normals`
"""
from __future__ import annotations

from collections import defaultdict, deque

import numpy as np


def weld_key(verts):
    """Equality of the weld: fp32 compare per coordinate, so -0 is +0; the caller keeps non-finite vertices apart."""
    v = np.ascontiguousarray(verts, dtype=np.float32) + np.float32(0.0)      # -0 + 0 = +0
    return v.view(np.uint32)


def weld(verts, faces):
    """-> (verts, faces, remap).  First occurrence kept, kept vertices in their original order, no face removed."""
    verts = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    keys = weld_key(verts)
    finite = np.isfinite(verts).all(axis=1)
    first, remap, keep = {}, np.empty(len(verts), np.int64), []
    for i in range(len(verts)):
        k = tuple(keys[i]) if finite[i] else ("own", i)
        if k not in first:
            first[k] = len(keep)
            keep.append(i)
        remap[i] = first[k]
    return verts[keep], remap[faces], remap


def face_edges(face):
    a, b, c = (int(x) for x in face)
    return [(min(a, b), max(a, b)), (min(b, c), max(b, c)), (min(c, a), max(c, a))]


def cluster_triangles(faces):
    """-> (labels [F], counts [K]).  Faces sharing an undirected edge key are adjacent ((a, a) of a degenerate face
    included); breadth-first from the lowest unvisited face, clusters numbered in that order."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    by_edge = defaultdict(list)
    for f, face in enumerate(faces):
        for e in set(face_edges(face)):
            by_edge[e].append(f)
    labels, counts = np.full(len(faces), -1, np.int64), []
    for start in range(len(faces)):
        if labels[start] >= 0:
            continue
        k, n, queue = len(counts), 0, deque([start])
        labels[start] = k
        while queue:
            f = queue.popleft()
            n += 1
            for e in face_edges(faces[f]):
                for g in by_edge[e]:
                    if labels[g] < 0:
                        labels[g] = k
                        queue.append(g)
        counts.append(n)
    return labels, np.asarray(counts, np.int64)


def drop_small_clusters(faces, min_tri):
    """The reference removes a face iff its cluster has fewer than `min_tri` faces; kept faces stay in order."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    labels, counts = cluster_triangles(faces)
    return faces[counts[labels] >= min_tri] if len(faces) else faces


def face_normals(verts, faces, dtype=np.float64):
    """Unnormalised (v1 - v0) x (v2 - v0) in `dtype`, component by component as the kernel writes it."""
    t = np.asarray(verts).astype(dtype)[np.asarray(faces, dtype=np.int64).reshape(-1, 3)]
    u, w = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    return np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1],
                     u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                     u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1).astype(dtype)


def normal_sums(verts, faces, dtype=np.float64):
    """Per vertex the sum of its corners' face normals, ascending face index, then corner (what `np.add.at` does over
    the row-major corner list)."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    s = np.zeros((len(verts), 3), dtype)
    np.add.at(s, faces.reshape(-1), np.repeat(face_normals(verts, faces, dtype), 3, axis=0))
    return s


def vertex_normals(verts, faces, dtype=np.float64):
    s = normal_sums(verts, faces, dtype)
    with np.errstate(all="ignore"):
        length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1] + s[:, 2] * s[:, 2]).astype(dtype)).astype(dtype)
        n = (s / length[:, None]).astype(dtype)
    bad = ~(length > 0) | ~np.isfinite(n).all(axis=1)
    n[bad] = (0.0, 0.0, 1.0)
    return n


def compact_vertices(verts, faces):
    """-> (verts, faces, remap) without the vertices no face names; remap is -1 for a dropped vertex."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    used = np.zeros(len(verts), bool)
    used[faces.reshape(-1)] = True
    remap = np.where(used, np.cumsum(used) - 1, -1).astype(np.int64)
    return np.asarray(verts)[used], remap[faces], remap


def transform(verts, normals, T):
    """Open3D's `transform`: points through the 4x4 in fp64 (rounded once to fp32 here), normals through its 3x3."""
    T = np.asarray(T, dtype=np.float64)
    rot = lambda x: x[:, 0:1] * T[:3, 0] + x[:, 1:2] * T[:3, 1] + x[:, 2:3] * T[:3, 2]     # left to right, no matmul
    v = (rot(np.asarray(verts, np.float64)) + T[:3, 3]).astype(np.float32)
    n = None if normals is None else rot(np.asarray(normals, np.float64)).astype(np.float32)
    return v, n
