"""The mesh-finishing oracle (tests/mesh_ref.py) checked against independent facts, on the CPU: clusters against scipy's
connected components, the weld by closing a surface that marching cubes produced in two halves, normals by geometry."""
import numpy as np
import pytest

import mc_ref
import mesh_ref
from test_mc import euler, noise, sphere, unbalanced


def two_halves(vol):
    """Marching cubes on vol[:h + 1] and vol[h:], the second shifted back along x: the two chunks share the plane x = h,
    where their vertices have the same bits (x = h + 0 exactly, y and z from the same values)."""
    h = vol.shape[0] // 2
    va, fa = mc_ref.marching_cubes(vol[:h + 1])
    vb, fb = mc_ref.marching_cubes(vol[h:])
    vb = vb + np.array([h, 0, 0], np.float32)
    return (va, fa), (vb, fb)


def concat(parts):
    off, vs, fs = 0, [], []
    for v, f in parts:
        vs.append(np.asarray(v, np.float32))
        fs.append(np.asarray(f, np.int64) + off)
        off += len(v)
    return np.concatenate(vs), np.concatenate(fs)


def partition(labels):
    groups = {}
    for f, l in enumerate(labels):
        groups.setdefault(int(l), []).append(f)
    return sorted(groups.values())


def scipy_components(faces):
    """Face adjacency from the edge lists alone: a sparse face x edge incidence B, components of B B^T."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    faces = np.asarray(faces, np.int64)
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    e.sort(axis=1)
    _, eid = np.unique(e, axis=0, return_inverse=True)
    eid = eid.reshape(-1)
    f = np.tile(np.arange(len(faces)), 3)
    B = coo_matrix((np.ones(len(f)), (f, eid)), shape=(len(faces), eid.max() + 1)).tocsr()
    return connected_components(B @ B.T, directed=False)[1]


def strip(n):
    """n triangles in one chain: face i = (i, i + 1, i + 2)."""
    i = np.arange(n, dtype=np.int64)
    return np.stack([i, i + 1, i + 2], axis=1)


CLUSTER_CASES = {
    "strip": lambda: strip(200),
    "isolated": lambda: np.arange(3 * 50, dtype=np.int64).reshape(-1, 3),
    "fans_touching": lambda: np.array([[0, 1, 2], [0, 2, 3], [0, 4, 5], [0, 5, 6]], np.int64),
    "five_on_an_edge": lambda: np.array([[0, 1, k] for k in range(2, 7)], np.int64),
    "duplicate_degenerate": lambda: np.array([[0, 1, 2], [0, 1, 2], [3, 3, 4], [4, 5, 5], [6, 6, 7], [6, 7, 8]], np.int64),
    "noise": lambda: mesh_ref.weld(*concat(two_halves(noise(20))))[1],
}


@pytest.mark.parametrize("case", list(CLUSTER_CASES))
def test_clusters_agree_with_scipy_as_a_partition(case):
    faces = CLUSTER_CASES[case]()
    labels, counts = mesh_ref.cluster_triangles(faces)
    assert partition(labels) == partition(scipy_components(faces))
    assert np.array_equal(counts, np.bincount(labels))
    firsts = [np.flatnonzero(labels == k)[0] for k in range(len(counts))]
    assert firsts == sorted(firsts) and labels[0] == 0               # ids in order of the smallest face index


def test_clusters_of_the_small_cases():
    assert mesh_ref.cluster_triangles(CLUSTER_CASES["fans_touching"]())[1].tolist() == [2, 2]
    assert mesh_ref.cluster_triangles(CLUSTER_CASES["five_on_an_edge"]())[1].tolist() == [5]
    assert mesh_ref.cluster_triangles(CLUSTER_CASES["duplicate_degenerate"]())[0].tolist() == [0, 0, 1, 2, 3, 3]
    assert mesh_ref.drop_small_clusters(CLUSTER_CASES["duplicate_degenerate"](), 2).tolist() == [[0, 1, 2], [0, 1, 2],
                                                                                                   [6, 6, 7], [6, 7, 8]]


@pytest.mark.parametrize("field,counts", [(sphere, (712, 648, 1296, 2588)), (lambda: noise(20), (None, None, 6516, 14152))])
def test_weld_closes_a_surface_made_in_two_halves(field, counts):
    vol = field()
    (va, fa), (vb, fb) = two_halves(vol)
    wv, wf = mc_ref.marching_cubes(vol)
    v, f, remap = mesh_ref.weld(*concat([(va, fa), (vb, fb)]))
    if counts[0] is not None:
        assert (len(va), len(vb)) == counts[:2]
    assert (len(wv), len(wf)) == counts[2:]
    assert (len(v), len(f)) == (len(wv), len(wf))
    assert unbalanced(f) == 0                                        # closed
    assert len(remap) == len(va) + len(vb) and np.array_equal(v[remap], np.concatenate([va, vb]))
    assert np.array_equal(np.unique(remap, return_index=True)[1], np.flatnonzero(np.r_[True, np.diff(np.maximum.accumulate(remap)) > 0]))
    if field is sphere:
        assert euler(v, f) == 2
        # the same surface: a one-to-one match of the vertices (the shift h + (i + t) rounds once more than
        # (h + i) + t: two ulp of 24 away from the seam, none on it) and, through it, the same set of faces
        from scipy.spatial import cKDTree

        d, to_whole = cKDTree(wv.astype(np.float64)).query(v.astype(np.float64))
        assert d.max() <= 2 * np.spacing(np.float32(24)) and len(set(to_whole.tolist())) == len(wv)
        first = lambda a: np.take_along_axis(a, (a.argmin(1)[:, None] + np.arange(3)) % 3, axis=1)   # winding kept
        key = lambda a: sorted(map(tuple, first(a).tolist()))
        assert key(to_whole[f]) == key(wf)


def test_weld_rules():
    nan = np.float32("nan")
    v = np.array([[0, 0, 0], [1, 2, 3], [-0.0, 0, 0], [nan, 0, 0], [nan, 0, 0], [1, 2, 3], [np.inf, 0, 0], [np.inf, 0, 0]],
                 np.float32)
    f = np.array([[0, 2, 5], [3, 4, 1]], np.int64)
    wv, wf, remap = mesh_ref.weld(v, f)
    assert remap.tolist() == [0, 1, 0, 2, 3, 1, 4, 5]
    assert wf.tolist() == [[0, 0, 1], [2, 3, 1]] and len(wv) == 6     # a face may become degenerate and stays


def test_normals_of_the_sphere_are_radial():
    v, f = mc_ref.marching_cubes(sphere())
    n = mesh_ref.vertex_normals(v, f)
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-12)
    r = v.astype(np.float64) - (24 - 1) / 2
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    ang = np.arccos(np.clip(np.abs((n * r).sum(1)), 0, 1))
    assert ang.max() <= 0.2
    s = np.sign((n * r).sum(1))
    assert np.all(s == s[0])                                         # one consistent side


def test_normals_fallback():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 1]], np.int64)                   # the two faces cancel exactly
    assert mesh_ref.vertex_normals(v, f).tolist() == [[0, 0, 1]] * 4
    assert mesh_ref.vertex_normals(v, f[:1]).tolist() == [[0, 0, 1]] * 4   # +z here anyway; the unreferenced one by rule
    assert mesh_ref.vertex_normals(v, f[1:])[:3].tolist() == [[0, 0, -1]] * 3
