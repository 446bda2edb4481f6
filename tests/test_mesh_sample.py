"""Mesh surface sampling on the device (pings_amd/csrc/mesh_sample.hip, mesh_ops.sample_surface, eval_ops.eval_mesh and
crop_intersection) against the numpy restatement tests/mesh_sample_ref.py.  The contract is bit equality:
points, owning triangles and the count of every case are compared byte for byte, so there is no tolerance to derive
except where a test says so."""
import math

import numpy as np
import pytest
import torch

import mesh_sample_ref as ref
from pings_amd import _abi, _lib, eval_ops, mesh_ops

pytestmark = pytest.mark.gpu


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def host(t):
    return t.detach().cpu().numpy()


def run(verts, faces, n, seed=0, box=None):
    """sample_surface -> (points [count, 3], tri [count], count, status) on the host; the operator itself reads nothing."""
    _lib.sync_counts(reset=True)
    s = mesh_ops.sample_surface(dev(verts), dev(faces, torch.int64), n, seed=seed, box=box, return_tri=True)
    assert _lib.sync_counts(reset=True) == {}
    assert s.points.shape == (n, 3) and s.points.dtype == torch.float32 and s.tri.dtype == torch.int32
    count = int(s.count.item())
    assert count in (0, n)
    return host(s.points)[:count], host(s.tri)[:count], count, int(s.status.item())


def check(verts, faces, n, seed=0, box=None):
    """The device sample equals the restatement's bit for bit; -> the restatement's (points, tri, count, status)."""
    got, want = run(verts, faces, n, seed, box), ref.sample(verts, faces, n, seed, box)
    assert got[2] == want[2] and got[3] == want[3]
    assert np.array_equal(got[1], want[1])
    assert got[0].tobytes() == want[0].tobytes()
    return want


def random_mesh(seed, V, F):
    rng = np.random.default_rng(seed)
    faces = np.stack([rng.permutation(V)[:3] for _ in range(F)])          # three different corners: no chance degenerates
    return rng.uniform(-3, 3, (V, 3)).astype(np.float32), faces


# ------------------------------------------------------------------ face-count and point-count edges
def test_one_triangle():
    verts = np.array([[1, 2, 3], [2, 2, 3.5], [1, 4, 2]], np.float32)
    for n in (1, 100):
        _, tri, count, status = check(verts, [[0, 1, 2]], n)
        assert count == n and status == 0 and (tri == 0).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_one_face_past_a_wave(n):
    verts, faces = random_mesh(0, 40, 65)
    _, tri, count, _ = check(verts, faces, n, seed=n)
    assert count == n and (np.diff(tri) >= 0).all()


def test_fewer_points_than_faces():
    verts, faces = random_mesh(1, 200, 300)
    _, tri, count, _ = check(verts, faces, 7)
    assert count == 7 and len(set(tri.tolist())) <= 7


def test_degenerate_triangles_own_nothing():
    verts, faces = random_mesh(2, 40, 65)
    verts = np.concatenate([verts, np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], np.float32)])     # exactly collinear
    faces[0] = [5, 5, 9]
    faces[32] = [40, 41, 42]
    faces[64] = [7, 11, 11]
    q, _ = ref.areas_q(verts, faces)
    assert q[[0, 32, 64]].tolist() == [0, 0, 0] and (np.delete(q, [0, 32, 64]) > 0).all()
    _, tri, count, status = check(verts, faces, 3000)
    assert count == 3000 and status == 0 and not np.isin(tri, [0, 32, 64]).any()
    assert tri[0] == 1 and tri[-1] == 63


def test_one_large_triangle_among_many_small_ones():
    """10 m^2 among 2,000 of 1e-6 m^2: the owner search crosses long runs of equal bounds on both sides of it."""
    small = math.sqrt(2e-6)
    verts = [[0, 0, 0], [small, 0, 0], [0, small, 0], [0, 0, 1], [math.sqrt(20.0), 0, 1], [0, math.sqrt(20.0), 1]]
    faces = np.array([[0, 1, 2]] * 1000 + [[3, 4, 5]] + [[0, 1, 2]] * 1000)
    for n in (50, 20000):
        _, tri, count, _ = check(np.array(verts, np.float32), faces, n)
        got = np.bincount(tri, minlength=2001)
        assert count == n and got[1000] >= n - 5 and got.max() == got[1000]
    assert (got[:1000] > 0).sum() + (got[1001:] > 0).sum() >= 2       # the small ones own a few of 20,000 points


# ------------------------------------------------------------------ status
def test_status_cases():
    tri3 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0]], np.float32)
    # all degenerate: no point, no bit
    pts, _, count, status = check(tri3, [[0, 0, 1], [1, 1, 2], [2, 2, 2]], 100)
    assert (count, status, len(pts)) == (0, 0, 0)
    # an index outside [0, V): its bit, and the other triangle owns every point
    _, tri, count, status = check(tri3, [[0, 1, 4], [0, 1, 2], [0, -1, 2]], 100)
    assert count == 100 and status == _abi.MESH_SAMPLE_INDEX and (tri == 1).all()
    # a NaN vertex: its bit
    _, tri, count, status = check(tri3, [[0, 1, 2], [0, 1, 3]], 100)
    assert count == 100 and status == _abi.MESH_SAMPLE_NONFINITE and (tri == 0).all()
    # above the area cap (one face: 2^30 m^2): the other bit, and the drivers raise after their one read
    big = np.array([[0, 0, 0], [3e5, 0, 0], [0, 3e5, 0]], np.float32)
    _, _, count, status = check(big, [[0, 1, 2]], 100)
    assert count == 0 and status == _abi.MESH_SAMPLE_AREA_CAP
    target = np.zeros((4, 3), np.float32)
    with pytest.raises(_lib.PingsHipError, match="area cap"):
        eval_ops.eval_mesh((big, np.array([[0, 1, 2]])), target, gt_bbx_mask_on=False, mesh_sample_point=100)
    with pytest.raises(_lib.PingsHipError, match="area cap"):
        eval_ops.crop_intersection(target, [(big, np.array([[0, 1, 2]]))], mesh_sample_point=100)
    with pytest.raises(ValueError):
        mesh_ops.sample_surface(dev(tri3[:, :2]), dev([[0, 1, 2]], torch.int64), 10)
    with pytest.raises(ValueError):
        mesh_ops.sample_surface(dev(tri3), dev([[0, 1, 2]], torch.int32), 10)


# ------------------------------------------------------------------ the fused box crop
def grid_mesh(k, z=None):
    """(k+1) x (k+1) vertices over the unit square, 2 k^2 triangles; coordinates i / k."""
    i, j = np.meshgrid(np.arange(k + 1), np.arange(k + 1), indexing="ij")
    x, y = (i / k).ravel(), (j / k).ravel()
    verts = np.column_stack([x, y, np.zeros_like(x) if z is None else z(x, y)]).astype(np.float32)
    a = (i[:-1, :-1] * (k + 1) + j[:-1, :-1]).ravel()
    faces = np.concatenate([np.column_stack([a, a + k + 1, a + 1]), np.column_stack([a + 1, a + k + 1, a + k + 2])])
    return verts, faces.astype(np.int64)


def test_box_crop_on_a_grid_mesh():
    verts, faces = grid_mesh(32, lambda x, y: 0.25 * x * y)
    lo, hi = [8 / 32, 0.0, -1.0], [24 / 32, 20 / 32, 1.0]                 # bounds exactly on vertex rows
    kept = ref.crop_faces(verts, faces, lo, hi)
    assert len(kept) == 2 * 16 * 20                                        # the rows on the bounds are inside
    n = 5000
    want_pts, want_tri, count, _ = ref.sample(verts, kept, n, seed=11)     # the survivors alone: the same Q
    index = {tuple(f): t for t, f in enumerate(faces.tolist())}
    original = np.array([index[tuple(f)] for f in kept.tolist()], np.int32)
    for box in ((lo, hi), dev(np.array([lo, hi]), torch.float64)):
        pts, tri, got_count, status = run(verts, faces, n, seed=11, box=box)
        assert got_count == count == n and status == 0
        assert pts.tobytes() == want_pts.tobytes() and np.array_equal(tri, original[want_tri])
    check(verts, faces, n, seed=11, box=(lo, hi))
    # one ulp inside the row at 8 / 32: that row of vertices, and its triangles, are gone
    _, tri, _, _ = check(verts, faces, n, seed=11, box=([np.nextafter(np.float32(0.25), np.float32(1)), 0, -1], hi))
    assert verts[faces[np.unique(tri)]][..., 0].min() == np.float32(9 / 32)
    # a box that excludes everything
    pts, _, count, status = check(verts, faces, n, box=([2, 2, 2], [3, 3, 3]))
    assert (count, status) == (0, 0)


def test_crop_box_is_open3d_s_crop():
    verts, faces = grid_mesh(8, lambda x, y: x - y)
    lo, hi = [0.25, 0.0, -0.5], [0.75, 0.5, 1.0]
    _lib.sync_counts(reset=True)
    v, f = mesh_ops.crop_box(dev(verts), dev(faces, torch.int64), lo, hi)
    assert _lib.sync_counts(reset=True) == {"mesh_crop_box": 1}
    inside = ((verts >= np.array(lo)) & (verts <= np.array(hi))).all(1)
    assert np.array_equal(host(v), verts[inside])                          # kept vertices in order
    kept = ref.crop_faces(verts, faces, lo, hi)
    assert len(kept) > 0 and np.array_equal(host(v)[host(f)], verts[kept])


# ------------------------------------------------------------------ repeatability
def test_runs_repeat_and_seeds_differ():
    verts, faces = random_mesh(3, 500, 1000)
    a, b, c = run(verts, faces, 10000, seed=5), run(verts, faces, 10000, seed=5), run(verts, faces, 10000, seed=6)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert np.array_equal(a[1], c[1]) and (a[0] != c[0]).any(1).mean() > 0.99
    big = run(verts, faces, 10000, seed=2 ** 64 - 1)                       # the whole 64 bits of the seed are used
    assert big[0].tobytes() == ref.sample(verts, faces, 10000, 2 ** 64 - 1)[0].tobytes()


# ------------------------------------------------------------------ eval_mesh
SQUARE = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32), np.array([[0, 1, 2], [1, 3, 2]]))
N_EVAL = 200000


@pytest.fixture(scope="module")
def target():
    g = np.arange(51) / 50.0
    x, y = np.meshgrid(g, g, indexing="ij")
    return np.column_stack([x.ravel(), y.ravel(), np.full(x.size, 0.01)]).astype(np.float32)


def same_dict(a, b):
    assert list(a) == list(b) == list(eval_ops.PAIR_KEYS)
    for k in a:
        assert a[k] == b[k] or (math.isnan(a[k]) and math.isnan(b[k])), (k, a[k], b[k])


@pytest.fixture(scope="module")
def square_result(target):
    _lib.sync_counts(reset=True)
    got = eval_ops.eval_mesh(SQUARE, target, mesh_sample_point=N_EVAL)
    return got, _lib.sync_counts(reset=True)


def test_eval_mesh_equals_eval_pair_of_the_restatement_s_sample(target, square_result):
    got, reads = square_result
    assert reads == {"eval_pair": 1}                                       # the whole call: one host read
    pts, _, count, _ = ref.sample(*SQUARE, N_EVAL, 0, ref.target_box(target, 0.02))
    assert count == N_EVAL
    same_dict(got, eval_ops.eval_pair(dev(pts), dev(target)))
    assert got["Recall[Completeness](%)"] == 100.0 and got["Precision[Accuracy](%)"] == 100.0
    # the defect the feature removes: the four vertices of the same surface cover almost none of the target
    assert eval_ops.eval_pair(dev(SQUARE[0]), dev(target))["Recall[Completeness](%)"] < 5.0
    # device tensors and a Mesh are taken as they are
    mesh = mesh_ops.Mesh(dev(SQUARE[0]), dev(SQUARE[1], torch.int64), None, None)
    same_dict(got, eval_ops.eval_mesh(mesh, dev(target), mesh_sample_point=N_EVAL))


def test_eval_mesh_does_not_depend_on_the_triangulation(target, square_result):
    fine = eval_ops.eval_mesh(grid_mesh(50), target, mesh_sample_point=N_EVAL)
    # centroids of full 0.02 m cells move by less than a tenth of a cell between two samples of this density
    assert abs(fine["Chamfer_L1(m)"] - square_result[0]["Chamfer_L1(m)"]) < 0.02 / 10
    assert fine["Recall[Completeness](%)"] == 100.0


def test_eval_mesh_empty_crop(target):
    away = (SQUARE[0] + np.float32(10.0), SQUARE[1])
    same_dict(eval_ops.eval_mesh(away, target, mesh_sample_point=1000),
              eval_ops.eval_pair(np.zeros((0, 3)), target))
    assert eval_ops.eval_mesh(away, target, mesh_sample_point=1000, gt_bbx_mask_on=False)["Recall[Completeness](%)"] == 0


def test_eval_mesh_reads_paths(tmp_path, target, square_result):
    mesh_ops.write_ply(tmp_path / "pred.ply", *SQUARE)
    mesh_ops.write_ply(tmp_path / "trgt.ply", target, np.zeros((0, 3), np.int64))
    same_dict(square_result[0], eval_ops.eval_mesh(tmp_path / "pred.ply", str(tmp_path / "trgt.ply"),
                                                   mesh_sample_point=N_EVAL))


# ------------------------------------------------------------------ crop_intersection
def test_crop_intersection(tmp_path):
    a = SQUARE
    b = (SQUARE[0] + np.array([0.5, 0, 0], np.float32), SQUARE[1])
    gx, gy = np.meshgrid(0.025 + 0.05 * np.arange(30), 0.025 + 0.05 * np.arange(20), indexing="ij")
    gt = np.column_stack([gx.ravel(), gy.ravel(), np.full(gx.size, 0.02)]).astype(np.float32)    # over the union
    n, thre = 20000, 0.1
    out = tmp_path / "crop.ply"
    _lib.sync_counts(reset=True)
    kept = eval_ops.crop_intersection(gt, [a, b], out, dist_thre=thre, mesh_sample_point=n, seed=4)
    assert _lib.sync_counts(reset=True) == {"eval_crop_intersection": 1}
    # brute force in fp64 against the restatement's samples
    near = np.ones(len(gt), bool)
    for verts, faces in (a, b):
        pts = ref.sample(verts, faces, n, 4)[0].astype(np.float64)
        d = np.sqrt(((gt.astype(np.float64)[:, None, :] - pts[None, :, :]) ** 2).sum(-1).min(1))
        assert not (np.abs(d - thre) < 1e-5).any()                         # no point is too close to call
        near &= d < thre
    assert near.sum() == 14 * 20                                           # the columns 0.425 .. 1.075
    assert kept.is_cuda and np.array_equal(host(kept), gt[near])
    back = mesh_ops.read_ply(out)
    assert np.array_equal(back["verts"], gt[near].astype(np.float64)) and back["faces"].shape == (0, 3)
