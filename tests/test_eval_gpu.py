"""View evaluation on the device (pings_amd/eval_ops.py, csrc/eval.hip) against the fp64 restatement
(tests/eval_ref.py).

EPS = 2^-24 is fp32's rounding unit and X the largest |coordinate| of a case's inputs.  The bounds:
  nn_distance      |d - d64| <= 4 EPS (d64 + X): one rounding of each coordinate difference, three products, two sums
                   and a root.  An index is right when the fp64 distance to it is within that bound of the minimum.
  voxel_centroids  inputs keep 0.1 cell away from every face, so the partition is not in question; the mean is formed
                   in fp64 and rounded once: |c - c64| <= 8 EPS X (the issue's bound; the code needs EPS X).
  backproject      formed in fp64 from fp32 depths and rounded once: <= 8 EPS X; kept pixels, order and colours exact.
  view_metrics     the project's 1e-4 relative gate on each mse, on L1 and on RMSE.
  eval_pair        see test_eval_pair_sheets."""
import math

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import eval_ref
from pings_amd import _lib, eval_ops
from pings_amd.ssim import fused_ssim

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
F64 = np.float64
ORIGIN = np.array([40.0, -25.0, 3.0])


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def host(t):
    return t.detach().cpu().numpy()


def eval_reads():
    """{name: count} of the host reads noted since the last reset; every one of this module's is named eval_*."""
    return _lib.sync_counts(reset=True)


# ------------------------------------------------------------------ inputs
def sheet(rng, n, noise=0.0, outliers=0.0, size=(10.0, 6.0)):
    """n points of a wavy sheet of `size` metres around ORIGIN, fp32; a fraction `outliers` of them lifted 4-6 m off it."""
    xy = rng.uniform([0.0, 0.0], size, (n, 2))
    z = 0.3 * np.sin(xy[:, 0]) * np.cos(1.3 * xy[:, 1])
    p = np.column_stack([xy, z]) + rng.normal(0.0, noise, (n, 3)) if noise else np.column_stack([xy, z])
    k = int(round(n * outliers))
    if k:
        p[rng.choice(n, k, replace=False), 2] += rng.uniform(4.0, 6.0, k)
    return (p + ORIGIN).astype(np.float32)


@pytest.fixture(scope="module")
def sheets():
    rng = np.random.default_rng(7)
    return sheet(rng, 5000, noise=0.01, outliers=0.01), sheet(rng, 2000)


def voxel_cloud(rng, n, min_point, voxel, kmax, ncells):
    """One explicit minimum point, then n points at anchor + (k + u) voxel with u in [0.1, 0.9] and k >= 1 on every
    axis (so the minimum stays the minimum), rounded to fp32: no coordinate within 0.1 cell of a face."""
    m = np.asarray(min_point, np.float32)
    anchor = m.astype(F64) - voxel / 2
    cells = rng.integers(1, kmax + 1, (ncells, 3))
    k = cells[rng.integers(0, ncells, n)]
    p = anchor + (k + rng.uniform(0.1, 0.9, (n, 3))) * voxel
    return np.concatenate([m[None], p.astype(np.float32)])


# ------------------------------------------------------------------ nn_distance
def check_nn(src, dst, max_dist, **kw):
    src, dst = np.asarray(src, np.float32), np.asarray(dst, np.float32)
    dist, idx = eval_ops.nn_distance(dev(src), dev(dst), max_dist, **kw)
    assert dist.dtype == torch.float32 and idx.dtype == torch.int64 and dist.shape == idx.shape == (len(src),)
    dist, idx = host(dist).astype(F64), host(idx)
    s64, d64 = src.astype(F64), dst.astype(F64)
    dmin = cKDTree(d64).query(s64, k=1)[0]
    X = max(np.abs(src).max(), np.abs(dst).max())
    bound = 4 * EPS * (dmin + X)
    undecided = np.abs(dmin - max_dist) <= bound          # fp32 cannot tell which side of max_dist these are on
    found = idx >= 0
    assert ((found == (dmin < max_dist)) | undecided).all()
    assert np.array_equal(np.isinf(dist), ~found) and (idx[~found] == -1).all() and (idx < len(dst)).all()
    err = np.abs(dist[found] - dmin[found])
    print(f"nn: {found.sum()} found of {len(src)}, max err / bound = {(err / bound[found]).max() if found.any() else 0:.3f}")
    assert (err <= bound[found]).all()
    to_idx = np.linalg.norm(s64[found] - d64[idx[found]], axis=1)
    assert (np.abs(to_idx - dmin[found]) <= bound[found]).all()
    return dist, idx


def test_nn_single_dst_point():
    rng = np.random.default_rng(0)
    dist, idx = check_nn(ORIGIN + rng.uniform(-1, 1, (50, 3)), ORIGIN[None], 1.2)
    assert set(idx.tolist()) == {0, -1}


def test_nn_single_query():
    rng = np.random.default_rng(1)
    check_nn(ORIGIN[None] + 0.3, ORIGIN + rng.uniform(0, 1, (700, 3)), 0.5)


def test_nn_300_points_in_one_cell():
    rng = np.random.default_rng(2)
    dst = ORIGIN + 0.2 + rng.uniform(0, 0.01, (300, 3))
    check_nn(ORIGIN + rng.uniform(0, 0.5, (200, 3)), dst, 1.0, cell=0.5)


def test_nn_points_on_cell_faces_and_corners():
    """dst's lower corner is ORIGIN and the cell 0.25, so ORIGIN + k * 0.25 lies exactly on faces / corners in fp32."""
    rng = np.random.default_rng(3)
    k = rng.integers(0, 9, (400, 3))
    on = ORIGIN + k * 0.25
    on[:, 0] += np.where(rng.random(400) < 0.5, 0.0, rng.uniform(0, 0.25, 400))      # half on a face only
    dst = np.concatenate([ORIGIN[None], on, ORIGIN + rng.uniform(0, 2.25, (300, 3))]).astype(np.float32)
    q = ORIGIN + rng.integers(-1, 10, (600, 3)) * 0.25
    q32 = q.astype(np.float32)
    nudged = np.concatenate([q32, np.nextafter(q32, np.float32(np.inf)), np.nextafter(q32, np.float32(-np.inf))])
    check_nn(nudged, dst, 0.6, cell=0.25)


def test_nn_queries_outside_the_box_on_every_side():
    rng = np.random.default_rng(4)
    dst = ORIGIN + rng.uniform(0, 1, (500, 3))
    q = []
    for axis in range(3):
        for side in (-1.0, 1.0):
            for off in (0.3, 0.7, 5.0):                   # nearer and farther than max_dist = 0.5
                p = ORIGIN + rng.uniform(0, 1, (40, 3))
                p[:, axis] = ORIGIN[axis] + (1.0 + off if side > 0 else -off)
                q.append(p)
    dist, idx = check_nn(np.concatenate(q), dst, 0.5)
    assert (idx >= 0).any() and (idx < 0).any()


def test_nn_max_dist_smaller_than_the_cell():
    rng = np.random.default_rng(5)
    dst = ORIGIN + rng.uniform(0, 2, (3000, 3))
    dist, idx = check_nn(ORIGIN + rng.uniform(0, 2, (1000, 3)), dst, 0.1, cell=0.5)
    assert (idx >= 0).any() and (idx < 0).any()


def test_nn_ring_cap_reached_by_sparse_far_points():
    rng = np.random.default_rng(6)
    dst = ORIGIN + rng.uniform(0, 3, (60, 3))
    dist, idx = check_nn(ORIGIN + rng.uniform(-0.5, 3.5, (1500, 3)), dst, 0.65, cell=0.1)     # 6.5 cells: 7 rings
    assert (dist[idx >= 0] > 0.6).any() and (idx < 0).any()


def test_nn_duplicates_go_to_the_smallest_index():
    rng = np.random.default_rng(8)
    base = (ORIGIN + rng.uniform(0, 2, (400, 3))).astype(np.float32)
    perm = rng.permutation(400)
    dst = np.concatenate([base[perm[:150]], base, base[perm[100:300]]])       # up to three copies of a point
    src = (ORIGIN + rng.uniform(0, 2, (800, 3))).astype(np.float32)
    dist, idx = check_nn(src, dst, 1.0)
    d2, near = cKDTree(base.astype(F64)).query(src.astype(F64), k=2)
    clear = (d2[:, 1] - d2[:, 0]) > 16 * EPS * (d2[:, 1] + np.abs(dst).max())   # fp32 cannot confuse the two nearest
    assert clear.sum() > 700
    first = {}
    for i, p in enumerate(map(bytes, dst)):
        first.setdefault(p, i)
    want = np.array([first[bytes(base[j])] for j in near[:, 0]])
    assert np.array_equal(idx[clear], want[clear])


def test_nn_sheets_with_outliers(sheets):
    src, dst = sheets
    dist, idx = check_nn(src, dst, 1.0, spacing=0.05)
    assert (idx < 0).sum() == 50                           # the 1 % lifted 4-6 m off the sheet
    # any query order gives the same answer
    perm = np.random.default_rng(9).permutation(len(src))
    d2, i2 = eval_ops.nn_distance(dev(src[perm]), dev(dst), 1.0, spacing=0.05)
    assert np.array_equal(host(d2).astype(F64), dist[perm]) and np.array_equal(host(i2), idx[perm])


def test_nn_correspondance_lists(sheets):
    src, dst = sheets
    eval_reads()
    ind, d = eval_ops.nn_correspondance(dst[:500], src[:300], 0.5, True)
    assert eval_reads() == {"eval_nn_correspondance": 1}
    rd, ri = eval_ref.nn_distance(src[:300], dst[:500], 0.5)
    keep = ri >= 0
    assert isinstance(ind, list) and isinstance(d, list) and len(ind) == len(d) == keep.sum()
    assert np.allclose(d, rd[keep], rtol=0, atol=4 * EPS * 60)
    ind2, d2 = eval_ops.nn_correspondance(dst[:500], src[:300], 0.5, False)
    assert len(d2) == 300 and np.allclose(d2, np.where(keep, rd, 0.5), rtol=0, atol=4 * EPS * 60)


# ------------------------------------------------------------------ voxel_centroids
def check_voxel(p32, voxel):
    got = host(eval_ops.voxel_centroids(dev(p32), voxel)).astype(F64)
    want = eval_ref.voxel_centroids(p32.astype(F64), voxel)
    assert got.shape == want.shape                          # cell count
    X = np.abs(p32).max()
    err = np.abs(got - want).max()
    print(f"voxel: {len(p32)} points, {len(want)} cells, max err {err:.3e}, bound {8 * EPS * X:.3e}")
    assert err <= 8 * EPS * X                               # row by row: the order too
    return got


def test_voxel_single_point():
    got = check_voxel(np.array([[40.1, -25.3, 3.7]], np.float32), 0.05)
    assert got.shape == (1, 3)


def test_voxel_1500_points_in_one_voxel():
    rng = np.random.default_rng(10)
    m = ORIGIN.astype(np.float32)
    p = np.concatenate([m[None], (m + rng.uniform(0, 0.4, (1500, 3)) * 0.05).astype(np.float32)])
    assert check_voxel(p, 0.05).shape == (1, 3)


def test_voxel_cloud_near_origin_offset():
    rng = np.random.default_rng(11)
    p = voxel_cloud(rng, 20000, ORIGIN, 0.05, 60, 8000)
    got = check_voxel(p, 0.05)
    assert 5000 < len(got) <= 8001
    again = host(eval_ops.voxel_centroids(dev(p), 0.05))
    assert np.array_equal(again.astype(F64), got)           # bitwise from run to run


def test_voxel_all_negative_coordinates():
    rng = np.random.default_rng(12)
    p = voxel_cloud(rng, 3000, [-40.0, -25.0, -3.0], 0.02, 40, 900)
    assert (p < 0).all()
    check_voxel(p, 0.02)


def test_voxel_anchor_is_half_a_cell_below_the_minimum():
    p = np.array([[0.2, 0.0, 0.0], [0.8, 0.0, 0.0], [1.1, 0.0, 0.0]], np.float32)
    got = check_voxel(p, 1.0)
    assert np.allclose(got, [[0.2, 0, 0], [0.95, 0, 0]], rtol=0, atol=1e-6)      # anchored at 0: 0.5 and 1.1


def test_voxel_reads_once():
    eval_reads()
    eval_ops.voxel_centroids(dev(sheet(np.random.default_rng(13), 1000)), 0.1)
    assert eval_reads() == {"eval_voxel_count": 1}


# ------------------------------------------------------------------ backproject_depth
H, W = 37, 53
K = (48.5, 47.25, 26.2, 18.4)
TRUNC = 10.0


def extrinsic():
    a, b = 0.4, -0.25
    Rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    E = np.eye(4)
    E[:3, :3] = Rz @ Rx
    E[:3, 3] = -E[:3, :3] @ ORIGIN          # world -> camera of a camera standing at ORIGIN
    return E


@pytest.fixture(scope="module")
def rgbd():
    rng = np.random.default_rng(20)
    depth = rng.uniform(0.5, 12.0, (H, W)).astype(np.float32)       # some beyond depth_trunc
    depth[rng.random((H, W)) < 0.1] = 0.0
    depth[rng.random((H, W)) < 0.05] = TRUNC                        # equal to depth_trunc: dropped
    rgb = rng.random((3, H, W)).astype(np.float32)
    rgb[:, 0, :5] = [[1.0], [0.0], [0.999999]]
    alpha = rng.random((H, W)).astype(np.float32)
    return depth, rgb, alpha


def check_backproject(depth, rgb, alpha, min_alpha, E):
    eval_reads()
    out = eval_ops.backproject_depth(dev(depth)[None], K, E, TRUNC, rgb=None if rgb is None else dev(rgb),
                                     alpha=None if alpha is None else dev(alpha), min_alpha=min_alpha)
    assert eval_reads() == {"eval_backproject_count": 1}
    pts, col = out if rgb is not None else (out, None)
    want, wcol, pix = eval_ref.backproject_depth(depth, K, E, TRUNC, rgb, alpha, min_alpha)
    assert pts.shape == (len(want), 3)                      # M
    if len(want):
        X = max(np.abs(want).max(), depth.max())
        err = np.abs(host(pts).astype(F64) - want).max()
        print(f"backproject: {len(want)} of {depth.size} pixels, max err {err:.3e}, bound {8 * EPS * X:.3e}")
        assert err <= 8 * EPS * X                           # row by row: the pixel order too
    if rgb is not None:
        assert np.array_equal(host(col), wcol.astype(np.float32))
    return pix


def test_backproject_image_with_colours(rgbd):
    depth, rgb, _ = rgbd
    pix = check_backproject(depth, rgb, None, None, extrinsic())
    assert 0 < len(pix) < H * W and (depth.reshape(-1)[pix] < TRUNC).all() and (depth == TRUNC).sum() > 20


def test_backproject_alpha_mask_and_identity(rgbd):
    depth, rgb, alpha = rgbd
    pix = check_backproject(depth, None, alpha, 0.5, np.eye(4))
    assert (alpha.reshape(-1)[pix] > 0.5).all()
    assert len(pix) < len(check_backproject(depth, None, None, None, np.eye(4)))


def test_backproject_all_zero_depth(rgbd):
    _, rgb, _ = rgbd
    pts, col = eval_ops.backproject_depth(torch.zeros(1, H, W, device="cuda"), K, extrinsic(), TRUNC, rgb=dev(rgb))
    assert pts.shape == col.shape == (0, 3)


# ------------------------------------------------------------------ view_metrics
def check_view(rgb, gt, depth, gtd, alpha, min_alpha, dmin=0.5, dmax=8.0):
    d = lambda a: None if a is None else dev(a)
    eval_reads()
    m = eval_ops.view_metrics(d(rgb), d(gt), d(depth), d(gtd), d(alpha), depth_min=dmin, depth_max=dmax,
                              min_alpha=min_alpha, ssim=False)
    assert eval_reads() == {"eval_view_metrics": 1}
    rec = host(eval_ops.view_metrics_record(d(rgb), d(gt), d(depth), d(gtd), d(alpha), depth_min=dmin, depth_max=dmax,
                                            min_alpha=min_alpha, ssim=False))
    want = eval_ref.view_metrics(rgb, gt, depth, gtd, alpha, depth_min=dmin, depth_max=dmax, min_alpha=min_alpha)
    C = rgb.shape[0]
    print("view: mse", rec[5:5 + C], want["mse"], "l1", m.depth_l1, want["depth_l1"], "rmse", m.depth_rmse,
          want["depth_rmse"], "n", m.n_valid, want["n_valid"])
    assert np.allclose(rec[5:5 + C], want["mse"], rtol=1e-4, atol=0) and np.isnan(rec[5 + C:]).all()
    assert m.n_valid == want["n_valid"] and math.isnan(m.ssim)
    if math.isinf(want["psnr"]):
        assert m.psnr == math.inf
    else:
        assert m.psnr == pytest.approx(want["psnr"], abs=20 * math.log10(1 + 1e-4))
    if want["n_valid"]:
        assert m.depth_l1 == pytest.approx(want["depth_l1"], rel=1e-4)
        assert m.depth_rmse == pytest.approx(want["depth_rmse"], rel=1e-4)
    else:
        assert math.isnan(m.depth_l1) and math.isnan(m.depth_rmse)
    return m


def test_view_metrics_image(rgbd):
    depth, rgb, alpha = rgbd
    rng = np.random.default_rng(21)
    gt = np.clip(rgb + rng.normal(0, 0.05, rgb.shape), 0, 1).astype(np.float32)
    gtd = (depth + rng.normal(0, 0.1, depth.shape)).astype(np.float32)
    m = check_view(rgb, gt, depth[None], gtd[None], alpha[None], 0.5)
    m2 = check_view(rgb, gt, depth, gtd, None, None)
    assert 0 < m.n_valid < m2.n_valid < H * W
    assert math.isnan(check_view(rgb, gt, None, None, None, None).depth_l1)


def test_view_metrics_one_pixel():
    rgb, gt = np.array([[[0.5]], [[0.25]], [[1.0]]], np.float32), np.array([[[0.25]], [[0.75]], [[0.0]]], np.float32)
    m = check_view(rgb, gt, np.array([[1.0]], np.float32), np.array([[1.5]], np.float32), None, None)
    assert (m.depth_l1, m.depth_rmse, m.n_valid) == (0.5, 0.5, 1)


def test_view_metrics_identical_images_and_empty_mask(rgbd):
    depth, rgb, _ = rgbd
    m = check_view(rgb, rgb.copy(), depth, depth, None, None, dmin=20.0, dmax=30.0)
    assert m.psnr == math.inf and m.n_valid == 0 and math.isnan(m.depth_l1) and math.isnan(m.depth_rmse)


def test_view_metrics_ssim_is_fused_ssim(rgbd):
    _, rgb, _ = rgbd
    gt = np.clip(rgb + np.random.default_rng(22).normal(0, 0.05, rgb.shape), 0, 1).astype(np.float32)
    a, b = dev(rgb), dev(gt)
    eval_reads()
    m = eval_ops.view_metrics(a, b, depth_min=0.1, depth_max=10.0)
    assert eval_reads() == {"eval_view_metrics": 1}
    want = fused_ssim(a.unsqueeze(0), b.unsqueeze(0), train=False)
    assert np.float32(m.ssim).tobytes() == host(want).astype(np.float32).tobytes() and 0 < m.ssim < 1


# ------------------------------------------------------------------ eval_pair
PAIR = dict(down_sample_res=0.05, threshold=0.1, truncation_acc=1.0, truncation_com=1.0)     # the mapper's call


@pytest.fixture(scope="module")
def pair_clouds():
    # 6 m x 4 m: dense enough that few nearest-neighbour distances come near the 0.1 m threshold.  On the restatement
    # alone, seeds 30..33 give A = 0, 2, 0, 0 of about 16,900 distances here (6..19 on a 10 m x 6 m sheet)
    rng = np.random.default_rng(30)
    return sheet(rng, 20000, 0.02, 0.01, (6.0, 4.0)), sheet(rng, 6000, size=(6.0, 4.0))


def test_eval_pair_sheets(pair_clouds):
    """A distance within 1e-4 m of the threshold or of a truncation is one fp32 cannot decide; A counts them in the
    restatement (at most 5, a property of the inputs).  Inlier and outlier counts may then differ by A, and the two
    means and Chamfer-L2 agree to 1e-5 relative plus A * truncation / n for the undecided points."""
    pred, trgt = pair_clouds
    want, (dp, dr) = eval_ref.eval_pair(pred, trgt, **PAIR, details=True)
    A = int(sum((np.abs(d[np.isfinite(d)] - t) < 1e-4).sum() for d in (dp, dr) for t in (0.1, 1.0)))
    n_p, n_r = int(np.isfinite(dp).sum()), len(dr)
    print(f"eval_pair: {len(dp)} + {len(dr)} centroids, {len(dp) - n_p} pred outliers, A = {A}")
    assert A <= 5 and n_p > 1000 and len(dp) - n_p >= 100
    eval_reads()
    got = eval_ops.eval_pair(dev(pred), dev(trgt), **PAIR)
    assert eval_reads() == {"eval_pair": 1}                 # one host read for the whole call
    assert list(got) == list(eval_ref.KEYS)
    for k in eval_ref.KEYS:
        print(f"  {k}: {got[k]!r} (restatement {want[k]!r})")
    for k in eval_ref.KEYS[7:]:
        assert got[k] == want[k]
    for k, n in (("MAE_accuracy(m)", n_p), ("MAE_completeness(m)", n_r), ("Chamfer_L2(m)", min(n_p, n_r))):
        assert abs(got[k] - want[k]) <= 1e-5 * want[k] + A * 1.0 / n, k
    assert abs(got["Chamfer_L1(m)"] - 0.5 * (got["MAE_accuracy(m)"] + got["MAE_completeness(m)"])) < 1e-15
    for k, n in (("Precision[Accuracy](%)", n_p), ("Recall[Completeness](%)", n_r)):
        assert abs(got[k] - want[k]) <= 100.0 * (A / n + A / max(n - A, 1)) + 1e-9, k
    p, r = got["Precision[Accuracy](%)"], got["Recall[Completeness](%)"]
    assert got["F-score(%)"] == pytest.approx(2 * p * r / (p + r), rel=1e-14)
    assert eval_ops.eval_pair(dev(pred), dev(trgt), **PAIR) == got       # equal from call to call


def test_eval_pair_takes_host_clouds_and_device_counts(pair_clouds):
    pred, trgt = pair_clouds
    got = eval_ops.eval_pair(dev(pred[:3000]), dev(trgt[:1000]), **PAIR)
    from types import SimpleNamespace as NS
    assert eval_ops.eval_pair(NS(points=pred[:3000].astype(F64)), trgt[:1000], **PAIR) == got
    # buffers longer than their live length, the lengths on the device (what backproject_device hands over)
    n = torch.tensor([3000], dtype=torch.int64, device="cuda")
    m = torch.tensor([1000], dtype=torch.int64, device="cuda")
    eval_reads()
    assert eval_ops.eval_pair(dev(pred[:4000]), dev(trgt[:1500]), **PAIR, pred_count=n, trgt_count=m) == got
    assert eval_reads() == {"eval_pair": 1}


def test_eval_pair_empty_pred_is_nan(pair_clouds):
    got = eval_ops.eval_pair(torch.zeros(0, 3, device="cuda"), dev(pair_clouds[1]), **PAIR)
    assert all(math.isnan(got[k]) for k in eval_ref.KEYS[:7]) and got["Spacing(m)"] == 0.05
    # every pred point an outlier: numpy's NaN on the precision side only
    far = eval_ops.eval_pair(dev(pair_clouds[1] + np.float32(50.0)), dev(pair_clouds[1]), **PAIR)
    assert math.isnan(far["MAE_accuracy(m)"]) and math.isnan(far["F-score(%)"])
    assert far["MAE_completeness(m)"] == 1.0 and far["Recall[Completeness](%)"] == 0.0
