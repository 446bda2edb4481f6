"""fp64 numpy restatement of pings_amd/eval_ops.py: what the reference's per-view evaluation computes
(utils/mapper.py:1950-2056, eval/eval_mesh_utils.py:100-182) with Open3D's rules for RGBD back-projection and
`voxel_down_sample` written out.  Plain and slow on purpose; test_eval_ref.py checks it against hand-computed cases."""
from __future__ import annotations

import contextlib
import warnings

import numpy as np

WORKERS = -1     # threads of the KD-tree query (scipy: -1 = all); tools/eval_time.py sets its own

KEYS = ("MAE_accuracy(m)", "MAE_completeness(m)", "Chamfer_L1(m)", "Chamfer_L2(m)", "Precision[Accuracy](%)",
        "Recall[Completeness](%)", "F-score(%)", "Spacing(m)", "Inlier_threshold(m)", "Outlier_truncation_acc(m)",
        "Outlier_truncation_com(m)")


@contextlib.contextmanager
def _quiet():
    """numpy's NaN for an empty mean or 0 / 0 is the expected answer here, not a warning."""
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        yield


def view_metrics(rgb, gt, depth=None, gt_depth=None, alpha=None, *, depth_min, depth_max, min_alpha=None):
    """-> dict(mse [C], psnr, depth_l1, depth_rmse, n_valid); NaN depth figures on an empty mask."""
    rgb, gt = np.asarray(rgb, np.float64), np.asarray(gt, np.float64)
    mse = ((rgb - gt) ** 2).reshape(rgb.shape[0], -1).mean(1)
    with _quiet():
        psnr = float(np.mean(20.0 * np.log10(1.0 / np.sqrt(mse))))
        out = dict(mse=mse, psnr=psnr, depth_l1=float("nan"), depth_rmse=float("nan"), n_valid=0)
        if depth is not None and gt_depth is not None:
            d, g = np.asarray(depth, np.float64), np.asarray(gt_depth, np.float64)
            mask = (g > depth_min) & (d > depth_min) & (g < depth_max) & (d < depth_max)
            if alpha is not None and min_alpha is not None:
                mask &= np.asarray(alpha, np.float64) > min_alpha
            e = np.abs(g - d)[mask]
            out.update(depth_l1=float(np.mean(e)), depth_rmse=float(np.sqrt(np.mean(e ** 2))), n_valid=int(mask.sum()))
    return out


def backproject_depth(depth, K, extrinsic, depth_trunc, rgb=None, alpha=None, min_alpha=None):
    """depth [H, W] -> (points [M, 3], colors [M, 3] or None, kept pixel indices [M]) in row-major pixel order."""
    d = np.asarray(depth, np.float64)
    d = d.reshape(d.shape[-2:])
    H, W = d.shape
    keep = (d > 0) & (d < depth_trunc)
    if alpha is not None and min_alpha is not None:
        keep &= np.asarray(alpha, np.float64).reshape(H, W) > min_alpha
    v, u = np.nonzero(keep)                      # row-major
    z = d[v, u]
    fx, fy, cx, cy = (float(k) for k in K)
    cam = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z, np.ones_like(z)], 1)
    pts = (cam @ np.linalg.inv(np.asarray(extrinsic, np.float64)).T)[:, :3]
    col = None
    if rgb is not None:
        c = np.asarray(rgb, np.float32)
        byte = np.clip(np.floor(c * np.float32(255.0)), 0, 255)          # (rgb * 255).byte(): fp32 product, truncated
        col = (byte.astype(np.float64) / 255.0)[:, v, u].T
    return pts, col, v * W + u


def voxel_cells(points, voxel):
    """Integer cell [N, 3] of each point on the grid anchored at min_bound - voxel/2."""
    p = np.asarray(points, np.float64)
    anchor = p.min(0) - voxel * 0.5
    return np.floor((p - anchor) / voxel).astype(np.int64)


def voxel_centroids(points, voxel, cells=None):
    """Open3D voxel_down_sample: mean of each occupied cell, ascending linear cell key with x fastest."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    if len(p) == 0:
        return np.zeros((0, 3))
    c = voxel_cells(p, voxel) if cells is None else cells
    dims = c.max(0) + 1
    key = c[:, 0] + dims[0] * (c[:, 1] + dims[1] * c[:, 2])
    uniq, inv = np.unique(key, return_inverse=True)
    out = np.zeros((len(uniq), 3))
    np.add.at(out, inv, p)
    return out / np.bincount(inv)[:, None]


def nn_distance(src, dst, max_dist, brute=False):
    """-> (dist [N], idx [N]): the nearest dst point of every src point, +inf / -1 where none is closer than max_dist."""
    s, d = np.asarray(src, np.float64).reshape(-1, 3), np.asarray(dst, np.float64).reshape(-1, 3)
    if len(s) == 0 or len(d) == 0:
        return np.full(len(s), np.inf), np.full(len(s), -1, np.int64)
    if brute:
        d2 = ((s[:, None, :] - d[None, :, :]) ** 2).sum(-1)
        idx = d2.argmin(1)
        dist = np.sqrt(d2[np.arange(len(s)), idx])
    else:
        from scipy.spatial import cKDTree
        dist, idx = cKDTree(d).query(s, k=1, workers=WORKERS)
    far = ~(dist < max_dist)
    return np.where(far, np.inf, dist), np.where(far, -1, idx).astype(np.int64)


def pair_from_distances(dist_p, dist_r, down_sample_res, threshold, truncation_acc, truncation_com):
    """eval_pair from the two distance lists of `nn_distance` (+inf = no neighbour below the truncation)."""
    dist_p = np.asarray(dist_p, np.float64)
    dist_p = dist_p[np.isfinite(dist_p)]                                  # precision side: outliers dropped
    dist_r = np.asarray(dist_r, np.float64)
    dist_r = np.where(np.isfinite(dist_r), dist_r, truncation_com)        # recall side: outliers clamped
    with _quiet():
        mp, mr = np.mean(dist_p), np.mean(dist_r)
        l2 = np.sqrt(0.5 * (np.mean(dist_p ** 2) + np.mean(dist_r ** 2)))
        precision = np.mean((dist_p < threshold).astype("float")) * 100.0
        recall = np.mean((dist_r < threshold).astype("float")) * 100.0
        fscore = 2 * precision * recall / (precision + recall)
    vals = (mp, mr, 0.5 * (mp + mr), l2, precision, recall, fscore, down_sample_res, threshold, truncation_acc,
            truncation_com)
    return {k: float(v) for k, v in zip(KEYS, vals)}


def eval_pair(pred, trgt, down_sample_res=0.02, threshold=0.05, truncation_acc=0.5, truncation_com=0.5, brute=False,
              downsample=True, details=False):
    """The reference's eval_pair.  details=True also returns (dist_p, dist_r) before dropping / clamping."""
    nan = pair_from_distances([], [], down_sample_res, threshold, truncation_acc, truncation_com)
    P, T = np.asarray(pred, np.float64).reshape(-1, 3), np.asarray(trgt, np.float64).reshape(-1, 3)
    if downsample:
        P, T = voxel_centroids(P, down_sample_res), voxel_centroids(T, down_sample_res)
    if len(P) == 0 or len(T) == 0:
        return (nan, (np.zeros(0), np.zeros(0))) if details else nan
    dist_p, _ = nn_distance(P, T, truncation_acc, brute)
    dist_r, _ = nn_distance(T, P, truncation_com, brute)
    m = pair_from_distances(dist_p, dist_r, down_sample_res, threshold, truncation_acc, truncation_com)
    return (m, (dist_p, dist_r)) if details else m
