"""View evaluation without a GPU (pings_amd/eval_ops.py, csrc/eval.hip): the fp64 restatement
(tests/eval_ref.py) against cases worked out by hand, and the argument checks of the operators and of their C entry
points, all of which answer before any GPU work."""
import math
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import eval_ref
from pings_amd import _lib, eval_ops

# ------------------------------------------------------------------ the restatement against hand-computed cases
PRED = np.array([[0.0, 0.1, 0.0],     # 0.1 from t0: exactly the threshold, not an inlier
                 [1.0, 0.05, 0.0],    # 0.05 from t1: an inlier
                 [1.0, 0.0, 0.5],     # 0.5 from t1: exactly the truncation, an outlier
                 [9.0, 0.0, 0.0]])    # 5 from t2: an outlier
TRGT = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [4.0, 0.0, 0.0]])   # t2: nearest pred point 3.04 away


def test_pair_strict_comparisons_and_outliers():
    m, (dp, dr) = eval_ref.eval_pair(PRED, TRGT, 0.02, threshold=0.1, truncation_acc=0.5, truncation_com=0.5,
                                     brute=True, downsample=False, details=True)
    assert dp.tolist() == [0.1, 0.05, math.inf, math.inf]          # strict < at the truncation
    assert dr.tolist() == [0.1, 0.05, math.inf]
    # precision side: the two outliers are dropped from the mean and from the count
    assert m["MAE_accuracy(m)"] == pytest.approx((0.1 + 0.05) / 2, rel=1e-15)
    assert m["Precision[Accuracy](%)"] == pytest.approx(50.0)       # strict < at the threshold: 0.1 is no inlier
    # recall side: the outlier counts with the truncation distance
    assert m["MAE_completeness(m)"] == pytest.approx((0.1 + 0.05 + 0.5) / 3, rel=1e-15)
    assert m["Recall[Completeness](%)"] == pytest.approx(100.0 / 3)
    assert m["Chamfer_L1(m)"] == pytest.approx(0.5 * (0.075 + 0.65 / 3), rel=1e-15)
    assert m["Chamfer_L2(m)"] == pytest.approx(math.sqrt(0.5 * (0.0125 / 2 + 0.2625 / 3)), rel=1e-15)
    assert m["F-score(%)"] == pytest.approx(2 * 50.0 * (100 / 3) / (50.0 + 100 / 3))
    assert list(m) == list(eval_ref.KEYS) == list(eval_ops.PAIR_KEYS) and len(m) == 11
    assert (m["Spacing(m)"], m["Inlier_threshold(m)"], m["Outlier_truncation_acc(m)"]) == (0.02, 0.1, 0.5)
    # the KD-tree path of the restatement gives the same lists
    _, (dp2, dr2) = eval_ref.eval_pair(PRED, TRGT, 0.02, 0.1, 0.5, 0.5, downsample=False, details=True)
    assert dp2.tolist() == dp.tolist() and dr2.tolist() == dr.tolist()


def test_pair_nan_where_numpy_gives_nan():
    m = eval_ref.eval_pair(np.zeros((0, 3)), TRGT, 0.02, 0.1, 0.5, 0.5)
    assert all(math.isnan(m[k]) for k in eval_ref.KEYS[:7]) and m["Spacing(m)"] == 0.02
    # every pred point an outlier: the precision side is empty (NaN), the recall side all clamped
    m = eval_ref.eval_pair(TRGT + 50.0, TRGT, 0.02, 0.1, 0.5, 0.5, downsample=False)
    assert math.isnan(m["MAE_accuracy(m)"]) and math.isnan(m["Precision[Accuracy](%)"]) and math.isnan(m["F-score(%)"])
    assert m["MAE_completeness(m)"] == 0.5 and m["Recall[Completeness](%)"] == 0.0
    # the same figures from the operator's own sums
    got = eval_ops.pair_metrics([0, 0, 0, 0, 3, 1.5, 0.75, 0], 0.02, 0.1, 0.5, 0.5)
    assert {k: v for k, v in got.items() if not math.isnan(v)} == {k: v for k, v in m.items() if not math.isnan(v)}
    assert [k for k, v in got.items() if math.isnan(v)] == [k for k, v in m.items() if math.isnan(v)]


ANCHOR_CLOUD = np.array([[0.2, 0.0, 0.0], [0.8, 0.0, 0.0], [1.1, 0.0, 0.0]])


def test_voxel_grid_is_anchored_half_a_cell_below_the_minimum():
    # anchor -0.3: cells floor(0.5), floor(1.1), floor(1.4) = 0, 1, 1; a grid anchored at 0 would give 0, 0, 1
    c = eval_ref.voxel_centroids(ANCHOR_CLOUD, 1.0)
    assert np.allclose(c, [[0.2, 0, 0], [0.95, 0, 0]], rtol=0, atol=1e-15)
    at_origin = eval_ref.voxel_centroids(ANCHOR_CLOUD, 1.0, cells=np.floor(ANCHOR_CLOUD).astype(np.int64))
    assert np.allclose(at_origin, [[0.5, 0, 0], [1.1, 0, 0]], rtol=0, atol=1e-15)


def test_voxel_order_is_x_fastest():
    p = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    assert eval_ref.voxel_centroids(p, 0.5).tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]


def test_backprojection_of_a_2x2_image():
    depth = np.array([[1.0, 0.0], [2.0, 3.0]])            # one zero, one pixel equal to depth_trunc: both dropped
    rgb = np.stack([np.full((2, 2), 0.5), np.full((2, 2), 1.0), np.full((2, 2), 0.999)]).astype(np.float32)
    K = (2.0, 2.0, 0.5, 0.5)
    pts, col, pix = eval_ref.backproject_depth(depth, K, np.eye(4), 3.0, rgb=rgb)
    assert pix.tolist() == [0, 2]                          # row-major pixel order
    assert pts.tolist() == [[-0.25, -0.25, 1.0], [-0.5, 0.5, 2.0]]
    assert np.array_equal(col, [[127 / 255, 1.0, 254 / 255]] * 2)
    # extrinsic maps world to camera: a camera displaced by t sees world points at cam - t
    E = np.eye(4)
    E[:3, 3] = [1.0, 2.0, 3.0]
    pts2, _, _ = eval_ref.backproject_depth(depth, K, E, 3.0)
    assert np.allclose(pts2, pts - [1.0, 2.0, 3.0], rtol=0, atol=1e-15)
    # an alpha mask drops pixels as a zero depth does
    _, _, pix3 = eval_ref.backproject_depth(depth, K, E, 3.0, alpha=np.array([[0.4, 1.0], [0.9, 1.0]]), min_alpha=0.4)
    assert pix3.tolist() == [2]


def test_view_metrics_by_hand():
    rgb, gt = np.full((1, 1, 2), 0.5), np.full((1, 1, 2), 0.25)
    d, g = np.array([[1.0, 2.0]]), np.array([[1.5, 5.0]])
    m = eval_ref.view_metrics(rgb, gt, d, g, depth_min=0.5, depth_max=5.0)      # gt 5.0 is not < 5.0
    assert m["mse"].tolist() == [0.0625] and m["psnr"] == pytest.approx(20 * math.log10(4.0))
    assert (m["depth_l1"], m["depth_rmse"], m["n_valid"]) == (0.5, 0.5, 1)
    m = eval_ref.view_metrics(rgb, rgb, d, g, depth_min=2.0, depth_max=5.0)
    assert m["psnr"] == math.inf and math.isnan(m["depth_l1"]) and math.isnan(m["depth_rmse"]) and m["n_valid"] == 0


# ------------------------------------------------------------------ argument checks, before any GPU work
def test_operators_check_their_arguments():
    f = torch.zeros
    kw = dict(depth_min=0.1, depth_max=10.0)
    with pytest.raises(ValueError):
        eval_ops.view_metrics(f(3, 4), f(3, 4), **kw)
    with pytest.raises(ValueError):
        eval_ops.view_metrics(f(3, 4, 5), f(3, 4, 6), **kw)
    with pytest.raises(TypeError):
        eval_ops.view_metrics(f(3, 4, 5, dtype=torch.float64), f(3, 4, 5), **kw)
    with pytest.raises(_lib.PingsHipError, match="no CPU fallback"):
        eval_ops.view_metrics(f(3, 4, 5), f(3, 4, 5), **kw)
    with pytest.raises(ValueError):
        eval_ops.backproject_depth(f(4, 5, 6), (1, 1, 0, 0), np.eye(4), 5.0)
    with pytest.raises(TypeError):
        eval_ops.backproject_depth(np.zeros((4, 5), np.float32), (1, 1, 0, 0), np.eye(4), 5.0)
    with pytest.raises(_lib.PingsHipError):
        eval_ops.backproject_depth(f(1, 4, 5), (1, 1, 0, 0), np.eye(4), 5.0)
    with pytest.raises(ValueError):
        eval_ops.voxel_centroids(f(7, 2), 0.1)
    with pytest.raises(ValueError):
        eval_ops.voxel_centroids(f(7, 3), 0.0)
    with pytest.raises(TypeError):
        eval_ops.voxel_centroids(f(7, 3, dtype=torch.float16), 0.1)
    with pytest.raises(_lib.PingsHipError):
        eval_ops.voxel_centroids(f(7, 3), 0.1)
    with pytest.raises(ValueError):
        eval_ops.nn_distance(f(7, 3), f(3, 7), 1.0)
    with pytest.raises(ValueError):
        eval_ops.nn_distance(f(7, 3), f(7, 3), math.inf)
    with pytest.raises(TypeError):
        eval_ops.nn_distance(f(7, 3), f(7, 3, dtype=torch.int32), 1.0)
    with pytest.raises(_lib.PingsHipError):
        eval_ops.nn_distance(f(7, 3), f(7, 3), 1.0)
    with pytest.raises(ValueError):
        eval_ops.eval_pair(np.zeros((4, 2)), np.zeros((4, 3)))
    with pytest.raises(ValueError):
        eval_ops.eval_pair(np.zeros((4, 3)), np.zeros((4, 3)), threshold=-1.0)
    with pytest.raises(_lib.PingsHipError):
        eval_ops.eval_pair(f(4, 3), f(4, 3))
    # empty clouds never reach the device: numpy's NaN, and the reference's empty lists
    assert math.isnan(eval_ops.eval_pair(np.zeros((0, 3)), NS(points=np.zeros((5, 3))))["F-score(%)"])
    assert eval_ops.nn_correspondance(np.zeros((0, 3)), np.zeros((5, 3)), 0.5) == ([], [])
    assert eval_ops.default_cell(1.0, 0.05) == 0.125 and eval_ops.default_cell(0.5, 0.2) == 0.4


def test_entry_points_reject_null_pointers_and_empty_shapes():
    L = _lib.lib()
    calls = {
        "pings_eval_view_metrics": (None, None, 3, 16, None, None, None, 0.0, 1.0, 0.0, 0, None, None, None, None),
        "pings_eval_backproject": (None, None, None, 4, 4, None, None, 1.0, 0.0, 0, None, None, None, None, None),
        "pings_eval_voxel_centroids": (None, 8, None, 0.1, None, None, None, None, None),
        "pings_eval_nn_build": (None, 8, None, 0.1, None, None, None),
        "pings_eval_nn_query": (None, 8, None, None, 8, 0.1, 0.5, None, None, None),
        "pings_eval_pair_reduce": (None, 8, None, None, 8, None, 0.1, 0.5, None, None, None),
    }
    for name, args in calls.items():
        assert getattr(L, name)(*args) == 1, name
        assert b"null" in L.pings_last_error(), name
    for name in ("pings_eval_view_metrics_scratch_bytes", "pings_eval_backproject_scratch_bytes",
                 "pings_eval_voxel_scratch_bytes", "pings_eval_nn_scratch_bytes"):
        assert getattr(L, name)(0) == 0, name
        assert getattr(L, name)(1000) > 0, name
    # empty shapes and a truncation that spans too many cells are status codes too (pointers need only be non-null)
    p = 4096
    assert L.pings_eval_voxel_centroids(p, 0, None, 0.1, p, p, p, p, None) == 1
    assert L.pings_eval_nn_build(p, 0, None, 0.1, p, p, None) == 1
    assert L.pings_eval_nn_query(p, 8, None, p, 8, 0.001, 1.0, p, p, None) == 1
    assert b"too many cells" in L.pings_last_error()
    assert L.pings_eval_view_metrics(p, p, 5, 16, None, None, None, 0.0, 1.0, 0.0, 0, None, p, p, None) == 1


def test_install_binds_both_names():
    mod = NS(eval_pair=None, nn_correspondance=None, eval_mesh=lambda: None)
    eval_ops.install(mod)
    assert mod.eval_pair is eval_ops.eval_pair and mod.nn_correspondance is eval_ops.nn_correspondance
