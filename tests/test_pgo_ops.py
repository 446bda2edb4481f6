"""pings_amd.pgo_ops on the device against the fp64 restatement tests/pgo_ref.py, at the shapes where the kernels of
csrc/pgo.hip can go wrong: one and two nodes, a loop over three, 64 / 65 factors and nodes (launch tail), 257 nodes with
0, 1, 10 and 11 loops (1 + 6 L = 61 and 67 right-hand sides straddle a wave of columns; the graphs run with chunks of 64
columns so that 67 needs a second chunk), loops that share a node, the same pair twice, "loops" between consecutive
nodes in both directions, a full covariance, a drift-radius prior on every node, a graph at its optimum, rejected
trials, and `remove_last`.

Bounds.  `error()` is the same fp64 sum on both sides: 1e-12 relative, at values moved off the start so that the cost is
not rounding noise.  Final poses are compared with `pgo_ref` run to rel_tol = 1e-12; the gap between two fp64 minimisers
is set by the stopping rule, not by the device, so the bound is measured: `python tests/pgo_ref.py` runs the reference
against itself over `pgo_ref.COMPARED` with the factor order permuted and lambda_0 * 100 and prints the largest spread,
    translation 1.321e-08 m, rotation 2.342e-10 rad,
and the bounds below are ten times that.  `pose_diff @ before == after` is fp64 rounding of 4x4 products of poses
whose entries stay below 100: 64 * 2^-53 * 100 < 1e-12.
"""
import functools
import types

import numpy as np
import pytest
import torch

import pgo_ref as R
from pings_amd import _lib, pgo_ops

pytestmark = pytest.mark.gpu

TRAN_BOUND = 10 * 1.321e-08      # m
ROT_BOUND = 10 * 2.342e-10       # rad
CHUNK = 64


def _device_graph(name):
    return R.build_case(name, pgo_ops.PoseGraph("cuda", chunk=CHUNK))


def _moved(poses, seed=21):
    rng = np.random.default_rng(seed)
    # node 0 of a graph with several nodes stays: its fixed prior (weight 1e18) would otherwise be the whole cost
    return np.stack([x if n == 0 and len(poses) > 1 else
                     x @ R.exp_se3(np.concatenate([rng.normal(0, 0.02, 3), rng.normal(0, 0.1, 3)]))
                     for n, x in enumerate(poses)])


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(cost at the moved values, optimised poses, records) of the reference; computed once and shared."""
    g = R.build_case(name, R.RefGraph())
    moved = _moved(g.poses())
    cost = g.error(list(moved))
    recs = g.optimize(50, 1e-12)
    return cost, np.stack(g.X), recs


def _check_records(recs):
    assert [r.iteration for r in recs] == list(range(len(recs)))
    cost = recs[0].cost_before
    for a, b in zip(recs, recs[1:]):
        assert b.lam == pytest.approx(a.lam / 10.0 if a.accepted else a.lam * 10.0, rel=1e-14)
    for r in recs:
        assert r.cost_before == cost                    # a rejected trial leaves the poses where they were
        assert np.isfinite(r.cost_before) and not (r.status & (pgo_ops.ST_NOT_POSDEF | pgo_ops.ST_NEAR_PI))
        if r.accepted:
            assert r.cost_after <= cost
            cost = r.cost_after
        else:
            assert not r.cost_after <= cost


@pytest.mark.parametrize("name", R.COMPARED)
def test_device_matches_reference(name):
    want_cost, want_poses, _ = _reference(name)
    g = _device_graph(name)
    before = g.poses()
    n = before.shape[0]
    got_cost = g.error(_moved(before))
    print(f"{name}: error {got_cost!r} reference {want_cost!r}")
    assert abs(got_cost - want_cost) <= 1e-12 * want_cost
    assert g.last_status == 0

    _lib.sync_counts(reset=True)
    recs = g.optimize(50, 1e-12)
    counts = _lib.sync_counts(reset=True)
    assert counts == {"pgo_iteration": len(recs)}
    assert 1 <= len(recs) <= 50
    if recs[0].cost_before > 1e-6:                      # n257_L0 starts at its optimum: its cost is rounding noise
        assert recs[-1].status & pgo_ops.ST_CONVERGED
    _check_records(recs)

    after = g.poses_torch()
    dt, dr = R.pose_gap(after.cpu().numpy(), want_poses)
    print(f"{name}: {len(recs)} trials, gap to the reference {dt:.3e} m {dr:.3e} rad")
    assert dt <= TRAN_BOUND and dr <= ROT_BOUND

    again = _device_graph(name)
    again_recs = again.optimize(50, 1e-12)
    assert torch.equal(again.poses_torch(), after) and again_recs == recs

    diff = g.pose_diff()
    assert diff.dtype == torch.float64 and tuple(diff.shape) == (n, 4, 4)
    before_t = torch.from_numpy(before).to(diff.device)
    assert (diff @ before_t - after).abs().max().item() <= 1e-12
    assert torch.equal(g.pose_diff(torch.float32), diff.to(torch.float32))
    assert np.array_equal(g.poses(), after.cpu().numpy())


def test_graph_at_its_optimum():
    g = _device_graph("at_optimum")
    before = g.poses_torch()
    assert g.error() == 0.0
    recs = g.optimize(10, 1e-5)
    assert len(recs) == 1 and recs[0].accepted and recs[0].status == pgo_ops.ST_CONVERGED
    assert recs[0].cost_before == 0.0 and recs[0].cost_after == 0.0
    assert torch.equal(g.poses_torch(), before)         # delta = 0 exactly, and no NaN
    eye = torch.eye(4, dtype=torch.float64, device=before.device).expand(20, 4, 4)
    assert torch.equal(g.pose_diff(), eye)


def test_rejected_trials_raise_lambda_and_never_raise_the_cost():
    g = _device_graph("rejected_step")
    start = g.error()
    _lib.sync_counts(reset=True)
    recs = g.optimize(40, 1e-5, lambda0=1e-12)
    assert _lib.sync_counts(reset=True) == {"pgo_iteration": len(recs)}
    assert recs[0].lam == 1e-12 and recs[0].cost_before == start and start > 1e6
    _check_records(recs)
    rejected = [k for k, r in enumerate(recs) if not r.accepted]
    print("accepted:", "".join("1" if r.accepted else "0" for r in recs), "final", recs[-1])
    assert rejected, "no trial was rejected"
    assert all(recs[k + 1].lam > recs[k].lam for k in rejected if k + 1 < len(recs))
    final = min(r.cost_after for r in recs if r.accepted)
    assert final <= 1e-12 * start
    assert g.error() == final


def test_remove_last_after_a_rejected_loop_leaves_the_error_bitwise():
    cfg = types.SimpleNamespace(silence=True, pgo_tran_std=0.04, pgo_rot_std=0.01, end_frame=1000, pgo_with_isam=False,
                                pgo_error_thre_frame=500.0, pgo_max_iter=50, device="cuda", dtype=torch.float32)
    src, truth = R.loop_graph(40, [], seed=0)
    poses = src.poses()
    odom = [f[2] for f in src.factors if f[1] >= 0]
    ref = pgo_ops.PoseGraphManager(cfg, graph=R.RefGraph())
    dev = pgo_ops.PoseGraphManager(cfg)
    assert isinstance(dev.graph, pgo_ops.PoseGraph)
    for pgm in (ref, dev):
        pgm.add_pose_prior(0, poses[0], fixed=True)
        for k in range(40):
            pgm.add_frame_node(k, poses[k])
            pgm.init_poses = poses[:k + 1]
            if k > 0:
                pgm.add_odometry_factor(k, k - 1, odom[k - 1])
    base = dev.graph.error(_moved(poses))
    assert abs(base - ref.graph.error(list(_moved(poses)))) <= 1e-12 * base
    bad = R.inv_se3(poses[2]) @ poses[39] @ R.exp_se3([0, 0, 0, 30.0, 0, 0])   # 0.5 (30 / 0.04)^2 > 39 * 500
    assert dev.add_loop_factor(39, 2, bad) is False and ref.add_loop_factor(39, 2, bad) is False
    assert dev.graph.num_factors() == 40 and dev.graph.error(_moved(poses)) == base
    good = R.inv_se3(truth[2]) @ truth[39]
    assert dev.add_loop_factor(39, 2, good) is True and ref.add_loop_factor(39, 2, good) is True
    dev.optimize_pose_graph()
    ref.optimize_pose_graph()
    assert dev.pgo_count == 1 and dev.pgo_poses.shape == (40, 4, 4)
    # both stopped at the first accepted trial whose decrease was at most 1e-5 of the cost; what a converging run
    # still had to gain is less than its last decrease, so the two costs agree to 2e-5, and a cost gap dc over the
    # weakest information (625 / m^2, 1 / radians(0.01)^2) bounds the pose gap by sqrt(2 dc / information)
    assert dev.last_error == pytest.approx(ref.last_error, rel=2e-5)
    dt, dr = R.pose_gap(dev.pgo_poses, ref.pgo_poses)
    dc = 2e-5 * ref.last_error
    assert dt <= np.sqrt(2 * dc / 625.0) and dr <= np.sqrt(2 * dc) * np.radians(0.01)
    diff = dev.pose_diff_torch()
    assert diff.dtype == torch.float32 and diff.is_cuda
    assert np.abs(diff.cpu().numpy() - dev.get_pose_diff()).max() <= 1e-5   # fp32 rounding of entries below 50
    text = dev.graph.g2o()
    assert text.count("VERTEX_SE3:QUAT") == 40 and text.count("EDGE_SE3:QUAT") == 40


def test_pose_diff_feeds_adjust_map_like_the_numpy_round_trip():
    from pings_amd import neural_map as NM

    g = _device_graph("n64")
    init = g.poses()
    g.optimize(50, 1e-5)
    rng = np.random.default_rng(5)
    n = 100
    pts = torch.from_numpy(rng.normal(0, 5, (n, 3)).astype(np.float32))
    quat = torch.from_numpy(rng.normal(0, 1, (n, 4)).astype(np.float32))
    quat = quat / quat.norm(dim=1, keepdim=True)
    ts = torch.from_numpy(rng.integers(0, 64, n).astype(np.int32))

    def new_map():
        return types.SimpleNamespace(neural_points=pts.clone().cuda(), point_orientations=quat.clone().cuda(),
                                     point_ts_create=ts.clone().cuda(), point_ts_update=ts.clone().cuda(),
                                     use_mid_ts=False, after_pgo=False)

    for dtype in (torch.float32, torch.float64):
        a, b = new_map(), new_map()
        NM.adjust_map(a, g.pose_diff(dtype))
        host = np.matmul(g.poses(), np.linalg.inv(init))                 # pings.py:595: numpy, then torch.tensor(...)
        NM.adjust_map(b, torch.tensor(host, device="cuda", dtype=dtype))
        moved = (a.neural_points - pts.cuda()).norm(dim=1).max().item()
        assert moved > 1e-3
        if dtype is torch.float64:
            # X_after X_before^-1 by the rigid inverse against numpy's LU inverse: fp64 rounding of entries below 50,
            # then the fp32 points of adjust_map round both the same way except at a tie
            assert (a.neural_points - b.neural_points).abs().max().item() <= 4e-6
            assert (a.point_orientations - b.point_orientations).abs().max().item() <= 2e-7
        else:
            # the two fp32 matrices differ by at most one rounding of an entry below 4 (2^-22), times a point of at
            # most 25 m, three terms and the translation; the quaternion sees rotation entries one ulp of 1 apart
            assert (a.neural_points - b.neural_points).abs().max().item() <= 4 * 2.0 ** -22 * 25
            assert (a.point_orientations - b.point_orientations).abs().max().item() <= 1e-6


def test_the_graph_refuses_what_it_cannot_hold():
    g = pgo_ops.PoseGraph("cuda")
    with pytest.raises(ValueError):
        g.error()
    g.add_node(np.eye(4))
    g.add_prior(1, np.eye(4), np.eye(6))                 # node 1 does not exist yet
    with pytest.raises(ValueError):
        g.error()
    g.add_node(np.eye(4))
    assert g.error() == 0.0
    with pytest.raises(ValueError):
        g.add_between(1, 1, np.eye(4), np.eye(6))
    with pytest.raises(ValueError):
        pgo_ops.PoseGraph("cuda", chunk=100)
