"""Pose-graph optimisation without a device: the fp64 restatement tests/pgo_ref.py against itself (the mathematics the
device kernels are tested against in tests/test_pgo_ops.py) and the host side of pings_amd/pgo_ops.py (factor
classification, g2o text, the manager's bookkeeping on a `pgo_ref.RefGraph`, install / uninstall).

The 40-node, 3-loop graph: the figures 2164 -> 167.893 quoted when the unit was proposed came from a generator that was
not recorded; `pgo_ref.loop_graph(40, ..., seed=0)` is this repository's graph with the same shape and sigmas, its
figures are 3413.10 -> 242.818, and what is asserted is what that run established: the dense Levenberg-Marquardt
converges in a few trials and the tridiagonal-plus-Woodbury solve agrees with the dense one to rounding.
"""
import types

import numpy as np
import pytest

import pgo_ref as R
from pings_amd import pgo_ops


def _numeric_jacobian(fn, h=1e-6):
    cols = []
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        cols.append((fn(d) - fn(-d)) / (2 * h))
    return np.stack(cols, axis=1)


@pytest.mark.parametrize("angle", [0.0, 1e-12, 1e-9, 1e-8, 1e-5, 9.99e-3, 1.001e-2, 0.3, 1.5, 2.9])
def test_exp_log_round_trip(angle):
    rng = np.random.default_rng(3)
    w = rng.normal(0, 1, 3)
    xi = np.concatenate([w / np.linalg.norm(w) * angle, rng.normal(0, 3, 3)])
    T = R.exp_se3(xi)
    back, th = R.log_se3(T)
    assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-15)
    assert abs(th - angle) <= 1e-15 + 1e-13 * angle
    assert np.abs(back - xi).max() <= 1e-14 * max(1.0, np.abs(xi).max())
    assert np.abs(R.exp_se3(back) - T).max() <= 1e-14 * max(1.0, np.abs(T).max())


def test_series_and_closed_forms_meet_at_the_threshold():
    below, above = R.coeffs(R.SERIES_ANGLE * (1 - 1e-9)), R.coeffs(R.SERIES_ANGLE * (1 + 1e-9))
    # the closed forms cancel: (2 t - 3 sin t + t cos t) / (2 t^5) keeps about six digits at t = 1e-2
    for a, b, tol in zip(below, above, (1e-12, 1e-11, 1e-10, 1e-6, 1e-4, 1e-10)):
        assert abs(a - b) <= tol * abs(a)


@pytest.mark.parametrize("angle", [1e-9, 5e-3, 2e-2, 0.7, 2.5])
def test_dlog_against_central_differences(angle):
    rng = np.random.default_rng(4)
    w = rng.normal(0, 1, 3)
    xi = np.concatenate([w / np.linalg.norm(w) * angle, rng.normal(0, 1, 3)])
    T = R.exp_se3(xi)
    num = _numeric_jacobian(lambda d: R.log_se3(T @ R.exp_se3(d))[0])
    assert np.abs(R.dlog(xi) - num).max() <= 2e-9


@pytest.mark.parametrize("prior", [False, True])
def test_factor_jacobians_against_central_differences(prior):
    rng = np.random.default_rng(5)
    Xi, Xj = R.random_pose(rng), R.random_pose(rng)
    A = rng.normal(0, 1, (6, 6))
    W = R.sqrt_info_cov((A @ A.T + 6 * np.eye(6)) * 1e-2)
    if prior:
        Z = Xi @ R.exp_se3(rng.normal(0, 0.4, 6))
        r, Ji, Jj = R.jacobians(Xi, None, Z, W)
        assert Jj is None
        num = _numeric_jacobian(lambda d: R.residual(Xi @ R.exp_se3(d), None, Z, W)[0])
        assert np.abs(Ji - num).max() <= 1e-8 * np.abs(Ji).max()
        return
    Z = R.inv_se3(Xi) @ Xj @ R.exp_se3(rng.normal(0, 0.4, 6))
    r, Ji, Jj = R.jacobians(Xi, Xj, Z, W)
    num_i = _numeric_jacobian(lambda d: R.residual(Xi @ R.exp_se3(d), Xj, Z, W)[0])
    num_j = _numeric_jacobian(lambda d: R.residual(Xi, Xj @ R.exp_se3(d), Z, W)[0])
    assert np.abs(Ji - num_i).max() <= 1e-8 * np.abs(Ji).max()
    assert np.abs(Jj - num_j).max() <= 1e-8 * np.abs(Jj).max()


def test_sqrt_information_of_a_covariance():
    A = np.random.default_rng(6).normal(0, 1, (6, 6))
    cov = A @ A.T + np.eye(6)
    for W in (R.sqrt_info_cov(cov), pgo_ops.sqrt_info_from_covariance(cov)):
        assert np.allclose(W.T @ W, np.linalg.inv(cov), rtol=1e-12, atol=1e-14)
        assert np.allclose(W, np.triu(W))
    assert np.array_equal(pgo_ops.sqrt_info_from_sigmas([0.5, 1, 2, 4, 8, 16]), np.diag([2, 1, .5, .25, .125, .0625]))


def test_two_node_graph_with_a_closed_form_optimum():
    """Node 0 fixed at the origin, two translation-only measurements of node 1 with weights wa, wb: the optimum is
    their information-weighted mean and the cost there is wa^2 wb^2 / (wa^2 + wb^2) |ta - tb|^2 / 2."""
    ta, tb, wa, wb = np.array([1.0, 0.5, -0.25]), np.array([1.5, 0.0, 0.25]), 3.0, 5.0
    g = R.RefGraph()
    g.add_node(np.eye(4))
    g.add_node(R.exp_se3([0.3, -0.2, 0.1, 4.0, 4.0, 4.0]))
    g.add_prior(0, np.eye(4), R.sqrt_info_sigmas([1e-9] * 6))
    for t, w in ((ta, wa), (tb, wb)):
        Z = np.eye(4)
        Z[:3, 3] = t
        g.add_between(0, 1, Z, w * np.eye(6))
    recs = g.optimize(30, 1e-14)
    want = (wa ** 2 * ta + wb ** 2 * tb) / (wa ** 2 + wb ** 2)
    assert np.abs(g.X[1][:3, 3] - want).max() <= 1e-9
    assert np.abs(g.X[1][:3, :3] - np.eye(3)).max() <= 1e-9
    assert np.abs(g.X[0] - np.eye(4)).max() <= 1e-12
    cost = 0.5 * wa ** 2 * wb ** 2 / (wa ** 2 + wb ** 2) * np.sum((ta - tb) ** 2)
    assert abs(recs[-1].cost_after - cost) <= 1e-9 * cost
    costs = [r.cost_after for r in recs if r.accepted]
    assert all(b <= a for a, b in zip(costs, costs[1:]))


def test_forty_nodes_three_loops():
    g, truth = R.loop_graph(40, [(0, 39), (5, 30), (10, 25)], seed=0)
    drift = np.linalg.norm(g.X[-1][:3, 3] - truth[-1][:3, 3])
    assert 0.05 < drift < 1.0
    H, grad = g.linearize(g.X)
    dense = g.solve_damped(H, grad, 1e-5)
    direct = R.tridiagonal_woodbury_solve(g, g.X, 1e-5)
    assert np.abs(dense - direct).max() <= 1e-12 * np.abs(dense).max()
    recs = g.optimize(50, 1e-5)
    assert len(recs) <= 4 and all(r.accepted for r in recs) and recs[-1].status == R.ST_CONVERGED
    assert abs(recs[0].cost_before - 3413.1049) <= 1e-3
    assert abs(recs[-1].cost_after - 242.8179) <= 1e-3
    after, _ = R.pose_gap(g.X, truth)
    assert after < 0.5 * drift


def test_classify_builds_the_lists_the_kernels_read():
    fi = np.array([0, 0, 1, 2, 0, 3, 0, 2], np.int32)
    fj = np.array([-1, 1, 2, 3, 3, 2, 3, -1], np.int32)
    kind, lcol, loop_f, node_off, node_ent = pgo_ops.classify(fi, fj, 4)
    assert kind.tolist() == [0, 1, 1, 1, 2, 1, 2, 0]
    assert lcol.tolist() == [-1, -1, -1, -1, 0, -1, 1, -1] and loop_f.tolist() == [4, 6]
    assert node_off.tolist() == [0, 4, 6, 10, 14]
    assert node_ent.tolist() == [0, 2, 8, 12, 3, 4, 5, 6, 11, 14, 7, 9, 10, 13]
    with pytest.raises(ValueError):
        pgo_ops.classify(np.array([0, 4]), np.array([-1, 1]), 4)
    with pytest.raises(ValueError):
        pgo_ops.classify(np.array([2]), np.array([2]), 4)


def test_g2o_text_round_trip():
    g = R.build_case("full_covariance", R.RefGraph())
    fi = [f[0] for f in g.factors]
    fj = [f[1] for f in g.factors]
    Z, W = np.stack([f[2] for f in g.factors]), np.stack([f[3] for f in g.factors])
    text = pgo_ops.g2o_text(g.poses(), fi, fj, Z, W)
    lines = text.splitlines()
    assert sum(l.startswith("VERTEX_SE3:QUAT ") for l in lines) == 48
    assert sum(l.startswith("EDGE_SE3:QUAT ") for l in lines) == len(g.factors) - 1     # the prior has no line
    assert all(len(l.split()) == (9 if l.startswith("V") else 31) for l in lines)
    back = R.parse_g2o(text)
    for n, x in enumerate(g.poses()):
        assert np.abs(back["vertices"][n] - x).max() <= 1e-14 * max(1.0, np.abs(x).max())
    between = [f for f in g.factors if f[1] >= 0]
    perm = [3, 4, 5, 0, 1, 2]
    for (i, j, z, info), (fi_, fj_, z_, w_) in zip(back["edges"], between):
        assert (i, j) == (fi_, fj_)
        assert np.abs(z - z_).max() <= 1e-14 * max(1.0, np.abs(z_).max())
        want = (w_.T @ w_)[np.ix_(perm, perm)]
        assert np.abs(info - want).max() <= 1e-15 * np.abs(want).max()
    # the default sigmas: translation first in the file
    assert np.allclose(np.diag(back["edges"][0][3]), [625.0] * 3 + [1.0 / np.radians(0.01) ** 2] * 3)


def test_quaternions_of_half_turns():
    for axis in range(3):
        w = np.zeros(3)
        w[axis] = np.pi - 1e-3
        Rm = R.exp_se3(np.concatenate([w, np.zeros(3)]))[:3, :3]
        q = pgo_ops._rot_to_quat(Rm)
        assert abs(np.linalg.norm(q) - 1.0) <= 1e-15
        assert np.abs(R._pose_from_tq([0, 0, 0, *q])[:3, :3] - Rm).max() <= 1e-15


# ---------------------------------------------------------------- the manager on a RefGraph
def _config(**over):
    base = dict(silence=True, pgo_tran_std=0.04, pgo_rot_std=0.01, end_frame=1000, pgo_with_isam=False,
                pgo_error_thre_frame=500.0, pgo_max_iter=50, device="cpu")
    base.update(over)
    return types.SimpleNamespace(**base)


def _drive(pgm, poses, odom, frames, loop=None):
    """pings.py:555-604 for the frames given: node, init_poses, odometry, drift, then the loop and the correction."""
    travel = np.concatenate([[0.0], np.cumsum([np.linalg.norm(z[:3, 3]) for z in odom])])
    accepted = None
    for frame_id in frames:
        pgm.add_frame_node(frame_id, poses[frame_id])
        pgm.init_poses = poses[:frame_id + 1]
        if frame_id > 0:
            pgm.add_odometry_factor(frame_id, frame_id - 1, odom[frame_id - 1])
            pgm.estimate_drift(travel[:frame_id + 1], frame_id, correct_ratio=0.01)
        if loop is not None and frame_id == loop[0]:
            accepted = pgm.add_loop_factor(frame_id, loop[1], loop[2])
            if accepted:
                pgm.optimize_pose_graph()
                pgm.loop_edges.append(np.array([loop[1], frame_id], dtype=np.uint32))
                pgm.loop_trans.append(loop[2])
                pgm.last_loop_idx = frame_id
                pgm.min_loop_idx = min(pgm.min_loop_idx, loop[1])
    return travel, accepted


def _trajectory(n=40, seed=0):
    src, truth = R.loop_graph(n, [], seed=seed)
    poses = src.poses()
    odom = [f[2] for f in src.factors if f[1] >= 0]
    return poses, odom, truth


def test_manager_follows_the_reference_call_order():
    poses, odom, truth = _trajectory()
    pgm = pgo_ops.PoseGraphManager(_config(), graph=R.RefGraph())
    pgm.add_pose_prior(0, poses[0], fixed=True)         # pings.py:193, before the node exists
    assert pgm.min_loop_idx == 1001 and pgm.last_loop_idx == 0 and pgm.pgo_count == 0
    loop_tf = R.inv_se3(truth[2]) @ truth[39]
    travel, accepted = _drive(pgm, poses, odom, range(40), loop=(39, 2, loop_tf))
    assert accepted is True
    assert pgm.curr_node_idx == 39 and pgm.pgo_count == 1 and pgm.last_loop_idx == 39 and pgm.min_loop_idx == 2
    assert pgm.drift_radius == pytest.approx((travel[39] - travel[0]) * 0.01)
    assert pgm.pgo_poses.shape == (40, 4, 4) and pgm.cur_pose.shape == (4, 4)
    assert np.array_equal(pgm.cur_pose, pgm.pgo_poses[39])
    diff = pgm.get_pose_diff()
    assert diff.shape == (40, 4, 4)
    assert np.abs(diff @ poses - pgm.pgo_poses).max() <= 1e-12
    assert np.abs(diff[0] - np.eye(4)).max() <= 1e-9                       # the fixed node stays
    before = np.linalg.norm(poses[39][:3, 3] - (truth[2] @ loop_tf)[:3, 3])
    after = np.linalg.norm(pgm.pgo_poses[39][:3, 3] - (pgm.pgo_poses[2] @ loop_tf)[:3, 3])
    assert after < 0.1 * before
    recs = pgm.graph.records
    assert pgm.last_error == [r.cost_after for r in recs if r.accepted][-1]
    # a second drive: the drift estimate now carries the corrected part (min_loop_idx < last_loop_idx)
    pgm.estimate_drift(travel, 39, correct_ratio=0.01)
    assert pgm.drift_radius == pytest.approx((travel[2] + travel[39] * 0.01) * 0.01)


def test_manager_rejects_a_loop_by_the_error_threshold():
    poses, odom, truth = _trajectory()
    pgm = pgo_ops.PoseGraphManager(_config(pgo_error_thre_frame=50.0), graph=R.RefGraph())
    pgm.add_pose_prior(0, poses[0], fixed=True)
    _drive(pgm, poses, odom, range(40))
    base = pgm.graph.error()
    count = pgm.graph.num_factors()
    good = R.inv_se3(poses[2]) @ poses[39] @ R.exp_se3([0, 0, 0, 0.3, 0, 0])     # error 0.5 (0.3 / 0.04)^2 = 28.1
    bad = R.inv_se3(poses[2]) @ poses[39] @ R.exp_se3([0, 0, 0, 3.0, 0, 0])      # error 2812
    thre = 0.0 + 39 * 50.0
    assert pgm.add_loop_factor(39, 2, bad) is False
    assert pgm.graph.num_factors() == count and pgm.graph.error() == base
    pgm.last_error = 1000.0                               # the threshold moves with the last optimised error
    assert thre + 1000.0 > 2812.5 + base
    assert pgm.add_loop_factor(39, 2, bad) is True
    pgm.graph.remove_last()
    pgm.last_error = 0.0
    assert pgm.add_loop_factor(39, 2, bad, reject_outlier=False) is True
    pgm.graph.remove_last()
    assert pgm.add_loop_factor(39, 2, good) is True
    assert pgm.graph.num_factors() == count + 1
    isam = pgo_ops.PoseGraphManager(_config(pgo_with_isam=True, pgo_error_thre_frame=50.0), graph=R.RefGraph())
    isam.add_pose_prior(0, poses[0], fixed=True)
    _drive(isam, poses, odom, range(40))
    assert isam.add_loop_factor(39, 2, bad) is True       # the reference does not test the error under iSAM


def test_manager_priors_covariances_and_gaps():
    poses, odom, _ = _trajectory(8)
    g = R.RefGraph()
    pgm = pgo_ops.PoseGraphManager(_config(), graph=g)
    pgm.add_frame_node(0, poses[0])
    pgm.add_frame_node(0, poses[3])                       # an existing node keeps its value
    assert g.num_nodes() == 1 and np.array_equal(g.X[0], poses[0])
    with pytest.raises(ValueError):
        pgm.add_frame_node(2, poses[2])
    pgm.add_pose_prior(0, poses[0], fixed=True)
    assert np.array_equal(np.diag(g.factors[-1][3]), np.full(6, 1.0 / 1e-9))
    pgm.drift_radius = 0.5
    pgm.add_pose_prior(0, poses[0])
    assert np.allclose(np.diag(g.factors[-1][3]), [1 / (0.5 * np.radians(10.0))] * 3 + [1 / 0.5001] * 3)
    pgm.add_frame_node(1, poses[1])
    cov = np.diag([1e-6, 2e-6, 3e-6, 1e-3, 2e-3, 3e-3]) + 1e-7
    pgm.add_odometry_factor(1, 0, odom[0], cov=cov)
    i, j, Z, W = g.factors[-1]
    assert (i, j) == (0, 1) and np.array_equal(Z, odom[0])
    assert np.allclose(W.T @ W, np.linalg.inv(cov), rtol=1e-10)
    pgm.add_odometry_factor(1, 0, odom[0])
    assert np.allclose(np.diag(g.factors[-1][3]), [1 / np.radians(0.01)] * 3 + [25.0] * 3)


def test_manager_files_and_offline_pgo(tmp_path):
    poses, odom, truth = _trajectory(30)
    pgm = pgo_ops.PoseGraphManager(_config(), graph=R.RefGraph())
    pgm.loop_edges = [np.array([1, 29], dtype=np.uint32), np.array([4, 20], dtype=np.uint32)]
    pgm.loop_trans = [R.inv_se3(truth[1]) @ truth[29], R.inv_se3(truth[4]) @ truth[20]]
    pgm.write_loops(tmp_path / "loops.txt")
    other = pgo_ops.PoseGraphManager(_config(), graph=R.RefGraph())
    assert other.read_loops(tmp_path / "loops.txt") is True
    assert [e.tolist() for e in other.loop_edges] == [[1, 29], [4, 20]]
    assert all(np.abs(a[:3] - b[:3]).max() <= 1e-6 for a, b in zip(other.loop_trans, pgm.loop_trans))
    assert pgm.read_loops(tmp_path / "absent.txt") is False and pgm.loop_edges == []     # as the reference: cleared
    other.loop_trans = [np.vstack([t, [0, 0, 0, 1.0]]) for t in other.loop_trans]
    other.offline_pgo(poses)
    assert other.pgo_poses.shape == (30, 4, 4) and other.pgo_count == 1
    assert R.pose_gap(other.pgo_poses, truth)[0] < R.pose_gap(poses, truth)[0]
    with pytest.raises(Exception, match="plot_loops"):
        other.plot_loops(tmp_path / "loops.png")


def test_install_and_uninstall_on_a_stub_module():
    class Original:
        def plot_loops(self, path, vis_now=False):
            return ("drawn", len(self.pgo_poses), path)

    pgo_mod, importer = types.ModuleType("utils.pgo"), types.ModuleType("pings")
    pgo_mod.PoseGraphManager = importer.PoseGraphManager = Original
    try:
        pgo_ops.install(pgo_mod, importer)
        pgo_ops.install(pgo_mod, importer)                # twice changes nothing
        assert pgo_mod.PoseGraphManager is pgo_ops.PoseGraphManager is importer.PoseGraphManager
        assert pgo_mod._pings_pose_graph_manager_original is Original
        pgm = importer.PoseGraphManager(_config(), graph=R.RefGraph())
        pgm.pgo_poses = np.zeros((3, 4, 4))
        assert pgm.plot_loops("x.png") == ("drawn", 3, "x.png")
    finally:
        pgo_ops.uninstall(pgo_mod, importer)
    assert pgo_mod.PoseGraphManager is Original and importer.PoseGraphManager is Original
    assert not hasattr(pgo_mod, "_pings_pose_graph_manager_original")
    assert pgo_ops.PoseGraphManager._original is None


def test_a_graph_needs_a_hip_device():
    with pytest.raises(Exception, match="HIP device"):
        pgo_ops.PoseGraph("cpu")
