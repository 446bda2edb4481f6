"""fp64 numpy restatement of pose-graph optimisation (pings_amd/pgo_ops.py, csrc/pgo.hip).

The contract: poses X_n in SE(3) as T_world<-frame 4x4.  A between factor (i, j, Z, W) has the whitened residual
r = W Log(Z^-1 X_i^-1 X_j), a prior (i, Z, W) has r = W Log(Z^-1 X_i); Log is the full SE(3) logarithm, rotation first,
translation multiplied by V^-1.  Cost = 1/2 sum |r|^2.  Updates X_n <- X_n Exp(delta_n).  Levenberg-Marquardt with
lambda diag(H) damping, lambda / 10 on an accepted trial and * 10 on a rejected one; every trial counts as one
iteration; it stops at max_iter, after an accepted trial whose relative decrease is at most rel_tol, or when lambda
passes LAMBDA_MAX.  Everything here is dense and slow on purpose.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

Record = namedtuple("Record", "cost_before cost_after lam accepted status iteration")

SERIES_ANGLE = 1e-2         # below it the trigonometric coefficients are their Taylor series (three terms)
NEAR_PI = 0.1               # residual rotations within this of pi are out of contract
LAMBDA_MAX = 1e5            # GTSAM's lambdaUpperBound
ST_NEAR_PI, ST_NOT_POSDEF, ST_NONFINITE, ST_CONVERGED, ST_LAMBDA_MAX = 1, 2, 4, 8, 16


def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def coeffs(th):
    """sin t / t, (1 - cos t) / t^2, (t - sin t) / t^3, (t^2 + 2 cos t - 2) / (2 t^4),
    (2 t - 3 sin t + t cos t) / (2 t^5), 1 / t^2 - (1 + cos t) / (2 t sin t)."""
    t2 = th * th
    if th < SERIES_ANGLE:
        return (1.0 - t2 / 6.0 + t2 * t2 / 120.0, 0.5 - t2 / 24.0 + t2 * t2 / 720.0,
                1.0 / 6.0 - t2 / 120.0 + t2 * t2 / 5040.0, 1.0 / 24.0 - t2 / 720.0 + t2 * t2 / 40320.0,
                1.0 / 120.0 - t2 / 2520.0 + t2 * t2 / 120960.0, 1.0 / 12.0 + t2 / 720.0 + t2 * t2 / 30240.0)
    s, c = np.sin(th), np.cos(th)
    return (s / th, (1.0 - c) / t2, (th - s) / (t2 * th), (t2 + 2.0 * c - 2.0) / (2.0 * t2 * t2),
            (2.0 * th - 3.0 * s + th * c) / (2.0 * t2 * t2 * th), 1.0 / t2 - (1.0 + c) / (2.0 * th * s))


def exp_se3(xi):
    """xi = (omega, v) -> 4x4 with R = Exp(omega), t = V v."""
    w, v = np.asarray(xi[:3], float), np.asarray(xi[3:], float)
    th = np.sqrt(w @ w)
    a, b, c = coeffs(th)[:3]
    Wm = skew(w)
    W2 = Wm @ Wm
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + a * Wm + b * W2
    T[:3, 3] = (np.eye(3) + b * Wm + c * W2) @ v
    return T


def log_so3(R):
    """(omega, theta): theta = atan2(|s|, (tr - 1) / 2) with s = vee(R - R^T) / 2, omega = s theta / sin theta."""
    s = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    sn = np.sqrt(s @ s)
    th = np.arctan2(sn, 0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1.0))
    if th < SERIES_ANGLE:
        k = 1.0 + th * th / 6.0 + 7.0 * th ** 4 / 360.0
    else:
        k = th / sn
    return s * k, th


def log_se3(T):
    """4x4 -> (xi, theta), xi = (omega, V^-1 t)."""
    w, th = log_so3(T[:3, :3])
    Wm = skew(w)
    e = coeffs(th)[5]
    v = (np.eye(3) - 0.5 * Wm + e * (Wm @ Wm)) @ T[:3, 3]
    return np.concatenate([w, v]), th


def inv_se3(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def adjoint(T):
    """Ad(T) in the rotation-first order: [[R, 0], [[t]x R, R]]."""
    R, t = T[:3, :3], T[:3, 3]
    A = np.zeros((6, 6))
    A[:3, :3] = R
    A[3:, 3:] = R
    A[3:, :3] = skew(t) @ R
    return A


def dlog(xi):
    """d Log(T Exp(d)) / d d at T = Exp(xi): the inverse right Jacobian of SE(3), [[A, 0], [-A Q A, A]]."""
    w, v = np.asarray(xi[:3], float), np.asarray(xi[3:], float)
    th = np.sqrt(w @ w)
    _, _, a1, a2, a3, e = coeffs(th)
    Wm, V = skew(-w), skew(-v)                      # the right Jacobian is the left one at -xi
    W2 = Wm @ Wm
    A = np.eye(3) - 0.5 * Wm + e * W2
    WV, VW = Wm @ V, V @ Wm
    WVW = WV @ Wm
    Q = (0.5 * V + a1 * (WV + VW + WVW) + a2 * (Wm @ WV + VW @ Wm - 3.0 * WVW)
         + a3 * (WVW @ Wm + Wm @ WVW))
    J = np.zeros((6, 6))
    J[:3, :3] = A
    J[3:, 3:] = A
    J[3:, :3] = -A @ Q @ A
    return J


def sqrt_info_sigmas(sigmas):
    return np.diag(1.0 / np.asarray(sigmas, float))


def sqrt_info_cov(cov):
    """W with W^T W = cov^-1: the transposed Cholesky factor of the information matrix."""
    return np.linalg.cholesky(np.linalg.inv(np.asarray(cov, float))).T


def residual(Xi, Xj, Z, W):
    """(r, theta) of one factor; Xj None for a prior."""
    h = Xi if Xj is None else inv_se3(Xi) @ Xj
    xi, th = log_se3(inv_se3(Z) @ h)
    return W @ xi, th


def jacobians(Xi, Xj, Z, W):
    """(r, J_i, J_j) with respect to X <- X Exp(d); for a prior J_i is the only one and J_j is None."""
    h = Xi if Xj is None else inv_se3(Xi) @ Xj
    xi, _ = log_se3(inv_se3(Z) @ h)
    Jj = W @ dlog(xi)
    if Xj is None:
        return W @ xi, Jj, None
    return W @ xi, -Jj @ adjoint(inv_se3(h)), Jj


class RefGraph:
    """The interface of pgo_ops.PoseGraph on the host, dense."""

    def __init__(self):
        self.X = []             # 4x4 each
        self.factors = []       # (i, j or -1, Z, W)
        self.records = []
        self._before = None

    # ---- growth
    def num_nodes(self):
        return len(self.X)

    def num_factors(self):
        return len(self.factors)

    def add_node(self, pose):
        self.X.append(np.array(pose, float))
        return len(self.X) - 1

    def add_prior(self, i, Z, W):
        self.factors.append((int(i), -1, np.array(Z, float), np.array(W, float)))

    def add_between(self, i, j, Z, W):
        assert i != j
        self.factors.append((int(i), int(j), np.array(Z, float), np.array(W, float)))

    def remove_last(self):
        self.factors.pop()

    def poses(self):
        return np.stack(self.X) if self.X else np.zeros((0, 4, 4))

    def pose_diff(self):
        before = self._before if self._before is not None else self.poses()
        return np.stack([a @ inv_se3(b) for a, b in zip(self.X, before)])

    # ---- cost
    def error(self, values=None, order=None):
        X = self.X if values is None else values
        total, status = 0.0, 0
        for f in (range(len(self.factors)) if order is None else order):
            i, j, Z, W = self.factors[f]
            r, th = residual(X[i], None if j < 0 else X[j], Z, W)
            total += 0.5 * (r @ r)
            if th > np.pi - NEAR_PI:
                status |= ST_NEAR_PI
        self.status = status
        return total

    def linearize(self, X, order=None):
        n = len(X)
        H, g = np.zeros((6 * n, 6 * n)), np.zeros(6 * n)
        for f in (range(len(self.factors)) if order is None else order):
            i, j, Z, W = self.factors[f]
            r, Ji, Jj = jacobians(X[i], None if j < 0 else X[j], Z, W)
            si = slice(6 * i, 6 * i + 6)
            H[si, si] += Ji.T @ Ji
            g[si] += Ji.T @ r
            if j >= 0:
                sj = slice(6 * j, 6 * j + 6)
                H[sj, sj] += Jj.T @ Jj
                H[sj, si] += Jj.T @ Ji
                H[si, sj] += Ji.T @ Jj
                g[sj] += Jj.T @ r
        return H, g

    @staticmethod
    def solve_damped(H, g, lam):
        d = np.diag(H).copy()
        A = H + lam * np.diag(d)
        s = 1.0 / np.sqrt(np.where(d > 0, d * (1.0 + lam), 1.0))       # symmetric scaling: the prior spans 1e18
        return s * np.linalg.solve(A * s[:, None] * s[None, :], -g * s)

    def optimize(self, max_iter=50, rel_tol=1e-5, lambda0=1e-5, order=None):
        """Returns one Record per trial."""
        self._before = self.poses()
        lam, status = float(lambda0), 0
        self.records = []
        for it in range(max_iter):
            before = self.error(order=order)
            status |= self.status
            H, g = self.linearize(self.X, order)
            delta = self.solve_damped(H, g, lam)
            cand = [x @ exp_se3(delta[6 * n:6 * n + 6]) for n, x in enumerate(self.X)]
            after = self.error(cand, order)
            status |= self.status
            if not np.isfinite(after):
                status |= ST_NONFINITE
            accepted = bool(after <= before)
            used = lam
            if accepted:
                self.X = cand
                lam /= 10.0
                if before - after <= rel_tol * before:
                    status |= ST_CONVERGED
            else:
                lam *= 10.0
                if lam > LAMBDA_MAX:
                    status |= ST_LAMBDA_MAX
            self.records.append(Record(before, after, used, accepted, status, it))
            if status & (ST_CONVERGED | ST_LAMBDA_MAX):
                break
        return self.records


def tridiagonal_woodbury_solve(graph: RefGraph, X, lam):
    """The device's route in numpy: T = tridiagonal part + lam diag(H), U from the factors with |i - j| > 1,
    delta = T^-1 b - T^-1 U (I + U^T T^-1 U)^-1 U^T T^-1 b with b = -g.  Returns delta."""
    n = len(X)
    T, g, cols = np.zeros((6 * n, 6 * n)), np.zeros(6 * n), []
    hd = np.zeros(6 * n)
    for i, j, Z, W in graph.factors:
        r, Ji, Jj = jacobians(X[i], None if j < 0 else X[j], Z, W)
        si = slice(6 * i, 6 * i + 6)
        g[si] += Ji.T @ r
        hd[si] += np.sum(Ji * Ji, axis=0)
        if j >= 0:
            sj = slice(6 * j, 6 * j + 6)
            g[sj] += Jj.T @ r
            hd[sj] += np.sum(Jj * Jj, axis=0)
        if j >= 0 and abs(i - j) > 1:
            U = np.zeros((6 * n, 6))
            U[si] = Ji.T
            U[sj] = Jj.T
            cols.append(U)
            continue
        T[si, si] += Ji.T @ Ji
        if j >= 0:
            T[sj, sj] += Jj.T @ Jj
            T[sj, si] += Jj.T @ Ji
            T[si, sj] += Ji.T @ Jj
    T += lam * np.diag(hd)
    s = 1.0 / np.sqrt(np.where(np.diag(T) > 0, np.diag(T), 1.0))
    Ts = T * s[:, None] * s[None, :]
    solve = lambda B: (s[:, None] * np.linalg.solve(Ts, s[:, None] * B.reshape(6 * n, -1))).reshape(B.shape)
    x0 = solve(-g)
    if not cols:
        return x0
    U = np.concatenate(cols, axis=1)
    Y = solve(U)
    y = np.linalg.solve(np.eye(U.shape[1]) + U.T @ Y, U.T @ x0)
    return x0 - Y @ y


# ---------------------------------------------------------------- synthetic graphs
def random_pose(rng, rot=0.5, tran=2.0):
    return exp_se3(np.concatenate([rng.normal(0, rot, 3), rng.normal(0, tran, 3)]))


def loop_graph(n, loops, seed=0, rot_std_deg=0.01, tran_std=0.04, noise_rot=2e-3, noise_tran=8e-3, fixed_sigma=1e-9,
               graph=None):
    """A closed-ring trajectory of n poses (one turn of a circle of about 1 m steps), odometry with accumulated noise,
    a fixed prior on node 0 and exact loop factors for the (i, j) pairs in `loops`.  Returns (graph, true poses)."""
    rng = np.random.default_rng(seed)
    g = RefGraph() if graph is None else graph
    step = exp_se3(np.array([0.0, 0.0, 2.0 * np.pi / max(n, 8), 1.0, 0.0, 0.0]))
    truth = [np.eye(4)]
    for _ in range(n - 1):
        truth.append(truth[-1] @ step)
    sig = np.array([np.radians(rot_std_deg)] * 3 + [tran_std] * 3)
    W = sqrt_info_sigmas(sig)
    odom = [np.eye(4)]
    meas = []
    for k in range(n - 1):
        z = step @ exp_se3(np.concatenate([rng.normal(0, noise_rot, 3), rng.normal(0, noise_tran, 3)]))
        meas.append(z)
        odom.append(odom[-1] @ z)
    for k in range(n):
        g.add_node(odom[k])
    g.add_prior(0, np.eye(4), sqrt_info_sigmas([fixed_sigma] * 6))
    for k in range(n - 1):
        g.add_between(k, k + 1, meas[k], W)
    for i, j in loops:
        g.add_between(i, j, inv_se3(truth[i]) @ truth[j], W)
    return g, truth


# ---------------------------------------------------------------- g2o text
def parse_g2o(text):
    """{'vertices': {id: 4x4}, 'edges': [(i, j, 4x4, information 6x6 in g2o's translation-first order)]}."""
    verts, edges = {}, []
    for line in text.splitlines():
        p = line.split()
        if not p:
            continue
        if p[0] == "VERTEX_SE3:QUAT":
            verts[int(p[1])] = _pose_from_tq([float(x) for x in p[2:9]])
        elif p[0] == "EDGE_SE3:QUAT":
            vals = [float(x) for x in p[10:31]]
            info = np.zeros((6, 6))
            info[np.triu_indices(6)] = vals
            info = info + info.T - np.diag(np.diag(info))
            edges.append((int(p[1]), int(p[2]), _pose_from_tq([float(x) for x in p[3:10]]), info))
    return {"vertices": verts, "edges": edges}


def _pose_from_tq(v):
    x, y, z, qx, qy, qz, qw = v
    T = np.eye(4)
    T[:3, :3] = np.array([
        [1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
        [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
        [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])
    T[:3, 3] = [x, y, z]
    return T


# ---------------------------------------------------------------- the graphs of tests/test_pgo_ops.py
def _loops257(count):
    return [(10 * k, 250 - 7 * k) for k in range(count)]


def build_case(name, g):
    """Fills `g` (a RefGraph or anything with its add_* methods) with the named graph; the same calls in the same order
    whatever `g` is, so a device graph and the reference hold identical numbers."""
    const = sqrt_info_sigmas([np.radians(0.01)] * 3 + [0.04] * 3)
    if name == "n1":
        rng = np.random.default_rng(11)
        x = random_pose(rng)
        g.add_node(x)
        g.add_prior(0, x @ exp_se3(rng.normal(0, 0.1, 6)), const)
    elif name == "n2":
        loop_graph(2, [], seed=2, graph=g)
    elif name == "n3_loop":
        loop_graph(3, [(0, 2)], seed=3, graph=g)
    elif name == "n64":
        loop_graph(64, [(0, 63)], seed=4, graph=g)
    elif name == "n65":
        loop_graph(65, [(0, 64), (2, 40)], seed=5, graph=g)
    elif name.startswith("n257_L"):
        loop_graph(257, _loops257(int(name[6:])), seed=6, graph=g)
    elif name == "shared_node":
        loop_graph(48, [(3, 30), (3, 44)], seed=7, graph=g)
    elif name == "same_pair_twice":
        loop_graph(48, [(5, 40), (5, 40)], seed=8, graph=g)
    elif name == "consecutive_loop":
        loop_graph(48, [(7, 8), (21, 20), (2, 45)], seed=9, graph=g)
    elif name == "full_covariance":
        _, truth = loop_graph(48, [(1, 40)], seed=10, graph=g)
        A = np.random.default_rng(10).normal(0, 1, (6, 6))
        cov = (A @ A.T + 6.0 * np.eye(6)) * np.outer([2e-4] * 3 + [3e-2] * 3, [2e-4] * 3 + [3e-2] * 3)
        g.add_between(4, 36, inv_se3(truth[4]) @ truth[36], sqrt_info_cov(cov))
    elif name == "prior_all":
        loop_graph(48, [(0, 47)], seed=12, graph=g)
        radius = 0.3
        W = sqrt_info_sigmas([radius * np.radians(10.0)] * 3 + [radius + 1e-4] * 3)
        for n, x in enumerate(g.poses()):
            if n > 0:
                g.add_prior(n, x, W)
    elif name == "at_optimum":
        for n in range(20):                             # exactly representable: every residual is exactly zero
            x = np.eye(4)
            x[0, 3] = float(n)
            g.add_node(x)
        g.add_prior(0, np.eye(4), sqrt_info_sigmas([1e-9] * 6))
        z = np.eye(4)
        z[0, 3] = 1.0
        for n in range(19):
            g.add_between(n, n + 1, z, const)
        z5 = np.eye(4)
        z5[0, 3] = 12.0
        g.add_between(3, 15, z5, const)
    elif name == "rejected_step":
        # 20 m steps, exact measurements, a start whose heading error accumulates to about 2 rad: the optimum has cost
        # zero, and once the cost is down at the rounding floor a trial's cost comes out above the one before it
        rng = np.random.default_rng(0)
        n = 24
        step = exp_se3(np.array([0.0, 0.0, 2.0 * np.pi / n, 20.0, 0.0, 0.0]))
        truth, x = [np.eye(4)], np.eye(4)
        for _ in range(n - 1):
            truth.append(truth[-1] @ step)
        g.add_node(x)
        for _ in range(n - 1):
            x = x @ step @ exp_se3(np.concatenate([rng.normal(0, 2.0 / np.sqrt(n), 3), np.zeros(3)]))
            g.add_node(x)
        g.add_prior(0, np.eye(4), sqrt_info_sigmas([1e-9] * 6))
        for k in range(n - 1):
            g.add_between(k, k + 1, step, const)
        for i, j in ((0, 23), (4, 16)):
            g.add_between(i, j, inv_se3(truth[i]) @ truth[j], const)
    else:
        raise KeyError(name)
    return g


COMPARED = ["n1", "n2", "n3_loop", "n64", "n65", "n257_L0", "n257_L1", "n257_L10", "n257_L11", "shared_node",
            "same_pair_twice", "consecutive_loop", "full_covariance", "prior_all"]


def pose_gap(A, B):
    """(largest translation gap, largest rotation angle) between two pose lists."""
    dt = max(float(np.linalg.norm(a[:3, 3] - b[:3, 3])) for a, b in zip(A, B))
    dr = max(float(log_so3(a[:3, :3].T @ b[:3, :3])[1]) for a, b in zip(A, B))
    return dt, dr


def measure_spread(names=COMPARED):
    """The gap between two fp64 minimisers of the same graphs: factor order permuted and lambda_0 * 100 against the
    plain run, both to rel_tol = 1e-12.  tests/test_pgo_ops.py takes ten times the largest as its bound."""
    worst_t = worst_r = 0.0
    for name in names:
        a = build_case(name, RefGraph())
        a.optimize(50, 1e-12)
        b = build_case(name, RefGraph())
        order = np.random.default_rng(99).permutation(len(b.factors))
        b.optimize(50, 1e-12, lambda0=1e-3, order=order)
        dt, dr = pose_gap(a.X, b.X)
        print(f"{name:18s} trials {len(a.records):2d} / {len(b.records):2d}  translation {dt:.3e} m  rotation {dr:.3e} rad")
        worst_t, worst_r = max(worst_t, dt), max(worst_r, dr)
    print(f"largest spread: translation {worst_t:.3e} m, rotation {worst_r:.3e} rad")
    return worst_t, worst_r


if __name__ == "__main__":
    measure_spread()
