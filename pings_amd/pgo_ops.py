"""Pose-graph optimisation on the HIP device (csrc/pgo.hip).

`PoseGraph` is the device graph: SE(3) nodes 0 .. N-1, prior and between factors with 6x6 square-root information
(rotation first), the cost 1/2 sum |W Log(Z^-1 X_i^-1 X_j)|^2 and Levenberg-Marquardt whose trials are solved, judged
and committed by the device; the host reads one record per trial.  `PoseGraphManager` follows the reference's
`utils/pgo.py` (a wrapper over GTSAM) method for method on top of it, and `install` rebinds the reference's name.
There is no CPU path: a graph is created on a HIP device.  `PoseGraphManager(config, graph=...)` takes any object with
`PoseGraph`'s methods, which is how the bookkeeping is tested without a device.
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional

import numpy as np
import torch

from . import _abi, _lib

ST_NEAR_PI, ST_NOT_POSDEF, ST_NONFINITE = _abi.PGO_ST_NEAR_PI, _abi.PGO_ST_NOT_POSDEF, _abi.PGO_ST_NONFINITE
ST_CONVERGED, ST_LAMBDA_MAX = _abi.PGO_ST_CONVERGED, _abi.PGO_ST_LAMBDA_MAX
FIXED_SIGMA = 1e-9          # the reference's `fixed_cov`


class TrialRecord(NamedTuple):
    cost_before: float
    cost_after: float
    lam: float              # the damping this trial was solved with
    accepted: bool
    status: int             # ST_* bits, sticky over one `optimize`
    iteration: int


# ---------------------------------------------------------------- host helpers (numpy, fp64)
def sqrt_info_from_sigmas(sigmas) -> np.ndarray:
    """`noiseModel.Diagonal.Sigmas`: W = diag(1 / sigma)."""
    return np.diag(1.0 / np.asarray(sigmas, dtype=np.float64))


def sqrt_info_from_covariance(cov) -> np.ndarray:
    """`noiseModel.Gaussian.Covariance`: W with W^T W = cov^-1, the transposed Cholesky factor of the information."""
    return np.ascontiguousarray(np.linalg.cholesky(np.linalg.inv(np.asarray(cov, dtype=np.float64))).T)


def classify(fi: np.ndarray, fj: np.ndarray, n_nodes: int):
    """(kind, lcol, loop_f, node_off, node_ent) of a factor list, as csrc/pgo.hip reads them: kind PGO_PRIOR /
    PGO_CHAIN (|i - j| = 1) / PGO_LOOP, the loops numbered in factor order, and per node the entries 2 f + slot
    (slot 0: the node is fi) in factor order, so that duplicates are summed and every sum has one order."""
    fi, fj = np.asarray(fi, np.int64), np.asarray(fj, np.int64)
    if fi.size and (fi.min() < 0 or fi.max() >= n_nodes or fj.min() < -1 or fj.max() >= n_nodes):
        raise ValueError(f"pgo_ops: a factor names a node outside 0 .. {n_nodes - 1}")
    if np.any(fi == fj):
        raise ValueError("pgo_ops: a between factor joins a node with itself")
    kind = np.where(fj < 0, _abi.PGO_PRIOR, np.where(np.abs(fi - fj) == 1, _abi.PGO_CHAIN, _abi.PGO_LOOP))
    is_loop = kind == _abi.PGO_LOOP
    lcol = np.where(is_loop, np.cumsum(is_loop) - 1, -1)
    loop_f = np.nonzero(is_loop)[0]
    f = np.arange(fi.size, dtype=np.int64)
    has_j = fj >= 0
    nodes = np.concatenate([fi, fj[has_j]])
    ents = np.concatenate([2 * f, 2 * f[has_j] + 1])
    order = np.lexsort((ents, nodes))                   # by node, then by factor and slot
    node_off = np.zeros(n_nodes + 1, dtype=np.int64)
    np.cumsum(np.bincount(nodes, minlength=n_nodes), out=node_off[1:])
    as32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    return as32(kind), as32(lcol), as32(loop_f), as32(node_off), as32(ents[order])


def _rot_to_quat(R: np.ndarray):
    """(qx, qy, qz, qw) of a rotation matrix, qw >= 0."""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2.0
        q = ((R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s)
    else:
        k = int(np.argmax(np.diag(R)))
        a, b = (k + 1) % 3, (k + 2) % 3
        s = np.sqrt(1.0 + R[k, k] - R[a, a] - R[b, b]) * 2.0
        v = [0.0, 0.0, 0.0]
        v[k] = 0.25 * s
        v[a] = (R[a, k] + R[k, a]) / s
        v[b] = (R[b, k] + R[k, b]) / s
        q = (v[0], v[1], v[2], (R[b, a] - R[a, b]) / s)
    q = np.asarray(q, dtype=np.float64)
    return q if q[3] >= 0 else -q


def g2o_text(poses: np.ndarray, fi, fj, Z: np.ndarray, W: np.ndarray) -> str:
    """The graph as g2o text: one `VERTEX_SE3:QUAT id x y z qx qy qz qw` per node and one `EDGE_SE3:QUAT i j x y z qx
    qy qz qw` + the 21 upper-triangular entries of the information matrix, in g2o's translation-first order, per
    between factor.  Priors have no g2o line (GTSAM's writer leaves them out as well)."""
    perm = [3, 4, 5, 0, 1, 2]
    iu = np.triu_indices(6)
    lines = []
    for n, X in enumerate(poses):
        q = _rot_to_quat(X[:3, :3])
        lines.append("VERTEX_SE3:QUAT %d " % n + " ".join(repr(float(v)) for v in (*X[:3, 3], *q)))
    for f in range(len(fi)):
        if fj[f] < 0:
            continue
        q = _rot_to_quat(Z[f][:3, :3])
        info = (W[f].T @ W[f])[np.ix_(perm, perm)]
        lines.append("EDGE_SE3:QUAT %d %d " % (fi[f], fj[f]) +
                     " ".join(repr(float(v)) for v in (*Z[f][:3, 3], *q, *info[iu])))
    return "\n".join(lines) + "\n"


def _pose_array(pose, what: str) -> np.ndarray:
    if isinstance(pose, torch.Tensor):
        pose = pose.detach().cpu().numpy()
    a = np.asarray(pose, dtype=np.float64)
    if a.shape != (4, 4):
        raise ValueError(f"pgo_ops: {what} must be 4x4, got {a.shape}")
    return a


# ---------------------------------------------------------------- the device graph
class PoseGraph:
    """Nodes and factors live in device buffers that grow by doubling; a host mirror of what was added feeds them, so
    adding a node or a factor costs one small copy to the device at the next use and no host wait."""

    def __init__(self, device="cuda", chunk: int = 128):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.PingsHipError("pgo_ops.PoseGraph runs on the HIP device only; there is no CPU fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if chunk < 64 or chunk % 64:
            raise ValueError("pgo_ops: chunk must be a multiple of 64")
        self.chunk = int(chunk)
        self._n = self._f = 0                           # nodes, factors
        self._n_up = self._f_up = 0                     # of which already on the device
        self._Xh = np.zeros((16, 4, 4))
        self._fih, self._fjh = np.zeros(16, np.int32), np.zeros(16, np.int32)
        self._Zh, self._Wh = np.zeros((16, 4, 4)), np.zeros((16, 6, 6))
        f64 = dict(dtype=torch.float64, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        self._Xd = torch.zeros((16, 4, 4), **f64)
        self._fid, self._fjd = torch.zeros(16, **i32), torch.zeros(16, **i32)
        self._Zd, self._Wd = torch.zeros((16, 4, 4), **f64), torch.zeros((16, 6, 6), **f64)
        self._host_stale = False                        # the device holds newer poses than _Xh
        self._lists = None                              # (n, f, tensors) of the last classification
        self._scratch = torch.empty(0, dtype=torch.uint8, device=self.device)
        self._state = torch.zeros(8, **f64)
        self._record = torch.zeros(_abi.PGO_RECORD, **f64)
        self._status = torch.zeros(1, **i32)
        self._cost = torch.zeros(1, **f64)
        self._before: Optional[torch.Tensor] = None     # poses at the start of the last optimize
        self.records: List[TrialRecord] = []
        self.last_status = 0

    # ---- growth
    def num_nodes(self) -> int:
        return self._n

    def num_factors(self) -> int:
        return self._f

    @staticmethod
    def _grown(host: np.ndarray, need: int) -> np.ndarray:
        if need <= host.shape[0]:
            return host
        out = np.zeros((max(need, 2 * host.shape[0]),) + host.shape[1:], dtype=host.dtype)
        out[:host.shape[0]] = host
        return out

    def _grown_dev(self, dev: torch.Tensor, need: int, keep: int) -> torch.Tensor:
        if need <= dev.shape[0]:
            return dev
        out = torch.zeros((max(need, 2 * dev.shape[0]),) + tuple(dev.shape[1:]), dtype=dev.dtype, device=dev.device)
        out[:keep] = dev[:keep]
        return out

    def add_node(self, pose) -> int:
        """Appends node N with the initial value `pose` (T_world<-frame, 4x4) and returns its id."""
        self._Xh = self._grown(self._Xh, self._n + 1)
        self._Xh[self._n] = _pose_array(pose, "a pose")
        self._n += 1
        return self._n - 1

    def set_poses(self, values) -> None:
        """Replaces the value of every node ([N, 4, 4], numpy or tensor); the factors stay."""
        vals = values.detach().cpu().numpy() if isinstance(values, torch.Tensor) else values
        vals = np.asarray(vals, dtype=np.float64)
        if vals.shape != (self._n, 4, 4):
            raise ValueError(f"pgo_ops: values must be [{self._n}, 4, 4], got {vals.shape}")
        self._Xh[:self._n] = vals
        self._n_up = 0                                  # everything is sent again at the next use
        self._host_stale = False

    def _add(self, i: int, j: int, Z, W) -> None:
        W = np.asarray(W, dtype=np.float64)
        if W.shape != (6, 6):
            raise ValueError(f"pgo_ops: the square-root information must be 6x6, got {W.shape}")
        if i < 0 or j < -1 or i == j:
            raise ValueError(f"pgo_ops: bad factor nodes ({i}, {j})")
        need = self._f + 1
        self._fih, self._fjh = self._grown(self._fih, need), self._grown(self._fjh, need)
        self._Zh, self._Wh = self._grown(self._Zh, need), self._grown(self._Wh, need)
        self._fih[self._f], self._fjh[self._f] = i, j
        self._Zh[self._f], self._Wh[self._f] = _pose_array(Z, "a measurement"), W
        self._f += 1
        self._lists = None

    def add_prior(self, i: int, Z, W) -> None:
        """r = W Log(Z^-1 X_i).  The node may be added later, before the graph is next used."""
        self._add(int(i), -1, Z, W)

    def add_between(self, i: int, j: int, Z, W) -> None:
        """r = W Log(Z^-1 X_i^-1 X_j), Z = T_i<-j."""
        self._add(int(i), int(j), Z, W)

    def remove_last(self) -> None:
        """Drops the factor added last; everything before it stays where it is, bit for bit."""
        if self._f == 0:
            raise IndexError("pgo_ops: the graph has no factor")
        self._f -= 1
        self._f_up = min(self._f_up, self._f)
        self._lists = None

    # ---- device state
    def _upload(self) -> None:
        n, f = self._n, self._f
        if n > self._n_up:
            self._Xd = self._grown_dev(self._Xd, n, self._n_up)
            self._Xd[self._n_up:n] = torch.from_numpy(self._Xh[self._n_up:n]).to(self.device)
            self._n_up = n
        if f > self._f_up:
            k = self._f_up
            self._fid, self._fjd = self._grown_dev(self._fid, f, k), self._grown_dev(self._fjd, f, k)
            self._Zd, self._Wd = self._grown_dev(self._Zd, f, k), self._grown_dev(self._Wd, f, k)
            self._fid[k:f] = torch.from_numpy(self._fih[k:f]).to(self.device)
            self._fjd[k:f] = torch.from_numpy(self._fjh[k:f]).to(self.device)
            self._Zd[k:f] = torch.from_numpy(self._Zh[k:f]).to(self.device)
            self._Wd[k:f] = torch.from_numpy(self._Wh[k:f]).to(self.device)
            self._f_up = f

    def _args(self) -> _abi.PgoArgs:
        n, f = self._n, self._f
        if n < 1 or f < 1:
            raise ValueError("pgo_ops: the graph needs at least one node and one factor")
        if self._lists is None or self._lists[0] != n:
            parts = classify(self._fih[:f], self._fjh[:f], n)
            self._lists = (n, f, [torch.from_numpy(p).to(self.device) for p in parts])
        self._upload()
        kind, lcol, loop_f, node_off, node_ent = self._lists[2]
        n_loops = int(loop_f.numel())
        L = _lib.lib()
        if not hasattr(L, "pings_pgo_scratch_bytes"):
            raise _lib.PingsHipError(f"{_lib.LIB_PATH} has no pings_pgo_scratch_bytes: rebuild it with "
                                     "`python -m pings_amd.build`")
        need = int(L.pings_pgo_scratch_bytes(n, f, n_loops, self.chunk))
        if need == 0:
            raise _lib.PingsHipError("pings_pgo_scratch_bytes refused the graph's shape")
        if self._scratch.numel() < need:
            self._scratch = torch.empty(max(need, 2 * self._scratch.numel()), dtype=torch.uint8, device=self.device)
        return _abi.PgoArgs(n, f, n_loops, int(node_ent.numel()), self.chunk, 0, 0.0,
                            self._fid.data_ptr(), self._fjd.data_ptr(), kind.data_ptr(), lcol.data_ptr(),
                            loop_f.data_ptr() if n_loops else None, node_off.data_ptr(), node_ent.data_ptr(),
                            self._Zd.data_ptr(), self._Wd.data_ptr(), self._Xd.data_ptr(), self._state.data_ptr(),
                            self._record.data_ptr(), self._status.data_ptr(), self._scratch.data_ptr())

    def _call(self, name: str, *args) -> None:
        L = _lib.lib()
        if not hasattr(L, name):    # a library built before this entry existed (same ABI version: additions only)
            raise _lib.PingsHipError(f"{_lib.LIB_PATH} has no {name}: rebuild it with `python -m pings_amd.build`")
        fn = getattr(L, name)
        if self.device.index != torch.cuda.current_device():
            with torch.cuda.device(self.device):
                st = fn(*args, _lib.stream_ptr(self.device))
        else:
            st = fn(*args, _lib.stream_ptr(self.device))
        _lib.check(st, name)

    # ---- cost and optimisation
    @torch.no_grad()
    def error(self, values=None) -> float:
        """1/2 sum |r|^2 at the graph's own poses, or at `values` [N, 4, 4] (numpy or tensor); one host read.
        `last_status` holds ST_NEAR_PI if a residual rotation is out of contract."""
        a = self._args()
        if values is None:
            vals = self._Xd
        else:
            vals = values if isinstance(values, torch.Tensor) else torch.from_numpy(np.asarray(values, np.float64))
            vals = vals.detach().to(device=self.device, dtype=torch.float64).contiguous()
            if tuple(vals.shape) != (self._n, 4, 4):
                raise ValueError(f"pgo_ops: values must be [{self._n}, 4, 4], got {tuple(vals.shape)}")
        self._status.zero_()
        self._call("pings_pgo_cost", C.byref(a), vals.data_ptr(), self._cost.data_ptr())
        _lib.note_sync("pgo_error")
        cost, status = torch.cat([self._cost, self._status.to(torch.float64)]).tolist()
        self.last_status = int(status)
        return cost

    @torch.no_grad()
    def optimize(self, max_iter: int = 50, rel_tol: float = 1e-5, lambda0: float = 1e-5) -> List[TrialRecord]:
        """Levenberg-Marquardt: at most `max_iter` trials (an accepted and a rejected trial count alike), lambda / 10
        after an accepted and * 10 after a rejected one.  It stops after an accepted trial whose decrease is at most
        `rel_tol` of the cost, or when lambda passes 1e5.  One host read per trial and none besides."""
        a = self._args()
        self._before = self._Xd[:self._n].clone()
        self._state.copy_(torch.tensor([lambda0, 0, 0, 0, 0, 0, 0, 0], dtype=torch.float64), non_blocking=True)
        self._status.zero_()
        a.rel_tol = float(rel_tol)
        host = (C.c_double * _abi.PGO_RECORD)()
        self.records = []
        for it in range(int(max_iter)):
            a.iteration = it
            self._call("pings_pgo_iteration", C.byref(a))
            self._call("pings_pgo_read_record", self._record.data_ptr(), C.addressof(host))
            _lib.note_sync("pgo_iteration")
            rec = TrialRecord(host[0], host[1], host[2], host[3] != 0.0, int(host[4]), int(host[5]))
            self.records.append(rec)
            if rec.status & (ST_CONVERGED | ST_LAMBDA_MAX):
                break
        self._host_stale = True
        self.last_status = self.records[-1].status if self.records else 0
        return self.records

    # ---- results
    def poses_torch(self) -> torch.Tensor:
        """[N, 4, 4] fp64 on the device (a copy)."""
        self._upload()
        return self._Xd[:self._n].clone()

    def poses(self) -> np.ndarray:
        """[N, 4, 4] fp64 on the host; one host read if an optimisation has run since the last call."""
        if self._host_stale:
            _lib.note_sync("pgo_poses")
            self._Xh[:self._n_up] = self._Xd[:self._n_up].cpu().numpy()
            self._host_stale = False
        return self._Xh[:self._n].copy()

    @torch.no_grad()
    def pose_diff(self, dtype=torch.float64) -> torch.Tensor:
        """[N, 4, 4] on the device: X_n now times the inverse of X_n at the start of the last `optimize` (identity for
        a node added since), computed in fp64 and rounded once to `dtype`."""
        self._upload()
        n = self._n
        after = self._Xd[:n].contiguous()
        before = after
        if self._before is not None:
            before = after.clone()
            before[:self._before.shape[0]] = self._before
        out64 = torch.empty((n, 4, 4), dtype=torch.float64, device=self.device) if dtype is not torch.float32 else None
        out32 = torch.empty((n, 4, 4), dtype=torch.float32, device=self.device) if dtype is torch.float32 else None
        self._call("pings_pgo_pose_diff", after.data_ptr(), before.data_ptr(), n,
                   out64.data_ptr() if out64 is not None else None, out32.data_ptr() if out32 is not None else None)
        if out32 is not None:
            return out32
        return out64 if dtype is torch.float64 else out64.to(dtype)

    def g2o(self) -> str:
        return g2o_text(self.poses(), self._fih[:self._f], self._fjh[:self._f], self._Zh[:self._f], self._Wh[:self._f])


# ---------------------------------------------------------------- the reference's manager
class PoseGraphManager:
    """`utils/pgo.py:PoseGraphManager` on `PoseGraph`: the same methods, attributes and return types.  Differences:
    `pgo_with_isam` runs the same Levenberg-Marquardt to convergence on the whole graph (iSAM2's single relinearisation
    per update is not reproduced, and the factors are kept); `plot_loops` is delegated to the reference's class when
    `install` kept one; the robust noise models the reference constructs and never uses are absent."""

    _original = None        # the class `install` replaced

    def __init__(self, config, graph=None):
        self.config = config
        self.silence = config.silence
        self.fixed_cov = np.full(6, FIXED_SIGMA)
        tran_std, rot_std = config.pgo_tran_std, config.pgo_rot_std         # m, degree
        self.const_cov = np.array([np.radians(rot_std)] * 3 + [tran_std] * 3)      # first rotation, then translation
        self.odom_cov = self.const_cov
        self.loop_cov = self.const_cov
        self.graph = graph if graph is not None else PoseGraph(getattr(config, "device", "cuda"))
        self.rel_tol = 1e-5                             # LevenbergMarquardtParams' relativeErrorTol

        self.cur_pose = None
        self.curr_node_idx = None
        self.graph_optimized = None
        self.init_poses = None      # as np.array
        self.pgo_poses = None       # as np.array

        self.loop_edges_vis = []
        self.loop_edges = []
        self.loop_trans = []

        self.min_loop_idx = config.end_frame + 1
        self.last_loop_idx = 0
        self.drift_radius = 0.0     # m
        self.pgo_count = 0
        self.last_error = 0.0

    # ---- graph
    def add_frame_node(self, frame_id, init_pose):
        """Creates the frame's node with its initial guess (4x4, T_world<-cur) if it does not exist yet."""
        self.curr_node_idx = frame_id
        n = self.graph.num_nodes()
        if frame_id < n:
            return
        if frame_id > n:
            raise ValueError(f"pgo_ops: node ids are 0 .. N-1; frame {frame_id} would leave a gap after {n - 1}")
        self.graph.add_node(init_pose)

    def add_pose_prior(self, frame_id: int, prior_pose: np.ndarray, fixed: bool = False):
        if fixed:
            sigmas = self.fixed_cov
        else:
            tran_sigma = self.drift_radius + 1e-4       # avoid divide by 0
            rot_sigma = self.drift_radius * np.radians(10.0)
            sigmas = np.array([rot_sigma] * 3 + [tran_sigma] * 3)
        self.graph.add_prior(frame_id, prior_pose, sqrt_info_from_sigmas(sigmas))

    def _between(self, cur_id, other_id, transform, cov, default):
        W = sqrt_info_from_sigmas(default) if cov is None else sqrt_info_from_covariance(cov)
        self.graph.add_between(other_id, cur_id, transform, W)

    def add_odometry_factor(self, cur_id: int, last_id: int, odom_transform: np.ndarray, cov=None):
        """`odom_transform` 4x4 as T_prev<-cur; `cov` a 6x6 covariance or None for the configured sigmas."""
        self._between(cur_id, last_id, odom_transform, cov, self.odom_cov)

    def add_loop_factor(self, cur_id: int, loop_id: int, loop_transform: np.ndarray, cov=None, reject_outlier=True):
        """`loop_transform` 4x4 as T_loop<-cur.  Returns False, with the factor removed again, when the graph's error
        at the current values passes `last_error + (cur_id - last_loop_idx) * pgo_error_thre_frame`."""
        self._between(cur_id, loop_id, loop_transform, cov, self.loop_cov)
        if reject_outlier and not self.config.pgo_with_isam:
            cur_error = self.graph.error()
            valid_error_thre = self.last_error + (cur_id - self.last_loop_idx) * self.config.pgo_error_thre_frame
            if cur_error > valid_error_thre:
                if not self.silence:
                    print("A loop edge rejected due to too large error")
                self.graph.remove_last()
                return False
        return True

    def optimize_pose_graph(self):
        records = self.graph.optimize(self.config.pgo_max_iter, self.rel_tol)
        if not self.config.pgo_with_isam and records:
            error_before = records[0].cost_before
            error_after = error_before
            for rec in records:
                if rec.accepted:
                    error_after = rec.cost_after
            self.last_error = error_after
            if not self.silence:
                print("PGO done")
                print("error %f --> %f:" % (error_before, error_after))
        self.graph_optimized = self.graph
        self.pgo_poses = np.array(self.init_poses, dtype=np.float64, copy=True)
        upto = self.curr_node_idx + 1
        self.pgo_poses[:upto] = self.graph.poses()[:upto]
        self.cur_pose = self.pgo_poses[self.curr_node_idx]
        self.pgo_count += 1

    def get_pose_diff(self):
        assert self.pgo_poses.shape[0] == self.init_poses.shape[0], \
            "poses before and after pgo must have the same size."
        return np.matmul(self.pgo_poses, np.linalg.inv(self.init_poses))

    def pose_diff_torch(self, dtype=None) -> torch.Tensor:
        """`get_pose_diff` without the host: [N, 4, 4] on the device in `dtype` (default `config.dtype`), ready for
        `adjust_map`, `transform_data_pool` and the camera pool."""
        if dtype is None:
            dtype = getattr(self.config, "dtype", torch.float32)
        return self.graph.pose_diff(dtype)

    def estimate_drift(self, travel_dist, used_frame_id, drfit_ratio=0.01, correct_ratio=0.005):
        self.drift_radius = (travel_dist[used_frame_id] - travel_dist[self.last_loop_idx]) * drfit_ratio
        if self.min_loop_idx < self.last_loop_idx:      # the loop has been corrected previously
            self.drift_radius += (travel_dist[self.min_loop_idx] + travel_dist[used_frame_id] * correct_ratio) \
                * drfit_ratio

    def offline_pgo(self, odom_poses):
        """PGO with known odometry and the loops of `read_loops` (for debugging); the result is `pgo_poses`."""
        self.graph = type(self.graph)(self.graph.device) if isinstance(self.graph, PoseGraph) else type(self.graph)()
        for i in range(len(odom_poses)):
            self.add_frame_node(i, odom_poses[i])
        self.add_pose_prior(0, odom_poses[0], fixed=True)
        for i in range(len(odom_poses) - 1):
            self.add_odometry_factor(i + 1, i, np.linalg.inv(odom_poses[i]) @ odom_poses[i + 1])
        for i in range(len(self.loop_edges)):
            self.add_loop_factor(int(self.loop_edges[i][1]), int(self.loop_edges[i][0]), self.loop_trans[i],
                                 reject_outlier=False)
        if self.init_poses is None:
            self.init_poses = np.asarray(odom_poses, dtype=np.float64)
        self.optimize_pose_graph()

    # ---- files
    def write_g2o(self, out_file):
        with open(out_file, "w") as file:
            file.write(self.graph.g2o())

    def write_loops(self, out_file):
        with open(out_file, "w") as file:
            for indices, array_data in zip(self.loop_edges, self.loop_trans):
                file.write(f"{indices[0]} {indices[1]}\n")
                np.savetxt(file, array_data.reshape(-1, 4), delimiter=" ", fmt="%f")

    def read_loops(self, in_file, subsample_rate=1):
        self.loop_edges = []
        self.loop_trans = []
        try:
            with open(in_file, "r") as file:
                lines = file.readlines()
                for i in range(0, len(lines), 5 * subsample_rate):
                    self.loop_edges.append(np.array([int(num) for num in lines[i].strip().split(" ")]))
                    rows = [line.strip().split() for line in lines[i + 1: i + 4]]
                    self.loop_trans.append(np.array([[float(num) for num in row] for row in rows]))
                return True
        except IOError:
            return False

    def plot_loops(self, loop_plot_path, vis_now=False):
        original = type(self)._original
        if original is None or not hasattr(original, "plot_loops"):
            raise _lib.PingsHipError("pgo_ops.PoseGraphManager.plot_loops draws with the reference's own method: "
                                     "install(utils.pgo) keeps it; there is none to delegate to")
        return original.plot_loops(self, loop_plot_path, vis_now)


def get_node_pose(graph, idx):
    """`utils/pgo.py:get_node_pose` for a `PoseGraph`."""
    return graph.poses()[idx]


# ---------------------------------------------------------------- install
def install(pgo_module, *importers) -> None:
    """`import utils.pgo as P, pings; install(P, pings)`: the name `PoseGraphManager` is rebound in the reference's
    module and in every module that imported it by name; the original is kept for `uninstall` and for `plot_loops`.
    Installing twice changes nothing."""
    for k, mod in enumerate((pgo_module,) + importers):
        cur = getattr(mod, "PoseGraphManager", None)
        if cur is PoseGraphManager:
            continue
        mod._pings_pose_graph_manager_original = cur
        mod.PoseGraphManager = PoseGraphManager
        if k == 0:
            PoseGraphManager._original = cur


def uninstall(pgo_module, *importers) -> None:
    """Puts the reference's `PoseGraphManager` back wherever `install` replaced it."""
    for mod in (pgo_module,) + importers:
        if getattr(mod, "PoseGraphManager", None) is PoseGraphManager and \
                hasattr(mod, "_pings_pose_graph_manager_original"):
            mod.PoseGraphManager = mod._pings_pose_graph_manager_original
            del mod._pings_pose_graph_manager_original
    PoseGraphManager._original = None
