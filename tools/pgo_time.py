"""Time pose-graph optimisation on the device (`pings_amd.pgo_ops`, csrc/pgo.hip) against an fp64 host restatement of
the same Levenberg-Marquardt with `scipy.sparse.linalg.spsolve`, in the same process.

The graph is a synthetic loop trajectory: N poses on laps of a circle (1 m steps, 500 poses per lap), odometry with
accumulated noise, a fixed prior on node 0 and L exact loop factors between poses one or more laps apart, spread
evenly; sigmas 0.01 degree and 0.04 m as in the shipped configurations.  N = 1,000 / 5,000 / 20,000 with L = 10 / 100.

Per graph: wall time of `PoseGraph.optimize(pgo_max_iter = 50, rel_tol = 1e-5)` (host clock around a call that ends in
the trial's host read, after warm-up, median and min over --iters with the poses put back before every call), the
trials taken, host reads per trial (`_lib.sync_counts`), launches per trial (counted from the entry's C code, see
`launches`), the split of one optimisation into linearise / factor / sweeps / capacitance / step from the library's
HIP-event stage timer in a separate pass, and the same optimisation by `host_lm` (one run, wall time and trials).
Both sides start from the same poses and stop at a relative decrease of 1e-5, so their final costs must agree to
2e-5 relative, or the tool fails.

    python tools/pgo_time.py [--iters 5] [--warmup 1] [--sizes 1000,5000,20000] [--loops 10,100]
                             [--out profiles/pgo/pgo_time.json]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pings_amd import _lib, pgo_ops  # noqa: E402

SIGMAS = np.array([np.radians(0.01)] * 3 + [0.04] * 3)
LAP = 500
MAX_ITER, REL_TOL, LAMBDA0 = 50, 1e-5, 1e-5


def launches(n_loops: int, chunk: int) -> int:
    """Kernel launches of one trial (pings_pgo_iteration + the two polled reads of pings_pgo_read_record)."""
    cols = 1 + 6 * n_loops
    cw = min(cols, chunk)
    chunks = -(-cols // cw) if n_loops else 0
    return 3 + 1 + 4 * chunks + (1 if n_loops else 0) + 2 + 4 + 2


# ---------------------------------------------------------------- batched SE(3) in numpy (the contract of pgo_ops)
def skew(w):
    S = np.zeros(w.shape[:-1] + (3, 3))
    S[..., 0, 1], S[..., 0, 2], S[..., 1, 0] = -w[..., 2], w[..., 1], w[..., 2]
    S[..., 1, 2], S[..., 2, 0], S[..., 2, 1] = -w[..., 0], -w[..., 1], w[..., 0]
    return S


def coeffs(th):
    t2 = th * th
    small = th < 1e-2
    t = np.where(small, 1.0, th)
    s, c = np.sin(t), np.cos(t)
    q2 = t * t
    big = [s / t, (1 - c) / q2, (t - s) / (q2 * t), (q2 + 2 * c - 2) / (2 * q2 * q2),
           (2 * t - 3 * s + t * c) / (2 * q2 * q2 * t), 1 / q2 - (1 + c) / (2 * t * s)]
    ser = [1 - t2 / 6 + t2 * t2 / 120, 0.5 - t2 / 24 + t2 * t2 / 720, 1 / 6 - t2 / 120 + t2 * t2 / 5040,
           1 / 24 - t2 / 720 + t2 * t2 / 40320, 1 / 120 - t2 / 2520 + t2 * t2 / 120960,
           1 / 12 + t2 / 720 + t2 * t2 / 30240]
    return [np.where(small, a, b)[..., None, None] for a, b in zip(ser, big)]


def exp_se3(xi):
    w, v = xi[..., :3], xi[..., 3:]
    k = coeffs(np.linalg.norm(w, axis=-1))
    Wm = skew(w)
    W2 = Wm @ Wm
    T = np.zeros(xi.shape[:-1] + (4, 4))
    T[..., :3, :3] = np.eye(3) + k[0] * Wm + k[1] * W2
    T[..., :3, 3] = ((np.eye(3) + k[1] * Wm + k[2] * W2) @ v[..., None])[..., 0]
    T[..., 3, 3] = 1.0
    return T


def log_se3(T):
    Rm = T[..., :3, :3]
    s = 0.5 * np.stack([Rm[..., 2, 1] - Rm[..., 1, 2], Rm[..., 0, 2] - Rm[..., 2, 0], Rm[..., 1, 0] - Rm[..., 0, 1]], -1)
    sn = np.linalg.norm(s, axis=-1)
    th = np.arctan2(sn, 0.5 * (np.trace(Rm, axis1=-2, axis2=-1) - 1.0))
    kk = np.where(th < 1e-2, 1 + th * th / 6 + 7 * th ** 4 / 360, th / np.where(sn > 0, sn, 1.0))
    w = s * kk[..., None]
    Wm = skew(w)
    v = ((np.eye(3) - 0.5 * Wm + coeffs(th)[5] * (Wm @ Wm)) @ T[..., :3, 3, None])[..., 0]
    return np.concatenate([w, v], -1)


def inv_se3(T):
    out = np.zeros_like(T)
    Rt = np.swapaxes(T[..., :3, :3], -1, -2)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -(Rt @ T[..., :3, 3, None])[..., 0]
    out[..., 3, 3] = 1.0
    return out


def dlog(xi):
    k = coeffs(np.linalg.norm(xi[..., :3], axis=-1))
    Wm, V = skew(-xi[..., :3]), skew(-xi[..., 3:])
    A = np.eye(3) - 0.5 * Wm + k[5] * (Wm @ Wm)
    WV, VW = Wm @ V, V @ Wm
    WVW = WV @ Wm
    Q = 0.5 * V + k[2] * (WV + VW + WVW) + k[3] * (Wm @ WV + VW @ Wm - 3 * WVW) + k[4] * (WVW @ Wm + Wm @ WVW)
    J = np.zeros(xi.shape[:-1] + (6, 6))
    J[..., :3, :3] = A
    J[..., 3:, 3:] = A
    J[..., 3:, :3] = -A @ Q @ A
    return J


def adjoint(T):
    A = np.zeros(T.shape[:-2] + (6, 6))
    A[..., :3, :3] = T[..., :3, :3]
    A[..., 3:, 3:] = T[..., :3, :3]
    A[..., 3:, :3] = skew(T[..., :3, 3]) @ T[..., :3, :3]
    return A


# ---------------------------------------------------------------- the host restatement
def host_cost(X, fi, fj, Z, W):
    between = fj >= 0
    h = X[fi].copy()
    h[between] = inv_se3(X[fi[between]]) @ X[fj[between]]
    r = (W @ log_se3(inv_se3(Z) @ h)[..., None])[..., 0]
    return 0.5 * float(np.sum(r * r)), r, h


def host_lm(X, fi, fj, Z, W, max_iter=MAX_ITER, rel_tol=REL_TOL, lam=LAMBDA0):
    """The LM of pgo_ops on the host: batched numpy linearisation, a scipy CSC normal matrix, spsolve."""
    n = X.shape[0]
    between = fj >= 0
    bi, bj = fi[between], fj[between]
    trials = 0
    for _ in range(max_iter):
        trials += 1
        before, r, h = host_cost(X, fi, fj, Z, W)
        Jj = W @ dlog(log_se3(inv_se3(Z) @ h))
        Ji = Jj.copy()                                   # a prior's one Jacobian
        Ji[between] = -Jj[between] @ adjoint(inv_se3(h[between]))
        g = np.zeros((n, 6))
        np.add.at(g, fi, (np.swapaxes(Ji, -1, -2) @ r[..., None])[..., 0])
        np.add.at(g, bj, (np.swapaxes(Jj[between], -1, -2) @ r[between, :, None])[..., 0])
        JiT, JjT = np.swapaxes(Ji, -1, -2), np.swapaxes(Jj[between], -1, -2)
        blocks = np.concatenate([JiT @ Ji, JjT @ Jj[between], JjT @ Ji[between], JiT[between] @ Jj[between]])
        rows = np.concatenate([fi, bj, bj, bi])
        cols = np.concatenate([fi, bj, bi, bj])
        ri = (rows[:, None, None] * 6 + np.arange(6)[None, :, None]).repeat(6, 2).reshape(-1)
        ci = (cols[:, None, None] * 6 + np.arange(6)[None, None, :]).repeat(6, 1).reshape(-1)
        H = sp.coo_matrix((blocks.reshape(-1), (ri, ci)), shape=(6 * n, 6 * n)).tocsc()     # duplicates are summed
        d = H.diagonal()
        delta = spla.spsolve(H + sp.diags(lam * d, format="csc"), -g.reshape(-1)).reshape(n, 6)
        cand = X @ exp_se3(delta)
        after = host_cost(cand, fi, fj, Z, W)[0]
        if after <= before:
            X = cand
            lam /= 10.0
            if before - after <= rel_tol * before:
                break
        else:
            lam *= 10.0
            if lam > 1e5:
                break
    return X, host_cost(X, fi, fj, Z, W)[0], trials


# ---------------------------------------------------------------- the graph
def trajectory(n, n_loops, seed=0):
    rng = np.random.default_rng(seed)
    step = np.array([0.0, 0.0, 2 * np.pi / LAP, 1.0, 0.0, 0.0])
    steps = exp_se3(np.tile(step, (n - 1, 1)))
    noise = np.concatenate([rng.normal(0, 2e-4, (n - 1, 3)), rng.normal(0, 4e-3, (n - 1, 3))], -1)
    meas = steps @ exp_se3(noise)
    truth, odom = [np.eye(4)], [np.eye(4)]
    for k in range(n - 1):
        truth.append(truth[-1] @ steps[k])
        odom.append(odom[-1] @ meas[k])
    truth, odom = np.stack(truth), np.stack(odom)
    ends = np.linspace(LAP + 30, n - 1, n_loops).astype(np.int64)
    starts = ends - LAP * np.maximum(1, (ends // LAP) * (np.arange(n_loops) % 2))      # one lap back, or to the first lap
    fi = np.concatenate([[0], np.arange(n - 1), starts]).astype(np.int32)
    fj = np.concatenate([[-1], np.arange(1, n), ends]).astype(np.int32)
    Z = np.concatenate([np.eye(4)[None], meas, inv_se3(truth[starts]) @ truth[ends]])
    W = np.tile(np.diag(1.0 / SIGMAS), (fi.size, 1, 1))
    W[0] = np.diag([1.0 / pgo_ops.FIXED_SIGMA] * 6)
    return odom, fi, fj, Z, W


def stage_split(graph, X0):
    """ms per stage of one optimisation, from the library's HIP-event stage timer (its own pass: events slow the host)."""
    L = _lib.lib()
    graph.set_poses(X0)
    L.pings_prof_enable(1)
    graph.optimize(MAX_ITER, REL_TOL, LAMBDA0)
    buf = C.create_string_buffer(1 << 16)
    _lib.check(L.pings_prof_report(buf, len(buf)), "pings_prof_report")
    L.pings_prof_enable(0)
    out = {}
    for line in buf.value.decode().splitlines():
        name, count, ms = line.split()
        if name.startswith("pgo_"):
            out[name[4:]] = {"calls": int(count), "ms": round(float(ms), 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="1000,5000,20000")
    ap.add_argument("--loops", default="10,100")
    ap.add_argument("--chunk", type=int, default=128)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pgo_time: no HIP device; this tool measures on the device only")
    res = {"device": torch.cuda.get_device_name(0), "max_iter": MAX_ITER, "rel_tol": REL_TOL, "chunk": a.chunk,
           "graphs": []}
    for n in (int(s) for s in a.sizes.split(",")):
        for n_loops in (int(s) for s in a.loops.split(",")):
            X0, fi, fj, Z, W = trajectory(n, n_loops)
            g = pgo_ops.PoseGraph("cuda", chunk=a.chunk)
            for x in X0:
                g.add_node(x)
            g.add_prior(0, Z[0], W[0])
            for f in range(1, fi.size):
                g.add_between(int(fi[f]), int(fj[f]), Z[f], W[f])
            ts, reads, recs = [], 0, []
            for k in range(a.warmup + a.iters):
                g.set_poses(X0)
                g.error()                                # uploads the poses: not part of the optimisation
                torch.cuda.synchronize()
                _lib.sync_counts(reset=True)
                t0 = time.perf_counter()
                recs = g.optimize(MAX_ITER, REL_TOL, LAMBDA0)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if k >= a.warmup:
                    ts.append(dt)
                    reads += sum(_lib.sync_counts(reset=True).values())
            final = g.error()
            t0 = time.perf_counter()
            _, host_final, host_trials = host_lm(X0, fi, fj, Z, W)
            host_s = time.perf_counter() - t0
            entry = {"nodes": n, "loops": n_loops, "trials": len(recs),
                     "cost_before": recs[0].cost_before, "cost_after": final,
                     "device_ms_median": round(1e3 * statistics.median(ts), 3), "device_ms_min": round(1e3 * min(ts), 3),
                     "device_ms_per_trial": round(1e3 * statistics.median(ts) / len(recs), 3),
                     "host_reads_per_trial": reads / (a.iters * len(recs)),
                     "launches_per_trial": launches(n_loops, a.chunk),
                     "stages_ms": stage_split(g, X0),
                     "host_spsolve_ms": round(1e3 * host_s, 1), "host_trials": host_trials, "host_cost_after": host_final}
            print(json.dumps(entry), flush=True)
            if not abs(final - host_final) <= 2e-5 * max(host_final, 1e-30):
                raise SystemExit(f"pgo_time: device cost {final!r} and host cost {host_final!r} disagree")
            res["graphs"].append(entry)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
