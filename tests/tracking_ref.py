"""Restatement of the geometric branch of the odometry loop (utils/tracker.py:43-210 `Tracker.tracking` and :353-605
`registration_step` without the photometric and colour-consistency terms) for the tests of
`pings_amd.tracker_ops.tracking`, written against two injected callables so that it runs anywhere:

    query(points) -> (sdf[n], grad[n,3], mask[n] bool, std[n])     the SDF head of query_source_points
    solve(points, grad, residual, weight[n,1], lm_lambda) -> dT      implicit_reg's step (fp64 4x4)

On the CPU (`cpu_query` / `cpu_solve`: oracle/sdf_cpu + oracle/tracker_cpu in float64) it is pinned to the
reference's own runs by tests/golden/tracking_*.npz (tools/make_tracking_golden.py); on the device, with the HIP
`query_source_points` / `implicit_reg` drop-ins, it is the loop as it stood before the device-resident one
(tools/tracking_time.py).  Every host decision is kept, so it waits on the host as often as the reference."""
import math

import torch

from oracle import sdf_cpu, tracker_cpu


def cpu_query(npm, dec, bs, nn_k):
    def q(points):
        outs = [tracker_cpu.query_source_points(npm, dec, points[h:h + bs], mask_min_nn_count=nn_k)
                for h in range(0, points.shape[0], bs)]
        s, g, m, _, std = (torch.cat(t) for t in zip(*outs))
        return s, g, m, std
    return q


def cpu_solve(points, grad, res, w, lm_lambda):
    return tracker_cpu.implicit_reg(points, grad, res, w, lm_lambda)[0]


def cpu_map(st):
    """The fixture's map in float64 on the oracle (map and decoder)."""
    npm = sdf_cpu.NeuralPointMap(st)
    for k, v in list(vars(npm).items()):
        if torch.is_tensor(v) and v.dtype == torch.float32:
            setattr(npm, k, v.double())
    npm.dtype = torch.float64
    p = [torch.as_tensor(st["dec." + k]).double() for k in ("layers.0.weight", "layers.0.bias", "lout.weight",
                                                               "lout.bias")]
    return npm, sdf_cpu.MLP(*p, float(st["sdf_scale"]))


def step(query, solve, cfg, points, normals, labels, GM_dist, GM_grad, lm_lambda):
    """One registration step: (dT, valid count, residual mean in cm, valid mask)."""
    sdf, grad, mask, std = query(points)
    gnorm = grad.norm(dim=-1)
    max_std = cfg.surface_sample_range_m * cfg.max_sdf_std_ratio
    valid = mask & (gnorm < cfg.reg_max_grad_norm) & (gnorm > cfg.reg_min_grad_norm) & (std < max_std)
    p = points[valid]
    n = p.shape[0]
    if n < 10:
        return torch.eye(4, dtype=torch.float64, device=points.device), n, 0.0, valid
    g, gn, s, lab = grad[valid], gnorm[valid], sdf[valid], labels[valid]
    if cfg.reg_dist_div_grad_norm:
        s = s / gn
    r = s - lab
    res_cm = float(r.abs().mean()) * 100.0
    w = torch.ones_like(r)
    weighted = False
    if GM_dist is not None:
        w = w * (GM_dist / (GM_dist + r * r)) ** 2
        weighted = True
    if GM_grad is not None:
        w = w * (GM_grad / (GM_grad + (gn - 1.0) ** 2)) ** 2
        weighted = True
    if normals is not None:
        unit = g / (gn.unsqueeze(-1) + 1e-7)
        w = w * (0.5 + (normals[valid] * unit).sum(dim=1).abs())
        weighted = True
    if weighted:                   # the reference normalises only when some weight made w a tensor
        w = w / (2.0 * w.mean())
    return solve(p, g, r, w.unsqueeze(1), lm_lambda), n, res_cm, valid


def transform(points, T):
    return points @ T[:3, :3].to(points.dtype).T + T[:3, 3].to(points.dtype)


def tracking(query, solve, cfg, source_points, init_pose, normals=None, labels=None):
    """The loop with its decisions: returns (T, valid_flag, trace) with trace = [(dT, count, residual_cm), ...]."""
    T = torch.eye(4, dtype=torch.float64, device=source_points.device) if init_pose is None else init_pose
    GM_dist = cfg.reg_GM_dist_m if cfg.reg_GM_dist_m > 0 else None
    GM_grad = cfg.reg_GM_grad if cfg.reg_GM_grad > 0 else None
    N = source_points.shape[0]
    if labels is None:
        labels = torch.zeros(N, dtype=source_points.dtype, device=source_points.device)
    converged, valid_flag, last = False, True, 1e5
    trace = []
    i = -1
    for i in range(cfg.reg_iter_n):
        dT, count, res, _ = step(query, solve, cfg, transform(source_points, T), normals, labels, GM_dist, GM_grad,
                                 cfg.reg_lm_lambda)
        trace.append((dT, count, res))
        T = dT @ T
        if (res - last) / last > 1.1:
            valid_flag = False
        else:
            last = res
        if count < 10 or count / N < 0.05:
            valid_flag = False
        if not valid_flag or converged:
            break
        c = (float(torch.trace(dT[:3, :3])) - 1.0) / 2.0
        rot = math.degrees(math.acos(c)) if -1.0 <= c <= 1.0 else float("nan")   # torch.acos: NaN outside
        tran = float(dT[:3, 3].norm())
        if abs(rot) < cfg.reg_term_thre_deg and tran < cfg.reg_term_thre_m or i == cfg.reg_iter_n - 2:
            converged = True
    if trace and trace[-1][2] > cfg.surface_sample_range_m * 60.0:
        valid_flag = False
    if not valid_flag and i < 10:
        T = init_pose
    return T, valid_flag, trace
