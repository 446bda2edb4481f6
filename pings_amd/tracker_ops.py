"""Tracker registration step on the HIP device.

`query_source_points` — drop-in for `Tracker.query_source_points` (utils/tracker.py:212-351): SDF value, analytic SDF
gradient, spread of the per-neighbour predictions, marching-cubes / registration mask and certainty of every source
point come from ONE fused kernel launch per batch (`pings_sdf_forward`: hash-grid kNN + feature gather + decoder +
IDW + d/dx), where the reference runs query_feature, the decoder, an autograd backward through all of it and a
dozen element-wise kernels, 50-100 times per frame.  Colour and semantic queries without a gradient run HIP
`query_feature`, the head's decoder on the fused kernels and `pings_head_reduce`; the colour with its Jacobian for the
photometric term (`query_color_grad`) is `pings_color_forward` on the neighbour rows the SDF launch emitted (one more
launch; colour decoders it does not cover keep the reference's torch tail behind the HIP `query_feature`).

`implicit_reg` — drop-in for the module-level function (utils/tracker.py:608-689): the 6x6 normal equations come from
`pings_reg_normal_equations` (one pass, fp64 accumulation, fixed-order reduction); LM damping, the fp64 6x6 solve and
the exponential map run in `pings_reg_solve` (one single-thread kernel, the reference's formulas).

`tracking` — drop-in for `Tracker.tracking` (utils/tracker.py:43-210): the odometry loop with the pose in device
memory.  Each iteration runs `pings_reg_transform`, the fused query, `pings_reg_assemble` (validity, residual, weights
and the normal equations in one pass, nothing compacted) and `pings_reg_step` (solve, pose update, convergence
quantities), then reads ONE 8-word record back; the reference's decision logic runs on those host numbers.
`registration_step` — drop-in for `Tracker.registration_step` (:353-605) on the same two kernels; it keeps the
reference's host reads (compacted `valid_points`, the residual as a float).

`install(tracker_module)` rebinds `query_source_points` and `implicit_reg`; `install(tracker_module, loop=True)` also
rebinds `Tracker.tracking` and `Tracker.registration_step`, keeping the originals for what the loop delegates (the
photometric and colour-consistency configurations, and the Open3D weight cloud of a `vis_result` run).
`install(tracker_module, loop=True, colour=True)` runs those two colour configurations in the device loop as well:
SDF forward with the neighbour rows out, `pings_color_forward` on them, `pings_reg_assemble_color`, the unchanged
`pings_reg_step`, one record read.  Host tensors raise: there is no CPU path (oracle/tracker_cpu.py is the CPU
restatement used by the tests).
"""
from __future__ import annotations

import ctypes as C
import math
import struct

import torch

from . import _abi, _lib
from . import neural_points as _np
from ._abi import REG_ILL_CONDITIONED, REG_NONFINITE, REG_SINGULAR     # re-exported: the solve's status bits

_REG_CHECK = __import__("os").environ.get("PINGS_REG_CHECK", "1") != "0"
last_solve_status = None    # int32[1] device tensor of the most recent `implicit_reg` (REG_* bit mask)
# float64 [iterations, 24] device tensor of the most recent `tracking` call, one row per executed iteration: valid
# count, residual (cm), rotation (deg), translation (m), status bits, sum w, sum w r^2, 0, then dT row-major (16)
last_trace = None
_ORIG = {}                  # the reference's Tracker.tracking / registration_step, kept by install(loop=True)
_COLOUR = False             # install(loop=True, colour=True): the colour configurations run in the device loop
TRACE_ROW = 24


def normal_equations(points, sdf_grad, sdf_residual, weight):
    """N[6,6] = J^T (w J), g[6] = -(J w)^T r with J = [points x sdf_grad, sdf_grad] (fp32 tensors on the device)."""
    if not points.is_cuda:
        raise _lib.PingsHipError("implicit_reg runs on the HIP device only (got a CPU tensor); there is no CPU fallback")
    L = _lib.lib()
    f = lambda t: t.detach().to(torch.float32).contiguous()
    p, g = f(points), f(sdf_grad)
    r, w = f(sdf_residual).reshape(-1), f(weight).reshape(-1)
    n = p.shape[0]
    dev = p.device
    out = torch.empty(42, dtype=torch.float32, device=dev)
    scratch = torch.empty(L.pings_reg_normal_equations_scratch_bytes(), dtype=torch.uint8, device=dev)
    _lib.check(L.pings_reg_normal_equations(_lib.ptr(p), _lib.ptr(g), _lib.ptr(r), _lib.ptr(w), n, _lib.ptr(scratch),
                                            _lib.ptr(out), _lib.stream_ptr(dev)), "pings_reg_normal_equations")
    return out[:36].view(6, 6), out[36:]


def implicit_reg(points, sdf_grad, sdf_residual, weight, lm_lambda=0.0, require_cov=False, require_eigen=False):
    """One LM step of point-to-implicit-model registration (utils/tracker.py:608-689): returns
    (T_mat[4,4] fp64, cov_mat[6,6] | None, eigenvalues[3] | None)."""
    N_mat, g_vec = normal_equations(points, sdf_grad, sdf_residual, weight)
    N_mat_raw = N_mat
    # damping, fp64 solve and exponential map in one kernel (`pings_reg_solve`; N_mat / g_vec are views of one buffer)
    L = _lib.lib()
    T_mat = torch.empty(4, 4, dtype=torch.float64, device=points.device)
    # The reference's `torch.linalg.inv` (utils/tracker.py:668) synchronises to read LAPACK's info word and raises
    # LinAlgError on a singular N.  The kernel leaves a status word; it is read back here with one polled wait (the
    # tracker compares the step against its thresholds on the host a few lines later anyway, :165-172), so a
    # degenerate registration surfaces where the reference's does instead of as NaN poses.  PINGS_REG_CHECK=0 skips
    # the wait (status stays on the device in `last_solve_status`).
    status_dev = torch.empty(1, dtype=torch.int32, device=points.device)
    host = C.c_int32(0)
    checked = _REG_CHECK
    _lib.check(L.pings_reg_solve_checked(N_mat.data_ptr(), float(lm_lambda), T_mat.data_ptr(), None,
                                         status_dev.data_ptr(), C.byref(host) if checked else None,
                                         _lib.stream_ptr(points.device)), "pings_reg_solve_checked")
    global last_solve_status
    last_solve_status = status_dev
    if checked:
        _lib.note_sync("reg_solve_status")
        st = int(host.value)
        if st & REG_SINGULAR:
            raise torch.linalg.LinAlgError(
                "implicit_reg: the damped normal matrix is singular (a pivot is exactly zero or not finite); "
                "the reference's torch.linalg.inv raises here as well (utils/tracker.py:668)")
        if st & (REG_ILL_CONDITIONED | REG_NONFINITE):
            import warnings

            warnings.warn("implicit_reg: " + ("non-finite registration step" if st & REG_NONFINITE else
                          "normal matrix ill-conditioned (smallest pivot < 1e-7 of its largest entry)") +
                          "; the step is returned as computed, as the reference's inverse would be", RuntimeWarning)
    eigenvalues = None
    if require_eigen:
        eigenvalues = torch.linalg.eigvals(N_mat_raw[3:, 3:]).real
    cov_mat = None
    if require_cov:
        w = weight.reshape(-1)
        mse = torch.mean(w * sdf_residual.reshape(-1) ** 2)
        cov_mat = torch.linalg.inv(N_mat_raw) * mse
    return T_mat, cov_mat, eigenvalues


def query_source_points(self, coord, bs, query_sdf=True, query_sdf_grad=True, query_color=False,
                        query_color_grad=False, query_sem=False, query_mask=True, query_certainty=True,
                        query_locally=True, mask_min_nn_count: int = 4):
    """`Tracker.query_source_points` (utils/tracker.py:212-351): same arguments, same 8-tuple
    (sdf_pred, sdf_grad, color_pred, color_grad, sem_pred, mc_mask, certainty, sdf_std)."""
    if not coord.is_cuda:
        raise _lib.PingsHipError("query_source_points runs on the HIP device only; there is no CPU fallback")
    n = coord.shape[0]
    dev = coord.device
    iters = math.ceil(n / bs) if n else 0
    single = iters == 1
    sdf_pred = torch.zeros(n, device=dev) if query_sdf and not single else None
    sdf_std = torch.zeros(n, device=dev) if query_sdf and not single else None
    sdf_grad = torch.zeros(n, 3, device=dev) if query_sdf_grad and not single else None
    mc_mask = torch.zeros(n, device=dev, dtype=torch.bool) if query_mask and not single else None
    certainty = torch.zeros(n, device=dev) if query_certainty and not single else None
    channels = getattr(self.config, "color_channel", 3)
    color_pred = torch.zeros(n, channels, device=dev) if query_color else None
    color_grad = torch.zeros(n, channels, 3, device=dev) if query_color_grad else None
    sem_pred = torch.zeros(n, device=dev) if query_sem else None
    npm = self.neural_points
    # the photometric term: the fused colour kernel on the neighbour rows of the SDF launch, when it covers the decoder
    colour_native = bool(query_color and query_color_grad) and _np.colour_fused_supported(npm, self.color_mlp)
    for k in range(iters):
        head, tail = k * bs, min((k + 1) * bs, n)
        x = coord[head:tail]
        idx = None
        if query_sdf or query_mask or query_certainty:
            s, g, cnt, cert, std, *rest = _np.sdf_fused(npm, self.sdf_mlp, x, need_grad=bool(query_sdf_grad),
                                                        need_certainty=bool(query_certainty),
                                                        query_locally=query_locally, use_only_valid_points=True,
                                                        need_std=True, want_idx=colour_native)
            idx = rest[0] if rest else None
            if iters == 1:   # the usual case (bs >= n): hand the kernel's outputs over, no zero fills, no slice copies
                if query_sdf:
                    sdf_pred, sdf_std = s, std
                if query_sdf_grad:
                    sdf_grad = g
                if query_mask:
                    mc_mask = cnt >= mask_min_nn_count
                if query_certainty:
                    certainty = cert
            else:
                if query_sdf:
                    sdf_pred[head:tail] = s
                    sdf_std[head:tail] = std
                if query_sdf_grad:
                    sdf_grad[head:tail] = g
                if query_mask:
                    mc_mask[head:tail] = cnt >= mask_min_nn_count
                if query_certainty:
                    certainty[head:tail] = cert
        if query_sem or (query_color and not query_color_grad):
            # heads without a gradient w.r.t. the query (:322-331): HIP query_feature, the head's decoder on the fused
            # MFMA kernels and one activation + IDW-sum (+ arg-max) pass (csrc/heads.hip), as in the mesher
            from . import decoder as _dec
            from .mesher_ops import head_reduce

            with torch.no_grad():
                gf, cf, w_knn, _, _ = npm.query_feature(x.detach(), accumulate_stability=False, query_locally=query_locally,
                                                        query_geo_feature=bool(query_sem),
                                                        query_color_feature=bool(query_color and not query_color_grad),
                                                        use_only_valid_points=True)
                wk = None if self.config.weighted_first else w_knn
                if query_sem:
                    sem_pred[head:tail] = head_reduce(_dec.mlp(self.sem_mlp, gf), wk,
                                                      _abi.HEAD_SEMANTIC).to(sem_pred.dtype)
                if query_color and not query_color_grad:
                    color_pred[head:tail] = head_reduce(_dec.mlp(self.color_mlp, cf), wk, _abi.HEAD_COLOR)
        if colour_native:
            if idx is None:
                idx = _np.radius_neighborhood_topk(npm, x, bool(npm.temporal_local_map_on and query_locally), True, True,
                                                   query_locally)[0]
            col, jac = _np.color_fused(npm, self.color_mlp, x, idx, need_jac=True, query_locally=query_locally)
            color_pred[head:tail] = col
            color_grad[head:tail] = jac
        elif query_color and query_color_grad:   # decoders the kernel does not cover: HIP query_feature + the reference's torch tail
            xc = x.detach().clone().requires_grad_(bool(query_color_grad))
            _, color_feature, w_knn, _, _ = npm.query_feature(xc, accumulate_stability=False, query_locally=query_locally,
                                                              query_color_feature=True, use_only_valid_points=True)
            col = self.color_mlp.regress_color(color_feature)
            if not self.config.weighted_first:
                col = torch.sum(col * w_knn, dim=1)
            if query_color_grad:
                for i in range(channels):
                    (gi,) = torch.autograd.grad(col[:, i].sum(), xc, retain_graph=True)
                    color_grad[head:tail, i, :] = gi.detach()
            color_pred[head:tail] = col.detach()
    return sdf_pred, sdf_grad, color_pred, color_grad, sem_pred, mc_mask, certainty, sdf_std


# ---------------------------------------------------------------- device-resident odometry loop
def _loop_lib():
    L = _lib.lib()
    if not hasattr(L, "pings_reg_step"):
        raise _lib.PingsHipError(f"{_lib.LIB_PATH} has no pings_reg_step: rebuild it with `python -m pings_amd.build`")
    return L


class _Loop:
    """Buffers and argument block of one `tracking` / `registration_step` call (caller-owned scratch of the kernels)."""

    def __init__(self, self_, points, labels, normals, min_grad, max_grad, GM_dist, GM_grad, lm_lambda, weighted,
                 pose, trace_rows=0, valid_out=False, colours=None, colour_mode=0):
        if not points.is_cuda:
            raise _lib.PingsHipError("tracking runs on the HIP device only (got a CPU tensor); there is no CPU fallback")
        cfg = self_.config
        self.L = L = _loop_lib()
        dev = points.device
        self.dev, self.n = dev, int(points.shape[0])
        f = lambda t: t.detach().to(dev, torch.float32).contiguous()
        self.src = f(points)
        self.cur = torch.empty_like(self.src)
        self.label = f(labels).reshape(-1)
        self.normals = f(normals) if normals is not None else None
        self.part = torch.empty(int(L.pings_reg_partials(self.n)) * 32, dtype=torch.float64, device=dev)
        self.T = pose
        self.delta = torch.empty(4, 4, dtype=torch.float64, device=dev)
        self.record = torch.empty(8, dtype=torch.int32, device=dev)
        self.trace = torch.zeros(max(trace_rows, 1), TRACE_ROW, dtype=torch.float64, device=dev) if trace_rows else None
        self.valid = torch.empty(self.n, dtype=torch.bool, device=dev) if valid_out else None
        self.host = (C.c_int32 * 8)()
        flags = (_abi.REG_F_NORMALS if normals is not None else 0) | \
                (_abi.REG_F_DIV_GRAD if cfg.reg_dist_div_grad_norm else 0) | (_abi.REG_F_WEIGHTED if weighted else 0)
        max_std = cfg.surface_sample_range_m * cfg.max_sdf_std_ratio
        a = _abi.RegLoopArgs(self.n, flags, 0, trace_rows, float(min_grad), float(max_grad), float(max_std),
                             float(GM_dist) if GM_dist is not None else 0.0,
                             float(GM_grad) if GM_grad is not None else 0.0, float(lm_lambda))
        a.src, a.cur, a.label, a.normals = self.src.data_ptr(), self.cur.data_ptr(), self.label.data_ptr(), \
            _lib.ptr(self.normals)
        a.valid = _lib.ptr(self.valid)
        a.part, a.T, a.delta, a.record = (t.data_ptr() for t in (self.part, self.T, self.delta, self.record))
        a.trace = _lib.ptr(self.trace)
        self.args = a
        self.stream = _lib.stream_ptr(dev)
        self.bs = int(cfg.infer_bs)
        self.nn_k = int(getattr(cfg, "track_mask_query_nn_k", getattr(cfg, "query_nn_k", 4)))
        self.colour = None
        if colour_mode:
            ch = int(cfg.color_channel)
            self.src_colour = colours.detach().to(dev, torch.float32)[:, :ch].contiguous()
            self.photo_part = torch.zeros(int(L.pings_reg_partials(self.n)), dtype=torch.float64, device=dev)
            self.colour = _abi.RegColorArgs(self.src_colour.data_ptr(), None, None, ch, int(colour_mode),
                                            float(getattr(cfg, "photometric_loss_weight", 0.0)),
                                            self.photo_part.data_ptr())

    def transform(self):
        _lib.check(self.L.pings_reg_transform(C.byref(self.args), self.stream), "pings_reg_transform")
        return self.cur

    def iterate(self, self_, it, sync_tag):
        """query, assemble, step and the one host read; returns (valid count, status, residual cm, rot deg, tran m)."""
        a = self.args
        if self.colour is None:
            # the colour query is skipped: no weight uses it in the configurations that reach this path
            sdf, grad, _, _, _, mask, _, std = query_source_points(self_, self.cur, self.bs, True, True, False, False,
                                                                    query_certainty=False, query_locally=True,
                                                                    mask_min_nn_count=self.nn_k)
            keep = [t.contiguous() for t in (sdf, grad, std, mask)]
        else:
            keep = [None if t is None else t.contiguous() for t in self._query_colour(self_)]
            c = self.colour
            c.color_pred, c.color_jac = keep[4].data_ptr(), _lib.ptr(keep[5])
        a.sdf, a.grad, a.std = (t.data_ptr() for t in keep[:3])
        a.mask = keep[3].view(torch.uint8).data_ptr()
        a.iter = it
        if self.colour is None:
            _lib.check(self.L.pings_reg_assemble(C.byref(a), self.stream), "pings_reg_assemble")
        else:
            _lib.check(self.L.pings_reg_assemble_color(C.byref(a), C.byref(self.colour), self.stream),
                       "pings_reg_assemble_color")
        _lib.check(self.L.pings_reg_step(C.byref(a), self.stream), "pings_reg_step")
        _lib.check(self.L.pings_reg_read_record(self.record.data_ptr(), C.addressof(self.host), self.stream),
                   "pings_reg_read_record")
        _lib.note_sync(sync_tag)
        del keep
        h = self.host
        raw = bytes(h)
        res, rot, tran = struct.unpack("<3d", raw[8:32])
        return int(h[0]), int(h[1]), res, rot, tran

    def _query_colour(self, self_):
        """(sdf, grad, std, mask, colour, jac | None) of the current points: per batch the SDF forward with its neighbour
        rows out, then the colour forward on those rows (with the Jacobian for the photometric term only)."""
        npm, jac_on = self_.neural_points, self.colour.mode == _abi.REG_COLOR_PHOTO
        outs = []
        for head in range(0, self.n, self.bs):
            x = self.cur[head:head + self.bs]
            s, g, cnt, _, std, idx = _np.sdf_fused(npm, self_.sdf_mlp, x, need_grad=True, need_certainty=False,
                                                   query_locally=True, use_only_valid_points=True, need_std=True,
                                                   want_idx=True)
            col, jac = _np.color_fused(npm, self_.color_mlp, x, idx, need_jac=jac_on, query_locally=True)
            outs.append((s, g, std, cnt >= self.nn_k, col, jac))
        if len(outs) == 1:
            return [t for t in outs[0] if t is not None] + ([None] if not jac_on else [])
        cols = list(zip(*outs))
        return [torch.cat(c) for c in cols[:5]] + [torch.cat(cols[5]) if jac_on else None]

    def photo_residual(self, count):
        """mean |I_pred - I_src| over the valid points of the last assemble (one host read)."""
        _lib.note_sync("registration_step_photo")
        return float(self.photo_part.sum().item()) / count


def _check_status(status, warned):
    if status & REG_SINGULAR:
        raise torch.linalg.LinAlgError(
            "tracking: the damped normal matrix is singular (a pivot is exactly zero or not finite); the reference's "
            "torch.linalg.inv raises here as well (utils/tracker.py:668)")
    if status & (REG_ILL_CONDITIONED | REG_NONFINITE) and not warned:
        import warnings

        warnings.warn("tracking: " + ("non-finite registration step" if status & REG_NONFINITE else
                      "normal matrix ill-conditioned (smallest pivot < 1e-7 of its largest entry)") +
                      "; the step is applied as computed, as the reference's inverse would be (warned once per call)",
                      RuntimeWarning, stacklevel=3)
        return True
    return warned


def _say(self, msg):
    if not self.silence:
        print(msg)


def _original(name):
    f = _ORIG.get(name)
    if f is None:
        raise NotImplementedError(f"tracker_ops: this configuration runs the reference's own `Tracker.{name}`; "
                                  "bind the loop with install(tracker_module, loop=True) so that it is kept")
    return f


def _colour_branch(cfg, colors):
    """The reference's colour-using branches (photometric term, consistency weight): delegated to the saved originals
    unless install(..., loop=True, colour=True) put them into the device loop (`_colour_mode`)."""
    colors_on = colors is not None and cfg.color_on
    return colors_on and (cfg.photometric_loss_on or cfg.consist_wieght_on)


def _colour_mode(self, cfg, points, colors):
    """The colour configuration in the device loop (install(..., colour=True)): PINGS_REG_COLOR_* of the reference's
    branch, or 0 when the call goes to the saved original (option off, or a colour decoder / channel count the
    kernels do not cover).  Host tensors raise."""
    if not _COLOUR:
        return 0
    if not points.is_cuda or not colors.is_cuda:
        raise _lib.PingsHipError("tracking with colours runs on the HIP device only (got a CPU tensor); there is no "
                                 "CPU fallback")
    if int(cfg.color_channel) not in (1, 3) or colors.shape[1] < int(cfg.color_channel) or \
            not _np.colour_fused_supported(self.neural_points, getattr(self, "color_mlp", None)):
        return 0
    # an `elif` in the reference: the consistency weight is ignored when the photometric term is on
    return _abi.REG_COLOR_PHOTO if cfg.photometric_loss_on else _abi.REG_COLOR_CONSIST


def tracking(self, source_points, init_pose=None, source_colors=None, source_normals=None, source_semantics=None,
             source_sdf=None, cur_ts=None, loop_reg: bool = False, vis_result: bool = False):
    """`Tracker.tracking` (utils/tracker.py:43-210): same arguments, same (T, cov_mat, weight_pc, valid_flag).  One
    host read per iteration (`note_sync("tracking_iteration")`); the records of the call are left in `last_trace`."""
    global last_trace
    cfg = self.config
    colour_mode = 0
    if _colour_branch(cfg, source_colors):
        colour_mode = _colour_mode(self, cfg, source_points, source_colors)
        if not colour_mode:
            return _original("tracking")(self, source_points, init_pose, source_colors, source_normals,
                                         source_semantics, source_sdf, cur_ts, loop_reg, vis_result)
    if not source_points.is_cuda:
        raise _lib.PingsHipError("tracking runs on the HIP device only (got a CPU tensor); there is no CPU fallback")
    dev = source_points.device
    pose = torch.eye(4, dtype=torch.float64, device=dev) if init_pose is None else \
        init_pose.detach().to(dev, torch.float64).clone().contiguous()
    min_grad_norm, max_grad_norm = cfg.reg_min_grad_norm, cfg.reg_max_grad_norm
    cur_GM_dist_m = cfg.reg_GM_dist_m if cfg.reg_GM_dist_m > 0 else None
    cur_GM_grad = cfg.reg_GM_grad if cfg.reg_GM_grad > 0 else None
    lm_lambda, iter_n = cfg.reg_lm_lambda, cfg.reg_iter_n
    term_thre_deg, term_thre_m = cfg.reg_term_thre_deg, cfg.reg_term_thre_m
    max_valid_final_sdf_residual_cm = cfg.surface_sample_range_m * 0.6 * 100.0
    min_valid_ratio, max_increment_sdf_residual_ratio = 0.05, 1.1
    eigenvalue_ratio_thre, min_valid_points = 0.005, 10
    converged, valid_flag, last_sdf_residual_cm = False, True, 1e5
    cov_mat = eigenvalues = weight_point_cloud = None
    source_point_count = source_points.shape[0]
    _say(self, f"# Source point for registeration : {source_point_count}")
    if source_sdf is None:
        source_sdf = torch.zeros(source_point_count, device=dev)
    # (with a colour term the reference's w is a tensor whatever else is on)
    weighted = cur_GM_dist_m is not None or cur_GM_grad is not None or source_normals is not None or bool(colour_mode)
    lp = _Loop(self, source_points, source_sdf, source_normals, min_grad_norm, max_grad_norm, cur_GM_dist_m,
               cur_GM_grad, lm_lambda, weighted, pose, trace_rows=max(int(iter_n), 1), colours=source_colors,
               colour_mode=colour_mode)
    warned = False
    i = -1
    for i in range(iter_n):
        cur_points = lp.transform()
        if vis_result and converged:
            # the Open3D weight cloud, covariance and eigenvalues: the reference's own registration_step on the current
            # points (its query and implicit_reg are this module's after install); its dT goes back into the pose
            (delta_T, cov_mat, eigenvalues, weight_point_cloud, valid_points_torch, sdf_residual_cm,
             _photo) = _original("registration_step")(self, cur_points, source_normals, source_sdf, source_colors,
                                                      min_grad_norm, max_grad_norm, cur_GM_dist_m, cur_GM_grad,
                                                      lm_lambda, True)
            delta_T = delta_T.to(dev, torch.float64)
            pose.copy_(delta_T @ pose)
            valid_point_count = valid_points_torch.shape[0]
            lp.trace[i, 0], lp.trace[i, 1] = float(valid_point_count), float(sdf_residual_cm)
            lp.trace[i, 8:] = delta_T.reshape(16)
        else:
            valid_point_count, status, sdf_residual_cm, rot_deg, tran_m = lp.iterate(self, i, "tracking_iteration")
            warned = _check_status(status, warned)
            cov_mat = eigenvalues = weight_point_cloud = None
        if (sdf_residual_cm - last_sdf_residual_cm) / last_sdf_residual_cm > max_increment_sdf_residual_ratio:
            _say(self, "(Warning) registration failed: wrong optimization")
            valid_flag = False
        else:
            last_sdf_residual_cm = sdf_residual_cm
        if (valid_point_count < min_valid_points) or (1.0 * valid_point_count / source_point_count < min_valid_ratio):
            _say(self, "(Warning) registration failed: not enough valid points")
            valid_flag = False
        if not valid_flag or converged:
            break
        # rot_deg is NaN when (tr dT - 1) / 2 > 1: the comparison is False and the loop goes on, as the reference's
        if abs(rot_deg) < term_thre_deg and tran_m < term_thre_m or i == iter_n - 2:
            converged = True
    last_trace = lp.trace[: i + 1]
    _say(self, f"# Valid source point             : {valid_point_count}")
    _say(self, f"Odometry residual (cm): {sdf_residual_cm}")
    if sdf_residual_cm > max_valid_final_sdf_residual_cm:
        _say(self, "(Warning) registration failed: too large final residual")
        valid_flag = False
    if eigenvalues is not None:
        min_eigenvalue = torch.min(eigenvalues).item()
        if cfg.eigenvalue_check and min_eigenvalue < valid_point_count * eigenvalue_ratio_thre:
            _say(self, "(Warning) registration failed: eigenvalue check failed")
            valid_flag = False
    if cov_mat is not None:
        cov_mat = cov_mat.detach().cpu().numpy()
    T = pose
    if not valid_flag and i < 10:   # not valid within 10 iterations: the initial guess (None when none was given)
        T = init_pose
        cov_mat = None
    return T, cov_mat, weight_point_cloud, valid_flag


def registration_step(self, points: torch.Tensor, normals: torch.Tensor, sdf_labels: torch.Tensor,
                      colors: torch.Tensor, min_grad_norm, max_grad_norm, GM_dist=None, GM_grad=None, lm_lambda=0.0,
                      vis_weight_pc=False):
    """`Tracker.registration_step` (utils/tracker.py:353-605) on the loop's kernels (identity pose): returns the
    reference's (T, cov_mat, eigenvalues, weight_point_cloud, valid_points, sdf_residual_cm, photo_residual).  Keeps
    the reference's host reads (compacted valid_points, the residual as a float); `tracking` does not call it."""
    cfg = self.config
    colour_mode = 0
    if not vis_weight_pc and _colour_branch(cfg, colors):
        colour_mode = _colour_mode(self, cfg, points, colors)
    if vis_weight_pc or (_colour_branch(cfg, colors) and not colour_mode):
        return _original("registration_step")(self, points, normals, sdf_labels, colors, min_grad_norm, max_grad_norm,
                                              GM_dist, GM_grad, lm_lambda, vis_weight_pc)
    if not points.is_cuda:
        raise _lib.PingsHipError("registration_step runs on the HIP device only (got a CPU tensor); there is no CPU "
                                 "fallback")
    dev = points.device
    pose = torch.eye(4, dtype=torch.float64, device=dev)
    weighted = GM_dist is not None or GM_grad is not None or normals is not None or bool(colour_mode)
    lp = _Loop(self, points, sdf_labels, normals, min_grad_norm, max_grad_norm, GM_dist, GM_grad, lm_lambda, weighted,
               pose, valid_out=True, colours=colors, colour_mode=colour_mode)
    lp.cur.copy_(lp.src)     # the points arrive transformed already
    count, status, res_cm, _, _ = lp.iterate(self, 0, "registration_step")
    valid_points = points[lp.valid]
    if count < 10:
        return lp.delta, None, None, None, valid_points, 0.0, 0.0
    _check_status(status, False)
    photo = lp.photo_residual(count) if colour_mode == _abi.REG_COLOR_PHOTO else None
    return lp.delta, None, None, None, valid_points, res_cm, photo


def install(tracker_module, loop: bool = False, colour: bool = False) -> None:
    """`import utils.tracker as T; install(T)`: Tracker.query_source_points and implicit_reg -> HIP.  With loop=True
    also Tracker.tracking and Tracker.registration_step (the originals are kept for what the loop delegates).  With
    loop=True and colour=True the photometric and colour-consistency configurations run in the device loop too; an
    install without it turns that off again."""
    global _COLOUR
    _COLOUR = bool(loop and colour)
    tracker_module.Tracker.query_source_points = query_source_points
    tracker_module.implicit_reg = implicit_reg
    if loop:
        cls = tracker_module.Tracker
        for name, fn in (("tracking", tracking), ("registration_step", registration_step)):
            cur = cls.__dict__.get(name)
            if cur is not fn:           # installing twice keeps the first originals
                _ORIG[name] = cur
            setattr(cls, name, fn)
