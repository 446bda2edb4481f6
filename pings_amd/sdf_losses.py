"""SDF-sample loss block of the mapper on the HIP device (csrc/sdf_loss.hip).

`sdf_losses(mapper, coord, sdf_label, ts, weight, color_label, ...)` evaluates the loss the SDF mapping loop
(utils/mapper.py:836-930) and every joint iteration (:1493-1544) compute inline — BCE on the SDF labels, the Eikonal
term over every `gradient_decimation`-th sample of the free-space band and the colour L1 over the near-surface samples
with a colour label — without a host wait: the reference selects both subsets with boolean indexing (a `nonzero`
each); here the subset sizes stay on the device.  The values come back un-weighted; the caller keeps the lambdas:

    S = sdf_losses(self, coord, sdf_label, ts, weight, color_label, eikonal=self.config.weight_e > 0,
                   color=self.config.color_on, color_weighted=False)
    sdf_loss = S.bce * self.config.lambda_sdf                          # and so on

Every launch size depends on B and d only: the Eikonal rows are compacted on the device into a buffer of capacity
ceil(B/d) whose padding rows go through the same central differences and receive an exactly zero upstream gradient.
An empty subset gives NaN, as torch's mean of an empty tensor does in the reference.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _abi, _lib
from . import decoder as _dec
from . import neural_points as _np

F_EIK, F_COL, F_COL_W, F_BCE_W, F_WF = 1, 2, 4, 8, 16


class SdfLosses(NamedTuple):
    bce: torch.Tensor         # BCEWithLogits(sdf_pred / sdf_scale, sigmoid(label / sdf_scale)), mean over the B rows
    eikonal: torch.Tensor     # mean (|g| - 1)^2 over the ceil(M/d) Eikonal rows (NaN when M = 0; 0 when disabled)
    color: torch.Tensor       # mean |colour - label| over (colour rows x channels) (NaN when none; 0 when disabled)
    counts: torch.Tensor      # float64 [2]: Eikonal rows, colour rows
    sdf_pred: torch.Tensor    # [B]
    query: tuple              # the five query_feature outputs (geo, colour, weights, nn_counts, certainty)


def _f32(t):
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    return t if t.is_contiguous() else t.contiguous()


class _Block(torch.autograd.Function):
    """(decoder SDF per neighbour, colour decoder output, Eikonal gradient rows) -> the three losses, counts, sdf_pred."""

    @staticmethod
    def forward(ctx, s, c, g, st):
        L = _lib.lib()
        a = st["args"]
        dev = s.device
        keep = st["keep"]
        keep["s"] = _f32(s)
        keep["c"] = _f32(c) if c is not None else None
        keep["g"] = _f32(g) if g is not None else None
        a.s, a.c, a.g = (_lib.ptr(keep[k]) for k in ("s", "c", "g"))
        B = int(a.B)
        pred = torch.empty(B, dtype=torch.float32, device=dev)
        # the outputs live in a small buffer of their own: a caller holding the losses does not keep the workspace
        res = torch.empty(4, dtype=torch.float64, device=dev)
        counts, losses = res[:2], res[2:].view(torch.float32)[:3]
        a.sdf_pred, a.losses, a.counts = pred.data_ptr(), losses.data_ptr(), counts.data_ptr()
        _lib.check(L.pings_sdf_loss_reduce(C.byref(a), _lib.stream_ptr(dev)), "pings_sdf_loss_reduce")
        ctx.st = st
        ctx.shapes = [None if t is None else t.shape for t in (s, c, g)]
        ctx.save_for_backward(s, c, g)        # torch's version check: an in-place change before backward raises
        ctx.mark_non_differentiable(counts)
        ctx.set_materialize_grads(False)
        return tuple(losses.unbind(0)) + (counts, pred.view(B))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_bce, g_eik, g_col, _g_counts, g_pred):
        L = _lib.lib()
        ctx.saved_tensors
        st = ctx.st
        a = st["args"]
        dev = st["keep"]["s"].device
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        gl = torch.stack([zero if x is None else x.detach().to(torch.float32) for x in (g_bce, g_eik, g_col)])
        gp = _f32(g_pred) if g_pred is not None else None
        s_shape, c_shape, g_shape = ctx.shapes
        d_s = torch.empty(s_shape, dtype=torch.float32, device=dev)
        d_c = torch.empty(c_shape, dtype=torch.float32, device=dev) if c_shape is not None else None
        d_g = torch.empty(g_shape, dtype=torch.float32, device=dev) if g_shape is not None else None
        a.gl, a.g_pred, a.d_s, a.d_c, a.d_g = gl.data_ptr(), _lib.ptr(gp), d_s.data_ptr(), _lib.ptr(d_c), _lib.ptr(d_g)
        _lib.check(L.pings_sdf_loss_backward(C.byref(a), _lib.stream_ptr(dev)), "pings_sdf_loss_backward")
        a.gl = a.g_pred = a.d_s = a.d_c = a.d_g = None
        need = ctx.needs_input_grad
        return (d_s if need[0] else None), (d_c if need[1] else None), (d_g if need[2] else None), None


def _check_vec(name, t, B, dtype_ok=True):
    if not torch.is_tensor(t) or t.dim() != 1 or t.shape[0] != B:
        raise ValueError(f"sdf_losses: {name} must be a [{B}] tensor, got {tuple(getattr(t, 'shape', ()))}")
    if dtype_ok and t.dtype != torch.float32:
        raise TypeError(f"sdf_losses: {name} must be float32, got {t.dtype}")


def sdf_losses(mapper, coord: torch.Tensor, sdf_label: torch.Tensor, ts: torch.Tensor, weight: torch.Tensor,
               color_label: Optional[torch.Tensor] = None, *, eikonal: bool = True, color: bool = False,
               color_weighted: Optional[bool] = None) -> SdfLosses:
    """The SDF-sample loss block of both mapping loops.  `mapper` is the Mapper (its `config`, `sdf_scale`,
    `neural_points`, `sdf_mlp` and, with `color`, `color_mlp` are read).  `eikonal` / `color` switch the two subset terms
    (the caller's `ekional_loss_on and weight_e > 0` / `color_on`; `color` also queries the colour features).  The BCE
    term is weighted by |weight| iff `config.loss_weight_on`; `color_weighted` weights the colour term the same way
    (None: `config.loss_weight_on`, the SDF loop; the joint iteration passes False).
    Side effects are those of `query_feature(coord, ts, query_color_feature=color)` in training mode."""
    cfg = mapper.config
    if str(getattr(cfg, "main_loss_type", "bce")) != "bce":
        raise NotImplementedError(f"sdf_losses: main_loss_type {cfg.main_loss_type!r} is not implemented (only 'bce', "
                                  "the one every shipped config uses)")
    if bool(getattr(mapper, "require_gradient", False)) or (eikonal and not bool(getattr(cfg, "numerical_grad", True))):
        raise NotImplementedError(
            "sdf_losses: the analytic Eikonal branch (require_gradient, numerical_grad: False) is not supported: the "
            "reference differentiates the masked copy sdf_pred[mask] w.r.t. coord[mask], which is not an input of it, "
            "and torch raises 'One of the differentiated Tensors appears to not have been used in the graph' "
            "(DESIGN.md §4)")
    if not torch.is_tensor(coord) or coord.dim() != 2 or coord.shape[1] != 3 or coord.shape[0] == 0:
        raise ValueError(f"sdf_losses: coord must be a non-empty [B,3] tensor, got {tuple(getattr(coord, 'shape', ()))}")
    if coord.dtype != torch.float32:
        raise TypeError(f"sdf_losses: coord must be float32, got {coord.dtype}")
    B = int(coord.shape[0])
    _check_vec("sdf_label", sdf_label, B)
    _check_vec("weight", weight, B)
    if ts is not None:
        _check_vec("ts", ts, B, dtype_ok=False)
        if ts.dtype.is_floating_point:
            raise TypeError(f"sdf_losses: ts must be an integer tensor, got {ts.dtype}")
    d = int(getattr(cfg, "gradient_decimation", 1))
    if d < 1:
        raise ValueError(f"sdf_losses: gradient_decimation must be >= 1, got {d}")
    npm, dec = mapper.neural_points, mapper.sdf_mlp
    if not _np.fused_supported(npm, dec):
        raise NotImplementedError("sdf_losses: the block needs the fused SDF kernels' decoder shape (one hidden ReLU "
                                  "level of at most 64 units, no layer norm: every shipped config)")
    cmlp = None
    if color:
        cmlp = getattr(mapper, "color_mlp", None)
        if cmlp is None or not _dec._supported(cmlp):
            raise NotImplementedError("sdf_losses: the colour term needs a colour decoder of the fused MLP kernels' "
                                      "shape (one hidden ReLU level: every shipped config)")
        Cc = int(cmlp.lout.weight.shape[0])
        if not torch.is_tensor(color_label) or tuple(color_label.shape) != (B, Cc):
            raise ValueError(f"sdf_losses: color_label must be [{B},{Cc}], got "
                             f"{tuple(getattr(color_label, 'shape', ()))}")
        if color_label.dtype != torch.float32:
            raise TypeError(f"sdf_losses: color_label must be float32, got {color_label.dtype}")
        if Cc > 8:
            raise ValueError(f"sdf_losses: at most 8 colour channels, got {Cc}")
    if not coord.is_cuda:
        raise _lib.PingsHipError("sdf_losses runs on the HIP device only (got a CPU tensor); there is no CPU fallback")
    L = _lib.lib()
    dev = coord.device
    cap = (B + d - 1) // d
    loss_w = bool(getattr(cfg, "loss_weight_on", False))
    color_w = loss_w if color_weighted is None else bool(color_weighted)

    # main query (training side effects: certainty accumulation, ts_update), decoder, colour decoder
    query = _np.query_feature(npm, coord, ts, query_color_feature=bool(color))
    geo, col, wk = query[0], query[1], query[2]
    wf = geo.dim() == 2
    k = int(wk.shape[1])
    s = _dec.sdf(dec, geo).reshape((B,) if wf else (B, k))
    c = _dec.mlp(cmlp, col) if color else None

    flags = (F_EIK * bool(eikonal)) | (F_COL * bool(color)) | (F_COL_W * bool(color and color_w)) | \
            (F_BCE_W * loss_w) | (F_WF * wf)
    a = _abi.SdfLossArgs(B, cap, k, int(c.shape[-1]) if color else 0, d, flags, float(mapper.sdf_scale),
                         float(getattr(cfg, "free_sample_end_dist_m", 0.0)),
                         float(0.5 * getattr(cfg, "surface_sample_range_m", 0.0)))
    keep = {"coord": _f32(coord), "label": _f32(sdf_label), "w": _f32(wk).view(B, k),
            "weight": _f32(weight) if (flags & (F_COL_W | F_BCE_W)) else None,
            "color_label": _f32(color_label) if color else None}
    nb = int(L.pings_sdf_loss_partials(B, cap))
    ws = torch.empty(3 + cap + 8 * nb, dtype=torch.int32, device=dev)   # meta | idx | part (fp64, 8-byte aligned)
    keep["meta"], keep["idx"] = ws[:2], ws[2:2 + cap]
    off = (2 + cap + 1) // 2 * 2
    keep["part"] = ws[off:off + 8 * nb].view(torch.float64)
    keep["xsel"] = torch.empty(cap, 3, dtype=torch.float32, device=dev) if eikonal else None
    for n in ("coord", "label", "weight", "color_label", "w", "meta", "idx", "part", "xsel"):
        setattr(a, n, _lib.ptr(keep[n]))
    st = {"args": a, "keep": keep}
    g = None
    if eikonal:
        _lib.check(L.pings_sdf_loss_select(C.byref(a), _lib.stream_ptr(dev)), "pings_sdf_loss_select")
        eps = float(cfg.voxel_size_m) * float(cfg.num_grad_step_ratio)
        g = _np.numerical_gradient(npm, dec, keep["xsel"], None, eps, True)
    bce, eik, colv, counts, pred = _Block.apply(s, c, g, st)
    return SdfLosses(bce, eik, colv, counts, pred, query)
