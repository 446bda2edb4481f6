"""Semantic loss block of the mapper on the HIP device (csrc/sem_loss.hip).

`semantic_loss(mapper, geo_feature, weight_knn, sem_label)` evaluates what the SDF mapping loop computes inline with
`semantic_on` (utils/mapper.py:863-866, 929-946) — `sem_label_prob` of the geo features, the IDW sum over the
neighbours, the label mask, `[::sem_label_decimation]` and `NLLLoss(reduction="mean")` — without a host wait: the
reference's two boolean-index selections are a `nonzero` each; here the selection stays on the device.  It takes the
query `sdf_losses` already made, so the gradient reaches the geo feature table through the same node as the SDF term:

    S = sdf_losses(self, coord, sdf_label, ts, weight, color_label, ...)
    R = semantic_loss(self, S.query[0], S.query[2], sem_label)
    cur_loss = cur_loss + self.config.weight_s * R.nll

`semantic_nll(raw, w, sem_label, ...)` is the block itself on raw decoder outputs.  Every launch size depends on B, k,
S and d only; no row selected gives NaN, as torch's NLLLoss of an empty input, with a zero gradient.  A label >= S is
treated as unlabelled and counted (the reference's NLLLoss device-asserts there).
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _abi, _lib
from . import decoder as _dec

F_WF, F_FREESPACE, F_LABEL_I64 = 1, 2, 4


class SemanticLoss(NamedTuple):
    nll: torch.Tensor         # 0-dim: NLLLoss(mean) over the selected rows (NaN when there is none)
    counts: torch.Tensor      # float64 [2]: selected rows, labels >= S
    selected: torch.Tensor    # bool [B]: the rows of nonzero(label_mask)[::d]


def _plain(t):
    t = t.detach()
    return t if t.is_contiguous() else t.contiguous()


class _Block(torch.autograd.Function):
    """raw decoder output -> (nll, counts, selected); `st` carries the argument block and the tensors it points to."""

    @staticmethod
    def forward(ctx, raw, st):
        L = _lib.lib()
        a, keep = st["args"], st["keep"]
        dev = raw.device
        B = int(a.B)
        keep["raw"] = _plain(raw)
        res = torch.empty(3, dtype=torch.float64, device=dev)            # counts | loss: apart from the workspace
        counts, loss = res[:2], res[2:].view(torch.float32)[:1]
        selected = torch.empty(B, dtype=torch.bool, device=dev)
        keep["selected"] = selected
        a.raw, a.selected, a.loss, a.counts = keep["raw"].data_ptr(), selected.data_ptr(), loss.data_ptr(), \
            counts.data_ptr()
        _lib.check(L.pings_sem_loss_forward(C.byref(a), _lib.stream_ptr(dev)), "pings_sem_loss_forward")
        ctx.st = st
        ctx.shape = raw.shape
        ctx.save_for_backward(raw)            # torch's version check: an in-place change before backward raises
        ctx.mark_non_differentiable(counts, selected)
        return loss.view(()), counts, selected

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_nll, _g_counts, _g_selected):
        L = _lib.lib()
        ctx.saved_tensors
        a, keep = ctx.st["args"], ctx.st["keep"]
        dev = keep["raw"].device
        gl = g_nll.detach().to(torch.float32).reshape(1).contiguous()
        d_raw = torch.empty(ctx.shape, dtype=torch.float32, device=dev)
        a.gl, a.d_raw = gl.data_ptr(), d_raw.data_ptr()
        _lib.check(L.pings_sem_loss_backward(C.byref(a), _lib.stream_ptr(dev)), "pings_sem_loss_backward")
        a.gl = a.d_raw = None
        return d_raw, None


def semantic_nll(raw: torch.Tensor, w: Optional[torch.Tensor], sem_label: torch.Tensor, *,
                 freespace_label_on: bool = False, decimation: int = 1) -> SemanticLoss:
    """NLLLoss(mean) of the IDW-summed log-softmax over every `decimation`-th labelled row.  `raw` is the semantic
    decoder's output, [B, k, S] with the weights `w` [B, k], or [B, S] with `w` None (`weighted_first`); `sem_label` is
    an int32 or int64 [B] tensor.  A row is labelled iff its label is > 0 (>= 0 with `freespace_label_on`)."""
    if not torch.is_tensor(raw) or raw.dim() != (2 if w is None else 3) or raw.shape[0] == 0 or raw.shape[-1] == 0:
        raise ValueError("semantic_nll: raw must be a non-empty [B,k,S] tensor with weights, [B,S] without, got "
                         f"{tuple(getattr(raw, 'shape', ()))}")
    if raw.dtype != torch.float32:
        raise TypeError(f"semantic_nll: raw must be float32, got {raw.dtype}")
    B, S = int(raw.shape[0]), int(raw.shape[-1])
    k = 1 if w is None else int(raw.shape[1])
    if w is not None:
        if not torch.is_tensor(w) or tuple(w.shape) not in ((B, k), (B, k, 1)):
            raise ValueError(f"semantic_nll: w must be [{B},{k}], got {tuple(getattr(w, 'shape', ()))}")
        if w.dtype != torch.float32:
            raise TypeError(f"semantic_nll: w must be float32, got {w.dtype}")
    if not torch.is_tensor(sem_label) or sem_label.dim() != 1 or sem_label.shape[0] != B:
        raise ValueError(f"semantic_nll: sem_label must be a [{B}] tensor, got {tuple(getattr(sem_label, 'shape', ()))}")
    if sem_label.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"semantic_nll: sem_label must be int32 or int64, got {sem_label.dtype}")
    d = int(decimation)
    if d < 1:
        raise ValueError(f"semantic_nll: decimation must be >= 1, got {d}")
    if not (raw.is_cuda and sem_label.is_cuda and (w is None or w.is_cuda)):
        raise _lib.PingsHipError("semantic_nll runs on the HIP device only (got a CPU tensor); there is no CPU fallback")
    L = _lib.lib()
    dev = raw.device
    flags = (F_WF * (w is None)) | (F_FREESPACE * bool(freespace_label_on)) | \
            (F_LABEL_I64 * (sem_label.dtype == torch.int64))
    a = _abi.SemLossArgs(B, k, S, d, flags)
    keep = {"w": _plain(w).view(B, k) if w is not None else None, "label": _plain(sem_label),
            "scratch": torch.empty(int(L.pings_sem_loss_scratch_bytes(B)) // 8, dtype=torch.float64, device=dev)}
    for n in ("w", "label", "scratch"):
        setattr(a, n, _lib.ptr(keep[n]))
    return SemanticLoss(*_Block.apply(raw, {"args": a, "keep": keep}))


def semantic_loss(mapper, geo_feature: torch.Tensor, weight_knn: torch.Tensor,
                  sem_label: torch.Tensor) -> SemanticLoss:
    """The semantic term of the SDF mapping loop on the query of `sdf_losses`: `geo_feature` is `S.query[0]` ([B,k,F],
    or [B,F] with `weighted_first`), `weight_knn` is `S.query[2]`.  `mapper.sem_mlp` and the config's `weighted_first`,
    `freespace_label_on` and `sem_label_decimation` are read; the caller keeps `weight_s`."""
    cfg = mapper.config
    sem_mlp = getattr(mapper, "sem_mlp", None)
    if sem_mlp is None:
        raise ValueError("semantic_loss: the mapper has no semantic decoder (sem_mlp)")
    wf = bool(getattr(cfg, "weighted_first", False))
    if not torch.is_tensor(geo_feature) or geo_feature.dim() != (2 if wf else 3):
        raise ValueError(f"semantic_loss: geo_feature must be {'[B,F]' if wf else '[B,k,F]'} "
                         f"(weighted_first: {wf}), got {tuple(getattr(geo_feature, 'shape', ()))}")
    if not wf and not torch.is_tensor(weight_knn):
        raise ValueError("semantic_loss: weight_knn must be the [B,k] neighbour weights of the query")
    d = int(getattr(cfg, "sem_label_decimation", 1))
    if d < 1:
        raise ValueError(f"semantic_loss: sem_label_decimation must be >= 1, got {d}")
    raw = _dec.mlp(sem_mlp, geo_feature)
    return semantic_nll(raw, None if wf else weight_knn, sem_label,
                        freespace_label_on=bool(getattr(cfg, "freespace_label_on", False)), decimation=d)
