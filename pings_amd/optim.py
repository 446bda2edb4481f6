"""Fused AdamW: one HIP launch per optimiser step.

`utils/tools.py:142-365` builds a stock `torch.optim.AdamW` with one parameter group per decoder, one per feature table
and six per camera, and the mapper calls `opt.step()` once per iteration: well over a hundred `_foreach_*` dispatches
for an update that moves 28 bytes per element.  `FusedAdamW` keeps torch's state (`step` on the host, `exp_avg`,
`exp_avg_sq`, created lazily on the first gradient), so `state_dict()` / `load_state_dict()` interchange with
`torch.optim.AdamW`, and hands every contiguous fp32 HIP parameter that has a gradient to `pings_adamw_step` as one job.
What the kernel does not take (CPU tensors, other dtypes, non-contiguous tensors) goes through torch's own functional
`adamw` with the same state in the same step.

`install(tools_module, *caller_modules)` wraps the reference's `setup_optimizer`; its group logic stays its own.
"""
from __future__ import annotations

import ctypes as C

import torch
from torch.optim.adamw import adamw as _torch_adamw

from . import _abi, _lib

MAX_JOBS = _abi.ADAMW_MAX_JOBS
CHUNK = _abi.ADAMW_CHUNK

_REJECTED = ("amsgrad", "maximize", "capturable", "differentiable", "fused")


class _Slot:
    """The ctypes job of one parameter, kept between steps: the betas and eps are written when they change, the
    pointers, the size and the step-dependent scalars every step."""
    __slots__ = ("job", "hyper")

    def __init__(self):
        self.job = _abi.AdamwJob()
        self.hyper = None


def _takes(t: torch.Tensor) -> bool:
    return t.is_cuda and t.dtype is torch.float32 and t.layout is torch.strided and t.is_contiguous()


class FusedAdamW(torch.optim.AdamW):
    """`torch.optim.AdamW` whose `step()` is one `pings_adamw_step` call for every HIP fp32 parameter.

    The arithmetic is torch's single-tensor AdamW operation by operation (differences are rounding only), each
    parameter keeps its own step count (a parameter without a gradient is skipped and does not advance), and results
    are bitwise reproducible.  `amsgrad`, `maximize`, `capturable`, `differentiable`, `fused` and a tensor-valued `lr`
    are not supported and raise `ValueError` at construction.  `last_launches` is the number of kernel launches of the
    last `step()` (1, or ceil(jobs / 48) for more than 48 live tensors; 0 when nothing went to the kernel)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *,
                 maximize=False, foreach=None, capturable=False, differentiable=False, fused=None):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, maximize=maximize, foreach=foreach,
                         capturable=capturable, differentiable=differentiable, fused=fused)
        for group in self.param_groups:     # options may also arrive inside the group dicts
            for key in _REJECTED:
                if group.get(key):
                    raise ValueError(f"FusedAdamW does not support {key}=True")
            if any(isinstance(group[k], torch.Tensor) for k in ("lr", "eps", "weight_decay")) or \
                    any(isinstance(b, torch.Tensor) for b in group["betas"]):
                raise ValueError("FusedAdamW takes lr, betas, eps and weight_decay as Python numbers, not tensors")
        self.last_launches = 0
        self._slots: dict = {}
        self._table = (_abi.AdamwJob * MAX_JOBS)()
        self._launches = C.c_int(0)

    def _job_table(self, n: int):
        if n > len(self._table):
            self._table = (_abi.AdamwJob * (2 * n))()
        return self._table

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()

        slots = self._slots
        live = []                   # slots of this step's jobs
        device = None               # the jobs' device: the first HIP parameter's
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            lr, wd, eps = group["lr"], group["weight_decay"], group["eps"]
            scalars = {}            # step count -> (step_size, bc2_sqrt); most tensors of a group share one
            rest = ([], [], [], [], [])
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
                state = self.state[p]
                if len(state) == 0:             # torch's lazy initialisation; `step` lives on the host
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                m, v = state["exp_avg"], state["exp_avg_sq"]
                if not (_takes(p) and (device is None or p.device == device)
                        and all(_takes(t) and t.device == p.device and t.numel() == p.numel() for t in (g, m, v))):
                    for lst, t in zip(rest, (p, g, m, v, state["step"])):
                        lst.append(t)
                    continue
                slot = slots.get(p)
                if slot is None:
                    slot = slots[p] = _Slot()
                job = slot.job
                device = p.device
                step_t = state["step"]
                if step_t.device.type != "cpu":     # a state dict of AdamW(fused=True) or a capturable one: one read,
                    step_t = state["step"] = step_t.to("cpu", torch.float32)    # then `step` lives on the host
                step_t += 1
                t = step_t.item()
                sc = scalars.get(t)
                if sc is None:
                    sc = scalars[t] = (lr / (1 - beta1 ** t), (1 - beta2 ** t) ** 0.5)
                job.p, job.g, job.m, job.v, job.n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
                job.decay = 1 - lr * wd
                job.step_size, job.bc2_sqrt = sc
                if slot.hyper != (beta1, beta2, eps):       # first step, or the caller changed the group (rare)
                    slot.hyper = (beta1, beta2, eps)
                    job.beta1, job.beta2 = beta1, beta2
                    job.one_minus_beta1, job.one_minus_beta2 = 1 - beta1, 1 - beta2
                    job.eps = eps
                live.append(slot)
            if rest[0]:
                _torch_adamw(rest[0], rest[1], rest[2], rest[3], [], rest[4], foreach=group["foreach"],
                             capturable=False, differentiable=False, fused=False, amsgrad=False, beta1=beta1,
                             beta2=beta2, lr=lr, weight_decay=wd, eps=eps, maximize=False)

        self.last_launches = 0
        if live:
            table = self._job_table(len(live))
            for i, slot in enumerate(live):
                table[i] = slot.job
            L = _lib.lib()
            if not hasattr(L, "pings_adamw_step"):  # a library built before this entry existed (same ABI version)
                raise _lib.PingsHipError(f"{_lib.LIB_PATH} has no pings_adamw_step: rebuild it with "
                                         "`python -m pings_amd.build`")
            if device.index != torch.cuda.current_device():
                with torch.cuda.device(device):
                    st = L.pings_adamw_step(table, len(live), C.byref(self._launches), _lib.stream_ptr(device))
            else:
                st = L.pings_adamw_step(table, len(live), C.byref(self._launches), _lib.stream_ptr(device))
            _lib.check(st, "pings_adamw_step")
            self.last_launches = self._launches.value
        return loss


def install(tools_module, *caller_modules) -> None:
    """`import utils.tools as T, utils.mapper as M; install(T, M)`: `setup_optimizer` returns a `FusedAdamW` with the
    groups and hyper-parameters of the `AdamW` the reference built (its group logic stays its own); any other
    optimiser (`config.opt_adam = False` gives SGD) is returned untouched.  The name is rebound in `tools_module` and
    in every caller module that imported it by name.  Installing twice changes nothing."""
    orig = tools_module.setup_optimizer
    if hasattr(orig, "_pings_original"):
        fused_setup = orig
    else:
        def fused_setup(*args, **kwargs):
            opt = orig(*args, **kwargs)
            if isinstance(opt, torch.optim.AdamW) and not isinstance(opt, FusedAdamW):
                return FusedAdamW([dict(g) for g in opt.param_groups])
            return opt

        fused_setup.__name__ = "setup_optimizer"
        fused_setup.__doc__ = orig.__doc__
        fused_setup._pings_original = orig
    for mod in (tools_module, *caller_modules):
        mod.setup_optimizer = fused_setup


def uninstall(tools_module, *caller_modules) -> None:
    """Puts the reference's own `setup_optimizer` back wherever `install` replaced it."""
    for mod in (tools_module, *caller_modules):
        orig = getattr(mod.setup_optimizer, "_pings_original", None)
        if orig is not None:
            mod.setup_optimizer = orig
