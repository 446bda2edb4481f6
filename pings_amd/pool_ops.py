"""The mapper's SDF training-sample pool on the HIP device (csrc/pool.hip).

Three drop-in methods and one free function on the reference's own tensors; no pool state lives here:

  `sample`               `DataSampler.sample` (utils/data_sampler.py:18-264): three random draws and one kernel
  `get_batch`            `Mapper.get_batch` (utils/mapper.py:704-771): the reference's `randint` calls and one kernel
  `transform_data_pool`  `Mapper.transform_data_pool` (utils/mapper.py:774-778): range check, one read, one kernel
  `window_rows`          the sample window of `process_frame` (utils/mapper.py:429-438): one read, no [N] temporary

`install` rebinds the three methods and keeps the originals, which the methods call for the inputs the kernels do not
take (CPU tensors, other dtypes, `color_valid_mask`).  The random draws are the reference's own calls in the
reference's order, so under one seed the samples and the batch indices are the reference's.
"""
from __future__ import annotations

import ctypes as C
from contextlib import nullcontext

import torch

from . import _abi, _lib

_status_words: dict = {}       # device -> int32 [1]: bit 0 = a get_batch index was out of range (pings_pool_draw)


def _entry(name: str):
    L = _lib.lib()
    if not hasattr(L, name):    # a library built before this entry existed (same ABI version)
        raise _lib.PingsHipError(f"{_lib.LIB_PATH} has no {name}: rebuild it with `python -m pings_amd.build`")
    return getattr(L, name)


def _guard(dev):
    return torch.cuda.device(dev) if dev.index != torch.cuda.current_device() else nullcontext()


def _original(self, name: str):
    orig = getattr(type(self), f"_pings_{name}_original", None)
    if orig is None:
        raise _lib.PingsHipError(f"pool_ops.{name}: these inputs take the reference's own method, and none was kept "
                                 "(`pool_ops.install` keeps it); the HIP path needs contiguous float32 device tensors")
    return orig


def _f32_dev(t, dev=None) -> bool:
    return (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype is torch.float32 and t.is_contiguous()
            and (dev is None or t.device == dev))


def _status_word(dev) -> torch.Tensor:
    w = _status_words.get(dev)
    if w is None:
        w = _status_words[dev] = torch.zeros(1, dtype=torch.int32, device=dev)
    return w


def last_status(device=None) -> int:
    """The status word of `get_batch` on `device` (default: the current one), read and cleared: bit 0 is set when an
    index of a batch was outside the pool (a stale `local_sample_indices` / `new_idx`; the reference raises there) and
    that row was zero-filled.  One host read, made only when asked for."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    w = _status_words.get(dev)
    if w is None:
        return 0
    _lib.note_sync("pool_status")
    v = int(w.item())
    if v:
        w.zero_()
    return v


# ---------------------------------------------------------------- DataSampler.sample
@torch.no_grad()
def sample(self, points_torch, normal_torch, sem_label_torch, color_torch, color_valid_mask=None, _noise=None):
    """`DataSampler.sample`: (coord [P*S,3], sdf_label [P*S], normal [P*S,3] | None, sem [P*S] int32 | None,
    color [P*S,C] | None, weight [P*S]) in the reference's ray-wise order.  `torch.randn(P*ns, 1)`,
    `torch.rand(P*nf, 1)` and `torch.rand(P*nb, 1)` are drawn on the device in this order (zero-size ones included), so
    the generator ends where the reference leaves it.  `_noise` (tests) supplies the three tensors instead.  The class's
    original method is called for `color_valid_mask`, CPU tensors, non-float32 points and `P == 0`."""
    cfg = self.config
    pts = points_torch
    if (color_valid_mask is not None or not isinstance(pts, torch.Tensor) or not pts.is_cuda
            or pts.dtype is not torch.float32 or pts.dim() != 2 or pts.shape[1] != 3 or pts.shape[0] == 0
            or (normal_torch is not None and not (_f32_dev(normal_torch.contiguous(), pts.device)
                                                  and tuple(normal_torch.shape) == tuple(pts.shape)))
            or (color_torch is not None and not (_f32_dev(color_torch.contiguous(), pts.device)
                                                 and color_torch.dim() == 2 and 1 <= color_torch.shape[1] <= 4
                                                 and color_torch.shape[0] == pts.shape[0]))
            or (sem_label_torch is not None and not (sem_label_torch.is_cuda and sem_label_torch.dim() == 1
                                                     and sem_label_torch.shape[0] == pts.shape[0]
                                                     and not sem_label_torch.is_floating_point()))):
        return _original(self, "sample")(self, points_torch, normal_torch, sem_label_torch, color_torch,
                                         color_valid_mask)
    dev = pts.device
    P = int(pts.shape[0])
    ns, nf, nb = int(cfg.surface_sample_n), int(cfg.free_front_n), int(cfg.free_behind_n)
    S = ns + nf + nb + 1
    if _noise is None:
        rdev = getattr(self, "dev", dev)
        z_s = torch.randn(P * ns, 1, device=rdev)
        u_f = torch.rand(P * nf, 1, device=rdev)
        u_b = torch.rand(P * nb, 1, device=rdev)
    else:
        z_s, u_f, u_b = _noise
    for t, n, what in ((z_s, P * ns, "surface"), (u_f, P * nf, "front"), (u_b, P * nb, "behind")):
        if not _f32_dev(t, dev) or t.numel() != n:
            raise _lib.PingsHipError(f"pool_ops.sample: the {what} noise must hold {n} float32 values on {dev}")
    pts = pts.detach().contiguous()
    normal = None if normal_torch is None else normal_torch.detach().contiguous()
    color = None if color_torch is None else color_torch.detach().contiguous()
    sem = None
    if sem_label_torch is not None:
        sem = sem_label_torch.detach()
        if sem.dtype not in (torch.int32, torch.int64):
            sem = sem.to(torch.int64)
        sem = sem.contiguous()
    Cc = 0 if color is None else int(color.shape[1])
    rows = P * S
    coord = torch.empty(rows, 3, dtype=torch.float32, device=dev)
    label = torch.empty(rows, dtype=torch.float32, device=dev)
    weight = torch.empty(rows, dtype=torch.float32, device=dev)
    o_normal = None if normal is None else torch.empty(rows, 3, dtype=torch.float32, device=dev)
    o_sem = None if sem is None else torch.empty(rows, dtype=torch.int32, device=dev)
    o_color = None if color is None else torch.empty(rows, Cc, dtype=torch.float32, device=dev)
    p = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
    a = _abi.PoolSampleArgs(
        P, ns, nf, nb, Cc, int(bool(cfg.dist_weight_on)), int(bool(cfg.behind_dropoff_on)),
        int(sem is not None and sem.dtype is torch.int64), 0,
        float(cfg.surface_sample_range_m), float(cfg.free_sample_begin_ratio), float(cfg.free_sample_end_dist_m),
        float(cfg.dist_weight_scale), float(cfg.max_range),
        p(pts), p(normal), p(sem), p(color), p(z_s), p(u_f), p(u_b),
        p(coord), p(label), p(weight), p(o_normal), p(o_sem), p(o_color))
    fn = _entry("pings_pool_sample")
    with _guard(dev):
        st = fn(C.byref(a), _lib.stream_ptr(dev))
    _lib.check(st, "pings_pool_sample")
    return coord, label, o_normal, o_sem, o_color, weight


# ---------------------------------------------------------------- Mapper.get_batch
def _i64(t: torch.Tensor) -> torch.Tensor:
    return (t if t.dtype is torch.int64 else t.to(torch.int64)).contiguous()


@torch.no_grad()
def get_batch(self, global_coord=True, _draws=None):
    """`Mapper.get_batch`: (coord, sdf_label, ts, normal_label, sem_label, color_label, weight).  The `torch.randint`
    calls are the reference's, history first and then new, and its branches are kept as written (with
    `new_idx_count == 0` the batch is drawn from `self.pool_sample_count` rows and `local_sample_indices` is ignored).
    The index chain and every gather are one launch; nothing is read back: an index outside the pool (the reference
    raises) zero-fills that row and sets bit 0 of `last_status()`.  `_draws` (tests) supplies `(r_hist, r_new | None)`."""
    cfg = self.config
    pools = [self.global_coord_pool, self.sdf_label_pool, self.time_pool, self.normal_label_pool, self.sem_label_pool,
             self.color_pool, self.weight_pool]
    coord_pool = pools[0]
    if coord_pool is None or not all(t is None or (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous()
                                                   and t.device == coord_pool.device) for t in pools):
        return _original(self, "get_batch")(self, global_coord)
    dev = coord_pool.device
    local = self.local_sample_indices
    pool_sample_count = int(local.shape[0]) if local is not None else int(self.pool_sample_count)
    r_new, new_idx = None, None
    if (cfg.bs_new_sample > 0 and self.new_idx is not None and not self.dataset.lose_track
            and not self.dataset.stop_status):
        new_idx_count = int(self.new_idx.shape[0])
        if new_idx_count > 0:
            bs_new = min(new_idx_count, int(cfg.bs_new_sample))
            bs_history = int(cfg.bs) - bs_new
            if _draws is None:
                r_hist = torch.randint(0, pool_sample_count, (bs_history,), device=self.device)
                r_new = torch.randint(0, new_idx_count, (bs_new,), device=self.device)
            else:
                r_hist, r_new = _draws
            new_idx = self.new_idx
        else:                                           # uniformly sample the pool (:735-738)
            r_hist = (torch.randint(0, self.pool_sample_count, (cfg.bs,), device=self.device) if _draws is None
                      else _draws[0])
            local = None
    else:
        r_hist = torch.randint(0, pool_sample_count, (cfg.bs,), device=self.device) if _draws is None else _draws[0]
    r_hist = _i64(r_hist)
    bs_history = int(r_hist.shape[0])
    bs_new = 0 if r_new is None else int(r_new.shape[0])
    bs = bs_history + bs_new
    if local is not None:
        local = _i64(local)
    if r_new is not None:
        r_new, new_idx = _i64(r_new), _i64(new_idx)
    for t in (r_hist, r_new, local, new_idx):
        if t is not None and t.device != dev:
            raise _lib.PingsHipError(f"pool_ops.get_batch: an index tensor is on {t.device}, the pool on {dev}")
    n_rows = int(coord_pool.shape[0])
    live = [t for t in pools if t is not None]
    if any(int(t.shape[0]) != n_rows for t in live):
        raise _lib.PingsHipError("pool_ops.get_batch: the pool tensors do not have the same number of rows")
    jobs = (_abi.GatherJob * len(live))()
    outs = []
    for g, src in enumerate(live):
        out = torch.empty((bs,) + tuple(src.shape[1:]), dtype=src.dtype, device=dev)
        row = src.element_size()
        for d in src.shape[1:]:
            row *= int(d)
        outs.append(out)
        jobs[g] = _abi.GatherJob(src.data_ptr() if src.numel() else None, out.data_ptr(), row, bs)
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
    fn = _entry("pings_pool_draw")
    with _guard(dev):
        word = _status_word(dev)
        st = 0 if bs == 0 else fn(jobs, len(live), ptr(r_hist), bs_history, ptr(r_new), bs_new, ptr(local),
                                  0 if local is None else int(local.shape[0]), ptr(new_idx),
                                  0 if new_idx is None else int(new_idx.shape[0]), n_rows, word.data_ptr(),
                                  _lib.stream_ptr(dev))
    _lib.check(st, "pings_pool_draw")
    it = iter(outs)
    coord, sdf_label, ts, normal, sem, color, weight = (None if t is None else next(it) for t in pools)
    return coord, sdf_label, ts, normal, sem, color, weight


# ---------------------------------------------------------------- Mapper.transform_data_pool
@torch.no_grad()
def _transform_in_place(pool: torch.Tensor, ts: torch.Tensor, pose_diff_torch: torch.Tensor) -> None:
    dev = pool.device
    n = int(pool.shape[0])
    pose = pose_diff_torch.detach().to(dev)
    if pose.dim() != 3 or tuple(pose.shape[1:]) != (4, 4):
        raise ValueError(f"pose_diff_torch must be [T, 4, 4], got {tuple(pose.shape)}")
    if pose.dtype not in (torch.float64, torch.float32):
        pose = pose.to(torch.float32)                   # what `transformation.to(points)` gives
    pose = pose.contiguous()
    T = int(pose.shape[0])
    if n == 0:
        return
    if int(ts.shape[0]) != n or ts.dim() != 1:
        raise IndexError(f"time_pool has shape {tuple(ts.shape)}, the pool {n} rows")
    ts_i64 = int(ts.dtype is torch.int64)
    mm = torch.empty(2, dtype=torch.int64, device=dev)
    with _guard(dev):
        st = _entry("pings_pool_ts_range")(ts.data_ptr(), ts_i64, n, mm.data_ptr(), _lib.stream_ptr(dev))
        _lib.check(st, "pings_pool_ts_range")
        _lib.note_sync("pool_transform_bounds")         # once per loop closure; `pose_diff_torch[time_pool]` raises
        lo, hi = mm.tolist()
        if lo < -T or hi >= T:                          # before any row is moved
            raise IndexError(f"time_pool holds timestamps in [{lo}, {hi}], outside pose_diff_torch of size {T}")
        st = _entry("pings_pool_transform")(n, pool.data_ptr(), ts.data_ptr(), ts_i64, pose.data_ptr(),
                                            int(pose.dtype is torch.float64), T, None, _lib.stream_ptr(dev))
    _lib.check(st, "pings_pool_transform")


def transform_data_pool(self, pose_diff_torch):
    """`Mapper.transform_data_pool`: `p <- R[ts] p + t[ts]` in place on `self.global_coord_pool` (the same storage is
    re-assigned), without the reference's `[N,4,4]` gather.  A timestamp outside `[-T, T)` raises `IndexError` before
    any row is moved.  A pool that is not a contiguous float32 device tensor, or that requires grad, takes the class's
    original method."""
    pool, ts = self.global_coord_pool, self.time_pool
    if not (_f32_dev(pool) and not pool.requires_grad and pool.dim() == 2 and pool.shape[1] == 3
            and isinstance(ts, torch.Tensor) and ts.device == pool.device and ts.is_contiguous()
            and ts.dtype in (torch.int32, torch.int64) and isinstance(pose_diff_torch, torch.Tensor)):
        return _original(self, "transform_data_pool")(self, pose_diff_torch)
    _transform_in_place(pool, ts, pose_diff_torch)
    self.global_coord_pool = pool


# ---------------------------------------------------------------- the sample window of process_frame
@torch.no_grad()
def window_rows(global_coord_pool, origin, radius, range_filter_2d) -> torch.Tensor:
    """Ascending int64 rows of `global_coord_pool` [N,3] within `radius` of `origin` (in x, y only when
    `range_filter_2d`): utils/mapper.py:429-438 without its three pool-sized temporaries; one host read (the count).

    Departure from the reference: the result is ALWAYS 1-D.  The reference's `torch.nonzero(mask).squeeze()` is 0-dim
    for a window of exactly one row, and its next line (`.shape[0]`) then fails.

    A pool that is not a contiguous float32 device tensor, or an origin tensor of another dtype (torch would promote
    the subtraction), is evaluated with the reference's torch expression."""
    pool = global_coord_pool
    if isinstance(origin, torch.Tensor) and origin.dtype is torch.float32:
        org = origin.detach().reshape(-1)
    elif isinstance(origin, torch.Tensor):
        org = None
    else:
        org = torch.as_tensor(origin, dtype=torch.float32).reshape(-1)
    if not (_f32_dev(pool) and pool.dim() == 2 and pool.shape[1] == 3 and org is not None and org.numel() == 3):
        rel = pool - origin
        dist = torch.norm(rel[:, :2], p=2, dim=1) if range_filter_2d else torch.norm(rel, p=2, dim=1)
        return torch.nonzero(dist < radius).reshape(-1)
    dev = pool.device
    org = org.to(dev).contiguous()
    n = int(pool.shape[0])
    L = _lib.lib()
    count = C.c_int64(0)
    with _guard(dev):
        scratch = torch.empty(_entry("pings_pool_window_scratch_bytes")(n), dtype=torch.uint8, device=dev)
        _lib.note_sync("pool_window_count")
        _lib.check(L.pings_pool_window_count(pool.data_ptr(), n, org.data_ptr(), float(radius), int(bool(range_filter_2d)),
                                             scratch.data_ptr(), C.byref(count), _lib.stream_ptr(dev)),
                   "pings_pool_window_count")
        k = int(count.value)
        rows = torch.empty(k, dtype=torch.int64, device=dev)
        if k:
            _lib.check(L.pings_pool_window(pool.data_ptr(), n, org.data_ptr(), float(radius), int(bool(range_filter_2d)),
                                           scratch.data_ptr(), rows.data_ptr(), k, _lib.stream_ptr(dev)),
                       "pings_pool_window")
    return rows


# ---------------------------------------------------------------- install
_METHODS = (("sample", sample), ("get_batch", get_batch), ("transform_data_pool", transform_data_pool))


def _rebind(cls, name, fn):
    if cls.__dict__.get(name) is not fn:
        setattr(cls, f"_pings_{name}_original", getattr(cls, name, None))
        setattr(cls, name, fn)


def _restore(cls, name, fn):
    if cls.__dict__.get(name) is fn:
        orig = cls.__dict__.get(f"_pings_{name}_original")
        if orig is not None:
            setattr(cls, name, orig)
        else:
            delattr(cls, name)
    if f"_pings_{name}_original" in cls.__dict__:
        delattr(cls, f"_pings_{name}_original")


def install(sampler_cls=None, mapper_cls=None) -> None:
    """`from utils.data_sampler import DataSampler; from utils.mapper import Mapper; install(DataSampler, Mapper)`:
    rebinds `DataSampler.sample`, `Mapper.get_batch` and `Mapper.transform_data_pool`.  The originals are kept on the
    classes for the fallbacks and for `uninstall`.  Installing twice changes nothing."""
    if sampler_cls is not None:
        _rebind(sampler_cls, "sample", sample)
    if mapper_cls is not None:
        _rebind(mapper_cls, "get_batch", get_batch)
        _rebind(mapper_cls, "transform_data_pool", transform_data_pool)


def uninstall(sampler_cls=None, mapper_cls=None) -> None:
    """Puts the reference's own methods back wherever `install` replaced them."""
    if sampler_cls is not None:
        _restore(sampler_cls, "sample", sample)
    if mapper_cls is not None:
        _restore(mapper_cls, "get_batch", get_batch)
        _restore(mapper_cls, "transform_data_pool", transform_data_pool)
