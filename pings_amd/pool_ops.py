"""The mapper's SDF training-sample pool on the HIP device (csrc/pool.hip, csrc/pool_frame.hip; DESIGN §2.5g,
INTEGRATION §4k).

Drop-in methods and free functions on the reference's own tensors; no pool state lives here:

  `sample`               `DataSampler.sample` (utils/data_sampler.py:18-264): three random draws and one kernel
  `get_batch`            `Mapper.get_batch` (utils/mapper.py:704-771): the reference's `randint` calls and one kernel
  `transform_data_pool`  `Mapper.transform_data_pool` (utils/mapper.py:774-778): range check, one read, one kernel
  `window_rows`          the sample window of `process_frame` (utils/mapper.py:429-438): one read, no [N] temporary
  `process_frame`        `Mapper.process_frame` (utils/mapper.py:170-526), composed of the kernels of this package and
                         `append_frame` (:340-366, one launch), `filter_pool` (:386-423, one read), `select_update`
                         (:262-284, one read) on a `PoolStore`, the growable backing kept on the mapper instance

`install` rebinds the three methods (with `frame=True` also `process_frame`) and keeps the originals, which the methods
call for the inputs the kernels do not take (CPU tensors, other dtypes, `color_valid_mask`, the mono-depth branch).  The
random draws are the reference's own calls in the reference's order, so under one seed the samples, the batch indices
and the rows the capacity filter discards are the reference's.
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


# ---------------------------------------------------------------- the growable backing of the pool
POOL_NAMES = ("global_coord_pool", "sdf_label_pool", "weight_pool", "time_pool", "sem_label_pool", "color_pool",
              "normal_label_pool")
_OPTIONAL = POOL_NAMES[4:]
_filter_words: dict = {}       # device -> int32 [1]: bit 0 = a discard draw was outside the pool (pings_pool_discard_mark)


class PoolStore:
    """Two buffer sets (front and back) behind the mapper's seven pool attributes, which are leading-row views of the
    front set: contiguous tensors with the reference's names, shapes and dtypes.  `append_frame` writes new rows behind
    the views (geometric growth; a regrow is one copy per tensor), `filter_pool` compacts front into back and swaps.
    The back set is allocated when a filter first needs it and dropped by a regrow, so a full pool costs two buffer
    sets (2 x 36 B per row with RGB colour, 2 x 52 B with labels and normals too).  The store keeps no pool state of
    its own: the
    attributes are the pool, and an attribute that is no longer the store's view (after `free_pool`, a load, a user
    assignment; told by data pointer, shape and dtype) is taken in again with one copy."""

    GROWTH, MIN_ROWS = 1.5, 4096

    def __init__(self, device):
        self.device = torch.device(device)
        self.capacity, self.rows = 0, 0
        self.front: dict = {}
        self.back: dict = {}

    def owns(self, name: str, t) -> bool:
        buf = self.front.get(name)
        return (buf is not None and isinstance(t, torch.Tensor) and t.dtype is buf.dtype and t.device == buf.device
                and tuple(t.shape) == (self.rows,) + tuple(buf.shape[1:]) and t.is_contiguous()
                and (self.rows == 0 or t.data_ptr() == buf.data_ptr()))   # torch: a view of no rows has no pointer

    def _empty(self, rows: int, like: torch.Tensor) -> torch.Tensor:
        return torch.empty((rows,) + tuple(like.shape[1:]), dtype=like.dtype, device=self.device)

    def reserve(self, rows: int, back: bool = False) -> None:
        """Room for `rows` rows in the front set; `back` also puts the back set in place."""
        if rows > self.capacity:
            cap = max(int(rows), int(self.capacity * self.GROWTH), self.MIN_ROWS)
            self.back.clear()
            for name, buf in list(self.front.items()):
                new = self._empty(cap, buf)
                new[:self.rows].copy_(buf[:self.rows])
                self.front[name] = new
            self.capacity = cap
        for name in [k for k in self.back if k not in self.front]:
            del self.back[name]
        if back:
            for name, buf in self.front.items():
                b = self.back.get(name)
                if b is None or b.shape != buf.shape or b.dtype is not buf.dtype:
                    self.back[name] = torch.empty_like(buf)

    def drop(self, name: str) -> None:
        self.front.pop(name, None)
        self.back.pop(name, None)

    def adopt(self, mapper, room: int = 0) -> None:
        """Takes the mapper's pool attributes as they are now: nothing is done for the store's own views, any other
        tensor is copied into the front set once (with `room` more rows behind it when a buffer has to be made)."""
        tensors = {name: getattr(mapper, name, None) for name in POOL_NAMES}
        for name in POOL_NAMES[:4]:
            if not isinstance(tensors[name], torch.Tensor):     # `free_pool`: the reference's torch.cat raises as well
                raise TypeError(f"pool_ops: mapper.{name} is {type(tensors[name]).__name__}, expected a Tensor")
        live = {k: t for k, t in tensors.items() if t is not None}
        n = int(tensors["global_coord_pool"].shape[0])
        for name, t in live.items():
            if not (isinstance(t, torch.Tensor) and t.device == self.device and int(t.shape[0]) == n):
                raise _lib.PingsHipError(f"pool_ops: mapper.{name} must be a tensor of {n} rows on {self.device}")
        for name in [k for k in self.front if k not in live]:
            self.drop(name)
        stale = [name for name, t in live.items() if not self.owns(name, t)]
        if stale:
            if n + room > self.capacity:
                self.back.clear()
                self.capacity = max(n + room, self.MIN_ROWS)
                stale = list(live)                              # every buffer is replaced; the views are read below
            for name in stale:
                t = live[name].detach()
                buf = self.front.get(name)
                if (buf is None or int(buf.shape[0]) != self.capacity or buf.dtype is not t.dtype
                        or tuple(buf.shape[1:]) != tuple(t.shape[1:])):
                    buf = self._empty(self.capacity, t)
                    self.back.pop(name, None)
                elif n and t.data_ptr() != buf.data_ptr() and (t.untyped_storage().data_ptr()
                                                               == buf.untyped_storage().data_ptr()):
                    t = t.clone()                               # a shifted slice of this very buffer
                buf[:n].copy_(t)
                self.front[name] = buf
        self.rows = n
        if stale:
            self.publish(mapper)

    def publish(self, mapper) -> None:
        """Re-points the mapper's attributes at the front set; a pool the store does not hold is None."""
        for name in POOL_NAMES:
            buf = self.front.get(name)
            setattr(mapper, name, None if buf is None else buf[:self.rows])

    def swap(self) -> None:
        self.front, self.back = self.back, self.front


def pool_store(mapper) -> PoolStore:
    """The mapper's `PoolStore` (`mapper._pings_pool_store`), made on first use on the pool's device."""
    store = getattr(mapper, "_pings_pool_store", None)
    dev = mapper.global_coord_pool.device
    if store is None or store.device != dev:
        store = mapper._pings_pool_store = PoolStore(dev)
    return store


def _pose_dev(pose, dev) -> torch.Tensor:
    pose = pose.detach().to(dev)
    if tuple(pose.shape) != (4, 4):
        raise ValueError(f"the pose must be [4, 4], got {tuple(pose.shape)}")
    if pose.dtype not in (torch.float64, torch.float32):
        pose = pose.to(torch.float32)                   # what `transformation.to(points)` gives
    return pose.contiguous()


def _rows_f32(t, rows, tail, dev, what):
    if not (_f32_dev(t, dev) and tuple(t.shape) == (rows,) + tail):
        raise _lib.PingsHipError(f"pool_ops: {what} must be a contiguous float32 tensor of shape "
                                 f"{(rows,) + tail} on {dev}")


# ---------------------------------------------------------------- process_frame: pool growth (:340-366)
@torch.no_grad()
def append_frame(mapper, coord, sdf_label, normal_label, sem_label, color_label, weight, cur_pose, frame_id) -> None:
    """utils/mapper.py:340-366: appends one frame's samples to every pool tensor in ONE launch (`global_coord` =
    `cur_pose` applied to `coord`, `time` = `frame_id`, the others copied), in place behind the mapper's views.  No
    pool-sized copy unless the store has to grow; no host read.  A label that is None sets its pool to None, as the
    reference does; a label whose pool is None raises `TypeError`, as the reference's `torch.cat` does."""
    dev = mapper.global_coord_pool.device if isinstance(mapper.global_coord_pool, torch.Tensor) else coord.device
    m = int(coord.shape[0])
    _rows_f32(coord, m, (3,), dev, "coord")
    _rows_f32(sdf_label, m, (), dev, "sdf_label")
    _rows_f32(weight, m, (), dev, "weight")
    if normal_label is not None:
        _rows_f32(normal_label, m, (3,), dev, "normal_label")
    Cc = 0
    if color_label is not None:
        Cc = int(color_label.shape[1]) if color_label.dim() == 2 else 0
        if not 1 <= Cc <= 4:
            raise _lib.PingsHipError("pool_ops: color_label must be [m, C] with 1 <= C <= 4")
        _rows_f32(color_label, m, (Cc,), dev, "color_label")
    if sem_label is not None:
        if not (isinstance(sem_label, torch.Tensor) and sem_label.device == dev and tuple(sem_label.shape) == (m,)
                and not sem_label.is_floating_point()):
            raise _lib.PingsHipError(f"pool_ops: sem_label must be an integer tensor of shape {(m,)} on {dev}")
        sem_label = sem_label.detach().to(torch.int32).contiguous()
    pose = _pose_dev(cur_pose, dev)
    store = pool_store(mapper)
    store.adopt(mapper, room=m)
    for name, t in zip(_OPTIONAL, (sem_label, color_label, normal_label)):
        if t is None:
            store.drop(name)
        elif name not in store.front:
            raise TypeError(f"pool_ops: mapper.{name} is None and this frame has a tensor for it")
        elif store.front[name].dtype is not t.dtype or tuple(store.front[name].shape[1:]) != tuple(t.shape[1:]):
            raise _lib.PingsHipError(f"pool_ops: mapper.{name} holds rows of another dtype or width than this frame's")
    for name, dt in zip(POOL_NAMES[:4], (torch.float32, torch.float32, torch.float32, torch.int32)):
        if store.front[name].dtype is not dt:
            raise _lib.PingsHipError(f"pool_ops: mapper.{name} must be {dt}")
    n = store.rows
    store.reserve(n + m)
    f = store.front
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    a = _abi.PoolAppendArgs(
        n, m, store.capacity, int(frame_id), Cc, int(pose.dtype is torch.float64), 0, pose.data_ptr(),
        p(coord), p(sdf_label), p(weight), p(sem_label), p(color_label), p(normal_label),
        p(f["global_coord_pool"]), p(f["sdf_label_pool"]), p(f["weight_pool"]), p(f["time_pool"]),
        p(f.get("sem_label_pool")), p(f.get("color_pool")), p(f.get("normal_label_pool")))
    fn = _entry("pings_pool_append")
    with _guard(dev):
        st = fn(C.byref(a), _lib.stream_ptr(dev))
    _lib.check(st, "pings_pool_append")
    store.rows = n + m
    store.publish(mapper)


# ---------------------------------------------------------------- process_frame: capacity filter (:386-423)
def last_filter_status(device=None) -> int:
    """The status word of `filter_pool` on `device` (default: the current one), read and cleared: bit 0 is set when a
    discard draw was outside the pool (it was skipped).  One host read, made only when asked for."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    w = _filter_words.get(dev)
    if w is None:
        return 0
    _lib.note_sync("pool_status")
    v = int(w.item())
    if v:
        w.zero_()
    return v


@torch.no_grad()
def filter_pool(mapper, _draws=None) -> None:
    """utils/mapper.py:386-423: with more than `config.pool_capacity` rows, `torch.randint(0, rows, (rows - capacity,))`
    (the reference's call, at the same point: under one seed the generator ends where the reference leaves it) marks
    rows of a byte mask, and every pool tensor is compacted by it in one stable pass into the store's back set, which
    then becomes the front.  Sets `cur_sample_count` (kept rows among the last `cur_sample_count`) and
    `pool_sample_count` from the call's one host read.  Duplicates in the draw are the reference's: fewer rows go than
    were drawn.  At or under the capacity nothing is drawn, moved or read: the reference's masks are all ones there.
    `_draws` (tests) supplies the draw.  Memory across the call: a byte per row, the draw and 16 B per 2048 rows."""
    store = pool_store(mapper)
    store.adopt(mapper)
    n, dev = store.rows, store.device
    cur = int(mapper.cur_sample_count)
    tail = n if cur <= 0 or cur > n else cur            # `filter_mask[-cur:]`: -0 and an over-long slice take every row
    capacity = int(mapper.config.pool_capacity)
    if n <= capacity:
        mapper.cur_sample_count, mapper.pool_sample_count = tail, n
        return
    discard_count = n - capacity
    r = torch.randint(0, n, (discard_count,), device=mapper.device) if _draws is None else _draws
    r = _i64(r)
    if r.device != dev or tuple(r.shape) != (discard_count,):
        raise _lib.PingsHipError(f"pool_ops.filter_pool: the draw must hold {discard_count} indices on {dev}")
    keep = torch.ones(n, dtype=torch.uint8, device=dev)
    with _guard(dev):
        word = _filter_words.get(dev)
        if word is None:
            word = _filter_words[dev] = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(_entry("pings_pool_discard_mark")(r.data_ptr(), discard_count, n, keep.data_ptr(), word.data_ptr(),
                                                     _lib.stream_ptr(dev)), "pings_pool_discard_mark")
    kept, kept_tail = _compact_by(store, keep, tail)
    store.publish(mapper)
    mapper.cur_sample_count = kept_tail
    mapper.pool_sample_count = kept


def _compact_by(store: PoolStore, keep: torch.Tensor, tail: int):
    """Compacts every tensor of the store's front set by the byte mask `keep` into the back set and swaps the sets:
    (kept rows, kept rows among the last `tail`), the call's one host read."""
    n, dev = store.rows, store.device
    if not (keep.dtype is torch.uint8 and keep.device == dev and tuple(keep.shape) == (n,) and keep.is_contiguous()):
        raise _lib.PingsHipError(f"pool_ops: the keep mask must hold {n} bytes on {dev}")
    store.reserve(store.capacity, back=True)
    counts = (C.c_int64 * 2)(0, 0)
    with _guard(dev):
        stream = _lib.stream_ptr(dev)
        scratch = torch.empty(_entry("pings_pool_compact_scratch_bytes")(n), dtype=torch.uint8, device=dev)
        _lib.note_sync("pool_filter_counts")
        _lib.check(_entry("pings_pool_compact_count")(keep.data_ptr(), n, tail, scratch.data_ptr(), counts, stream),
                   "pings_pool_compact_count")
        names = list(store.front)
        jobs = (_abi.GatherJob * len(names))()
        for g, name in enumerate(names):
            src, dst = store.front[name], store.back[name]
            row = src.element_size()
            for d in src.shape[1:]:
                row *= int(d)
            jobs[g] = _abi.GatherJob(src.data_ptr(), dst.data_ptr(), row, store.capacity)
        _lib.check(_entry("pings_pool_compact")(jobs, len(names), keep.data_ptr(), n, scratch.data_ptr(), stream),
                   "pings_pool_compact")
    store.swap()
    store.rows = int(counts[0])
    return int(counts[0]), int(counts[1])


# ---------------------------------------------------------------- process_frame: update points (:262-284)
@torch.no_grad()
def select_update(coord, sdf_label, color, normal, pose, thr=None):
    """(points, colours | None, normals | None) of the rows with `|sdf_label| < thr` in ascending order: the points
    moved by `pose`, the normals rotated by its rotation only (utils/mapper.py:270-284 without the three mask indexings
    and two `transform_torch` calls).  One host read (the count).  `thr=None` takes every row: one launch, no read."""
    dev = coord.device
    n = int(coord.shape[0])
    _rows_f32(coord, n, (3,), dev, "coord")
    Cc = 0
    if color is not None:
        Cc = int(color.shape[1]) if color.dim() == 2 else 0
        if not 1 <= Cc <= 4:
            raise _lib.PingsHipError("pool_ops: the colours must be [n, C] with 1 <= C <= 4")
        _rows_f32(color, n, (Cc,), dev, "color")
    if normal is not None:
        _rows_f32(normal, n, (3,), dev, "normal")
    pose = _pose_dev(pose, dev)
    scratch, k = None, n
    with _guard(dev):
        stream = _lib.stream_ptr(dev)
        if thr is not None:
            _rows_f32(sdf_label, n, (), dev, "sdf_label")
            scratch = torch.empty(_entry("pings_pool_select_scratch_bytes")(n), dtype=torch.uint8, device=dev)
            count = C.c_int64(0)
            _lib.note_sync("pool_update_rows")
            _lib.check(_entry("pings_pool_select_count")(sdf_label.data_ptr() if n else None, n, float(thr),
                                                         scratch.data_ptr(), C.byref(count), stream),
                       "pings_pool_select_count")
            k = int(count.value)
        points = torch.empty(k, 3, dtype=torch.float32, device=dev)
        o_color = None if color is None else torch.empty(k, Cc, dtype=torch.float32, device=dev)
        o_normal = None if normal is None else torch.empty(k, 3, dtype=torch.float32, device=dev)
        if k:
            p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
            a = _abi.PoolSelectArgs(n, k, Cc, int(pose.dtype is torch.float64), int(thr is None), 0,
                                    0.0 if thr is None else float(thr), pose.data_ptr(), coord.data_ptr(),
                                    None if thr is None else sdf_label.data_ptr(), p(color), p(normal), p(scratch),
                                    points.data_ptr(), p(o_color), p(o_normal))
            _lib.check(_entry("pings_pool_select_update")(C.byref(a), stream), "pings_pool_select_update")
    return points, o_color, o_normal


# ---------------------------------------------------------------- process_frame: mono-depth points (:297-331)
@torch.no_grad()
def _mono_update(self, mono, update_points, cur_pose_torch, frame_id: int) -> None:
    """The mono-depth branch of `Mapper.process_frame` (utils/mapper.py:297-331) without normals.  `mono`'s xyz columns
    are moved by the pose in place, as the reference leaves the caller's tensor (`select_update`, one launch).  The
    rows above the 0.98 quantile (`mono_depth_for_high_z`) or below the 0.2 quantile of the update points' z plus
    `voxel_size_m` (a device scalar, one compare launch) become a row list with one host read; one gather, then
    `neural_map.voxel_down_sample` at `monodepth_gaussian_res` and `neural_points.update(..., is_reliable=True)`,
    which is skipped when no row is left."""
    from . import neural_map

    cfg, dev = self.config, mono.device
    if int(mono.shape[0]) == 0:
        return
    mono[:, :3] = select_update(mono[:, :3].contiguous(), None, None, None, cur_pose_torch)[0]
    z = update_points[:, 2]
    if self.dataset.loader.mono_depth_for_high_z:
        used = mono[:, 2] > torch.quantile(z, 0.98) + cfg.voxel_size_m
    else:
        used = mono[:, 2] < torch.quantile(z, 0.2) + cfg.voxel_size_m
    with _guard(dev):
        rows, k, _ = neural_map._mask_rows(_lib.lib(), used)
        if k == 0:
            return
        kept = neural_map._gather_many(_lib.lib(), [(mono, k)], rows)[0]
        idx = neural_map.voxel_down_sample(kept[:, :3], cfg.monodepth_gaussian_res)
        kept = neural_map._gather_many(_lib.lib(), [(kept, int(idx.shape[0]))], idx)[0]
    self.neural_points.update(kept[:, :3], kept[:, 3:], None, cur_pose_torch[:3, 3], cur_pose_torch[:3, :3], frame_id,
                              is_reliable=True)


# ---------------------------------------------------------------- Mapper.process_frame
def _frame_on_device(self, point_cloud_torch, frame_label_torch, frame_normal_torch, cur_pose_torch) -> bool:
    pc = point_cloud_torch
    if not (_f32_dev(pc) and pc.dim() == 2 and pc.shape[1] >= 3 and isinstance(cur_pose_torch, torch.Tensor)
            and tuple(cur_pose_torch.shape) == (4, 4)):
        return False
    dev = pc.device
    if frame_normal_torch is not None and not (_f32_dev(frame_normal_torch, dev)
                                               and tuple(frame_normal_torch.shape) == (int(pc.shape[0]), 3)):
        return False
    if frame_label_torch is not None and not (isinstance(frame_label_torch, torch.Tensor)
                                              and frame_label_torch.device == dev and frame_label_torch.is_contiguous()
                                              and tuple(frame_label_torch.shape) == (int(pc.shape[0]),)):
        return False
    for name, dt in zip(POOL_NAMES, (torch.float32, torch.float32, torch.float32, torch.int32, torch.int32,
                                     torch.float32, torch.float32)):
        t = getattr(self, name, None)
        if t is not None and not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype is dt
                                  and t.is_contiguous()):
            return False
    return isinstance(self.global_coord_pool, torch.Tensor)


def process_frame(self, point_cloud_torch, frame_label_torch, frame_normal_torch, cur_pose_torch, frame_id: int,
                  filter_dynamic: bool = False, mono_depth_point_cloud_torch=None,
                  mono_depth_point_normals_torch=None):
    """`Mapper.process_frame` (utils/mapper.py:170-526) with the reference's signature and side effects, composed of
    this package's kernels: `reset_local_map` / `dynamic_filter` as bound on the class, one row list for the static
    points, `self.sampler.sample`, `select_update`, `self.neural_points.update`, `append_frame`, `filter_pool` on filter
    frames, `window_rows` and `frame_ops.new_samples`.  Host reads of its own, outside `reset_local_map`,
    `dynamic_filter` and `update`: at most one each for the static rows, the update rows, the filter counts, the window
    and the new samples.

    Departures: `local_sample_indices` is always 1-D (`window_rows`), and the window is tested in float32 against the
    pose's translation rounded to float32 (the reference promotes to the pose's dtype).

    With `config.monodepth_on` and a mono-depth cloud (a float32 [M, 3 + color_channel] device tensor, as
    `camfront_ops.mono_frame` leaves it) the branch of :297-331 follows the main `update`: `_mono_update`.

    CPU or non-float32 tensors, a non-contiguous pool, a mono-depth cloud on the CPU or of another dtype and mono-depth
    normals take the class's original method."""
    cfg = self.config
    mono = mono_depth_point_cloud_torch if (mono_depth_point_cloud_torch is not None and cfg.monodepth_on) else None
    mono_ok = mono is None or (mono_depth_point_normals_torch is None and _f32_dev(mono) and mono.dim() == 2
                               and int(mono.shape[1]) == 3 + int(cfg.color_channel)
                               and isinstance(point_cloud_torch, torch.Tensor)
                               and mono.device == point_cloud_torch.device)
    if not mono_ok or not _frame_on_device(self, point_cloud_torch, frame_label_torch, frame_normal_torch,
                                           cur_pose_torch):
        return _original(self, "process_frame")(self, point_cloud_torch, frame_label_torch, frame_normal_torch,
                                                cur_pose_torch, frame_id, filter_dynamic,
                                                mono_depth_point_cloud_torch, mono_depth_point_normals_torch)
    from . import frame_ops, neural_map                 # both import this module

    dev = point_cloud_torch.device
    N = int(point_cloud_torch.shape[0])
    frame_origin_torch = cur_pose_torch[:3, 3]
    frame_orientation_torch = cur_pose_torch[:3, :3]
    frame_point_torch = point_cloud_torch[:, :3]
    frame_color_torch = point_cloud_torch[:, 3:] if cfg.color_channel > 0 else None

    # dynamic filtering (:199-229)
    self.static_mask = torch.ones(N, dtype=torch.bool, device=cfg.device)
    if filter_dynamic:
        self.neural_points.reset_local_map(frame_origin_torch, frame_orientation_torch, frame_id)
        frame_point_torch_global = select_update(frame_point_torch.contiguous(), None, None, None, cur_pose_torch)[0]
        self.static_mask = self.dynamic_filter(frame_point_torch_global)
        with torch.no_grad(), _guard(dev):
            rows, k, _ = neural_map._mask_rows(_lib.lib(), self.static_mask)      # the one read for all frame tensors
            if not self.silence:
                print("# Dynamic points filtered: ", N - k)
            pairs = [(point_cloud_torch, k)]
            if frame_label_torch is not None:
                pairs.append((frame_label_torch, k))
            if frame_normal_torch is not None:
                pairs.append((frame_normal_torch, k))
            got = iter(neural_map._gather_many(_lib.lib(), pairs, rows))
        kept = next(got)
        frame_point_torch = kept[:, :3]
        if frame_color_torch is not None:
            frame_color_torch = kept[:, 3:]
        if frame_label_torch is not None:
            frame_label_torch = next(got)
        if frame_normal_torch is not None:
            frame_normal_torch = next(got)
    self.dataset.static_mask = self.static_mask

    # sampling data for training (:234-254)
    coord, sdf_label, normal_label, sem_label, color_label, weight = self.sampler.sample(
        frame_point_torch, frame_normal_torch, frame_label_torch, frame_color_torch)
    self.sdf_train_frame_count += 1
    self.cur_sample_count = sdf_label.shape[0]
    self.pool_sample_count = self.sdf_label_pool.shape[0]

    # update the neural point map (:258-294)
    if cfg.from_sample_points:
        thr = None if cfg.from_all_samples else cfg.surface_sample_range_m * cfg.map_surface_ratio
        update_points, update_colors, update_normals = select_update(
            coord.contiguous(), sdf_label, None if frame_color_torch is None else color_label,
            None if frame_normal_torch is None else normal_label, cur_pose_torch, thr)
    else:
        update_points, update_colors, update_normals = select_update(
            frame_point_torch.contiguous(), None, None if frame_color_torch is None else frame_color_torch.contiguous(),
            frame_normal_torch, cur_pose_torch)
    if cfg.prune_map_on and ((frame_id + 1) % cfg.prune_freq_frame == 0):
        if self.neural_points.prune_map(cfg.max_prune_certainty):
            self.neural_points.recreate_hash(None, None, True, True, frame_id)
    self.neural_points.update(update_points, update_colors, update_normals, frame_origin_torch,
                              frame_orientation_torch, frame_id)
    if mono is not None:
        _mono_update(self, mono, update_points, cur_pose_torch, frame_id)
    self.neural_points.record_memory(verbose=(not self.silence), record_footprint=True)

    # the data pool (:340-426)
    append_frame(self, coord.contiguous(), sdf_label, normal_label, sem_label, color_label, weight, cur_pose_torch,
                 frame_id)
    if (frame_id + 1) % cfg.pool_filter_freq == 0:
        filter_pool(self)
    else:
        self.cur_sample_count = coord.shape[0]
        self.pool_sample_count = self.global_coord_pool.shape[0]

    # the sample window (:429-443)
    self.local_sample_indices = window_rows(self.global_coord_pool, frame_origin_torch.to(torch.float32),
                                            cfg.window_radius, cfg.range_filter_2d)
    if not self.silence:
        print("# Total sample in pool: ", self.pool_sample_count)
        print("# Current sample      : ", self.cur_sample_count)
        print("# Local sample        : ", self.local_sample_indices.shape[0])

    # the newly observed region (:447-513)
    if cfg.bs_new_sample > 0:
        frame_ops.new_samples(self, frame_id)


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


def install(sampler_cls=None, mapper_cls=None, frame: bool = False) -> None:
    """`from utils.data_sampler import DataSampler; from utils.mapper import Mapper; install(DataSampler, Mapper)`:
    rebinds `DataSampler.sample`, `Mapper.get_batch` and `Mapper.transform_data_pool`; with `frame=True` also
    `Mapper.process_frame`, which then calls `window_rows` and `frame_ops.new_samples` for the user.  The originals are
    kept on the classes for the fallbacks and for `uninstall`.  Installing twice changes nothing."""
    if sampler_cls is not None:
        _rebind(sampler_cls, "sample", sample)
    if mapper_cls is not None:
        _rebind(mapper_cls, "get_batch", get_batch)
        _rebind(mapper_cls, "transform_data_pool", transform_data_pool)
        if frame:
            _rebind(mapper_cls, "process_frame", process_frame)


def uninstall(sampler_cls=None, mapper_cls=None) -> None:
    """Puts the reference's own methods back wherever `install` replaced them."""
    if sampler_cls is not None:
        _restore(sampler_cls, "sample", sample)
    if mapper_cls is not None:
        _restore(mapper_cls, "get_batch", get_batch)
        _restore(mapper_cls, "transform_data_pool", transform_data_pool)
        _restore(mapper_cls, "process_frame", process_frame)
