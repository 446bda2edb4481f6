"""The mapper's per-frame point tests on the HIP device (csrc/frame.hip).

One free function and three drop-in methods on the reference's own tensors; no pool or map state lives here:

  `new_samples`                   the new-sample test of `process_frame` (utils/mapper.py:447-513): count, one read, emit
  `dynamic_filter`                `Mapper.dynamic_filter` (:528-566): one fused query and one mask launch, no read
  `dynamic_filter_neural_points`  `Mapper.dynamic_filter_neural_points` (:568-585): the same on the local points
  `check_invalid_neural_points`   `Mapper.check_invalid_neural_points` (:1636-1655): one read (the stable count)

`install` rebinds the three methods and keeps the originals, which the methods call for the inputs the kernels do not
take (CPU tensors, a decoder outside `neural_points.fused_supported`, non-float32 tensors).  There is no torch path of
this module's own: with no original kept, such a call raises.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _abi, _lib, neural_map, neural_points
from .pool_ops import _entry, _f32_dev, _guard, _rebind, _restore

_dynamic_counts: dict = {}     # device -> int64 0-dim: zeros of the last static mask (pings_frame_static_mask)


def _original(self, name: str):
    orig = getattr(type(self), f"_pings_{name}_original", None)
    if orig is None:
        raise _lib.PingsHipError(f"frame_ops.{name}: these inputs take the reference's own method, and none was kept "
                                 "(`frame_ops.install` keeps it); the HIP path needs contiguous float32 device tensors "
                                 "and a decoder the fused SDF query covers")
    return orig


def _mask_dev(t, dev) -> bool:
    return (isinstance(t, torch.Tensor) and t.device == dev and t.dtype in (torch.bool, torch.uint8) and t.dim() == 1
            and t.is_contiguous())


def _u8(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.uint8) if t.dtype is torch.bool else t


# ---------------------------------------------------------------- the new-sample test of process_frame
@torch.no_grad()
def new_sample_rows(npm, coord: torch.Tensor, sdf_label: torch.Tensor, new_certainty_thre: float,
                    surface_sample_range_m: float, pool_offset: int = 0) -> torch.Tensor:
    """Ascending int64 rows r (+ `pool_offset`) of `coord` [n,3] / `sdf_label` [n] whose own cell of the map holds no
    point of certainty >= `new_certainty_thre` and with |sdf_label| < 3 * surface_sample_range_m: utils/mapper.py:451-492
    without the neighbourhood toggle.  The one-cell `max_valid_dist2` is an argument of the kernel: `neighbor_dx`,
    `neighbor_K` and `max_valid_dist2` of the map are neither written nor read.  One host read (the count)."""
    dev = coord.device
    n = int(coord.shape[0])
    if not (_f32_dev(coord) and coord.dim() == 2 and coord.shape[1] == 3 and _f32_dev(sdf_label, dev)
            and sdf_label.dim() == 1 and int(sdf_label.shape[0]) == n):
        raise _lib.PingsHipError("frame_ops.new_sample_rows: coord [n,3] and sdf_label [n] must be contiguous float32 "
                                 "tensors on one HIP device")
    table, pts, certs = npm.buffer_pt_index, npm.neural_points, npm.point_certainties
    if not (isinstance(table, torch.Tensor) and table.device == dev and table.dtype is torch.int64
            and _f32_dev(pts.contiguous(), dev) and _f32_dev(certs.contiguous(), dev)):
        raise _lib.PingsHipError("frame_ops.new_sample_rows: the map's table (int64), points and certainties (float32) "
                                 f"must be on {dev}")
    table, pts, certs = table.contiguous(), pts.contiguous(), certs.contiguous()
    res = float(npm.resolution)
    m = _abi.KnnMap(table.data_ptr(), int(table.shape[0]), pts.data_ptr() if pts.numel() else None, None, None, 0, 0,
                    0.0, None, None, 0, 0, None, None, 1, 1, res, 0.0, None, 0, None, None, None, 0)
    count = C.c_int64(0)
    with _guard(dev):
        scratch = torch.empty(_entry("pings_frame_new_scratch_bytes")(n), dtype=torch.uint8, device=dev)
        _lib.note_sync("frame_new_samples")
        _lib.check(_entry("pings_frame_new_count")(
            C.byref(m), certs.data_ptr() if certs.numel() else None, int(pts.shape[0]),
            coord.data_ptr() if n else None, sdf_label.data_ptr() if n else None, n,
            3 * ((1 + 1) * res) ** 2,                              # set_search_neighborhood(1, 0.0), :1058
            float(new_certainty_thre), float(surface_sample_range_m) * 3.0, scratch.data_ptr(), C.byref(count),
            _lib.stream_ptr(dev)), "pings_frame_new_count")
        k = int(count.value)
        rows = torch.empty(k, dtype=torch.int64, device=dev)
        if k:
            _lib.check(_entry("pings_frame_new_rows")(scratch.data_ptr(), n, int(pool_offset), rows.data_ptr(), k,
                                                      _lib.stream_ptr(dev)), "pings_frame_new_rows")
    return rows


def new_samples(mapper, frame_id=None) -> None:
    """The block `if self.config.bs_new_sample > 0:` of `process_frame` (utils/mapper.py:447-513) on the mapper's own
    tensors: sets `mapper.new_idx` (int64, ascending, rows of the pool), `mapper.new_obs_ratio` and
    `mapper.adaptive_iter_offset` with the reference's branches as written.  `frame_id` is `process_frame`'s argument
    (default: `mapper.dataset.processed_frame`); only the restart branch reads it.  `cur_sample_count == 0` raises
    `ZeroDivisionError` before any launch, as :500 does after its launches.  2 library calls and 1 host read; the map's
    `neighbor_dx`, `neighbor_K` and `max_valid_dist2` stay as they are (same objects)."""
    cfg = mapper.config
    if not cfg.bs_new_sample > 0:
        return
    cur = int(mapper.cur_sample_count)
    if cur == 0:
        raise ZeroDivisionError("division by zero")        # new_sample_count / self.cur_sample_count (:500)
    pool, label = mapper.global_coord_pool, mapper.sdf_label_pool
    if not (_f32_dev(pool) and _f32_dev(label, pool.device)):
        raise _lib.PingsHipError("frame_ops.new_samples: global_coord_pool and sdf_label_pool must be contiguous float32 "
                                 "tensors on one HIP device (there is no torch path)")
    offset = int(mapper.pool_sample_count) - cur
    mapper.new_idx = new_sample_rows(mapper.neural_points, pool[-cur:], label[-cur:], cfg.new_certainty_thre,
                                     cfg.surface_sample_range_m, offset)
    new_sample_count = int(mapper.new_idx.shape[0])
    mapper.adaptive_iter_offset = 0
    mapper.new_obs_ratio = new_sample_count / mapper.cur_sample_count
    if cfg.adaptive_iters:
        if mapper.new_obs_ratio < cfg.new_sample_ratio_less:
            mapper.adaptive_iter_offset = -5
        elif mapper.new_obs_ratio > cfg.new_sample_ratio_more:
            mapper.adaptive_iter_offset = 5
            if frame_id is None:
                frame_id = mapper.dataset.processed_frame
            if frame_id > cfg.freeze_after_frame and mapper.new_obs_ratio > cfg.new_sample_ratio_restart:
                mapper.adaptive_iter_offset = 10


# ---------------------------------------------------------------- Mapper.dynamic_filter[_neural_points]
def last_dynamic_count(device=None) -> torch.Tensor:
    """Number of dynamic points (zeros) of the last static mask formed on `device` (default: the current one): an
    int64 0-dim tensor ON the device, never read here."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    w = _dynamic_counts.get(dev)
    if w is None:
        w = _dynamic_counts[dev] = torch.zeros((), dtype=torch.int64, device=dev)
    return w


def _fused_ok(self, pts) -> bool:
    npm = self.neural_points
    return (_f32_dev(pts.detach().contiguous() if isinstance(pts, torch.Tensor) else None) and pts.dim() == 2
            and pts.shape[1] == 3 and npm.neural_points.device == pts.device
            and neural_points.fused_supported(npm, self.sdf_mlp))


@torch.no_grad()
def _static_mask(self, pts: torch.Tensor, type_2_on: bool) -> torch.Tensor:
    cfg = self.config
    dev = pts.device
    sdf, grad, _, cert = neural_points.sdf_fused(self.neural_points, self.sdf_mlp, pts, need_grad=type_2_on,
                                                 need_certainty=True)
    n = int(sdf.shape[0])
    mask = torch.empty(n, dtype=torch.bool, device=dev)
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
    with _guard(dev):
        word = last_dynamic_count(dev)
        _lib.check(_entry("pings_frame_static_mask")(
            ptr(sdf), ptr(cert), ptr(grad), n, float(cfg.dynamic_certainty_thre),
            cfg.dynamic_sdf_ratio_thre * cfg.voxel_size_m, float(cfg.dynamic_min_grad_norm_thre) if type_2_on else 0.0,
            ptr(_u8(mask)), word.data_ptr(), _lib.stream_ptr(dev)), "pings_frame_static_mask")
    return mask


def dynamic_filter(self, points_torch, type_2_on: bool = True):
    """`Mapper.dynamic_filter`: the bool mask of the static points.  One `sdf_fused` launch (value, analytic gradient
    when `type_2_on`, certainty) and one mask launch; nothing is read back, the number of dynamic points stays on the
    device as `last_dynamic_count()`.  `points_torch.requires_grad_(True)` is kept as the side effect of `type_2_on`.
    CPU or non-float32 points and a decoder outside `neural_points.fused_supported` take the class's original method."""
    if not _fused_ok(self, points_torch):
        return _original(self, "dynamic_filter")(self, points_torch, type_2_on)
    if type_2_on:
        points_torch.requires_grad_(True)
    return _static_mask(self, points_torch.detach().contiguous(), bool(type_2_on))


def dynamic_filter_neural_points(self):
    """`Mapper.dynamic_filter_neural_points`: strategy 1 on the local neural points, as `dynamic_filter` without the
    gradient."""
    pts = self.neural_points.local_neural_points
    if not _fused_ok(self, pts):
        return _original(self, "dynamic_filter_neural_points")(self)
    return _static_mask(self, pts.detach().contiguous(), False)


# ---------------------------------------------------------------- Mapper.check_invalid_neural_points
@torch.no_grad()
def check_invalid_neural_points(self, stability_threshold=1.0, render_min_nn_count: int = 6):
    """`Mapper.check_invalid_neural_points`: for the local points with certainty > `stability_threshold`,
    valid = |sdf| < dynamic_sdf_ratio_thre * voxel_size_m and nn_count >= `render_min_nn_count`, written to
    `local_valid_gs_mask` and, through the local -> global rows, to `valid_gs_mask`.  The stable rows come from
    `pings_mask_rows` (the call's one read), the query runs in chunks of `infer_bs` into arrays allocated once, and one
    launch writes both masks.  The reference then copies the whole local mask to the global one (:1655); every other
    local row already equals its global entry (`reset_local_map` gathered it from there), so only the stable rows are
    written.  `valid_gs_mask` is written through its raw pointer, so the map's generation is bumped as
    `neural_map.update` does: the search index is rebuilt before the next query.  No stable row: no launch, nothing
    written."""
    npm, cfg = self.neural_points, self.config
    pts, certs = npm.local_neural_points, npm.local_point_certainties
    lv, gv = npm.local_valid_gs_mask, npm.valid_gs_mask
    if not (isinstance(pts, torch.Tensor) and _f32_dev(pts.contiguous()) and _f32_dev(certs, pts.device)
            and _mask_dev(lv, pts.device) and _mask_dev(gv, pts.device) and int(lv.shape[0]) == int(pts.shape[0])
            and neural_points.fused_supported(npm, self.sdf_mlp)):
        return _original(self, "check_invalid_neural_points")(self, stability_threshold, render_min_nn_count)
    dev = pts.device
    L = _lib.lib()
    with _guard(dev):
        rows, k, _ = neural_map._mask_rows(L, certs > stability_threshold)
        if k == 0:
            return
        lidx = getattr(npm, "_local_idx", None)
        if lidx is None or int(lidx.shape[0]) != int(pts.shape[0]) + 1:   # local map set by other code
            _lib.note_sync("frame_local_rows")
            lidx = torch.nonzero(npm.local_mask).flatten()
        if lidx.dtype is not torch.int64 or int(lidx.shape[0]) < int(lv.shape[0]):
            raise _lib.PingsHipError("frame_ops.check_invalid_neural_points: the local map has fewer global rows "
                                     f"({int(lidx.shape[0])}) than local points ({int(lv.shape[0])})")
        stable = neural_map._gather(L, pts, rows, k)
        sdf = torch.empty(k, dtype=torch.float32, device=dev)
        cnt = torch.empty(k, dtype=torch.int64, device=dev)
        bs = max(int(cfg.infer_bs), 1)
        for head in range(0, k, bs):
            tail = min(head + bs, k)
            neural_points.sdf_fused(npm, self.sdf_mlp, stable[head:tail], out=(sdf[head:tail], cnt[head:tail]))
        _lib.check(_entry("pings_frame_valid_scatter")(
            rows.data_ptr(), k, sdf.data_ptr(), cnt.data_ptr(), cfg.dynamic_sdf_ratio_thre * cfg.voxel_size_m,
            int(render_min_nn_count), lidx.contiguous().data_ptr(), int(lv.shape[0]), int(gv.shape[0]),
            _u8(lv).data_ptr(), _u8(gv).data_ptr(), _lib.stream_ptr(dev)), "pings_frame_valid_scatter")
    npm._pings_table_gen = getattr(npm, "_pings_table_gen", 0) + 1


# ---------------------------------------------------------------- install
_METHODS = (("dynamic_filter", dynamic_filter), ("dynamic_filter_neural_points", dynamic_filter_neural_points),
            ("check_invalid_neural_points", check_invalid_neural_points))


def install(mapper_cls) -> None:
    """`from utils.mapper import Mapper; install(Mapper)`: rebinds `Mapper.dynamic_filter`,
    `Mapper.dynamic_filter_neural_points` and `Mapper.check_invalid_neural_points`.  The originals are kept on the class
    for the fallbacks and for `uninstall`.  Installing twice changes nothing."""
    for name, fn in _METHODS:
        _rebind(mapper_cls, name, fn)


def uninstall(mapper_cls) -> None:
    """Puts the reference's own methods back wherever `install` replaced them."""
    for name, fn in _METHODS:
        _restore(mapper_cls, name, fn)
