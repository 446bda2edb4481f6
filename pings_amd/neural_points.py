"""HIP-backed neural-point query path behind the reference's `NeuralPoints` interface.

Reference functions mirrored (model/neural_gaussians.py):
* `radius_neighborhood_search(points, time_filtering)` :1061-1115  -> `radius_neighborhood_topk`
  (the HIP kernel returns the nn_k nearest directly instead of the [B,K] candidate matrices)
* `query_feature(...)` :506-725 — same signature, same five return values, same side effects
  (certainty accumulation :664-689).  One HIP kernel forward (search + top-k + weights + gather), one
  backward (d/dx through neighbour vectors and weights; feature gradients by a deterministic row
  scatter-add) and one for the backward of the backward (`get_gradient(create_graph=True)`,
  utils/tools.py:409-419): `pings_query_feature_{forward,backward,double_backward}`.
* `Mapper.sdf` / `sdf_batch` (utils/mapper.py:2273-2318), tracker / mesher bulk queries
  -> `sdf_fused` (one kernel: search + gather + IDW + MLP [+ analytic gradient]).

The functions take the reference's own `NeuralPoints` object (duck-typed: only the attributes
it already has are read), so `NeuralPoints.query_feature = pings_amd.neural_points.query_feature`
is the whole integration.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _abi, _lib


def _nn_k(npm):
    return int(npm.config.query_nn_k) if hasattr(npm, "config") else int(npm.nn_k)


def _dx32(npm):
    """int32 copy of neighbor_dx on the device (cached on the object, rebuilt if it changes)."""
    dx = npm.neighbor_dx
    cache = getattr(npm, "_pings_dx32", None)
    if cache is None or cache[0] is not dx or cache[2] != dx._version:
        cache = (dx, dx.to(torch.int32).contiguous(), dx._version)
        npm._pings_dx32 = cache
    return cache[1]


USE_COMPACT_TABLE = True  # set False to read the reference's dense table directly (identical results)
# Which search-side layout the kernels read: "blocks" = the cell-block index (pings_knn_blocks_build; falls back to the
# table on the device if its exactness conditions do not hold), "table" = the reference's table / its compact mirror.
# All give identical results; PINGS_KNN_INDEX selects for A/B runs and the tests cover both.
KNN_INDEX = os.environ.get("PINGS_KNN_INDEX", "blocks")


def _max_abs_dx(npm) -> int:
    """max |neighbor_dx| as a host value (one read-back per neighbourhood tensor, cached on the object)."""
    dx = npm.neighbor_dx
    cache = getattr(npm, "_pings_dxmax", None)
    if cache is None or cache[0] is not dx or cache[2] != dx._version:
        _lib.note_sync("knn_neighbourhood_extent")
        cache = (dx, int(dx.abs().max().item()) if dx.numel() else 0, dx._version)
        npm._pings_dxmax = cache
    return cache[1]


class _BlockIndex:
    __slots__ = ("src", "versions", "scalars", "blocks", "records", "status", "mask", "baked", "args")


def _same_tensors(held, now) -> bool:
    return len(held) == len(now) and all(a is b for a, b in zip(held, now))


def _block_index(npm):
    """The cell-block index of the map's search-side tensors (csrc/knn_blocks.hip), rebuilt whenever any of them
    changes.  "Changes" = a different tensor OBJECT (the cache keeps the objects it was built from alive, so a new
    tensor cannot come back at an old address: `data_ptr()` alone is not an identity — a per-frame `global2local`
    re-created by the same op sequence has the same pointer, shape and version counter as last frame's), torch's
    in-place version counter, or the generation `neural_map.update` bumps after HIP kernels wrote through raw
    pointers."""
    table, pts = npm.buffer_pt_index, npm.neural_points
    N = int(pts.shape[0])
    opt = {n: getattr(npm, n, None) for n in ("point_ts_create", "travel_dist", "free_gs_mask", "valid_gs_mask",
                                              "global2local")}
    for n, t in list(opt.items()):
        if not torch.is_tensor(t) or not t.is_cuda:
            opt[n] = None
    ts, td = opt["point_ts_create"], opt["travel_dist"]
    if ts is None or td is None or ts.shape[0] < N or td.numel() == 0:
        ts = td = None
    free = opt["free_gs_mask"] if opt["free_gs_mask"] is not None and opt["free_gs_mask"].shape[0] >= N else None
    valid = opt["valid_gs_mask"] if opt["valid_gs_mask"] is not None and opt["valid_gs_mask"].shape[0] >= N else None
    g2l = opt["global2local"] if opt["global2local"] is not None and opt["global2local"].shape[0] >= N else None
    src = (table, pts, ts, td, free, valid, g2l, npm.neighbor_dx)
    versions = tuple(-1 if t is None else t._version for t in src)
    scalars = (getattr(npm, "_pings_table_gen", 0), float(npm.resolution), float(npm.max_valid_dist2), N)
    cache = getattr(npm, "_pings_blocks", None)
    if cache is not None and _same_tensors(cache.src, src) and cache.versions == versions and cache.scalars == scalars:
        return cache
    L = _lib.lib()
    dev = pts.device
    bi = _BlockIndex()
    bi.src, bi.versions, bi.scalars = src, versions, scalars
    bi.args = {}
    entries = L.pings_knn_blocks_entries(N)
    bi.blocks = torch.empty(entries * 4, dtype=torch.int64, device=dev)
    bi.records = torch.empty(max(N, 1) * 4, dtype=torch.int64, device=dev)
    bi.status = torch.empty(8, dtype=torch.int32, device=dev)
    bi.mask = entries - 1
    bi.baked = dict(ts=ts is not None, free=free is not None, valid=valid is not None, g2l=g2l is not None)
    keep = [table.contiguous(), pts.contiguous()]
    ts32 = ts.to(torch.int32).contiguous() if ts is not None else None
    td32 = td.to(torch.float32).contiguous() if td is not None else None
    fr8 = _as_u8(free) if free is not None else None
    va8 = _as_u8(valid) if valid is not None else None
    g2lc = g2l.to(torch.int64).contiguous() if g2l is not None else None
    keep += [ts32, td32, fr8, va8, g2lc]
    m = _abi.KnnMap(keep[0].data_ptr(), int(table.shape[0]), keep[1].data_ptr(), _lib.ptr(ts32), _lib.ptr(td32), 0, 0,
                    0.0, _lib.ptr(fr8), _lib.ptr(va8), 0, 0, _lib.ptr(g2lc), None, 0, 0, float(npm.resolution),
                    float(npm.max_valid_dist2), None, 0, None, None, None, 0)
    st = L.pings_knn_blocks_build(C.byref(m), N, int(td32.numel()) if td32 is not None else 0, _max_abs_dx(npm),
                                  bi.blocks.data_ptr(), entries, bi.records.data_ptr(), bi.status.data_ptr(),
                                  _lib.stream_ptr(dev))
    _lib.check(st, "pings_knn_blocks_build")
    npm._pings_blocks = bi
    return bi


def _compact_table(npm):
    """Cache-resident mirror of `buffer_pt_index`, rebuilt whenever the dense tensor changes: another tensor object
    (the cache keeps the one it was built from alive — see `_block_index`), torch's in-place version counter
    (torch-side writes), the explicit generation `neural_map.update` bumps after the HIP insert kernel wrote the table
    through its raw pointer (which torch's counter cannot see), and the point count."""
    table = npm.buffer_pt_index
    key = (table._version, table.shape[0], getattr(npm, "_pings_table_gen", 0), int(npm.neural_points.shape[0]))
    cache = getattr(npm, "_pings_compact", None)
    if cache is not None and cache[0] == key and cache[2] is table:
        return cache[1]
    L = _lib.lib()
    entries = L.pings_knn_compact_entries(int(npm.neural_points.shape[0]))
    comp = torch.empty(entries, 2, dtype=torch.int32, device=table.device)
    st = L.pings_knn_compact_build(_lib.ptr(table.contiguous()), int(table.shape[0]), _lib.ptr(comp), entries,
                                   _lib.stream_ptr(table.device))
    _lib.check(st, "pings_knn_compact_build")
    npm._pings_compact = (key, comp, table)
    return comp


def _as_u8(mask: torch.Tensor) -> torch.Tensor:
    return mask.contiguous().view(torch.uint8) if mask.dtype == torch.bool else mask.to(torch.uint8).contiguous()


class _MapArgs:
    """Builds the C struct and keeps every tensor it points to alive."""

    def __init__(self, npm, time_filtering: bool, use_free: bool, use_valid: bool, query_locally: bool,
                 index: bool = True):
        dev = npm.neural_points.device
        if not npm.neural_points.is_cuda:
            raise _lib.PingsHipError("the neural-point map must live on the HIP device (no CPU fallback)")
        self.keep = []

        def k(t):
            self.keep.append(t)
            return t.data_ptr()

        table = npm.buffer_pt_index
        if table.dtype != torch.int64:
            raise TypeError("buffer_pt_index must be int64 (neural_gaussians.py:46,86)")
        ts = npm.point_ts_create.to(torch.int32) if time_filtering else None
        td = npm.travel_dist.to(torch.float32).contiguous() if time_filtering else None
        free = _as_u8(npm.free_gs_mask) if use_free else None
        valid = _as_u8(npm.valid_gs_mask) if use_valid else None
        g2l = npm.global2local.contiguous() if query_locally else None
        dx = _dx32(npm)
        blk = None
        if index and KNN_INDEX == "blocks" and table.shape[0] < (1 << 31):
            blk = _block_index(npm)
            b = blk.baked
            if (time_filtering and not b["ts"]) or (use_free and not b["free"]) or (use_valid and not b["valid"]) or \
                    (query_locally and not b["g2l"]):
                blk = None
        comp = _compact_table(npm) if (index and USE_COMPACT_TABLE and blk is None) else None
        self.c = _abi.KnnMap(
            k(table.contiguous()), int(table.shape[0]), k(npm.neural_points.contiguous()),
            k(ts.contiguous()) if ts is not None else None, k(td) if td is not None else None,
            int(npm.cur_ts), int(bool(time_filtering)), float(npm.diff_travel_dist_local),
            k(free) if free is not None else None, k(valid) if valid is not None else None,
            int(use_free), int(use_valid), k(g2l) if g2l is not None else None, k(dx), int(dx.shape[0]),
            _nn_k(npm), float(npm.resolution), float(npm.max_valid_dist2),
            k(comp) if comp is not None else None, int(comp.shape[0] - 1) if comp is not None else 0,
            k(blk.blocks) if blk is not None else None, k(blk.records) if blk is not None else None,
            k(blk.status) if blk is not None else None, int(blk.mask) if blk is not None else 0)
        self.device = dev
        self.nn_k = _nn_k(npm)


def _map_args(npm, time_filtering: bool, use_free: bool, use_valid: bool, query_locally: bool) -> _MapArgs:
    """`_MapArgs` of a query, reused across calls: with the cell-block index in use, the index object has already been
    validated against every tensor the struct points to (identity + version counters), so the struct built for it stays
    valid until the index is rebuilt; only the per-call scalars join the key.  (~20 us of Python per query otherwise —
    at the reference's batch of 16,384 the training step is host-bound.)"""
    if KNN_INDEX == "blocks" and npm.neural_points.is_cuda and npm.buffer_pt_index.shape[0] < (1 << 31):
        blk = _block_index(npm)
        key = (bool(time_filtering), bool(use_free), bool(use_valid), bool(query_locally), int(npm.cur_ts),
               float(npm.diff_travel_dist_local), _nn_k(npm))
        a = blk.args.get(key)
        if a is None:
            a = blk.args[key] = _MapArgs(npm, time_filtering, use_free, use_valid, query_locally)
        return a
    return _MapArgs(npm, time_filtering, use_free, use_valid, query_locally)


def radius_neighborhood_topk(npm, points: torch.Tensor, time_filtering: bool = False,
                             use_only_measured_points: bool = False, use_only_valid_points: bool = False,
                             query_locally: bool = False, return_global: bool = False):
    """nn_k nearest valid neural points of every query: (idx[B,k] int64, d2[B,k], nn_counts[B] int64).

    Equivalent to `radius_neighborhood_search` (:1061-1115) followed by the masking, counting,
    sort and top-k of `query_feature` (:544-569)."""
    L = _lib.lib()
    pts = points.detach().to(torch.float32).contiguous()
    B = pts.shape[0]
    a = _map_args(npm, time_filtering, use_only_measured_points, use_only_valid_points, query_locally)
    idx = torch.empty(B, a.nn_k, dtype=torch.int64, device=pts.device)
    d2 = torch.empty(B, a.nn_k, dtype=torch.float32, device=pts.device)
    cnt = torch.empty(B, dtype=torch.int64, device=pts.device)
    gidx = torch.empty(B, a.nn_k, dtype=torch.int64, device=pts.device) if return_global else None
    st = L.pings_knn_search(C.byref(a.c), _lib.ptr(pts), B, _lib.ptr(idx), _lib.ptr(d2), _lib.ptr(cnt),
                            _lib.ptr(gidx), _lib.stream_ptr(pts.device))
    _lib.check(st, "pings_knn_search")
    if return_global:
        return idx, d2, cnt, gidx
    return idx, d2, cnt


def radius_neighborhood_search(self, points: torch.Tensor, time_filtering: bool = False):
    """`NeuralPoints.radius_neighborhood_search` (model/neural_gaussians.py:1061-1115) as it stands: (dist2[B,K] fp32,
    idx[B,K] int64, -1 = no point) for every candidate cell.  The query paths use the fused search
    (`radius_neighborhood_topk`); this is for the callers that want the raw pair — `query_certainty` (:1117-1133), which
    the mapper runs on every frame's new samples with the one-cell neighbourhood (utils/mapper.py:461-475).  Reads the
    reference's table directly (no search index is built for it: the neighbourhood changes around the call)."""
    L = _lib.lib()
    pts = points.detach().to(torch.float32).contiguous()
    B = int(pts.shape[0])
    a = _MapArgs(self, time_filtering, False, False, False, index=False)
    K = int(a.c.K)
    d2 = torch.empty(B, K, dtype=torch.float32, device=pts.device)
    idx = torch.empty(B, K, dtype=torch.int64, device=pts.device)
    _lib.check(L.pings_knn_cells(C.byref(a.c), _lib.ptr(pts), B, int(self.neural_points.shape[0]), _lib.ptr(d2),
                                 _lib.ptr(idx), _lib.stream_ptr(pts.device)), "pings_knn_cells")
    return d2, idx


def rows_scatter_add(dst_row: torch.Tensor, src: torch.Tensor, rows: int, w: torch.Tensor = None,
                     src_row: torch.Tensor = None, F: int = None) -> torch.Tensor:
    """out[r] = sum over pairs p with dst_row[p] == r (ascending p) of w[p] * src[src_row[p], :F]; [rows, F], bitwise
    reproducible (`pings_rows_scatter_add`: the backward of a row gather without float atomics)."""
    L = _lib.lib()
    if src.dim() == 2 and src.stride(1) == 1 and src.stride(0) >= src.shape[1] and src.is_cuda:
        src2, ld = src, int(src.stride(0))          # a column slice of a row-major table is read where it lies
    else:
        src2 = src.reshape(-1, src.shape[-1]).contiguous()
        ld = int(src2.shape[1])
    F = int(src2.shape[1] if F is None else F)
    dst = dst_row.reshape(-1).to(torch.int64).contiguous()
    n = dst.shape[0]
    out = torch.empty(rows, F, dtype=torch.float32, device=src.device)
    scratch = torch.empty(L.pings_rows_scatter_add_scratch_bytes(n, rows), dtype=torch.uint8, device=src.device)
    wv = w.reshape(-1).to(torch.float32).contiguous() if w is not None else None
    sr = src_row.reshape(-1).to(torch.int64).contiguous() if src_row is not None else None
    if not src2.is_cuda:
        raise _lib.PingsHipError("rows_scatter_add runs on the HIP device only (no CPU fallback)")
    _lib.check(L.pings_rows_scatter_add(_lib.ptr(dst), n, src2.data_ptr(), ld, F, _lib.ptr(wv),
                                        _lib.ptr(sr), rows, _lib.ptr(scratch), _lib.ptr(out),
                                        _lib.stream_ptr(src.device)), "pings_rows_scatter_add")
    return out


class _QfState:
    """What the backward kernels need besides the differentiable inputs (kept alive by the autograd graph)."""
    __slots__ = ("tables", "keep", "gpoints", "idx", "gidx", "nn_k", "rows", "B", "Fg", "Fc", "weighted_first",
                 "has_geo", "has_color", "geo_buf", "col_buf", "plan")


def _qf_tables(st: _QfState, geo: torch.Tensor, col: torch.Tensor) -> _abi.QfTables:
    """C struct for the CURRENT values of the feature tables (the double backward of weighted_first reads them)."""
    t = st.tables
    return _abi.QfTables(_lib.ptr(geo) if st.has_geo else None, _lib.ptr(col) if st.has_color else None,
                         st.Fg if st.has_geo else 0, st.Fc if st.has_color else 0, t["points"].data_ptr(),
                         t["quat"].data_ptr() if t["quat"] is not None else None,
                         t["cert"].data_ptr() if t["cert"] is not None else None, int(t["after_pgo"]),
                         int(st.weighted_first))


def _c32(t):
    return None if t is None else t.detach().to(torch.float32).contiguous()


def _qf_forward(x, geo_tab, col_tab, npm, opts, want_n: bool):
    """Launches `pings_query_feature_forward`; returns (state, geo, colour, w [B,k], n [B,k,3] | None, cnt, cert)."""
    L = _lib.lib()
    (query_ts, accumulate_stability, query_locally, query_geo, query_color, use_meas, use_valid) = opts[:7]
    dev = x.device
    q = _c32(x)
    B = q.shape[0]
    a = _map_args(npm, bool(npm.temporal_local_map_on and query_locally), use_meas, use_valid, query_locally)
    nn_k = a.nn_k
    cfg = getattr(npm, "config", None)
    wf = bool(cfg.weighted_first) if cfg is not None else bool(npm.weighted_first)
    if len(opts) > 7 and opts[7] is not None:       # layer_norm_on: rows are wanted per neighbour whatever the config says
        wf = bool(opts[7])
    pts = (npm.local_neural_points if query_locally else npm.neural_points).detach().contiguous()
    quat = (npm.local_point_orientations if query_locally else npm.point_orientations)
    quat = quat.detach().contiguous() if quat is not None else None
    cert_tab = npm.local_point_certainties if query_locally else npm.point_certainties
    has_geo = bool(query_geo) and geo_tab is not None
    has_col = bool(query_color) and col_tab is not None
    geo_c = _c32(geo_tab) if has_geo else None
    col_c = _c32(col_tab) if has_col else None
    st = _QfState()
    st.tables = {"points": pts, "quat": quat, "cert": cert_tab.detach() if cert_tab is not None else None,
                 "after_pgo": bool(npm.after_pgo)}
    st.gpoints = npm.neural_points.detach().contiguous()
    st.nn_k, st.B, st.weighted_first = nn_k, B, wf
    st.has_geo, st.has_color = has_geo, has_col
    st.Fg = int(geo_c.shape[1]) if has_geo else 0
    st.Fc = int(col_c.shape[1]) if has_col else 0
    st.rows = int((geo_c if has_geo else col_c).shape[0])
    st.plan = None
    if has_geo and has_col and geo_c.shape[0] != col_c.shape[0]:
        raise ValueError("query_feature: geo and colour feature tables must have the same number of rows")
    if cert_tab is not None and (not cert_tab.is_contiguous() or cert_tab.dtype != torch.float32):
        raise _lib.PingsHipError("query_feature: certainty table must be contiguous float32 (updated in place)")
    tabs = _qf_tables(st, geo_c, col_c)
    f32 = dict(dtype=torch.float32, device=dev)
    shape = (lambda F: (B, F + 3)) if wf else (lambda F: (B, nn_k, F + 3))
    geo = torch.empty(shape(st.Fg), **f32) if has_geo else None
    col = torch.empty(shape(st.Fc), **f32) if has_col else None
    w = torch.empty(B, nn_k, **f32)
    n = torch.empty(B, nn_k, 3, **f32) if want_n else None
    idx = torch.empty(B, nn_k, dtype=torch.int64, device=dev)
    gidx = torch.empty(B, nn_k, dtype=torch.int64, device=dev)
    cnt = torch.empty(B, dtype=torch.int64, device=dev)
    cert = torch.empty(B, **f32) if cert_tab is not None else None
    ts_tab = qts = None
    accumulate = bool(accumulate_stability and cert_tab is not None)       # :664-689, under no_grad in the reference
    if accumulate:
        if query_locally and query_ts is not None:
            ts_tab = npm.local_point_ts_update
            if ts_tab.dtype != torch.int32 or not ts_tab.is_contiguous():
                raise TypeError("local_point_ts_update must be a contiguous int32 tensor (neural_gaussians.py:138)")
            qts = query_ts.detach().to(torch.int32).contiguous()
    _lib.check(L.pings_query_feature_forward(
        C.byref(a.c), C.byref(tabs), _lib.ptr(q), B, _lib.ptr(geo), _lib.ptr(col), _lib.ptr(w), _lib.ptr(idx),
        _lib.ptr(gidx), _lib.ptr(cnt), _lib.ptr(cert), None, _lib.ptr(qts), _lib.ptr(ts_tab), _lib.ptr(n),
        _lib.stream_ptr(dev)), "pings_query_feature_forward")
    if accumulate and B > 0:
        # the queried certainty (:691-695) is computed from the values gathered BEFORE the accumulation (:615-620): the
        # increments go in as a second O(B k) launch behind the forward kernel, straight into the table
        _lib.check(L.pings_query_feature_accumulate(idx.data_ptr(), w.data_ptr(), B * nn_k, cert_tab.data_ptr(),
                                                    _lib.stream_ptr(dev)), "pings_query_feature_accumulate")
    st.idx, st.gidx = idx, gidx
    st.geo_buf, st.col_buf = geo, col
    st.keep = a      # the map tensors the C struct points at
    return st, geo, col, w, n, cnt, cert


# ---------------------------------------------------------------- weighted_first: one graph node
class _QfBackward(torch.autograd.Function):
    """The backward of `_QueryFeature` as a differentiable op of its own: (g_geo, g_color, g_w, x, geo table, colour
    table) -> (g_x, g_geo_table, g_color_table).  Its backward is `pings_query_feature_double_backward`."""

    @staticmethod
    def forward(ctx, g_geo, g_col, g_w, x, geo_tab, col_tab, st: _QfState, need_geo, need_col):
        L = _lib.lib()
        dev = x.device
        q = _c32(x)
        gg, gc, gw = _c32(g_geo), _c32(g_col), _c32(g_w)
        geo_c, col_c = _c32(geo_tab), _c32(col_tab)
        tabs = _qf_tables(st, geo_c, col_c)
        f32 = dict(dtype=torch.float32, device=dev)
        g_x = torch.empty(st.B, 3, **f32)
        g_gt = torch.empty(st.rows, st.Fg, **f32) if (need_geo and st.has_geo) else None
        g_ct = torch.empty(st.rows, st.Fc, **f32) if (need_col and st.has_color) else None
        scratch = None
        if g_gt is not None or g_ct is not None:
            scratch = torch.empty(L.pings_query_feature_scratch_bytes(st.B, st.nn_k, st.rows), dtype=torch.uint8, device=dev)
        _lib.check(L.pings_query_feature_backward(
            C.byref(tabs), _lib.ptr(st.gpoints), _lib.ptr(q), st.B, st.nn_k, _lib.ptr(st.idx), _lib.ptr(st.gidx),
            _lib.ptr(gg), _lib.ptr(gc), None, _lib.ptr(gw), st.rows, _lib.ptr(scratch), _lib.ptr(g_x), _lib.ptr(g_gt),
            _lib.ptr(g_ct), _lib.stream_ptr(dev)), "pings_query_feature_backward")
        ctx.st = st
        ctx.save_for_backward(gg, gc, gw, q, geo_c, col_c)
        ctx.set_materialize_grads(False)
        return g_x, g_gt, g_ct

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gg_x, gg_gt, gg_ct):
        L = _lib.lib()
        st = ctx.st
        gg, gc, gw, q, geo_c, col_c = ctx.saved_tensors
        dev = q.device
        tabs = _qf_tables(st, geo_c, col_c)
        f32 = dict(dtype=torch.float32, device=dev)
        wf = st.weighted_first
        d_gg = torch.empty_like(gg) if gg is not None else None
        d_gc = torch.empty_like(gc) if gc is not None else None
        d_gw = torch.empty(st.B, st.nn_k, **f32)
        need = ctx.needs_input_grad
        d_x = torch.empty(st.B, 3, **f32) if need[3] else None
        d_gt = torch.empty(st.rows, st.Fg, **f32) if (wf and need[4] and st.has_geo) else None
        d_ct = torch.empty(st.rows, st.Fc, **f32) if (wf and need[5] and st.has_color) else None
        scratch = None
        if d_gt is not None or d_ct is not None:
            scratch = torch.empty(L.pings_query_feature_scratch_bytes(st.B, st.nn_k, st.rows), dtype=torch.uint8, device=dev)
        _lib.check(L.pings_query_feature_double_backward(
            C.byref(tabs), _lib.ptr(st.gpoints), _lib.ptr(q), st.B, st.nn_k, _lib.ptr(st.idx), _lib.ptr(st.gidx),
            _lib.ptr(gg), _lib.ptr(gc), _lib.ptr(gw), _lib.ptr(_c32(gg_x)), _lib.ptr(_c32(gg_gt)), _lib.ptr(_c32(gg_ct)),
            st.rows, _lib.ptr(scratch), _lib.ptr(d_gg), _lib.ptr(d_gc), None, _lib.ptr(d_gw), _lib.ptr(d_x),
            _lib.ptr(d_gt), _lib.ptr(d_ct), _lib.stream_ptr(dev)), "pings_query_feature_double_backward")
        return d_gg, d_gc, (d_gw if gw is not None else None), d_x, d_gt, d_ct, None, None, None


class _QueryFeature(torch.autograd.Function):
    """weighted_first mode (:701-705): the outputs mix tables and geometry (sum_k w_k [f_k, n_k]), one graph node."""

    @staticmethod
    def forward(ctx, x, geo_tab, col_tab, npm, opts):
        st, geo, col, w, _, cnt, cert = _qf_forward(x, geo_tab, col_tab, npm, opts, want_n=False)
        ctx.st = st
        ctx.save_for_backward(x, geo_tab if st.has_geo else None, col_tab if st.has_color else None)
        ctx.mark_non_differentiable(cnt)
        if cert is not None:
            ctx.mark_non_differentiable(cert)
        ctx.set_materialize_grads(False)
        # aliases of the buffers the state keeps (st.geo_buf / st.col_buf): returning the state's own tensor objects
        # closes the cycle output -> grad_fn -> ctx -> st -> output, which only the cycle collector frees
        alias = lambda t: None if t is None else t.detach()
        return alias(geo), alias(col), w.unsqueeze(-1), cnt, cert

    @staticmethod
    def backward(ctx, g_geo, g_col, g_w, _g_cnt, _g_cert):
        x, geo_tab, col_tab = ctx.saved_tensors
        st = ctx.st
        need = ctx.needs_input_grad
        if g_w is not None:
            g_w = g_w.reshape(st.B, st.nn_k)
        g_x, g_gt, g_ct = _QfBackward.apply(g_geo, g_col, g_w, x, geo_tab, col_tab, st, bool(need[1]), bool(need[2]))
        return (g_x if need[0] else None), g_gt, g_ct, None, None


# ---------------------------------------------------------------- per-neighbour mode: table path and query path apart
# The outputs are [feature rows | neighbour vector] per (query, neighbour): the feature columns depend only on the
# tables, the vector and the weights only on the query.  Each gets its own graph node, so that
# `get_gradient(x, sdf)` (utils/tools.py:409-419) runs the cheap geometry backward alone and the table scatter only
# runs when a table gradient is actually asked for (autograd cannot tell a monolithic Function which inputs a
# particular backward call wants).  The forward kernel has already written both parts interleaved into one buffer;
# `_QfInterleave` hands that buffer out without a copy.
class _QfGeomBackward(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g_n, g_w, x, st: _QfState):
        L = _lib.lib()
        dev = x.device
        q = _c32(x)
        gn, gw = _c32(g_n), _c32(g_w)
        if gn is None:
            gn = torch.zeros(st.B, st.nn_k, 3, dtype=torch.float32, device=dev)
        tabs = _qf_tables(st, None, None) if False else _abi.QfTables(
            None, None, 0, 0, st.tables["points"].data_ptr(),
            st.tables["quat"].data_ptr() if st.tables["quat"] is not None else None, None,
            int(st.tables["after_pgo"]), 0)
        g_x = torch.empty(st.B, 3, dtype=torch.float32, device=dev)
        _lib.check(L.pings_query_feature_backward(
            C.byref(tabs), _lib.ptr(st.gpoints), _lib.ptr(q), st.B, st.nn_k, _lib.ptr(st.idx), _lib.ptr(st.gidx),
            None, None, _lib.ptr(gn), _lib.ptr(gw), st.rows, None, _lib.ptr(g_x), None, None, _lib.stream_ptr(dev)),
            "pings_query_feature_backward")
        ctx.st = st
        ctx.tabs_args = None
        ctx.save_for_backward(gn, gw, q)
        ctx.set_materialize_grads(False)
        return g_x

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gg_x):
        L = _lib.lib()
        st = ctx.st
        gn, gw, q = ctx.saved_tensors
        dev = q.device
        if gg_x is None:
            return None, None, None, None
        tabs = _abi.QfTables(None, None, 0, 0, st.tables["points"].data_ptr(),
                             st.tables["quat"].data_ptr() if st.tables["quat"] is not None else None, None,
                             int(st.tables["after_pgo"]), 0)
        f32 = dict(dtype=torch.float32, device=dev)
        d_gn = torch.empty(st.B, st.nn_k, 3, **f32)
        d_gw = torch.empty(st.B, st.nn_k, **f32)
        d_x = torch.empty(st.B, 3, **f32) if ctx.needs_input_grad[2] else None
        _lib.check(L.pings_query_feature_double_backward(
            C.byref(tabs), _lib.ptr(st.gpoints), _lib.ptr(q), st.B, st.nn_k, _lib.ptr(st.idx), _lib.ptr(st.gidx),
            None, None, _lib.ptr(gw), _lib.ptr(_c32(gg_x)), None, None, st.rows, None, None, None, _lib.ptr(d_gn),
            _lib.ptr(d_gw), _lib.ptr(d_x), None, None, _lib.stream_ptr(dev)), "pings_query_feature_double_backward")
        return d_gn, (d_gw if gw is not None else None), d_x, None


class _QfGeom(torch.autograd.Function):
    """x -> (neighbour vectors n [B,k,3], weights w [B,k,1], nn_counts, certainty); launches the forward kernel, which
    also fills the interleaved output buffers kept in the state."""

    @staticmethod
    def forward(ctx, x, geo_tab, col_tab, npm, opts, box):
        st, geo, col, w, n, cnt, cert = _qf_forward(x, geo_tab, col_tab, npm, opts, want_n=True)
        box.append(st)
        ctx.st = st
        ctx.save_for_backward(x)
        ctx.mark_non_differentiable(cnt)
        if cert is not None:
            ctx.mark_non_differentiable(cert)
        ctx.set_materialize_grads(False)
        return n, w.unsqueeze(-1), cnt, cert

    @staticmethod
    def backward(ctx, g_n, g_w, _g_cnt, _g_cert):
        (x,) = ctx.saved_tensors
        st = ctx.st
        if g_n is None and g_w is None:
            return None, None, None, None, None, None
        if g_w is not None:
            g_w = g_w.reshape(st.B, st.nn_k)
        return _QfGeomBackward.apply(g_n, g_w, x, st), None, None, None, None, None


class _QfTable(torch.autograd.Function):
    """feature table -> the feature columns of the interleaved output (a view of the buffer the forward kernel filled);
    backward: deterministic row scatter-add of the upstream rows (`pings_rows_plan_build` once per batch, `_apply`
    per table), reading the upstream gradient in place through its row stride."""

    @staticmethod
    def forward(ctx, tab, st: _QfState, which: int):
        ctx.st, ctx.which = st, which
        buf, F = (st.col_buf, st.Fc) if which else (st.geo_buf, st.Fg)
        return buf[..., :F]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if g is None:
            return None, None, None
        return _table_grad(ctx.st, ctx.which, g), None, None


def _table_grad(st: _QfState, which: int, g: torch.Tensor) -> torch.Tensor:
    """Deterministic row scatter-add of the upstream rows `g` ([B, k, F] or the first F columns of [B, k, F+3]) into a
    dense [rows, F] table gradient (`pings_rows_plan_build` once per batch, `_apply` per table)."""
    L = _lib.lib()
    F = st.Fc if which else st.Fg
    dev = g.device
    n_pairs = st.B * st.nn_k
    if st.plan is None:
        plan = torch.empty(L.pings_rows_plan_bytes(n_pairs, st.rows), dtype=torch.uint8, device=dev)
        _lib.check(L.pings_rows_plan_build(_lib.ptr(st.idx), n_pairs, st.rows, _lib.ptr(plan), _lib.stream_ptr(dev)),
                   "pings_rows_plan_build")
        st.plan = plan
    g = g.detach()
    if g.dtype != torch.float32:
        g = g.to(torch.float32)
    # usually a strided view [B, k, F] of the contiguous [B, k, F+3] upstream gradient: read it where it lies
    ld = g.stride(1) if g.dim() == 3 else 0
    if not (g.dim() == 3 and g.stride(2) == 1 and g.stride(0) == st.nn_k * ld and ld >= F):
        g = g.reshape(st.B, st.nn_k, -1)[..., :F].contiguous()
        ld = F
    out = torch.empty(st.rows, F, dtype=torch.float32, device=dev)
    _lib.check(L.pings_rows_plan_apply(_lib.ptr(st.plan), n_pairs, st.rows, g.data_ptr(), ld, F, None,
                                       _lib.ptr(out), _lib.stream_ptr(dev)), "pings_rows_plan_apply")
    return out


class _QfRows(torch.autograd.Function):
    """feature table -> the whole [B, k, F+3] rows in ONE node, for queries that carry no gradient themselves (the
    mapper's sample points, mapper.py:848-866): the neighbour-vector columns are constants then, so the
    _QfGeom / _QfTable / _QfInterleave split (which exists for d/dx) is two autograd nodes and ~40 us of Python too
    many per step at the reference's batch size."""

    @staticmethod
    def forward(ctx, tab, st: _QfState, which: int):
        ctx.st, ctx.which = st, which
        return (st.col_buf if which else st.geo_buf).detach()     # an alias: see _QueryFeature.forward

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if g is None:
            return None, None, None
        return _table_grad(ctx.st, ctx.which, g), None, None


class _QfInterleave(torch.autograd.Function):
    """(feature columns, neighbour vectors) -> the [B, k, F+3] rows: zero-copy, the forward kernel wrote them
    interleaved already; backward = the two column slices of the upstream gradient (views; differentiable)."""

    @staticmethod
    def forward(ctx, feat, n, buf):
        ctx.F = feat.shape[-1]
        return buf.detach()     # an alias: `buf` is the state's own tensor, and the state hangs off _QfGeom's ctx

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None
        return g[..., :ctx.F], g[..., ctx.F:], None


def query_feature(self, query_points: torch.Tensor, query_ts: torch.Tensor = None,
                  accumulate_stability: bool = True, query_locally: bool = True,
                  query_geo_feature: bool = True, query_color_feature: bool = False,
                  use_only_measured_points: bool = True, use_only_valid_points: bool = False):
    """Drop-in for `NeuralPoints.query_feature` (model/neural_gaussians.py:506-725): same arguments, same five
    return values (geo [B,k,Fg+3] | [B,Fg+3], colour, weights [B,k,1], nn_counts [B], certainty [B]), same side
    effects, differentiable twice w.r.t. the query, once w.r.t. the feature tables (twice in weighted_first mode)."""
    if not query_geo_feature and not query_color_feature:
        raise SystemExit("you need to at least query one kind of feature")  # :521-522
    if not query_points.is_cuda:
        raise _lib.PingsHipError("query_feature runs on the HIP device only (got a CPU tensor); there is no CPU "
                                 "fallback — the CPU restatement is oracle/sdf_cpu.py (tests only)")
    cfg = self.config
    layer_norm = bool(getattr(cfg, "layer_norm_on", False))
    feats = (self.local_geo_features if query_locally else self.geo_features) if query_geo_feature else None
    cfeats = (self.local_color_features if query_locally else self.color_features) if query_color_feature else None
    opts = (query_ts, bool(accumulate_stability), bool(query_locally), bool(query_geo_feature),
            bool(query_color_feature), bool(use_only_measured_points), bool(use_only_valid_points))
    if layer_norm:
        # config.layer_norm_on (utils/config.py:95; no shipped config sets it): `F.layer_norm` over the gathered feature
        # rows BEFORE the neighbour vector is appended and before the weighted sum (:591-592, :605-606, :701-710).  The
        # kernels deliver the per-neighbour rows; normalisation and, in weighted_first mode, the sum are the
        # reference's own torch operators on the device (not a fused path: an option no configuration uses).
        geo, col, w, cnt, cert = _query_feature_rows(self, query_points, feats, cfeats, opts + (False,))
        F_ = torch.nn.functional

        def norm(rows, dim):
            if rows is None:
                return None
            rows = torch.cat((F_.layer_norm(rows[..., :dim], [dim]), rows[..., dim:]), dim=-1)
            return torch.sum(rows * w, dim=1) if bool(cfg.weighted_first) else rows

        return (norm(geo, feats.shape[1] if feats is not None else 0),
                norm(col, cfeats.shape[1] if cfeats is not None else 0), w, cnt, cert)
    if bool(cfg.weighted_first):
        return _QueryFeature.apply(query_points, feats, cfeats, self, opts)
    return _query_feature_rows(self, query_points, feats, cfeats, opts)


def _query_feature_rows(self, query_points, feats, cfeats, opts):
    """Per-neighbour mode of `query_feature`: ([B,k,Fg+3], [B,k,Fc+3], w [B,k,1], nn_counts, certainty)."""
    if not (torch.is_grad_enabled() and query_points.requires_grad):
        # no gradient to the query: run the kernel outside autograd, one node per table that wants a gradient
        with torch.no_grad():
            st, _, _, w, _, cnt, cert = _qf_forward(query_points, feats, cfeats, self, opts, want_n=False)
        track = torch.is_grad_enabled()
        geo = col = None
        if st.has_geo:
            geo = _QfRows.apply(feats, st, 0) if (track and feats.requires_grad) else st.geo_buf
        if st.has_color:
            col = _QfRows.apply(cfeats, st, 1) if (track and cfeats.requires_grad) else st.col_buf
        return geo, col, w.unsqueeze(-1), cnt, cert
    box = []
    n, w, cnt, cert = _QfGeom.apply(query_points, feats.detach() if feats is not None else None,
                                    cfeats.detach() if cfeats is not None else None, self, opts, box)
    st = box[0]
    geo = _QfInterleave.apply(_QfTable.apply(feats, st, 0), n, st.geo_buf) if st.has_geo else None
    col = _QfInterleave.apply(_QfTable.apply(cfeats, st, 1), n, st.col_buf) if st.has_color else None
    return geo, col, w, cnt, cert


def fused_supported(npm, decoder) -> bool:
    """Whether the fused SDF kernels cover this (map, decoder) pair: one hidden level of at most 64 units, ReLU, biases,
    F <= 61, no layer norm — every shipped configuration (pings.py:147, utils/config.py:95,145-146).  Everything else
    runs `_sdf_composed`: the same result from `query_feature` + the decoder's own layers, on the device."""
    cfg = getattr(npm, "config", None)
    if cfg is not None and getattr(cfg, "layer_norm_on", False):
        return False
    layers = getattr(decoder, "layers", None)
    if layers is None or len(layers) != 1 or getattr(decoder, "use_leaky_relu", False):
        return False
    l0, lo = layers[0], decoder.lout
    if l0.bias is None or lo.bias is None or lo.weight.shape[0] != 1:
        return False
    return int(l0.weight.shape[0]) <= 64 and int(l0.weight.shape[1]) - 3 <= 61


def _sdf_composed(npm, decoder, x, need_grad=False, need_certainty=False, query_locally=True,
                  use_only_measured_points=True, use_only_valid_points=False, need_std=False, train=False):
    """`Mapper.sdf` composed from its parts (utils/mapper.py:2273-2289: `query_feature` -> `Decoder.sdf` -> IDW sum) for
    the decoder / map options the fused kernels do not implement (`layer_norm_on`, leaky ReLU, more than one hidden
    level, wide layers): the search, gather and weights are the HIP `query_feature`, the decoder is the module's own
    `sdf` (fused when its shape allows, else its torch layers on the device).  Same return tuple as `sdf_fused`;
    `train=True` keeps the graph (returns sdf with grad_fn) instead of detaching."""
    cfg = getattr(npm, "config", None)
    weighted_first = bool(cfg.weighted_first) if cfg is not None else bool(npm.weighted_first)
    xq = x if train else x.detach()
    want_gx = need_grad and not train
    if want_gx:
        xq = xq.clone().requires_grad_(True)
    with torch.enable_grad() if (want_gx or train) else torch.no_grad():
        geo, _, w, cnt, cert = query_feature(npm, xq, accumulate_stability=False, query_locally=query_locally,
                                             use_only_measured_points=use_only_measured_points,
                                             use_only_valid_points=use_only_valid_points)
        dec_sdf = getattr(decoder, "sdf", None)
        if dec_sdf is None:
            from . import decoder as _dec

            pred = _dec.sdf(decoder, geo)
        else:
            pred = dec_sdf(geo)
        std = None
        if weighted_first:
            s_ = pred
        else:
            mean = torch.sum(pred * w, dim=1)
            if need_std:
                std = torch.sqrt(torch.sum(w * (pred - mean.unsqueeze(-1)) ** 2, dim=1)).squeeze(1)
            s_ = mean.squeeze(1)
        grad = torch.autograd.grad(s_.sum(), xq)[0] if want_gx else None
    if not train:
        s_ = s_.detach()
        std = std.detach() if std is not None else None
    res = (s_, grad, cnt, cert if need_certainty else None)
    if need_std:
        res = res + (std if std is not None else torch.zeros_like(s_),)
    return res


def sdf_fused(npm, decoder, x: torch.Tensor, need_grad: bool = False, need_certainty: bool = False,
              query_locally: bool = True, use_only_measured_points: bool = True,
              use_only_valid_points: bool = False, need_std: bool = False, want_idx: bool = False, out=None):
    """Fused inference query = `Mapper.sdf(x)` under no_grad (utils/mapper.py:2273-2289) and, with
    need_grad, the analytic gradient the tracker asks autograd for (utils/tracker.py:282-321).

    Returns (sdf[B], grad[B,3] | None, nn_counts[B], certainty[B] | None) and, with need_std, a fifth value
    sdf_std[B] (spread of the per-neighbour predictions, utils/tracker.py:303-313).  `decoder` is the
    reference's `Decoder` (model/decoder.py) with one hidden level, or any object with
    `layers[0].weight/.bias`, `lout.weight/.bias`, `sdf_scale`.  With want_idx the neighbour rows idx[B,k] (int64, -1 =
    none; rows of the local or global tables, as queried) are appended: what `color_fused` takes.  `out` = (sdf[B],
    nn_counts[B]) lets a chunked caller have the kernel write into slices of its own arrays (contiguous float32 /
    int64 on the query's device); they are then the tensors returned."""
    if out is not None:
        B_ = int(x.shape[0])
        if not (len(out) == 2 and all(t.is_cuda and t.is_contiguous() and t.shape == (B_,) and t.device == x.device
                                      for t in out) and out[0].dtype is torch.float32 and out[1].dtype is torch.int64):
            raise _lib.PingsHipError("sdf_fused: `out` must be (float32 [B], int64 [B]), contiguous, on the query's device")
    if not fused_supported(npm, decoder):
        res = _sdf_composed(npm, decoder, x, need_grad, need_certainty, query_locally, use_only_measured_points,
                            use_only_valid_points, need_std)
        if out is not None:
            out[0].copy_(res[0])
            out[1].copy_(res[2])
            res = (out[0], res[1], out[1]) + res[3:]
        if want_idx:
            res = res + (radius_neighborhood_topk(npm, x, bool(npm.temporal_local_map_on and query_locally),
                                                  use_only_measured_points, use_only_valid_points, query_locally)[0],)
        return res
    L = _lib.lib()
    q = x.detach().to(torch.float32).contiguous()
    B = q.shape[0]
    cfg = getattr(npm, "config", None)
    weighted_first = bool(cfg.weighted_first) if cfg is not None else bool(npm.weighted_first)
    a = _map_args(npm, bool(npm.temporal_local_map_on and query_locally), use_only_measured_points,
                 use_only_valid_points, query_locally)
    W1 = decoder.layers[0].weight.detach().to(torch.float32).contiguous()
    b1 = decoder.layers[0].bias.detach().to(torch.float32).contiguous()
    W2 = decoder.lout.weight.detach().to(torch.float32).contiguous()
    b2 = decoder.lout.bias.detach().to(torch.float32).contiguous()
    feats = (npm.local_geo_features if query_locally else npm.geo_features).detach().contiguous()
    pts = (npm.local_neural_points if query_locally else npm.neural_points).contiguous()
    quat = (npm.local_point_orientations if query_locally else npm.point_orientations).contiguous()
    cert_tab = (npm.local_point_certainties if query_locally else npm.point_certainties).contiguous()
    F = feats.shape[1]
    if W1.shape[1] != F + 3:
        raise ValueError(f"decoder input dim {W1.shape[1]} != feature dim {F} + 3")
    dec = _abi.SdfDecoder(W1.data_ptr(), b1.data_ptr(), W2.data_ptr(), b2.data_ptr(), int(W1.shape[0]), int(F),
                          float(decoder.sdf_scale), int(weighted_first))
    dev = q.device
    sdf = torch.empty(B, dtype=torch.float32, device=dev) if out is None else out[0]
    grad = torch.empty(B, 3, dtype=torch.float32, device=dev) if need_grad else None
    cnt = torch.empty(B, dtype=torch.int64, device=dev) if out is None else out[1]
    cert = torch.empty(B, dtype=torch.float32, device=dev) if need_certainty else None
    std = torch.empty(B, dtype=torch.float32, device=dev) if need_std else None
    idx = torch.empty(B, a.nn_k, dtype=torch.int64, device=dev) if want_idx else None
    st = L.pings_sdf_forward(C.byref(a.c), C.byref(dec), _lib.ptr(feats), _lib.ptr(pts), _lib.ptr(quat),
                             _lib.ptr(cert_tab), int(bool(npm.after_pgo)), _lib.ptr(q), B, _lib.ptr(sdf),
                             _lib.ptr(grad), _lib.ptr(cnt), _lib.ptr(cert), _lib.ptr(idx), None, _lib.ptr(std), None,
                             _lib.stream_ptr(dev))
    _lib.check(st, "pings_sdf_forward")
    res = (sdf, grad, cnt, cert, std) if need_std else (sdf, grad, cnt, cert)
    return res + (idx,) if want_idx else res


def colour_fused_supported(npm, decoder) -> bool:
    """Whether `color_fused` covers this (map, colour decoder) pair: one hidden level of at most 64 units, ReLU, biases,
    1-3 output channels, Fc <= 61, no layer norm.  Everything else keeps the composed path (`query_feature` + the
    decoder's own layers + autograd)."""
    cfg = getattr(npm, "config", None)
    if cfg is not None and getattr(cfg, "layer_norm_on", False):
        return False
    layers = getattr(decoder, "layers", None)
    if layers is None or len(layers) != 1 or getattr(decoder, "use_leaky_relu", False):
        return False
    l0, lo = layers[0], decoder.lout
    if l0.bias is None or lo.bias is None or not 1 <= int(lo.weight.shape[0]) <= 3:
        return False
    return int(l0.weight.shape[0]) <= 64 and int(l0.weight.shape[1]) - 3 <= 61 and _nn_k(npm) <= 16


def color_fused(npm, decoder, x: torch.Tensor, idx: torch.Tensor, need_jac: bool = True, query_locally: bool = True):
    """Fused colour query (`pings_color_forward`): colour[B,C] = IDW of sigmoid(colour decoder) over the neighbours
    `idx[B,k]` (from `sdf_fused(want_idx=True)` or `radius_neighborhood_topk`, same `query_locally`) and, with need_jac,
    jac[B,C,3] = d colour / d x, what utils/tracker.py:328-336 gets from one autograd pass per channel.  Returns
    (colour, jac | None)."""
    if not x.is_cuda:
        raise _lib.PingsHipError("color_fused runs on the HIP device only (got a CPU tensor); there is no CPU fallback")
    if not colour_fused_supported(npm, decoder):
        raise _lib.PingsHipError("color_fused: this colour decoder is not covered by the fused kernel "
                                 "(see colour_fused_supported)")
    L = _lib.lib()
    q = x.detach().to(torch.float32).contiguous()
    B = q.shape[0]
    cfg = getattr(npm, "config", None)
    weighted_first = bool(cfg.weighted_first) if cfg is not None else bool(npm.weighted_first)
    W1 = decoder.layers[0].weight.detach().to(torch.float32).contiguous()
    b1 = decoder.layers[0].bias.detach().to(torch.float32).contiguous()
    W2 = decoder.lout.weight.detach().to(torch.float32).contiguous()
    b2 = decoder.lout.bias.detach().to(torch.float32).contiguous()
    feats = (npm.local_color_features if query_locally else npm.color_features).detach().to(torch.float32).contiguous()
    pts = (npm.local_neural_points if query_locally else npm.neural_points).detach().contiguous()
    quat = (npm.local_point_orientations if query_locally else npm.point_orientations).detach().contiguous()
    Fc, ch = int(feats.shape[1]), int(W2.shape[0])
    if W1.shape[1] != Fc + 3:
        raise ValueError(f"colour decoder input dim {W1.shape[1]} != colour feature dim {Fc} + 3")
    ix = idx.detach().to(torch.int64).contiguous()
    if ix.dim() != 2 or ix.shape[0] != B:
        raise ValueError(f"idx must be [B, k] for B = {B} queries, got {tuple(ix.shape)}")
    rows = min(int(feats.shape[0]), int(pts.shape[0]), int(quat.shape[0]))
    dec = _abi.ColorDecoder(W1.data_ptr(), b1.data_ptr(), W2.data_ptr(), b2.data_ptr(), int(W1.shape[0]), Fc, ch,
                            int(weighted_first))
    dev = q.device
    col = torch.empty(B, ch, dtype=torch.float32, device=dev)
    jac = torch.empty(B, ch, 3, dtype=torch.float32, device=dev) if need_jac else None
    _lib.check(L.pings_color_forward(C.byref(dec), _lib.ptr(feats), rows, _lib.ptr(pts), _lib.ptr(quat),
                                     int(bool(npm.after_pgo)), _lib.ptr(q), B, _lib.ptr(ix), int(ix.shape[1]),
                                     _lib.ptr(col), _lib.ptr(jac), _lib.stream_ptr(dev)), "pings_color_forward")
    return col, jac


_SCRATCH_BYTES = {}


def _sdf_scratch(L, B, nn_k, F, H, rows, dev):
    key = (B, nn_k, F, H, rows)
    n = _SCRATCH_BYTES.get(key)
    if n is None:
        n = _SCRATCH_BYTES[key] = L.pings_sdf_backward_scratch_bytes(B, nn_k, F, H, rows)
    return torch.empty(n, dtype=torch.uint8, device=dev)


def _sdf_first_order(st, g_sdf):
    """(g_x, gF, gW1, gb1, gW2, gb2) of the fused query for the upstream gradient g_sdf [B] (no autograd here)."""
    L = _lib.lib()
    q, f, W1c, b1c, W2c, b2c, idx, gidx, w, pts, quat, gpts, unit = st["saved"]
    sdf_scale, weighted_first, after_pgo, nn_k = st["meta"]
    B, F, H = q.shape[0], f.shape[1], W1c.shape[0]
    dev = q.device
    g = g_sdf.detach()
    if g.dtype != torch.float32 or not g.is_contiguous():
        g = g.to(torch.float32).contiguous()
    gF = gW1 = gb1 = gW2 = gb2 = None
    if st["need_params"]:
        dec = _abi.SdfDecoder(W1c.data_ptr(), b1c.data_ptr(), W2c.data_ptr(), b2c.data_ptr(), int(H), int(F),
                              float(sdf_scale), int(weighted_first))
        gF = torch.empty_like(f)
        flat = torch.empty(H * (F + 5) + 1, dtype=torch.float32, device=dev)      # one allocation for the decoder
        gW1, gb1 = flat[:H * (F + 3)].view(H, F + 3), flat[H * (F + 3):H * (F + 4)]
        gW2, gb2 = flat[H * (F + 4):H * (F + 5)].view(1, H), flat[H * (F + 5):]
        scratch = _sdf_scratch(L, B, nn_k, F, H, f.shape[0], dev)
        base = flat.data_ptr()
        _lib.check(L.pings_sdf_backward(C.byref(dec), f.data_ptr(), f.shape[0], pts.data_ptr(), quat.data_ptr(),
                                        int(after_pgo), q.data_ptr(), B, nn_k, idx.data_ptr(), w.data_ptr(), g.data_ptr(),
                                        scratch.data_ptr(), gF.data_ptr(), base, base + 4 * H * (F + 3),
                                        base + 4 * H * (F + 4), base + 4 * H * (F + 5), _lib.stream_ptr(dev)),
                   "pings_sdf_backward")
    gx = unit * g.unsqueeze(1) if unit is not None else None
    return g, (gx, gF, gW1, gb1, gW2, gb2)


class _SdfTrainBackward(torch.autograd.Function):
    """The backward of `_SdfTrain` as a differentiable op: (g_sdf, x, feats, W1, b1, W2, b2) -> (g_x, g_feats, g_W1,
    g_b1, g_W2, g_b2).  g_x = g_sdf * dS/dx uses the analytic gradient the forward kernel produced; the parameter
    gradients come from `pings_sdf_backward`.  Its own backward (`pings_sdf_double_backward`) propagates a gradient
    arriving at g_x — the Eikonal / consistency losses on dS/dx (utils/mapper.py:1445-1448) — to the features and the
    decoder; gradients arriving at the parameter-gradient outputs (third-order use) are not supported.  Only entered
    when the backward itself is being recorded (create_graph=True); a plain backward calls `_sdf_first_order`."""

    @staticmethod
    def forward(ctx, g_sdf, x, feats, W1, b1, W2, b2, st):
        g, out = _sdf_first_order(st, g_sdf)
        ctx.st = st
        ctx.save_for_backward(g)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gg_x, gg_F, gg_W1, gg_b1, gg_W2, gg_b2):
        if any(t is not None for t in (gg_F, gg_W1, gg_b1, gg_W2, gg_b2)):
            raise NotImplementedError("sdf_train: differentiating the PARAMETER gradients once more is not implemented")
        if gg_x is None:
            return (None,) * 8
        L = _lib.lib()
        st = ctx.st
        (g,) = ctx.saved_tensors
        q, f, W1c, b1c, W2c, b2c, idx, gidx, w, pts, quat, gpts, unit = st["saved"]
        sdf_scale, weighted_first, after_pgo, nn_k = st["meta"]
        B, F, H = q.shape[0], f.shape[1], W1c.shape[0]
        dev = q.device
        ggx = gg_x.detach().to(torch.float32).contiguous()
        v = (ggx * g.unsqueeze(1)).contiguous()            # Phi = sum_b <v_b, dS_b/dx>
        dec = _abi.SdfDecoder(W1c.data_ptr(), b1c.data_ptr(), W2c.data_ptr(), b2c.data_ptr(), int(H), int(F),
                              float(sdf_scale), int(weighted_first))
        f32 = dict(dtype=torch.float32, device=dev)
        dF = torch.empty_like(f)
        dW1, db1 = torch.empty(H, F + 3, **f32), torch.empty(H, **f32)
        dW2, db2 = torch.empty(1, H, **f32), torch.empty(1, **f32)
        scratch = _sdf_scratch(L, B, nn_k, F, H, f.shape[0], dev)
        _lib.check(L.pings_sdf_double_backward(
            C.byref(dec), _lib.ptr(f), f.shape[0], _lib.ptr(pts), _lib.ptr(quat), _lib.ptr(gpts), int(after_pgo),
            _lib.ptr(q), B, nn_k, _lib.ptr(idx), _lib.ptr(gidx), _lib.ptr(w), _lib.ptr(v), _lib.ptr(scratch),
            _lib.ptr(dF), _lib.ptr(dW1), _lib.ptr(db1), _lib.ptr(dW2), _lib.ptr(db2), _lib.stream_ptr(dev)),
            "pings_sdf_double_backward")
        d_g = (ggx * unit).sum(1) if unit is not None else None     # g_x is linear in g_sdf
        # the gradient w.r.t. the query (a third derivative of S) is not produced: None
        return d_g, None, dF, dW1, db1, dW2, db2, None


def _c(t):
    t = t.detach()
    return t if t.is_contiguous() else t.contiguous()


def _sdf_train_forward(x, feats, W1, b1, W2, b2, npm, sdf_scale, weighted_first, query_locally, use_meas, use_valid,
                       need_gx):
    """`pings_sdf_forward` with the neighbour lists kept: (sdf [B], nn_counts [B], state for `_sdf_first_order`)."""
    L = _lib.lib()
    q = x.detach()
    if q.dtype != torch.float32 or not q.is_contiguous():
        q = q.to(torch.float32).contiguous()
    B = q.shape[0]
    a = _map_args(npm, bool(npm.temporal_local_map_on and query_locally), use_meas, use_valid, query_locally)
    f, W1c, b1c, W2c, b2c = _c(feats), _c(W1), _c(b1), _c(W2), _c(b2)
    F = f.shape[1]
    dec = _abi.SdfDecoder(W1c.data_ptr(), b1c.data_ptr(), W2c.data_ptr(), b2c.data_ptr(), int(W1c.shape[0]),
                          int(F), float(sdf_scale), int(weighted_first))
    pts = _c(npm.local_neural_points if query_locally else npm.neural_points)
    quat = _c(npm.local_point_orientations if query_locally else npm.point_orientations)
    gpts = _c(npm.neural_points)
    dev = q.device
    nn_k = a.nn_k
    sdf = torch.empty(B, dtype=torch.float32, device=dev)
    cnt = torch.empty(B, dtype=torch.int64, device=dev)
    idx = torch.empty(B, nn_k, dtype=torch.int64, device=dev)
    w = torch.empty(B, nn_k, dtype=torch.float32, device=dev)
    gidx = torch.empty(B, nn_k, dtype=torch.int64, device=dev) if need_gx else None
    unit = torch.empty(B, 3, dtype=torch.float32, device=dev) if need_gx else None
    st = L.pings_sdf_forward(C.byref(a.c), C.byref(dec), f.data_ptr(), pts.data_ptr(), quat.data_ptr(), None,
                             int(bool(npm.after_pgo)), q.data_ptr(), B, sdf.data_ptr(), _lib.ptr(unit), cnt.data_ptr(),
                             None, idx.data_ptr(), w.data_ptr(), None, _lib.ptr(gidx), _lib.stream_ptr(dev))
    _lib.check(st, "pings_sdf_forward")
    state = {"saved": (q, f, W1c, b1c, W2c, b2c, idx, gidx, w, pts, quat, gpts, unit),
             "meta": (float(sdf_scale), int(weighted_first), bool(npm.after_pgo), nn_k),
             "need_params": any(t.requires_grad for t in (feats, W1, b1, W2, b2)), "keep": a}
    return sdf, cnt, state


class _SdfTrain(torch.autograd.Function):
    """S(x) with fused first- and second-order backward to the feature table and the decoder
    (`pings_sdf_forward` / `pings_sdf_backward` / `pings_sdf_double_backward`)."""

    @staticmethod
    def forward(ctx, x, feats, W1, b1, W2, b2, npm, sdf_scale, weighted_first, query_locally, use_meas, use_valid):
        sdf, cnt, ctx.state = _sdf_train_forward(x, feats, W1, b1, W2, b2, npm, sdf_scale, weighted_first,
                                                 query_locally, use_meas, use_valid, x.requires_grad)
        ctx.save_for_backward(x, feats, W1, b1, W2, b2)
        ctx.mark_non_differentiable(cnt)
        return sdf, cnt

    @staticmethod
    def backward(ctx, g_sdf, _g_cnt):
        x, feats, W1, b1, W2, b2 = ctx.saved_tensors
        if g_sdf is None:
            return (None,) * 12
        if not torch.is_grad_enabled():           # plain backward: nothing will differentiate this call
            return _sdf_first_order(ctx.state, g_sdf)[1] + (None,) * 6
        out = _SdfTrainBackward.apply(g_sdf, x, feats, W1, b1, W2, b2, ctx.state)
        return tuple(out) + (None,) * 6


def sdf_train(npm, decoder, x: torch.Tensor, query_locally: bool = True, use_only_measured_points: bool = True,
              use_only_valid_points: bool = False):
    """Differentiable `Mapper.sdf(x)` (utils/mapper.py:2273-2289) for the training loop: one fused forward
    kernel and one fused, deterministic backward to `local_geo_features` and the decoder parameters
    (first order: use `query_feature` when the loss needs a gradient of the gradient, mapper.py:1448).
    Returns (sdf[B], nn_counts[B])."""
    cfg = getattr(npm, "config", None)
    if not fused_supported(npm, decoder):
        s_, _, cnt, _ = _sdf_composed(npm, decoder, x, False, False, query_locally, use_only_measured_points,
                                      use_only_valid_points, train=True)
        return s_, cnt
    weighted_first = bool(cfg.weighted_first) if cfg is not None else bool(npm.weighted_first)
    feats = npm.local_geo_features if query_locally else npm.geo_features
    l0, lo = decoder.layers[0], decoder.lout
    return _SdfTrain.apply(x, feats, l0.weight, l0.bias, lo.weight, lo.bias, npm, float(decoder.sdf_scale),
                           weighted_first, query_locally, use_only_measured_points, use_only_valid_points)


# ---------------------------------------------------------------- fused finite-difference gradient
class _NumGrad(torch.autograd.Function):
    """`Mapper.get_numerical_gradient` (utils/mapper.py:2319-2370) as ONE graph node: shifted points, fused SDF query
    and central differences forward (3 launches); the differences' adjoint and the fused SDF backward to the feature
    table and the decoder backward.  The reference's op sequence is ~25 torch operators each way."""

    @staticmethod
    def forward(ctx, x, sdf_x, feats, W1, b1, W2, b2, npm, sdf_scale, weighted_first, eps, two_side):
        L = _lib.lib()
        q = x.detach()
        if q.dtype != torch.float32 or not q.is_contiguous():
            q = q.to(torch.float32).contiguous()
        N = q.shape[0]
        dev = q.device
        blocks = 6 if two_side else 3
        xs = torch.empty(blocks * N, 3, dtype=torch.float32, device=dev)
        stream = _lib.stream_ptr(dev)
        _lib.check(L.pings_stencil_points(q.data_ptr(), N, float(eps), int(two_side), xs.data_ptr(), stream),
                   "pings_stencil_points")
        s, _cnt, state = _sdf_train_forward(xs, feats, W1, b1, W2, b2, npm, sdf_scale, weighted_first, True, True,
                                            False, False)
        s0 = None
        if not two_side:
            s0 = sdf_x.detach()
            if s0.dtype != torch.float32 or not s0.is_contiguous():
                s0 = s0.to(torch.float32).contiguous()
        grad = torch.empty(N, 3, dtype=torch.float32, device=dev)
        _lib.check(L.pings_stencil_gradient(s.data_ptr(), _lib.ptr(s0), N, float(eps), int(two_side), grad.data_ptr(),
                                            stream), "pings_stencil_gradient")
        ctx.state, ctx.N, ctx.eps, ctx.two_side = state, N, float(eps), bool(two_side)
        ctx.need_s0 = (not two_side) and sdf_x is not None and sdf_x.requires_grad
        return grad

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if g is None:
            return (None,) * 12
        L = _lib.lib()
        N = ctx.N
        dev = g.device
        gg = g.detach()
        if gg.dtype != torch.float32 or not gg.is_contiguous():
            gg = gg.to(torch.float32).contiguous()
        up = torch.empty((6 if ctx.two_side else 3) * N, dtype=torch.float32, device=dev)
        up0 = torch.empty(N, dtype=torch.float32, device=dev) if ctx.need_s0 else None
        _lib.check(L.pings_stencil_gradient_backward(gg.data_ptr(), N, ctx.eps, int(ctx.two_side), up.data_ptr(),
                                                     _lib.ptr(up0), _lib.stream_ptr(dev)),
                   "pings_stencil_gradient_backward")
        _, (_gx, gF, gW1, gb1, gW2, gb2) = _sdf_first_order(ctx.state, up)
        return (None, up0, gF, gW1, gb1, gW2, gb2) + (None,) * 5


def numerical_gradient(npm, decoder, x, sdf_x=None, eps=0.02, two_side=True):
    """Fused `Mapper.get_numerical_gradient`: [N,3] finite-difference SDF gradient at `x` (local query, measured points
    only — the defaults `Mapper.sdf` uses), differentiable w.r.t. `local_geo_features`, the decoder and (one-sided)
    `sdf_x`; `x` itself is treated as a constant (callers with `x.requires_grad` take the composed path)."""
    cfg = getattr(npm, "config", None)
    if not fused_supported(npm, decoder):
        raise NotImplementedError("numerical_gradient: the fused node needs the fused SDF kernels (caller composes)")
    weighted_first = bool(cfg.weighted_first) if cfg is not None else bool(npm.weighted_first)
    l0, lo = decoder.layers[0], decoder.lout
    return _NumGrad.apply(x, sdf_x, npm.local_geo_features, l0.weight, l0.bias, lo.weight, lo.bias, npm,
                          float(decoder.sdf_scale), weighted_first, float(eps), bool(two_side))


def install(neural_points_cls) -> None:
    """Route the reference's `NeuralPoints.query_feature` through the HIP search kernel."""
    neural_points_cls.query_feature = query_feature
    neural_points_cls.radius_neighborhood_search = radius_neighborhood_search
