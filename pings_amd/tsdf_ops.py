"""Depth-view fusion into a sparse TSDF volume and its mesh, on the HIP device (csrc/tsdf.hip): what
`SLAMDataset.o3d_tsdf_fusion` (dataset/slam_dataset.py:1154-1193) does with Open3D's `ScalableTSDFVolume`, and the link
between `render(...)["surf_depth"]` and `mesh_ops.finish_mesh` / `eval_ops.eval_pair`.

  TSDFVolume.integrate     one depth (+ colour) view: touch -> (one host read) -> assign new blocks -> update
  TSDFVolume.integrate_points  one LiDAR scan, optionally carving free space (csrc/tsdf_points.hip):
                           ray touch -> (one host read) -> assign -> accumulate integer sums -> apply
  TSDFVolume.dense         a box of grid points as dense tsdf / weight / colour arrays
  TSDFVolume.extract_mesh  per chunk densify -> marching cubes (csrc/mc.hip, unchanged) -> vertices from global integers,
                           then `mesh_ops.finish_mesh`
  install(module)          rebinds `SLAMDataset.o3d_tsdf_fusion`; with `lidar=True` adds `SLAMDataset.lidar_tsdf_fusion`

Images are fp32 tensors on the HIP device and a CPU tensor raises `PingsHipError`: there is no CPU fallback.  The
rules are restated in fp64 numpy by tests/tsdf_ref.py and tests/tsdf_points_ref.py.  Every host read is recorded with `_lib.note_sync`."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _abi, _lib
from . import mesh_ops

B = _abi.TSDF_BLOCK
VOX = B * B * B
_BIAS = 1 << 20
_MASK = (1 << 21) - 1


def _host_array(m, what: str) -> np.ndarray:
    if isinstance(m, torch.Tensor):
        if m.is_cuda:
            _lib.note_sync("tsdf_" + what)
        m = m.detach().cpu().numpy()
    return np.asarray(m, dtype=np.float64)


def _intrinsic(K) -> tuple:
    """(fx, fy, cx, cy) of a 3x3 array or tensor, or of an object with `.intrinsic_matrix` (Open3D's)."""
    K = _host_array(getattr(K, "intrinsic_matrix", K), "intrinsic")
    if K.shape != (3, 3):
        raise ValueError(f"K must be 3x3, got {K.shape}")
    return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])


def _image(name: str, t, shapes) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor, got {type(t).__name__}")
    if tuple(t.shape) not in shapes:
        raise ValueError(f"{name} must have shape {' or '.join(str(list(s)) for s in shapes)}, got {list(t.shape)}")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    if not t.is_cuda:
        raise _lib.PingsHipError(f"{name}: pings_amd.tsdf_ops runs on the HIP device only (got a CPU tensor); "
                                 "there is no CPU fallback")
    return t.detach().contiguous()


def _f64x(values):
    values = [float(v) for v in values]
    return (C.c_double * len(values))(*values)


class TSDFVolume:
    """A growable set of 8^3-voxel blocks: fp32 `tsdf` (1 where nothing was seen), fp32 `weight` (the number of views
    averaged) and, with `color`, three fp32 colour planes in [0, 1].  Grid point g lies at origin + voxel_length * g.
    A block's slot never changes; within a frame new blocks take slots in ascending (bx, by, bz), so the whole store
    is the same bits from run to run.  Growth is geometric (one copy per field)."""

    GROWTH = 1.5

    def __init__(self, voxel_length, sdf_trunc, color=True, origin=(0.0, 0.0, 0.0), device=None, capacity_blocks=4096):
        self.voxel_length, self.sdf_trunc = float(voxel_length), float(sdf_trunc)
        if not (self.voxel_length > 0.0 and self.sdf_trunc > 0.0 and math.isfinite(self.voxel_length)
                and math.isfinite(self.sdf_trunc)):
            raise ValueError("voxel_length and sdf_trunc must be positive and finite")
        if 2.0 * self.sdf_trunc > B * self.voxel_length:
            raise ValueError(f"2 * sdf_trunc = {2.0 * self.sdf_trunc} exceeds the block edge {B} * voxel_length = "
                             f"{B * self.voxel_length}: a pixel would touch more than 8 blocks")
        self.origin = tuple(float(v) for v in origin)
        if len(self.origin) != 3:
            raise ValueError("origin must have 3 components")
        self.color = bool(color)
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if dev.type != "cuda":
            raise _lib.PingsHipError("TSDFVolume lives on the HIP device only; there is no CPU fallback")
        self.device = dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())
        self._capacity0 = max(1, int(capacity_blocks))
        self.reset()

    # ------------------------------------------------------------------ store and table
    def reset(self) -> None:
        """Back to the empty volume with the capacity it was created with."""
        self.n_blocks, self.capacity, self._frame = 0, 0, 0
        self._keys = self._tsdf = self._weight = self._color = None
        self._tkeys = self._tslots = self._tstamps = None
        self._lists = self._tindex = None
        self._reserve(self._capacity0)

    def _reserve(self, blocks: int) -> None:
        if blocks <= self.capacity:
            return
        cap = max(int(blocks), int(self.capacity * self.GROWTH))
        dev, n = self.device, self.n_blocks

        def grown(old, *shape, dtype=torch.float32):
            new = torch.empty((cap, *shape), dtype=dtype, device=dev)
            if old is not None and n:
                new[:n].copy_(old[:n])
            return new

        self._keys = grown(self._keys, dtype=torch.int64)
        self._tsdf = grown(self._tsdf, VOX)
        self._weight = grown(self._weight, VOX)
        if self.color:
            self._color = grown(self._color, 3, VOX)
        self.capacity = cap

    def _table(self, blocks: int) -> None:
        """A table of at least twice `blocks` entries; a larger one is filled again from the store's keys."""
        size = 1 << max(10, (2 * int(blocks) - 1).bit_length())
        if self._tkeys is not None and size <= self._tkeys.shape[0]:
            return
        if size >= 1 << 31:
            raise _lib.PingsHipError("TSDFVolume: the block table would pass 2**31 entries")
        dev = self.device
        self._tkeys = torch.full((size,), -1, dtype=torch.int64, device=dev)
        self._tslots = torch.full((size,), -1, dtype=torch.int32, device=dev)
        self._tstamps = torch.zeros(size, dtype=torch.int32, device=dev)
        if self.n_blocks:
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            _lib.check(_lib.lib().pings_tsdf_table_insert(_lib.ptr(self._keys), self.n_blocks, _lib.ptr(self._tkeys),
                                                          _lib.ptr(self._tslots), size, _lib.ptr(status),
                                                          _lib.stream_ptr(dev)), "pings_tsdf_table_insert")

    def block_coords(self) -> torch.Tensor:
        """[n_blocks, 3] int64 block indices (grid point // 8) in slot order, on the device."""
        k = self._keys[:self.n_blocks]
        return torch.stack(((k >> 42) - _BIAS, ((k >> 21) & _MASK) - _BIAS, (k & _MASK) - _BIAS), dim=1)

    # ------------------------------------------------------------------ integrate
    def integrate(self, depth, K, extrinsic, color=None, *, depth_trunc=math.inf, depth_min=0.0, stride=4) -> None:
        """Fuses one view.  depth [H, W] (or [1, H, W]) fp32 z-depth in metres, valid where finite and depth_min < d <
        depth_trunc; color [3, H, W] fp32 in [0, 1] (required with a colour volume); K a 3x3 array or an object with
        `.intrinsic_matrix`; extrinsic the host 4x4 world -> camera matrix (fp64, rounded to fp32 once).  Every valid
        pixel with u % stride == v % stride == 0 touches the blocks within sdf_trunc of its point; exactly the touched
        blocks are updated.  One host read (touched and new block counts and the status, one record); a frame without a
        valid pixel ends after it."""
        if isinstance(depth, torch.Tensor) and depth.dim() == 3 and depth.shape[0] == 1:
            depth = depth[0]
        if not isinstance(depth, torch.Tensor) or depth.dim() != 2 or depth.numel() == 0:
            raise ValueError("depth must be a [H, W] or [1, H, W] tensor and not empty")
        H, W = (int(s) for s in depth.shape)
        d = _image("depth", depth, [(H, W)])
        if self.color and color is None:
            raise ValueError("a colour volume needs the view's colour image")
        img = _image("color", color, [(3, H, W)]) if self.color else None
        if d.device != self.device or (img is not None and img.device != self.device):
            raise _lib.PingsHipError(f"TSDFVolume on {self.device} got an image on {d.device}")
        stride = int(stride)
        if stride < 1:
            raise ValueError(f"stride must be at least 1, got {stride}")
        E = _host_array(extrinsic, "extrinsic")
        if E.shape != (4, 4):
            raise ValueError(f"extrinsic must be 4x4, got {E.shape}")
        intr = _f64x(_intrinsic(K))
        ext, inv = _f64x(E[:3].reshape(-1)), _f64x(np.linalg.inv(E)[:3].reshape(-1))
        org = _f64x(self.origin)
        dev, L = self.device, _lib.lib()
        st = _lib.stream_ptr(dev)

        list_cap = 8 * math.ceil(W / stride) * math.ceil(H / stride)
        self._table(self.n_blocks + list_cap)
        if self._lists is None or self._lists[0].shape[0] < list_cap:
            self._lists = (torch.empty(list_cap, dtype=torch.int32, device=dev),
                           torch.empty(list_cap, dtype=torch.int64, device=dev),
                           torch.zeros(4, dtype=torch.int32, device=dev))
        touched, new_keys, counters = self._lists
        tsize = self._tkeys.shape[0]
        self._frame += 1
        tot = (C.c_int64 * 3)(0, 0, 0)
        _lib.note_sync("tsdf_touch")
        _lib.check(L.pings_tsdf_touch(_lib.ptr(d), H, W, intr, inv, org, self.voxel_length, self.sdf_trunc,
                                      float(depth_min), float(depth_trunc), stride, self._frame, _lib.ptr(self._tkeys),
                                      _lib.ptr(self._tslots), _lib.ptr(self._tstamps), tsize, touched.shape[0],
                                      _lib.ptr(touched), _lib.ptr(new_keys), _lib.ptr(counters), tot, st),
                   "pings_tsdf_touch")
        n_touched, n_new, status = min(int(tot[0]), list_cap), min(int(tot[1]), list_cap), int(tot[2])
        if status & _abi.TSDF_TABLE_FULL:
            raise _lib.PingsHipError("tsdf_ops internal error: the block table filled up")
        if n_new:
            self._reserve(self.n_blocks + n_new)
            scratch = torch.empty(L.pings_tsdf_assign_scratch_bytes(n_new), dtype=torch.uint8, device=dev)
            _lib.check(L.pings_tsdf_assign(_lib.ptr(new_keys), n_new, self.n_blocks, self.capacity, _lib.ptr(scratch),
                                           _lib.ptr(self._tkeys), _lib.ptr(self._tslots), tsize, _lib.ptr(self._keys),
                                           _lib.ptr(self._tsdf), _lib.ptr(self._weight), _lib.ptr(self._color), st),
                       "pings_tsdf_assign")
            self.n_blocks += n_new
        if n_touched:
            _lib.check(L.pings_tsdf_update(_lib.ptr(d), _lib.ptr(img), H, W, intr, ext, org, self.voxel_length,
                                           self.sdf_trunc, float(depth_min), float(depth_trunc), _lib.ptr(touched),
                                           n_touched, _lib.ptr(self._tkeys), _lib.ptr(self._tslots), tsize, self.capacity,
                                           _lib.ptr(self._tsdf), _lib.ptr(self._weight), _lib.ptr(self._color), st),
                       "pings_tsdf_update")
        if status & _abi.TSDF_EXTENT:
            raise _lib.PingsHipError("tsdf_ops: a pixel lies beyond 2**20 blocks from the origin and was left out; "
                                     "use a larger voxel_length or an origin near the scene")

    # ------------------------------------------------------------------ integrate a LiDAR scan
    def _points_block_bound(self, n: int, space_carving: bool, max_range: float) -> int:
        """A host-side bound on the blocks one scan can name, so that table and lists are sized without a read."""
        if not space_carving:
            return 8 * n                          # a segment of 2 sdf_trunc plus one cube: 2 blocks per axis
        edge, reach = B * self.voxel_length, max_range + self.sdf_trunc
        per_ray = 3 * (math.floor(reach / edge) + 2) - 2            # a line leaves a block through one face at a time
        cube = (math.ceil(2.0 * reach / edge) + 2) ** 3             # every block within reach of the sensor
        return min(n * per_ray, cube)

    def integrate_points(self, points, origin, colors=None, *, space_carving=False, sdf_mode="point", min_range=0.0,
                         max_range=math.inf, max_weight=None) -> None:
        """Fuses one LiDAR scan.  points [N, 3] fp32 in the world frame, valid where finite and min_range < |p - o| <
        max_range; origin the sensor position o, a host sequence of 3 or a device tensor [3] (taken without a host
        copy); colors [N, 3] fp32 in [0, 1] (required with a colour volume).  Every valid point's ray samples the
        voxels whose cubes it crosses between max(0, r - sdf_trunc) (0 with `space_carving`, which needs a finite
        max_range) and r + sdf_trunc; `sdf_mode` is "point" (signed distance to the point, VDB-Fusion's) or "ray" (the
        projective distance along the ray).  A voxel averages all its samples of the call at once from exact integer
        sums, so the store does not depend on the order of the rows; `max_weight` caps the weight afterwards.  One host
        read (touched and new block counts and the status); a scan without a valid point ends after it."""
        if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
            raise ValueError("points must be a [N, 3] tensor")
        n = int(points.shape[0])
        pts = _image("points", points, [(n, 3)])
        if self.color and colors is None:
            raise ValueError("a colour volume needs the scan's colours")
        col = _image("colors", colors, [(n, 3)]) if self.color else None
        if pts.device != self.device or (col is not None and col.device != self.device):
            raise _lib.PingsHipError(f"TSDFVolume on {self.device} got a scan on {pts.device}")
        if sdf_mode not in ("point", "ray"):
            raise ValueError(f"sdf_mode must be 'point' or 'ray', got {sdf_mode!r}")
        min_range, max_range = float(min_range), float(max_range)
        if not (0.0 <= min_range < max_range):
            raise ValueError(f"0 <= min_range < max_range, got {min_range} and {max_range}")
        if space_carving and not math.isfinite(max_range):
            raise ValueError("space carving needs a finite max_range: it bounds the blocks a scan can name")
        if n > _abi.TSDF_POINTS_MAX:
            raise ValueError(f"a scan holds at most {_abi.TSDF_POINTS_MAX} points (the count field of the accumulators), "
                             f"got {n}; split it")
        cap = math.inf if max_weight is None else float(max_weight)
        if not cap >= 1.0:
            raise ValueError(f"max_weight must be at least 1, got {max_weight}")
        dev, L = self.device, _lib.lib()
        if isinstance(origin, torch.Tensor):
            if origin.device != dev or origin.numel() != 3:
                raise ValueError(f"origin must be a tensor of 3 on {dev} or a host sequence of 3")
            sensor = origin.detach().reshape(3).to(torch.float32).contiguous()
        else:
            o = np.asarray(origin, dtype=np.float64).reshape(-1)
            if o.shape != (3,):
                raise ValueError("origin must have 3 components")
            sensor = torch.tensor(o.tolist(), dtype=torch.float32, device=dev)
        org, st = _f64x(self.origin), _lib.stream_ptr(dev)
        mode = _abi.TSDF_SDF_RAY if sdf_mode == "ray" else _abi.TSDF_SDF_POINT
        carve = int(bool(space_carving))

        list_cap = max(1, self._points_block_bound(n, carve, max_range))
        self._table(self.n_blocks + list_cap)
        if self._lists is None or self._lists[0].shape[0] < list_cap:
            self._lists = (torch.empty(list_cap, dtype=torch.int32, device=dev),
                           torch.empty(list_cap, dtype=torch.int64, device=dev),
                           torch.zeros(4, dtype=torch.int32, device=dev))
        touched, new_keys, counters = self._lists
        tsize = self._tkeys.shape[0]
        if self._tindex is None or self._tindex.shape[0] != tsize:
            self._tindex = torch.empty(tsize, dtype=torch.int32, device=dev)
        self._frame += 1
        tot = (C.c_int64 * 3)(0, 0, 0)
        _lib.note_sync("tsdf_touch_points")
        _lib.check(L.pings_tsdf_points_touch(_lib.ptr(pts), n, _lib.ptr(sensor), org, self.voxel_length, self.sdf_trunc,
                                             min_range, max_range, carve, self._frame, _lib.ptr(self._tkeys),
                                             _lib.ptr(self._tslots), _lib.ptr(self._tstamps), _lib.ptr(self._tindex),
                                             tsize, touched.shape[0], _lib.ptr(touched), _lib.ptr(new_keys),
                                             _lib.ptr(counters), tot, st), "pings_tsdf_points_touch")
        n_touched, n_new, status = int(tot[0]), int(tot[1]), int(tot[2])
        if status & _abi.TSDF_TABLE_FULL or n_touched > list_cap:
            raise _lib.PingsHipError("tsdf_ops internal error: a scan named more blocks than its bound")
        if n_new:
            self._reserve(self.n_blocks + n_new)
            scratch = torch.empty(L.pings_tsdf_assign_scratch_bytes(n_new), dtype=torch.uint8, device=dev)
            _lib.check(L.pings_tsdf_assign(_lib.ptr(new_keys), n_new, self.n_blocks, self.capacity, _lib.ptr(scratch),
                                           _lib.ptr(self._tkeys), _lib.ptr(self._tslots), tsize, _lib.ptr(self._keys),
                                           _lib.ptr(self._tsdf), _lib.ptr(self._weight), _lib.ptr(self._color), st),
                       "pings_tsdf_assign")
            self.n_blocks += n_new
        if n_touched:
            acc = torch.zeros((n_touched, 4 if self.color else 1, VOX), dtype=torch.int64, device=dev)   # one fill
            _lib.check(L.pings_tsdf_points_accumulate(_lib.ptr(pts), _lib.ptr(col), n, _lib.ptr(sensor), org,
                                                      self.voxel_length, self.sdf_trunc, min_range, max_range, carve,
                                                      mode, self._frame, _lib.ptr(self._tkeys), _lib.ptr(self._tslots),
                                                      _lib.ptr(self._tstamps), _lib.ptr(self._tindex), tsize, n_touched,
                                                      _lib.ptr(acc), st), "pings_tsdf_points_accumulate")
            _lib.check(L.pings_tsdf_points_apply(_lib.ptr(touched), n_touched, _lib.ptr(self._tslots), tsize,
                                                 self.capacity, _lib.ptr(acc), int(self.color), cap,
                                                 _lib.ptr(self._tsdf), _lib.ptr(self._weight), _lib.ptr(self._color), st),
                       "pings_tsdf_points_apply")
        if status & _abi.TSDF_EXTENT:
            raise _lib.PingsHipError("tsdf_ops: a ray lies beyond 2**20 blocks from the origin and was left out; "
                                     "use a larger voxel_length or an origin near the scene")

    # ------------------------------------------------------------------ dense boxes and the mesh
    def _densify(self, lo, hi, min_weight, want_weight, want_color):
        lo, hi = [int(v) for v in lo], [int(v) for v in hi]
        if len(lo) != 3 or len(hi) != 3 or any(h <= l for l, h in zip(lo, hi)):
            raise ValueError(f"dense box [{lo}, {hi}) is empty or not 3-D")
        n = [h - l for l, h in zip(lo, hi)]
        dev, L = self.device, _lib.lib()
        self._table(self.n_blocks)
        t = torch.empty(n, device=dev)
        w = torch.empty(n, device=dev) if want_weight else None
        c = torch.empty((*n, 3), device=dev) if want_color and self.color else None
        lo3 = (C.c_int64 * 3)(*lo)
        _lib.check(L.pings_tsdf_densify(_lib.ptr(self._tkeys), _lib.ptr(self._tslots), self._tkeys.shape[0],
                                        self.capacity, _lib.ptr(self._tsdf), _lib.ptr(self._weight),
                                        _lib.ptr(self._color), lo3, n[0], n[1], n[2], float(min_weight), _lib.ptr(t),
                                        _lib.ptr(w), _lib.ptr(c), _lib.stream_ptr(dev)), "pings_tsdf_densify")
        return t, w, c, lo3, n

    def dense(self, lo, hi):
        """The grid points lo <= g < hi (integers per axis) as (tsdf [nx, ny, nz], weight [nx, ny, nz], colour
        [nx, ny, nz, 3] or None).  Voxels of absent blocks read tsdf 1, weight 0, colour 0.  No host read."""
        t, w, c, _, _ = self._densify(lo, hi, 0.0, True, True)
        return t, w, c

    def extract_mesh(self, min_weight=1, min_tri=0, normals=True, chunk=256) -> mesh_ops.Mesh:
        """The zero surface of the cells whose 8 corners all have weight >= min_weight, as a finished mesh: the
        bounding box of the blocks is walked in chunks of `chunk` grid points per axis that share one plane of points,
        each chunk densified (+inf where unobserved, which marching cubes skips), meshed with PINGS_MC_ASCENT so that
        (v1 - v0) x (v2 - v0) points to the free-space side, and its vertices recomputed from global integers so that
        the chunks weld without seams.  Host reads: the block coordinates once, one per meshed chunk (its totals) and
        those of `finish_mesh`."""
        chunk = int(chunk)
        if chunk < 2:
            raise ValueError(f"chunk must be at least 2 grid points, got {chunk}")
        dev, L = self.device, _lib.lib()
        if self.n_blocks == 0:
            return mesh_ops.finish_mesh([], min_tri, normals, torch.zeros(0, 3, device=dev) if self.color else None)
        _lib.note_sync("tsdf_block_coords")
        bc = self.block_coords().cpu().numpy()
        lo, hi = bc.min(0) * B, (bc.max(0) + 1) * B
        starts = [range(int(lo[a]), int(hi[a]) - 1, chunk - 1) for a in range(3)]
        st = _lib.stream_ptr(dev)
        org = _f64x(self.origin)
        flags = _abi.MC_ASCENT
        parts, cols = [], []
        for sx in starts[0]:
            in_x = bc[(bc[:, 0] * B < sx + chunk) & (bc[:, 0] * B + B > sx)]
            for sy in starts[1]:
                in_xy = in_x[(in_x[:, 1] * B < sy + chunk) & (in_x[:, 1] * B + B > sy)]
                for sz in starts[2]:
                    if not ((in_xy[:, 2] * B < sz + chunk) & (in_xy[:, 2] * B + B > sz)).any():
                        continue
                    s = (sx, sy, sz)
                    e = [min(s[a] + chunk, int(hi[a])) for a in range(3)]
                    vol, _, col, lo3, (nx, ny, nz) = self._densify(s, e, float(min_weight), False, True)
                    scratch = torch.empty(L.pings_mc_scratch_bytes(nx, ny, nz), dtype=torch.uint8, device=dev)
                    tot = (C.c_int64 * 2)(0, 0)
                    _lib.note_sync("mc_count")
                    _lib.check(L.pings_mc_count(_lib.ptr(vol), None, nx, ny, nz, 0.0, flags, _lib.ptr(scratch), tot, st),
                               "pings_mc_count")
                    nv, nf = int(tot[0]), int(tot[1])
                    if nv == 0 or nf == 0:
                        continue
                    keys = torch.empty(nv, dtype=torch.int64, device=dev)
                    local = torch.empty(nv, 3, device=dev)        # fl32(i_local + t): differs between chunks, not used
                    faces = torch.empty(nf, 3, dtype=torch.int64, device=dev)
                    _lib.check(L.pings_mc_emit(_lib.ptr(vol), None, nx, ny, nz, 0.0, flags, _lib.ptr(scratch), nv, nf,
                                               _lib.ptr(keys), _lib.ptr(local), _lib.ptr(faces), st), "pings_mc_emit")
                    verts = torch.empty(nv, 3, device=dev)
                    vcol = torch.empty(nv, 3, device=dev) if col is not None else None
                    _lib.check(L.pings_tsdf_vertices(_lib.ptr(keys), nv, _lib.ptr(vol), _lib.ptr(col), lo3, nx, ny, nz,
                                                     org, self.voxel_length, _lib.ptr(verts), _lib.ptr(vcol), st),
                               "pings_tsdf_vertices")
                    parts.append((verts, faces))
                    if vcol is not None:
                        cols.append(vcol)
        colors = (torch.cat(cols) if cols else torch.zeros(0, 3, device=dev)) if self.color else None
        return mesh_ops.finish_mesh(parts, min_tri, normals, colors)


# ---------------------------------------------------------------------- SLAMDataset.o3d_tsdf_fusion
def o3d_tsdf_fusion(self, frame_step=1, output_path=None, vox_size=0.02, trunc_dist=0.06):
    """`SLAMDataset.o3d_tsdf_fusion` without Open3D: every `frame_step`-th frame's main-camera image (H x W x 4: RGB
    0-255 and depth in metres) is fused at the ground-truth pose, extrinsic T_c_l @ inv(gt_poses[i]), depths kept
    below config.max_range; the mesh is written to `output_path` as PLY and returned as an Open3D mesh when Open3D
    imports, else as a `mesh_ops.Mesh`."""
    dev = getattr(self, "device", None)
    dev = torch.device(dev) if dev is not None and torch.device(dev).type == "cuda" else None
    volume = TSDFVolume(vox_size, trunc_dist, color=True, device=dev)
    loader, cfg = self.loader, self.config
    T_c_l = np.asarray(loader.T_c_l, dtype=np.float64)
    for frame_id in range(0, self.total_pc_count, frame_step):
        frame = loader[cfg.begin_frame + frame_id * cfg.step_frame]
        rgbd = np.asarray(frame["img"][loader.main_cam_name])
        rgb = np.ascontiguousarray(rgbd[:, :, :3].astype(np.uint8).transpose(2, 0, 1))      # Open3D's Image(uint8)
        color = torch.from_numpy(rgb).to(volume.device).to(torch.float32) / 255.0
        depth = torch.from_numpy(np.ascontiguousarray(rgbd[:, :, 3], dtype=np.float32)).to(volume.device)
        T_c_w = T_c_l @ np.linalg.inv(np.asarray(self.gt_poses[frame_id], dtype=np.float64))
        volume.integrate(depth, loader.intrinsic, T_c_w, color, depth_trunc=cfg.max_range, stride=4)
    mesh = volume.extract_mesh()
    if output_path is not None:
        mesh_ops.write_ply(str(output_path), mesh.verts, mesh.faces, mesh.normals, mesh.colors)
        print(f"Save the mesh resulting from TSDF fusion to {output_path}")
    try:
        import open3d  # noqa: F401
    except ImportError:
        return mesh
    return mesh_ops.to_open3d(mesh)


# ---------------------------------------------------------------------- SLAMDataset.lidar_tsdf_fusion
def lidar_tsdf_fusion(self, voxel_size, sdf_trunc=None, space_carving=False, sdf_mode="point", frame_step=1,
                      down_vox_m=None, use_gt_pose=False, output_path=None, color=False):
    """The replay loop of `SLAMDataset.write_merged_point_cloud` (dataset/slam_dataset.py:1021-1101) with its
    commented-out VDB-Fusion baseline switched on: per frame the loader, `intrinsic_correct` when
    `kitti_correction_on`, the dataset's own `deskew_at_frame`, voxel down-sampling, the range and height crop, the
    pose (gt / pgo / odom in the reference's order), then `TSDFVolume.integrate_points(points, pose[:3, 3])`.
    `sdf_trunc` defaults to 4 voxels (2 sdf_trunc is then exactly the block edge); carving reaches `config.max_range`.
    `color` fuses columns 3:6 of a 3-channel cloud.  The mesh is written to `output_path` as PLY and returned as
    `o3d_tsdf_fusion` returns it.  No Open3D call."""
    from . import lidar_ops, neural_map

    cfg = self.config
    dev = getattr(self, "device", None)
    dev = torch.device(dev) if dev is not None and torch.device(dev).type == "cuda" else None
    sdf_trunc = 4.0 * float(voxel_size) if sdf_trunc is None else float(sdf_trunc)
    volume = TSDFVolume(voxel_size, sdf_trunc, color=bool(color), device=dev)
    down_vox_m = cfg.vox_down_m if down_vox_m is None else down_vox_m
    # what the crop lets through, with room for the fp32 rounding of the transform: the carving bound of every scan
    reach = float(cfg.max_range)
    if cfg.range_filter_2d:
        reach = math.hypot(reach, max(abs(float(cfg.min_z)), abs(float(cfg.max_z))))
    reach *= 1.001
    for frame_id in range(0, self.total_pc_count, frame_step):
        self.init_temp_data()
        self.read_frame_with_loader(frame_id, False, False)
        if self.cur_point_cloud_torch is None:
            continue
        if cfg.kitti_correction_on:
            correct = getattr(lidar_ops._module_of(self), "intrinsic_correct", None) \
                or lidar_ops._kept_original("intrinsic_correct")
            self.cur_point_cloud_torch = correct(self.cur_point_cloud_torch, cfg.correction_deg)
        if cfg.deskew:
            if frame_id == 0:
                continue                            # as the reference: the first frame has no motion to deskew with
            self.deskew_at_frame(self.get_tran_in_frame(frame_id, use_gt_pose))
        cloud = self.cur_point_cloud_torch.to(volume.device, torch.float32)
        idx = neural_map.voxel_down_sample(cloud[:, :3], down_vox_m)
        cloud, = lidar_ops.select_rows(idx, cloud)
        keep = lidar_ops.crop_rows(cloud, cfg.min_z, cfg.max_z, cfg.min_range, cfg.max_range, cfg.range_filter_2d)
        cloud, = lidar_ops.select_rows(keep, cloud)
        if use_gt_pose and self.gt_pose_provided:
            pose = self.gt_poses[frame_id]
        elif cfg.pgo_on:
            pose = self.pgo_poses[frame_id]
        elif cfg.track_on:
            pose = self.odom_poses[frame_id]
        elif self.gt_pose_provided:
            pose = self.gt_poses[frame_id]
        else:
            raise _lib.PingsHipError("lidar_tsdf_fusion: the dataset has no pose for the frame")
        pose = torch.as_tensor(np.asarray(pose, dtype=np.float64), device=volume.device)
        world = (cloud[:, :3].double() @ pose[:3, :3].T + pose[:3, 3]).float().contiguous()
        cols = cloud[:, 3:6].contiguous() if color else None
        volume.integrate_points(world, pose[:3, 3], cols, space_carving=space_carving, sdf_mode=sdf_mode,
                                max_range=reach if space_carving else math.inf)
    mesh = volume.extract_mesh()
    if output_path is not None:
        mesh_ops.write_ply(str(output_path), mesh.verts, mesh.faces, mesh.normals, mesh.colors)
        print(f"Save the mesh resulting from LiDAR TSDF fusion to {output_path}")
    try:
        import open3d  # noqa: F401
    except ImportError:
        return mesh
    return mesh_ops.to_open3d(mesh)


def install(slam_dataset_module, lidar=False) -> None:
    """`import dataset.slam_dataset as D; install(D)`: SLAMDataset.o3d_tsdf_fusion -> the fusion above.  With
    `lidar=True` the class also gets `lidar_tsdf_fusion`, a method the reference does not have."""
    slam_dataset_module.SLAMDataset.o3d_tsdf_fusion = o3d_tsdf_fusion
    if lidar:
        slam_dataset_module.SLAMDataset.lidar_tsdf_fusion = lidar_tsdf_fusion
