"""Time sparse TSDF fusion on the device (`pings_amd.tsdf_ops`, csrc/tsdf.hip): `integrate` of one 1392x512 frame at
voxel_length 0.05, and `extract_mesh`.

The frame is analytic: a camera 1.6 m above a ground plane, looking along it at a wall 20 m ahead (fx = fy = 720), with
a smooth colour image.  `integrate` is timed twice: into a fresh volume (every touched block is new: table inserts,
the sort, the growth copies) and into the volume that already holds the blocks (the steady state of a sequence).

The comparison is a dense-grid torch restatement in the same process, warmed: the same update rule over the bounding
box of the touched blocks as one dense [nx, ny, nz] grid (every voxel of the box projected, gathered and averaged with
elementwise torch ops).  Host clock around synchronised calls after warm-up; per entry: wall time (median, min), host
reads per call (`_lib.sync_counts`), launches per call (from the entry's C code, see LAUNCHES; the torch restatement's
elementwise launches are not counted).  Achieved bandwidth is 40 B per updated voxel (tsdf, weight and three colours
read and written) over the wall time of the steady-state call, next to 512 * 40 B per touched block (what the update
kernel streams when every voxel of a touched block is updated); DESIGN §2.5e records 5.0 TB/s for a streaming
read-modify-write kernel on this device.  Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run.

    python tools/tsdf_time.py [--iters 10] [--warmup 3] [--out profiles/tsdf/tsdf_time.json]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pings_amd import _lib, tsdf_ops  # noqa: E402

LAUNCHES = {"integrate": "clear counters + touch + (new blocks: radix sort + assign) + update = 3 to 5",
            "extract_mesh": "per chunk: densify + marching cubes (count, 2 scans, totals, verts, faces) + vertices = 8; "
                            "then finish_mesh (tools/mesh_time.py)"}
H, W, FX, CX, CY = 512, 1392, 720.0, 695.5, 255.5
VOXEL, TRUNC, DEPTH_TRUNC, STRIDE = 0.05, 0.15, 25.0, 4


def scene(dev):
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    b = (v - CY) / FX                                      # camera y points down: the ground is at y = +1.6
    ground = torch.where(b > 0, 1.6 / b.clamp_min(1e-9), torch.full_like(b, float("inf")))
    depth = torch.minimum(ground, torch.full_like(b, 20.0)).float().to(dev)
    color = torch.stack([0.5 + 0.5 * torch.sin(0.01 * u), 0.5 + 0.5 * torch.cos(0.013 * v), (u + v) / (H + W)])
    return depth, color.float().to(dev)


def timed(fn, iters, warmup, before=None):
    for _ in range(warmup):
        if before:
            before()
        out = fn()
    torch.cuda.synchronize()
    ts, reads = [], 0
    for _ in range(iters):
        if before:
            before()
            torch.cuda.synchronize()
        _lib.sync_counts(reset=True)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
        reads += sum(_lib.sync_counts(reset=True).values())
    return out, {"wall_ms_median": round(1e3 * statistics.median(ts), 3), "wall_ms_min": round(1e3 * min(ts), 3),
                 "host_reads_per_call": reads / iters}


def torch_dense_integrate(state, lo, depth, color, E):
    """The update rule over one dense grid whose first point is grid point `lo` (in place on `state`)."""
    tsdf, weight, col = state
    dev = tsdf.device
    ax = [torch.arange(n, device=dev, dtype=torch.float32) + float(l) for n, l in zip(tsdf.shape, lo)]
    gx, gy, gz = torch.meshgrid(*ax, indexing="ij")
    px, py, pz = gx * VOXEL, gy * VOXEL, gz * VOXEL
    R, t = E[:3, :3], E[:3, 3]
    x = R[0, 0] * px + R[0, 1] * py + R[0, 2] * pz + t[0]
    y = R[1, 0] * px + R[1, 1] * py + R[1, 2] * pz + t[1]
    z = R[2, 0] * px + R[2, 1] * py + R[2, 2] * pz + t[2]
    fu, fv = torch.floor(FX * x / z + CX + 0.5), torch.floor(FX * y / z + CY + 0.5)
    ok = (z > 0) & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
    pix = (torch.where(ok, fv, torch.zeros_like(fv)) * W + torch.where(ok, fu, torch.zeros_like(fu))).long()
    d = depth.reshape(-1)[pix]
    ok &= torch.isfinite(d) & (d > 0) & (d < DEPTH_TRUNC)
    sdf = (d - z) * torch.sqrt(1 + ((fu - CX) / FX) ** 2 + ((fv - CY) / FX) ** 2)
    ok &= sdf > -TRUNC
    tt = torch.clamp_max(sdf / TRUNC, 1.0)
    w1 = weight + 1
    tsdf.copy_(torch.where(ok, (tsdf * weight + tt) / w1, tsdf))
    c = color.reshape(3, -1)[:, pix].permute(1, 2, 3, 0)
    col.copy_(torch.where(ok[..., None], (col * weight[..., None] + c) / w1[..., None], col))
    weight.copy_(torch.where(ok, w1, weight))
    return state


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda")
    depth, color = scene(dev)
    K = np.array([[FX, 0.0, CX], [0.0, FX, CY], [0.0, 0.0, 1.0]])
    E = np.eye(4)
    res = {"device": torch.cuda.get_device_name(0), "image": [H, W], "voxel_length": VOXEL, "sdf_trunc": TRUNC,
           "depth_trunc": DEPTH_TRUNC, "stride": STRIDE, "launches": LAUNCHES}

    vol = tsdf_ops.TSDFVolume(VOXEL, TRUNC)
    call = lambda: vol.integrate(depth, K, E, color, depth_trunc=DEPTH_TRUNC, stride=STRIDE)
    _, e = timed(call, a.iters, a.warmup, before=vol.reset)
    res["integrate_fresh"] = {**e, "blocks": vol.n_blocks}
    w0 = float(vol._weight[:vol.n_blocks].sum())
    call()
    updated = int(round(float(vol._weight[:vol.n_blocks].sum()) - w0))
    _, e = timed(call, a.iters, a.warmup)
    sec = 1e-3 * e["wall_ms_median"]
    res["integrate_steady"] = {**e, "blocks": vol.n_blocks, "updated_voxels": updated,
                               "GBps_40B_per_updated_voxel": round(40.0 * updated / sec / 1e9, 1),
                               "GBps_40B_per_touched_voxel": round(40.0 * 512 * vol.n_blocks / sec / 1e9, 1)}
    mesh, e = timed(lambda: vol.extract_mesh(), max(2, a.iters // 2), 1)
    res["extract_mesh"] = {**e, "verts": int(mesh.verts.shape[0]), "faces": int(mesh.faces.shape[0])}

    bc = vol.block_coords().cpu().numpy()
    lo, hi = bc.min(0) * 8, (bc.max(0) + 1) * 8
    n = [int(x) for x in hi - lo]
    state = (torch.ones(n, device=dev), torch.zeros(n, device=dev), torch.zeros((*n, 3), device=dev))
    Et = torch.from_numpy(E).float().to(dev)
    _, e = timed(lambda: torch_dense_integrate(state, lo, depth, color, Et), max(2, a.iters // 2), 1)
    res["torch_dense_box_integrate"] = {**e, "box": n, "voxels": int(np.prod(n)),
                                        "updated_voxels": int((state[1] > 0).sum())}
    for k in ("integrate_fresh", "integrate_steady", "extract_mesh", "torch_dense_box_integrate"):
        print(k, json.dumps(res[k]), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
