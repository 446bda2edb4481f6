"""Time device marching cubes (`mesher_ops.marching_cubes`, csrc/mc.hip) and one mesher chunk (`mesher_ops.mesh_bbx`).

Host clock around synchronised calls after warm-up; per shape: wall time (median), host reads per call
(`_lib.sync_counts`), vertex and face counts, and the bytes the kernels must move (volume and mask read twice, outputs
written once) for the roofline against kernel times from a separate `rocprofv3 --kernel-trace --stats` run.

  shapes   chunk    106 x 106 x 40, the reference's mesher chunk (split_chunks(..., mc_res_m * 100) plus padding)
           street   512 x 512 x 128: ground plane, boxes, noise
           cap      1000 x 1000 x 500 = 5e8 points, the reference's cap (get_query_from_bbx)
  mesh_bbx the gs_f32 map of tests/golden at a 3 cm voxel (fused SDF + mask query, then marching cubes)

skimage, when importable, is timed on the same host arrays; otherwise its entry reads "not measured".

    python tools/mc_time.py [--iters 10] [--warmup 3] [--skip-cap] [--out profiles/mc/mc_time.json]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path
from types import SimpleNamespace as NS

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from pings_amd import _lib, mesher_ops as MO  # noqa: E402


def street(nx, ny, nz, dev, seed=0):
    """Signed distance-like field of a street: ground at z = 0.2 nz, a few dozen boxes, small noise; built in x slabs."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    nb = 40
    lo = torch.rand(nb, 3, generator=g) * torch.tensor([nx, ny, 0.0]) + torch.tensor([0.0, 0.0, 0.2 * nz])
    size = torch.rand(nb, 3, generator=g) * torch.tensor([0.15 * nx, 0.15 * ny, 0.5 * nz]) + 4
    lo, hi = lo.to(dev), (lo + size).to(dev)
    vol = torch.empty(nx, ny, nz, device=dev)
    j = torch.arange(ny, device=dev, dtype=torch.float32)[None, :, None]
    k = torch.arange(nz, device=dev, dtype=torch.float32)[None, None, :]
    gn = torch.Generator(device=dev).manual_seed(seed)
    step = max(1, 2 ** 26 // (ny * nz))
    for x0 in range(0, nx, step):
        i = torch.arange(x0, min(nx, x0 + step), device=dev, dtype=torch.float32)[:, None, None]
        d = k - 0.2 * nz - 0.5
        for b in range(nb):
            q = torch.maximum(torch.maximum(lo[b, 0] - i, i - hi[b, 0]), torch.maximum(lo[b, 1] - j, j - hi[b, 1]))
            d = torch.minimum(d, torch.maximum(q, torch.maximum(lo[b, 2] - k, k - hi[b, 2])))
        vol[x0:x0 + d.shape[0]] = d + 0.3 * torch.rand(d.shape, generator=gn, device=dev) - 0.15
    return vol


def timed(fn, iters, warmup):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ts = []
    _lib.sync_counts(reset=True)
    for _ in range(iters):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    reads = sum(_lib.sync_counts(reset=True).values()) / iters
    return out, 1e3 * statistics.median(ts), 1e3 * min(ts), reads


def mc_entry(name, vol, mask, iters, warmup):
    (v, f), med, best, reads = timed(lambda: MO.marching_cubes(vol, 0.0, mask), iters, warmup)
    n = vol.numel()
    moved = 2 * 4 * n + (2 * n if mask is not None else 0) + v.shape[0] * (12 + 8) + f.shape[0] * 24
    e = {"shape": list(vol.shape), "points": n, "mask": mask is not None, "wall_ms_median": round(med, 3),
         "wall_ms_min": round(best, 3), "host_reads_per_call": reads, "verts": int(v.shape[0]),
         "faces": int(f.shape[0]), "bytes_moved": int(moved)}
    print(name, json.dumps(e), flush=True)
    return e


def skimage_entry(vol, mask, iters):
    try:
        from skimage import measure
    except Exception:
        return "not measured"
    a = vol.cpu().numpy()
    m = None if mask is None else mask.cpu().numpy().astype(bool)
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        measure.marching_cubes(a, level=0.0, allow_degenerate=False, mask=m)
        ts.append(time.perf_counter() - t0)
    return {"wall_ms_median": round(1e3 * statistics.median(ts), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-cap", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "marching_cubes": {}, "skimage": {}}
    shapes = {"chunk": (106, 106, 40), "street": (512, 512, 128)}
    if not a.skip_cap:
        shapes["cap"] = (1000, 1000, 500)
    for name, shp in shapes.items():
        vol = street(*shp, dev)
        mask = (torch.rand(shp, device=dev) > 0.05) if name != "cap" else None
        res["marching_cubes"][name] = mc_entry(name, vol, mask, a.iters if name != "cap" else 3, a.warmup)
        res["skimage"][name] = skimage_entry(vol, mask, 3) if name != "cap" else "not measured"
        del vol, mask
        torch.cuda.empty_cache()

    from test_sdf import _Dec, _gpu_map, load
    gd = ROOT / "tests" / "golden"
    st = load(gd, "gs_f32")
    z = np.load(gd / "mesher_grid.npz")
    fake = NS(neural_points=_gpu_map(st), sdf_mlp=_Dec(st), sem_mlp=None, color_mlp=None,
              config=NS(weighted_first=bool(st["weighted_first"]), color_channel=3, pad_voxel=1, skip_top_voxel=1,
                        infer_bs=2 ** 18, mc_mask_on=True))
    vs = 0.03
    (v, f), med, best, reads = timed(lambda: MO.mesh_bbx(fake, z["gs_f32_min"], z["gs_f32_max"], vs, mesh_min_nn=4),
                                     a.iters, a.warmup)
    _, num, _ = MO.grid_from_bbx(z["gs_f32_min"], z["gs_f32_max"], vs, 1, 1, dev)
    res["mesh_bbx"] = {"map": "gs_f32", "voxel": vs, "shape": [int(k) for k in num], "wall_ms_median": round(med, 3),
                       "wall_ms_min": round(best, 3), "host_reads_per_call": reads, "verts": int(v.shape[0]),
                       "faces": int(f.shape[0])}
    print("mesh_bbx", json.dumps(res["mesh_bbx"]), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
