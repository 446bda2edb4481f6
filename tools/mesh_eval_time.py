"""Time mesh scoring on the device (`mesh_ops.sample_surface`, `eval_ops.eval_mesh`; csrc/mesh_sample.hip).

The mesh is a marching-cubes surface of a wavy height field (`mesher_ops.marching_cubes`, as tools/mesh_time.py builds
its input), about 10^6 faces at the default --n, scaled to 0.05 m voxels; the target is 2 M points of the same
analytic surface.

Host clock around synchronised calls after warm-up; per entry: wall time (median, min), host reads per call
(`_lib.sync_counts`) and launches per call.  The library's launches are counted from the entry's C code (LAUNCHES);
the torch restatement's are counted by `torch.profiler` over one call when it is available.
  sample_surface   N = 1 M and 20 M, with the algorithmic bytes of the sampling kernel (12 B stored, 36 B of vertices
                   and 24 B of indices gathered, 8 log2(F) B of Q read per point) over the wall time of the whole call
  torch_sample     the same allocation written with torch operators in the same process: fp64 areas, torch.cumsum,
                   torch.searchsorted, torch.rand (float cumsum: scan-order dependent; no fused crop)
  eval_mesh        the reference's defaults (20 M samples, 0.02 / 0.05 / 0.5) against the 2 M-point target

    python tools/mesh_eval_time.py [--iters 20] [--warmup 3] [--n 720] [--out profiles/eval/mesh_eval_time.json]
"""
import argparse
import json
import math
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pings_amd import _lib, eval_ops as EO, mesh_ops, mesher_ops as MO  # noqa: E402

VOXEL = 0.05
LAUNCHES = {"sample_surface": "areas + sum-scan + sample = 3 (the library scan counted as one)",
            "eval_mesh": "2 torch reductions and 4 small torch ops for the box + 3 of the sampler + 23 of eval_pair "
                         "(2 x 6 voxel, 2 x 5 search, 1 reduce)"}


def height(x, y):
    return 0.6 + 0.35 * torch.sin(0.45 * x) * torch.cos(0.6 * y)


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
    return out, {"wall_ms_median": round(1e3 * statistics.median(ts), 3), "wall_ms_min": round(1e3 * min(ts), 3),
                 "host_reads_per_call": reads}


def torch_sample(verts, faces, n):
    t = verts[faces].double()
    area = 0.5 * torch.linalg.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]).norm(dim=1)
    cdf = torch.cumsum(area, 0)
    bound = torch.round(cdf * (n / cdf[-1]))
    tri = torch.searchsorted(bound, torch.arange(n, device=verts.device, dtype=torch.float64), right=True)
    tri.clamp_(max=faces.shape[0] - 1)
    u = torch.rand(n, 2, device=verts.device, dtype=torch.float64)
    s = u[:, 0].sqrt()
    tv = verts[faces[tri]].double()
    p = (1 - s)[:, None] * tv[:, 0] + (s * (1 - u[:, 1]))[:, None] * tv[:, 1] + (s * u[:, 1])[:, None] * tv[:, 2]
    return p.float()


def kernel_launches(fn):
    """Device kernels of one call, by torch.profiler; None where the profiler is not usable."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "Memcpy" not in e.name
                and "Memset" not in e.name)
        return n or None
    except Exception as e:   # noqa: BLE001
        print("torch.profiler not usable:", type(e).__name__, e, flush=True)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=720, help="grid points per horizontal axis of the height field")
    ap.add_argument("--target", type=int, default=2_000_000)
    ap.add_argument("--no-profiler", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda")
    n, nz = a.n, 24
    ax = torch.arange(n, device=dev, dtype=torch.float32) * VOXEL
    az = torch.arange(nz, device=dev, dtype=torch.float32) * VOXEL
    X, Y, Z = torch.meshgrid(ax, ax, az, indexing="ij")
    verts, faces = MO.marching_cubes(Z - height(X, Y))
    del X, Y, Z
    verts = (verts * VOXEL).contiguous()
    F, V = int(faces.shape[0]), int(verts.shape[0])
    g = torch.Generator(device="cpu").manual_seed(0)
    xy = torch.rand(a.target, 2, generator=g).to(dev) * ((n - 1) * VOXEL)
    target = torch.cat([xy, height(xy[:, 0:1], xy[:, 1:2])], 1).contiguous()
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "faces": F, "verts": V,
           "target_points": int(target.shape[0]), "launches": LAUNCHES}
    print(json.dumps({k: res[k] for k in ("faces", "verts", "target_points")}), flush=True)

    for N in (1_000_000, 20_000_000):
        s, e = timed(lambda: mesh_ops.sample_surface(verts, faces, N), a.iters, a.warmup)
        assert int(s.count.item()) == N and int(s.status.item()) == 0
        per_point = 12 + 36 + 24 + 8 * math.log2(F)
        mesh_pass = F * (24 + 36 + 8 + 16)                  # areas: indices, vertices, q out; scan: q in, Q out
        alg = N * per_point + mesh_pass
        e.update(own_launches=3, algorithmic_bytes=int(alg), stored_bytes=12 * N,
                 achieved_GBps_algorithmic=round(alg / (e["wall_ms_median"] * 1e-3) / 1e9, 1),
                 achieved_GBps_stored=round(12 * N / (e["wall_ms_median"] * 1e-3) / 1e9, 1))
        res[f"sample_surface_{N // 1_000_000}M"] = e
        print("sample_surface", N, json.dumps(e), flush=True)
        del s
        _, t = timed(lambda: torch_sample(verts, faces, N), a.iters, a.warmup)
        res[f"torch_sample_{N // 1_000_000}M"] = t
        print("torch_sample", N, json.dumps(t), flush=True)
        torch.cuda.empty_cache()

    m, e = timed(lambda: EO.eval_mesh((verts, faces), target), a.iters, a.warmup)
    e.update(mesh_sample_point=20_000_000, metrics=m)
    res["eval_mesh_defaults"] = e
    print("eval_mesh", json.dumps(e), flush=True)
    # what scoring the vertex list gives on the same inputs (the figure reported before eval_mesh existed)
    res["eval_pair_of_vertices"] = {"metrics": EO.eval_pair(verts, target)}
    print("eval_pair(verts)", json.dumps(res["eval_pair_of_vertices"]), flush=True)

    def write():
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text(json.dumps(res, indent=1) + "\n")

    write()
    if not a.no_profiler:        # last, and after the figures are on disk: the count does not depend on N
        res["torch_sample_kernel_launches"] = kernel_launches(lambda: torch_sample(verts, faces, 1_000_000))
        res["sample_surface_kernel_launches"] = kernel_launches(lambda: mesh_ops.sample_surface(verts, faces, 1_000_000))
        print("launches", res["torch_sample_kernel_launches"], res["sample_surface_kernel_launches"], flush=True)
        write()


if __name__ == "__main__":
    main()
