"""Time LiDAR-scan fusion into the sparse TSDF volume on the device (`TSDFVolume.integrate_points`,
csrc/tsdf_points.hip).

The scan is synthetic and at street scale: a sensor 1.8 m above a ground plane between two walls 10 m to either side,
64 beams from -25 to +3 degrees by 1875 azimuths = 120,000 rows; a ray that returns nothing within 50 m is a NaN row.
voxel_length 0.1, sdf_trunc 0.4, max_range 50 m, sdf_mode "point", no colour.  Four cases: band-limited and carved,
each into a fresh volume (every touched block is new: table inserts, the sort, the growth copies) and into the volume
that already holds the blocks.

The comparison is a torch restatement in the same process, warmed: the same samples from torch ops (per axis the face
crossings of every ray as a padded [rays, faces] tensor, all of them sorted per ray, the cube at the middle of each
interval), then `index_add_` of count and value into dense accumulators over the bounding box of the device volume's
blocks, and the average.  It runs in chunks of CHUNK rays to bound its memory.  Host clock around synchronised calls after
warm-up; per entry: wall time (median, min), host reads per call (`_lib.sync_counts`), launches per call (from the
entry's code, see LAUNCHES; the torch restatement's launches are not counted).

    python tools/tsdf_points_time.py [--iters 10] [--warmup 3] [--out profiles/tsdf/tsdf_points_time.json]
"""
import argparse
import json
import math
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pings_amd import _lib, tsdf_ops  # noqa: E402

LAUNCHES = {"integrate_points": "clear counters + ray touch + (new blocks: radix sort + assign) + accumulator fill + "
                                "accumulate + apply = 5 to 7, plus one 3-float copy when the origin is a host sequence"}
BEAMS, AZIMUTHS = 64, 1875
VOXEL, TRUNC, MAX_RANGE, SENSOR_Z, WALL = 0.1, 0.4, 50.0, 1.8, 10.0
CHUNK = 20000


def scene(dev):
    el = torch.deg2rad(torch.linspace(-25.0, 3.0, BEAMS, dtype=torch.float64))
    az = torch.arange(AZIMUTHS, dtype=torch.float64) * (2.0 * math.pi / AZIMUTHS) + 0.001
    el, az = torch.meshgrid(el, az, indexing="ij")
    d = torch.stack([torch.cos(el) * torch.cos(az), torch.cos(el) * torch.sin(az), torch.sin(el)], -1).reshape(-1, 3)
    inf = torch.full_like(d[:, 0], float("inf"))
    ground = torch.where(d[:, 2] < 0, SENSOR_Z / (-d[:, 2]).clamp_min(1e-12), inf)
    wall = torch.where(d[:, 1].abs() > 0, WALL / d[:, 1].abs().clamp_min(1e-12), inf)
    s = torch.minimum(ground, wall)
    o = torch.tensor([0.0, 0.0, SENSOR_Z], dtype=torch.float64)
    pts = o + s[:, None] * d
    pts[s >= MAX_RANGE - 1.0] = float("nan")
    return pts.float().to(dev), o.float().to(dev)


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


def torch_points_integrate(state, lo, pts, o, carve):
    """The rules of §2.9b over one dense grid whose first point is grid point `lo` (in place on `state`)."""
    tsdf, weight = state
    n = tsdf.shape
    cnt, sm = torch.zeros(tsdf.numel(), device=tsdf.device), torch.zeros(tsdf.numel(), device=tsdf.device)
    faces = int(math.ceil(((MAX_RANGE if carve else 0.0) + 2.0 * TRUNC) / VOXEL)) + 2
    steps = torch.arange(faces, device=tsdf.device, dtype=torch.float32)
    lo_t = torch.tensor([float(x) for x in lo], device=tsdf.device)
    x0 = o / VOXEL + 0.5                                   # cube index = floor(x0 + s d / voxel)
    for head in range(0, pts.shape[0], CHUNK):
        p = pts[head:head + CHUNK]
        v = p - o
        r = v.norm(dim=1)
        ok = torch.isfinite(r) & (r > 0) & (r < MAX_RANGE)
        p, v, r = p[ok], v[ok], r[ok]
        d = v / r[:, None]
        dv = d / VOXEL
        s1 = (r + TRUNC)[:, None]
        s0 = torch.zeros_like(s1) if carve else (r - TRUNC).clamp_min(0.0)[:, None]
        cuts = [s0, s1]
        for a in range(3):
            xa = x0[a] + s0[:, 0] * dv[:, a]
            first = torch.where(dv[:, a] > 0, torch.ceil(xa), torch.floor(xa))
            m = first[:, None] + torch.sign(dv[:, a])[:, None] * steps
            s = (m - x0[a]) / dv[:, a, None]
            cuts.append(torch.where(torch.isfinite(s) & (s > s0) & (s < s1), s, s1))       # padding: empty intervals
        cuts = torch.cat(cuts, 1).sort(1).values
        a0, a1 = cuts[:, :-1], cuts[:, 1:]
        g = torch.floor(x0 + (0.5 * (a0 + a1))[..., None] * dv[:, None, :])
        c = g * VOXEL
        pc, co = p[:, None, :] - c, c - o
        dist = pc.norm(dim=2)
        sdf = torch.where((co * pc).sum(2) >= 0, dist, -dist)
        gi = g - lo_t
        inside = ((gi >= 0) & (gi < torch.tensor([float(x) for x in n], device=g.device))).all(2)
        upd = (a1 > a0) & (sdf > -TRUNC) & inside
        idx = ((gi[..., 0] * n[1] + gi[..., 1]) * n[2] + gi[..., 2]).long()[upd]
        cnt.index_add_(0, idx, torch.ones_like(idx, dtype=torch.float32))
        sm.index_add_(0, idx, (sdf / TRUNC).clamp_max(1.0)[upd])
    cnt, sm = cnt.view(n), sm.view(n)
    tsdf.copy_(torch.where(cnt > 0, (tsdf * weight + sm) / (weight + cnt).clamp_min(1.0), tsdf))
    weight.add_(cnt)
    return state


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda")
    pts, o = scene(dev)
    res = {"device": torch.cuda.get_device_name(0), "rows": int(pts.shape[0]),
           "valid_rows": int(torch.isfinite(pts).all(1).sum()), "voxel_length": VOXEL, "sdf_trunc": TRUNC,
           "max_range": MAX_RANGE, "sdf_mode": "point", "color": False, "launches": LAUNCHES}
    keys = []
    for name, carve in (("band", False), ("carved", True)):
        vol = tsdf_ops.TSDFVolume(VOXEL, TRUNC, color=False)
        call = lambda: vol.integrate_points(pts, o, space_carving=carve, max_range=MAX_RANGE)
        _, e = timed(call, a.iters, a.warmup, before=vol.reset)
        vol.reset()
        call()
        w = vol._weight[:vol.n_blocks]
        shape = {"blocks": vol.n_blocks, "updated_voxels": int((w > 0).sum()), "samples": int(w.sum()),
                 "store_MB": round(vol.n_blocks * 512 * 8 / 1e6, 1), "accumulators_MB": round(vol.n_blocks * 4096 / 1e6, 1),
                 "table_entries": int(vol._tkeys.shape[0])}
        res[f"{name}_fresh"] = {**e, **shape}
        _, e = timed(call, a.iters, a.warmup)
        res[f"{name}_warm"] = {**e, "blocks": vol.n_blocks}

        bc = vol.block_coords().cpu().numpy()
        lo, hi = bc.min(0) * 8, (bc.max(0) + 1) * 8
        n = [int(x) for x in hi - lo]
        state = (torch.ones(n, device=dev), torch.zeros(n, device=dev))
        _, e = timed(lambda: torch_points_integrate(state, lo, pts, o, carve), max(2, a.iters // 2), 1)
        state = (torch.ones(n, device=dev), torch.zeros(n, device=dev))
        torch_points_integrate(state, lo, pts, o, carve)
        res[f"torch_dense_{name}"] = {**e, "box": n, "voxels": n[0] * n[1] * n[2],
                                      "updated_voxels": int((state[1] > 0).sum()), "samples": int(state[1].sum())}
        keys += [f"{name}_fresh", f"{name}_warm", f"torch_dense_{name}"]
        del vol, state
        torch.cuda.empty_cache()
    for k in keys:
        print(k, json.dumps(res[k]), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
