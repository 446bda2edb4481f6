"""Time view evaluation on the device (`pings_amd.eval_ops`, csrc/eval.hip).

Host clock around synchronised calls after warm-up; per stage: wall time (median, min), host reads per call
(`_lib.sync_counts`), launches of the library's own kernels per call (the rocPRIM sort and scan launches show in the
kernel trace), and the bytes the stage must move (inputs read once, outputs written once) for the roofline against
kernel times from a separate `rocprofv3 --kernel-trace --stats` run.

  shapes   view   a 1920 x 1080 synthetic street depth image (ground, two facades, a far wall) back-projected, against
                  a 120,000-point lidar-like cloud of the same surfaces, at 0.05 / 0.1 / 1.0 (the mapper's call)
           mesh   2 M against 2 M points of a wavy surface at eval_mesh's 0.02 / 0.05 / 0.5
  baselines, same run
           (a) host   the fp64 restatement (tests/eval_ref.py) with cKDTree.query(workers=16)
           (b) brute  chunked torch.cdist(...).min on the device over the same down-sampled clouds, both directions;
                      with --brute-queries N only the first N queries of each direction are timed and the figure is
                      scaled to all of them (recorded as such)
The device figures are also checked against (a) at the timed sizes with the tolerances of tests/test_eval_gpu.py and
the differences recorded.

    python tools/eval_time.py [--iters 5] [--warmup 2] [--shapes view,mesh] [--no-baselines]
                              [--out profiles/eval/eval_time.json]
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
sys.path.insert(0, str(ROOT / "tests"))

import eval_ref  # noqa: E402
from pings_amd import _lib, eval_ops as EO  # noqa: E402

H, W = 1080, 1920
K = (1000.0, 1000.0, 959.5, 539.5)
OWN_LAUNCHES = {"view_metrics": 2, "backproject": 2, "voxel_centroids": 6, "nn_distance": 5, "eval_pair": 2 * 6 + 2 * 5 + 1}


def street_depth(rng, noise=0.01):
    """Depth of a camera 1.6 m above a road between two facades 6 m to either side, a wall 45 m ahead, sky = 0."""
    v, u = np.mgrid[0:H, 0:W]
    rx, ry = (u - K[2]) / K[0], (v - K[3]) / K[1]
    with np.errstate(divide="ignore"):
        ground = np.where(ry > 0, 1.6 / ry, np.inf)
        side = np.where(rx != 0, 6.0 / np.abs(rx), np.inf)
    z = np.minimum(np.minimum(ground, side), 45.0)
    top = (z * -ry) > 9.0                        # facades 9 m high, sky above
    z = z + rng.normal(0, noise, z.shape) * (z / 10.0)
    z[top] = 0.0
    return z.astype(np.float32)


def extrinsic():
    E = np.eye(4)
    a = 0.3
    E[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    E[:3, 3] = -E[:3, :3] @ np.array([40.0, -25.0, 3.0])
    return E


def wavy(rng, n, noise):
    xy = rng.uniform([0.0, 0.0], [40.0, 25.0], (n, 2))
    z = 0.5 * np.sin(0.7 * xy[:, 0]) * np.cos(0.9 * xy[:, 1]) + rng.normal(0, noise, n)
    return (np.column_stack([xy, z]) + [40.0, -25.0, 3.0]).astype(np.float32)


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


def brute_min(src, dst, chunk_elems=2 ** 28):
    """Nearest-neighbour distance by brute force, what a user writes today: chunked torch.cdist(...).min."""
    step = max(1, chunk_elems // max(dst.shape[0], 1))
    return torch.cat([torch.cdist(src[i:i + step], dst).min(1).values for i in range(0, src.shape[0], step)])


def pair_entry(name, pred, trgt, kw, iters, warmup, brute_queries, baselines=True):
    res, thr, tacc, tcom = kw["down_sample_res"], kw["threshold"], kw["truncation_acc"], kw["truncation_com"]
    e = {"pred_points": int(pred.shape[0]), "trgt_points": int(trgt.shape[0]), **kw}
    P, t = timed(lambda: EO.voxel_centroids(pred, res), iters, warmup)
    T = EO.voxel_centroids(trgt, res)
    n, m = int(P.shape[0]), int(T.shape[0])
    e["pred_cells"], e["trgt_cells"] = n, m
    e["voxel_centroids_pred"] = {**t, "own_launches": OWN_LAUNCHES["voxel_centroids"],
                                 "bytes_moved": int(pred.shape[0]) * (3 * 12 + 2 * 12) + n * 12}
    cell = EO.default_cell(tacc, res)
    (d, _), t = timed(lambda: EO.nn_distance(P, T, tacc, cell=cell), iters, warmup)
    e["nn_distance_pred_to_trgt"] = {**t, "cell": cell, "own_launches": OWN_LAUNCHES["nn_distance"],
                                     "bytes_moved": m * (2 * 12 + 2 * 12 + 24) + n * (12 + 12)}
    got, t = timed(lambda: EO.eval_pair(pred, trgt, **kw), iters, warmup)
    e["eval_pair"] = {**t, "own_launches": OWN_LAUNCHES["eval_pair"], "metrics": got}
    print(name, "device", json.dumps(e), flush=True)
    if not baselines:
        return e

    # (b) brute force on the device over the same centroids, both directions
    nq = min(brute_queries, n, m) if brute_queries else 0
    sp, st = (P[:nq], T[:nq]) if nq else (P, T)
    (bp, br), t = timed(lambda: (brute_min(sp, T), brute_min(st, P)), 1, 1)
    scale = (n + m) / (sp.shape[0] + st.shape[0])
    e["baseline_brute_cdist"] = {"wall_ms": round(t["wall_ms_median"] * scale, 1), "queries_timed": [int(sp.shape[0]), int(st.shape[0])],
                                 "scaled_to_all_queries": bool(nq), "nn_vs_brute_max_abs_diff":
                                 float((torch.where(torch.isinf(d[:sp.shape[0]]), bp, d[:sp.shape[0]]) - bp).abs().max())}
    print(name, "brute", json.dumps(e["baseline_brute_cdist"]), flush=True)

    # (a) the restatement on the host, and the check of the device figures against it
    eval_ref.WORKERS = 16
    ph, th = pred.cpu().numpy(), trgt.cpu().numpy()
    t0 = time.perf_counter()
    want, (dp, dr) = eval_ref.eval_pair(ph, th, **kw, details=True)
    host_ms = 1e3 * (time.perf_counter() - t0)
    A = int(sum((np.abs(x[np.isfinite(x)] - lim) < 1e-4).sum() for x in (dp, dr) for lim in (thr, tacc, tcom)))
    n_p, n_r = int(np.isfinite(dp).sum()), len(dr)
    diffs, ok = {}, len(dp) == n and len(dr) == m
    for k in eval_ref.KEYS[:7]:
        diffs[k] = {"device": got[k], "host_fp64": want[k], "abs_diff": abs(got[k] - want[k])}
    for k, cnt in (("MAE_accuracy(m)", n_p), ("MAE_completeness(m)", n_r), ("Chamfer_L2(m)", min(n_p, n_r))):
        ok = ok and diffs[k]["abs_diff"] <= 1e-5 * want[k] + A * max(tacc, tcom) / max(cnt, 1)
    for k, cnt in (("Precision[Accuracy](%)", n_p), ("Recall[Completeness](%)", n_r)):
        ok = ok and diffs[k]["abs_diff"] <= 100.0 * (A / max(cnt, 1) + A / max(cnt - A, 1)) + 1e-9
    e["baseline_host_ckdtree"] = {"wall_ms": round(host_ms, 1), "workers": 16, "cells": [len(dp), len(dr)]}
    e["check_against_host"] = {"undecided_distances_A": A, "within_tolerance": bool(ok), "figures": diffs}
    print(name, "host", json.dumps(e["baseline_host_ckdtree"]), json.dumps(e["check_against_host"]), flush=True)
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="view,mesh")
    ap.add_argument("--brute-queries", type=int, default=65536, help="mesh shape only; 0 = all queries")
    ap.add_argument("--no-baselines", action="store_true", help="device stages only (for a profiler run)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    out = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup}
    shapes = a.shapes.split(",")
    if "view" in shapes:
        depth_h = street_depth(rng)
        E = extrinsic()
        depth = torch.from_numpy(depth_h).to(dev)[None]
        rgb = torch.rand(3, H, W, device=dev)
        gt = (rgb + 0.05 * torch.randn(3, H, W, device=dev)).clamp(0, 1)
        gtd = depth + 0.05 * torch.randn(1, H, W, device=dev)
        alpha = torch.rand(1, H, W, device=dev)
        v = {"image": [H, W]}
        for ssim in (False, True):
            m, t = timed(lambda: EO.view_metrics(rgb, gt, depth, gtd, alpha, depth_min=0.5, depth_max=40.0,
                                                 min_alpha=0.1, ssim=ssim), a.iters, a.warmup)
            v["view_metrics_ssim" if ssim else "view_metrics"] = {
                **t, "own_launches": OWN_LAUNCHES["view_metrics"], "bytes_moved": 4 * H * W * 9, "metrics": list(m)}
        want = eval_ref.view_metrics(rgb.cpu().numpy(), gt.cpu().numpy(), depth.cpu().numpy(), gtd.cpu().numpy(),
                                     alpha.cpu().numpy(), depth_min=0.5, depth_max=40.0, min_alpha=0.1)
        v["check_against_host"] = {"psnr": [m.psnr, want["psnr"]], "depth_l1": [m.depth_l1, want["depth_l1"]],
                                   "depth_rmse": [m.depth_rmse, want["depth_rmse"]], "n_valid": [m.n_valid, want["n_valid"]]}
        (pts, col), t = timed(lambda: EO.backproject_depth(depth, K, E, 40.0, rgb=rgb), a.iters, a.warmup)
        v["backproject"] = {**t, "own_launches": OWN_LAUNCHES["backproject"], "points": int(pts.shape[0]),
                            "bytes_moved": 4 * H * W * 5 + int(pts.shape[0]) * 24}
        wp, _, _ = eval_ref.backproject_depth(depth_h, K, E, 40.0)
        v["backproject"]["check_against_host"] = {"points": [int(pts.shape[0]), len(wp)], "max_abs_diff":
                                                  float(np.abs(pts.cpu().numpy() - wp).max()) if len(wp) == pts.shape[0] else None}
        print("view", json.dumps(v), flush=True)
        lidar = wp[rng.choice(len(wp), 120000, replace=False)] + rng.normal(0, 0.02, (120000, 3))
        trgt = torch.from_numpy(lidar.astype(np.float32)).to(dev)
        v["pair"] = pair_entry("view", pts.contiguous(), trgt, dict(down_sample_res=0.05, threshold=0.1, truncation_acc=1.0,
                                                                   truncation_com=1.0), a.iters, a.warmup, 0, not a.no_baselines)
        out["view"] = v
        del depth, rgb, gt, gtd, alpha, pts, col, trgt
        torch.cuda.empty_cache()
    if "mesh" in shapes:
        pred = torch.from_numpy(wavy(rng, 2_000_000, 0.01)).to(dev)
        trgt = torch.from_numpy(wavy(rng, 2_000_000, 0.0)).to(dev)
        out["mesh"] = {"pair": pair_entry("mesh", pred, trgt, dict(down_sample_res=0.02, threshold=0.05, truncation_acc=0.5,
                                                                  truncation_com=0.5), a.iters, a.warmup, a.brute_queries,
                                           not a.no_baselines)}
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
