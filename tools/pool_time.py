"""Wall time, launches and host waits of the four sample-pool functions against their torch transcription.

For `sample`, `get_batch`, `transform_data_pool` and `window_rows` of pings_amd/pool_ops.py, each next to the float32
torch transcription of the reference (tests/pool_ref.py, with the reference's random draws inside the timed call), on
the device, at the shape of the reference's defaults: 120,000 points with S = 6 (3 surface, 2 front, 0 behind samples),
a pool of 10^7 rows with about 2*10^6 rows in the window, bs = 16,384 with bs_new_sample = 2,048, 2,000 poses;
`get_batch` also at bs = 131,072.

Wall time: the two versions alternate inside one loop after a warm-up, a synchronise on both sides of every call;
median and minimum over --iters calls.  Host waits and launches: the helpers of tools/pose_step_time.py
(`torch.cuda.set_sync_debug_mode("warn")` plus the reads the package counts; device events of a torch.profiler pass,
taken after the timing because tracing slows the host).

    python tools/pool_time.py [--iters 20] [--pool 10000000] [--out profiles/pool/pool_time.json]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path
from types import SimpleNamespace as NS

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

RADIUS, POSES = 50.0, 2000
TORCH_READS = ("pool_transform_bounds", "pool_status")     # package-counted reads that torch sees as well


def build(pool_rows, points, dev):
    import pool_ref as PR
    from pings_amd import pool_ops

    g = torch.Generator(device=dev).manual_seed(3)
    cfg = PR.sample_cfg(3, 2, 0, True, False)
    pts, _, _, col = (None if t is None else t.to(dev) for t in PR.sample_inputs(points, 3, False, False, False, 1))
    sampler = NS(config=cfg, dev=torch.device(dev))

    def torch_sample():
        P = pts.shape[0]
        noise = (torch.randn(P * 3, 1, device=dev), torch.rand(P * 2, 1, device=dev), torch.rand(0, 1, device=dev))
        return PR.sample(cfg, pts, None, None, col, noise)

    # a cube in which a fifth of the points lies within RADIUS of its centre
    side = RADIUS * (4.18879 / 0.2) ** (1.0 / 3.0)
    origin = torch.tensor([120.0, -40.0, 3.0], device=dev)
    m = NS(global_coord_pool=origin + (torch.rand(pool_rows, 3, device=dev, generator=g) - 0.5) * side,
           sdf_label_pool=torch.randn(pool_rows, device=dev, generator=g),
           time_pool=torch.randint(0, POSES, (pool_rows,), device=dev, generator=g, dtype=torch.int32),
           weight_pool=torch.randn(pool_rows, device=dev, generator=g), normal_label_pool=None, sem_label_pool=None,
           color_pool=torch.rand(pool_rows, 3, device=dev, generator=g), pool_sample_count=pool_rows,
           device=torch.device(dev), dataset=NS(lose_track=False, stop_status=False))
    m.local_sample_indices = pool_ops.window_rows(m.global_coord_pool, origin, RADIUS, False)
    m.new_idx = torch.arange(max(0, pool_rows - points * 6), pool_rows, device=dev)[::3].contiguous()
    pose = PR.rigid_poses(POSES, torch.float32, seed=4).to(dev)     # the mapper's dtype: [N,4,4] is 640 MB
    pose[:, :3, 3] *= 0.01          # the pool is transformed again and again: keep it near the window

    def torch_batch():
        (nh, hh), (nn, hn) = PR.draw_sizes(m)
        return PR.get_batch(m, torch.randint(0, hh, (nh,), device=dev), torch.randint(0, hn, (nn,), device=dev))

    def torch_transform():
        m.global_coord_pool = PR.transform(m.global_coord_pool, m.time_pool, pose)

    def torch_window():
        rel = m.global_coord_pool - origin
        return torch.nonzero(torch.norm(rel, p=2, dim=1) < RADIUS).squeeze()

    def with_bs(fn, bs):
        def f():
            m.config = NS(bs=bs, bs_new_sample=2048)
            return fn()
        return f

    pairs = {
        "sample": (lambda: pool_ops.sample(sampler, pts, None, None, col), torch_sample),
        "get_batch_bs16384": (with_bs(lambda: pool_ops.get_batch(m), 16384), with_bs(torch_batch, 16384)),
        "get_batch_bs131072": (with_bs(lambda: pool_ops.get_batch(m), 131072), with_bs(torch_batch, 131072)),
        "transform_data_pool": (lambda: pool_ops.transform_data_pool(m, pose), torch_transform),
        "window_rows": (lambda: pool_ops.window_rows(m.global_coord_pool, origin, RADIUS, False), torch_window),
    }
    shape = {"points": points, "S": 6, "pool_rows": pool_rows, "window_rows": int(m.local_sample_indices.shape[0]),
             "new_idx_rows": int(m.new_idx.shape[0]), "bs_new_sample": 2048, "poses": POSES}
    return pairs, shape


def time_pair(ours, theirs, iters):
    for _ in range(3):
        ours()
        theirs()
    wall = ([], [])
    for _ in range(iters):
        for k, fn in enumerate((ours, theirs)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    return [{"wall_ms_median": round(statistics.median(w), 4), "wall_ms_min": round(min(w), 4)} for w in wall]


def main():
    from pose_step_time import host_waits, launches

    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--pool", type=int, default=10_000_000)
    ap.add_argument("--points", type=int, default=120_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pool_time.py measures on a HIP device; none is available")
    pairs, shape = build(a.pool, a.points, "cuda")
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "shape": shape, "calls": {}}
    nothing = lambda: None  # noqa: E731
    # torch adds a once-per-process warning about the sync debug mode itself to the first report: spend it here
    host_waits(lambda: torch.zeros(1, device="cuda").item(), nothing)

    def waits(fn):
        w = host_waits(fn, nothing)
        # reads made through torch (`.tolist()`, `.item()`) are reported by torch too: count them once
        w["total"] = w["torch_reported"] + sum(v for k, v in w["package_counted"].items() if k not in TORCH_READS)
        return w

    for name, (ours, theirs) in pairs.items():
        t_ours, t_theirs = time_pair(ours, theirs, a.iters)
        res["calls"][name] = {"pool_ops": {**t_ours, "host_waits": waits(ours)},
                              "torch": {**t_theirs, "host_waits": waits(theirs)}}
    for name, (ours, theirs) in pairs.items():
        res["calls"][name]["pool_ops"].update(launches(ours, nothing))
        res["calls"][name]["torch"].update(launches(theirs, nothing))
        print(name, json.dumps(res["calls"][name]), flush=True)
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
