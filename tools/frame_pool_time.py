"""Wall time, launches, device time and host waits of the pool part of `process_frame` against its torch transcription.

`append_frame`, `filter_pool` and the two followed by `window_rows` (pings_amd/pool_ops.py), each next to the float32
torch transcription of the reference's lines (tests/frame_pool_ref.py, utils/mapper.py:340-438, with the reference's
`randint` inside the timed call), on the device, at the shape of the reference's defaults: a frame of 720,000 sample
rows onto a pool of 10^7 rows with RGB colour and no normals, `pool_capacity` 10^7, so that the filter runs at
1.072 * 10^7 rows.

Every call starts from the same pool: the preparation (re-pointing views or attributes, no launch) is outside the timed
region.  Wall time: the two versions alternate inside one loop after a warm-up, a synchronise on both sides of every
call; median and minimum over --iters calls.  Host waits and launches: the helpers of tools/pose_step_time.py.  No time
is a gate.

    python tools/frame_pool_time.py [--iters 20] [--pool 10000000] [--rows 720000] [--out profiles/pool/frame_pool_time.json]
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

RADIUS = 50.0
NAMES = ("global_coord_pool", "sdf_label_pool", "weight_pool", "time_pool", "color_pool")


def build(pool_rows, rows, dev):
    import frame_pool_ref as FR
    import pool_ref as PR
    from pings_amd import pool_ops

    g = torch.Generator(device=dev).manual_seed(3)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    origin = torch.tensor([120.0, -40.0, 3.0], device=dev)
    side = RADIUS * (4.18879 / 0.2) ** (1.0 / 3.0)      # a fifth of the pool lies in the window
    base = dict(global_coord_pool=origin + (torch.rand(pool_rows, 3, device=dev, generator=g) - 0.5) * side,
                sdf_label_pool=r(pool_rows), weight_pool=r(pool_rows),
                time_pool=torch.randint(0, 100, (pool_rows,), device=dev, generator=g, dtype=torch.int32),
                color_pool=torch.rand(pool_rows, 3, device=dev, generator=g))
    frame = (r(rows, 3) * 20.0, r(rows) * 0.3, None, None, torch.rand(rows, 3, device=dev, generator=g), r(rows))
    pose = PR.rigid_poses(1, torch.float64, seed=4)[0].to(dev)
    pose[:3, 3] = origin.double()
    cfg = NS(pool_capacity=pool_rows)

    def state():
        return NS(config=cfg, device=torch.device(dev), cur_sample_count=rows, pool_sample_count=pool_rows,
                  sem_label_pool=None, normal_label_pool=None, **base)

    # the library's mapper: the store's front set holds the pool and one frame behind it
    mo = state()
    store = pool_ops.pool_store(mo)
    store.adopt(mo, room=rows)
    pool_ops.append_frame(mo, *frame, pose, 100)
    store.reserve(store.capacity, back=True)
    # the transcription's mapper: the base tensors, and the same pool one frame later
    mt = state()
    FR.append(mt, *frame, pose, 100)
    full = {k: getattr(mt, k) for k in NAMES}

    def ours_at(n):
        def prep():
            store.rows = n
            store.publish(mo)
            mo.cur_sample_count = rows
        return prep

    def theirs_at(tensors):
        def prep():
            for k in NAMES:
                setattr(mt, k, tensors[k])
            mt.cur_sample_count = rows
        return prep

    def torch_filter():
        n = mt.global_coord_pool.shape[0]
        FR.filter_pool(mt, torch.randint(0, n, (n - cfg.pool_capacity,), device=dev))

    def torch_window():
        rel = mt.global_coord_pool - origin
        return torch.nonzero(torch.norm(rel, p=2, dim=1) < RADIUS).squeeze()

    def ours_all():
        pool_ops.append_frame(mo, *frame, pose, 100)
        pool_ops.filter_pool(mo)
        return pool_ops.window_rows(mo.global_coord_pool, origin, RADIUS, False)

    def torch_all():
        FR.append(mt, *frame, pose, 100)
        torch_filter()
        return torch_window()

    calls = {
        "append_frame": ((ours_at(pool_rows), lambda: pool_ops.append_frame(mo, *frame, pose, 100)),
                         (theirs_at(base), lambda: FR.append(mt, *frame, pose, 100))),
        "filter_pool": ((ours_at(pool_rows + rows), lambda: pool_ops.filter_pool(mo)),
                        (theirs_at(full), torch_filter)),
        "pool_part_of_process_frame": ((ours_at(pool_rows), ours_all), (theirs_at(base), torch_all)),
    }
    shape = {"pool_rows": pool_rows, "frame_rows": rows, "pool_capacity": pool_rows, "colour_channels": 3,
             "bytes_per_row": 36, "store_capacity_rows": store.capacity}
    return calls, shape


def time_pair(ours, theirs, iters):
    for _ in range(3):
        for prep, fn in (ours, theirs):
            prep()
            fn()
    wall = ([], [])
    for _ in range(iters):
        for k, (prep, fn) in enumerate((ours, theirs)):
            prep()
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
    ap.add_argument("--rows", type=int, default=720_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frame_pool_time.py measures on a HIP device; none is available")
    calls, shape = build(a.pool, a.rows, "cuda")
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "shape": shape, "calls": {}}
    nothing = lambda: None  # noqa: E731
    host_waits(lambda: torch.zeros(1, device="cuda").item(), nothing)    # torch's once-per-process warning

    def both(pair):                                     # the preparation launches nothing and waits for nothing
        prep, fn = pair
        return lambda: (prep(), fn())

    for name, (ours, theirs) in calls.items():
        t_ours, t_theirs = time_pair(ours, theirs, a.iters)
        res["calls"][name] = {"pool_ops": {**t_ours, "host_waits": host_waits(both(ours), nothing)},
                              "torch": {**t_theirs, "host_waits": host_waits(both(theirs), nothing)}}
    for name, (ours, theirs) in calls.items():
        res["calls"][name]["pool_ops"].update(launches(both(ours), nothing))
        res["calls"][name]["torch"].update(launches(both(theirs), nothing))
        print(name, json.dumps(res["calls"][name]), flush=True)
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
