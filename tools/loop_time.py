"""Wall time, launches and host waits of one `detect_global_loop`-shaped call against its torch transcription.

The call is what `NeuralPointMapContextManager.detect_global_loop` does on a frame with candidates: `set_virtual_node`
on the local map (2 * 5 + 1 poses) followed by `detect_loop`.  Ours: the methods of pings_amd/loop_ops.py rebound onto a
manager class.  Theirs: the float32 torch transcription of the reference (tests/loop_ref.py) on the same device, in the
same process.  Defaults: a local map of 10^5 points with 8 features, 11 poses, 1,000 candidate nodes, descriptors
[20,60], features on.  Both thresholds are opened, so that every call runs the ring-key search AND the shift search.

Wall time: the two versions alternate inside one loop after a warm-up, a synchronise on both sides of every call;
median and minimum over --iters calls.  Host waits and launches: the helpers of tools/pose_step_time.py, taken after the
timing because tracing slows the host.  No time is a gate.

    python tools/loop_time.py [--iters 20] [--points 100000] [--nodes 1000] [--out profiles/loop/loop_time.json]
"""
import argparse
import json
import sys
import types
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))


def build(points, nodes, use_feature, dev):
    import loop_ref as LR
    from pings_amd import loop_ops

    mod = types.SimpleNamespace(
        ptcloud2sc_torch=LR.ptcloud2sc_torch, sc2rk=LR.sc2rk, distance_sc_torch=LR.distance_sc_torch,
        distance_sc_feature_torch=LR.distance_sc_feature_torch,
        NeuralPointMapContextManager=type("NeuralPointMapContextManager", (LR.NeuralPointMapContextManager,), {}))
    loop_ops.install(mod)
    cfg = LR.make_config(device=dev, end_frame=nodes + 1, loop_with_feature=use_feature, local_map_context=True)
    ours, theirs = mod.NeuralPointMapContextManager(cfg), LR.NeuralPointMapContextManager(cfg)
    for m in (ours, theirs):                         # both gates open: every call runs the shift search as well
        m.ringkey_dist_thre, m.sc_cosdist_threshold = 1e4, 2.0
    world = LR.field(points, seed=1).to(dev)
    feats = LR.features(world, 8, seed=1).to(dev) if use_feature else None
    g = torch.Generator().manual_seed(2)
    frame = LR.pose()
    for i in range(nodes + 1):                       # node i sees a sparse part of the field from a pose of its own
        at = LR.pose(centre=(150.0 + float(torch.rand(1, generator=g)) * 40 - 20,
                             -80.0 + float(torch.rand(1, generator=g)) * 40 - 20, 3.0),
                     yaw=float(torch.rand(1, generator=g)) * 6.28) if i < nodes else frame
        pick = torch.randperm(points, generator=g)[:4000].to(dev)
        Ti = torch.linalg.inv(at).to(dev)
        cloud = (world[pick].double() @ Ti[:3, :3].T + Ti[:3, 3]).float().contiguous()
        f = feats[pick].contiguous() if use_feature else None
        for m in (ours, theirs):
            m.add_node(i, cloud, f)
    cand = np.arange(nodes)
    cur, last = frame.to(dev), LR.pose(centre=(149.0, -81.0, 3.0)).to(dev)

    def call(m):
        def run():
            m.query_contexts, m.tran_from_frame = [], []
            m.set_virtual_node(world, cur, last, feats)
            return m.detect_loop(cand, use_feature=use_feature)
        return run

    shape = {"local_map_points": points, "feature_dim": 8 if use_feature else 0, "poses": 11, "candidates": nodes,
             "context_shape": [20, 60]}
    return call(ours), call(theirs), shape


def main():
    from pool_time import time_pair
    from pose_step_time import host_waits, launches

    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--nodes", type=int, default=1000)
    ap.add_argument("--plain", action="store_true", help="descriptors without features")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loop_time.py measures on a HIP device; none is available")
    ours, theirs, shape = build(a.points, a.nodes, not a.plain, "cuda")
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "shape": shape,
           "result": {"loop_ops": str(ours()[:2]), "torch": str(theirs()[:2])}}
    nothing = lambda: None  # noqa: E731
    # torch adds a once-per-process warning about the sync debug mode itself to the first report: spend it here
    host_waits(lambda: torch.zeros(1, device="cuda").item(), nothing)
    t_ours, t_theirs = time_pair(ours, theirs, a.iters)
    res["call"] = {"loop_ops": {**t_ours, "host_waits": host_waits(ours, nothing)},
                   "torch": {**t_theirs, "host_waits": host_waits(theirs, nothing)}}
    print(json.dumps(res["call"]), flush=True)
    res["call"]["loop_ops"].update(launches(ours, nothing))
    res["call"]["torch"].update(launches(theirs, nothing))
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
