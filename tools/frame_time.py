"""Wall time, launches and host waits of the per-frame point tests against their torch transcription.

For `new_samples`, `dynamic_filter` (type 2 on and off), `dynamic_filter_neural_points` and
`check_invalid_neural_points` of pings_amd/frame_ops.py, each next to the float32 torch transcription of the reference's
lines (tests/frame_ref.py) on the device with this package's installs underneath it: the map's `query_feature` and
`radius_neighborhood_search` are the ones of pings_amd/neural_points.py, the decoder's `sdf` the one of
pings_amd/decoder.py.  Shapes: a map of 10^6 neural points (all local), 120,000 x 6 new samples, 120,000 frame points,
about 500,000 stable rows; `dynamic_filter_neural_points` queries the 10^6 local points.

Wall time: the two versions alternate inside one loop after a warm-up, a synchronise on both sides of every call;
median and minimum over --iters calls.  Host waits and launches: the helpers of tools/pose_step_time.py, taken after the
timing because tracing slows the host.  No time is a gate.

    python tools/frame_time.py [--iters 20] [--map 1000000] [--out profiles/frame/frame_time.json]
"""
import argparse
import json
import sys
from pathlib import Path
from types import SimpleNamespace as NS

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

TORCH_READS = ("mask_rows_count_torch",)     # no package-counted read of these calls goes through torch


def build(map_points, points, samples_per_point, dev):
    import frame_ref as FR
    from oracle import sdf_cpu
    from pings_amd import decoder as hdec
    from pings_amd import frame_ops
    from pings_amd import neural_points as hnp

    class Map(sdf_cpu.NeuralPointMap):            # the oracle's attribute set with the package's query path installed
        query_feature = hnp.query_feature
        radius_neighborhood_search = hnp.radius_neighborhood_search

    class Dec:                                    # duck-typed `Decoder` with `decoder.install` applied
        def __init__(self, st):
            t = lambda k: torch.as_tensor(st["dec." + k]).to(dev)  # noqa: E731
            self.layers = [NS(weight=t("layers.0.weight"), bias=t("layers.0.bias"))]
            self.lout = NS(weight=t("lout.weight"), bias=t("lout.bias"))
            self.sdf_scale, self.use_leaky_relu = float(st["sdf_scale"]), False

        def sdf(self, features):
            return hdec.sdf(self, features)

    st, dec_st = sdf_cpu.synthetic_map(map_points)
    n = st["neural_points"].shape[0]
    g = torch.Generator().manual_seed(5)
    st["point_certainties"] = (torch.rand(n, generator=g) * 2.0).numpy()
    st["local_point_certainties"] = torch.where(torch.rand(n, generator=g) < 0.5, 4.0, 0.25).float().numpy()
    cfg = NS(voxel_size_m=float(st["resolution"]), new_certainty_thre=1.0, surface_sample_range_m=0.25,
             dynamic_certainty_thre=1.0, dynamic_sdf_ratio_thre=0.0, dynamic_min_grad_norm_thre=0.05, infer_bs=131072,
             weighted_first=bool(st["weighted_first"]), query_nn_k=int(st["nn_k"]), layer_norm_on=False, num_nei_cells=2,
             search_alpha=0.8, **FR.ADAPTIVE)
    npm = Map({**st}, device=dev)
    npm.config = cfg
    npm.color_feature_dim = 0
    npm.local_valid_gs_mask = torch.ones(n, dtype=torch.bool, device=dev)
    npm.local_mask = torch.ones(n + 1, dtype=torch.bool, device=dev)
    npm._local_idx = torch.arange(n + 1, device=dev)
    coord, label = FR.frame_samples(st, points * samples_per_point, seed=1)
    m = FR.stand_in(npm, Dec(dec_st), cfg, device=dev,
                    **{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in FR.pool_of(coord, label, 0).items()})
    x = FR.frame_points(st, points, seed=2).to(dev)

    def torch_check():
        FR.check_invalid_neural_points(m)
        npm._pings_table_gen = getattr(npm, "_pings_table_gen", 0) + 1     # what the masked write needs under our index

    pairs = {
        "new_samples": (lambda: frame_ops.new_samples(m, 0), lambda: FR.new_samples(m, 0)),
        "dynamic_filter_type2": (lambda: frame_ops.dynamic_filter(m, x.detach().clone(), True),
                                 lambda: FR.dynamic_filter(m, x.detach().clone(), True)),
        "dynamic_filter": (lambda: frame_ops.dynamic_filter(m, x.detach().clone(), False),
                           lambda: FR.dynamic_filter(m, x.detach().clone(), False)),
        "dynamic_filter_neural_points": (lambda: frame_ops.dynamic_filter_neural_points(m),
                                         lambda: FR.dynamic_filter_neural_points(m)),
        "check_invalid_neural_points": (lambda: frame_ops.check_invalid_neural_points(m), torch_check),
    }
    shape = {"map_points": n, "new_samples": int(coord.shape[0]), "frame_points": points,
             "stable_rows": int((npm.local_point_certainties > 1.0).sum()), "infer_bs": cfg.infer_bs}
    return pairs, shape


def main():
    from pool_time import time_pair
    from pose_step_time import host_waits, launches

    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--map", type=int, default=1_000_000)
    ap.add_argument("--points", type=int, default=120_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frame_time.py measures on a HIP device; none is available")
    pairs, shape = build(a.map, a.points, 6, "cuda")
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "shape": shape, "calls": {}}
    nothing = lambda: None  # noqa: E731
    # torch adds a once-per-process warning about the sync debug mode itself to the first report: spend it here
    host_waits(lambda: torch.zeros(1, device="cuda").item(), nothing)

    def waits(fn):
        w = host_waits(fn, nothing)
        w["total"] = w["torch_reported"] + sum(v for k, v in w["package_counted"].items() if k not in TORCH_READS)
        return w

    for name, (ours, theirs) in pairs.items():
        t_ours, t_theirs = time_pair(ours, theirs, a.iters)
        res["calls"][name] = {"frame_ops": {**t_ours, "host_waits": waits(ours)},
                              "torch": {**t_theirs, "host_waits": waits(theirs)}}
        print(name, json.dumps(res["calls"][name]), flush=True)
    for name, (ours, theirs) in pairs.items():
        res["calls"][name]["frame_ops"].update(launches(ours, nothing))
        res["calls"][name]["torch"].update(launches(theirs, nothing))
        print(name, json.dumps(res["calls"][name]), flush=True)
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
