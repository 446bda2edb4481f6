"""Time the mapper's SDF-sample loss block (utils/mapper.py:836-930): the inline composition exactly as bench.py's
`bench_sdf_step` runs it (query_feature -> Decoder.sdf -> IDW sum -> boolean-mask Eikonal selection ->
get_numerical_gradient -> BCE + Eikonal, every call bound to this package) against the block
(`pings_amd.sdf_losses`), forward + backward, on the same 1M-point synthetic map and the same batch.

A second pair adds the colour term (16 colour features per point, a 19 -> 64 -> 3 colour decoder; colour labels on
every row, 20 % of them invalid): the inline side is the joint iteration's `color_feature[valid_color_mask]` ->
`regress_color` -> IDW sum -> `color_diff_loss`.  Inline and block runs alternate (`--rounds`); per run: wall time
per iteration (median of synchronised iterations), kernel-time sum and launch count (torch.profiler), host waits
(torch's sync-debug warnings).

    python tools/sdf_loss_time.py [--iters 30] [--rounds 3] [--out profiles/sdfloss/sdf_loss_time.json]
"""
import argparse
import json
import statistics
import sys
import time
import warnings
from pathlib import Path
from types import SimpleNamespace as NS

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402
from pings_amd import decoder as hdec, mapper_ops as hmap, neural_points as hnp  # noqa: E402
from pings_amd.sdf_losses import sdf_losses  # noqa: E402


def setup(dev, n_points=1_000_000, seed=0):
    npm, dec = bench.sdf_synth_map(n_points, dev)
    n = npm.local_geo_features.shape[0]
    g = torch.Generator(device=dev).manual_seed(seed)
    npm.local_geo_features = torch.nn.Parameter(npm.local_geo_features.detach().clone())
    npm.local_color_features = torch.nn.Parameter(0.1 * torch.randn(n, 16, generator=g, device=dev))
    npm.color_features = npm.local_color_features
    npm.color_feature_dim = 16
    for layer in (dec.layers[0], dec.lout):
        layer.weight, layer.bias = torch.nn.Parameter(layer.weight), torch.nn.Parameter(layer.bias)
    P = lambda *s: torch.nn.Parameter(torch.randn(*s, generator=g, device=dev) / (s[-1] ** 0.5 if len(s) > 1 else 10))
    cm = NS(layers=[NS(weight=P(64, 19), bias=P(64))], lout=NS(weight=P(3, 64), bias=P(3)), use_leaky_relu=False)
    cfg = NS(weighted_first=False, semantic_on=False, numerical_grad=True, gradient_decimation=10,
             voxel_size_m=float(npm.resolution), num_grad_step_ratio=0.2, free_sample_end_dist_m=0.5,
             surface_sample_range_m=0.5, loss_weight_on=False, ekional_loss_on=True, weight_e=0.5, weight_i=1.0,
             main_loss_type="bce")
    mapper = NS(neural_points=npm, sdf_mlp=dec, color_mlp=cm, config=cfg, dtype=torch.float32, device=dev,
                sdf_scale=float(dec.sdf_scale), require_gradient=False)
    params = [npm.local_geo_features, npm.local_color_features, dec.layers[0].weight, dec.layers[0].bias,
              dec.lout.weight, dec.lout.bias, cm.layers[0].weight, cm.layers[0].bias, cm.lout.weight, cm.lout.bias]
    return mapper, params


def batch(mapper, B, dev):
    """bench_sdf_step's batch (bench.py:807-810), plus colour labels."""
    npm = mapper.neural_points
    g = torch.Generator(device=dev).manual_seed(11)
    coord = bench.sdf_queries(npm, B, dev, seed=13)
    sdf_label = 0.25 * torch.randn(B, generator=g, device=dev)
    ts = torch.zeros(B, dtype=torch.int32, device=dev)
    weight = torch.ones(B, device=dev)
    color_label = torch.rand(B, 3, generator=g, device=dev)
    color_label[torch.rand(B, generator=g, device=dev) < 0.2, 0] = -1.0
    return coord, sdf_label, ts, weight, color_label


def inline(mapper, b, color):
    """bench.py:819-830 (and, with colour, utils/mapper.py:1503-1535's colour lines)."""
    cfg, npm, dec = mapper.config, mapper.neural_points, mapper.sdf_mlp
    coord, sdf_label, ts, weight, color_label = b
    sigma = mapper.sdf_scale
    apply_eikonal_mask = torch.abs(sdf_label) < cfg.free_sample_end_dist_m
    geo_feature, color_feature, weight_knn, _, certainty = hnp.query_feature(npm, coord, ts, query_color_feature=color)
    sdf_pred = hdec.sdf(dec, geo_feature)
    sdf_pred = torch.sum(sdf_pred * weight_knn, dim=1).squeeze(1)
    if color:
        valid_color_mask = (torch.abs(sdf_label) < 0.5 * cfg.surface_sample_range_m) & (color_label[:, 0] >= 0.0)
        cp = torch.sigmoid(hdec.mlp(mapper.color_mlp, color_feature[valid_color_mask]))
        cp = torch.sum(cp * weight_knn[valid_color_mask], dim=1)
    coord_for_eikonal = coord[apply_eikonal_mask]
    sdf_pred_for_eikonal = sdf_pred[apply_eikonal_mask]
    grad = hmap.get_numerical_gradient(mapper, coord_for_eikonal[::cfg.gradient_decimation],
                                       sdf_pred_for_eikonal[::cfg.gradient_decimation],
                                       cfg.voxel_size_m * cfg.num_grad_step_ratio)
    label_op = torch.sigmoid(sdf_label / sigma)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(sdf_pred / sigma, label_op)
    loss = loss + cfg.weight_e * ((grad.norm(2, dim=-1) - 1.0) ** 2).mean()
    if color:
        loss = loss + cfg.weight_i * torch.abs(cp - color_label[valid_color_mask]).mean()
    return loss


def block(mapper, b, color):
    cfg = mapper.config
    S = sdf_losses(mapper, *b, eikonal=True, color=color, color_weighted=False)
    loss = S.bce + cfg.weight_e * S.eikonal
    return loss + cfg.weight_i * S.color if color else loss


def measure(fn, params, iters):
    def it():
        for p in params:
            p.grad = None
        fn().backward()
    for _ in range(3):
        it()
    torch.cuda.synchronize()
    walls = []
    for _ in range(iters):
        t0 = time.perf_counter()
        it()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    walls.sort()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            it()
        finally:
            torch.cuda.set_sync_debug_mode(0)
    waits = sum("synchroniz" in str(x.message).lower() for x in w)
    kern = launches = None
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            it()
            torch.cuda.synchronize()
        evs = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        kern = round(sum(e.device_time for e in evs) / 1e3, 4)
        launches = len(evs)
    except Exception as e:                      # profiler unavailable: report the rest
        kern = f"unavailable: {type(e).__name__}"
    return {"wall_ms_median": round(walls[len(walls) // 2], 4), "wall_ms_min": round(walls[0], 4),
            "kernel_ms_sum": kern, "device_ops": launches, "host_waits": waits}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda"
    mapper, params = setup(dev)
    res = {"neural_points": int(mapper.neural_points.neural_points.shape[0]), "gradient_decimation": 10,
           "device": torch.cuda.get_device_name(0)}
    for B in (8192, 16384):
        b = batch(mapper, B, dev)
        for color in (False, True):
            key = f"B{B}" + ("_colour" if color else "")
            runs = {"inline": [], "block": []}
            for _ in range(a.rounds):               # alternate: inline, block, inline, block, ...
                runs["inline"].append(measure(lambda: inline(mapper, b, color), params, a.iters))
                runs["block"].append(measure(lambda: block(mapper, b, color), params, a.iters))
            res[key] = {k: {"wall_ms_median_of_rounds": round(statistics.median(r["wall_ms_median"] for r in v), 4),
                            "rounds": v} for k, v in runs.items()}
            print(key, {k: v["wall_ms_median_of_rounds"] for k, v in res[key].items()}, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
