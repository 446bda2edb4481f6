"""Time the mapper's Gaussian-space loss block (utils/mapper.py:1331-1483): the inline torch block as an unmodified
mapper runs it (with the library installed: `Mapper.sdf` is `pings_amd.mapper_ops.sdf`) against the fused block
(`pings_amd.gaussian_losses`), forward + backward.

Scene: the Gaussian count of bench.py's `render_step` leg (458,377 spawned Gaussians, 85 % visible), gaussian_bs =
16,384 (bs 8192 x gaussian_bs_ratio 2.0, config/run_kitti_gs.yaml), R in {0, 1}, on the 160k-point synthetic SDF map
(oracle/sdf_cpu.synthetic_map; the Gaussians lie within a voxel of its points).  Shipped lambdas: opacity, area, SDF
consistency and SDF-normal consistency on, isotropy and entropy off.  Reports per block: wall time per iteration
(median of synchronised iterations), kernel-time sum and launch count (torch.profiler), and host waits (torch's
sync-debug warnings).

    python tools/gauss_loss_time.py [--iters 20] [--out profiles/gaussloss/gauss_loss_time.json]
"""
import argparse
import json
import sys
import time
import warnings
from pathlib import Path
from types import SimpleNamespace as NS

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oracle import sdf_cpu  # noqa: E402
from pings_amd import mapper_ops  # noqa: E402
from pings_amd.gaussian_losses import gaussian_losses  # noqa: E402


def scene(dev, P=458_377, n_points=160_000, seed=0):
    st, dec_st = sdf_cpu.synthetic_map(n_points, seed=seed)
    npm = sdf_cpu.NeuralPointMap(st, device=dev)
    npm.config = NS(query_nn_k=npm.nn_k, weighted_first=False, layer_norm_on=False)
    npm.color_feature_dim = 0
    npm.local_geo_features.requires_grad_(True)
    t = lambda k: torch.nn.Parameter(torch.as_tensor(dec_st["dec." + k]).to(dev))
    dec = NS(layers=[NS(weight=t("layers.0.weight"), bias=t("layers.0.bias"))],
             lout=NS(weight=t("lout.weight"), bias=t("lout.bias")), sdf_scale=float(dec_st["sdf_scale"]),
             use_leaky_relu=False)
    g = torch.Generator(device=dev).manual_seed(seed + 1)
    pts = npm.neural_points
    base = pts[torch.randint(0, pts.shape[0], (P,), generator=g, device=dev)]
    pkg = {"gaussian_xyz": base + 0.1 * torch.randn(P, 3, generator=g, device=dev),
           "gaussian_rot": torch.randn(P, 4, generator=g, device=dev),
           "gaussian_scale": 0.02 + 0.1 * torch.rand(P, 3, generator=g, device=dev),
           "gaussian_alpha": torch.rand(P, 1, generator=g, device=dev) * 1.2 - 0.1,
           "visibility_filter": torch.rand(P, generator=g, device=dev) < 0.85, "local_view_gaussian_count": P,
           "gaussian_free_mask": torch.zeros(P, dtype=torch.bool, device=dev),
           "contributions": torch.rand(P, generator=g, device=dev)}
    pkg["alpha_all"] = pkg["gaussian_alpha"].view(-1)
    for k in ("gaussian_xyz", "gaussian_rot", "gaussian_scale", "gaussian_alpha"):
        pkg[k].requires_grad_(True)
    return npm, dec, pkg


def torch_block(self, pkg):
    """utils/mapper.py:1331-1483 with the shipped lambdas (the caller weights; here all 1)."""
    c = self.config
    alpha_all, gaussian_alpha = pkg["alpha_all"], pkg["gaussian_alpha"]
    gaussian_xyz, gaussian_rot, gaussian_scale = pkg["gaussian_xyz"], pkg["gaussian_rot"], pkg["gaussian_scale"]
    opacity_loss = 0.0
    masked = alpha_all < c.min_alpha
    if torch.sum(masked) > 0:
        opacity_loss = 0.0 - alpha_all[masked].mean()
    mask = pkg["visibility_filter"][:pkg["local_view_gaussian_count"]] & (gaussian_alpha > c.min_alpha).squeeze(-1)
    mask = mask & (pkg["contributions"] > c.gs_contribution_threshold) & (~pkg["gaussian_free_mask"])
    count = torch.sum(mask).item()
    area_loss = sdf_cons = sdf_ncons = inv = 0.0
    if count > 10:
        true_idx = torch.where(mask)[0]
        bs = int(c.bs * c.gaussian_bs_ratio)
        idx = true_idx[torch.randperm(count)[:min(count, bs)]]
        scaling = gaussian_scale[idx]
        area_loss = (scaling[:, 0] * scaling[:, 1]).mean() / c.voxel_size_m ** 2
        alpha_s = gaussian_alpha[idx]
        xyz = gaussian_xyz[idx]
        q = gaussian_rot[idx]
        r, x, y, z = q.split(1, -1)
        n = torch.nn.functional.normalize(torch.cat([2 * (x * z + r * y), 2 * (y * z - r * x), 1 - 2 * (x * x + y * y)], -1))
        K, R = xyz.shape[0], c.gs_consist_shift_count
        shift = (torch.randn(K * R, device=xyz.device) - 0.5) * 2.0 * c.gs_consist_shift_range_m
        x_all = torch.cat((xyz, xyz.repeat(R, 1) + n.repeat(R, 1) * shift[:, None]), 0)
        n_all = torch.cat((n, n.repeat(R, 1)), 0)
        label = torch.cat((torch.zeros(K, device=xyz.device), shift), 0)
        x_all.requires_grad_(True)
        s, _, vnn = self.sdf(x_all, min_nn_count=3)
        gr = torch.autograd.grad(s, x_all, torch.ones_like(s), create_graph=True, retain_graph=True)[0]
        gn = gr.norm(dim=-1, keepdim=True).squeeze()
        valid = (gn < c.valid_grad_max_thre) & (gn > c.valid_grad_min_thre) & vnn
        inv = alpha_s[~valid[:K]].mean()
        torch.sum(valid).item()                                  # valid_grad_count (:1465)
        sdf_cons = torch.abs(s[valid] - label[valid]).mean()
        gh = gr / (gn.unsqueeze(-1) + 1e-7)
        sdf_ncons = (1.0 - (gh[valid] * n_all[valid]).sum(dim=1)).mean()
    return opacity_loss + area_loss + sdf_cons + sdf_ncons + inv


def fused_block(self, pkg, gen):
    G = gaussian_losses(self, pkg, gs_type="gaussian_surfel", opacity=True, area=True, sdf_consistency=True,
                        generator=gen)
    return G.opacity + G.area + G.sdf_cons + G.sdf_normal_cons + G.invalid_opacity


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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda"
    npm, dec, pkg = scene(dev)
    res = {"gaussians": pkg["gaussian_xyz"].shape[0], "neural_points": int(npm.neural_points.shape[0]),
           "gaussian_bs": 16384, "device": torch.cuda.get_device_name(0)}
    params = [pkg[k] for k in ("gaussian_xyz", "gaussian_rot", "gaussian_scale", "gaussian_alpha")] + \
             [npm.local_geo_features, dec.layers[0].weight, dec.layers[0].bias, dec.lout.weight, dec.lout.bias]
    for R in (0, 1):
        cfg = NS(bs=8192, gaussian_bs_ratio=2.0, min_alpha=0.05, gs_contribution_threshold=0.1,
                 gs_consist_shift_count=R, gs_consist_shift_range_m=0.1, valid_grad_min_thre=0.4,
                 valid_grad_max_thre=2.0, voxel_size_m=0.25, weighted_first=False)
        m = NS(config=cfg, neural_points=npm, sdf_mlp=dec, dtype=torch.float32, device=dev)
        m.sdf = lambda x, get_std=False, min_nn_count=1, _m=m: mapper_ops.sdf(_m, x, get_std, min_nn_count)
        gen = torch.Generator(device=dev).manual_seed(5)
        res[f"R{R}"] = {"torch_inline": measure(lambda: torch_block(m, pkg), params, a.iters),
                        "fused": measure(lambda: fused_block(m, pkg, gen), params, a.iters)}
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
