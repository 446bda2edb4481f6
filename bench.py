#!/usr/bin/env python3
"""bench.py — PINGS hot-path benchmark on MI355X (contract: see the build prompt / DESIGN.md §measurement).

Headline metric (BASELINE.json): raster fwd+bwd Mpix/s at 1M Gaussians, 1920x1080 (SURVEY.md §8d
Metric 1).  A plain run sets up, warms up, times the K steps and prints the headline line, nothing more; with --full
the same line also carries the per-kernel times, the roofline, the CPU-oracle baselines and parity, Metric 2 (SDF
Msamples/s) and the secondary legs (other workloads, tile-rectangle rules, training steps, decoders, SSIM, map).

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full [--no-sdf] [--no-cpu-baseline]]
  (--dump-outputs: the last timed step's outputs as DIR/<name>.npy, for comparing two builds output for output;
   N > 1: launched by torch.distributed.run, one rank per GPU; every rank renders its own camera
   view of the same Gaussian cloud and the parameter gradients are all-reduced over RCCL, as a
   multi-view training step would; weak scaling.)

One "step" = rasteriser forward + backward over one view through the public autograd API
(pings_amd.rasterizer.SurfelGaussianRasterizer -> libpings_hip.so), inputs resident in HBM.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import sys
import time
from pathlib import Path

# The ROCm runtime completes a blocked host wait (hipStreamSynchronize, torch's .item() / nonzero / synchronize) through
# an interrupt; with HSA_ENABLE_INTERRUPT=0 it polls the completion signal in user space instead.  On a healthy box the
# two measure the same (A/B in profiles/README.md, r03: every leg within noise); on one box of this pool blocked waits
# returned only with a 60 Hz tick (16 ms each: headline 11.7 instead of 1.15 ms/step).  The library's own read-backs
# poll pinned memory and do not depend on this; the variable covers torch's waits (the mapper's boolean-mask indexing
# in `sdf_step`, the synchronise that ends every timed region).  Set before the runtime initialises; an explicit
# setting in the environment wins.
os.environ.setdefault("HSA_ENABLE_INTERRUPT", "0")

import torch  # noqa: E402

ROOT = Path(__file__).resolve().parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md)


def synth_cloud(P, W, H, fx, fy, device, seed=42):
    """SURVEY.md §8d Metric 1 input: frustum-aligned box z in [1,60] m covering 1.3x the FoV,
    scales log-uniform [0.02,0.5] m (3rd = 1e-7), N(0,1) quaternions, opacity U(0.05,1), colour U(0,1)."""
    g = torch.Generator(device=device).manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, device=device)
    z = 1.0 + 59.0 * r(P)
    x = (2 * r(P) - 1) * 1.3 * (W / (2 * fx)) * z
    y = (2 * r(P) - 1) * 1.3 * (H / (2 * fy)) * z
    means = torch.stack([x, y, z], 1).contiguous()
    scales = torch.exp(math.log(0.02) + (math.log(0.5) - math.log(0.02)) * r(P, 3))
    scales[:, 2] = 1e-7
    rot = torch.nn.functional.normalize(torch.randn(P, 4, generator=g, device=device), dim=1)
    op = 0.05 + 0.95 * r(P, 1)
    col = r(P, 3)
    return means, col, op, scales.contiguous(), rot.contiguous()


def camera(W, H, fx, fy, cx, cy, znear, zfar, rank, device):
    """Settings record for `rank`'s view: rank 0 looks down +z from the origin, other ranks are
    perturbed by a few degrees / decimetres (different cameras of one rig)."""
    from oracle_free_camera import projection  # local helper below (no oracle import in the timed path)

    g = torch.Generator().manual_seed(1000 + rank)
    T = torch.eye(4, dtype=torch.float64)
    if rank > 0:
        w = (torch.rand(3, generator=g, dtype=torch.float64) - 0.5) * 0.12
        th = w.norm()
        K = torch.tensor([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=torch.float64)
        T[:3, :3] = torch.eye(3, dtype=torch.float64) + torch.sin(th) / th * K + (1 - torch.cos(th)) / th ** 2 * K @ K
        T[:3, 3] = (torch.rand(3, generator=g, dtype=torch.float64) - 0.5) * 0.6
    return projection(W, H, fx, fy, cx, cy, znear, zfar, T, device)


def pmc_traffic(stage, workload=None):
    """HBM bytes per launch of `stage`'s kernel from the newest committed rocprofv3 --pmc summary
    (profiles/rNN/*pmc_traffic.json: separate FETCH_SIZE / WRITE_SIZE passes of this very command, FETCH_SIZE
    doubled as MI355X_MICROARCH.md §HBM prescribes for gfx950).  PMC counters cannot be read from inside the
    timed process, so the figure is the one measured when the profile was taken; it is attached only when the
    summary records the SAME workload (gaussians / width / height / mode) as this run, otherwise None."""
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
    try:
        files = sorted(os.path.join(d, f) for d, _, fs in os.walk(root) for f in fs
                       if f.endswith("pmc_traffic.json") and not f.startswith(("sdf_", "ssim_")))
        if not files:
            return None, None, None
        data = json.load(open(files[-1]))
        meta = data.get("_workload")
        if workload is not None and meta is not None and any(meta.get(k) != v for k, v in workload.items()):
            return None, None, None
        if workload is not None and meta is None and (workload.get("gaussians"), workload.get("width"),
                                                      workload.get("height"), workload.get("mode")) != (1_000_000, 1920, 1080, "surfel"):
            return None, None, None   # round-1 summaries carry no workload record; they were taken on the default
        for name, v in data.items():
            if name.startswith(stage + "_"):
                # the calibrated figure where the summary has one (profiles/pmc_summary.py: this kernel's reads are
                # not wide streaming reads, so the blanket x2 of the guide over-corrects them; profiles/pmc_calib.hip)
                return (int(v.get("hbm_bytes_calibrated", v["hbm_bytes_corrected"])),
                        os.path.relpath(files[-1], os.path.dirname(root)), v.get("valu_insts"))
    except Exception:
        pass
    return None, None, None


def valu_calibration():
    """The newest committed vector-issue calibration (profiles/rNN/valu_calibration.json from profiles/valu_calib.hip), or None."""
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
    try:
        files = sorted(os.path.join(d, f) for d, _, fs in os.walk(root) for f in fs if f == "valu_calibration.json")
        if not files:
            return None
        cal = json.load(open(files[-1]))
        cal["_file"] = os.path.relpath(files[-1], os.path.dirname(root))
        return cal
    except Exception:
        return None


def parse_prof(txt):
    out = {}
    for line in txt.strip().splitlines():
        name, cnt, ms = line.split()
        out[name] = (int(cnt), float(ms))
    return out


def best_threads(fn, candidates=(8, 16, 32, 64, 128)):
    """Thread count (torch intra-op) at which `fn()` runs fastest on this host, probed once each."""
    best, best_t = None, float("inf")
    ncpu = os.cpu_count() or 8
    for n in candidates:
        if n > ncpu:
            break
        torch.set_num_threads(n)
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        if dt < best_t:
            best, best_t = n, dt
    torch.set_num_threads(best or min(8, ncpu))
    return torch.get_num_threads()


# fp32 operations per vector instruction in the record loop of blend_bwd_kernel<0,4> (tools/valu_mix.py on the gfx950 ISA)
BLEND_BWD_FLOPS_PER_VALU = 0.99

# largest fraction of (pixels, Gaussians) the parity gates may set aside as "undecidable in fp32" per test scene
# (measured in round 4: street 0.034 % / 21.6 %, room 0.036 % / 5.5 %, cloud 27.8 % / 21.0 % — the pixel
# ceilings are the verdict's, the Gaussian ceilings twice the measured values)
UNDECIDABLE_CEILING = {"street": (0.001, 0.45), "room": (0.001, 0.12), "cloud": (0.30, 0.45)}


def cpu_baseline_raster(dev, P_sample=16000, W=480, H=272):
    """The oracle (kind "port") timed on a bounded sample of the raster workload — the same cloud statistics,
    P_sample Gaussians, WxH pixels, fp32, fwd + autograd bwd, on the host cores — and, since the oracle's outputs
    are there anyway, used as the CHECKER of the HIP path on the very same inputs: `parity` holds the max relative
    error of every output and gradient (HIP fp32 vs oracle fp32; normalised by the reference's max-abs)."""
    from oracle import raster_cpu as R

    fx = fy = 1000.0 * W / 1920.0
    cx, cy = W / 2 - 0.5, H / 2 - 0.5
    means, col, op, scales, rot = synth_cloud(P_sample, W, H, fx, fy, "cpu", seed=42)
    cam = R.look_at_camera(W, H, fx, fy, cx, cy, 0.05, 110.0, dtype=torch.float32)
    s = R.Settings(H, W, cam["tanfovx"], cam["tanfovy"], torch.ones(3), 1.0, cam["viewmatrix"], cam["projmatrix"],
                   cam["projmatrix_raw"], cam["prcppoint"], front_only=True)
    g = torch.Generator().manual_seed(11)
    ups = [torch.randn(c, H, W, generator=g) for c in (3, 3, 1, 1)]
    keys = ("color", "normal", "depth", "alpha")

    def run():
        leaves = [t.clone().requires_grad_(True) for t in (means, col, op, scales, rot)]
        th, rh = torch.zeros(3, requires_grad=True), torch.zeros(3, requires_grad=True)
        out = R.rasterize(*leaves, s, th, rh)
        loss = sum((out[k] * u).sum() for k, u in zip(keys, ups))
        return out, torch.autograd.grad(loss, leaves + [th, rh])

    def undecidable():
        """Pixels / Gaussians fp32 cannot decide (oracle `margins=True`: within 3e-5 of a discrete blend decision, or a
        quadratic form whose fp32 rounding exceeds 2e-5 of a blended channel) - untimed second oracle forward."""
        with torch.no_grad():
            o = R.rasterize(means, col, op, scales, rot, s, margins=True)
        pix = (o["pixel_margin"] < 3e-5) | (o["pixel_cond"] > 2e-5)
        gs = (o["gaussian_margin"] < 3e-5) | (o["gaussian_cond"] > 2e-5)
        return pix, gs

    small = lambda: R.rasterize(means[:2000], col[:2000], op[:2000], scales[:2000], rot[:2000], s)
    threads = best_threads(small)
    t0 = time.time()
    out, grads = run()
    dt = time.time() - t0
    # the HIP path on the same inputs
    from pings_amd import rasterizer as hr
    dcam = camera(W, H, fx, fy, cx, cy, 0.05, 110.0, 0, dev)
    rs = hr.SurfelRasterizationSettings(
        image_height=H, image_width=W, tanfovx=dcam["tanfovx"], tanfovy=dcam["tanfovy"], bg=torch.ones(3, device=dev),
        scale_modifier=1.0, viewmatrix=dcam["viewmatrix"], projmatrix=dcam["projmatrix"],
        projmatrix_raw=dcam["projmatrix_raw"], patch_bbox=torch.tensor([0, 0, H - 1, W - 1], dtype=torch.float32, device=dev),
        prcppoint=dcam["prcppoint"], sh_degree=0, campos=dcam["campos"], prefiltered=False, debug=False,
        config=torch.tensor([1, 1, 1, 1, 1], dtype=torch.float32, device=dev))
    rast = hr.SurfelGaussianRasterizer(rs)
    hl = [t.to(dev).requires_grad_(True) for t in (means, col, op, scales, rot)]
    th, rh = torch.zeros(3, device=dev, requires_grad=True), torch.zeros(3, device=dev, requires_grad=True)
    img, nrm, dep, alp, radii, contrib = rast(means3D=hl[0], means2D=torch.zeros_like(hl[0]), colors_precomp=hl[1],
                                              opacities=hl[2], scales=hl[3], rotations=hl[4], theta=th, rho=rh)
    torch.autograd.backward([img, nrm, dep, alp], [u.to(dev) for u in ups])

    def rel(a, b):
        """[max-abs error / max|ref|, relative L2 error, entries off by more than 1e-4 max|ref|]"""
        a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
        scale = max(b.abs().max().item(), 1e-30)
        d = (a - b).abs()
        return [float(f"{d.max().item() / scale:.3e}"), float(f"{(d.norm() / max(b.norm().item(), 1e-30)).item():.3e}"),
                int((d > 1e-4 * scale).sum())]

    pix_flag, g_flag = undecidable()

    def rel_outside(a, b, flag, per_pixel):
        """max-abs error / max|ref| over the entries fp32 CAN decide (pixels / Gaussian rows outside the flagged set)"""
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        scale = max(b.abs().max().item(), 1e-30)
        d = (a - b).abs()
        d = d.amax(0) if per_pixel else d.reshape(d.shape[0], -1).amax(1)
        return float(f"{d[~flag].max().item() / scale:.3e}")

    def rel_l2_flagged(a, b, flag):
        """[relative L2 error over the FLAGGED pixels alone, how many of them are off by more than 1e-4 max|ref|]: the
        flagged set is not exempt — tests/test_raster.py lets 1 % of it (at least 4 pixels) exceed 1e-4, each by at most
        one alpha = 1/255 contribution"""
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        if not bool(flag.any()):
            return [0.0, 0]
        d = (a - b)[:, flag]
        scale = max(b.abs().max().item(), 1e-30)
        return [float(f"{(d.norm() / max(b[:, flag].norm().item(), 1e-30)).item():.3e}"),
                int((d.abs().amax(0) > 1e-4 * scale).sum())]

    # the undecidable set must not grow silently.  Ceilings for THIS scene (the cloud's thin footprints
    # put a rounding bound above 2e-5 on ~28 % of the pixels; tests/test_raster.py holds the street / room ceilings)
    pix_frac, g_frac = float(pix_flag.float().mean()), float(g_flag.float().mean())
    parity = {"format": "[max_rel_err, rel_l2_err, entries > 1e-4, max_rel_err over the DECIDABLE pixels / Gaussians]",
              "undecidable_pixels": int(pix_flag.sum()), "undecidable_gaussians": int(g_flag.sum()),
              "undecidable_pixel_frac": round(pix_frac, 5), "undecidable_gaussian_frac": round(g_frac, 5),
              "undecidable_frac_ceiling": {"pixels": UNDECIDABLE_CEILING["cloud"][0], "gaussians": UNDECIDABLE_CEILING["cloud"][1]},
              "undecidable_within_ceiling": bool(pix_frac <= UNDECIDABLE_CEILING["cloud"][0]
                                                 and g_frac <= UNDECIDABLE_CEILING["cloud"][1]),
              "flagged_pixels_rel_l2": {k: rel_l2_flagged(t, out[k], pix_flag) for k, t in zip(keys, (img, nrm, dep, alp))},
              "radii_equal": bool((radii.cpu() == out["radii"]).all())}
    for k, t in zip(keys, (img, nrm, dep, alp)):
        parity[k] = rel(t, out[k]) + [rel_outside(t, out[k], pix_flag, True)]
    parity["contributions"] = rel(contrib, out["contributions"]) + [rel_outside(contrib, out["contributions"], g_flag, False)]
    for name, a, b in zip(("d_means3D", "d_colors", "d_opacities", "d_scales", "d_rotations", "d_theta", "d_rho"),
                          [t.grad for t in hl] + [th.grad, rh.grad], grads):
        parity[name] = rel(a.reshape(b.shape), b)
        if b.numel() > 8:
            parity[name].append(rel_outside(a.reshape(b.shape), b, g_flag, False))
    parity["note"] = ("HIP fp32 vs oracle fp32 on identical inputs.  The fourth figure is the max error over the pixels / "
                      "Gaussians that fp32 can decide: the oracle reports, per pixel, the relative distance to the nearest "
                      "discrete decision of the blend (alpha < 1/255 skip, power > 0 skip, T < 1e-4 stop, 0.99 clamp, "
                      "surfel-depth clamp / den test) and the fp32 rounding of the footprint's quadratic form; pixels "
                      "within 3e-5 / above 2e-5 and the Gaussians evaluated in them are IDENTIFIED and counted, not "
                      "dropped by rank (tests/test_raster.py::test_mid_size_scene_* gates the same way)")
    return {"value": round(W * H / dt / 1e6, 6), "unit": "Mpix/s", "cores": threads,
            "kind": "port",
            "sample": f"oracle/raster_cpu.py fp32 fwd+bwd, {P_sample} Gaussians of the same distribution at "
                      f"{W}x{H} ({dt:.1f} s of CPU work, {threads} torch threads = the fastest of 8..128 on this host; "
                      f"host has {os.cpu_count()} logical cores)",
            "parity": parity}


# --------------------------------------------------------------------------- SDF (Metric 2)
SDF_PRIMES = (73856093, 19349669, 83492791)


def sdf_synth_map(n_points, device, voxel=0.25, search_alpha=0.8, nn_k=6, feat_dim=32, hidden=64,
                  buffer_size=int(1e8), seed=42, weighted_first=False):
    """SURVEY.md §8d Metric 2 map, built on the device: neural points on the wavy sheet
    z = 2 sin(0.3x) + cos(0.2y), one per 0.25 m voxel, inserted into the 1e8-slot int64 hash table
    with the reference's rule (later insert wins, model/neural_gaussians.py:243-247,299-308)."""
    g = torch.Generator(device=device).manual_seed(seed)
    side = (n_points * 1.15) ** 0.5 * voxel
    xy = (torch.rand(int(n_points * 4), 2, generator=g, device=device) - 0.5) * side
    z = 2.0 * torch.sin(0.3 * xy[:, 0]) + torch.cos(0.2 * xy[:, 1])
    pts = torch.cat([xy, z[:, None]], 1)
    cells = torch.floor(pts / voxel).to(torch.int64)
    key = (cells[:, 0] + 2 ** 20) * 2 ** 42 + (cells[:, 1] + 2 ** 20) * 2 ** 21 + (cells[:, 2] + 2 ** 20)
    uniq, inv = torch.unique(key, return_inverse=True)
    first = torch.full((uniq.shape[0],), key.shape[0], dtype=torch.int64, device=device)
    first.scatter_reduce_(0, inv, torch.arange(key.shape[0], device=device), reduce="amin")
    first = torch.sort(first).values[:n_points]
    pts, cells = pts[first].contiguous(), cells[first]
    n = pts.shape[0]
    primes = torch.tensor(SDF_PRIMES, dtype=torch.int64, device=device)
    h = torch.fmod((cells * primes).sum(-1), buffer_size)
    slots = torch.where(h < 0, h + buffer_size, h)
    table = torch.full((buffer_size,), -1, dtype=torch.int64, device=device)
    table.scatter_reduce_(0, slots, torch.arange(n, device=device), reduce="amax")
    dx = torch.arange(-2, 3, dtype=torch.int64, device=device)
    dxyz = torch.stack(torch.meshgrid(dx, dx, dx, indexing="ij"), -1).reshape(-1, 3)
    dxyz = dxyz[(dxyz ** 2).sum(-1) < (2 + search_alpha) ** 2]
    feats = torch.cat([0.05 * torch.randn(n, feat_dim, generator=g, device=device),
                       torch.zeros(1, feat_dim, device=device)])
    in_dim = feat_dim + 3
    dec = {"layers.0.weight": torch.randn(hidden, in_dim, generator=g, device=device) / in_dim ** 0.5,
           "layers.0.bias": 0.1 * torch.randn(hidden, generator=g, device=device),
           "lout.weight": torch.randn(1, hidden, generator=g, device=device) / hidden ** 0.5,
           "lout.bias": 0.1 * torch.randn(1, generator=g, device=device)}
    from types import SimpleNamespace as NS

    npm = NS(buffer_pt_index=table, neural_points=pts, point_orientations=None, geo_features=feats,
             color_features=None, point_ts_create=torch.zeros(n, dtype=torch.int32, device=device),
             point_certainties=torch.zeros(n, device=device),
             free_gs_mask=torch.zeros(n, dtype=torch.bool, device=device),
             valid_gs_mask=torch.ones(n, dtype=torch.bool, device=device),
             travel_dist=torch.zeros(1, device=device), cur_ts=0, diff_travel_dist_local=1e9,
             local_neural_points=pts, local_geo_features=feats, local_color_features=None,
             local_point_certainties=torch.zeros(n, device=device),
             local_point_ts_update=torch.zeros(n, dtype=torch.int32, device=device),
             local_point_orientations=torch.tensor([1.0, 0, 0, 0], device=device).repeat(n, 1),
             global2local=torch.cat([torch.arange(n, device=device), torch.tensor([-1], device=device)]),
             neighbor_dx=dxyz, max_valid_dist2=3 * ((2 + 1) * voxel) ** 2, resolution=voxel, after_pgo=False,
             temporal_local_map_on=False, nn_k=nn_k, weighted_first=weighted_first, geo_feature_dim=feat_dim,
             color_feature_dim=0, dtype=torch.float32,
             config=NS(query_nn_k=nn_k, weighted_first=weighted_first, layer_norm_on=False))
    npm.point_orientations = npm.local_point_orientations
    decoder = NS(layers=[NS(weight=dec["layers.0.weight"], bias=dec["layers.0.bias"])],
                 lout=NS(weight=dec["lout.weight"], bias=dec["lout.bias"]), sdf_scale=0.55 * 0.05,
                 use_leaky_relu=False)
    return npm, decoder


def sdf_queries(npm, B, device, seed=7):
    g = torch.Generator(device=device).manual_seed(seed)
    sel = torch.randint(0, npm.neural_points.shape[0], (B,), generator=g, device=device)
    return (npm.neural_points[sel] + torch.randn(B, 3, generator=g, device=device) * (0.5 * npm.resolution)).contiguous()


def bench_sdf(dev, steps, warmup, n_points=1_000_000):
    """The 1M-point Metric-2 map: tracker registration step here, query / training rates in `bench_sdf_sweep`."""
    from pings_amd import neural_points as hnp

    npm, dec = sdf_synth_map(n_points, dev)
    out = {"voxel_m": 0.25, "K": int(npm.neighbor_dx.shape[0]), "nn_k": 6, "feature_dim": 32, "hidden": 64,
           "buffer_size": int(1e8), "algorithmic_bytes_per_sample_fwd": 2428}
    # one tracker registration iteration = query_source_points (sdf, d sdf/dx, std, mask, certainty:
    # one fused kernel per batch) + implicit_reg (6x6 normal equations kernel + fp64 solve), 131072 source points
    from types import SimpleNamespace as NS_
    from pings_amd import tracker_ops as TO
    B = 131072
    x = sdf_queries(npm, B, dev)
    fake = NS_(neural_points=npm, sdf_mlp=dec, config=NS_(weighted_first=False, color_channel=3))

    def reg_step():
        sdf, grad, _, _, _, mask, cert, std = TO.query_source_points(fake, x, B, True, True, False, False,
                                                                    query_locally=True, mask_min_nn_count=4)
        w = torch.ones(B, 1, device=dev) * mask[:, None]
        return TO.implicit_reg(x, grad, sdf, w, lm_lambda=1e-4)

    for _ in range(warmup):
        reg_step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        reg_step()
    torch.cuda.synchronize()
    t_r = (time.perf_counter() - t0) / steps
    out["tracker_step"] = {"source_points": B, "ms_per_iteration": round(t_r * 1e3, 4),
                           "Mpoints_s": round(B / t_r / 1e6, 2)}
    return out, npm, dec


def bench_decoder(dev, steps, warmup, n_points=125_000):
    """The five spawn decoders (pings.py:156-160; hidden 128, 8 Gaussians per neural point) forward + backward on
    n_points visible neural points through the MFMA kernel: TFLOP/s against the fp32 matrix peak (157.3 TFLOP/s)."""
    from pings_amd import _lib

    g = torch.Generator(device=dev).manual_seed(3)
    shapes = [("xyz", 32, 24), ("rot", 32, 32), ("scale", 32, 24), ("alpha", 32, 8), ("color", 19, 24)]
    nets = []
    for name, fin, fout in shapes:
        mk = lambda *s: torch.randn(*s, generator=g, device=dev).requires_grad_(True)
        nets.append((mk(n_points, fin), mk(128, fin), mk(128), mk(fout, 128), mk(fout), torch.randn(n_points, fout, generator=g, device=dev)))

    from pings_amd.mlp import fused_mlp_group

    leaves = [t for n_ in nets for t in n_[:5]]

    def step():   # the five decoders in one launch each way, as `spawn_gaussians` issues them
        ys = fused_mlp_group([n_[0] for n_ in nets], [n_[1:5] for n_ in nets])
        torch.autograd.grad(ys, leaves, [n_[5] for n_ in nets])

    L = _lib.lib()
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    L.pings_prof_enable(1)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    L.pings_prof_enable(0)
    buf = C.create_string_buffer(4096)
    L.pings_prof_report(buf, len(buf))
    prof = parse_prof(buf.value.decode())
    flop_f = sum(2 * n_points * (fin * 128 + 128 * fout) for _, fin, fout in shapes)
    t_f, t_b = prof["mlp_fwd"][1] / steps * 1e-3, prof["mlp_bwd"][1] / steps * 1e-3
    return {"neural_points": n_points, "launches": "grouped: 1 forward, 1 backward + 1 reduce for the five decoders",
            "fwd_ms": round(t_f * 1e3, 4), "bwd_ms": round(t_b * 1e3, 4),
            "bwd_frac_of_fp32_mfma_peak": round(2 * flop_f / t_b / 157.3e12, 3),
            "fwd_TFLOPs": round(flop_f / t_f / 1e12, 1), "bwd_TFLOPs": round(2 * flop_f / t_b / 1e12, 1),
            "mfma_peak_TFLOPs": 157.3, "fwd_frac_of_fp32_mfma_peak": round(flop_f / t_f / 157.3e12, 3),
            "wall_ms_fwd_bwd_autograd": round(dt * 1e3, 4)}


def bench_image_losses(dev, steps, warmup, W=1920, H=1080, with_cpu=True):
    """the photometric loss block of the mapper (mapper.py:1197-1295) at 1080p, fused forward and
    backward kernels against HBM: 61 B/pixel read forward, 61 B read + 44 B written backward."""
    from pings_amd.image_losses import image_losses
    from pings_amd import _lib

    g = torch.Generator(device=dev).manual_seed(4)
    r = lambda c: torch.rand(c, H, W, generator=g, device=dev)
    rgb, gt, depth, alpha = r(3).requires_grad_(True), r(3), (1 + 9 * r(1)).requires_grad_(True), r(1).requires_grad_(True)
    gt_depth = depth.detach() + 0.3 * (r(1) - 0.5)
    n = torch.nn.functional.normalize(r(3) - 0.5, dim=0).requires_grad_(True)
    m = torch.nn.functional.normalize(n.detach() + 0.3 * (r(3) - 0.5), dim=0).requires_grad_(True)
    sky = r(1) < 0.2
    opts = dict(depth_min=0.3, depth_max=20.0, depth_min_accu_alpha=0.4)

    def step(fn, leaves, *a):
        o = fn(*a, **opts)
        o = o if isinstance(o, dict) else o._asdict()
        tot = o["rgb_l1"] + 0.5 * o["depth_l1"] + 0.1 * o["normal_depth_consist"] + 0.1 * o["sky"]
        return torch.autograd.grad(tot, leaves)

    L = _lib.lib()
    args = (rgb, gt, depth, gt_depth, alpha, n, m, sky)
    leaves = [rgb, depth, alpha, n, m]
    for _ in range(warmup):
        step(image_losses, leaves, *args)
    torch.cuda.synchronize()
    L.pings_prof_enable(1)
    t0 = time.perf_counter()
    for _ in range(steps):
        step(image_losses, leaves, *args)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    L.pings_prof_enable(0)
    buf = C.create_string_buffer(4096)
    L.pings_prof_report(buf, len(buf))
    prof = parse_prof(buf.value.decode())
    t_f, t_b = prof["image_losses_fwd"][1] / steps * 1e-3, prof["image_losses_bwd"][1] / steps * 1e-3
    px = W * H
    out = {"width": W, "height": H, "fwd_ms": round(t_f * 1e3, 4), "bwd_ms": round(t_b * 1e3, 4),
           "fwd_GBs": round(61 * px / t_f / 1e9, 1), "bwd_GBs": round(105 * px / t_b / 1e9, 1), "hbm_peak_GBs": HBM_PEAK_GBS,
           "frac_of_hbm_peak_fwd_bwd": [round(61 * px / t_f / 1e9 / HBM_PEAK_GBS, 3), round(105 * px / t_b / 1e9 / HBM_PEAK_GBS, 3)],
           "wall_ms_fwd_bwd_autograd": round(dt * 1e3, 4)}
    if with_cpu:
        from oracle.imgloss_cpu import image_losses as ref  # checker / CPU baseline leg only
        cl = [t.detach().cpu().requires_grad_(True) for t in leaves]
        ca = (cl[0], gt.cpu(), cl[1], gt_depth.cpu(), cl[2], cl[3], cl[4], sky.cpu())
        step(ref, cl, *ca)
        t0 = time.perf_counter()
        k = 10
        for _ in range(k):
            step(ref, cl, *ca)
        tc = (time.perf_counter() - t0) / k
        out["cpu_baseline"] = {"value": round(px / tc / 1e6, 2), "unit": "Mpix/s", "cores": torch.get_num_threads(), "kind": "port",
                               "sample": f"oracle/imgloss_cpu.py (reference torch op sequence), {k} fwd+bwd passes at {W}x{H}"}
        out["Mpix_s_fwd_bwd_kernels"] = round(px / (t_f + t_b) / 1e6, 1)
    return out


def bench_map(dev, frames=6, n_scan=1_000_000, voxel=0.1, with_cpu=True):
    """per-frame map maintenance — voxel down-sampling + `update` (hash insert, appends) +
    `reset_local_map` + `assign_local_to_global` on a growing map (1M-point scans of a wavy street-sized sheet,
    0.1 m voxels, 1e8-slot table), HIP path vs the CPU oracle (the reference's torch op sequence) on the same scans."""
    from pings_amd import neural_map as NM
    from oracle import map_cpu as MC

    kw = dict(temporal_local_map_on=True, use_mid_ts=False, range_filter_2d=True, local_map_radius=60.0,
              sorrounding_map_radius=84.0, diff_travel_dist_local=300.0)
    g = torch.Generator().manual_seed(5)
    scans = []
    for ts in range(frames):
        xy = (torch.rand(n_scan, 2, generator=g) - 0.5) * 160.0 + torch.tensor([8.0 * ts, 0.0])
        z = 2.0 * torch.sin(0.3 * xy[:, 0]) + torch.cos(0.2 * xy[:, 1]) + 0.02 * torch.randn(n_scan, generator=g)
        scans.append((torch.cat([xy, z[:, None]], 1), torch.rand(n_scan, 3, generator=g),
                      torch.tensor([8.0 * ts, 0.0, 1.5])))
    td = torch.arange(frames + 1, dtype=torch.float32) * 8.0

    def run(mod, m, device):
        ts_ms = []
        for ts, (pts, cols, sensor) in enumerate(scans):
            pts, cols, sensor = pts.to(device), cols.to(device), sensor.to(device)
            if device != "cpu":
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            if mod is NM:
                NM.update(m, pts, cols, None, sensor, None, cur_ts=ts)
                NM.assign_local_to_global(m)
            else:
                MC.update(m, pts, cols, ts)
                MC.reset_local_map(m, sensor, ts)
                MC.assign_local_to_global(m)
            if device != "cpu":
                torch.cuda.synchronize()
            ts_ms.append((time.perf_counter() - t0) * 1e3)
        return ts_ms

    mh = NM.new_map(100_000_000, 32, 16, voxel, device=str(dev), **kw)
    mh.travel_dist = td.to(dev)
    t_hip = run(NM, mh, str(dev))
    out = {"scan_points": n_scan, "voxel_m": voxel, "frames": frames, "map_points_final": int(mh.neural_points.shape[0]),
           "local_points_final": int(mh.local_neural_points.shape[0]), "buffer_size": 100_000_000,
           "ms_per_frame": [round(t, 3) for t in t_hip],
           "Mpoints_s": round(n_scan * (frames - 1) / (sum(t_hip[1:]) * 1e-3) / 1e6, 2)}
    del mh
    torch.cuda.empty_cache()
    if with_cpu:
        mc = MC.new_map(100_000_000, 32, 16, voxel, **kw)
        mc.travel_dist = td
        n_cpu = 3
        scans_cpu = scans[:n_cpu]
        scans_full, scans[:] = list(scans), scans_cpu
        t_cpu = run(MC, mc, "cpu")
        scans[:] = scans_full
        out["cpu_baseline"] = {"value": round(n_scan * (n_cpu - 1) / (sum(t_cpu[1:]) * 1e-3) / 1e6, 3), "unit": "Mpoints/s",
                               "cores": torch.get_num_threads(), "kind": "port",
                               "sample": f"oracle/map_cpu.py (reference torch op sequence), first {n_cpu} of the same scans "
                                         f"({sum(t_cpu) / 1e3:.1f} s of CPU work; host has {os.cpu_count()} logical cores)"}
    return out


def _timeit(fn, steps, warmup, repeats=3):
    """Seconds per call: best of `repeats` timed runs of `steps` calls each (secondary legs only — the headline's timed
    region is one run of exactly K steps, as the contract asks).  The small-batch legs are host-bound and a GPU box's
    host jitters (thread wake-ups, frequency ramps: the same binary measured 0.16 and 0.31 ms per fused SDF step within
    one process), so a single run says little; every leg is measured the same way."""
    for _ in range(warmup):
        fn()
    best = float("inf")
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) / steps)
    return best


def _prof_run(L, fn, steps):
    """Per-stage HIP-event times (ms per step) of `steps` calls of fn with every library stage recorded."""
    L.pings_prof_only(None)
    L.pings_prof_enable(1)
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    L.pings_prof_enable(0)
    buf = C.create_string_buffer(16384)
    L.pings_prof_report(buf, len(buf))
    return {k: v[1] / steps for k, v in parse_prof(buf.value.decode()).items()}


DUMP_BUDGET_BYTES = 60_000_000   # --dump-outputs: all arrays together stay under 64 MB
DUMP_SEED = 0


def dump_outputs(out_dir, arrays):
    """--dump-outputs: write every tensor of `arrays` ({name: tensor}) as out_dir/<name>.npy, float64 if the tensor is
    float64 or an integer type (exact), float32 otherwise.  The budget is split evenly between the arrays; an array over
    its share keeps a fixed sample of its items, as [k, values per item].  Items are the rows of a [P, ...] array and
    the pixels of a [C, H, W] image.  The sample is the first k of a permutation seeded with DUMP_SEED, in ascending
    order: two runs (or two builds) with the same arguments write the same items, and arrays with the same item count
    share the items the smaller sample keeps.  Returns {name: {"shape": full shape, "items_kept": k or None when whole}}."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    share = DUMP_BUDGET_BYTES // len(arrays)
    perms = {}
    written = {}
    for name, t in arrays.items():
        t = t.detach()
        exact64 = t.dtype == torch.float64 or not t.is_floating_point()
        a = t.to(torch.float64 if exact64 else torch.float32).cpu().numpy()
        kept = None
        if a.nbytes > share:
            rows = a.reshape(a.shape[0], -1).T if a.ndim == 3 else a.reshape(a.shape[0], -1)
            kept = max(1, share // rows[0].nbytes)
            if rows.shape[0] not in perms:
                perms[rows.shape[0]] = np.random.default_rng(DUMP_SEED).permutation(rows.shape[0])
            a = np.ascontiguousarray(rows[np.sort(perms[rows.shape[0]][:kept])])
        np.save(os.path.join(out_dir, f"{name}.npy"), a)
        written[name] = {"shape": list(t.shape), "items_kept": kept}
    return written


def bench_sdf_sweep(dev, steps, warmup, sizes=(200_000, 1_000_000, 5_000_000), with_cpu=True):
    """Metric 2 at the three map sizes BASELINE.md §3 names (N_np = 2e5 / 1e6 / 5e6, 1e8-slot table, K = 81, k = 6,
    F = 32, hidden 64) plus the C1 (PIN-SLAM, config/run_pin_slam.yaml) variant: forward and training-step rates at
    B = 16,384 and 131,072, each forward with an explicit roofline object (algorithmic 2,428 B/sample, SURVEY §8d,
    against the HBM peak; `traffic` = PMC bytes per launch when a matching profile is committed)."""
    from pings_amd import neural_points as hnp

    L = _lib_handle()
    out = {}
    for n_points in sizes:
        npm, dec = sdf_synth_map(n_points, dev)
        leg = {"neural_points": int(npm.neural_points.shape[0])}
        for B in (16384, 131072):
            x = sdf_queries(npm, B, dev)
            fwd = lambda: hnp.sdf_fused(npm, dec, x, use_only_measured_points=False)
            t_wall = _timeit(fwd, steps, warmup)
            t_k = _prof_run(L, fwd, steps)["sdf_forward"] * 1e-3
            alg = 2428 * B
            leg[f"B{B}"] = {"fwd_Msamples_s": round(B / t_wall / 1e6, 2), "fwd_kernel_ms": round(t_k * 1e3, 4),
                            "roofline": {"kernel": "sdf_forward_kernel", "bound": "hbm",
                                         "achieved": round(alg / t_k / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                         "frac": round(alg / t_k / 1e9 / HBM_PEAK_GBS, 4), "algorithmic_bytes": alg,
                                         "traffic": sdf_pmc_traffic(n_points, B)}}
            tr = leg[f"B{B}"]["roofline"]["traffic"]
            if tr:
                # the kernel's reads are one 64-B half-line request per probe / row (profiles/pmc_calib.hip: FETCH_SIZE
                # is exact for them), and the chip serves 54.5 G such random requests per second when a kernel does
                # nothing else (read_gather8 over a 1 GiB table, profiles/r02/pmc_calibration_kernel_stats.csv): THAT
                # is the ceiling of this kernel, not the 8 TB/s of streamed bytes
                leg[f"B{B}"]["roofline"]["sector_requests"] = {
                    "per_launch": int(tr / 64), "achieved_G_s": round(tr / 64 / t_k / 1e9, 1), "peak_G_s": 54.5,
                    "frac": round(tr / 64 / t_k / 54.5e9, 3)}
            leg[f"B{B}"].update(sdf_train_rates(npm, dec, x, steps, warmup))
        leg["index_rebuild_ms"] = index_rebuild_ms(npm)
        if n_points == 1_000_000:
            leg["sdf_step"] = {f"B{b}": bench_sdf_step(npm, dec, dev, steps, warmup, b) for b in (8192, 16384)}
        out[f"N{n_points}"] = leg
        del npm, dec
        torch.cuda.empty_cache()
    # C1: voxel 0.4, search_alpha 0.5, F = 8, weighted_first, B = 10,000 (config/run_pin_slam.yaml)
    npm, dec = sdf_synth_map(200_000, dev, voxel=0.4, search_alpha=0.5, feat_dim=8, weighted_first=True)
    x = sdf_queries(npm, 10000, dev)
    fwd = lambda: hnp.sdf_fused(npm, dec, x, use_only_measured_points=False)
    t_wall = _timeit(fwd, steps, warmup)
    c1 = {"neural_points": int(npm.neural_points.shape[0]), "voxel_m": 0.4, "K": int(npm.neighbor_dx.shape[0]),
          "feature_dim": 8, "weighted_first": True, "B": 10000, "fwd_Msamples_s": round(10000 / t_wall / 1e6, 2)}
    c1.update(sdf_train_rates(npm, dec, x, steps, warmup))
    if with_cpu:
        c1["cpu_baseline"], _ = cpu_baseline_sdf(npm, dec, B=10000, reps=20, weighted_first=True, label="C1 map")
    out["C1_pin_slam"] = c1
    del npm, dec
    torch.cuda.empty_cache()
    return out


def index_rebuild_ms(npm, reps=5):
    """The cell-block index of the search (csrc/knn_blocks.hip) is rebuilt whenever a tensor it was built from changes,
    i.e. after every `update` / `reset_local_map` of a mapped frame: its cost belongs to the frame, not to any query
    ('in no bench figure').  Forced here by dropping the cached index; best of `reps`."""
    from pings_amd import neural_points as hnp

    best = float("inf")
    for _ in range(reps):
        npm.__dict__.pop("_pings_blocks", None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hnp._block_index(npm)
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return round(best * 1e3, 4)


def sdf_pmc_traffic(n_points, B):
    """HBM bytes per launch of sdf_forward_kernel from the committed PMC summary of this configuration, or None."""
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
    try:
        files = sorted(os.path.join(d, f) for d, _, fs in os.walk(root) for f in fs if f.endswith("sdf_pmc_traffic.json"))
        if files:
            rec = json.load(open(files[-1])).get(f"N{n_points}_B{B}", {})
            return rec.get("hbm_bytes_calibrated", rec.get("hbm_bytes_corrected"))
    except Exception:
        pass
    return None


def sdf_train_rates(npm, dec, x, steps, warmup):
    """Training-step rates on one map / batch: (a) the fused S(x) with its fused first-order backward, (b) the path an
    unmodified mapper reaches — `query_feature` + the decoder in torch autograd (mapper.py:848-866), first order —
    (c) the same with the Eikonal term through get_gradient(create_graph=True) (mapper.py:874-875, :1448), and
    (d) as (b) with `Decoder.sdf` bound to the fused MFMA decoder (`pings_amd.decoder.install`)."""
    from types import SimpleNamespace as NS_

    from pings_amd import neural_points as hnp

    B = x.shape[0]
    keep = npm.local_geo_features
    P_ = [torch.nn.Parameter(t.detach().clone()) for t in (dec.layers[0].weight, dec.layers[0].bias, dec.lout.weight, dec.lout.bias)]
    dec_t = NS_(layers=[NS_(weight=P_[0], bias=P_[1])], lout=NS_(weight=P_[2], bias=P_[3]), sdf_scale=dec.sdf_scale,
                use_leaky_relu=False)
    feats = keep.detach().clone().requires_grad_(True)
    npm.local_geo_features = feats
    wf = bool(npm.config.weighted_first)

    def fused():
        s_, _ = hnp.sdf_train(npm, dec_t, x, use_only_measured_points=False)
        return torch.autograd.grad(s_.abs().mean(), [feats] + P_)

    def sdf_of(xq):
        geo, _, w, c, _ = hnp.query_feature(npm, xq, accumulate_stability=False, use_only_measured_points=False)
        h = torch.relu(torch.nn.functional.linear(geo, P_[0], P_[1]))
        s_ = torch.nn.functional.linear(h, P_[2], P_[3]).squeeze(-1) * dec.sdf_scale
        return s_ if wf else (s_ * w.squeeze(-1)).sum(1)

    def dropin():
        return torch.autograd.grad(sdf_of(x).abs().mean(), [feats] + P_)

    def dropin_fused_decoder():
        from pings_amd import decoder as hdec

        geo, _, w, c, _ = hnp.query_feature(npm, x, accumulate_stability=False, use_only_measured_points=False)
        s_ = hdec.sdf(dec_t, geo).squeeze(-1)
        s_ = s_ if wf else (s_ * w.squeeze(-1)).sum(1)
        return torch.autograd.grad(s_.abs().mean(), [feats] + P_)

    def dropin_eikonal():
        xq = x.detach().clone().requires_grad_(True)
        s_ = sdf_of(xq)
        g = torch.autograd.grad(s_, xq, torch.ones_like(s_), create_graph=True)[0]
        loss = s_.abs().mean() + 0.5 * ((g.norm(2, dim=-1) - 1.0) ** 2).mean()
        return torch.autograd.grad(loss, [feats] + P_)

    r = {}
    try:
        for name, fn in (("fwd_bwd_fused_Msamples_s", fused), ("fwd_bwd_query_feature_Msamples_s", dropin),
                         ("fwd_bwd_eikonal_query_feature_Msamples_s", dropin_eikonal),
                         ("fwd_bwd_query_feature_fused_decoder_Msamples_s", dropin_fused_decoder)):
            r[name] = round(B / _timeit(fn, steps, warmup) / 1e6, 2)
    finally:
        npm.local_geo_features = keep
    return r


def _malloc_probe(dev, mb=64, n=3):
    try:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        t_a, t_f = [], []
        for _ in range(n):
            t0 = time.perf_counter()
            x = torch.empty(mb << 20, dtype=torch.uint8, device=dev)
            x[:1] = 0
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            del x
            torch.cuda.empty_cache()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            t_a.append((t1 - t0) * 1e3)
            t_f.append((t2 - t1) * 1e3)
        return {"MB": mb, "alloc_ms": round(sorted(t_a)[n // 2], 3), "free_ms": round(sorted(t_f)[n // 2], 3)}
    except Exception as e:      # never let a probe take the line down
        return {"error": repr(e)}


def _alloc_traffic(step, dev, n=3):
    """Allocator traffic of `n` steady-state steps (torch.cuda.memory_stats deltas per step): a step that frees by
    reference counting finds every block in torch's cache — device allocations per step mean a hipMalloc each (tens of
    microseconds; milliseconds on some boxes) and usually a reference cycle through an autograd ctx."""
    step()
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_stats(dev)
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    m1 = torch.cuda.memory_stats(dev)
    d = lambda k: (m1.get(k, 0) - m0.get(k, 0)) / float(n)
    return {"num_device_alloc": round(d("num_device_alloc"), 2), "num_device_free": round(d("num_device_free"), 2),
            "active_MB_delta": round(d("active_bytes.all.current") / 2**20, 2),
            "reserved_MB_delta": round(d("reserved_bytes.all.current") / 2**20, 2)}


def bench_sdf_step(npm, dec, dev, steps, warmup, B, with_adam=True):
    """One iteration of the SDF mapping loop exactly as an unmodified mapper runs it (utils/mapper.py:822-905 with the
    shipped defaults, utils/config.py:170-181: BCE main loss, numerical Eikonal gradient on every 10th sample inside the
    free-space band, weight_e 0.5): `query_feature(coord, ts)` with the training-mode side effects -> `Decoder.sdf` ->
    IDW sum -> boolean-mask selection of the Eikonal samples (the mapper's own host synchronisation) ->
    `get_numerical_gradient` (six shifted queries per sample through `Mapper.sdf`) -> BCE + Eikonal -> backward to
    `local_geo_features` and the decoder (-> Adam step, reported separately).  Everything the mapper calls is bound to
    this package the way INTEGRATION.md binds it (`neural_points.install`, `decoder.install`, `mapper_ops.install`)."""
    from types import SimpleNamespace as NS_

    from pings_amd import decoder as hdec, mapper_ops as hmap, neural_points as hnp

    L = _lib_handle()
    keep = npm.local_geo_features
    P_ = [torch.nn.Parameter(t.detach().clone()) for t in (dec.layers[0].weight, dec.layers[0].bias, dec.lout.weight, dec.lout.bias)]
    dec_t = NS_(layers=[NS_(weight=P_[0], bias=P_[1])], lout=NS_(weight=P_[2], bias=P_[3]), sdf_scale=dec.sdf_scale,
                use_leaky_relu=False)
    feats = torch.nn.Parameter(keep.detach().clone())
    npm.local_geo_features = feats
    cfg = NS_(weighted_first=False, color_on=False, semantic_on=False, numerical_grad=True, gradient_decimation=10,
              voxel_size_m=float(npm.resolution), num_grad_step_ratio=0.2, free_sample_end_dist_m=0.5,
              loss_weight_on=False, ekional_loss_on=True, weight_e=0.5)
    mapper = NS_(neural_points=npm, sdf_mlp=dec_t, config=cfg, dtype=torch.float32, device=dev)
    g = torch.Generator(device=dev).manual_seed(11)
    coord = sdf_queries(npm, B, dev, seed=13)
    sdf_label = 0.25 * torch.randn(B, generator=g, device=dev)
    ts = torch.zeros(B, dtype=torch.int32, device=dev)
    weight = torch.ones(B, device=dev)
    sigma = float(dec.sdf_scale)
    bce = torch.nn.BCEWithLogitsLoss(reduction="mean")
    leaves = [feats] + P_
    opt = torch.optim.Adam([{"params": [feats], "lr": 0.01}, {"params": P_, "lr": 0.01}], betas=(0.9, 0.99), eps=1e-15)
    eps = cfg.voxel_size_m * cfg.num_grad_step_ratio
    info = {}

    def iteration(adam):
        apply_eikonal_mask = torch.abs(sdf_label) < cfg.free_sample_end_dist_m                       # :843
        geo_feature, _, weight_knn, _, certainty = hnp.query_feature(npm, coord, ts, query_color_feature=False)
        sdf_pred = hdec.sdf(dec_t, geo_feature)                                                         # :858
        sdf_pred = torch.sum(sdf_pred * weight_knn, dim=1).squeeze(1)                                   # :861
        coord_for_eikonal = coord[apply_eikonal_mask]                                                   # :872
        sdf_pred_for_eikonal = sdf_pred[apply_eikonal_mask]
        grad = hmap.get_numerical_gradient(mapper, coord_for_eikonal[::cfg.gradient_decimation],
                                           sdf_pred_for_eikonal[::cfg.gradient_decimation], eps)        # :878-882
        w_ = torch.abs(weight).detach()
        label_op = torch.sigmoid(sdf_label / sigma)                                                     # loss.py:61-62
        loss = bce(sdf_pred / sigma, label_op)
        loss = loss + cfg.weight_e * ((grad.norm(2, dim=-1) - 1.0) ** 2).mean()                          # :916-921
        opt.zero_grad(set_to_none=True)                                                                 # :959-961
        loss.backward()
        if adam:
            opt.step()
        info["eikonal_samples"] = int(grad.shape[0])
        return w_

    out = {"B": B}
    try:
        t_nb = _timeit(lambda: iteration(False), steps, warmup)
        pr = _prof_run(L, lambda: iteration(False), max(2, steps // 4))
        out["device_allocs_per_iteration"] = _alloc_traffic(lambda: iteration(False), dev)
        out.update({"ms_per_iteration": round(t_nb * 1e3, 4), "Msamples_s": round(B / t_nb / 1e6, 2),
                    "eikonal_samples": info["eikonal_samples"], "shifted_queries": 6 * info["eikonal_samples"],
                    "stage_ms": {k: round(v, 4) for k, v in sorted(pr.items(), key=lambda kv: -kv[1])},
                    "stage_ms_sum": round(sum(pr.values()), 4)})
        if with_adam:
            t_a = _timeit(lambda: iteration(True), steps, warmup)
            out["ms_per_iteration_with_adam"] = round(t_a * 1e3, 4)
            out["Msamples_s_with_adam"] = round(B / t_a / 1e6, 2)
    finally:
        npm.local_geo_features = keep
    return out


def ssim_pmc_traffic(W, H):
    """HBM bytes of one ssim_fwd + ssim_bwd launch pair from the committed PMC summary of tools/ssim_pmc.py (1080p x 3,
    streaming kernels: 2 x FETCH_SIZE + WRITE_SIZE), or None for another image size / no summary."""
    if (W, H) != (1920, 1080):
        return None
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
    try:
        files = sorted(os.path.join(d, f) for d, _, fs in os.walk(root) for f in fs if f.endswith("ssim_pmc_traffic.json"))
        data = json.load(open(files[-1]))
        # (ssim_fwd_kernel / ssim_bwd_kernel: the tile kernels of rounds 1-3; ssim_*_sw_kernel: the sliding-window ones)
        tot = sum(v["hbm_bytes_corrected"] for k, v in data.items() if k.startswith(("ssim_fwd_", "ssim_bwd_")))
        return int(tot) or None
    except Exception:
        return None


def _lib_handle():
    from pings_amd import _lib

    L = _lib.lib()
    L.pings_prof_enable.argtypes = [C.c_int]
    L.pings_prof_report.argtypes = [C.c_char_p, C.c_size_t]
    L.pings_prof_only.argtypes = [C.c_char_p]
    return L


def bench_ssim(dev, steps, warmup, W=1920, H=1080):
    """fused-SSIM (utils/mapper.py:1243) forward + backward at 1080p, 3 channels.  Byte model: forward
    reads both images (2 x 4 B) and, in training mode, writes the three partial-derivative maps (3 x 4 B) per
    pixel-channel; backward re-reads the maps and both images (5 x 4 B) and writes the gradient (4 B)."""
    from pings_amd.ssim import fused_ssim

    L = _lib_handle()
    g = torch.Generator(device=dev).manual_seed(6)
    a = torch.rand(1, 3, H, W, generator=g, device=dev).requires_grad_(True)
    b = (a.detach() + 0.1 * torch.randn(1, 3, H, W, generator=g, device=dev)).clamp(0, 1)

    def step():
        a.grad = None
        fused_ssim(a, b).backward()

    t_wall = _timeit(step, steps, warmup)
    pr = _prof_run(L, step, steps)
    t_f, t_b = pr["ssim_fwd"] * 1e-3, pr["ssim_bwd"] * 1e-3
    n = 3 * H * W
    bf, bb = 20 * n, 24 * n
    return {"width": W, "height": H, "channels": 3, "fwd_ms": round(t_f * 1e3, 4), "bwd_ms": round(t_b * 1e3, 4),
            "fwd_bwd_wall_ms": round(t_wall * 1e3, 4), "Mpix_s_fwd_bwd_kernels": round(H * W / (t_f + t_b) / 1e6, 1),
            "roofline": {"kernel": "ssim_fwd+ssim_bwd", "bound": "hbm", "achieved": round((bf + bb) / (t_f + t_b) / 1e9, 1),
                         "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round((bf + bb) / (t_f + t_b) / 1e9 / HBM_PEAK_GBS, 4),
                         "fwd_GBs": round(bf / t_f / 1e9, 1), "bwd_GBs": round(bb / t_b / 1e9, 1),
                         "algorithmic_bytes": bf + bb, "traffic": ssim_pmc_traffic(W, H)}}


def _surfel_rast(hr, dev, W, H, fx, fy):
    cam = camera(W, H, fx, fy, W / 2 - 0.5, H / 2 - 0.5, 0.05, 110.0, 0, dev)
    rs = hr.SurfelRasterizationSettings(
        image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=torch.ones(3, device=dev),
        scale_modifier=1.0, viewmatrix=cam["viewmatrix"], projmatrix=cam["projmatrix"],
        projmatrix_raw=cam["projmatrix_raw"], patch_bbox=torch.tensor([0, 0, H - 1, W - 1], dtype=torch.float32, device=dev),
        prcppoint=cam["prcppoint"], sh_degree=0, campos=cam["campos"], prefiltered=False, debug=False,
        config=torch.tensor([1, 1, 1, 1, 1], dtype=torch.float32, device=dev))
    return hr.SurfelGaussianRasterizer(rs)


def bench_raster_workload(dev, name, cloud, W, H, fx, steps, warmup):
    """Rasteriser forward + backward on one more workload shape ('also reported at C2, C3'), same step as
    the headline: Mpix/s, instance count, longest tile list and the stage times."""
    from pings_amd import rasterizer as hr

    L = _lib_handle()
    rast = _surfel_rast(hr, dev, W, H, fx, fx)
    params = [t.requires_grad_(True) for t in cloud]
    theta = torch.zeros(3, device=dev, requires_grad=True)
    rho = torch.zeros(3, device=dev, requires_grad=True)
    gg = torch.Generator(device=dev).manual_seed(7)
    ups = [torch.randn(c, H, W, generator=gg, device=dev) for c in (3, 3, 1, 1)]

    def step():
        for p_ in params + [theta, rho]:
            p_.grad = None
        img, nrm, dep, alp, radii, contrib = rast(means3D=params[0], means2D=torch.zeros_like(params[0]),
                                                  colors_precomp=params[1], opacities=params[2], scales=params[3],
                                                  rotations=params[4], theta=theta, rho=rho)
        torch.autograd.backward([img, nrm, dep, alp], ups)
        return radii

    radii = step()
    t = _timeit(step, steps, warmup)
    pr = _prof_run(L, step, max(2, steps // 4))
    with torch.no_grad():
        fs, _, _ = hr._forward(rast._prepared(), *[p_.detach() for p_ in params])
        _, rg_, _, nc_ = hr.debug_lists(fs)
        lens = rg_[:, 1] - rg_[:, 0]
    P = params[0].shape[0]
    return {"workload": name, "gaussians": P, "width": W, "height": H, "ms_per_step": round(t * 1e3, 4),
            "Mpix_s": round(W * H / t / 1e6, 1), "instances": int(fs.I), "visible_gaussians": int((radii > 0).sum().item()),
            "mean_list_len_per_tile": round(float(lens.float().mean()), 1), "longest_list": int(lens.max()),
            "max_contributors_per_pixel": int(nc_.max()),
            "kernels_ms": {k: round(v, 4) for k, v in pr.items()}}


class _BenchDecoder(torch.nn.Module):
    """Duck-typed `Decoder` (model/decoder.py:15-98): one hidden level, ReLU, bias."""

    def __init__(self, fin, hidden, out_dim, K, gen, device):
        super().__init__()
        self.layers = torch.nn.ModuleList([torch.nn.Linear(fin, hidden)])
        self.lout = torch.nn.Linear(hidden, out_dim * K)
        with torch.no_grad():
            self.layers[0].weight.copy_(torch.randn(hidden, fin, generator=gen) / fin ** 0.5)
            self.layers[0].bias.copy_(0.1 * torch.randn(hidden, generator=gen))
            self.lout.weight.copy_(torch.randn(out_dim * K, hidden, generator=gen) / hidden ** 0.5 * 0.5)
            self.lout.bias.copy_(0.1 * torch.randn(out_dim * K, generator=gen))
        self.out_k, self.mlp_out_dim, self.use_leaky_relu = K, out_dim * K, False
        self.to(device)


def bench_render_step(dev, steps, warmup, W=1920, H=1080, n_points=160_000, K=8, exchange=None):
    """One iteration of the Gaussian-mapping loop body as an unmodified mapper reaches it (utils/mapper.py:1126-1295,
    :1581): `render()` (markVisible -> spawn + the five decoders -> rasterise -> depth2normal -> exposure), the
    photometric loss block, fused-SSIM, backward to the neural-point features, the decoders, exposure and pose.
    The rasteriser object is constructed inside render() on every call, as the reference does (:149-201).
    n_points neural points on a street-like surface, K Gaussians each (F_g 32, F_c 16, hidden 128, pings.py:156-160).

    exchange = (world, rank) with world > 1: the multi-view step of SURVEY 8e as a training script would run it
     — every rank renders ITS camera of the rig (yawed by rank) over the same local map; the five
    decoders' parameters live in a hooked `GradBucket` (`zero(1)`; the all-reduce is fired from the post-accumulate
    hook of the last decoder gradient, i.e. from inside `loss.backward()`, while the spawn gather adjoint and the
    feature scatter still run), and the feature-table gradients — the ACTUAL spawn / decoder adjoint — travel through
    `RowSparseExchange` with the rows this view touched.  Called by every rank; the returned time is the max."""
    import math as _m
    from pings_amd import _lib
    from pings_amd.camera import Camera
    from pings_amd.image_losses import image_losses
    from pings_amd.renderer import render
    from pings_amd.ssim import fused_ssim

    L = _lib_handle()
    sys.path.insert(0, str(ROOT / "tests"))
    from scenes import street_scene

    g = torch.Generator().manual_seed(8)
    pos, base_col, _, _, _ = street_scene(n_points, device=dev, seed=2)
    n = pos.shape[0]
    quat = torch.tensor([1.0, 0, 0, 0], device=dev).repeat(n, 1)
    geo = (0.3 * torch.randn(n + 1, 32, generator=g)).to(dev).requires_grad_(True)
    cfe = (0.3 * torch.randn(n + 1, 16, generator=g)).to(dev).requires_grad_(True)
    decs = {"gauss_xyz": _BenchDecoder(32, 128, 3, K, g, dev), "gauss_rot": _BenchDecoder(32, 128, 4, K, g, dev),
            "gauss_scale": _BenchDecoder(32, 128, 3, K, g, dev), "gauss_alpha": _BenchDecoder(32, 128, 1, K, g, dev),
            "gauss_color": _BenchDecoder(16 + 3, 128, 3, K, g, dev)}
    data = {"position": pos, "orientation": quat, "color": base_col, "geo_feature": geo, "color_feature": cfe,
            "resolution": 0.2, "free_mask": torch.zeros(n, dtype=torch.bool, device=dev),
            "valid_mask": torch.ones(n, dtype=torch.bool, device=dev)}
    fx = 1000.0 * W / 1920.0
    T_cw = torch.eye(4, dtype=torch.float64)
    world, rank = exchange if exchange else (1, 0)
    if world > 1:      # the cameras of a rig: same position, yawed 25 degrees apart around the vertical (y) axis
        a = _m.radians(25.0 * (rank - 0.5 * (world - 1)))
        T_cw[0, 0], T_cw[0, 2], T_cw[2, 0], T_cw[2, 2] = _m.cos(a), -_m.sin(a), _m.sin(a), _m.cos(a)
    cam = Camera(W, H, fx, fx, W / 2 - 0.5, H / 2 - 0.5, 0.05, 110.0, T_cw, device=dev)
    bg = torch.ones(3, device=dev)
    gd = torch.Generator(device=dev).manual_seed(9)
    gt_rgb = torch.rand(3, H, W, generator=gd, device=dev)
    gt_depth = 2.0 + 40.0 * torch.rand(1, H, W, generator=gd, device=dev)
    sky = torch.rand(1, H, W, generator=gd, device=dev) < 0.1
    dec_params = [p for d in decs.values() for p in d.parameters()]
    per_view = [cam.exposure_mat, cam.exposure_offset, cam.cam_rot_delta, cam.cam_trans_delta]   # stay local (tools.py:291-337)
    leaves = [geo, cfe] + per_view + ([] if world > 1 else dec_params)
    info = {}
    bucket = ex = None
    if world > 1:
        from pings_amd import dist as pdist

        bucket = pdist.GradBucket(dec_params, overlap=True)      # p.grad become views of ONE flat buffer, hooks armed
        ex = pdist.RowSparseExchange()

    def step():
        for p_ in leaves:
            p_.grad = None
        if bucket is not None:
            bucket.zero(1)                                        # one backward pass (one view) on this rank
        pkg = render(cam, None, data, decs, None, bg, view_concat_on=True, learn_color_residual=True, d2n_on=True,
                     gs_type="gaussian_surfel")
        if pkg is not None:       # (None = a view that sees fewer than ten neural points, gaussian_renderer:224-292: such
            # a rank still takes part in the exchange below, with no rows)
            il = image_losses(pkg["render"], gt_rgb, pkg["surf_depth"], gt_depth, pkg["rend_alpha"], pkg["rend_normal"],
                              pkg["surf_normal"], sky, depth_min=0.3, depth_max=80.0, depth_min_accu_alpha=0.4)
            ssim = fused_ssim(pkg["render"].unsqueeze(0), gt_rgb.unsqueeze(0))
            loss = 0.8 * il.rgb_l1 + 0.2 * (1.0 - ssim) + 0.5 * il.depth_l1 + 0.05 * il.normal_depth_consist + 0.1 * il.sky
            loss.backward()                                       # world > 1: the decoder bucket's all-reduce starts in here
            info["gaussians"] = int(pkg["gaussian_xyz"].shape[0])
            info["visible_ratio"] = pkg["visible_neural_point_ratio"]
        elif bucket is not None:
            bucket.skip_backward()                                # keep the collective order: bucket, then rows
        if ex is not None:
            # rows of the [n + 1, 48] feature-gradient table this view wrote: the neural points it decoded (mapper.py:1581-1584)
            zg = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
            tab = torch.cat([zg(geo), zg(cfe)], 1)
            rows = torch.nonzero(tab.abs().amax(1) > 0).flatten()   # the count is a host value: it sizes the gather
            ex.reduce_(tab, rows)
            geo.grad, cfe.grad = tab[:, :32], tab[:, 32:]
            bucket.finish()                                       # before opt.step()
            info["exchange"] = dict(ex.last)

    step()
    _lib.sync_counts(reset=True)
    step()
    syncs = _lib.sync_counts(reset=True)
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
    t = _timeit(step, steps, warmup)
    if world > 1:
        tt = torch.tensor([t], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        t = tt.item()
        bucket.close()
        return {"width": W, "height": H, "neural_points": n, "views": world, "gaussians_rasterised_rank0": info.get("gaussians", 0),
                "ms_per_step": round(t * 1e3, 4), "Mpix_s_all_views": round(world * W * H / t / 1e6, 1),
                "exchange": info.get("exchange"),
                "bucket": "GradBucket(overlap=True).zero(1): the decoders' all-reduce is launched by the post-accumulate "
                          "hook inside loss.backward(); finish() before the optimiser step",
                "feature_rows": "RowSparseExchange on the [n + 1, 48] table of the real spawn / decoder adjoint"}
    pr = _prof_run(L, step, max(2, steps // 4))
    groups = {"decoders_fwd": ("mlp_fwd",), "decoders_bwd": ("mlp_bwd",), "ssim": ("ssim_fwd", "ssim_bwd"),
              "image_losses": ("image_losses_fwd", "image_losses_bwd")}
    # allocator traffic of the timed steps (a steady-state step should find every block in torch's cache: a device
    # allocation or free per step is a hipMalloc / hipFree with its implicit device wait)
    ms0 = torch.cuda.memory_stats(dev)
    seg0 = {sg["address"]: sg["total_size"] for sg in torch.cuda.memory_snapshot()}
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    ms1 = torch.cuda.memory_stats(dev)
    seg1 = {sg["address"]: sg["total_size"] for sg in torch.cuda.memory_snapshot()}
    allocs = {k: (ms1.get(k, 0) - ms0.get(k, 0)) / 3.0 for k in ("num_device_alloc", "num_device_free", "num_alloc_retries")}
    allocs["reserved_MB_delta_per_step"] = (ms1.get("reserved_bytes.all.current", 0) - ms0.get("reserved_bytes.all.current", 0)) / 3.0 / 2**20
    allocs["active_MB_delta_per_step"] = (ms1.get("active_bytes.all.current", 0) - ms0.get("active_bytes.all.current", 0)) / 3.0 / 2**20
    new_segs = sorted((sz for a_, sz in seg1.items() if a_ not in seg0), reverse=True)
    allocs["new_segments_in_3_steps"] = len(new_segs)
    allocs["largest_new_segment_MB"] = (new_segs[0] / 2**20) if new_segs else 0.0
    anomaly = None
    if t * 1e3 > 3.0 * max(sum(pr.values()), 1e-3):
        # The wall clock is several times the kernels' sum: some boxes of the pool wake a blocked host wait only on a
        # timer tick (round 3 saw 16 ms steps; the library's own waits poll pinned memory since).  Say WHERE the time
        # goes: each phase's issue time and the wait behind it, medians of five steps, plus the cost of an idle wait.
        ph = {k: [] for k in ("render_issue", "render_wait", "loss_issue", "loss_wait", "backward_issue", "backward_wait")}
        for _ in range(5):
            for p_ in leaves:
                p_.grad = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pkg = render(cam, None, data, decs, None, bg, view_concat_on=True, learn_color_residual=True, d2n_on=True,
                         gs_type="gaussian_surfel")
            t1 = time.perf_counter(); torch.cuda.synchronize(); t2 = time.perf_counter()
            il = image_losses(pkg["render"], gt_rgb, pkg["surf_depth"], gt_depth, pkg["rend_alpha"], pkg["rend_normal"],
                              pkg["surf_normal"], sky, depth_min=0.3, depth_max=80.0, depth_min_accu_alpha=0.4)
            ssim = fused_ssim(pkg["render"].unsqueeze(0), gt_rgb.unsqueeze(0))
            loss = 0.8 * il.rgb_l1 + 0.2 * (1.0 - ssim) + 0.5 * il.depth_l1 + 0.05 * il.normal_depth_consist + 0.1 * il.sky
            t3 = time.perf_counter(); torch.cuda.synchronize(); t4 = time.perf_counter()
            loss.backward()
            t5 = time.perf_counter(); torch.cuda.synchronize(); t6 = time.perf_counter()
            for k_, v_ in zip(ph, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4, t6 - t5)):
                ph[k_].append(v_ * 1e3)
        idle = []
        for _ in range(5):
            t0 = time.perf_counter(); torch.cuda.synchronize(); idle.append((time.perf_counter() - t0) * 1e3)
        tiny = torch.zeros(1, device=dev)
        item = []
        for _ in range(5):
            t0 = time.perf_counter(); tiny.add_(1.0).item(); item.append((time.perf_counter() - t0) * 1e3)
        med = lambda v: round(sorted(v)[len(v) // 2], 3)
        anomaly = {"note": "wall > 3x the kernels' sum on this box: per-phase host times (ms, medians of 5 synchronised steps)",
                   "phases_ms": {k_: med(v_) for k_, v_ in ph.items()}, "idle_synchronize_ms": med(idle),
                   "one_element_item_ms": med(item)}
    return {"width": W, "height": H, "neural_points": n, "gaussians_rasterised": info["gaussians"],
            "device_allocs_per_step": {k: round(float(v), 2) for k, v in allocs.items()}, "timing_anomaly": anomaly,
            "visible_neural_point_ratio": round(float(info["visible_ratio"]), 3), "ms_per_step": round(t * 1e3, 4),
            "Mpix_s": round(W * H / t / 1e6, 1), "host_syncs_per_render": syncs,
            "host_syncs_total": int(sum(syncs.values())),
            "stage_ms": {k: round(v, 4) for k, v in sorted(pr.items(), key=lambda kv: -kv[1])},
            "stage_ms_sum": round(sum(pr.values()), 4),
            "grouped_ms": {k: round(sum(pr.get(n_, 0.0) for n_ in v), 4) for k, v in groups.items()}}


def cpu_baseline_sdf(npm, dec, B=131072, reps=8, weighted_first=False, label="1M-point map"):
    """The reference's PyTorch-CPU SDF path (oracle port: same torch op sequence) on the host cores, one process,
    same map and queries as the GPU run (tensors copied to the host); the torch thread count is the fastest of
    8..128 on this host (the survey container's 8 vCPUs gave 0.26-0.36 Msamples/s)."""
    from oracle import sdf_cpu

    c = lambda t: t.detach().cpu().numpy()
    st = dict(buffer_size=int(npm.buffer_pt_index.shape[0]), buffer_pt_index=c(npm.buffer_pt_index),
              neural_points=c(npm.neural_points), point_orientations=c(npm.point_orientations),
              geo_features=c(npm.geo_features), point_ts_create=c(npm.point_ts_create),
              point_ts_update=c(npm.point_ts_create), point_certainties=c(npm.point_certainties),
              free_gs_mask=c(npm.free_gs_mask), valid_gs_mask=c(npm.valid_gs_mask), travel_dist=c(npm.travel_dist),
              cur_ts=0, diff_travel_dist_local=1e9, local_neural_points=c(npm.neural_points),
              local_point_orientations=c(npm.point_orientations), local_geo_features=c(npm.geo_features),
              local_point_certainties=c(npm.point_certainties), local_point_ts_update=c(npm.point_ts_create),
              global2local=c(npm.global2local), neighbor_dx=c(npm.neighbor_dx), max_valid_dist2=npm.max_valid_dist2,
              resolution=npm.resolution, after_pgo=False, temporal_local_map_on=False, nn_k=6,
              weighted_first=weighted_first)
    cm = sdf_cpu.NeuralPointMap(st)
    mlp = sdf_cpu.MLP(dec.layers[0].weight.cpu(), dec.layers[0].bias.cpu(), dec.lout.weight.cpu(), dec.lout.bias.cpu(),
                      dec.sdf_scale)
    x = sdf_queries(npm, B, npm.neural_points.device).cpu()
    with torch.no_grad():
        sdf_cpu.mapper_sdf(cm, mlp, x)  # warm-up
        threads = best_threads(lambda: sdf_cpu.mapper_sdf(cm, mlp, x[:min(B, 32768)]))
        t0 = time.time()
        for _ in range(reps):
            s, _ = sdf_cpu.mapper_sdf(cm, mlp, x)
        dt = (time.time() - t0) / reps
    return {"value": round(B / dt / 1e6, 4), "unit": "Msamples/s", "cores": threads, "kind": "port",
            "sample": f"oracle/sdf_cpu.py (reference torch op sequence) forward, 1 process, B={B} queries x {reps} reps on "
                      f"the same {label} ({dt * reps:.1f} s of CPU work, {threads} torch threads = the fastest of 8..128; "
                      f"host has {os.cpu_count()} logical cores)"}, s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--mode", default="surfel", choices=["surfel", "3dgs"])
    ap.add_argument("--full", action="store_true",
                    help="after the headline, measure and check everything else: per-kernel times and roofline, "
                         "CPU-oracle baselines and parity, Metric 2 (SDF) and the secondary legs")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU-oracle legs")
    ap.add_argument("--no-sdf", action="store_true", help="--full without Metric 2 and the secondary legs")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for N > 1 (nccl = RCCL)")
    ap.add_argument("--exchange-leg", action="store_true",
                    help="--full, N > 1: run the render_step_exchange leg even with --no-sdf (rehearsals)")
    ap.add_argument("--single-device", action="store_true",
                    help="rehearsal only: put every rank on cuda:0 (use with --backend gloo)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (rasteriser outputs and parameter "
                         "gradients of rank 0) as DIR/<name>.npy, under 64 MB in all (see dump_outputs)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.exchange_leg and not args.full:
        ap.error("--exchange-leg is a leg of --full")

    # backward passes run on the calling thread: the hand-off to autograd's per-device worker thread and back costs
    # 40-300 us per backward() depending on the box (measured: a two-operator graph 40 vs 73 us, the fused SDF step 178
    # vs 463 us on two boxes of this pool), which is the whole budget of a 0.16 ms training step.  One line in the
    # training script; no kernel, result or launch order changes.
    if os.environ.get("PINGS_BENCH_AUTOGRAD_MT", "0") != "1":      # A/B switch: 1 = torch's default worker thread
        torch.autograd.set_multithreading_enabled(False)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    assert torch.cuda.is_available(), "bench.py needs a HIP device"
    if args.single_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(args.backend, rank=rank, world_size=world)

    from pings_amd import _lib, dist as pdist, rasterizer as hr

    L = _lib.lib()
    L.pings_prof_enable.argtypes = [C.c_int]
    L.pings_prof_report.argtypes = [C.c_char_p, C.c_size_t]
    L.pings_prof_only.argtypes = [C.c_char_p]

    P, W, H = args.gaussians, args.width, args.height
    fx = fy = 1000.0 * W / 1920.0
    cx, cy = W / 2 - 0.5, H / 2 - 0.5
    means, col, op, scales, rot = synth_cloud(P, W, H, fx, fy, dev, seed=42)  # same cloud on every rank
    settings = camera(W, H, fx, fy, cx, cy, 0.05, 110.0, rank, dev)
    surfel = args.mode == "surfel"
    if surfel:
        rs = hr.SurfelRasterizationSettings(
            image_height=H, image_width=W, tanfovx=settings["tanfovx"], tanfovy=settings["tanfovy"],
            bg=torch.ones(3, device=dev), scale_modifier=1.0, viewmatrix=settings["viewmatrix"],
            projmatrix=settings["projmatrix"], projmatrix_raw=settings["projmatrix_raw"],
            patch_bbox=torch.tensor([0, 0, H - 1, W - 1], dtype=torch.float32, device=dev),
            prcppoint=settings["prcppoint"], sh_degree=0, campos=settings["campos"], prefiltered=False, debug=False,
            config=torch.tensor([1, 1, 1, 1, 1], dtype=torch.float32, device=dev))
        rast = hr.SurfelGaussianRasterizer(rs)
    else:
        rs = hr.GS3DRasterizationSettings(
            image_height=H, image_width=W, tanfovx=settings["tanfovx"], tanfovy=settings["tanfovy"],
            bg=torch.ones(3, device=dev), scale_modifier=1.0, viewmatrix=settings["viewmatrix"],
            projmatrix=settings["projmatrix"], projmatrix_raw=settings["projmatrix_raw"], sh_degree=0,
            campos=settings["campos"], prefiltered=False, debug=False)
        rast = hr.GS3DGaussianRasterizer(rs)

    params = [t.requires_grad_(True) for t in (means, col, op, scales, rot)]
    theta = torch.zeros(3, device=dev, requires_grad=True)
    rho = torch.zeros(3, device=dev, requires_grad=True)
    gg = torch.Generator(device=dev).manual_seed(7)
    gC = torch.randn(3, H, W, generator=gg, device=dev)
    gN = torch.randn(3, H, W, generator=gg, device=dev)
    gD = torch.randn(1, H, W, generator=gg, device=dev)
    gA = torch.randn(1, H, W, generator=gg, device=dev)
    stats = {}
    # N > 1: the exchange step of a multi-view iteration (mapper.py:1581-1584): mean over ranks of the
    # gradients of local_geo_features [N_np+1, 32] + local_color_features [N_np+1, 16] (ONE [N_np+1, 48] table, row-
    # sparse: only the neural points this rank's view sees) and of the six decoder MLPs (flat bucket, async all-reduce
    # overlapped with the table exchange).  The timed step stays the rasteriser step of the headline metric; the
    # feature-gradient rows are the per-neural-point sums of the Gaussian gradients (8 Gaussians per point) — the
    # spawn / decoder adjoint that produces the real values is measured in `render_step`, not here.
    ex = None
    if world > 1:
        n_np = P // 8
        # neural point i owns the eight Gaussians own[8i .. 8i+7] of the cloud sorted by 1 m voxel (spatially coherent,
        # as the Gaussians a neural point spawns are): what a view sees is then a coherent subset of the rows
        vox = torch.floor(means.detach()).to(torch.int64) + (1 << 20)
        own = torch.argsort((vox[:, 0] << 42) + (vox[:, 1] << 21) + vox[:, 2])[:n_np * 8].contiguous()
        # the cameras of a rig look in different directions (IPB-Car: four, ipb_car.py:88-133): the local map holds every
        # camera's sector and a view touches the rows of its own, so the shared table has world x P/8 rows and rank r's
        # neural points are rows r P/8 ..
        g_tab = torch.zeros(world * n_np + 1, 48, device=dev)
        mlp_shapes = [(128, 32), (128,), (24, 128), (24,), (128, 32), (128,), (32, 128), (32,), (128, 32), (128,),
                      (24, 128), (24,), (128, 32), (128,), (8, 128), (8,), (128, 19), (128,), (24, 128), (24,),
                      (64, 35), (64,), (1, 64), (1,)]
        mlp_params = [torch.nn.Parameter(torch.zeros(*sh, device=dev)) for sh in mlp_shapes]
        b_mlp = pdist.GradBucket(mlp_params, overlap=True)   # hooked: p.grad are views of one flat buffer
        ex = pdist.RowSparseExchange()

    def exchange(radii):
        b_mlp.zero(1)                                       # one backward pass reaches the decoders on this rank
        g14 = torch.cat([params[0].grad, params[1].grad, params[2].grad, params[3].grad, params[4].grad], 1)
        g_np = g14[own].view(n_np, 8, 14).sum(1)
        # the decoders' gradients arrive through AUTOGRAD (a stand-in for the spawn adjoint, which `render_step_exchange`
        # runs for real): every parameter receives g_np.mean() from one backward pass, each accumulation runs the bucket's
        # post-accumulate hook and the LAST one launches the asynchronous all-reduce — the public path, no private call
        torch.autograd.backward([sum(p_.sum() for p_ in mlp_params)], [g_np.mean().detach()])
        # ... so the decoder bucket travels while the table is compacted
        seen = (radii[own].view(n_np, 8) > 0).any(1)
        local = torch.nonzero(seen).flatten()               # the count sizes the gather (`render` reads it back anyway)
        rows = local + rank * n_np
        g_tab.zero_()
        g_tab[rows] = torch.cat([g_np, g_np, g_np, g_np[:, :6]], 1)[local]
        ex.reduce_(g_tab, rows, n_rows=int(rows.numel()))   # geo + colour rows as ONE [N, 48] table
        b_mlp.finish()

    def step():
        for p_ in params + [theta, rho]:
            p_.grad = None
        m2d = torch.zeros_like(means)
        out = rast(means3D=params[0], means2D=m2d, colors_precomp=params[1], opacities=params[2],
                   scales=params[3], rotations=params[4], theta=theta, rho=rho)
        if surfel:
            img, nrm, dep, alp, radii, contrib = out
            torch.autograd.backward([img, nrm, dep, alp], [gC, gN, gD, gA])
        else:
            img, radii, dep, alp, nt = out
            torch.autograd.backward([img, dep, alp], [gC, gD, gA])
        if world > 1:
            exchange(radii)
        stats["visible"] = radii
        return out

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    RASTER_STAGES = ("blend_bwd", "blend_fwd", "tile_sort", "preprocess", "gaussian_bwd")  # stages with a byte model

    def report():
        buf = C.create_string_buffer(8192)
        _lib.check(L.pings_prof_report(buf, len(buf)), "pings_prof_report")
        return parse_prof(buf.value.decode())

    # Warm-up, with every stage of the library recorded (HIP events on the launch stream): the per-stage breakdown.
    # Each recorded stage puts two event packets between dependent launches (~10 us of idle GPU each), so the TIMED
    # region below records only the dominant kernel — the one the roofline figure is computed for — live.
    step()  # first call: code-object load, allocator growth
    sync()
    L.pings_prof_only(None)
    L.pings_prof_enable(1)
    for _ in range(max(args.warmup, 1)):
        step()
    sync()
    L.pings_prof_enable(0)
    prof_all = report()
    dom = max((k for k in prof_all if k in RASTER_STAGES), key=lambda k: prof_all[k][1] / prof_all[k][0])
    L.pings_prof_only(dom.encode())
    L.pings_prof_enable(1)
    # the timed region launches back to back (one recorded stage instead of fifteen): let the runtime grow its
    # signal / kernarg pools for that pattern before the clock starts (a one-off 10-16 ms stall was seen inside the
    # first timed steps of a fresh process otherwise)
    for _ in range(max(args.warmup, 2)):
        step()
    sync()
    report()
    host_ms = []
    t0 = time.perf_counter()
    for i in range(args.steps):
        ts = time.perf_counter()
        out = step()
        host_ms.append((time.perf_counter() - ts) * 1e3)  # host-side issue time only (no sync)
        if i < args.steps - 1:
            del out  # released before the next step allocates, as when the result was discarded; the last one is dumped
    sync()
    elapsed = time.perf_counter() - t0
    L.pings_prof_enable(0)
    L.pings_prof_only(None)
    prof = dict(prof_all)
    prof.update(report())  # the dominant stage as measured inside the timed region

    t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = t.item()
    ms_per_step = elapsed / args.steps * 1e3
    value = world * W * H / (elapsed / args.steps) / 1e6

    # what the last timed step handed its caller: the rasteriser's outputs and the gradients of its inputs
    dumped = None
    if args.dump_outputs and rank == 0:
        names = (("image", "normal", "depth", "alpha", "radii", "contributions") if surfel
                 else ("image", "radii", "depth", "alpha", "n_touched"))
        arrays = dict(zip(names, out))
        for n, p_ in zip(("means3D", "colors", "opacities", "scales", "rotations", "theta", "rho"), params + [theta, rho]):
            if p_.grad is not None:
                arrays[f"grad_{n}"] = p_.grad
        dumped = {"dir": args.dump_outputs, "arrays": dump_outputs(args.dump_outputs, arrays)}
        del arrays
    del out

    line = None
    if rank == 0:
        line = {
            "metric": "raster fwd+bwd Mpix/s @1M Gaussians 1080p",
            "value": round(value, 3), "unit": "Mpix/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"{args.mode} rasteriser fwd+bwd, {P} Gaussians, {W}x{H}, one view per GPU"
                                   + (", then the multi-view exchange of SURVEY 8e over RCCL: row-sparse all-gather of the "
                                      "visible neural points' feature-gradient rows (shared table [N x P/8 + 1, 48]: every "
                                      "camera of the rig sees its own sector of the local map) + all-reduce of the six "
                                      "decoder MLPs" if world > 1 else ""),
                       "exchange": (ex.last if ex is not None else None),
                       "rect_rule": {"tight": "tight: published 3-sigma tile square minus the tiles in which no pixel can "
                                              "pass alpha >= 1/255 (output-identical to the square; legs raster_rect_3sigma / "
                                              "raster_rect_ellipse of --full time the other two rules)",
                                     "3sigma": "3sigma: published 3DGS tile square",
                                     "ellipse": "ellipse: truncating alpha-ellipse box of rounds 1-3 (NOT output-identical)"}[
                           {"3": "3sigma", "e": "ellipse"}.get(os.environ.get("PINGS_RASTER_RECT", "t")[:1], "tight")],
                       "gaussians": P, "width": W, "height": H},
            # False = torch.autograd.set_multithreading_enabled(False), see the top of main()
            "autograd_multithreading": os.environ.get("PINGS_BENCH_AUTOGRAD_MT", "0") == "1",
            "hsa_enable_interrupt": os.environ.get("HSA_ENABLE_INTERRUPT"),   # see the top of this file
            "host_issue_ms_per_step": {"min": round(min(host_ms), 3), "median": round(sorted(host_ms)[len(host_ms) // 2], 3),
                                       "max": round(max(host_ms), 3)},
        }

    # Everything below measures or checks something other than the headline, each in runs of its own: --full only.
    # N > 1: the real multi-view mapping step (every rank takes part: collectives inside), VERDICT r3 #7
    rse = None
    if args.full and world > 1 and (not args.no_sdf or args.exchange_leg):
        try:
            rse = bench_render_step(dev, max(args.steps // 2, 5), 2, exchange=(world, rank))
        except Exception as e:  # noqa: BLE001
            rse = {"error": f"{type(e).__name__}: {e}"}
        for p_ in params:
            p_.grad = None
        torch.cuda.empty_cache()
        dist.barrier()

    if rank == 0 and args.full:
        # instance count of this view (for the algorithmic-bytes figures)
        prep = rast._prepared()
        with torch.no_grad():
            fs, radii, _ = hr._forward(prep, params[0].detach(), params[1].detach(), params[2].detach(),
                                       params[3].detach(), params[4].detach())
        I = fs.I
        HW = W * H
        # instances a tile actually blends (front-to-back termination): the units the blend kernels process
        _, rg_, _, nc_ = hr.debug_lists(fs)
        gx_, gy_ = math.ceil(W / 16), math.ceil(H / 16)
        ncp = torch.zeros(gy_ * 16, gx_ * 16, dtype=torch.int32, device=dev)
        ncp[:H, :W] = nc_
        I_proc = int(ncp.view(gy_, 16, gx_, 16).permute(0, 2, 1, 3).reshape(gy_ * gx_, 256).max(1).values.sum().item())
        per = {k: v[1] / v[0] for k, v in prof.items()}  # avg ms per launch
        # algorithmic bytes per launch (SURVEY.md §8d terms that belong to each kernel)
        alg = {
            "blend_bwd": 32 * HW + 8 * HW + 32 * HW + 48 * I_proc,
            "blend_fwd": 48 * I_proc + 32 * HW + 8 * HW,
            "tile_sort": 24 * I,
            "preprocess": 56 * P + 8 * P,
            "gaussian_bwd": 56 * P + 64 * P,
        }
        achieved = alg[dom] / (per[dom] * 1e-3) / 1e9
        traffic, traffic_src, valu_insts = pmc_traffic(dom, dict(gaussians=P, width=W, height=H, mode=args.mode))
        roofline = {"kernel": dom, "bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS,
                    "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": traffic,
                    "traffic_source": traffic_src,
                    # the blend kernels are vector-ALU bound: wave-instructions issued per launch (SQ_INSTS_VALU of the
                    # committed PMC pass) / measured time, against 256 CUs x 4 SIMDs x 2.4 GHz / 2 cycles per wave64 op
                    "valu": None if not valu_insts else {
                        "wave_insts": int(valu_insts), "achieved_Ginst_s": round(valu_insts / (per[dom] * 1e-3) / 1e9, 1),
                        "peak_Ginst_s": 1228.8, "frac": round(valu_insts / (per[dom] * 1e-3) / 1228.8e9, 4),
                        # fp32 flops next to the issue fraction.  Executed flops = wave-instructions x 64
                        # lanes x the flops per vector instruction of the kernel's record loop (static mix of
                        # blend_bwd_kernel<0,4>'s ISA: 362 vector instructions, 360 fp32 operations counting an fma as two
                        # and a packed op as two lanes - selects, compares and moves carry none), every lane counted as
                        # active: an UPPER bound of the useful work, against the 157.3 TFLOP/s fp32 vector peak
                        "flops_per_valu_inst": BLEND_BWD_FLOPS_PER_VALU,
                        "TFLOP_s": round(valu_insts * 64 * BLEND_BWD_FLOPS_PER_VALU / (per[dom] * 1e-3) / 1e12, 1),
                        "peak_TFLOP_s": 157.3,
                        "flop_frac": round(valu_insts * 64 * BLEND_BWD_FLOPS_PER_VALU / (per[dom] * 1e-3) / 157.3e12, 4)},
                    "avg_ms": round(per[dom], 4), "launches_timed": prof[dom][0], "algorithmic_bytes": int(alg[dom]),
                    "measured": "HIP events around this kernel on its launch stream, inside the timed region; the "
                                "other stages ('kernels') come from the warm-up steps with every stage recorded",
                    "note": "blend kernels are fp32-VALU bound (LDS-broadcast records, ~250 flop per "
                            "fetched byte); see DESIGN.md"}
        if roofline["valu"]:
            # what the chip actually sustains (profiles/valu_calib.hip, measured on the same kind of box): the guide's
            # 2 cycles per wave64 instruction are the `peak`; a kernel of nothing but independent v_fma_f32 reaches 70 % of
            # that with eight waves per SIMD and 64 % with four.  Reported next to `frac`, never instead of it.
            cal = valu_calibration()
            if cal:
                best = max(r["fma_Ginst_s"] for r in cal["results"])
                roofline["valu"].update({
                    "measured_issue_rate_Ginst_s": {f"fma_{r['waves_per_simd']}_waves_per_simd": r["fma_Ginst_s"]
                                                    for r in cal["results"]},
                    "frac_of_measured_fma_rate": round(roofline["valu"]["achieved_Ginst_s"] / best, 4),
                    "calibration": cal["_file"]})
            # ADVICE r2 / VERDICT r2 #4: the dominant kernel is vector-issue bound, so THAT is the roofline
            # it is priced against — wave-instructions per launch (SQ_INSTS_VALU of the committed PMC pass of this very
            # workload) / the duration measured live, against 256 CUs x 4 SIMDs x 2.4 GHz / 2 cycles per wave64
            # instruction; the HBM figure on algorithmic bytes stays next to it
            hbm = {k: roofline[k] for k in ("achieved", "peak", "unit", "frac", "algorithmic_bytes")}
            v = roofline["valu"]
            roofline.update({"bound": "valu", "achieved": v["achieved_Ginst_s"], "peak": v["peak_Ginst_s"],
                             "unit": "G wave-instructions/s", "frac": v["frac"], "hbm": hbm})
        kernels = {k: {"avg_ms": round(per[k], 4),
                       "alg_GBs": round(alg[k] / (per[k] * 1e-3) / 1e9, 1) if k in alg else None} for k in per}
        cpu = None
        if not args.no_cpu_baseline:
            cpu = cpu_baseline_raster(dev)
        sdf = None
        if not args.no_sdf:
            for p_ in params:
                p_.grad = None
            del fs
            torch.cuda.empty_cache()
            sdf, npm, dec = bench_sdf(dev, max(args.steps, 5), max(args.warmup, 2))
            if not args.no_cpu_baseline:
                sdf["cpu_baseline"], _ = cpu_baseline_sdf(npm, dec)
            del npm, dec
            torch.cuda.empty_cache()
        ks, kw = max(args.steps, 5), max(args.warmup, 2)
        extras = {}
        if not args.no_sdf:
            sys.path.insert(0, str(ROOT / "tests"))
            from scenes import room_scene, street_scene

            def leg(name, fn):
                # an extra leg must never take the headline line down with it: its failure is reported in place
                try:
                    extras[name] = fn()
                except Exception as e:  # noqa: BLE001
                    extras[name] = {"error": f"{type(e).__name__}: {e}"}
                torch.cuda.empty_cache()

            try:
                sdf.update(bench_sdf_sweep(dev, ks, kw, with_cpu=not args.no_cpu_baseline))
            except Exception as e:  # noqa: BLE001
                sdf["sweep_error"] = f"{type(e).__name__}: {e}"
            torch.cuda.empty_cache()
            leg("ssim", lambda: bench_ssim(dev, ks, kw))
            leg("raster_c2", lambda: bench_raster_workload(dev, "C2 Replica-like room, 200k surfels, 640x480",
                                                           room_scene(200_000, device=dev, seed=1), 640, 480, 600.0, ks, kw))
            leg("raster_c3", lambda: bench_raster_workload(dev, "C3 KITTI-like street, 1M surfels, 1392x512",
                                                           street_scene(1_000_000, device=dev, seed=1), 1392, 512, 720.0, ks, kw))
            leg("raster_c3_cloud", lambda: bench_raster_workload(
                dev, "SURVEY 8d cloud at the C3 shape, 1M Gaussians, 1392x512",
                synth_cloud(1_000_000, 1392, 512, 725.0, 725.0, dev, seed=42), 1392, 512, 725.0, ks, kw))

            def rect_leg(rule):
                # the headline workload under another tile-rectangle rule (csrc/raster_fwd.hip:preprocess_kernel): the
                # published square without the lossless trimming, and the truncating box rounds 1-3 were timed on
                prev = os.environ.get("PINGS_RASTER_RECT")
                os.environ["PINGS_RASTER_RECT"] = rule
                try:
                    return bench_raster_workload(dev, f"headline cloud, PINGS_RASTER_RECT={rule}",
                                                 synth_cloud(P, W, H, fx, fy, dev, seed=42), W, H, fx, ks, kw)
                finally:
                    if prev is None:
                        os.environ.pop("PINGS_RASTER_RECT", None)
                    else:
                        os.environ["PINGS_RASTER_RECT"] = prev

            leg("raster_rect_3sigma", lambda: rect_leg("3sigma"))
            leg("raster_rect_ellipse", lambda: rect_leg("ellipse"))
            leg("render_step", lambda: bench_render_step(dev, ks, kw))
            leg("decoder", lambda: bench_decoder(dev, ks, kw))
            leg("map_maintenance", lambda: bench_map(dev, with_cpu=not args.no_cpu_baseline))
            leg("image_losses", lambda: bench_image_losses(dev, ks, kw, with_cpu=not args.no_cpu_baseline))
        if rse is not None:
            extras["render_step_exchange"] = rse
        decoder, map_maint, img_losses = extras.pop("decoder", None), extras.pop("map_maintenance", None), \
            extras.pop("image_losses", None)
        line["config"].update({"instances": int(I), "instances_blended": I_proc,
                               "visible_gaussians": int((radii > 0).sum().item()),
                               "mean_list_len_per_tile": round(I / (math.ceil(W / 16) * math.ceil(H / 16)), 1)})
        line.update({
            # what a device allocation costs on THIS box (hipMalloc + first use / hipFree of 64 MB through torch, cache
            # emptied first): the map-maintenance leg allocates while the map grows, and any step that misses torch's cache
            # pays this per block (20 ms render steps on a box where it is milliseconds)
            "device_malloc_probe": _malloc_probe(dev),
            "secondary_legs_timing": "best of 3 runs of `steps` calls (bench._timeit); the headline is one run of K steps",
            "roofline": roofline, "kernels": kernels, "cpu_baseline": cpu, "sdf": sdf, "decoder": decoder,
            "map_maintenance": map_maint, "image_losses": img_losses, **extras,
        })
    if rank == 0:
        if dumped is not None:
            line["dump_outputs"] = dumped
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.destroy_process_group()


# --------------------------------------------------------------------------- camera helper
class oracle_free_camera:  # namespace, so the timed path does not import oracle/
    @staticmethod
    def projection(W, H, fx, fy, cx, cy, znear, zfar, T_cw, device):
        """CamImage's matrices (cameras.py:57-70,207-219; graphics_utils.py:54-76) as fp32 device tensors."""
        tanfovx, tanfovy = W / (2.0 * fx), H / (2.0 * fy)
        top, bottom = znear * cy / fy, -znear * (H - cy) / fy
        right, left = znear * (W - cx) / fx, -znear * cx / fx
        Pm = torch.zeros(4, 4, dtype=torch.float64)
        Pm[0, 0] = 2.0 * znear / (right - left)
        Pm[1, 1] = 2.0 * znear / (top - bottom)
        Pm[0, 2] = -(right + left) / (right - left)
        Pm[1, 2] = (top + bottom) / (top - bottom)
        Pm[3, 2] = 1.0
        Pm[2, 2] = zfar / (zfar - znear)
        Pm[2, 3] = -(zfar * znear) / (zfar - znear)
        view = T_cw.T.contiguous()
        proj_raw = Pm.T.contiguous()
        f = lambda t: t.to(torch.float32).to(device).contiguous()
        return dict(tanfovx=tanfovx, tanfovy=tanfovy, viewmatrix=f(view), projmatrix=f(view @ proj_raw),
                    projmatrix_raw=f(proj_raw), campos=f(torch.linalg.inv(view)[3, :3]),
                    prcppoint=torch.tensor([cx / W, cy / H], dtype=torch.float32, device=device))


sys.modules["oracle_free_camera"] = oracle_free_camera  # type: ignore

if __name__ == "__main__":
    main()
