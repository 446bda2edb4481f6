"""Forward + backward time of the 2DGS backend next to the surfel backend on the same scene.

    python tools/raster2d_time.py [steps]

Two shapes: C2 (200k Gaussians of the room scene, 640x480) and the headline shape (1M Gaussians of the Metric-1 cloud,
1920x1080).  The surfel backend gets the scene's three scale columns, the 2DGS backend the first two.  The two backends
alternate step by step in one process (warm-up first); every step is one forward + backward of
sum(image * g) + sum(aux * g') with fixed random upstream maps, timed with HIP events.  Prints one JSON line:
{shape: {"surfel_ms": median, "2dgs_ms": median, "ratio": 2dgs / surfel, "visible_2dgs": Gaussians with
radius > 0 in the 2DGS run}}.
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import bench
from pings_amd import rasterizer as rz
from scenes import room_scene


def _camera(W, H, fx, dev):
    zn, zf = 0.05, 110.0
    P = torch.zeros(4, 4, device=dev)
    P[0, 0], P[1, 1], P[2, 2], P[2, 3], P[3, 2] = 2 * fx / W, 2 * fx / H, zf / (zf - zn), -zf * zn / (zf - zn), 1.0
    view = torch.eye(4, device=dev)
    return view.T.contiguous(), (view.T @ P.T).contiguous(), P.T.contiguous()


def _rasterizers(W, H, fx, dev):
    view, full, raw = _camera(W, H, fx, dev)
    common = dict(image_height=H, image_width=W, tanfovx=W / (2 * fx), tanfovy=H / (2 * fx),
                  bg=torch.ones(3, device=dev), scale_modifier=1.0, viewmatrix=view, projmatrix=full, sh_degree=0,
                  campos=torch.zeros(3, device=dev), prefiltered=False, debug=False)
    surf = rz.SurfelGaussianRasterizer(rz.SurfelRasterizationSettings(
        projmatrix_raw=raw, patch_bbox=torch.tensor([0.0, 0, H - 1, W - 1], device=dev),
        prcppoint=torch.tensor([0.5, 0.5], device=dev), config=torch.tensor([1.0, 1, 1, 1, 0], device=dev), **common))
    two = rz.Surfel2DGaussianRasterizer(rz.Surfel2DRasterizationSettings(**common))
    return surf, two


def measure(name, scene, W, H, fx, steps, warmup, dev):
    xyz, col, opa, sca, rot = [t.to(dev).float().contiguous() for t in scene]
    surf, two = _rasterizers(W, H, fx, dev)
    g = torch.Generator(device=dev).manual_seed(0)
    gi = torch.randn(3, H, W, generator=g, device=dev)
    g4 = torch.randn(4, H, W, generator=g, device=dev)
    g7 = torch.randn(7, H, W, generator=g, device=dev)
    leaves_s = [t.clone().requires_grad_(True) for t in (xyz, col, opa, sca, rot)]
    leaves_2 = [t.clone().requires_grad_(True) for t in (xyz, col, opa, sca[:, :2].contiguous(), rot)]
    info = {}

    def step_surfel():
        m2 = torch.zeros_like(xyz, requires_grad=True)
        img, nrm, dep, alp, radii, _ = surf(means3D=leaves_s[0], means2D=m2, colors_precomp=leaves_s[1],
                                            opacities=leaves_s[2], scales=leaves_s[3], rotations=leaves_s[4])
        ((img * gi).sum() + (torch.cat([nrm, dep], 0) * g4).sum() + (alp * gi[:1]).sum()).backward()

    def step_2d():
        m2 = torch.zeros_like(xyz, requires_grad=True)
        img, radii, allm = two(means3D=leaves_2[0], means2D=m2, colors_precomp=leaves_2[1], opacities=leaves_2[2],
                               scales=leaves_2[3], rotations=leaves_2[4])
        ((img * gi).sum() + (allm * g7).sum()).backward()
        info["visible_2dgs"] = radii  # kept on the device; counted after the loop

    times = {"surfel": [], "2dgs": []}
    for i in range(warmup + steps):
        for key, fn in (("surfel", step_surfel), ("2dgs", step_2d)):
            for t in leaves_s + leaves_2:
                t.grad = None
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= warmup:
                times[key].append(a.elapsed_time(b))
    s, t = statistics.median(times["surfel"]), statistics.median(times["2dgs"])
    return name, {"P": int(xyz.shape[0]), "W": W, "H": H, "surfel_ms": round(s, 3), "2dgs_ms": round(t, 3),
                  "ratio": round(t / s, 3), "visible_2dgs": int((info["visible_2dgs"] > 0).sum())}


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    dev = torch.device("cuda")
    torch.autograd.set_multithreading_enabled(False)
    out = {}
    k, v = measure("C2 room", room_scene(200_000, device=dev, seed=1), 640, 480, 600.0, steps, 3, dev)
    out[k] = v
    W, H = 1920, 1080
    k, v = measure("headline 1M", bench.synth_cloud(1_000_000, W, H, 1000.0, 1000.0, dev, seed=42), W, H, 1000.0,
                   steps, 2, dev)
    out[k] = v
    print(json.dumps(out))


if __name__ == "__main__":
    main()
