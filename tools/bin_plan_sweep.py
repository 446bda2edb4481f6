"""Where the two binning plans of pings_raster_render cost the same: python tools/bin_plan_sweep.py [--out FILE]
times one forward + backward step of the headline cloud with its scale range narrowed step by step (smaller footprints:
tiles saturate later, the front depth F grows and every front rank keeps fewer tiles, so F * tiles / instances rises)
under PINGS_BIN=s and PINGS_BIN=g.  The knob is read on every call, so one process alternates the two plans on the
same frame, `rounds` times each; per frame it prints F, the instance count, the ratio the default rule compares with
GATHER_COST (csrc/raster_common.hpp), the plan PINGS_BIN=g really took (it sorts where its tables do not fit) and the
median step time of either plan."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import bench
from pings_amd import _lib
from pings_amd import rasterizer as hr


def frame(dev, W, H, fx, smax, rounds, steps):
    means, col, op, scales, rot = bench.synth_cloud(1_000_000, W, H, fx, fx, dev, seed=42)
    # the same draws, mapped from log-uniform [0.02, 0.5] m onto [0.02, smax]
    u = (torch.log(scales[:, :2]) - math.log(0.02)) / (math.log(0.5) - math.log(0.02))
    scales[:, :2] = torch.exp(math.log(0.02) + (math.log(smax) - math.log(0.02)) * u)
    rast = bench._surfel_rast(hr, dev, W, H, fx, fx)
    params = [t.requires_grad_(True) for t in (means, col, op, scales.contiguous(), rot)]
    theta = torch.zeros(3, device=dev, requires_grad=True)
    rho = torch.zeros(3, device=dev, requires_grad=True)
    gg = torch.Generator(device=dev).manual_seed(7)
    ups = [torch.randn(c, H, W, generator=gg, device=dev) for c in (3, 3, 1, 1)]

    def step():
        for p_ in params + [theta, rho]:
            p_.grad = None
        out = rast(means3D=params[0], means2D=torch.zeros_like(params[0]), colors_precomp=params[1], opacities=params[2],
                   scales=params[3], rotations=params[4], theta=theta, rho=rho)
        torch.autograd.backward(list(out[:4]), ups)

    res = {"scale_max_m": smax}
    ms = {"s": [], "g": []}
    for r in range(rounds):
        for knob in ("s", "g"):
            os.environ["PINGS_BIN"] = knob
            ms[knob].append(bench._timeit(step, steps, 3) * 1e3)
            if r == 0:
                with torch.no_grad():
                    fs, _, _ = hr._forward(rast._prepared(), *[p_.detach() for p_ in params])
                plan, front = C.c_int32(0), C.c_uint32(0)
                _lib.check(_lib.lib().pings_raster_debug_bin_plan(C.byref(plan), C.byref(front)), "pings_raster_debug_bin_plan")
                nt = ((W + 15) // 16) * ((H + 15) // 16)
                if knob == "g":     # under PINGS_BIN=s nobody looks for the front depth
                    res.update(instances=int(fs.I), front_depth=int(front.value), footprint_class=int(fs.fclass),
                               front_tiles_per_instance=round(front.value * nt / max(int(fs.I), 1), 2))
                res["plan_taken_" + knob] = "gather" if plan.value == 1 else "sort"
    os.environ.pop("PINGS_BIN", None)
    for knob in ("s", "g"):
        res["ms_" + knob] = [round(v, 4) for v in ms[knob]]
        res["ms_median_" + knob] = round(statistics.median(ms[knob]), 4)
    res["gather_minus_sort_us"] = round((res["ms_median_g"] - res["ms_median_s"]) * 1e3, 1)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", default="0.5,0.45,0.4,0.35,0.32,0.3,0.28,0.25,0.13")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    torch.autograd.set_multithreading_enabled(False)
    W, H, fx = 1920, 1080, 1000.0
    frames = []
    for smax in [float(v) for v in a.scales.split(",")]:
        frames.append(frame(dev, W, H, fx, smax, a.rounds, a.steps))
        print(json.dumps(frames[-1]), flush=True)
    out = {"what": "headline cloud, scales log-uniform [0.02, scale_max_m]; one process, PINGS_BIN=s and =g alternating, "
                   f"{a.rounds} rounds of {a.steps} steps each, ms per forward + backward step",
           "width": W, "height": H, "gaussians": 1_000_000, "frames": frames}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
