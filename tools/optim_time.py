"""Time one optimiser step of the mapper's parameter groups: stock `torch.optim.AdamW` (default foreach), stock
`AdamW(fused=True)` and `pings_amd.optim.FusedAdamW`, in one process and in alternating rounds.

Two layouts, built as `setup_optimizer` builds them (utils/tools.py:142-365; one group per decoder, per feature table
and six per camera; betas (0.9, 0.99), eps 1e-15):

* joint  the joint iteration: the SDF, colour and five spawn decoders at the shipped widths (four tensors each), ten
         cameras of which one has gradients, feature tables of 1 M x 32 and 1 M x 16;
* sdf    the SDF loop: the two tables and the SDF decoder.

Per layout and variant: wall time per `step()` with a synchronise on both sides (median over --iters), host time of
`step()` alone (the call returns before the device finishes).  Kernel launches per step and their summed time come from
a torch.profiler pass in a process of its own (`--pass profile`; the default run starts it), because tracing slows
the host.  For the 1 M x 32 table on its own the kernel time is set against the 28 bytes an AdamW step moves per
element (p, g, m, v read; p, m, v written) and the 8 TB/s HBM peak.

    python tools/optim_time.py [--iters 50] [--rounds 3] [--out profiles/optim/optim_time.json]
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pings_amd.optim import FusedAdamW  # noqa: E402

HBM_PEAK = 8.0e12
BYTES_PER_ELEMENT = 28
VARIANTS = ("foreach", "torch_fused", "pings_fused")
DECODERS = {"sdf": (32, 64, 1), "color": (19, 64, 3), "gs_xyz": (32, 128, 24), "gs_scale": (32, 128, 24),
            "gs_rot": (32, 128, 32), "gs_alpha": (32, 128, 8), "gs_color": (19, 128, 24)}
CAMERA = {"exposure_a": (1,), "exposure_b": (1,), "exposure_mat": (3, 3), "exposure_offset": (3, 1), "dr": (3,),
          "dt": (3,)}


def layout(name, dev, rows=1_000_000, seed=0):
    """(groups, live parameters) of a layout; every variant gets its own copy from the same seed."""
    g = torch.Generator().manual_seed(seed)

    def par(*shape):
        return torch.nn.Parameter((0.1 * torch.randn(shape, generator=g)).to(dev))

    groups, live = [], []

    def group(n, ps, has_grad=True, **kw):
        groups.append({"params": ps, "name": n, **kw})
        if has_grad:
            live.extend(ps)

    decs = DECODERS if name == "joint" else {"sdf": DECODERS["sdf"]} if name == "sdf" else {}
    for n, (fin, hid, out) in decs.items():
        group(f"{n}_mlp_param", [par(hid, fin), par(hid), par(out, hid), par(out)], lr=0.01, weight_decay=0.0)
    if name == "joint":
        for cam in range(10):
            for n, shape in CAMERA.items():
                group(f"cam_{cam}_{n}", [par(*shape)], has_grad=cam == 0, lr=0.001)
    tables = {"joint": (32, 16), "sdf": (32, 16), "table": (32,)}[name]
    for width in tables:
        group(f"neural_point_features_{width}", [par(rows + 1 if name != "table" else rows, width)], lr=0.01,
              weight_decay=0.0)
    for p in live:
        p.grad = (torch.randn(p.shape, generator=g) * 1e-2).to(dev)
    return groups, live


def optimiser(variant, groups):
    kw = dict(betas=(0.9, 0.99), eps=1e-15)
    if variant == "foreach":
        return torch.optim.AdamW(groups, **kw)
    if variant == "torch_fused":
        return torch.optim.AdamW(groups, fused=True, **kw)
    return FusedAdamW(groups, **kw)


def time_steps(opt, iters):
    for _ in range(5):
        opt.step()
    torch.cuda.synchronize()
    wall, host = [], []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.step()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        wall.append((t2 - t0) * 1e3)
        host.append((t1 - t0) * 1e3)
    return {"wall_ms_median": round(statistics.median(wall), 4), "wall_ms_min": round(min(wall), 4),
            "host_ms_median": round(statistics.median(host), 4)}


def profile_step(opt, steps=5):
    from torch.profiler import ProfilerActivity, profile

    for _ in range(5):
        opt.step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            opt.step()
        torch.cuda.synchronize()
    # the device-side copy of the `Optimizer.step#...` annotation range is no kernel
    evs = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
           and not e.name.startswith("Optimizer.step#")]
    return {"launches_per_step": len(evs) / steps,
            "kernel_ms_per_step": round(sum(e.device_time for e in evs) / 1e3 / steps, 5),
            "kernels": sorted({e.name for e in evs})[:8]}


def run(mode, iters, rounds, rows):
    dev = "cuda"
    res = {}
    for name in ("joint", "sdf", "table"):
        opts = {}
        for v in VARIANTS:
            groups, live = layout(name, dev, rows)
            opts[v] = (optimiser(v, groups), live)      # `live` keeps the gradients alive
        elements = sum(p.numel() for p in opts["foreach"][1])
        entry = {"live_tensors": len(opts["foreach"][1]), "elements": elements}
        if mode == "time":
            per = {v: [] for v in VARIANTS}
            for _ in range(rounds):                     # alternate: foreach, torch_fused, pings_fused, foreach, ...
                for v in VARIANTS:
                    per[v].append(time_steps(opts[v][0], iters))
            entry["rounds"] = per
            entry["pings_below_both_in_every_round"] = all(
                per["pings_fused"][r]["wall_ms_median"] < min(per["foreach"][r]["wall_ms_median"],
                                                               per["torch_fused"][r]["wall_ms_median"])
                for r in range(rounds))
        else:
            per = {v: [profile_step(opts[v][0]) for _ in range(rounds)] for v in VARIANTS}
            for v in VARIANTS:
                for r in per[v]:
                    s = r["kernel_ms_per_step"] * 1e-3
                    r["bytes_per_s"] = round(BYTES_PER_ELEMENT * elements / s) if s else None
                    r["hbm_fraction"] = round(BYTES_PER_ELEMENT * elements / s / HBM_PEAK, 4) if s else None
            entry["profile_rounds"] = per
            entry["pings_last_launches"] = opts["pings_fused"][0].last_launches
        res[name] = entry
        print(name, json.dumps(entry), flush=True)
        del opts
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--pass", dest="mode", choices=("all", "time", "profile"), default="all")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_time.py measures on a HIP device; none is available")
    if a.mode == "profile":
        res = run("profile", a.iters, a.rounds, a.rows)
        print("PROFILE_JSON " + json.dumps(res))
        return
    res = {"device": torch.cuda.get_device_name(0), "rows": a.rows, "iters": a.iters,
           "bytes_per_element": BYTES_PER_ELEMENT, "hbm_peak_bytes_per_s": HBM_PEAK,
           "time": run("time", a.iters, a.rounds, a.rows)}
    if a.mode == "all":
        torch.cuda.synchronize()
        r = subprocess.run([sys.executable, __file__, "--pass", "profile", "--rounds", str(a.rounds), "--rows",
                            str(a.rows)], capture_output=True, text=True, timeout=600)
        line = [x for x in r.stdout.splitlines() if x.startswith("PROFILE_JSON ")]
        res["profile"] = json.loads(line[0][len("PROFILE_JSON "):]) if line else \
            {"error": (r.stderr or r.stdout)[-2000:]}
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
