"""Time the mapper's semantic term (utils/mapper.py:863-866, 929-946) from the semantic decoder's output on: the
reference's torch lines in fp32 on the device (log_softmax, IDW sum, two boolean-index selections, `[::d]`, NLLLoss)
against the block (`pings_amd.semantic_losses.semantic_nll`), forward + backward, on the same inputs at the
reference's shape (B = 16,384 samples, k = 6 neighbours, S = 21 classes) with d = 1 and d = 4.

Torch and block runs alternate (`--rounds`); per run: wall time of a whole synchronised forward + backward (median of
`--iters`), device launches (torch.profiler's device events) and host waits (torch's sync-debug warnings).  Kernel
times are not measured.

    python tools/sem_time.py [--iters 20] [--rounds 3] [--out profiles/sem/sem_time.json]
"""
import argparse
import json
import statistics
import sys
import time
import warnings
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pings_amd.semantic_losses import semantic_nll  # noqa: E402

B, K, S = 16384, 6, 21


def inputs(dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    raw = torch.randn(B, K, S, generator=g, device=dev).requires_grad_(True)
    w = torch.softmax(torch.randn(B, K, generator=g, device=dev), dim=1).unsqueeze(-1)
    y = torch.randint(-1, S, (B,), generator=g, device=dev, dtype=torch.int32)     # the pool's torch.int labels
    return raw, w, y


def torch_lines(raw, w, y, d):
    sem_pred = torch.nn.functional.log_softmax(raw, dim=-1)
    sem_pred = torch.sum(sem_pred * w, dim=1)
    label_mask = y > 0
    sem_pred = sem_pred[label_mask]
    sem_label = y[label_mask].long()
    return torch.nn.NLLLoss(reduction="mean")(sem_pred[::d, :], sem_label[::d])


def block(raw, w, y, d):
    return semantic_nll(raw, w, y, decimation=d).nll


def measure(fn, raw, iters):
    def it():
        raw.grad = None
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
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            it()
            torch.cuda.synchronize()
        launches = len([e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA])
    except Exception as e:                      # profiler unavailable: report the rest
        launches = f"unavailable: {type(e).__name__}"
    return {"wall_ms_median": round(walls[len(walls) // 2], 4), "wall_ms_min": round(walls[0], 4),
            "device_ops": launches, "host_waits": waits}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda"
    raw, w, y = inputs(dev)
    res = {"B": B, "k": K, "S": S, "device": torch.cuda.get_device_name(0)}
    for d in (1, 4):
        v_t, v_b = torch_lines(raw, w, y, d).detach(), block(raw, w, y, d).detach()
        g_t = torch.autograd.grad(torch_lines(raw, w, y, d), raw)[0]
        g_b = torch.autograd.grad(block(raw, w, y, d), raw)[0]
        runs = {"torch": [], "block": []}
        for _ in range(a.rounds):               # alternate: torch, block, torch, block, ...
            runs["torch"].append(measure(lambda: torch_lines(raw, w, y, d), raw, a.iters))
            runs["block"].append(measure(lambda: block(raw, w, y, d), raw, a.iters))
        res[f"d{d}"] = {k: {"wall_ms_median_of_rounds": round(statistics.median(r["wall_ms_median"] for r in v), 4),
                            "rounds": v} for k, v in runs.items()}
        res[f"d{d}"]["value_rel_diff"] = float((v_t - v_b).abs() / v_t.abs())
        res[f"d{d}"]["grad_max_abs_diff_over_max"] = float((g_t - g_b).abs().max() / g_t.abs().max())
        print(f"d{d}", {k: v["wall_ms_median_of_rounds"] for k, v in res[f"d{d}"].items() if isinstance(v, dict)},
              flush=True)
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
