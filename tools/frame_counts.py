"""What the per-Gaussian passes of the raster step have to visit: python tools/frame_counts.py [m1|c2|c3] [--out FILE]
prints, for one forward + backward of the workload (default m1, the headline frame), the Gaussians that survive
culling (nvalid), the depth ranks that keep a tile behind the occlusion bound, the front depth F (1 + the last of those
ranks; null where the frame cannot gather and the library does not look for it: set PINGS_BIN=g to see it) with the
binning plan the render took by it (PINGS_BIN forces either), the ranks with a live gradient row, the
(Gaussian, chunk) pairs of the row sums and the longest loop over chunk partials one rank runs.

The chunk scan is read out of the backward blob: carve_bwd (raster_layout.hip) puts cidx[I + 2] first and pair_off[P + 1]
behind it, each field on a 256-byte boundary."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import bench
from pings_amd import _lib
from pings_amd import rasterizer as hr


def workload(which, dev):
    if which == "c2":
        from scenes import room_scene
        return room_scene(200_000, device=dev, seed=1), 640, 480, 600.0
    if which == "c3":
        from scenes import street_scene
        return street_scene(1_000_000, device=dev, seed=1), 1392, 512, 720.0
    W, H = 1920, 1080
    return bench.synth_cloud(1_000_000, W, H, 1000.0, 1000.0, dev, seed=42), W, H, 1000.0


def frame_counts(which, dev):
    cloud, W, H, fx = workload(which, dev)
    rast = bench._surfel_rast(hr, dev, W, H, fx, fx)
    prep = rast._prepared()
    L = _lib.lib()
    with torch.no_grad():
        fs, radii, contrib = hr._forward(prep, *[t.detach() for t in cloud])
        P, I = fs.P, fs.I
        plan, front = C.c_int32(0), C.c_uint32(0)
        if hasattr(L, "pings_raster_debug_bin_plan"):      # an older PINGS_HIP_LIB build always sorts
            _lib.check(L.pings_raster_debug_bin_plan(C.byref(plan), C.byref(front)), "pings_raster_debug_bin_plan")
        num_tiles = ((W + 15) // 16) * ((H + 15) // 16)
        gg = torch.Generator(device=dev).manual_seed(7)
        ups = [torch.randn(c, H, W, generator=gg, device=dev) for c in (3, 3, 1, 1)]
        f32 = dict(dtype=torch.float32, device=dev)
        scratch = torch.empty(L.pings_raster_backward_bytes(P, I), dtype=torch.uint8, device=dev)
        grads = [torch.empty(P, c, **f32) for c in (3, 3, 3, 1, 3, 4)]
        d_tau = torch.empty(6, **f32)
        st = L.pings_raster_backward(
            prep.ref(), P, I, _lib.ptr(fs.means3D), _lib.ptr(fs.colors), _lib.ptr(fs.opacities), _lib.ptr(fs.scales),
            _lib.ptr(fs.rotations), _lib.ptr(fs.geom), _lib.ptr(fs.binning), _lib.ptr(fs.image), _lib.ptr(fs.color),
            _lib.ptr(fs.normal), _lib.ptr(fs.depth), _lib.ptr(fs.alpha), _lib.ptr(ups[0]), _lib.ptr(ups[1]),
            _lib.ptr(ups[2]), _lib.ptr(ups[3]), _lib.ptr(scratch), *[_lib.ptr(g) for g in grads], _lib.ptr(d_tau),
            fs.fclass, _lib.stream_ptr(dev))
        _lib.check(st, "pings_raster_backward")
        torch.cuda.synchronize()
        pair_off_at = (4 * (I + 2) + 255) // 256 * 256
        cidx = scratch[:4 * (I + 2)].view(torch.int32)
        pair_off = scratch[pair_off_at:pair_off_at + 4 * (P + 1)].view(torch.int32).long()
        chunks = pair_off[1:] - pair_off[:-1]
        owners, _, _, _ = hr.debug_lists(fs)
        nvalid = int((radii > 0).sum())
        out = {
            "workload": which, "gaussians": P, "width": W, "height": H, "footprint_class": fs.fclass, "instances": int(I),
            "nvalid": nvalid,
            "ranks_with_kept_tiles": int(torch.unique(owners).numel()),
            # 0xFFFFFFFF: the frame cannot gather (footprint class 1, or PINGS_BIN=s) and nobody looked for its front
            "front_depth": int(front.value) if front.value != 0xFFFFFFFF else None,
            "front_tiles_per_instance": round(front.value * num_tiles / max(int(I), 1), 3) if front.value != 0xFFFFFFFF else None,
            "binning_plan": "gather" if plan.value == 1 else "sort",
            "ranks_with_live_rows": int((chunks > 0).sum()),
            "live_rows": int(cidx[I]),
            "gaussian_chunk_pairs": int(pair_off[P]),
            "longest_partial_loop": int(chunks.max()),
            "gaussians_with_contributions": int((contrib != 0).sum()),
        }
        out["survivors_without_live_rows"] = nvalid - out["ranks_with_live_rows"]
        out["dead_share_of_survivors"] = round(out["survivors_without_live_rows"] / max(nvalid, 1), 4)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("which", nargs="?", default="m1", choices=["m1", "c2", "c3"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = frame_counts(a.which, torch.device("cuda"))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
