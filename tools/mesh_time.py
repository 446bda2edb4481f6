"""Time mesh finishing on the device (`pings_amd.mesh_ops`, csrc/mesh.hip): `finish_mesh` and each primitive.

The input is the concatenation of a few marching-cubes meshes of tests/test_mc.py-style fields (noise cubes side by
side, each meshed on its own, so the parts share nothing and the weld only removes what marching cubes never makes —
plus one field meshed in two halves, whose seam it closes), about 10^6 faces in all.

Host clock around synchronised calls after warm-up; per entry: wall time (median, min), host reads per call
(`_lib.sync_counts`), launches per call (counted from the kernel list in the entry's C code, see LAUNCHES) and sizes.
The comparison is a torch restatement in the same process: `torch.unique(dim=0, return_inverse=True)` for the weld
(which sorts the vertices instead of keeping their order), `index_add_` for the normals (float atomics: not
reproducible).  The cluster step has no torch restatement worth timing and is reported alone.  Kernel times come from a
separate `rocprofv3 --kernel-trace --stats` run of this script.

    python tools/mesh_time.py [--iters 10] [--warmup 3] [--fields 4] [--n 48] [--out profiles/mesh/mesh_time.json]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pings_amd import _lib, mesh_ops, mesher_ops as MO  # noqa: E402

# launches per call, library sorts and scans counted as one each (they are several kernels inside): from csrc/mesh.hip
LAUNCHES = {"weld": "3 key + 3 sort + heads + max-scan + rep + sum-scan + clear + gather + faces = 13",
            "cluster_triangles": "clear + keys + sort + union + flatten + scan + labels = 7",
            "drop_small_clusters": "7 of the clusters + keep + scan + compact = 10",
            "vertex_normals": "keys + sort + normals = 3",
            "compact_vertices": "clear + mark + scan + gather + faces = 5"}


def noise(n, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    v = torch.ones(n, n, n)
    v[2:-2, 2:-2, 2:-2] = torch.randn((n - 4,) * 3, generator=g)
    return v.to(dev)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ts = []
    _lib.sync_counts(reset=True)
    for _ in range(iters):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    reads = sum(_lib.sync_counts(reset=True).values()) / iters
    return out, {"wall_ms_median": round(1e3 * statistics.median(ts), 3), "wall_ms_min": round(1e3 * min(ts), 3),
                 "host_reads_per_call": reads}


def torch_weld(v, f):
    u, inv = torch.unique(v, dim=0, return_inverse=True)
    return u, inv[f]


def torch_normals(v, f):
    t = v[f]
    n = torch.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0], dim=1)
    s = torch.zeros_like(v)
    for c in range(3):
        s.index_add_(0, f[:, c], n)
    return torch.nn.functional.normalize(s, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fields", type=int, default=4)
    ap.add_argument("--n", type=int, default=48)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda")
    parts = []
    for k in range(a.fields):
        vol = noise(a.n, k, dev)
        shift = torch.tensor([k * a.n, 0.0, 0.0], device=dev)
        if k == 0:                                                   # one field in two halves: a seam to close
            h = a.n // 2
            v0, f0 = MO.marching_cubes(vol[:h + 1])
            v1, f1 = MO.marching_cubes(vol[h:])
            parts += [(v0, f0), (v1 + torch.tensor([float(h), 0.0, 0.0], device=dev), f1)]
        else:
            v, f = MO.marching_cubes(vol)
            parts.append((v * 0.1 + shift * 0.1, f))
    parts[0] = (parts[0][0] * 0.1, parts[0][1])
    parts[1] = (parts[1][0] * 0.1, parts[1][1])
    off, vs, fs = 0, [], []
    for v, f in parts:
        vs.append(v)
        fs.append(f + off)
        off += v.shape[0]
    verts, faces = torch.cat(vs), torch.cat(fs)
    res = {"device": torch.cuda.get_device_name(0), "parts": len(parts), "verts_in": int(verts.shape[0]),
           "faces_in": int(faces.shape[0]), "launches": LAUNCHES}
    print(json.dumps({k: res[k] for k in ("parts", "verts_in", "faces_in")}), flush=True)

    (wv, wf, _), e = timed(lambda: mesh_ops.weld(verts, faces), a.iters, a.warmup)
    res["weld"] = {**e, "verts_out": int(wv.shape[0])}
    (labels, counts), e = timed(lambda: mesh_ops.cluster_triangles(wf, wv.shape[0]), a.iters, a.warmup)
    res["cluster_triangles"] = {**e, "clusters": int(counts.shape[0]), "largest": int(counts.max())}
    min_tri = 300                                                    # the reference's default min_cluster_vertices
    kept, e = timed(lambda: mesh_ops.drop_small_clusters(wf, wv.shape[0], min_tri), a.iters, a.warmup)
    res["drop_small_clusters"] = {**e, "min_tri": min_tri, "faces_out": int(kept.shape[0])}
    _, e = timed(lambda: mesh_ops.vertex_normals(wv, wf), a.iters, a.warmup)
    res["vertex_normals"] = e
    (cv, _), e = timed(lambda: mesh_ops.compact_vertices(wv, kept), a.iters, a.warmup)
    res["compact_vertices"] = {**e, "verts_out": int(cv.shape[0])}
    m, e = timed(lambda: mesh_ops.finish_mesh(parts, min_tri=min_tri), a.iters, a.warmup)
    res["finish_mesh"] = {**e, "min_tri": min_tri, "verts_out": int(m.verts.shape[0]), "faces_out": int(m.faces.shape[0])}
    _, e = timed(lambda: torch_weld(verts, faces), a.iters, a.warmup)
    res["torch_unique_weld"] = e
    _, e = timed(lambda: torch_normals(wv, wf), a.iters, a.warmup)
    res["torch_index_add_normals"] = e
    res["torch_clusters"] = "not measured (no torch restatement worth timing)"
    for k in ("weld", "cluster_triangles", "drop_small_clusters", "vertex_normals", "compact_vertices", "finish_mesh",
              "torch_unique_weld", "torch_index_add_normals"):
        print(k, json.dumps(res[k]), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
