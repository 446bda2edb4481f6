"""Mesh finishing on the HIP device: what `Mesher.recon_aabb_collections_mesh` (utils/mesher.py:480-530, :583-636) does
with Open3D after marching cubes — concatenate the chunks, `remove_duplicated_vertices`, drop the connected clusters
below `config.min_cluster_vertices` triangles, `compute_vertex_normals`, `global_transform`, write the `.ply` — without
Open3D.  Kernels: csrc/mesh.hip; rules: DESIGN §2.7b, restated in numpy by tests/mesh_ref.py.  The semantic branch
(`estimate_sem`: colours by label, free-space vertices removed) is `label_colors` / `remove_vertices`
(csrc/mesh_label.hip).

Every primitive takes and returns device tensors (verts fp32 [V, 3], faces int64 [F, 3]); a CPU tensor raises
`PingsHipError`.  Empty inputs give empty outputs with no launch.  Host reads are recorded with `_lib.note_sync`."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _abi, _lib


class Mesh(NamedTuple):
    verts: torch.Tensor                   # [V, 3] fp32
    faces: torch.Tensor                   # [F, 3] int64
    normals: Optional[torch.Tensor]       # [V, 3] fp32 or None
    colors: Optional[torch.Tensor]        # [V, C] or None


def _check(verts, faces, what):
    for t in (verts, faces):
        if t is not None and not t.is_cuda:
            raise _lib.PingsHipError(f"{what} runs on the HIP device only (got a CPU tensor); there is no CPU fallback")
    if verts is not None and (verts.dim() != 2 or verts.shape[1] != 3):
        raise ValueError(f"{what}: verts must be [V, 3], got shape {tuple(verts.shape)}")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{what}: faces must be [F, 3], got shape {tuple(faces.shape)}")
    if faces.dtype != torch.int64:
        raise ValueError(f"{what}: faces must be int64, got {faces.dtype}")
    v = None if verts is None else verts.detach().to(torch.float32).contiguous()
    return v, faces.detach().contiguous()


def _scratch(nbytes, dev, what):
    if nbytes == 0:
        raise _lib.PingsHipError(f"{what}: the mesh is too large for 32-bit indices")
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def _no_vertices(faces, what):
    if faces.shape[0]:
        raise _lib.PingsHipError(f"{what}: faces name vertices of an empty vertex array")


def _weld(verts, faces):
    """-> (verts, faces, remap, kept): kept[j] is the old index of new vertex j (its group's first occurrence)."""
    verts, faces = _check(verts, faces, "weld")
    dev, V, F = verts.device, verts.shape[0], faces.shape[0]
    if V == 0:
        _no_vertices(faces, "weld")
        z = torch.zeros(0, dtype=torch.int64, device=dev)
        return verts, faces, z, z
    L = _lib.lib()
    scratch = _scratch(L.pings_mesh_weld_scratch_bytes(V, F), dev, "weld")
    vout = torch.empty(V, 3, device=dev)
    fout = torch.empty(F, 3, dtype=torch.int64, device=dev)
    remap = torch.empty(V, dtype=torch.int64, device=dev)
    kept = torch.empty(V, dtype=torch.int64, device=dev)
    n = C.c_int64(0)
    _lib.note_sync("mesh_weld")
    _lib.check(L.pings_mesh_weld(_lib.ptr(verts), V, _lib.ptr(faces) if F else None, F, _lib.ptr(scratch), _lib.ptr(vout),
                                 _lib.ptr(fout) if F else None, _lib.ptr(remap), _lib.ptr(kept), C.byref(n),
                                 _lib.stream_ptr(dev)), "pings_mesh_weld")
    return vout[:n.value], fout, remap, kept[:n.value]


def weld(verts, faces):
    """`remove_duplicated_vertices`: vertices whose three fp32 coordinates compare equal become one (-0 == +0; a vertex
    with a non-finite coordinate equals nothing), the first occurrence is kept, kept vertices keep their order, faces
    are remapped and none is removed.  -> (verts, faces, remap [V_in] int64).  One host read."""
    v, f, remap, _ = _weld(verts, faces)
    return v, f, remap


def _clusters(faces, n_verts, read):
    dev, F = faces.device, faces.shape[0]
    L = _lib.lib()
    scratch = _scratch(L.pings_mesh_clusters_scratch_bytes(F), dev, "cluster_triangles")
    labels = torch.empty(F, dtype=torch.int64, device=dev)
    counts = torch.empty(F, dtype=torch.int64, device=dev)
    k = C.c_int64(0)
    if read:
        _lib.note_sync("mesh_clusters")
    _lib.check(L.pings_mesh_clusters(_lib.ptr(faces), F, int(n_verts), _lib.ptr(scratch), _lib.ptr(labels),
                                     _lib.ptr(counts), C.byref(k) if read else None, _lib.stream_ptr(dev)),
               "pings_mesh_clusters")
    return scratch, labels, counts, k.value


def cluster_triangles(faces, n_verts):
    """`cluster_connected_triangles`: faces that share an undirected edge (min, max) are connected, faces that share
    only a vertex are not; a cluster's id is the rank of its smallest face index.  -> (labels [F], counts [K]) int64.
    One host read (K)."""
    _, faces = _check(None, faces, "cluster_triangles")
    if faces.shape[0] == 0:
        z = torch.zeros(0, dtype=torch.int64, device=faces.device)
        return z, z
    if n_verts <= 0:
        _no_vertices(faces, "cluster_triangles")
    _, labels, counts, k = _clusters(faces, n_verts, True)
    return labels, counts[:k]


def drop_small_clusters(faces, n_verts, min_tri):
    """`filter_isolated_vertices` (mesher.py:625-636): keeps face f iff its cluster has at least `min_tri` faces, in
    order.  Vertices are untouched.  One host read (clusters and kept faces together)."""
    _, faces = _check(None, faces, "drop_small_clusters")
    F, dev = faces.shape[0], faces.device
    if F == 0:
        return faces
    if n_verts <= 0:
        _no_vertices(faces, "drop_small_clusters")
    scratch, labels, counts, _ = _clusters(faces, n_verts, False)
    L = _lib.lib()
    out = torch.empty(F, 3, dtype=torch.int64, device=dev)
    tot = (C.c_int64 * 2)(0, 0)
    _lib.note_sync("mesh_drop_small")
    _lib.check(L.pings_mesh_drop_small(_lib.ptr(faces), F, _lib.ptr(labels), _lib.ptr(counts), int(min_tri),
                                       _lib.ptr(scratch), _lib.ptr(out), tot, _lib.stream_ptr(dev)),
               "pings_mesh_drop_small")
    return out[:int(tot[1])]


def vertex_normals(verts, faces):
    """`compute_vertex_normals(normalized=True)`: per vertex the sum, in ascending face and then corner order, of the
    unnormalised (v1 - v0) x (v2 - v0) of the corners that name it, normalised; (0, 0, 1) where the sum is zero or not
    finite.  fp32, no host read, so a face that names a vertex outside [0, V) is no error here: it contributes nothing."""
    verts, faces = _check(verts, faces, "vertex_normals")
    dev, V, F = verts.device, verts.shape[0], faces.shape[0]
    out = torch.empty(V, 3, device=dev)
    if V == 0:
        return out
    L = _lib.lib()
    scratch = _scratch(L.pings_mesh_vertex_normals_scratch_bytes(V, F), dev, "vertex_normals")
    _lib.check(L.pings_mesh_vertex_normals(_lib.ptr(verts), V, _lib.ptr(faces) if F else None, F, _lib.ptr(scratch),
                                           _lib.ptr(out), _lib.stream_ptr(dev)), "pings_mesh_vertex_normals")
    return out


def compact_vertices(verts, faces, *attrs):
    """Drops the vertices no face names (the reference never does); kept vertices keep their order, per-vertex `attrs`
    ([V, ...] device tensors, None passed through) follow.  -> (verts, faces, *attrs).  One host read."""
    verts, faces = _check(verts, faces, "compact_vertices")
    dev, V, F = verts.device, verts.shape[0], faces.shape[0]
    for a in attrs:
        if a is not None and (not a.is_cuda or a.shape[0] != V):
            raise ValueError("compact_vertices: every attribute is a device tensor with one row per vertex")
    if V == 0:
        _no_vertices(faces, "compact_vertices")
        return (verts, faces, *attrs)
    L = _lib.lib()
    scratch = _scratch(L.pings_mesh_compact_vertices_scratch_bytes(V, F), dev, "compact_vertices")
    vout = torch.empty(V, 3, device=dev)
    fout = torch.empty(F, 3, dtype=torch.int64, device=dev)
    remap = torch.empty(V, dtype=torch.int64, device=dev)
    kept = torch.empty(V, dtype=torch.int64, device=dev)
    n = C.c_int64(0)
    _lib.note_sync("mesh_compact_vertices")
    _lib.check(L.pings_mesh_compact_vertices(_lib.ptr(verts), V, _lib.ptr(faces) if F else None, F, _lib.ptr(scratch),
                                             _lib.ptr(vout), _lib.ptr(fout) if F else None, _lib.ptr(remap),
                                             _lib.ptr(kept), C.byref(n), _lib.stream_ptr(dev)),
               "pings_mesh_compact_vertices")
    kept = kept[:n.value]
    return (vout[:n.value], fout, *(None if a is None else a.index_select(0, kept) for a in attrs))


def label_colors(labels, table, valid, status=None):
    """Vertex colours by label (mesher.py:402-409, csrc/mesh_label.hip): `labels` int64 [V], `table` uint8 [T, 3] and
    `valid` bool [T] on the device -> (colors [V, 3] fp32 = table[label] / 255, drop [V] bool = label <= 0, the
    reference's `non_freespace_idx`).  A label outside the table, or one whose `valid` is false, gets colour 0 and is
    counted on the device: no host read here; `remove_vertices(..., drop)` reads the count with its own and raises
    ValueError where the reference's dict lookup raises KeyError.  `status` (device int32 [1]) may be passed in to
    collect the count of several calls."""
    for t in (labels, table, valid):
        if not t.is_cuda:
            raise _lib.PingsHipError("label_colors runs on the HIP device only (got a CPU tensor); there is no CPU "
                                     "fallback")
    if labels.dim() != 1 or labels.dtype != torch.int64:
        raise ValueError(f"label_colors: labels must be int64 [V], got {labels.dtype} {tuple(labels.shape)}")
    if table.dim() != 2 or table.shape[1] != 3 or table.dtype != torch.uint8 or table.shape[0] == 0:
        raise ValueError(f"label_colors: table must be uint8 [T, 3], got {table.dtype} {tuple(table.shape)}")
    if valid.dtype != torch.bool or tuple(valid.shape) != (table.shape[0],):
        raise ValueError(f"label_colors: valid must be bool [{table.shape[0]}], got {valid.dtype} {tuple(valid.shape)}")
    dev, V = labels.device, labels.shape[0]
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    colors = torch.empty(V, 3, device=dev)
    drop = torch.empty(V, dtype=torch.bool, device=dev)
    drop._pings_bad_labels = status            # travels to the host with the counts of remove_vertices
    if V:
        _lib.check(_lib.lib().pings_mesh_label_colors(_lib.ptr(labels.contiguous()), V, _lib.ptr(table.contiguous()),
                                                      _lib.ptr(valid.contiguous()), table.shape[0], _lib.ptr(colors),
                                                      _lib.ptr(drop), _lib.ptr(status), _lib.stream_ptr(dev)),
                   "pings_mesh_label_colors")
    return colors, drop


_label_colors = label_colors        # recon_mesh has a keyword of the same name


def _bad_labels_error(n) -> ValueError:
    return ValueError(f"label_colors: {n} vertex label(s) have no entry in the colour table")


def remove_vertices(verts, faces, drop, *attrs):
    """Open3D's `remove_vertices_by_mask`: the vertices with `drop` (bool [V], device) go and every face naming one
    goes; kept vertices and kept faces keep their order, indices are remapped, per-vertex `attrs` ([V, ...] device
    tensors, None passed through) follow.  -> (verts, faces, *attrs).  One host read: both counts in one record, and
    with them the bad-label count of the `label_colors` call that made `drop`, which raises ValueError."""
    verts, faces = _check(verts, faces, "remove_vertices")
    dev, V, F = verts.device, verts.shape[0], faces.shape[0]
    if not torch.is_tensor(drop) or not drop.is_cuda or drop.dtype != torch.bool or tuple(drop.shape) != (V,):
        raise ValueError(f"remove_vertices: drop must be a device bool [{V}] tensor")
    for a in attrs:
        if a is not None and (not a.is_cuda or a.shape[0] != V):
            raise ValueError("remove_vertices: every attribute is a device tensor with one row per vertex")
    if V == 0:
        _no_vertices(faces, "remove_vertices")
        return (verts, faces, *attrs)
    bad = getattr(drop, "_pings_bad_labels", None)
    L = _lib.lib()
    scratch = _scratch(L.pings_mesh_remove_vertices_scratch_bytes(V, F), dev, "remove_vertices")
    vout = torch.empty(V, 3, device=dev)
    fout = torch.empty(F, 3, dtype=torch.int64, device=dev)
    remap = torch.empty(V, dtype=torch.int64, device=dev)
    kept = torch.empty(V, dtype=torch.int64, device=dev)
    tot = (C.c_int64 * 3)(0, 0, 0)
    _lib.note_sync("mesh_remove_vertices")
    _lib.check(L.pings_mesh_remove_vertices(_lib.ptr(verts), V, _lib.ptr(faces) if F else None, F,
                                            _lib.ptr(drop.contiguous()), _lib.ptr(bad), _lib.ptr(scratch),
                                            _lib.ptr(vout), _lib.ptr(fout) if F else None, _lib.ptr(remap),
                                            _lib.ptr(kept), tot, _lib.stream_ptr(dev)), "pings_mesh_remove_vertices")
    if tot[2]:
        raise _bad_labels_error(int(tot[2]))
    kept = kept[:int(tot[0])]
    return (vout[:int(tot[0])], fout[:int(tot[1])],
            *(None if a is None else a.index_select(0, kept) for a in attrs))


def finish_mesh(parts, min_tri=0, normals=True, colors=None, transform=None, compact=False) -> Mesh:
    """The reference's order (mesher.py:500-523): concatenate `parts` (a list of device (verts, faces) pairs) with face
    offsets, weld, drop the clusters below `min_tri` faces when `min_tri > 0`, (with `compact`, an extension, drop the
    unreferenced vertices,) vertex normals, then the optional 4x4 `transform`: vertices in fp64 and rounded once, normals
    times its 3x3 block, as Open3D's `transform` does.  `colors` [sum V, C] follows the weld by first occurrence.
    Two host reads at most, three with `compact`."""
    parts = [(v, f) for v, f in parts]
    dev = next((v.device for v, _ in parts), torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available()
               else torch.device("cpu"))
    empty = Mesh(torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.int64, device=dev),
                 torch.zeros(0, 3, device=dev) if normals else None,
                 None if colors is None else colors[:0])
    checked, off = [], 0
    for v, f in parts:
        v, f = _check(v, f, "finish_mesh")
        checked.append((v, f + off if off else f))
        off += v.shape[0]
    if colors is not None and (not colors.is_cuda or colors.shape[0] != off):
        raise ValueError("finish_mesh: colors is a device tensor with one row per input vertex")
    if off == 0 or sum(f.shape[0] for _, f in checked) == 0:
        return empty
    verts = torch.cat([v for v, _ in checked])
    faces = torch.cat([f for _, f in checked])
    verts, faces, _, kept = _weld(verts, faces)
    if colors is not None:
        colors = colors.index_select(0, kept)
    if min_tri > 0:
        faces = drop_small_clusters(faces, verts.shape[0], min_tri)
    if compact:
        verts, faces, colors = compact_vertices(verts, faces, colors)
    nrm = vertex_normals(verts, faces) if normals else None
    if transform is not None:
        T = torch.as_tensor(np.asarray(transform, dtype=np.float64).reshape(4, 4)).to(dev)
        # elementwise, left to right (no library matmul): every product and sum is one fp64 rounding, the same anywhere
        rot = lambda x: x[:, 0:1] * T[:3, 0] + x[:, 1:2] * T[:3, 1] + x[:, 2:3] * T[:3, 2]
        verts = (rot(verts.double()) + T[:3, 3]).float()
        if nrm is not None:
            nrm = rot(nrm.double()).float()
    return Mesh(verts, faces, nrm, colors)


def recon_mesh(mesher, aabbs, voxel_size, query_locally=False, estimate_color=False, mesh_normal=True,
               filter_isolated_mesh=False, mesh_min_nn=10, mesh_path=None, estimate_sem=False,
               filter_free_space_vertices=True, label_colors=None):
    """`Mesher.recon_aabb_collections_mesh` without Open3D: `mesher_ops.mesh_bbx` per box (chunks past the point cap
    are skipped), vertex colours per chunk before the weld with `estimate_color`, `finish_mesh` with
    config.min_cluster_vertices and the mesher's global_transform (skipped when it is the identity), `write_ply` when
    `mesh_path` is given.  With `estimate_sem` (mesher.py:599-603, `estimate_vertices_sem`) each chunk's vertices are
    labelled by the semantic decoder and coloured by `label_colors` = (table uint8 [T, 3], valid bool [T]) on the
    device, the vertices with a label <= 0 and their faces are removed when `filter_free_space_vertices`, and
    `estimate_color` is ignored, as the reference's `else` does.  -> Mesh, or None without boxes."""
    from . import mesher_ops as MO

    if aabbs is None:
        return None
    cfg = mesher.config
    status = None
    if estimate_sem:
        if label_colors is None:
            raise ValueError("recon_mesh: estimate_sem needs label_colors = (table uint8 [T, 3], valid bool [T])")
        if getattr(mesher, "sem_mlp", None) is None:
            raise ValueError("recon_mesh: estimate_sem needs a semantic decoder (mesher.sem_mlp)")
        table, valid = label_colors
        estimate_color = False
    parts, cols = [], []
    for bbx in aabbs:
        bmin, bmax = (bbx.get_min_bound(), bbx.get_max_bound()) if hasattr(bbx, "get_min_bound") else bbx
        chunk = MO.mesh_bbx(mesher, bmin, bmax, voxel_size, query_locally, mesh_min_nn)
        if chunk is None:
            continue
        if estimate_sem:
            v, f = chunk
            if status is None:
                status = torch.zeros(1, dtype=torch.int32, device=v.device)
            c, drop = _label_colors(MO.label_vertices(mesher, v, query_locally), table, valid, status)
            if filter_free_space_vertices:
                v, f, c = remove_vertices(v, f, drop, c)
            chunk = (v, f)
            cols.append(c)
        parts.append(chunk)
        if estimate_color:
            _, _, c, _ = MO._query_device(mesher, chunk[0], cfg.infer_bs, False, False, True, False, query_locally)
            if getattr(cfg, "color_channel", 3) == 1:
                c = (c * 2.0).repeat(1, 3)       # mesher.py estimate_vertices_color: np.repeat(color_pred * 2.0, 3, axis=1)
            cols.append(c)
    if status is not None and not filter_free_space_vertices:
        _lib.note_sync("mesh_label_status")      # no remove_vertices call carried the count to the host
        n_bad = int(status.cpu())
        if n_bad:
            raise _bad_labels_error(n_bad)
    T = np.asarray(getattr(mesher, "global_transform", np.eye(4)), dtype=np.float64)
    mesh = finish_mesh(parts, min_tri=cfg.min_cluster_vertices if filter_isolated_mesh else 0, normals=mesh_normal,
                       colors=torch.cat(cols) if cols else None,
                       transform=None if np.array_equal(T, np.eye(4)) else T)
    if mesh_path is not None:
        write_ply(mesh_path, mesh.verts, mesh.faces, mesh.normals, mesh.colors)
    return mesh


def write_ply(path, verts, faces, normals=None, colors=None) -> None:
    """Binary little-endian PLY with the properties Open3D's writer emits, so the reference's tools read it back:
    double x y z, double nx ny nz when given, uchar red green blue when given (the colour clamped to [0, 1], times 255,
    rounded), list uchar uint vertex_indices.  Host code: one copy of each tensor to the host."""
    host = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    v = host(verts).astype("<f8").reshape(-1, 3)
    f = host(faces).reshape(-1, 3)
    fields = [("x", "<f8"), ("y", "<f8"), ("z", "<f8")]
    head = ["ply", "format binary_little_endian 1.0", "comment Created by pings_amd", f"element vertex {len(v)}",
            "property double x", "property double y", "property double z"]
    if normals is not None:
        fields += [("nx", "<f8"), ("ny", "<f8"), ("nz", "<f8")]
        head += ["property double nx", "property double ny", "property double nz"]
    if colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    head += [f"element face {len(f)}", "property list uchar uint vertex_indices", "end_header"]
    rec = np.empty(len(v), dtype=fields)
    rec["x"], rec["y"], rec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if normals is not None:
        n = host(normals).astype("<f8").reshape(-1, 3)
        rec["nx"], rec["ny"], rec["nz"] = n[:, 0], n[:, 1], n[:, 2]
    if colors is not None:
        c = host(colors).astype(np.float64).reshape(len(v), -1)
        if c.shape[1] != 3:
            raise ValueError(f"write_ply: colours must be [V, 3], got {c.shape}")
        c = np.rint(np.clip(c, 0.0, 1.0) * 255.0).astype(np.uint8)
        rec["red"], rec["green"], rec["blue"] = c[:, 0], c[:, 1], c[:, 2]
    tri = np.empty(len(f), dtype=[("n", "u1"), ("i", "<u4", (3,))])
    tri["n"], tri["i"] = 3, f
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(rec.tobytes())
        fh.write(tri.tobytes())


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def read_ply(path) -> dict:
    """The inverse of `write_ply`, and a reader of what Open3D writes: `verts` float64 [V, 3], `faces` int64 [F, 3] (an
    empty [0, 3] for a file without a face element: a cloud), and `normals` / `colors` float64 [V, 3] when the vertex
    element has nx ny nz / red green blue (uchar colours are divided by 255, as Open3D reads them).  Host numpy only.
    Formats `binary_little_endian` and `ascii`; any scalar vertex property is skipped by its declared size; faces are
    `list uchar int|uint vertex_indices` (or `vertex_index`) of three indices.  Everything else (big-endian, another
    element, a list property on vertices, a non-triangle face) raises ValueError naming the line."""
    data = open(path, "rb").read()
    end = data.find(b"end_header")
    stop = data.find(b"\n", end) if end >= 0 else -1
    if not data.startswith(b"ply") or stop < 0:
        raise ValueError(f"{path}: line 1: not a PLY file (no 'ply' ... 'end_header' header)")
    lines = data[:stop].decode("ascii", errors="replace").split("\n")
    body = data[stop + 1:]
    fmt, elements = None, []                      # elements: [name, count, [(property name, numpy type)], header line]
    for ln, raw in enumerate(lines, 1):
        tok = raw.split()
        bad = lambda why: ValueError(f"{path}: line {ln}: {why}: {raw.strip()!r}")
        if not tok or tok[0] in ("ply", "comment", "obj_info", "end_header"):
            continue
        if tok[0] == "format":
            if len(tok) < 2 or tok[1] not in ("binary_little_endian", "ascii"):
                raise bad("only binary_little_endian and ascii are read")
            fmt = tok[1]
        elif tok[0] == "element":
            if len(tok) != 3 or tok[1] not in ("vertex", "face") or not tok[2].isdigit():
                raise bad("only vertex and face elements are read")
            if tok[1] in [e[0] for e in elements] or (tok[1] == "vertex" and elements):
                raise bad("vertex comes first and each element once")
            elements.append([tok[1], int(tok[2]), [], ln])
        elif tok[0] == "property":
            if not elements:
                raise bad("a property before any element")
            el = elements[-1]
            if len(tok) >= 2 and tok[1] == "list":
                if el[0] == "vertex":
                    raise bad("list properties on vertices are not read")
                if (len(tok) != 5 or tok[2] not in ("uchar", "uint8") or _PLY_TYPES.get(tok[3]) not in ("i4", "u4")
                        or tok[4] not in ("vertex_indices", "vertex_index") or el[2]):
                    raise bad("a face is one 'list uchar int|uint vertex_indices'")
                el[2].append((tok[4], _PLY_TYPES[tok[3]]))
            else:
                if len(tok) != 3 or tok[1] not in _PLY_TYPES:
                    raise bad("unknown property type")
                if el[0] == "face":
                    raise bad("a face is one 'list uchar int|uint vertex_indices'")
                el[2].append((tok[2], _PLY_TYPES[tok[1]]))
        else:
            raise bad("unknown header line")
    if fmt is None or not elements or elements[0][0] != "vertex":
        raise ValueError(f"{path}: line {len(lines)}: the header has no format line or no vertex element")
    _, V, vprops, vline = elements[0]
    names = [n for n, _ in vprops]
    if len(set(names)) != len(names) or not {"x", "y", "z"} <= set(names):
        raise ValueError(f"{path}: line {vline}: the vertex element needs x, y and z, each property once")
    F, ftype, fline = 0, "u4", None
    if len(elements) > 1:
        _, F, fprops, fline = elements[1]
        if not fprops:
            raise ValueError(f"{path}: line {fline}: the face element has no vertex_indices list")
        ftype = fprops[0][1]
    if fmt == "ascii":
        rows = [r.split() for r in body.decode("ascii", errors="replace").split("\n")]
        rows = [(len(lines) + 1 + k, r) for k, r in enumerate(rows) if r]
        if len(rows) < V + F:
            raise ValueError(f"{path}: line {len(lines) + 1}: {V + F} data lines expected, {len(rows)} found")
        for ln, r in rows[:V]:
            if len(r) != len(vprops):
                raise ValueError(f"{path}: line {ln}: {len(vprops)} vertex values expected, {len(r)} found")
        cols = np.array([r for _, r in rows[:V]], dtype=np.float64).reshape(V, len(vprops))
        vert = {n: cols[:, k] for k, n in enumerate(names)}
        for ln, r in rows[V:V + F]:
            if r[0] != "3" or len(r) != 4:
                raise ValueError(f"{path}: line {ln}: only triangles are read, got a face of {r[0]} indices")
        faces = np.array([r[1:] for _, r in rows[V:V + F]], dtype=np.int64).reshape(F, 3)
    else:
        vdt = np.dtype([(n, "<" + t) for n, t in vprops])
        fdt = np.dtype([("n", "u1"), ("i", "<" + ftype, (3,))])
        if len(body) < V * vdt.itemsize:
            raise ValueError(f"{path}: line {vline}: {V} vertices declared, the data holds fewer")
        vert = np.frombuffer(body, dtype=vdt, count=V)
        rest = body[V * vdt.itemsize:]
        counts = np.frombuffer(rest, dtype=np.uint8)[:F * fdt.itemsize:fdt.itemsize]
        if len(counts) and (counts != 3).any():       # the first face that is no triangle is where the stride breaks
            k = int(np.flatnonzero(counts != 3)[0])
            raise ValueError(f"{path}: line {fline}: only triangles are read, face {k} has {int(counts[k])} indices")
        if len(rest) < F * fdt.itemsize:
            raise ValueError(f"{path}: line {fline}: {F} faces declared, the data holds fewer")
        faces = np.frombuffer(rest, dtype=fdt, count=F)["i"].astype(np.int64).reshape(F, 3)
    col = lambda *keys: np.stack([np.asarray(vert[k], dtype=np.float64) for k in keys], 1).reshape(V, 3)
    out = {"verts": col("x", "y", "z"), "faces": faces}
    if {"nx", "ny", "nz"} <= set(names):
        out["normals"] = col("nx", "ny", "nz")
    if {"red", "green", "blue"} <= set(names):
        c = col("red", "green", "blue")
        out["colors"] = c / 255.0 if dict(vprops)["red"] == "u1" else c
    return out


# ------------------------------------------------------------------ surface sampling and box crop
class SurfaceSample(NamedTuple):
    points: torch.Tensor                  # [n, 3] fp32; rows are written only when count == n
    tri: Optional[torch.Tensor]           # [n] int32, the owning triangle, with return_tri
    count: torch.Tensor                   # device int64 [1]: n, or 0 when no triangle has area (then nothing is written)
    status: torch.Tensor                  # device int32 [1]: MESH_SAMPLE_* bits OR-ed into it


def _box_device(box, dev) -> Optional[torch.Tensor]:
    """(lo, hi) -> a device fp64 [2, 3] tensor; a device tensor is taken as it is (no read), a host pair is uploaded."""
    if box is None:
        return None
    if isinstance(box, torch.Tensor):
        if not box.is_cuda:
            raise _lib.PingsHipError("sample_surface: box as a tensor lives on the HIP device; pass a host (lo, hi) pair "
                                     "otherwise")
        if box.dtype != torch.float64 or tuple(box.shape) != (2, 3):
            raise ValueError(f"box must be a float64 [2, 3] tensor, got {box.dtype} {list(box.shape)}")
        return box.detach().contiguous()
    lo, hi = box
    b = np.stack([np.asarray(lo, dtype=np.float64).reshape(3), np.asarray(hi, dtype=np.float64).reshape(3)])
    return torch.from_numpy(b).to(dev)


def sample_status_error(status: int) -> Optional[str]:
    """The text a caller raises with once it has read a sampler status, or None.  A non-finite vertex is no error: its
    triangles own no samples, as `vertex_normals` gives them no weight."""
    if status & _abi.MESH_SAMPLE_AREA_CAP:
        return ("sample_surface: a triangle is larger than the area cap (2**62 quanta of 2**-32 m^2 shared among the "
                "faces: 256 m^2 per triangle at 4 M faces); subdivide it or scale the mesh")
    if status & _abi.MESH_SAMPLE_INDEX:
        return "sample_surface: a face names a vertex outside [0, V)"
    return None


def sample_surface(verts, faces, n, *, seed=0, box=None, return_tri=False, status=None) -> SurfaceSample:
    """`n` points on the surface, `round(cdf_t * n) - round(cdf_{t-1} * n)` of them on triangle t (the allocation of
    Open3D's `sample_points_uniformly` as far as it is known), uniform inside each triangle by a
    counter-based generator keyed on (seed, point index): bit-equal to tests/mesh_sample_ref.py and the same from run to
    run.  `box` = (lo, hi), a host pair or a device fp64 [2, 3] tensor, drops every triangle with a vertex outside the
    inclusive box before the allocation (Open3D's `crop`), with no compaction.  -> SurfaceSample(points, tri, count,
    status); `status` (device int32 [1]) may be passed in to collect the bits of several calls.  No host read: whoever
    reads `status` raises with `sample_status_error`."""
    verts, faces = _check(verts, faces, "sample_surface")
    n, seed = int(n), int(seed)
    if not 0 <= n <= 2**31 - 1:
        raise ValueError(f"sample_surface: n must lie in [0, 2**31 - 1], got {n}")
    if not -2**63 <= seed < 2**64:
        raise ValueError("sample_surface: the seed is a 64-bit integer")
    dev, V, F = verts.device, verts.shape[0], faces.shape[0]
    if max(V, F) > 2**31 - 1:
        raise _lib.PingsHipError("sample_surface: the mesh is too large for 32-bit indices")
    bx = _box_device(box, dev)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    points = torch.empty(n, 3, device=dev)
    tri = torch.empty(n, dtype=torch.int32, device=dev) if return_tri else None
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    if n == 0 or F == 0 or V == 0:
        return SurfaceSample(points, tri, count, status)
    L = _lib.lib()
    scratch = _scratch(L.pings_mesh_sample_scratch_bytes(F), dev, "sample_surface")
    seed = seed - 2**64 if seed >= 2**63 else seed          # the same 64 bits, as the signed word the ABI carries
    _lib.check(L.pings_mesh_sample(_lib.ptr(verts), V, _lib.ptr(faces), F, _lib.ptr(bx), n, seed, _lib.ptr(scratch),
                                   _lib.ptr(points), _lib.ptr(tri), _lib.ptr(count), _lib.ptr(status),
                                   _lib.stream_ptr(dev)), "pings_mesh_sample")
    return SurfaceSample(points, tri, count, status)


def crop_box(verts, faces, lo, hi):
    """Open3D's `TriangleMesh.crop(AxisAlignedBoundingBox(lo, hi))`: the vertices with lo <= v <= hi on every axis (both
    ends inclusive, compared in fp64) renumbered in order, and the triangles whose three vertices are kept, in order.
    A vertex inside the box that no kept face names stays, as in Open3D (`compact_vertices` drops those).  Torch
    operators for the masks and gathers; -> (verts, faces).  One host read (both counts).  `eval_mesh` does not use
    it: its sampler crops in place."""
    verts, faces = _check(verts, faces, "crop_box")
    dev, V = verts.device, verts.shape[0]
    if V == 0:
        _no_vertices(faces, "crop_box")
        return verts, faces
    b = _box_device((lo, hi), dev)
    v64 = verts.double()
    inside = ((v64 >= b[0]) & (v64 <= b[1])).all(1)
    named = ((faces >= 0) & (faces < V)).all(1)
    keep = inside[faces.clamp(0, V - 1)].all(1) & named
    # kept rows first and in order, by a stable sort of the mask: no read until both counts travel together
    vrows, frows = torch.argsort(~inside, stable=True), torch.argsort(~keep, stable=True)
    _lib.note_sync("mesh_crop_box")
    nv, nf = torch.stack([inside.sum(), keep.sum()]).cpu().tolist()
    vrows = vrows[:nv]
    remap = torch.full((V,), -1, dtype=torch.int64, device=dev)
    remap[vrows] = torch.arange(nv, dtype=torch.int64, device=dev)
    return verts.index_select(0, vrows), remap[faces.index_select(0, frows[:nf])]


def to_open3d(mesh: Mesh):
    """A legacy `open3d.geometry.TriangleMesh` of `mesh` (what the reference's callers expect back).  Open3D is imported
    here and nowhere else; it is not installed where this package is tested, so this function is untested."""
    import open3d as o3d

    m = o3d.geometry.TriangleMesh(o3d.utility.Vector3dVector(mesh.verts.cpu().numpy().astype(np.float64)),
                                  o3d.utility.Vector3iVector(mesh.faces.cpu().numpy().astype(np.int32)))
    if mesh.normals is not None:
        m.vertex_normals = o3d.utility.Vector3dVector(mesh.normals.cpu().numpy().astype(np.float64))
    if mesh.colors is not None:
        m.vertex_colors = o3d.utility.Vector3dVector(mesh.colors.cpu().numpy().astype(np.float64))
    return m
