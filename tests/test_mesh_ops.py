"""Mesh finishing on the device (pings_amd/mesh_ops.py, csrc/mesh.hip) against its numpy restatement
(tests/mesh_ref.py).  Integers and copied floats compare with `torch.equal`; the normals against fp64 within
max(8 delta, 1e-6), delta being the deviation of an fp32 numpy evaluation of the same formula in the same order from the
fp64 one on the same input (measured: 1.2e-7 on the sphere, 2.0e-7 on the noise field, and the device's error equal to
it; the factor covers fma contraction and the square root and divisions, the floor inputs where delta is 0)."""
import functools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import abi_header as hdr
import mc_ref
import mesh_ref
from pings_amd import _abi
from test_mc import noise, sphere
from test_mesh_ref import concat, strip, two_halves

MESH_SYMBOLS = [p + s for p in ("pings_mesh_weld", "pings_mesh_clusters", "pings_mesh_drop_small",
                                "pings_mesh_vertex_normals", "pings_mesh_compact_vertices") for s in ("", "_scratch_bytes")]


# ---------------------------------------------------------------- CPU: the ABI and the PLY writer
def test_abi_declares_mesh_finishing():
    protos = hdr.prototypes()
    for name in MESH_SYMBOLS:
        assert name in protos and name in _abi.SIGNATURES
    assert hdr.expected_abi() == _abi.ABI_VERSION == 11              # additions only


def read_ply(path):
    """Header-driven reader of the binary little-endian PLY subset `write_ply` emits."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    types = {"double": "<f8", "uchar": "u1", "uint": "<u4"}
    counts, props, cur = {}, {}, None
    for ln in lines[2:]:
        w = ln.split()
        if w[0] == "element":
            cur = w[1]
            counts[cur], props[cur] = int(w[2]), []
        elif w[0] == "property":
            props[cur].append(tuple(w[1:]))
    vdt = np.dtype([(name, types[t]) for t, name in props["vertex"]])
    v = np.frombuffer(raw, vdt, counts["vertex"], end)
    assert props["face"] == [("list", "uchar", "uint", "vertex_indices")]
    fdt = np.dtype([("n", "u1"), ("i", "<u4", (3,))])
    f = np.frombuffer(raw, fdt, counts["face"], end + v.nbytes)
    assert end + v.nbytes + f.nbytes == len(raw) and np.all(f["n"] == 3)
    return lines, v, f["i"]


@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("with_colors", [False, True])
def test_write_ply_round_trip(tmp_path, with_normals, with_colors):
    from pings_amd import mesh_ops

    rng = np.random.default_rng(5)
    v = torch.from_numpy(rng.standard_normal((7, 3)).astype(np.float32) * 100)
    f = torch.from_numpy(rng.integers(0, 7, (5, 3)))
    n = torch.from_numpy(rng.standard_normal((7, 3)).astype(np.float32)) if with_normals else None
    c = torch.from_numpy(rng.uniform(-0.2, 1.2, (7, 3)).astype(np.float32)) if with_colors else None
    if with_colors:
        c[0] = torch.tensor([0.5, 0.25, 0.999])
    path = tmp_path / "m.ply"
    mesh_ops.write_ply(str(path), v, f, n, c)
    lines, rv, rf = read_ply(path)
    assert any(l.startswith("comment") and "pings_amd" in l for l in lines)
    assert not any("open3d" in l.lower() for l in lines)
    want = ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else []) + (["red", "green", "blue"] if with_colors else [])
    assert list(rv.dtype.names) == want
    assert all(rv.dtype[k] == np.dtype("<f8") for k in want if k not in ("red", "green", "blue"))
    assert len(rv) == 7 and rf.shape == (5, 3) and rf.dtype == np.dtype("<u4")
    assert np.array_equal(np.stack([rv["x"], rv["y"], rv["z"]], 1), v.numpy().astype(np.float64))
    assert np.array_equal(rf, f.numpy())
    if with_normals:
        assert np.array_equal(np.stack([rv["nx"], rv["ny"], rv["nz"]], 1), n.numpy().astype(np.float64))
    if with_colors:
        got = np.stack([rv["red"], rv["green"], rv["blue"]], 1)
        assert got.dtype == np.uint8
        assert np.array_equal(got, np.rint(np.clip(c.numpy().astype(np.float64), 0, 1) * 255).astype(np.uint8))
        assert got[0].tolist() == [128, 64, 255]


def test_mesh_ops_reject_host_tensors():
    from pings_amd import _lib, mesh_ops

    v, f = torch.rand(4, 3), torch.tensor([[0, 1, 2]])
    for call in (lambda: mesh_ops.weld(v, f), lambda: mesh_ops.cluster_triangles(f, 4),
                 lambda: mesh_ops.drop_small_clusters(f, 4, 1), lambda: mesh_ops.vertex_normals(v, f),
                 lambda: mesh_ops.compact_vertices(v, f), lambda: mesh_ops.finish_mesh([(v, f)])):
        with pytest.raises(_lib.PingsHipError, match="no CPU fallback"):
            call()


def test_install_binds_the_finishing_methods_only_on_request():
    from pings_amd import mesher_ops as MO

    def original(self, *a, **k):
        return "original"

    plain, fin = NS(Mesher=type("Mesher", (), {"recon_aabb_collections_mesh": original})), \
        NS(Mesher=type("Mesher", (), {"recon_aabb_collections_mesh": original}))
    MO.install(plain)
    MO.install(fin, finish=True)
    MO.install(fin, finish=True)                                     # twice: the saved original stays the original
    assert plain.Mesher.recon_aabb_collections_mesh is original and not hasattr(plain.Mesher, "recon_mesh")
    assert fin.Mesher.recon_aabb_collections_mesh is not original and fin.Mesher.recon_mesh is MO.recon_mesh
    assert fin.Mesher().recon_aabb_collections_mesh([], 0.1, estimate_sem=True) == "original"
    assert fin.Mesher().recon_aabb_collections_mesh(None, 0.1) is None


# ---------------------------------------------------------------- shared inputs and references (computed once, read only)
@functools.lru_cache(maxsize=None)
def halves(name):
    vol = sphere() if name == "sphere" else noise(20)
    v, f = concat(two_halves(vol))
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


@functools.lru_cache(maxsize=None)
def welded(name):
    out = mesh_ref.weld(*halves(name))
    for a in out:
        a.setflags(write=False)
    return out


def strip_mesh(n=5000):
    i = np.arange(n + 2)
    v = np.stack([i // 2, i % 2, np.sin(i * 0.37)], axis=1).astype(np.float32)
    f = strip(n)
    f[1::2] = f[1::2][:, [0, 2, 1]]                                   # one orientation along the strip
    return v, f


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                     # a copy: the shared references are read-only


def same(t, a):
    return torch.equal(t.cpu(), torch.from_numpy(np.ascontiguousarray(a)))


# ---------------------------------------------------------------- weld
def check_weld(v, f):
    from pings_amd import mesh_ops

    gv, gf, gr = mesh_ops.weld(dev(v), dev(f))
    rv, rf, rr = mesh_ref.weld(v, f)
    assert gv.dtype == torch.float32 and gf.dtype == torch.int64 and gr.dtype == torch.int64
    assert gv.cpu().numpy().tobytes() == rv.tobytes()               # bits: a kept -0 or NaN stays what it was
    assert same(gf, rf) and same(gr, rr)


@pytest.mark.gpu
@pytest.mark.parametrize("V", [1, 255, 256, 257, 4097])
def test_gpu_weld_random_groups(V):
    rng = np.random.default_rng(V)
    v = rng.choice(np.array([-1.5, -0.0, 0.0, 0.25, 1.0, 3.0, 1e30], np.float32), (V, 3))
    f = rng.integers(0, V, (max(V // 2, 1), 3))
    check_weld(v, f)


@pytest.mark.gpu
def test_gpu_weld_rules():
    nan, inf = np.float32("nan"), np.float32("inf")
    f = np.array([[0, 1, 2]], np.int64)
    check_weld(np.full((300, 3), 0.7, np.float32), np.array([[0, 150, 299], [1, 2, 3]], np.int64))   # all identical
    check_weld(np.array([[1, 2, 3], [1.0000001, 2, 3], [1, 2.0000002, 3], [1, 2, 3.0000002], [1, 2, 3]], np.float32),
               np.array([[0, 1, 4], [2, 3, 4]], np.int64))                                           # x, y or z only
    check_weld(np.array([[-0.0, 0.0, 5], [0.0, -0.0, 5], [0.0, 0.0, 5]], np.float32), f)
    check_weld(np.array([[nan, 1, 2], [nan, 1, 2], [0, 1, 2], [0, 1, 2], [inf, 0, 0], [inf, 0, 0], [0, -inf, 0]],
                        np.float32), np.array([[0, 1, 2], [3, 4, 5]], np.int64))
    check_weld(np.array([[1, 1, 1], [2, 2, 2]], np.float32), np.zeros((0, 3), np.int64))             # no faces
    # the last vertex of one chunk is the first of the next
    a = np.arange(257 * 3, dtype=np.float32).reshape(257, 3)
    b = np.concatenate([a[-1:], a[:40] + 0.5])
    v, ff = concat([(a, np.array([[0, 1, 256]], np.int64)), (b, np.array([[0, 1, 2]], np.int64))])
    check_weld(v, ff)
    assert mesh_ref.weld(v, ff)[2][257] == 256


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sphere", "noise"])
def test_gpu_weld_two_halves(name):
    check_weld(*halves(name))
    assert welded(name)[0].shape[0] == {"sphere": 1296, "noise": 6516}[name]


# ---------------------------------------------------------------- clusters
def check_clusters(f, n_verts=None):
    from pings_amd import mesh_ops

    n_verts = int(f.max()) + 1 if n_verts is None else n_verts
    gl, gc = mesh_ops.cluster_triangles(dev(f), n_verts)
    rl, rc = mesh_ref.cluster_triangles(f)
    assert gl.dtype == torch.int64 and gc.dtype == torch.int64
    assert same(gl, rl) and same(gc, rc)
    return rl, rc


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["natural", "reversed", "shuffled"])
def test_gpu_clusters_strip(order):
    f = strip(5000)
    f = {"natural": f, "reversed": f[::-1].copy(), "shuffled": f[np.random.default_rng(1).permutation(len(f))]}[order]
    _, rc = check_clusters(f)
    assert rc.tolist() == [5000]


@pytest.mark.gpu
def test_gpu_clusters_small_cases():
    check_clusters(np.array([[0, 1, 2]], np.int64))
    _, rc = check_clusters(np.arange(9000, dtype=np.int64).reshape(3000, 3))
    assert len(rc) == 3000
    _, rc = check_clusters(np.array([[0, 1, 2], [0, 2, 3], [0, 4, 5], [0, 5, 6]], np.int64))
    assert rc.tolist() == [2, 2]
    _, rc = check_clusters(np.array([[0, 1, k] for k in range(2, 7)], np.int64))
    assert rc.tolist() == [5]
    check_clusters(np.array([[0, 1, 2], [0, 1, 2], [3, 3, 4], [4, 5, 5], [6, 6, 7], [6, 7, 8], [2, 1, 0]], np.int64))
    # clusters whose smallest faces come in another order than their vertices
    check_clusters(np.array([[6, 7, 8], [0, 1, 2], [7, 6, 9], [3, 4, 5], [1, 0, 10], [4, 3, 11]], np.int64))


@pytest.mark.gpu
def test_gpu_clusters_and_drop_small_on_the_noise_mesh():
    from pings_amd import mesh_ops

    v, f, _ = welded("noise")
    rl, rc = check_clusters(f, len(v))
    assert len(rc) > 10 and len(set(rc.tolist())) > 3               # many clusters of mixed size
    size = int(np.sort(rc)[len(rc) // 2])
    d = dev(f)
    for min_tri in (0, 1, size, size + 1, int(rc.max()), int(rc.max()) + 1):
        got = mesh_ops.drop_small_clusters(d, len(v), min_tri)
        want = mesh_ref.drop_small_clusters(f, min_tri)
        assert same(got, want), min_tri
    assert (rc[rl] >= size).sum() > (rc[rl] >= size + 1).sum()      # the cluster of that size: kept, then dropped
    assert mesh_ops.drop_small_clusters(d, len(v), int(rc.max()) + 1).shape == (0, 3)
    assert same(mesh_ops.drop_small_clusters(d, len(v), 0), f)


# ---------------------------------------------------------------- normals
def world(v):
    return (np.float32(0.1) * v + np.float32(137.5)).astype(np.float32)


def check_normals(v, f, cancel=()):
    from pings_amd import mesh_ops

    want = mesh_ref.vertex_normals(v, f)
    delta = np.abs(mesh_ref.vertex_normals(v, f, np.float32).astype(np.float64) - want).max()
    # the condition of the sums, on the reference values: every referenced vertex outside the exact-cancel case
    fn = mesh_ref.face_normals(v, f)
    mass = np.zeros(len(v))
    np.add.at(mass, f.reshape(-1), np.repeat(np.linalg.norm(fn, axis=1), 3))
    total = np.linalg.norm(mesh_ref.normal_sums(v, f), axis=1)
    ref = np.zeros(len(v), bool)
    ref[f.reshape(-1)] = True
    ref[list(cancel)] = False
    cond = (mass[ref] / total[ref]).max() if ref.any() else 0.0
    got = mesh_ops.vertex_normals(dev(v), dev(f))
    assert got.dtype == torch.float32 and got.shape == (len(v), 3)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
    print(f"normals: delta {delta:.3g} err {err:.3g} condition {cond:.4g}")
    assert cond <= 50
    assert err <= max(8 * delta, 1e-6)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sphere", "noise", "strip"])
def test_gpu_vertex_normals(name):
    if name == "strip":
        v, f = strip_mesh()
    else:
        v, f, _ = welded(name)
    check_normals(world(v), f)


@pytest.mark.gpu
def test_gpu_vertex_normals_fallback_and_order():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [0, 0, 1]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 1], [4, 4, 1]], np.int64)        # 0, 1, 2 cancel exactly, 3 is unreferenced
    got = check_normals(v, f, cancel=(0, 1, 2, 4))
    assert got.cpu().tolist() == [[0, 0, 1]] * 5
    got = check_normals(v, np.array([[0, 2, 1]], np.int64))
    assert got.cpu().tolist() == [[0, 0, -1]] * 3 + [[0, 0, 1]] * 2
    # a vertex named by two corners of a face counts twice; no faces at all
    check_normals(v, np.array([[0, 1, 2], [1, 1, 4], [0, 1, 4]], np.int64))
    from pings_amd import mesh_ops

    assert mesh_ops.vertex_normals(dev(v), dev(np.zeros((0, 3), np.int64))).cpu().tolist() == [[0, 0, 1]] * 5


# ---------------------------------------------------------------- compact_vertices
@pytest.mark.gpu
def test_gpu_compact_vertices_after_drop_small():
    from pings_amd import mesh_ops

    v, f, _ = welded("noise")
    rc = mesh_ref.cluster_triangles(f)[1]
    kept = mesh_ref.drop_small_clusters(f, int(rc.max()))
    attr = np.arange(len(v) * 2, dtype=np.float32).reshape(-1, 2)
    gv, gf, ga, gnone = mesh_ops.compact_vertices(dev(v), dev(kept), dev(attr), None)
    rv, rf, remap = mesh_ref.compact_vertices(v, kept)
    assert 0 < len(rv) < len(v) and gnone is None
    assert same(gv, rv) and same(gf, rf) and same(ga, attr[remap >= 0])
    assert len(torch.unique(gf)) == gv.shape[0]                       # no unreferenced vertex is left
    assert torch.equal(gv[gf], dev(v)[dev(kept)])                     # the same triangles
    gv, gf = mesh_ops.compact_vertices(dev(v), dev(np.zeros((0, 3), np.int64)))
    assert gv.shape == (0, 3) and gf.shape == (0, 3)


# ---------------------------------------------------------------- finish_mesh
def ref_finish(parts, min_tri, colors, T, compact):
    v, f = concat(parts)
    wv, wf, remap = mesh_ref.weld(v, f)
    first = np.unique(remap, return_index=True)[1]
    col = None if colors is None else colors[first]
    if min_tri > 0:
        wf = mesh_ref.drop_small_clusters(wf, min_tri)
    if compact:
        wv, wf, cm = mesh_ref.compact_vertices(wv, wf)
        col = None if col is None else col[cm >= 0]
    n64 = mesh_ref.vertex_normals(wv, wf)
    n32 = mesh_ref.vertex_normals(wv, wf, np.float32)
    if T is None:
        return wv, wf, n64, n32.astype(np.float64), col
    tv, tn64 = mesh_ref.transform(wv, n64, T)
    return tv, wf, tn64.astype(np.float64), mesh_ref.transform(wv, n32, T)[1].astype(np.float64), col


def three_parts():
    v, f = mc_ref.marching_cubes(noise(20))
    far = mc_ref.marching_cubes(sphere(12, 3.3))
    (a, b) = two_halves(noise(20))
    return [a, b, (far[0] + np.float32(40), far[1])], len(v)


@pytest.mark.gpu
@pytest.mark.parametrize("n_parts,compact", [(2, False), (3, False), (3, True)])
def test_gpu_finish_mesh_equals_the_composed_steps(n_parts, compact):
    from pings_amd import _lib, mesh_ops

    parts, _ = three_parts()
    parts = parts[:n_parts]
    nv = sum(len(v) for v, _ in parts)
    colors = np.random.default_rng(2).uniform(0, 1, (nv, 3)).astype(np.float32)
    c, s = np.cos(0.3), np.sin(0.3)
    T = np.array([[c, -s, 0, 10.5], [s, c, 0, -3.25], [0, 0, 1, 100.0], [0, 0, 0, 1]])
    min_tri = 40
    dparts = [(dev(v), dev(f)) for v, f in parts]
    torch.cuda.synchronize()
    _lib.sync_counts(reset=True)
    m = mesh_ops.finish_mesh(dparts, min_tri=min_tri, colors=dev(colors), transform=T, compact=compact)
    reads = sum(_lib.sync_counts(reset=True).values())
    assert reads <= (3 if compact else 2), reads
    rv, rf, rn64, rn32, rcol = ref_finish(parts, min_tri, colors, T, compact)
    assert 0 < len(rf) < sum(len(f) for _, f in parts)
    assert same(m.verts, rv) and same(m.faces, rf) and same(m.colors, rcol)
    delta = np.abs(rn32 - rn64).max()
    assert np.abs(m.normals.cpu().numpy().astype(np.float64) - rn64).max() <= max(8 * delta, 1e-6)
    again = mesh_ops.finish_mesh(dparts, min_tri=min_tri, colors=dev(colors), transform=T, compact=compact)
    for a, b in zip(m, again):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()   # bitwise, every output
    plain = mesh_ops.finish_mesh(dparts, normals=False)
    assert plain.normals is None and plain.colors is None
    assert same(plain.verts, mesh_ref.weld(*concat(parts))[0]) and same(plain.faces, mesh_ref.weld(*concat(parts))[1])


@pytest.mark.gpu
def test_gpu_finish_mesh_of_nothing():
    from pings_amd import _lib, mesh_ops

    _lib.sync_counts(reset=True)
    z = torch.zeros(0, 3, device="cuda"), torch.zeros(0, 3, dtype=torch.int64, device="cuda")
    some = torch.rand(5, 3, device="cuda"), z[1]
    for parts in ([], [z], [z, z], [some, z]):
        m = mesh_ops.finish_mesh(parts, min_tri=3)
        assert m.verts.shape == (0, 3) and m.faces.shape == (0, 3) and m.normals.shape == (0, 3) and m.colors is None
        assert m.faces.dtype == torch.int64 and m.verts.is_cuda
    assert sum(_lib.sync_counts(reset=True).values()) == 0
    l, c = mesh_ops.cluster_triangles(z[1], 0)
    assert l.shape == (0,) and c.shape == (0,)
    assert mesh_ops.drop_small_clusters(z[1], 5, 1).shape == (0, 3)
    v, f, r = mesh_ops.weld(*z)
    assert v.shape == (0, 3) and f.shape == (0, 3) and r.shape == (0,)


# ---------------------------------------------------------------- recon_mesh
@pytest.mark.gpu
def test_gpu_recon_mesh_equals_finish_mesh_over_the_chunks(golden_dir, tmp_path):
    from pings_amd import mesh_ops, mesher_ops as MO
    from test_sdf import _Dec, _gpu_map, load

    name = "gs_f32"
    st = load(golden_dir, name)
    z = np.load(golden_dir / "mesher_grid.npz")
    T = np.eye(4)
    T[:3, 3] = (1.0, -2.0, 0.5)
    fake = NS(neural_points=_gpu_map(st), sdf_mlp=_Dec(st), sem_mlp=None, color_mlp=None, global_transform=T,
              config=NS(weighted_first=bool(st["weighted_first"]), color_channel=3, pad_voxel=1, skip_top_voxel=1,
                        infer_bs=1000, mc_mask_on=True, min_cluster_vertices=5))
    vs = float(z[f"{name}_voxel"])
    lo, hi = np.asarray(z[f"{name}_min"], np.float64), np.asarray(z[f"{name}_max"], np.float64)
    mid = lo[0] + vs * np.ceil((hi[0] - lo[0]) / vs / 2)
    boxes = [(lo, np.array([mid, hi[1], hi[2]])), (np.array([mid, lo[1], lo[2]]), hi)]      # two abutting boxes
    path = tmp_path / "recon.ply"
    m = mesh_ops.recon_mesh(fake, boxes, vs, filter_isolated_mesh=True, mesh_min_nn=4, mesh_path=str(path))
    chunks = [MO.mesh_bbx(fake, a, b, vs, mesh_min_nn=4) for a, b in boxes]
    assert all(c[1].shape[0] > 0 for c in chunks)
    want = mesh_ops.finish_mesh(chunks, min_tri=5, transform=T)
    assert m.faces.shape[0] > 0 and m.colors is None
    for a, b in zip(m[:3], want[:3]):
        assert torch.equal(a, b)
    _, rv, rf = read_ply(path)
    assert np.array_equal(np.stack([rv["x"], rv["y"], rv["z"]], 1), m.verts.cpu().numpy().astype(np.float64))
    assert np.array_equal(np.stack([rv["nx"], rv["ny"], rv["nz"]], 1), m.normals.cpu().numpy().astype(np.float64))
    assert np.array_equal(rf, m.faces.cpu().numpy())
    fake.global_transform = np.eye(4)
    plain = mesh_ops.recon_mesh(fake, boxes, vs, mesh_normal=False, mesh_min_nn=4)
    assert plain.normals is None and torch.equal(plain.faces, mesh_ops.finish_mesh(chunks, normals=False).faces)
    assert mesh_ops.recon_mesh(fake, None, vs) is None


# ---------------------------------------------------------------- errors
@pytest.mark.gpu
def test_gpu_bad_arguments_are_statuses_not_faults():
    from pings_amd import _lib, mesh_ops

    v = torch.rand(6, 3, device="cuda")
    bad = torch.tensor([[0, 1, 2], [3, 4, 6]], device="cuda")          # names vertex 6 of 6
    neg = torch.tensor([[0, 1, -1]], device="cuda")
    for f in (bad, neg):
        for call in (lambda: mesh_ops.weld(v, f), lambda: mesh_ops.cluster_triangles(f, 6),
                     lambda: mesh_ops.drop_small_clusters(f, 6, 1), lambda: mesh_ops.compact_vertices(v, f),
                     lambda: mesh_ops.finish_mesh([(v, f)])):
            with pytest.raises(_lib.PingsHipError, match="outside"):
                call()
        n = mesh_ops.vertex_normals(v, f)                              # no host read: the bad face contributes nothing
        assert torch.isfinite(n).all()
    assert mesh_ops.vertex_normals(v, bad)[3:].cpu().tolist() == [[0, 0, 1]] * 3
    good = bad.clamp(max=5)
    for call in (lambda: mesh_ops.weld(v[:, :2], good), lambda: mesh_ops.weld(v, good[:, :2]),
                 lambda: mesh_ops.weld(v, good.int()), lambda: mesh_ops.vertex_normals(v.reshape(-1), good),
                 lambda: mesh_ops.cluster_triangles(good.reshape(-1), 6),
                 lambda: mesh_ops.compact_vertices(v, good, torch.rand(5, device="cuda"))):
        with pytest.raises(ValueError):
            call()
    L = _lib.lib()
    assert L.pings_mesh_weld(None, 6, None, 2, None, None, None, None, None, None, None) == 1
    assert b"null" in L.pings_last_error()
    assert L.pings_mesh_clusters(None, 0, 6, None, None, None, None, None) == 1
    assert L.pings_mesh_weld_scratch_bytes(2 ** 31, 1) == 0 and L.pings_mesh_clusters_scratch_bytes(2 ** 31 // 3 + 1) == 0
    assert L.pings_mesh_weld_scratch_bytes(100, 10) > 0
    torch.cuda.synchronize()
