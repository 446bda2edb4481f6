"""Mesh surface sampling without a GPU: the numpy restatement (tests/mesh_sample_ref.py) against
properties worked out by hand, `mesh_ops.read_ply`, and the argument checks of the C entry points and the drivers, all
of which answer before any GPU work."""
import math
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import mesh_sample_ref as ref
from pings_amd import _abi, _lib, eval_ops, mesh_ops


def _fan(areas):
    """One right triangle per area, stacked along z (a leg is rounded to fp32 on its own): legs sqrt(2 A)."""
    verts, faces = [], []
    for k, a in enumerate(areas):
        e = math.sqrt(2.0 * a)
        verts += [[0, 0, k], [e, 0, k], [0, e, k]]
        faces.append([3 * k, 3 * k + 1, 3 * k + 2])
    return np.array(verts, np.float32), np.array(faces, np.int64)


def test_constants_are_the_abi_s():
    assert (ref.UNIT_BITS, ref.SUM_BITS) == (_abi.MESH_SAMPLE_UNIT_BITS, _abi.MESH_SAMPLE_SUM_BITS)
    assert (ref.ST_INDEX, ref.ST_NONFINITE, ref.ST_AREA_CAP) == (_abi.MESH_SAMPLE_INDEX, _abi.MESH_SAMPLE_NONFINITE,
                                                                 _abi.MESH_SAMPLE_AREA_CAP)
    assert ref.area_cap(1 << 22) == 256 << 32                              # 4 M faces: 256 m^2 per triangle
    assert not (ref.ST_INDEX | ref.ST_NONFINITE | ref.ST_AREA_CAP) & (_abi.EVAL_EXTENT | _abi.CAMFRONT_FULL)


def test_counts_follow_the_rounded_cdf_over_six_orders_of_magnitude():
    rng = np.random.default_rng(0)
    areas = 10.0 ** rng.uniform(-5.0, 1.0, 400)
    areas[[0, 1]] = [1e-5, 10.0]
    verts, faces = _fan(areas)
    q, status = ref.areas_q(verts, faces)
    assert status == 0 and (q > 0).all()
    assert np.allclose(q / 2.0 ** 32, areas, rtol=1e-5)                    # fp32 vertices
    N = 100_003
    tri = ref.owners(q, N)
    got = np.bincount(tri, minlength=len(q))
    Q = np.cumsum(q)
    cdf_n = np.rint(Q.astype(np.float64) * N / float(Q[-1])).astype(np.int64)
    assert np.array_equal(got, np.diff(cdf_n, prepend=0))
    assert got.sum() == N and (np.diff(tri) >= 0).all()
    assert got.min() == 0 and got.max() > 1000                             # both ends of the range are exercised
    # in proportion to area, to within the rounding of the two bounds
    assert np.abs(got - q / float(Q[-1]) * N).max() <= 1.0


def test_every_sample_lies_in_its_triangle():
    rng = np.random.default_rng(1)
    verts = rng.uniform(-2, 2, (60, 3)).astype(np.float32)
    faces = rng.integers(0, 60, (100, 3))
    pts, tri, count, status = ref.sample(verts, faces, 5000, seed=7)
    assert count == 5000 and status == 0 and pts.dtype == np.float32 and tri.dtype == np.int32
    for p, t in zip(pts.astype(np.float64), tri):
        v = verts[faces[t]].astype(np.float64)
        A = np.vstack([v.T, np.ones(3)])                                   # barycentrics: A w = (p, 1)
        w, *_ = np.linalg.lstsq(A, np.append(p, 1.0), rcond=None)
        edge = max(np.linalg.norm(v[1] - v[0]), np.linalg.norm(v[2] - v[0]), np.linalg.norm(v[2] - v[1]))
        assert (w >= -1e-6).all()
        assert np.linalg.norm(v.T @ w - p) < 1e-6 * edge


def test_samples_are_uniform_inside_a_triangle():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    n = 65536
    pts, tri, _, _ = ref.sample(verts, [[0, 1, 2]], n, seed=3)
    assert (tri == 0).all()
    bary = np.stack([1.0 - pts[:, 0] - pts[:, 1], pts[:, 0], pts[:, 1]], 1).astype(np.float64)
    sigma = math.sqrt(1.0 / 18.0 / n)                                      # variance of a barycentric coordinate: 1/18
    assert np.abs(bary.mean(0) - 1.0 / 3.0).max() < 5.0 * sigma
    u1, u2 = ref.uniforms(3, np.arange(n))
    assert u1.min() >= 0 and u1.max() < 1 and np.array_equal(u1 * 2.0 ** 32, np.floor(u1 * 2.0 ** 32))
    assert not np.array_equal(u1, ref.uniforms(4, np.arange(n))[0])
    # keyed on (seed, i) only: a longer run starts with the same numbers
    assert np.array_equal(ref.uniforms(3, np.arange(10))[1], u2[:10])


def test_crop_rule_is_inclusive_and_needs_all_three_vertices():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [2, 0, 0]], np.float32)
    faces = np.array([[0, 1, 2], [1, 3, 2], [1, 4, 3]])
    lo, hi = [0, 0, 0], [1, 1, 0]                                          # every kept vertex lies exactly on a bound
    assert ref.crop_faces(verts, faces, lo, hi).tolist() == [[0, 1, 2], [1, 3, 2]]     # vertex 4 is outside
    q, _ = ref.areas_q(verts, faces, (lo, hi))
    assert q.tolist() == [1 << 31, 1 << 31, 0]
    q, _ = ref.areas_q(verts, faces, (lo, [np.nextafter(1.0, 0.0), 1, 0]))
    assert q.tolist() == [0, 0, 0]
    assert ref.sample(verts, faces, 10, box=(lo, [0.5, 1, 0]))[2] == 0
    # a dropped face adds 0 to Q: the same cloud as sampling the survivors
    a, b = ref.sample(verts, faces, 1000, 5, (lo, hi)), ref.sample(verts, faces[:2], 1000, 5)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


def test_status_bits_of_the_restatement():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0]], np.float32)
    assert ref.areas_q(verts, [[0, 1, 2], [0, 1, 4]])[1] == ref.ST_INDEX
    assert ref.areas_q(verts, [[0, 1, 2], [0, 1, -1]])[1] == ref.ST_INDEX
    q, st = ref.areas_q(verts, [[0, 1, 3], [0, 1, 2]])
    assert st == ref.ST_NONFINITE and q.tolist() == [0, 1 << 31]
    big = np.array([[0, 0, 0], [3e5, 0, 0], [0, 3e5, 0]], np.float32)      # 4.5e10 m^2 > 2^30 m^2, the cap of one face
    q, st = ref.areas_q(big, [[0, 1, 2]])
    assert st == ref.ST_AREA_CAP and q.tolist() == [0]
    assert ref.areas_q(big * 0.1, [[0, 1, 2]])[1] == 0
    q, st = ref.areas_q(verts, [[0, 0, 1], [0, 1, 1]])                      # degenerate: no area, no bit
    assert st == 0 and q.tolist() == [0, 0] and ref.sample(verts, [[0, 0, 1]], 5)[2] == 0


# ------------------------------------------------------------------ read_ply
def _mesh():
    rng = np.random.default_rng(2)
    return (rng.normal(size=(7, 3)), rng.integers(0, 7, (5, 3)), rng.normal(size=(7, 3)), rng.uniform(0, 1, (7, 3)))


@pytest.mark.parametrize("with_normals, with_colors, with_faces",
                         [(True, True, True), (False, False, True), (True, False, False), (False, True, True)])
def test_read_ply_round_trip(tmp_path, with_normals, with_colors, with_faces):
    v, f, n, c = _mesh()
    f = f if with_faces else np.zeros((0, 3), np.int64)
    path = tmp_path / "m.ply"
    mesh_ops.write_ply(path, v, f, n if with_normals else None, c if with_colors else None)
    got = mesh_ops.read_ply(path)
    assert got["verts"].dtype == np.float64 and np.array_equal(got["verts"], v)
    assert got["faces"].dtype == np.int64 and got["faces"].shape == (len(f), 3) and np.array_equal(got["faces"], f)
    assert ("normals" in got) == with_normals and ("colors" in got) == with_colors
    if with_normals:
        assert np.array_equal(got["normals"], n)
    if with_colors:
        assert np.array_equal(got["colors"], np.rint(c * 255.0) / 255.0)


ASCII = """ply
format ascii 1.0
comment by hand
element vertex 4
property float x
property float y
property float quality
property float z
property uchar red
property uchar green
property uchar blue
element face 2
property list uchar int vertex_index
end_header
0 0 9.5 0 255 0 0
1 0 9.5 0.25 0 255 0
0 1 9.5 0.5 0 0 255
1 1 9.5 1 51 51 51
3 0 1 2
3 1 3 2
"""


def test_read_ply_ascii_with_an_extra_property(tmp_path):
    path = tmp_path / "a.ply"
    path.write_text(ASCII)
    got = mesh_ops.read_ply(path)
    assert got["verts"].tolist() == [[0, 0, 0], [1, 0, 0.25], [0, 1, 0.5], [1, 1, 1]]
    assert got["faces"].tolist() == [[0, 1, 2], [1, 3, 2]] and got["faces"].dtype == np.int64
    assert got["colors"].tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.2, 0.2, 0.2]] and "normals" not in got


def test_read_ply_binary_skips_unknown_properties_and_reads_a_cloud(tmp_path):
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\n"
            "property float z\nproperty float intensity\nproperty ushort ring\nend_header\n")
    rec = np.zeros(3, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4"), ("ring", "<u2")])
    rec["x"], rec["y"], rec["z"], rec["intensity"], rec["ring"] = [1, 2, 3], [4, 5, 6], [7, 8, 9], 0.5, 7
    path = tmp_path / "c.ply"
    path.write_bytes(head.encode() + rec.tobytes())
    got = mesh_ops.read_ply(path)
    assert got["verts"].tolist() == [[1, 4, 7], [2, 5, 8], [3, 6, 9]] and got["faces"].shape == (0, 3)
    assert sorted(got) == ["faces", "verts"]


@pytest.mark.parametrize("old, new, line", [
    ("format ascii 1.0", "format binary_big_endian 1.0", 2),
    ("3 1 3 2", "4 1 3 2 0", 20),
    ("property float quality", "property list uchar float quality", 7),
    ("property list uchar int vertex_index", "property list uchar short vertex_index", 13),
    ("element face 2", "element edge 2", 12),
    ("property float z", "property half z", 8),
])
def test_read_ply_rejects_what_it_does_not_read(tmp_path, old, new, line):
    path = tmp_path / "bad.ply"
    path.write_text(ASCII.replace(old, new))
    with pytest.raises(ValueError, match=f"line {line}:"):
        mesh_ops.read_ply(path)


def test_read_ply_rejects_binary_faces_that_are_no_triangles(tmp_path):
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty double x\nproperty double y\n"
            "property double z\nelement face 1\nproperty list uchar uint vertex_indices\nend_header\n")
    path = tmp_path / "quad.ply"
    path.write_bytes(head.encode() + np.zeros(12, "<f8").tobytes() + b"\x04" + np.arange(4, dtype="<u4").tobytes())
    with pytest.raises(ValueError, match="line 7:.*triangles"):
        mesh_ops.read_ply(path)
    (tmp_path / "none.ply").write_text("solid\n")
    with pytest.raises(ValueError, match="line 1:"):
        mesh_ops.read_ply(tmp_path / "none.ply")


# ------------------------------------------------------------------ argument checks, before any GPU work
def test_entry_point_rejects_null_pointers_and_empty_or_oversized_shapes():
    L = _lib.lib()
    p = 4096                                       # pointers need only be non-null: every case is refused before a launch
    int_max = 2 ** 31 - 1
    assert L.pings_mesh_sample(None, 3, None, 1, None, 8, 0, None, None, None, None, None, None) == 1
    assert b"null" in L.pings_last_error()
    assert L.pings_mesh_sample(p, 3, p, 1, None, 8, 0, p, p, None, None, p, None) == 1       # count is required
    assert b"null" in L.pings_last_error()
    assert L.pings_mesh_sample(p, 3, p, 0, None, 8, 0, p, p, None, p, p, None) == 1          # F = 0
    assert b"mesh" in L.pings_last_error()
    assert L.pings_mesh_sample(p, 0, p, 1, None, 8, 0, p, p, None, p, p, None) == 1          # V = 0
    assert L.pings_mesh_sample(p, 3, p, 1, None, 0, 0, p, p, None, p, p, None) == 1          # N = 0
    assert b"sample" in L.pings_last_error()
    assert L.pings_mesh_sample(p, 3, p, 1, None, int_max + 1, 0, p, p, None, p, p, None) == 1
    assert b"sample" in L.pings_last_error()
    assert L.pings_mesh_sample(p, 3, p, int_max + 1, None, 8, 0, p, p, None, p, p, None) == 1
    assert L.pings_mesh_sample_scratch_bytes(0) == 0
    assert L.pings_mesh_sample_scratch_bytes(int_max + 1) == 0
    assert L.pings_mesh_sample_scratch_bytes(1000) >= 2 * 8 * 1000


def test_drivers_check_their_arguments():
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64)
    with pytest.raises(_lib.PingsHipError, match="no CPU fallback"):
        mesh_ops.sample_surface(v, f, 10)
    with pytest.raises(_lib.PingsHipError, match="no CPU fallback"):
        mesh_ops.crop_box(v, f, [0, 0, 0], [1, 1, 1])
    with pytest.raises(NotImplementedError, match="Poisson"):
        eval_ops.eval_mesh((np.zeros((3, 3)), np.zeros((1, 3))), np.zeros((4, 3)), down_sample_res=0.0)
    with pytest.raises(ValueError):
        eval_ops.eval_mesh((np.zeros((3, 3)), np.zeros((1, 3))), np.zeros((4, 3)), down_sample_res=0.0,
                           possion_sample_on=False)
    with pytest.raises(ValueError):
        eval_ops.eval_mesh((np.zeros((3, 3)), np.zeros((1, 3))), np.zeros((4, 3)), mesh_sample_point=0)
    with pytest.raises(TypeError):
        eval_ops.eval_mesh(np.zeros((3, 3)), np.zeros((4, 3)))
    with pytest.raises(_lib.PingsHipError):
        eval_ops.eval_mesh((v, f), np.zeros((4, 3)))
    # an empty mesh or target never reaches the device: eval_pair's answer for an empty pred
    want = eval_ops.pair_metrics([0.0] * 8, 0.02, 0.05, 0.5, 0.5)
    got = eval_ops.eval_mesh((np.zeros((0, 3)), np.zeros((0, 3))), np.zeros((4, 3)))
    assert list(got) == list(want) and all(math.isnan(got[k]) for k in eval_ops.PAIR_KEYS[:7])
    assert [got[k] for k in eval_ops.PAIR_KEYS[7:]] == [want[k] for k in eval_ops.PAIR_KEYS[7:]]
    assert mesh_ops.sample_status_error(0) is None and mesh_ops.sample_status_error(_abi.MESH_SAMPLE_NONFINITE) is None
    assert "cap" in mesh_ops.sample_status_error(_abi.MESH_SAMPLE_AREA_CAP)
    assert "vertex" in mesh_ops.sample_status_error(_abi.MESH_SAMPLE_INDEX)


def test_install_binds_the_mesh_names_only_on_request():
    keep = lambda: None
    mod = NS(eval_pair=None, nn_correspondance=None, eval_mesh=keep, crop_intersection=keep)
    eval_ops.install(mod)
    assert mod.eval_mesh is keep and mod.crop_intersection is keep and mod.eval_pair is eval_ops.eval_pair
    eval_ops.install(mod, mesh=True)
    assert mod.eval_mesh is eval_ops.eval_mesh and mod.crop_intersection is eval_ops.crop_intersection
    assert mod.eval_pair is eval_ops.eval_pair and mod.nn_correspondance is eval_ops.nn_correspondance
