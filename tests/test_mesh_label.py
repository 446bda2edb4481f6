"""Labelled meshes (mesh_ops.label_colors / remove_vertices / recon_mesh(estimate_sem=True), csrc/mesh_label.hip)
against the numpy restatement of Open3D's remove_vertices_by_mask (tests/sem_ref.py) and the composed steps."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import abi_header as hdr
import sem_ref

COLOR_MAP = {0: [255, 255, 255], 1: [100, 150, 245], 4: [80, 30, 180]}


# ------------------------------------------------------------------ CPU
def test_restatement_removes_vertices_and_their_faces():
    v = np.arange(18, dtype=np.float32).reshape(6, 3)
    f = np.array([[0, 1, 2], [2, 3, 4], [3, 4, 5], [5, 3, 0]], dtype=np.int64)
    drop = np.array([False, True, False, False, False, False])
    rv, rf, kept = sem_ref.remove_vertices_by_mask(v, f, drop)
    assert kept.tolist() == [0, 2, 3, 4, 5] and np.array_equal(rv, v[[0, 2, 3, 4, 5]])
    assert rf.tolist() == [[1, 2, 3], [2, 3, 4], [4, 2, 0]]          # face 0 names vertex 1; the rest renumbered
    rv, rf, kept = sem_ref.remove_vertices_by_mask(v, f, np.ones(6, bool))
    assert rv.shape == (0, 3) and rf.shape == (0, 3) and kept.shape == (0,)
    rv, rf, kept = sem_ref.remove_vertices_by_mask(v, f, np.zeros(6, bool))
    assert np.array_equal(rv, v) and np.array_equal(rf, f)


def test_header_declares_the_mesh_label_symbols():
    names = hdr.header_symbols()
    for n in ("pings_mesh_label_colors", "pings_mesh_remove_vertices_scratch_bytes", "pings_mesh_remove_vertices"):
        assert n in names


def test_install_semantic_reads_the_colour_map_and_routes_estimate_sem():
    from pings_amd import mesher_ops as MO

    def original(self, *a, **k):
        return "original"

    def module(**kw):
        return NS(Mesher=type("Mesher", (), {"recon_aabb_collections_mesh": original}), **kw)

    fin, sem = module(sem_kitti_color_map=COLOR_MAP), module(sem_kitti_color_map=COLOR_MAP)
    MO.install(fin, finish=True)
    MO.install(sem, finish=True, semantic=True)
    MO.install(sem, finish=True, semantic=True)                      # twice: the saved original stays the original
    assert fin.Mesher().recon_aabb_collections_mesh([], 0.1, estimate_sem=True) == "original"
    assert not hasattr(fin.Mesher, "_pings_label_colors")
    assert sem.Mesher.recon_aabb_collections_mesh._pings_original is original
    assert sem.Mesher().recon_aabb_collections_mesh(None, 0.1, estimate_sem=True) is None      # not the original
    table, valid = sem.Mesher._pings_label_colors
    assert table.dtype == torch.uint8 and valid.dtype == torch.bool and not table.is_cuda
    assert table.tolist() == [[255, 255, 255], [100, 150, 245], [0, 0, 0], [0, 0, 0], [80, 30, 180]]
    assert valid.tolist() == [True, True, False, False, True]
    with pytest.raises(ValueError, match="finish=True"):
        MO.install(module(sem_kitti_color_map=COLOR_MAP), semantic=True)
    with pytest.raises(ValueError, match="sem_kitti_color_map"):
        MO.install(module(), finish=True, semantic=True)
    with pytest.raises(ValueError, match="0..255"):
        MO.color_table({0: [0, 0, 256]})
    with pytest.raises(ValueError, match="negative"):
        MO.color_table({-1: [0, 0, 0]})


def test_argument_validation():
    from pings_amd import _lib, mesh_ops, mesher_ops as MO

    v, f = torch.rand(4, 3), torch.tensor([[0, 1, 2]])
    table, valid = MO.color_table(COLOR_MAP)
    with pytest.raises(_lib.PingsHipError, match="no CPU fallback"):
        mesh_ops.remove_vertices(v, f, torch.zeros(4, dtype=torch.bool))
    with pytest.raises(_lib.PingsHipError, match="no CPU fallback"):
        mesh_ops.label_colors(torch.zeros(4, dtype=torch.int64), table, valid)
    mesher = NS(config=NS(infer_bs=100), sem_mlp=None)
    with pytest.raises(ValueError, match="label_colors"):
        mesh_ops.recon_mesh(mesher, [], 0.1, estimate_sem=True)
    with pytest.raises(ValueError, match="sem_mlp"):
        mesh_ops.recon_mesh(mesher, [], 0.1, estimate_sem=True, label_colors=(table, valid))
    with pytest.raises(ValueError, match="sem_mlp"):
        MO.label_vertices(mesher, v)


# ------------------------------------------------------------------ GPU
def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def check_remove(v, f, drop, attr):
    from pings_amd import _lib, mesh_ops

    _lib.sync_counts(reset=True)
    gv, gf, ga = mesh_ops.remove_vertices(dev(v), dev(f), dev(drop), dev(attr))
    assert _lib.sync_counts(reset=True) == ({"mesh_remove_vertices": 1} if len(v) else {})     # one host read
    rv, rf, kept = sem_ref.remove_vertices_by_mask(v, f, drop)
    assert gv.dtype == torch.float32 and gf.dtype == torch.int64
    assert tuple(gv.shape) == rv.shape and tuple(gf.shape) == rf.shape and tuple(ga.shape) == attr[kept].shape
    assert gv.cpu().numpy().tobytes() == rv.tobytes()
    assert np.array_equal(gf.cpu().numpy(), rf)
    assert ga.cpu().numpy().tobytes() == attr[kept].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("density", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("V", [1, 255, 256, 257, 4097])
def test_gpu_remove_vertices_random(V, density):
    rng = np.random.default_rng(V)
    v = rng.standard_normal((V, 3)).astype(np.float32)
    f = rng.integers(0, V, (2 * V, 3)).astype(np.int64)
    drop = rng.random(V) < density
    if density == 0.3 and V > 1:
        assert drop.any() and not drop.all()
    check_remove(v, f, drop, rng.standard_normal((V, 2)).astype(np.float32))


@pytest.mark.gpu
def test_gpu_remove_vertices_sphere_cut_by_a_half_space_and_empty_meshes():
    from pings_amd import mesh_ops, mesher_ops as MO
    from test_mc import sphere

    gv, gf = MO.marching_cubes(torch.from_numpy(sphere()).cuda())
    v, f = gv.cpu().numpy(), gf.cpu().numpy()
    drop = v[:, 0] > 11.5
    assert drop.any() and not drop.all()
    rv, rf, _ = sem_ref.remove_vertices_by_mask(v, f, drop)
    assert 0 < len(rf) < len(f)
    check_remove(v, f, drop, np.arange(len(v), dtype=np.int64))
    # no vertices, and no faces
    z = mesh_ops.remove_vertices(torch.zeros(0, 3, device="cuda"), torch.zeros(0, 3, dtype=torch.int64, device="cuda"),
                                 torch.zeros(0, dtype=torch.bool, device="cuda"), torch.zeros(0, 3, device="cuda"))
    assert [tuple(t.shape) for t in z] == [(0, 3), (0, 3), (0, 3)]
    check_remove(v, np.zeros((0, 3), np.int64), drop, np.arange(len(v), dtype=np.int64))
    with pytest.raises(Exception, match="outside"):
        mesh_ops.remove_vertices(gv, torch.tensor([[0, 1, len(v)]], device="cuda"), dev(drop))


@pytest.mark.gpu
def test_gpu_label_colors_lookup_is_exact_and_a_missing_label_raises_at_the_read():
    from pings_amd import _lib, mesh_ops, mesher_ops as MO

    table, valid = MO.color_table({k: [(37 * k + 11) % 256, (91 * k) % 256, 255 - k] for k in range(0, 40, 1) if k != 7},
                                  "cuda")
    T = table.shape[0]
    rng = np.random.default_rng(3)
    lab = rng.integers(0, T, 4097)
    lab[lab == 7] = 8
    labels = dev(lab.astype(np.int64))
    _lib.sync_counts(reset=True)
    colors, drop = mesh_ops.label_colors(labels, table, valid)
    assert _lib.sync_counts() == {}                                  # no host read
    want = table.cpu()[lab].float() / 255.0
    assert colors.dtype == torch.float32 and torch.equal(colors.cpu(), want)
    assert drop.dtype == torch.bool and np.array_equal(drop.cpu().numpy(), lab <= 0)
    v = torch.rand(4097, 3, device="cuda")
    f = torch.zeros(0, 3, dtype=torch.int64, device="cuda")
    out = mesh_ops.remove_vertices(v, f, drop, colors)               # every label has its colour: no error
    assert out[0].shape[0] == int((lab > 0).sum()) and torch.equal(out[2].cpu(), want[lab > 0])
    for bad in (T, -1, 7, 2 ** 40):                                  # past the table, negative, a hole, far outside
        lab2 = lab.copy()
        lab2[[5, 4000]] = bad
        c2, d2 = mesh_ops.label_colors(dev(lab2.astype(np.int64)), table, valid)
        keep = np.ones(4097, bool)
        keep[[5, 4000]] = False
        assert torch.equal(c2.cpu()[keep], want[keep]) and float(c2[5].abs().max()) == 0.0
        assert bool(d2[5]) == (bad <= 0)
        with pytest.raises(ValueError, match="2 vertex label"):
            mesh_ops.remove_vertices(v, f, d2, c2)


def _sem_decoder(IN, S, seed):
    g = torch.Generator().manual_seed(seed)
    p = [0.4 * torch.randn(64, IN, generator=g), 0.1 * torch.randn(64, generator=g),
         0.6 * torch.randn(S, 64, generator=g), torch.zeros(S)]
    p = [t.cuda() for t in p]
    return NS(layers=[NS(weight=p[0], bias=p[1])], lout=NS(weight=p[2], bias=p[3]), use_leaky_relu=False)


@pytest.mark.gpu
@pytest.mark.parametrize("filter_free", [True, False])
def test_gpu_recon_mesh_with_labels_equals_finish_mesh_over_labelled_chunks(golden_dir, filter_free):
    from pings_amd import mesh_ops, mesher_ops as MO
    from test_sdf import _Dec, _gpu_map, load

    name, S = "gs_f32", 3
    st = load(golden_dir, name)
    z = np.load(golden_dir / "mesher_grid.npz")
    T = np.eye(4)
    T[:3, 3] = (1.0, -2.0, 0.5)
    dec = _Dec(st)
    # The fixture's SDF is negative wherever the map has neighbours (-0.040 .. -0.026) and 0 where it has none, so its
    # zero level lies on grid points without a neighbour, and a vertex there has all-zero IDW weights: label 0 for
    # every vertex, whatever the decoder.  A bias of +0.033 m moves the level into the supported region; three in four
    # vertices then have neighbours and the seed-2 decoder gives them labels 0, 1 and 2 (about 1/4 end with label 0).
    dec.lout.bias = dec.lout.bias + 0.033 / dec.sdf_scale
    fake = NS(neural_points=_gpu_map(st), sdf_mlp=dec, sem_mlp=_sem_decoder(dec.layers[0].weight.shape[1], S, seed=2),
              color_mlp=None, global_transform=T,
              config=NS(weighted_first=bool(st["weighted_first"]), color_channel=3, pad_voxel=1, skip_top_voxel=1,
                        infer_bs=1000, mc_mask_on=True, min_cluster_vertices=5))
    vs = float(z[f"{name}_voxel"])
    lo, hi = np.asarray(z[f"{name}_min"], np.float64), np.asarray(z[f"{name}_max"], np.float64)
    mid = lo[0] + vs * np.ceil((hi[0] - lo[0]) / vs / 2)
    boxes = [(lo, np.array([mid, hi[1], hi[2]])), (np.array([mid, lo[1], lo[2]]), hi)]      # two abutting boxes
    lc = MO.color_table({0: [255, 255, 255], 1: [100, 150, 245], 2: [30, 60, 150]}, "cuda")
    m = mesh_ops.recon_mesh(fake, boxes, vs, mesh_min_nn=4, estimate_sem=True, estimate_color=True,
                            filter_free_space_vertices=filter_free, label_colors=lc)
    chunks, cols, n_drop, n_all = [], [], 0, 0
    for a, b in boxes:
        v, f = MO.mesh_bbx(fake, a, b, vs, mesh_min_nn=4)
        lab = MO.label_vertices(fake, v).cpu().numpy()
        assert lab.dtype == np.int64 and lab.min() >= 0 and lab.max() < S
        col = (lc[0].cpu().numpy()[lab].astype(np.float32) / np.float32(255.0))
        n_drop, n_all = n_drop + int((lab <= 0).sum()), n_all + len(lab)
        if filter_free:
            rv, rf, kept = sem_ref.remove_vertices_by_mask(v.cpu().numpy(), f.cpu().numpy(), lab <= 0)
            v, f, col = dev(rv), dev(rf), col[kept]
        chunks.append((v, f))
        cols.append(dev(col))
    print(f"vertices {n_all}, label <= 0: {n_drop}")
    assert 0 < n_drop < n_all                                        # some vertices are dropped and some are kept
    want = mesh_ops.finish_mesh(chunks, colors=torch.cat(cols), transform=T)
    assert m.faces.shape[0] > 0 and m.colors is not None and m.colors.shape == (m.verts.shape[0], 3)
    for a, b in zip(m, want):
        assert torch.equal(a, b)
    if filter_free:
        assert not bool((m.colors == 1.0).all(dim=1).any())          # label 0 is white: none is left
