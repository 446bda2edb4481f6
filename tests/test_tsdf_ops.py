"""Sparse TSDF fusion on the device (pings_amd/tsdf_ops.py, csrc/tsdf.hip) against its fp64 numpy
restatement (tests/tsdf_ref.py) on the analytic sphere scene and smaller inputs.

Outside the voxels the reference calls marginal (those fp32 cannot decide; their share is asserted from the reference
alone in tests/test_tsdf_ref.py) the block set and every weight are exact, and tsdf and colour pass the project's 1e-4
gate (`rel_err`; the largest reference tsdf is 1).  The extraction is compared on the device's own dense volume: faces
exactly, vertices within 1e-6 relative (one fp32 rounding of an fp64 evaluation is 6e-8)."""
import functools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import abi_header as hdr
import tsdf_ref as R
from conftest import rel_err
from pings_amd import _abi

KMAT = np.array([[R.K[0], 0.0, R.K[2]], [0.0, R.K[1], R.K[3]], [0.0, 0.0, 1.0]])
TSDF_SYMBOLS = ["pings_tsdf_table_insert", "pings_tsdf_touch", "pings_tsdf_assign_scratch_bytes", "pings_tsdf_assign",
                "pings_tsdf_update", "pings_tsdf_densify", "pings_tsdf_vertices"]


def test_abi_declares_tsdf_fusion():
    protos = hdr.prototypes()
    for name in TSDF_SYMBOLS:
        assert name in protos and name in _abi.SIGNATURES
    assert hdr.expected_abi() == _abi.ABI_VERSION == 11              # additions only


def test_the_block_edge_bounds_the_truncation_without_a_device():
    from pings_amd import tsdf_ops

    with pytest.raises(ValueError, match="block edge"):
        tsdf_ops.TSDFVolume(0.05, 0.2001, device="cuda:0")


# ---------------------------------------------------------------- helpers
def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


@functools.lru_cache(maxsize=None)
def frames():
    return [(dev(d), dev(c), E) for d, c, E in R.sphere_frames()]


def new_volume(**kw):
    from pings_amd import tsdf_ops

    return tsdf_ops.TSDFVolume(R.VOXEL, R.TRUNC, **kw)


def fuse(vol, n=3, **kw):
    for d, c, E in frames()[:n]:
        vol.integrate(d, KMAT, E, c if vol.color else None, **kw)
    return vol


@functools.lru_cache(maxsize=None)
def fused():
    """The three frames in a volume of ample capacity; read-only."""
    return fuse(new_volume())


def blocks_of(vol):
    return [tuple(r) for r in vol.block_coords().cpu().tolist()]


def agree(vol, ref, box=R.BOX):
    """Block set, weights exactly, tsdf and colour within 1e-4, all outside the reference's marginal set."""
    assert (set(blocks_of(vol)) ^ set(ref.coords)) <= ref.marginal_blocks
    t, w, c, m = ref.dense(*box)
    dt, dw, dc = vol.dense(*box)
    keep = torch.from_numpy(~m)
    upd = w > 0
    print(f"blocks {vol.n_blocks} / {ref.n_blocks}, updated {upd.sum()}, marginal {(m & upd).sum()}, "
          f"weight mismatches outside {(dw.cpu()[keep] != torch.from_numpy(w)[keep]).sum().item()}, "
          f"tsdf rel_err {rel_err(dt.cpu()[keep], torch.from_numpy(t)[keep]):.3e}")
    assert torch.equal(dw.cpu()[keep].double(), torch.from_numpy(w)[keep])
    assert rel_err(dt.cpu()[keep], torch.from_numpy(t)[keep]) <= 1e-4
    if vol.color:
        assert rel_err(dc.cpu()[keep], torch.from_numpy(c)[keep]) <= 1e-4
    else:
        assert dc is None
    return upd.sum()


def one_frame(depth, stride=4, color=True, **kw):
    """One frame of `depth` (numpy [H, W]) from the first camera into a fresh device volume and a fresh reference."""
    _, col, E = R.sphere_frames()[0]
    ref = R.Volume(R.VOXEL, R.TRUNC, color=color)
    ref.integrate(depth, R.K, E, col, stride=stride, **kw)
    vol = new_volume(color=color)
    vol.integrate(dev(depth), KMAT, E, dev(col) if color else None, stride=stride, **kw)
    return vol, ref


# ---------------------------------------------------------------- 1. the three frames against the reference
@pytest.mark.gpu
def test_every_frame_matches_the_reference_outside_the_marginal_voxels():
    _, snaps = R.sphere_reference()
    vol = new_volume()
    for (d, c, E), (coords, touched, (t, w, col, m), marginal_blocks) in zip(frames(), snaps):
        vol.integrate(d, KMAT, E, c)
        assert (set(blocks_of(vol)) ^ set(coords)) <= marginal_blocks
        if not marginal_blocks:
            assert blocks_of(vol) == coords                       # and in the same slot order
        dt, dw, dc = vol.dense(*R.BOX)
        keep = torch.from_numpy(~m)
        tt, tw, tc = torch.from_numpy(t), torch.from_numpy(w), torch.from_numpy(col)
        print(f"blocks {vol.n_blocks}, weight mismatches outside the marginal set "
              f"{(dw.cpu()[keep].double() != tw[keep]).sum().item()} (inside: "
              f"{(dw.cpu()[~keep].double() != tw[~keep]).sum().item()} of {(~keep).sum().item()}), "
              f"tsdf {rel_err(dt.cpu()[keep], tt[keep]):.3e} colour {rel_err(dc.cpu()[keep], tc[keep]):.3e}")
        assert torch.equal(dw.cpu()[keep].double(), tw[keep])
        assert rel_err(dt.cpu()[keep], tt[keep]) <= 1e-4
        assert rel_err(dc.cpu()[keep], tc[keep]) <= 1e-4
        # nothing outside the box, nothing but the defaults where no block is
        absent = (dw == 0)
        assert bool((dt[absent] == 1).all()) and bool((dc[absent] == 0).all())


# ---------------------------------------------------------------- 2. growth
@pytest.mark.gpu
def test_a_store_that_outgrows_its_capacity_keeps_values_and_slots():
    small = new_volume(capacity_blocks=64)
    fuse(small, 1)
    first = small.block_coords().clone()
    assert first.shape[0] > 64 and small.capacity >= first.shape[0]
    fuse_rest = frames()[1:]
    for d, c, E in fuse_rest:
        small.integrate(d, KMAT, E, c)
    big = fused()
    assert torch.equal(small.block_coords(), big.block_coords())
    assert torch.equal(small.block_coords()[:first.shape[0]], first)
    for a, b in zip(small.dense(*R.BOX), big.dense(*R.BOX)):
        assert torch.equal(a, b)
    n = big.n_blocks
    assert torch.equal(small._tsdf[:n], big._tsdf[:n]) and torch.equal(small._color[:n], big._color[:n])


# ---------------------------------------------------------------- 3. determinism
@pytest.mark.gpu
def test_two_runs_give_the_same_bits():
    a, b = fuse(new_volume()), fused()
    assert torch.equal(a.block_coords(), b.block_coords())
    for x, y in zip(a.dense(*R.BOX), b.dense(*R.BOX)):
        assert torch.equal(x, y)
    ma, mb = a.extract_mesh(chunk=24), b.extract_mesh(chunk=24)
    assert ma.faces.shape[0] > 5000
    for x, y in zip(ma, mb):
        assert torch.equal(x, y)


# ---------------------------------------------------------------- 4. edges
@pytest.mark.gpu
def test_one_frame_spans_negative_and_positive_blocks():
    depth = R.sphere_frames()[0][0]
    vol, ref = one_frame(depth)
    bc = vol.block_coords()
    assert int(bc.min()) < 0 <= int(bc.max())
    assert agree(vol, ref) > 5000
    # a negative grid point sits in the block below it: the dense box read back block by block
    t, w, _ = vol.dense(*R.BOX)
    for slot in range(0, vol.n_blocks, 13):
        g = (bc[slot] * 8 - torch.tensor(R.BOX[0], device=bc.device)).tolist()
        assert torch.equal(w[g[0]:g[0] + 8, g[1]:g[1] + 8, g[2]:g[2] + 8].reshape(-1), vol._weight[slot])


@pytest.mark.gpu
def test_a_single_valid_pixel():
    from pings_amd import _lib

    depth = np.zeros((R.H, R.W), np.float32)
    depth[28, 40] = 2.0
    _lib.sync_counts(reset=True)
    vol, ref = one_frame(depth)
    assert _lib.sync_counts() == {"tsdf_touch": 1}                    # the frame's one host read
    assert vol.n_blocks == ref.n_blocks == 8
    assert agree(vol, ref) > 0


@pytest.mark.gpu
def test_a_pixel_in_each_image_corner():
    depth = np.zeros((R.H, R.W), np.float32)
    depth[0, 0], depth[0, -1], depth[-1, 0], depth[-1, -1] = 2.0, 2.25, 2.5, 2.75
    vol, ref = one_frame(depth, stride=1)
    assert ref.n_blocks >= 4 * 8 - 8
    assert agree(vol, ref) > 0
    # with stride 4 only pixel (0, 0) is sampled, but every corner depth is still gathered by the update
    vol, ref = one_frame(depth, stride=4)
    assert ref.n_blocks == 8
    assert agree(vol, ref) > 0


@pytest.mark.gpu
def test_invalid_depths_are_left_out():
    depth = R.sphere_frames()[0][0].copy()
    depth[::3, ::5] = np.nan
    depth[1::3, 2::5] = np.inf
    depth[2::3, 3::5] = 0.0
    depth[4::8, 4::8] = -1.0
    far = depth >= 2.4
    assert far.sum() > 100 and (depth[np.isfinite(depth)] > 0).sum() - far.sum() > 100
    vol, ref = one_frame(depth, depth_trunc=2.4)
    assert agree(vol, ref) > 1000
    vol, ref = one_frame(depth, depth_trunc=2.4, depth_min=2.1)
    assert agree(vol, ref) > 100


@pytest.mark.gpu
def test_a_frame_without_a_valid_pixel_is_a_no_op():
    from pings_amd import _lib

    vol = fuse(new_volume(), 1)
    before = (vol.block_coords().clone(), *[x.clone() for x in vol.dense(*R.BOX)])
    d, c, E = frames()[1]
    _lib.sync_counts(reset=True)
    vol.integrate(torch.zeros_like(d), KMAT, E, c)
    vol.integrate(torch.full_like(d, float("nan")), KMAT, E, c)
    assert _lib.sync_counts() == {"tsdf_touch": 2}
    for x, y in zip(before, (vol.block_coords(), *vol.dense(*R.BOX))):
        assert torch.equal(x, y)
    empty = new_volume()
    empty.integrate(torch.zeros_like(d), KMAT, E, c)
    assert empty.n_blocks == 0 and empty.block_coords().shape == (0, 3)
    mesh = empty.extract_mesh()
    assert mesh.verts.shape == (0, 3) and mesh.faces.shape == (0, 3)
    t, w, col = empty.dense((-3, 0, 5), (4, 9, 7))
    assert t.shape == (7, 9, 2) and bool((t == 1).all()) and bool((w == 0).all()) and bool((col == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 7])
def test_strides(stride):
    vol, ref = one_frame(R.sphere_frames()[0][0], stride=stride)
    assert agree(vol, ref) > 5000


@pytest.mark.gpu
def test_colour_off():
    vol = fuse(new_volume(color=False))
    t, w, c = vol.dense(*R.BOX)
    assert c is None and vol._color is None
    bt, bw, _ = fused().dense(*R.BOX)
    assert torch.equal(t, bt) and torch.equal(w, bw)
    mesh = vol.extract_mesh(chunk=40)
    assert mesh.colors is None and mesh.faces.shape[0] > 5000
    with pytest.raises(ValueError, match="colour"):
        new_volume().integrate(frames()[0][0], KMAT, frames()[0][2])


@pytest.mark.gpu
def test_reset_and_a_non_zero_origin():
    d, c, E = frames()[0]
    vol = new_volume(origin=(0.013, -0.4, 0.21))
    vol.integrate(d, KMAT, E, c)
    ref = R.Volume(R.VOXEL, R.TRUNC, origin=(0.013, -0.4, 0.21))
    ref.integrate(R.sphere_frames()[0][0], R.K, E, R.sphere_frames()[0][1])
    assert agree(vol, ref) > 5000
    vol.reset()
    assert vol.n_blocks == 0 and bool((vol.dense(*R.BOX)[1] == 0).all())
    vol.integrate(d, KMAT, E, c)
    assert agree(vol, ref) > 5000


@pytest.mark.gpu
def test_arguments_that_raise():
    from pings_amd import _lib, tsdf_ops

    with pytest.raises(ValueError, match="block edge"):
        tsdf_ops.TSDFVolume(0.05, 0.2001)
    d, c, E = frames()[0]
    vol = new_volume()
    with pytest.raises(_lib.PingsHipError, match="CPU tensor"):
        vol.integrate(d.cpu(), KMAT, E, c)
    with pytest.raises(_lib.PingsHipError, match="CPU tensor"):
        vol.integrate(d, KMAT, E, c.cpu())
    with pytest.raises(ValueError):
        vol.integrate(d, KMAT[:2], E, c)
    with pytest.raises(ValueError):
        vol.integrate(d, KMAT, E[:3], c)
    with pytest.raises(ValueError):
        vol.integrate(d, KMAT, E, c, stride=0)
    assert vol.n_blocks == 0
    # K as a tensor and as an object with .intrinsic_matrix
    vol.integrate(d, torch.from_numpy(KMAT), E, c)
    other = new_volume()
    other.integrate(d, NS(intrinsic_matrix=KMAT), torch.from_numpy(E), c)
    assert torch.equal(vol.block_coords(), other.block_coords())
    # a block index beyond +-2**20 is reported, not filed
    far = np.eye(4)
    far[:3, 3] = (0.0, 0.0, -5e5)                      # camera 5e5 m up: block index 1.25e6 at voxel 0.05
    with pytest.raises(_lib.PingsHipError, match="2\\*\\*20"):
        other.integrate(d, KMAT, far, c)


# ---------------------------------------------------------------- 5. extraction
def _bounds(vol):
    bc = vol.block_coords().cpu().numpy()
    return bc.min(0) * 8, (bc.max(0) + 1) * 8


def _sorted_mesh(mesh):
    """Vertices in lexicographic order, faces renamed to it, rotated to start at their smallest index and sorted."""
    v = mesh.verts.cpu().numpy()
    order = np.lexsort((v[:, 2], v[:, 1], v[:, 0]))
    rank = np.empty(len(v), np.int64)
    rank[order] = np.arange(len(v))
    f = rank[mesh.faces.cpu().numpy()]
    k = f.argmin(1)
    f = np.stack([f[np.arange(len(f)), (k + i) % 3] for i in range(3)], 1)
    return v[order], f[np.lexsort((f[:, 2], f[:, 1], f[:, 0]))], mesh.colors.cpu().numpy()[order]


@pytest.mark.gpu
def test_extraction_matches_the_reference_on_the_devices_own_volume():
    vol = fused()
    lo, hi = _bounds(vol)
    t, w, c = (x.cpu().numpy() for x in vol.dense(lo, hi))
    rv, rf, rc = R.extract(R.masked(t, w), c, lo, vol.origin, R.VOXEL)
    mesh = vol.extract_mesh(min_weight=1, normals=False, chunk=256)
    assert mesh.normals is None and rf.shape[0] > 5000
    assert torch.equal(mesh.faces.cpu(), torch.from_numpy(rf))
    ev = np.abs(mesh.verts.cpu().numpy().astype(np.float64) - rv).max() / np.abs(rv).max()
    ec = np.abs(mesh.colors.cpu().numpy().astype(np.float64) - rc).max() / np.abs(rc).max()
    print(f"vertices {len(rv)} faces {len(rf)} vertex error {ev:.3e} colour error {ec:.3e}")
    assert ev <= 1e-6 and ec <= 1e-6
    # a higher min_weight meshes fewer cells, and the same ones as the reference
    rv2, rf2, _ = R.extract(R.masked(t, w, 2.0), c, lo, vol.origin, R.VOXEL)
    mesh2 = vol.extract_mesh(min_weight=2, normals=False)
    assert 0 < rf2.shape[0] < rf.shape[0] and torch.equal(mesh2.faces.cpu(), torch.from_numpy(rf2))


@pytest.mark.gpu
def test_chunks_weld_without_seams():
    vol = fused()
    a, b = vol.extract_mesh(chunk=16), vol.extract_mesh(chunk=64)
    va, fa, ca = _sorted_mesh(a)
    vb, fb, cb = _sorted_mesh(b)
    assert va.shape == vb.shape and fa.shape == fb.shape
    assert np.array_equal(va.view(np.uint32), vb.view(np.uint32))            # bit for bit
    assert np.array_equal(fa, fb)
    assert np.array_equal(ca.view(np.uint32), cb.view(np.uint32))
    vw, fw, _ = _sorted_mesh(vol.extract_mesh(chunk=256))                    # one chunk: no seam to begin with
    assert np.array_equal(vw.view(np.uint32), va.view(np.uint32)) and np.array_equal(fw, fa)


@pytest.mark.gpu
def test_faces_look_into_free_space():
    mesh = fused().extract_mesh(chunk=40)
    v, f = mesh.verts.double(), mesh.faces
    tri = v[f]
    normal = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert bool(((normal * tri.mean(1)).sum(1) > 0).all())
    assert bool(((mesh.normals.double() * v).sum(1) > 0).all())                 # vertex normals likewise
    assert float(mesh.colors.min()) >= 0.0 and float(mesh.colors.max()) <= 1.0


# ---------------------------------------------------------------- 6. the SLAMDataset method
@pytest.mark.gpu
def test_install_rebinds_o3d_tsdf_fusion(tmp_path):
    from pings_amd import mesh_ops, tsdf_ops
    from test_mesh_ops import read_ply

    a = 0.3
    T_c_l = np.array([[np.cos(a), -np.sin(a), 0.0, 0.1], [np.sin(a), np.cos(a), 0.0, -0.2], [0.0, 0.0, 1.0, 0.05],
                      [0.0, 0.0, 0.0, 1.0]])
    sphere = R.sphere_frames()
    poses = [np.linalg.inv(E) @ T_c_l for _, _, E in sphere]               # so that T_c_l @ inv(pose) is the extrinsic
    images = []
    for d, c, _ in sphere:
        rgb = np.rint(c.transpose(1, 2, 0) * 255.0)
        images.append(np.concatenate([rgb, d[:, :, None]], -1).astype(np.float64))      # H x W x 4: RGB 0-255 + depth

    class Loader:
        intrinsic = NS(intrinsic_matrix=KMAT)
        main_cam_name = "front"

        def __getitem__(self, i):
            return {"img": {"front": images[i - 5]}}

    Loader.T_c_l = T_c_l
    module = NS(SLAMDataset=type("SLAMDataset", (), {}))
    tsdf_ops.install(module)
    ds = module.SLAMDataset()
    ds.loader, ds.gt_poses, ds.total_pc_count = Loader(), poses, 3
    ds.config = NS(begin_frame=5, step_frame=1, max_range=2.9)
    path = tmp_path / "fused.ply"
    got = ds.o3d_tsdf_fusion(frame_step=1, output_path=path, vox_size=R.VOXEL, trunc_dist=R.TRUNC)
    assert isinstance(got, mesh_ops.Mesh)                                    # Open3D does not import here

    vol = tsdf_ops.TSDFVolume(R.VOXEL, R.TRUNC)
    for img, pose in zip(images, poses):
        color = dev(img[:, :, :3].astype(np.uint8).transpose(2, 0, 1)) / 255.0
        vol.integrate(dev(img[:, :, 3]), KMAT, T_c_l @ np.linalg.inv(pose), color, depth_trunc=2.9)
    want = vol.extract_mesh()
    assert want.faces.shape[0] > 3000
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    lines, rv, rf = read_ply(path)
    assert np.array_equal(rf.astype(np.int64), want.faces.cpu().numpy())
    assert np.array_equal(np.stack([rv["x"], rv["y"], rv["z"]], -1), want.verts.cpu().numpy().astype(np.float64))
    assert np.array_equal(np.stack([rv["nx"], rv["ny"], rv["nz"]], -1), want.normals.cpu().numpy().astype(np.float64))
    assert rv["red"].dtype == np.uint8 and len(rv) == want.verts.shape[0]
