"""The numpy restatement of the TSDF fusion (tests/tsdf_ref.py) on its own, without a GPU: that the
analytic scene is one fp32 can decide almost everywhere, that the fused surface is the sphere, and that chunked
extraction has no seams.

Measured with this file's scene (unit sphere, three 80x60 views, voxel 0.05, trunc 0.2, stride 4): 93 / 90 / 82 touched
blocks per frame, 168 blocks and 24,271 updated voxels after the third; 0.99 % of the updated voxels marginal (no
marginal block: 2 trunc equals the block edge, so every pixel names two blocks per axis); zero crossings off the sphere
by 0.107 voxel on average and 0.820 voxel at most (at silhouettes); 4,472 vertices and 8,191 faces."""
import numpy as np

import tsdf_ref as R


def _mesh(chunk=None):
    vol, snaps = R.sphere_reference()
    t, w, c, _ = snaps[-1][2]
    return R.extract(R.masked(t, w), c, R.BOX[0], vol.origin, R.VOXEL, chunk)


def test_the_scene_is_one_fp32_can_decide():
    """A condition on the scene, from the reference alone: under 2.5 % of the updated voxels are marginal."""
    vol, snaps = R.sphere_reference()
    for blocks, touched, (t, w, c, m), _ in snaps:
        upd = w > 0
        share = (m & upd).sum() / upd.sum()
        print(f"blocks {len(blocks)} touched {touched} updated {upd.sum()} marginal {share:.4%}")
        assert 50 <= touched <= 200 and share < 0.025
    assert snaps[-1][2][1].sum() > 20000            # enough updated voxels (and views) for the share to mean something
    assert snaps[-1][2][1].max() == 3.0


def test_zero_crossings_lie_on_the_sphere():
    verts, faces, colors = _mesh()
    err = np.abs(np.linalg.norm(verts, axis=1) - 1.0) / R.VOXEL
    print(f"crossing error in voxels: mean {err.mean():.4f} max {err.max():.4f}; {len(verts)} vertices {len(faces)} faces")
    assert len(faces) > 5000
    assert err.mean() <= 0.2 and err.max() <= 1.5
    assert colors.min() >= 0.0 and colors.max() <= 1.0
    tri = verts[faces]
    normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert ((normal * tri.mean(1)).sum(1) > 0).all()         # free space is outside the sphere


def test_chunked_extraction_gives_the_same_vertex_set():
    v1, f1, c1 = _mesh()
    for chunk in (16, 33):
        v2, f2, c2 = _mesh(chunk)
        assert f2.shape == f1.shape
        assert len(v2) > len(v1)                             # the shared planes are there twice before the weld
        assert set(map(tuple, np.hstack([v1, c1]))) == set(map(tuple, np.hstack([v2, c2])))


def test_a_frame_of_zeros_changes_nothing():
    depth, col, E = R.sphere_frames()[0]
    vol = R.Volume(R.VOXEL, R.TRUNC)
    vol.integrate(depth, R.K, E, col)
    before = [a.copy() for a in (vol.tsdf, vol.weight, vol.color, vol.marginal)], list(vol.coords)
    assert vol.integrate(np.zeros_like(depth), R.K, E, col) == set()
    bad = np.full_like(depth, np.nan)
    bad[::2] = np.inf
    bad[0, 0], bad[4, 4], bad[8, 8] = -1.0, 7.0, 5.0           # not positive, beyond and at depth_trunc
    assert vol.integrate(bad, R.K, E, col, depth_trunc=5.0) == set()
    assert list(vol.coords) == before[1]
    for a, b in zip((vol.tsdf, vol.weight, vol.color, vol.marginal), before[0]):
        assert np.array_equal(a, b)


def test_blocks_use_floor_division_on_both_sides_of_the_origin():
    vol, _ = R.sphere_reference()
    bc = np.array(vol.coords)
    assert bc.min() < 0 <= bc.max()
    t, w, _, _ = vol.dense(*R.BOX)
    for b, slot in list(vol.slots.items())[::17]:
        g = np.array(b) * R.B - np.array(R.BOX[0])
        assert np.array_equal(w[g[0]:g[0] + 8, g[1]:g[1] + 8, g[2]:g[2] + 8].reshape(-1), vol.weight[slot])
    with np.testing.assert_raises(ValueError):
        R.Volume(0.05, 0.2001)
