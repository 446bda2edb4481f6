"""The fp64 restatement of LiDAR-scan fusion (tests/tsdf_points_ref.py) checked on its own, without a
device: the ABI names, the share of voxels it calls marginal, hand-computed rays, carving, the weight cap and the
independence from the order of the points."""
import numpy as np
import pytest

import abi_header as hdr
import tsdf_points_ref as P
import tsdf_ref as R
from pings_amd import _abi

POINTS_SYMBOLS = ["pings_tsdf_points_touch", "pings_tsdf_points_accumulate", "pings_tsdf_points_apply"]
MARGINAL_CAP = 0.025                 # the project's cap of DESIGN §2.9


def test_abi_declares_point_fusion():
    protos = hdr.prototypes()
    for name in POINTS_SYMBOLS:
        assert name in protos and name in _abi.SIGNATURES
    defines = hdr.defines()
    assert defines["PINGS_TSDF_POINTS_SCALE_BITS"] == _abi.TSDF_POINTS_SCALE_BITS == P.SCALE_BITS
    assert defines["PINGS_TSDF_POINTS_MAX"] == _abi.TSDF_POINTS_MAX == P.MAX_POINTS
    # count above the sum: MAX_POINTS samples of at most 2^(SCALE_BITS + 1) stay below the count field
    assert P.MAX_POINTS << (P.SCALE_BITS + 1) < 1 << _abi.TSDF_POINTS_COUNT_SHIFT
    assert P.MAX_POINTS < 1 << (64 - _abi.TSDF_POINTS_COUNT_SHIFT)
    assert hdr.expected_abi() == _abi.ABI_VERSION                     # additions only


@pytest.mark.parametrize("carved", [False, True])
@pytest.mark.parametrize("sdf_mode", ["point", "ray"])
def test_the_marginal_share_stays_under_the_cap(sdf_mode, carved):
    vol, snaps = P.sphere_reference(sdf_mode, carved)
    rays = sum(len(s[0]) for s in P.sphere_scans(carved))
    samples = sum(sum(c.values()) for *_, c in snaps)
    t, w, c, m = snaps[-1][1]
    upd = w > 0
    share = (m & upd).sum() / upd.sum()
    print(f"{sdf_mode} carved={carved}: rays {rays}, updating samples per ray {samples / rays:.1f}, updated voxels "
          f"{upd.sum()}, blocks {vol.n_blocks}, marginal voxels {(m & upd).sum()} = {100 * share:.2f} %, marginal "
          f"blocks {len(vol.marginal_blocks)}")
    assert rays > (500 if carved else 2000) and upd.sum() > 10000
    assert share <= MARGINAL_CAP
    assert (t[upd] >= -1.0).all() and (t[upd] <= 1.0).all() and (t[~upd] == 1.0).all()
    assert (c[upd] >= 0.0).all() and (c[upd] <= 1.0).all()


def _one_ray(sdf_mode, carve, **kw):
    vol = P.Volume(1.0, 2.0, color=False)
    vol.integrate_points(np.array([[5.25, 0.125, -0.25]]), (0.25, 0.125, -0.25), space_carving=carve, sdf_mode=sdf_mode,
                         max_range=10.0, **kw)
    t, w, _, _ = vol.dense((-8, -8, -8), (16, 8, 8))
    return vol, t, w


def test_a_hand_computed_ray_along_x_projective():
    """o = (0.25, 0.125, -0.25), p = o + 5 e_x (all exact in fp32), voxel 1, trunc 2: s in [3, 7] is x in [3.25, 7.25],
    the cubes of g_x = 3 .. 7 (chords 0.25, 1, 1, 1, 0.75); sdf = 5 - (g_x - 0.25) = 2.25, 1.25, 0.25, -0.75, -1.75."""
    vol, t, w = _one_ray("ray", False)
    assert vol.coords == [(0, 0, 0)]
    line_t, line_w = t[8:, 8, 8], w[8:, 8, 8]                      # g = (0 .. 15, 0, 0)
    assert np.array_equal(line_w, [0, 0, 0, 1, 1, 1, 1, 1] + [0] * 8)
    want = np.array([1.0, 0.625, 0.125, -0.375, -0.875])
    assert np.abs(line_t[3:8] - want).max() <= 2.0 ** -(P.SCALE_BITS + 1)          # one quantisation
    assert w.sum() == 5 and (t[w == 0] == 1).all()


def test_a_hand_computed_ray_along_x_point_distance():
    """The same ray: p - c = (5.25 - g_x, 0.125, -0.25), |p - c| = sqrt((5.25 - g_x)^2 + 0.078125); (c - o).(p - c) =
    (g_x - 0.25)(5.25 - g_x) - 0.078125 is positive for g_x = 3, 4, 5 and negative for 6, 7."""
    vol, t, w = _one_ray("point", False)
    gx = np.arange(3, 8)
    dist = np.sqrt((5.25 - gx) ** 2 + 0.078125)
    want = np.minimum(1.0, np.where(gx <= 5, dist, -dist) / 2.0)
    assert want[0] == 1.0 and want[3] < 0
    assert np.abs(t[8:, 8, 8][3:8] - want).max() <= 2.0 ** -(P.SCALE_BITS + 1)
    assert np.array_equal(w[8:, 8, 8], [0, 0, 0, 1, 1, 1, 1, 1] + [0] * 8)


@pytest.mark.parametrize("sdf_mode", ["point", "ray"])
def test_free_space_is_seen_only_with_carving(sdf_mode):
    """g_x = 1, 2 lie between sensor and surface, further than trunc in front of it.  The sensor's own cube g_x = 0 has
    its centre behind the sensor: (c - o).(p - c) < 0 there, so the point distance is -|p - c| < -trunc and only the
    projective mode, 5.25 in front of the surface, sees it."""
    _, t, w = _one_ray(sdf_mode, False)
    assert (w[8:11, 8, 8] == 0).all() and (t[8:11, 8, 8] == 1).all()
    _, t, w = _one_ray(sdf_mode, True)
    own = 1 if sdf_mode == "ray" else 0
    assert w[8, 8, 8] == own and (w[9:16, 8, 8] == 1).all() and (t[8:12, 8, 8] == 1).all() and w.sum() == 7 + own


def test_the_weight_cap_clamps_and_is_what_the_next_call_averages_with():
    vol = P.Volume(1.0, 2.0, color=False)
    pts, o = np.array([[5.25, 0.125, -0.25]] * 5), (0.25, 0.125, -0.25)
    vol.integrate_points(pts, o, sdf_mode="ray", max_weight=3)                     # 5 samples per voxel at once
    t, w, _, _ = vol.dense((3, 0, 0), (8, 1, 1))
    assert (w == 3).all() and t[2, 0, 0] == 0.125
    vol.integrate_points(np.array([[4.25, 0.125, -0.25]]), o, sdf_mode="ray", max_weight=3)   # g_x = 5: sdf -0.75
    t, w, _, _ = vol.dense((3, 0, 0), (8, 1, 1))
    assert w[2, 0, 0] == 3 and t[2, 0, 0] == (0.125 * 3 - 0.375) / 4
    free = P.Volume(1.0, 2.0, color=False)
    free.integrate_points(pts, o, sdf_mode="ray")
    assert (free.dense((3, 0, 0), (8, 1, 1))[1] == 5).all()


@pytest.mark.parametrize("carved", [False, True])
def test_the_order_of_the_points_does_not_matter(carved):
    pts, col, o = P.sphere_scans(carved)[0]
    perm = np.random.default_rng(3).permutation(len(pts))
    kw = dict(space_carving=carved, max_range=P.CARVE_RANGE if carved else np.inf)
    a, b = P.Volume(R.VOXEL, R.TRUNC), P.Volume(R.VOXEL, R.TRUNC)
    a.integrate_points(pts, o, col, **kw)
    b.integrate_points(pts[perm], o, col[perm], **kw)
    assert a.coords == b.coords
    assert np.array_equal(a.tsdf, b.tsdf) and np.array_equal(a.weight, b.weight) and np.array_equal(a.color, b.color)


def test_invalid_points_and_arguments():
    vol = P.Volume(1.0, 2.0, color=False)
    pts = np.array([[5.25, 0.125, -0.25], [np.nan, 0, 0], [np.inf, 0, 0], [0.75, 0.125, -0.25], [30.25, 0.125, -0.25]])
    vol.integrate_points(pts, (0.25, 0.125, -0.25), sdf_mode="ray", min_range=1.0, max_range=20.0)
    assert vol.weight.sum() == 5
    with pytest.raises(ValueError):
        vol.integrate_points(pts, (0.25, 0.125, -0.25), space_carving=True)
