"""tests/camfront_ref.py (the restatement of the camera frame front-end) against the reference's own results
(tests/golden/camfront_*.npz, tools/make_camfront_golden.py) and against torch on the CPU; the library's entries;
`camfront_ops.install` on stand-ins.

CPU only.  Gates: depth and sky levels are copies of pixels, so they are equal; a bilinear level on the CPU sums four
0.25-weighted terms serially where the restatement (and the device) forms 0.5 (0.5 a + 0.5 b) + 0.5 (0.5 c + 0.5 d), which
differs in the last bit, so RGB and normal levels are held to the project's 1e-4 relative gate.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import camfront_ref as CR
from conftest import GOLDEN, rel_err
from pings_amd import _abi, _lib, camfront_ops

NAMES = ("rgb", "depth", "sky", "normal")


def _golden():
    with np.load(GOLDEN / "camfront_cam.npz") as z:
        return {k: np.asarray(z[k]) for k in z.files}


# ================================================================ fixtures
@pytest.mark.parametrize("rate", [0, 1])
@pytest.mark.parametrize("exact", [True, False])
def test_constructor_lists_match_the_reference(rate, exact):
    z = _golden()
    for H, W, seed in z["sizes"]:
        u8, depth, sky, normal = CR.example(int(H), int(W), int(seed))
        lists, best = CR.cam_lists(CR.u8_level0(u8), depth, sky, normal, img_down_rate=rate, exact=exact)
        tag = f"{H}x{W}.r{rate}"
        assert best == int(z[f"{tag}.cur_best_level"]) == rate
        assert z[f"{tag}.flags"].all()
        for name, ls in zip(NAMES, lists):
            assert [lv is not None for lv in ls] == z[f"{tag}.{name}.present"].tolist() == [k >= rate for k in range(4)]
            for k, lv in enumerate(ls):
                if lv is None:
                    continue
                ref = z[f"{tag}.{name}.{k}"]
                assert lv.shape == ref.shape == ((3 if name in ("rgb", "normal") else 1), H >> k, W >> k)
                if name in ("depth", "sky"):
                    assert lv.dtype == ref.dtype and np.array_equal(lv, ref), (tag, name, k)
                else:
                    assert rel_err(torch.from_numpy(lv), torch.from_numpy(ref)) <= 1e-4, (tag, name, k)


@pytest.mark.parametrize("H,W", [(8, 8), (9, 15), (17, 23), (33, 70)])
def test_index_rules_are_those_of_interpolate(H, W):
    _, depth, sky, normal = CR.example(H, W, seed=H)
    d, s, n = torch.from_numpy(depth), torch.from_numpy(sky), torch.from_numpy(normal)
    rd, rs, rn = CR.nearest_exact_levels(depth), CR.nearest_levels(sky), CR.bilinear_levels(normal)
    for k in range(1, 4):
        d = F.interpolate(d.unsqueeze(0), scale_factor=0.5, mode="nearest-exact").squeeze(0)
        s = F.interpolate(s.float().unsqueeze(0), scale_factor=0.5, mode="nearest").squeeze(0).bool()
        n = F.interpolate(n.unsqueeze(0), scale_factor=0.5, mode="bilinear", align_corners=False).squeeze(0)
        assert np.array_equal(d.numpy(), rd[k]) and np.array_equal(s.numpy(), rs[k])
        assert rn[k].shape == tuple(n.shape) and np.abs(rn[k] - n.numpy()).max() <= 2.0 ** -23


def test_the_two_roundings_of_a_bilinear_level_differ_by_an_ulp_at_most():
    u8, _, _, _ = CR.example(33, 70, seed=5)
    a, b = CR.bilinear_levels(CR.u8_level0(u8), exact=True), CR.bilinear_levels(CR.u8_level0(u8), exact=False)
    for x, y in zip(a[1:], b[1:]):
        assert np.abs(x.astype(np.float64) - y).max() <= 2.0 ** -24          # values <= 1: one unit in the last place


def test_clamp_keeps_a_nan_and_the_uint8_division_is_ieee():
    v = np.array([-1.0, -0.0, 0.25, 1.0, 1.5, np.nan, np.inf, -np.inf], np.float32)
    got = CR.clamp01(v)
    assert np.array_equal(got, torch.from_numpy(v).clamp(0.0, 1.0).numpy(), equal_nan=True) and np.isnan(got[5])
    u = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, 2)
    l0 = CR.u8_level0(u)
    assert l0.shape == (3, 16, 16) and l0.dtype == np.float32
    assert np.array_equal(l0[0].reshape(-1), (np.arange(256) / 255.0).astype(np.float32))      # rounded once


# ================================================================ the library
def test_the_library_exports_the_entry_and_refuses_bad_tables():
    L = _lib.lib()
    assert hasattr(L, "pings_camfront_pyramid")
    made = C.c_int(7)
    assert L.pings_camfront_pyramid(None, 1, C.byref(made), None) == 1 and made.value == 0
    table = (_abi.CamfrontMap * 1)(_abi.CamfrontMap(None, None, None, None, None, 0, 16, 1, 16, 16, _abi.CAMFRONT_DEPTH, 0))
    assert L.pings_camfront_pyramid(table, 1, None, None) == 1 and b"null" in L.pings_last_error()
    assert L.pings_camfront_pyramid(table, 0, None, None) == 1
    assert L.pings_camfront_pyramid(table, _abi.CAMFRONT_MAX_MAPS + 1, None, None) == 1
    table[0].src = 4096                                           # never dereferenced: the kind is refused first
    table[0].kind = 5
    assert L.pings_camfront_pyramid(table, 1, None, None) == 1 and b"kind" in L.pings_last_error()
    table[0].kind, table[0].H = _abi.CAMFRONT_DEPTH, 0
    assert L.pings_camfront_pyramid(table, 1, None, None) == 1 and b"size" in L.pings_last_error()
    assert _abi.CAMFRONT_TILE_H % 8 == 0 and _abi.CAMFRONT_TILE_W % 8 == 0
    assert _abi.CAMFRONT_MAX_MAPS == 4 * _abi.LIDAR_MAX_CAMS


def test_the_mono_cloud_entries_are_exported_and_refuse_null_pointers():
    L = _lib.lib()
    for name in ("pings_camfront_align", "pings_camfront_mono_cloud", "pings_camfront_voxel_average",
                 "pings_camfront_align_scratch_bytes", "pings_camfront_cloud_scratch_bytes",
                 "pings_camfront_voxel_scratch_bytes"):
        assert hasattr(L, name), name
    assert L.pings_camfront_align(None, None, 16, 1.0, 10.0, None, None, None) == 1 and b"null" in L.pings_last_error()
    assert L.pings_camfront_align(4096, 4096, 0, 1.0, 10.0, 4096, 4096, None) == 1       # refused before any access
    assert L.pings_camfront_mono_cloud(None, None, 8, 8, None, None, None, 1.0, 10.0, 5.0, 0, None, None, None, None,
                                       None, None) == 1 and b"null" in L.pings_last_error()
    assert L.pings_camfront_voxel_average(None, 8, None, 0.5, None, None, 8, None, None, None, None) == 1
    assert b"null" in L.pings_last_error()
    assert L.pings_camfront_voxel_average(4096, 8, None, 0.5, 4096, 4096, 8, 8192, 8192, 4096, None) == 1
    assert b"different words" in L.pings_last_error()
    assert L.pings_camfront_voxel_average(4096, 8, None, 0.0, 4096, 4096, 8, None, 4096, 4096, None) == 1
    assert L.pings_camfront_align_scratch_bytes() >= 256 * 7 * 8
    assert L.pings_camfront_cloud_scratch_bytes(0) == 0 and L.pings_camfront_cloud_scratch_bytes(33 * 70) > 0
    assert L.pings_camfront_voxel_scratch_bytes(100) == L.pings_eval_voxel_scratch_bytes(100) > 0
    assert _abi.CAMFRONT_MIN_FIT == CR.MIN_FIT == 100


# ================================================================ the restatement of the mono-depth cloud
def test_normal_equations_agree_with_polyfit_on_the_fit_setup():
    pred, lidar = CR.fit_example()
    n, k, b, before, after = CR.align(pred, lidar, 2.75, 60.0)
    m = CR.fit_mask(pred, lidar, 2.75, 60.0)
    x, y = pred[m].astype(np.float64), lidar[m].astype(np.float64)
    mx, my = x.mean(), y.mean()
    k2 = ((x * y).sum() - n * mx * my) / ((x * x).sum() - n * mx * mx)
    b2 = my - k2 * mx
    assert n == m.sum() and 300 < n < 2 ** 12
    assert abs(k2 - k) <= 1e-11 * abs(k) and abs(b2 - b) <= 1e-10 * abs(b)
    assert abs(k - 1.07) < 0.01 and 0.4 < after < 0.6 < before
    assert (x * x).mean() / x.var() < 6.0                                     # the amplification the 1e-8 gate assumes
    for valid in (0, 100, 101):
        got = CR.align(*CR.fit_example(seed=1, valid=valid), 2.75, 60.0)
        assert got[0] == valid and ((got[1], got[2]) == (1.0, 0.0)) == (valid <= 100)


@pytest.mark.parametrize("high_z", [True, False])
@pytest.mark.parametrize("H,W", [(33, 70), (9, 15)])
def test_the_restatements_own_undecided_share_is_under_the_cap(H, W, high_z):
    lim = dict(min_range=2.75, max_range=60.0, depth_trunc=50.0)
    pred, u8, K = CR.cloud_example(H, W, seed=W, high_z=high_z, k=1.07, b=-0.6, **lim)
    rows, sky, gated, und = CR.mono_cloud(pred, u8, K, CR.rig_pose(H), high_z=high_z, k=1.07, b=-0.6, **lim)
    assert und.mean() <= 1e-3                                                # the cap of lidar_ops' crop test
    assert len(rows) == ((gated > 0) & (gated < 50.0)).sum() > 0
    assert sky.any() and not sky.all() and (gated[sky] == 0).all()
    pred, u8, K = CR.cloud_example(H, W, seed=W, high_z=high_z, k=1.07, b=-0.6, nudge=True, **lim)
    assert not CR.mono_cloud(pred, u8, K, np.eye(4), high_z=high_z, k=1.07, b=-0.6, **lim)[3].any()


def test_voxel_average_restatement():
    rows = np.array([[0.0, 0.0, 0.0, 0.0, 0.5, 1.0], [0.1, 0.1, 0.1, 1.0, 0.5, 0.0],       # one cell
                     [1.0, 0.0, 0.0, 0.2, 0.2, 0.2],                                       # x + 1
                     [0.0, 1.0, 0.0, 0.4, 0.4, 0.4]], np.float32)                          # y + 1: behind x + 1
    out = CR.voxel_average(rows, 1.0)
    assert out.shape == (3, 6)
    assert np.allclose(out[0], [0.05, 0.05, 0.05, 0.5, 0.5, 0.5]) and np.allclose(out[1], rows[2]) and np.allclose(out[2], rows[3])
    for n in (1, 63, 5000):
        r = CR.voxel_rows(n, 0.8, seed=n)
        assert r.shape == (n, 6) and r.dtype == np.float32 and CR.voxel_cells(r, 0.8)[1].min() >= 1e-3


# ================================================================ install and fallbacks
class _Cam:
    """Stand-in with the reference's constructor signature; records what it was called with."""

    def __init__(self, frame_id, rgb_image, K_mat, z_min=0.1, z_max=100.0, cam_id="cam", img_down_rate=0,
                 depth_image=None, normal_img=None, sky_mask=None, device="cuda", cam_pose=None, img_width=None,
                 img_height=None, pyramid_level=4):
        self.called = dict(rgb_image=rgb_image, img_width=img_width, img_height=img_height, depth_image=depth_image,
                           pyramid_level=pyramid_level, img_down_rate=img_down_rate)


def test_install_round_trip():
    orig = _Cam.__dict__["__init__"]
    camfront_ops.install(cam_cls=_Cam)
    camfront_ops.install(cam_cls=_Cam)
    assert _Cam.__dict__["__init__"] is camfront_ops.cam_init and _Cam._pings___init___original is orig
    camfront_ops.uninstall(cam_cls=_Cam)
    assert _Cam.__dict__["__init__"] is orig and "_pings___init___original" not in _Cam.__dict__
    camfront_ops.uninstall(cam_cls=_Cam)
    assert _Cam.__dict__["__init__"] is orig


def test_fallbacks_reach_the_original_constructor():
    K = np.eye(3)
    camfront_ops.install(cam_cls=_Cam)
    try:
        rgb = torch.rand(3, 16, 16)                                           # a CPU tensor
        cam = _Cam(1, rgb, K, device="cpu", depth_image=torch.ones(1, 16, 16))
        assert cam.called["rgb_image"] is rgb and cam.called["depth_image"] is not None
        assert _Cam(1, None, K, img_width=4, img_height=4).called["img_width"] == 4
        assert _Cam(1, rgb.double(), K).called["rgb_image"].dtype is torch.float64
        assert _Cam(1, rgb, K, pyramid_level=3).called["pyramid_level"] == 3
    finally:
        camfront_ops.uninstall(cam_cls=_Cam)


def test_without_a_kept_original_the_constructor_raises():
    class Bare:
        pass

    with pytest.raises(_lib.PingsHipError, match="original"):
        camfront_ops.cam_init(Bare(), 1, torch.rand(3, 16, 16), np.eye(3))
    with pytest.raises(_lib.PingsHipError, match="device tensor"):
        camfront_ops.image_pyramid(torch.rand(3, 16, 16))


# ================================================================ the mono-depth branch of process_frame
@pytest.mark.parametrize("tag", list(CR.MONO_CASES))
def test_mono_branch_restatement_matches_the_reference(tag):
    from oracle import map_cpu

    with np.load(GOLDEN / "camfront_mono_frame.npz") as z:
        z = {k: torch.from_numpy(z[k]) for k in z.files}
    high_z, _ = CR.MONO_CASES[tag]
    res = CR.MONO_CFG["monodepth_gaussian_res"]
    moved, rows = CR.mono_update(z[f"{tag}_mono"], z[f"{tag}_u_points"][:, 2], z[f"{tag}_pose"], high_z,
                                 CR.MONO_CFG["voxel_size_m"], lambda p: map_cpu.voxel_down_sample(p, res))
    after = z[f"{tag}_mono_after"]
    assert rel_err(moved[:, :3], after[:, :3]) <= 1e-4 and torch.equal(moved[:, 3:].float(), after[:, 3:])
    assert not torch.equal(z[f"{tag}_mono"][:, :3], after[:, :3])
    if tag == "none":
        assert rows.shape[0] == 0 and f"{tag}_m_points" not in z
    else:
        want = z[f"{tag}_m_points"]
        assert rows.shape[0] == want.shape[0] > 5                             # same count and order
        assert rel_err(rows[:, :3], want) <= 1e-4 and torch.equal(rows[:, 3:], z[f"{tag}_m_colors"])
