"""No entry point writes past the scratch size the library reports for it.

Three entry points size their scratch and place their fields through one carve function each (pings_spawn_plan,
pings_tsdf_assign, pings_eval_backproject).  Each is called here directly with `scratch_bytes + 4096` bytes whose last
4096 are 0xA5: the guard is allocated memory, so a field placed behind the reported size shows as a changed guard byte
and not as a fault.  The outputs are compared with the same call made through the Python wrapper, which allocates
exactly the reported size.  The counts lie either side of a 256-byte field boundary of the scratch's first field.
"""
import ctypes as C

import numpy as np
import pytest
import torch

COUNTS = (1, 63, 64, 65, 257)
GUARD = 4096
SENTINEL = 7.5


def _guarded(nbytes, dev):
    assert nbytes > 0
    buf = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=dev)
    buf[nbytes:] = 0xA5
    return buf


def _guard_intact(buf):
    return bool((buf[-GUARD:] == 0xA5).all())


# ---------------------------------------------------------------- spawn plan: one flag word per candidate Gaussian
@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
def test_spawn_plan_stays_inside_its_scratch(count):
    from pings_amd import _abi, _lib, spawn

    dev = torch.device("cuda")
    L = _lib.lib()
    n, k, sd = count, 1, 3
    g = torch.Generator().manual_seed(4100 + count)
    raw = lambda w, s=1.0: (s * torch.randn(n, w * k, generator=g)).to(dev)
    xyz, rot, scale, alpha, color = raw(3), raw(4), raw(sd, 0.8), raw(1), raw(3)
    pos, quat = raw(3, 10.0), torch.nn.functional.normalize(raw(4), dim=1)
    dist_ratio = (0.5 * torch.rand(n, 1, generator=g)).to(dev)
    prm = dict(n=n, k=k, scale_dim=sd, surfel=1, color_residual=0, alpha_filter_on=1, scale_filter_on=1,
               displacement_range=0.5, unit_scale=0.125, max_scale=0.375, scale_filter_thr=0.1875)

    p = _abi.SpawnParams(**prm)
    dest = torch.full((n * k,), -7, dtype=torch.int32, device=dev)
    cnt = torch.full((1,), -7, dtype=torch.int32, device=dev)
    scratch = _guarded(L.pings_spawn_plan_scratch_bytes(n * k), dev)
    _lib.check(L.pings_spawn_plan(C.byref(p), _lib.ptr(alpha), _lib.ptr(scale), _lib.ptr(dist_ratio), _lib.ptr(scratch),
                                  _lib.ptr(dest), _lib.ptr(cnt), _lib.stream_ptr(dev)), "pings_spawn_plan")
    assert _guard_intact(scratch)

    kw = {key: prm[key] for key in ("n", "k", "displacement_range", "unit_scale", "max_scale", "scale_filter_thr")}
    out = spawn.activate(xyz, rot, scale, alpha, color, pos, quat, None, dist_ratio, None, surfel=True,
                         color_residual=False, alpha_filter_on=True, scale_filter_on=True, **kw)
    kept = dest >= 0
    assert int(cnt.item()) == out.count == int(kept.sum())
    assert torch.equal(dest[kept].cpu(), torch.arange(out.count, dtype=torch.int32))
    assert torch.equal(out.alpha, out.alpha_all[kept])          # the wrapper kept the same candidates, in order


# ---------------------------------------------------------------- TSDF assign: one sorted key per new block
@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
def test_tsdf_assign_stays_inside_its_scratch(count):
    from pings_amd import _lib, tsdf_ops

    dev = torch.device("cuda:0")
    L = _lib.lib()
    # pixel u of a one-row image at depth 8 lands on x = 8 u + tx with the band of +-1 inside block (u, 0, 1): every
    # pixel makes exactly one new block
    g = torch.Generator().manual_seed(4200 + count)
    t = (1.5 + 5.0 * torch.rand(3, generator=g)).double()
    cam_to_world = torch.eye(4, dtype=torch.float64)
    cam_to_world[:3, 3] = t
    depth = torch.full((1, count), 8.0, device=dev)
    image = torch.rand(3, 1, count, generator=g).to(dev)
    K = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    vol = tsdf_ops.TSDFVolume(1.0, 1.0, color=True, device=dev, capacity_blocks=count + 3)
    vol.integrate(depth, K, np.linalg.inv(cam_to_world.numpy()), image, stride=1)
    assert vol.n_blocks == count

    # the same assign on the wrapper's table and new-key list, into fresh stores
    cap, vox = vol.capacity, vol._tsdf.shape[1]
    new_keys = vol._lists[1][:count].clone()
    tslots = torch.full_like(vol._tslots, -1)
    keys = torch.full((cap,), -7, dtype=torch.int64, device=dev)
    tsdf, weight = (torch.full((cap, vox), SENTINEL, device=dev) for _ in range(2))
    color = torch.full((cap, 3, vox), SENTINEL, device=dev)
    scratch = _guarded(L.pings_tsdf_assign_scratch_bytes(count), dev)
    _lib.check(L.pings_tsdf_assign(_lib.ptr(new_keys), count, 0, cap, _lib.ptr(scratch), _lib.ptr(vol._tkeys),
                                   _lib.ptr(tslots), vol._tkeys.shape[0], _lib.ptr(keys), _lib.ptr(tsdf),
                                   _lib.ptr(weight), _lib.ptr(color), _lib.stream_ptr(dev)), "pings_tsdf_assign")
    assert _guard_intact(scratch)
    assert torch.equal(keys[:count], vol._keys[:count]) and torch.equal(tslots, vol._tslots)
    assert torch.equal(keys[:count], new_keys.sort().values)
    # what assign leaves in the fields (the wrapper's update pass has written into its own since)
    assert (tsdf[:count] == 1.0).all() and (weight[:count] == 0.0).all() and (color[:count] == 0.0).all()
    for store in (tsdf, weight, color):
        assert (store[count:] == SENTINEL).all()
    assert (keys[count:] == -7).all()


# ---------------------------------------------------------------- backproject: one count word per 256 pixels
@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("per", (1, 256), ids=("pixels", "blocks"))
def test_eval_backproject_stays_inside_its_scratch(count, per):
    from pings_amd import _lib, eval_ops

    dev = torch.device("cuda")
    L = _lib.lib()
    H, W = 1, count * per                  # `count` pixels, or `count` workgroups of 256 pixels
    g = torch.Generator().manual_seed(4300 + count + per)
    depth = (6.0 * torch.rand(H, W, generator=g)).to(dev)       # about a third lies beyond depth_trunc
    rgb = torch.rand(3, H, W, generator=g).to(dev)
    Kc, trunc = (50.0, 60.0, 0.5 * W, 0.5), 4.0
    extrinsic = torch.eye(4, dtype=torch.float64)
    extrinsic[:3, 3] = torch.tensor([0.25, -0.5, 1.0], dtype=torch.float64)
    want_p, want_c = eval_ops.backproject_depth(depth, Kc, extrinsic.numpy(), trunc, rgb=rgb)

    T = np.linalg.inv(extrinsic.numpy())                       # as the wrapper forms it
    points = torch.full((H * W, 3), SENTINEL, device=dev)
    colors = torch.full((H * W, 3), SENTINEL, device=dev)
    n_out = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = _guarded(L.pings_eval_backproject_scratch_bytes(H * W), dev)
    k4 = (C.c_double * 4)(*Kc)
    t12 = (C.c_double * 12)(*T[:3].reshape(-1).tolist())
    _lib.check(L.pings_eval_backproject(_lib.ptr(depth), _lib.ptr(rgb), None, H, W, k4, t12, trunc, 0.0, 0,
                                        _lib.ptr(scratch), _lib.ptr(points), _lib.ptr(colors), _lib.ptr(n_out),
                                        _lib.stream_ptr(dev)), "pings_eval_backproject")
    assert _guard_intact(scratch)
    m = int(n_out.item())
    assert m == want_p.shape[0] == int(((depth > 0) & (depth < trunc)).sum())
    assert torch.equal(points[:m], want_p) and torch.equal(colors[:m], want_c)
    assert (points[m:] == SENTINEL).all() and (colors[m:] == SENTINEL).all()
