"""Class-2 blend backward (blend_bwd_tile_kernel<MODE>): the swap-first row reduction (wave_reduce16_swap), its lane ->
slot map and store predicate, and the record loop unrolled by two, on the smallest scenes at which they can go wrong.
Every case forces the class-2 kernels the way test_blend_class2.py does and is run twice (bitwise reproducible).

One-hot cases: the upstream gradient is non-zero in ONE pixel (one lane, one of its four pixels) or ONE channel, so a
swapped operand order, a wrong row pairing, a wrong store predicate or two slots mixed drops, doubles or moves exactly
that contribution.  The gate is test_raster.py's, without the allowance for flipped decisions; the seeds below were
chosen on the CPU so that the fp32 oracle itself is within 1e-4 of the fp64 oracle on every case (the bound is then
1e-4 of each tensor's largest entry)."""
import functools

import pytest
import torch

from scenes import make_scene
from test_blend_class2 import _grads
from test_raster import _assert_grad_gate, _oracle, _oracle_grads

ONE_TILE_SEED = {"surfel": 3, "3dgs": 3}   # see the module docstring
PARTIAL_SEED = {"surfel": 5, "3dgs": 5}
BATCH_SEED = 7


def _facing(sc, seed, tilt=0.2):
    """Surfels turned towards the camera (make_scene's are randomly oriented, some edge-on: they cover nothing)."""
    g = torch.Generator().manual_seed(seed + 500)
    q = tilt * (torch.rand(sc["rot"].shape[0], 4, generator=g, dtype=torch.float64) - 0.5)
    q[:, 1] = 1.0   # half a turn about x: the normal points back at the camera (front_only keeps those)
    sc["rot"] = torch.nn.functional.normalize(q, dim=1)
    return sc


@functools.lru_cache(maxsize=None)
def _big_scene(mode, seed, P=3, W=16, H=16):
    """A few Gaussians, each much larger than the image."""
    sc = make_scene(P, W, H, seed=seed, zmin=2.0, zmax=4.0, smin=2.0, smax=4.0, surfel=(mode == "surfel"), behind_frac=0.0)
    sc["op"] = 0.3 + 0.4 * sc["op"]
    return _facing(sc, seed)


@functools.lru_cache(maxsize=None)
def _faint_scene(mode, P, seed=BATCH_SEED):
    """P faint Gaussians larger than the one tile: no pixel saturates, so n_contrib reaches P and the list is walked to
    its end.  Every eighth and (P > 64) the last of the first batch of 64 are dead instances: their opacity is 1e-5
    above the 1/255 floor, which keeps them in the tile's list, while alpha reaches 1/255 only within 0.005 sigma of the
    centre, where no pixel centre lies."""
    sc = make_scene(3 * P + 60, 16, 16, seed=seed, zmin=2.0, zmax=4.0, smin=2.0, smax=4.0, surfel=(mode == "surfel"), behind_frac=0.0)
    sc = _facing(sc, seed)
    sc["op"] = 0.01 + 0.03 * sc["op"]
    # P of the candidates in the tile's list, in list order (Gaussian index == position in the list); a dead position
    # takes the next candidate whose centre is inside the tile (it stays in the list) and 0.25 px from every pixel centre
    o = _oracle(sc, torch.float32, mode, True)[0]
    ids = torch.as_tensor(o["point_list"][int(o["ranges"][0, 0]):int(o["ranges"][0, 1])]).long()
    mx, my = o["geom"]["mx"].detach().double(), o["geom"]["my"].detach().double()
    off = torch.maximum((mx - mx.round()).abs(), (my - my.round()).abs())
    central = (mx > 1) & (mx < 14) & (my > 1) & (my < 14) & (off > 0.25)
    is_dead = lambda r: r % 8 == 5 or (r == 63 and P > 64)
    keep = []
    for i in ids.tolist():
        if len(keep) < P and (central[i] or not is_dead(len(keep))):
            keep.append(i)
    assert len(keep) == P
    for k in ["means", "scales", "rot", "op", "col"]:
        sc[k] = sc[k][keep].clone()
    sc["op"][[r for r in range(P) if is_dead(r)]] = (1.0 + 1e-5) / 255.0
    return sc


def _ups_grads(sc, dt, mode, ups):
    """_oracle_grads with given upstream gradients."""
    o, leaves, theta, rho = _oracle(sc, dt, mode, True, grads=True)
    gc, gn, gd, ga = ups
    loss = (o["color"] * gc.to(dt)).sum() + (o["depth"] * gd.to(dt)).sum() + (o["alpha"] * ga.to(dt)).sum()
    if mode == "surfel":
        loss = loss + (o["normal"] * gn.to(dt)).sum()
    return list(leaves) + ["theta", "rho"], torch.autograd.grad(loss, list(leaves.values()) + [theta, rho])


def _tile_twice(sc, mode, ups, monkeypatch):
    a = _grads(sc, mode, ups, "tile", monkeypatch)
    b = _grads(sc, mode, ups, "tile", monkeypatch)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), i
    return a


def _assert_close_to_scan(names, tile, scan):
    for name, a, c in zip(names, tile, scan):
        scale = max(c.abs().max().item(), 1e-30)
        assert (a - c).abs().max().item() <= 1e-4 * scale, (name, (a - c).abs().max().item() / scale)


def one_hot_mask(lane, h, r, W=16, H=16):
    m = torch.zeros(H, W, dtype=torch.bool)
    m[8 * r + (lane >> 3), 8 * h + (lane & 7)] = True
    return m


LANES = [0, 1, 2, 3, 4, 8, 16, 32, 63]


@pytest.mark.gpu
@pytest.mark.parametrize("h,r", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("lane", LANES)
@pytest.mark.parametrize("mode", ["surfel", "3dgs"])
def test_one_hot_pixel(mode, lane, h, r, monkeypatch):
    sc = _big_scene(mode, ONE_TILE_SEED[mode])
    m = one_hot_mask(lane, h, r)
    _, names, ref64, ups = _oracle_grads(sc, torch.float64, mode, True, pix_mask=m)
    _, _, ref32, _ = _oracle_grads(sc, torch.float32, mode, True, pix_mask=m)
    tile = _tile_twice(sc, mode, ups, monkeypatch)
    _assert_grad_gate(names, tile, ref64, ref32, f"one-hot pixel {mode} lane={lane} h={h} r={r}", flips_allowed=False)


def _channel_ups(which, W=16, H=16, seed=11):
    g = torch.Generator().manual_seed(seed)
    f64 = torch.float64
    gc, gn = torch.zeros(3, H, W, dtype=f64), torch.zeros(3, H, W, dtype=f64)
    gd, ga = torch.zeros(1, H, W, dtype=f64), torch.zeros(1, H, W, dtype=f64)
    if which == "colour0":
        gc[0] = torch.randn(H, W, generator=g, dtype=f64)
    else:
        gd[0] = torch.randn(H, W, generator=g, dtype=f64)
    return gc, gn, gd, ga


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["colour0", "depth"])
@pytest.mark.parametrize("mode", ["surfel", "3dgs"])
def test_one_hot_channel(mode, which, monkeypatch):
    """Dense in pixels, upstream gradient in colour channel 0 only (the other colour gradients are exactly zero: slots
    do not mix) or in the depth only (the depth slots against the oracle)."""
    sc = _big_scene(mode, ONE_TILE_SEED[mode])
    ups = _channel_ups(which)
    names, ref64 = _ups_grads(sc, torch.float64, mode, ups)
    _, ref32 = _ups_grads(sc, torch.float32, mode, ups)
    tile = _tile_twice(sc, mode, ups, monkeypatch)
    if which == "colour0":
        d_col = tile[names.index("col")]
        assert bool((d_col[:, 0] != 0).any()) and bool((d_col[:, 1:] == 0).all())
    _assert_grad_gate(names, tile, ref64, ref32, f"one-hot channel {mode} {which}", flips_allowed=False)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["surfel", "3dgs"])
def test_partial_tiles(mode, monkeypatch):
    """24x20: the tiles are cut in x and in y."""
    sc = _big_scene(mode, PARTIAL_SEED[mode], P=6, W=24, H=20)
    _, names, ref64, ups = _oracle_grads(sc, torch.float64, mode, True)
    _, _, ref32, _ = _oracle_grads(sc, torch.float32, mode, True)
    tile = _tile_twice(sc, mode, ups, monkeypatch)
    _assert_grad_gate(names, tile, ref64, ref32, f"partial tiles {mode}", flips_allowed=False)
    _assert_close_to_scan(names, tile, _grads(sc, mode, ups, "scan", monkeypatch))


@pytest.mark.gpu
@pytest.mark.parametrize("P", [63, 64, 65, 129])
@pytest.mark.parametrize("mode", ["surfel", "3dgs"])
def test_batch_edges(mode, P, monkeypatch):
    """Lists of 63, 64, 65 and 129 records: a batch short by one, full, one record in the second batch, one in the
    third; an odd and an even number of live records for the loop unrolled by two; dead instances inside and at the end
    of a batch."""
    sc = _faint_scene(mode, P)
    _, names, ref64, ups = _oracle_grads(sc, torch.float64, mode, True)
    _, _, ref32, _ = _oracle_grads(sc, torch.float32, mode, True)
    tile = _tile_twice(sc, mode, ups, monkeypatch)
    _assert_grad_gate(names, tile, ref64, ref32, f"batch edges {mode} P={P}", flips_allowed=False)
    _assert_close_to_scan(names, tile, _grads(sc, mode, ups, "scan", monkeypatch))
