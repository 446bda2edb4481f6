"""The lean trip of the wave-per-tile blend backward for records interior to their tile (csrc/raster_common.hpp:
blend_interior; PINGS_BLEND_INTERIOR, default on).  The lean trip leaves out only decisions that are the same at all
256 pixel positions of the tile and sums that are exactly zero, so with the knob on and off every output and every
gradient must agree bit for bit; the on-run is held to the fp64 oracle by the gate test_blend_class2_edges.py uses, and
its forward to the wave-per-quadrant forward.  Scenes: randomly oriented surfels of every size (edge-on ones,
slanted ones whose ray hit leaves the depth range inside a tile, centres inside tiles, alpha contours that cut tiles,
opacities of 0.99, the next float, 0.999 and 1, opacities just above 1/255) mixed with large faint surfels that face the
camera, the interior class.  Images of 150x100 and 156x108 (partial last tiles) and 32x32 (two by two tiles)."""
import numpy as np
import pytest
import torch

from scenes import make_scene
from test_blend_class2 import _forward_outputs, _grads
from test_blend_interior_host import interior_flags
from test_raster import _assert_grad_gate, _oracle, _oracle_grads

SIZES = [(150, 100, 71), (156, 108, 72), (32, 32, 73)]


def interior_scene(mode, W, H, seed, n_random=150, n_large=110, n_opaque=12):
    P = n_random + n_large + n_opaque
    sc = make_scene(P, W, H, seed=seed, zmin=1.0, zmax=6.0, smin=0.05, smax=1.5, surfel=(mode == "surfel"),
                    behind_frac=0.05)
    g = torch.Generator().manual_seed(seed + 500)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    cam = sc["cam"]
    view = cam["viewmatrix"].double()          # row-vector convention: p_cam = [p_world, 1] @ view
    Rcw = view[:3, :3].T                       # world -> camera rotation
    fx = W / (2.0 * cam["tanfovx"])
    # the random part: a share nearly opaque (clamp active), a share barely above the opacity floor
    u = rnd(P)
    op = sc["op"].view(-1)
    op[:n_random][u[:n_random] < 0.15] = 0.999
    op[:n_random][(u[:n_random] >= 0.15) & (u[:n_random] < 0.25)] = 1.0 / 255.0 + 1e-6
    # the large part: footprints of 0.6 .. 1.5 image widths, facing the camera within ~15 degrees, faint
    a, b = n_random, n_random + n_large + n_opaque
    pc = torch.cat([sc["means"][a:b], torch.ones(b - a, 1, dtype=torch.float64)], 1) @ view
    z = pc[:, 2].abs().clamp(min=1.0)
    s = (0.6 + 0.9 * rnd(b - a)) * W / fx * z
    sc["scales"][a:b, 0] = s
    sc["scales"][a:b, 1] = s * (0.5 + 0.5 * rnd(b - a))
    if mode != "surfel":
        sc["scales"][a:b, 2] = 0.05
    # rotation: the camera's orientation in the world (the surfel's normal = the view direction) times a small tilt
    tilt = (rnd(b - a, 3) - 0.5) * 0.5
    q_tilt = torch.nn.functional.normalize(torch.cat([torch.ones(b - a, 1, dtype=torch.float64), 0.5 * tilt], 1), dim=1)
    # (turned half round about x first: the normal, the rotation's third column, has to point AT the camera)
    q_cam = _quat_mul(_quat_of(Rcw.T), torch.tensor([0.0, 1.0, 0.0, 0.0], dtype=torch.float64))
    sc["rot"][a:b] = _quat_mul(q_cam.expand(b - a, 4), q_tilt)
    op[a:a + n_large] = 0.05 + 0.2 * rnd(n_large)
    # the opaque part, large as well: opacity 0.99 as fp32 has it, the next fp32 above, 0.999 and 1
    o99 = float(np.float32(0.99))
    vals = [o99, float(np.nextafter(np.float32(0.99), np.float32(2.0))), 0.999, 1.0]
    op[a + n_large:b] = torch.tensor([vals[i % 4] for i in range(n_opaque)], dtype=torch.float64)
    return sc


def _quat_of(M):
    """(w, x, y, z) of a rotation matrix (trace form; the camera poses of make_scene are close to identity)."""
    w = torch.sqrt(torch.clamp(1.0 + M[0, 0] + M[1, 1] + M[2, 2], min=1e-12)) / 2.0
    return torch.stack([w, (M[2, 1] - M[1, 2]) / (4 * w), (M[0, 2] - M[2, 0]) / (4 * w), (M[1, 0] - M[0, 1]) / (4 * w)])


def _quat_mul(p, q):
    pw, px, py, pz = p.unbind(-1)
    qw, qx, qy, qz = q.unbind(-1)
    return torch.stack([pw * qw - px * qx - py * qy - pz * qz, pw * qx + px * qw + py * qz - pz * qy,
                        pw * qy - px * qz + py * qw + pz * qx, pw * qz + px * qy - py * qx + pz * qw], -1)


def class_counts(sc):
    """(interior, general) among the scene's live (record, tile) pairs: the oracle's fp32 preprocess and lists, a pair
    live when it stands before the tile's last blended list position and passes the alpha tests at some pixel of the
    tile; the class from the library's own classifier."""
    o, *_ = _oracle(sc, torch.float32, "surfel", True)
    g = o["geom"]
    f = lambda k: g[k].detach().numpy().astype(np.float32)
    W, H = sc["W"], sc["H"]
    gx, gy = (W + 15) // 16, (H + 15) // 16
    ncp = np.zeros((gy * 16, gx * 16), dtype=np.int64)
    ncp[:H, :W] = o["n_contrib"].numpy().reshape(H, W)
    need = ncp.reshape(gy, 16, gx, 16).transpose(0, 2, 1, 3).reshape(gy * gx, 256).max(1)
    pl, rg = o["point_list"], o["ranges"]
    mx, my, pz, cx, cy, cz = f("mx"), f("my"), f("pz"), f("conic_x"), f("conic_y"), f("conic_z")
    nx, ny, nz, q, zhi = f("nx"), f("ny"), f("nz"), f("q"), f("zhi")
    opac = sc["op"].view(-1).numpy().astype(np.float32)
    recs, orgs = [], []
    for t in range(gx * gy):
        ids = pl[rg[t, 0]:rg[t, 0] + need[t]]
        X0, Y0 = 16.0 * (t % gx), 16.0 * (t // gx)
        xs, ys = np.meshgrid(np.arange(X0, min(X0 + 16, W), dtype=np.float32), np.arange(Y0, min(Y0 + 16, H), dtype=np.float32))
        for i in ids:
            dx, dy = mx[i] - xs, my[i] - ys
            power = np.float32(-0.5) * (cx[i] * dx * dx + cz[i] * dy * dy) - cy[i] * dx * dy
            if not ((power <= 0) & (opac[i] * np.exp(power) >= np.float32(1.0 / 255.0))).any():
                continue
            recs.append([mx[i], my[i], opac[i], pz[i], cx[i], cy[i], cz[i], zhi[i] - pz[i], 0, 0, 0, q[i], nx[i], ny[i], nz[i], 0])
            orgs.append([X0, Y0])
    prcp = sc["cam"]["prcppoint"].float().numpy()
    cxp = np.float32(prcp[0]) * np.float32(W) - np.float32(0.5)
    cyp = np.float32(prcp[1]) * np.float32(H) - np.float32(0.5)
    fx = np.float32(W / (2.0 * sc["cam"]["tanfovx"]))
    fy = np.float32(H / (2.0 * sc["cam"]["tanfovy"]))
    flags = interior_flags(np.array(recs, dtype=np.float32), np.array(orgs, dtype=np.float32), cxp, cyp, fx, fy)
    return int(flags.sum()), int((~flags).sum())


@pytest.mark.parametrize("W,H,seed", SIZES)
def test_scene_holds_both_classes(W, H, seed):
    """No GPU: at least 50 live pairs of each class, so both bodies run in the GPU tests below."""
    n_int, n_gen = class_counts(interior_scene("surfel", W, H, seed))
    print(f"{W}x{H}: interior {n_int}, general {n_gen}")
    assert n_int >= 50 and n_gen >= 50


def _fwd(sc, mode, knob, monkeypatch, ppl="4"):
    monkeypatch.setenv("PINGS_BLEND_INTERIOR", knob)
    return _forward_outputs(sc, mode, ppl, monkeypatch)


def _bwd(sc, mode, ups, knob, monkeypatch):
    monkeypatch.setenv("PINGS_BLEND_INTERIOR", knob)
    return _grads(sc, mode, ups, "tile", monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,seed", SIZES)
def test_interior_body_changes_no_bit_and_meets_the_oracle(W, H, seed, monkeypatch):
    sc = interior_scene("surfel", W, H, seed)
    on = _fwd(sc, "surfel", "1", monkeypatch)
    off = _fwd(sc, "surfel", "0", monkeypatch)
    quad = _fwd(sc, "surfel", "1", monkeypatch, ppl="-1")
    assert int(on["n_contrib"].max()) > 0
    for k in on:
        assert torch.equal(on[k], off[k]), k
        assert torch.equal(on[k], quad[k]), k
    _, names, ref64, ups = _oracle_grads(sc, torch.float64, "surfel", True)
    _, _, ref32, _ = _oracle_grads(sc, torch.float32, "surfel", True)
    g_on = _bwd(sc, "surfel", ups, "1", monkeypatch)
    g_off = _bwd(sc, "surfel", ups, "0", monkeypatch)
    for name, a, b in zip(names, g_on, g_off):
        assert torch.equal(a, b), name
    _assert_grad_gate(names, g_on, ref64, ref32, f"interior body {W}x{H} seed={seed}", flips_allowed=True)


@pytest.mark.gpu
def test_knob_changes_no_bit_in_3dgs_mode(monkeypatch):
    W, H, seed = 150, 100, 74
    sc = interior_scene("3dgs", W, H, seed)
    on = _fwd(sc, "3dgs", "1", monkeypatch)
    off = _fwd(sc, "3dgs", "0", monkeypatch)
    for k in on:
        assert torch.equal(on[k], off[k]), k
    _, names, _, ups = _oracle_grads(sc, torch.float32, "3dgs", True)
    g_on = _bwd(sc, "3dgs", ups, "1", monkeypatch)
    g_off = _bwd(sc, "3dgs", ups, "0", monkeypatch)
    for name, a, b in zip(names, g_on, g_off):
        assert torch.equal(a, b), name
