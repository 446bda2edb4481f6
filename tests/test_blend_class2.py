"""Footprint class 2 blend kernels (wave per 16x16 tile, four pixels per lane: blend_fwd_tile_kernel and
blend_bwd_tile_kernel<MODE>) on large-footprint scenes that reach their edge cases: pixels past n_contrib, power > 0,
alpha just around 1/255, raw = opacity * G above the 0.99 clamp, and (surfel) per-pixel depths clamped on both
sides and rays near the grazing threshold."""
import pytest
import torch

from scenes import make_scene
from test_raster import _assert_grad_gate, _hip_forward, _hip_grads, _oracle_grads


def _edge_scene(mode, seed, P=260, W=144, H=96):
    """Large splats (many tiles each), a share of them nearly opaque (raw > 0.99 at the centre: clamp active), a
    share barely above the 1/255 opacity floor (alpha within rounding of ALPHA_MIN); make_scene's surfels are flat and
    randomly oriented, so some are seen edge-on (den near zero, depth clamp active on both bounds)."""
    sc = make_scene(P, W, H, seed=seed, zmin=1.0, zmax=6.0, smin=0.05, smax=0.9, surfel=(mode == "surfel"))
    g = torch.Generator().manual_seed(seed + 100)
    u = torch.rand(P, generator=g, dtype=torch.float64)
    op = sc["op"].clone()
    op_flat = op.view(-1)
    op_flat[u < 0.2] = 0.999
    op_flat[(u >= 0.2) & (u < 0.3)] = 1.0 / 255.0 + 1e-6
    sc["op"] = op
    return sc


def _forward_outputs(sc, mode, ppl, monkeypatch):
    monkeypatch.setenv("PINGS_BLEND_PPL", ppl)
    monkeypatch.setenv("PINGS_BLEND_SEG", "0")   # no list regrouped into parallel segments by the quadrant forward
    monkeypatch.setenv("PINGS_BLEND_BWD", "pixel")
    hr, prep, fs, radii, per_g = _hip_forward(sc, mode, True)
    pl, rg, fT, nc = hr.debug_lists(fs)
    out = {"color": fs.color, "depth": fs.depth, "alpha": fs.alpha, "final_T": fT, "n_contrib": nc}
    if mode == "surfel":
        out["normal"] = fs.normal
    return {k: v.detach().cpu().clone() for k, v in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("mode,seed", [("surfel", 41), ("surfel", 42), ("3dgs", 43)])
def test_tile_forward_bit_identical_to_quadrant_forward(mode, seed, monkeypatch):
    """The wave-per-tile and the wave-per-quadrant forward blend each pixel serially front to back with the same
    operations: every image plane, final_T and n_contrib must agree bit for bit."""
    sc = _edge_scene(mode, seed)
    a = _forward_outputs(sc, mode, "4", monkeypatch)
    b = _forward_outputs(sc, mode, "-1", monkeypatch)
    nc = a["n_contrib"]
    assert int(nc.max()) > 0 and bool((nc < nc.max()).any())   # the scene does reach pixels past n_contrib
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _grads(sc, mode, ups, bwd, monkeypatch):
    if bwd == "tile":
        monkeypatch.setenv("PINGS_BLEND_PPL", "4")
        monkeypatch.setenv("PINGS_BLEND_BWD", "pixel")
    else:
        monkeypatch.setenv("PINGS_BLEND_PPL", "0")
        monkeypatch.setenv("PINGS_BLEND_BWD", "scan")
    _, got, _ = _hip_grads(sc, mode, True, ups)
    return [g.detach().cpu().clone() for g in got]


@pytest.mark.gpu
@pytest.mark.parametrize("mode,seed", [("surfel", 41), ("surfel", 42), ("3dgs", 43)])
def test_tile_backward_matches_scan_backward_and_oracle(mode, seed, monkeypatch):
    """The class-2 backward against the Gaussian-per-lane scan backward (1e-4 of each tensor's largest entry) and
    against the fp64 oracle under the gate of test_raster.py; it is also bitwise reproducible run to run."""
    sc = _edge_scene(mode, seed)
    _, names, ref64, ups = _oracle_grads(sc, torch.float64, mode, True)
    _, _, ref32, _ = _oracle_grads(sc, torch.float32, mode, True)
    tile = _grads(sc, mode, ups, "tile", monkeypatch)
    again = _grads(sc, mode, ups, "tile", monkeypatch)
    scan = _grads(sc, mode, ups, "scan", monkeypatch)
    for name, a, b, c in zip(names, tile, again, scan):
        assert torch.equal(a, b), name
        scale = max(c.abs().max().item(), 1e-30)
        assert (a - c).abs().max().item() <= 1e-4 * scale, (name, (a - c).abs().max().item() / scale)
    _assert_grad_gate(names, tile, ref64, ref32, f"class-2 {mode} seed={seed}", flips_allowed=True)
