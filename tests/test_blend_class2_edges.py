"""Footprint class 2 blend kernels on images that are NOT a whole number of 16x16 tiles.  The class-2 kernels give each
lane four pixels and compute a row's two pixels (x halves 8 apart) as one packed pair, so in the last tile column /
row a pair can hold one pixel inside the image and one outside it: the outside pixel must stay inert component-wise
(no blend, no gradient, transmittance untouched) while its partner blends.  150 x 100 leaves 6 / 4 pixels in the last
tile (only the left half of a pair inside); 156 x 108 leaves 12 / 12 (left half inside, right half partly).  Same three
properties as test_blend_class2.py: tile forward bit-identical to the wave-per-quadrant forward, class-2 backward within
1e-4 of the scan backward and under the fp64 oracle gate, bitwise reproducible."""
import pytest
import torch

from test_blend_class2 import _edge_scene, _forward_outputs, _grads
from test_raster import _assert_grad_gate, _oracle_grads

CASES = [("surfel", 61, 150, 100), ("3dgs", 62, 150, 100), ("surfel", 63, 156, 108), ("3dgs", 64, 156, 108)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode,seed,W,H", CASES)
def test_partial_tile_forward_bit_identical(mode, seed, W, H, monkeypatch):
    sc = _edge_scene(mode, seed, W=W, H=H)
    a = _forward_outputs(sc, mode, "4", monkeypatch)
    b = _forward_outputs(sc, mode, "-1", monkeypatch)
    nc = a["n_contrib"].reshape(H, W)
    # blending reaches into the partial last tile column and row
    assert int(nc[:, W - W % 16:].max()) > 0 and int(nc[H - H % 16:, :].max()) > 0
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("mode,seed,W,H", CASES)
def test_partial_tile_backward_matches_scan_and_oracle(mode, seed, W, H, monkeypatch):
    sc = _edge_scene(mode, seed, W=W, H=H)
    _, names, ref64, ups = _oracle_grads(sc, torch.float64, mode, True)
    _, _, ref32, _ = _oracle_grads(sc, torch.float32, mode, True)
    tile = _grads(sc, mode, ups, "tile", monkeypatch)
    again = _grads(sc, mode, ups, "tile", monkeypatch)
    scan = _grads(sc, mode, ups, "scan", monkeypatch)
    for name, a, b, c in zip(names, tile, again, scan):
        assert torch.equal(a, b), name
        scale = max(c.abs().max().item(), 1e-30)
        assert (a - c).abs().max().item() <= 1e-4 * scale, (name, (a - c).abs().max().item() / scale)
    _assert_grad_gate(names, tile, ref64, ref32, f"class-2 partial tiles {mode} {W}x{H} seed={seed}", flips_allowed=True)
