"""The fused colour query (`pings_color_forward`, pings_amd/csrc/knn_color.hip; `neural_points.color_fused`) against
the fp64 restatement of tests/tracking_colour_ref.py on the map of tests/golden/tracking_colour_photo.npz.

Seeded colour decoders (nn.Linear's default init) over C in {1, 3}, H in {24, 32, 64}, Fc = 8 (the fixture's table) and
16 (a random table), k in {6, 8}, both `weighted_first` values, `after_pgo` off and on (random unit quaternions), with
and without the Jacobian, at B in {1, 63, 257, 32,769}: 32,769 is one more than the 8,192 workgroups x 4 waves of the
grid cap, so one wave takes a second query.  The queries lie near the surface (0.5-voxel noise), 60 m away (no
neighbour) and 1.5 voxels outside a wall (fewer than k neighbours).

Gate: the project's parity gate, max |difference| <= 1e-4 max |reference| per array.  A Jacobian is
discontinuous where a hidden pre-activation changes sign; queries with a pre-activation within 16 * 2^-24 of its
magnitude sum are left out of the Jacobian comparison (their colour is still compared) and may be at most 0.5 % of B.
"""
import functools
from pathlib import Path
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import tracking_colour_ref as cref
import tracking_ref as ref

GOLDEN = Path(__file__).parent / "golden"
GATE = 1e-4

#        C   H  Fc  k  weighted_first after_pgo jac    B
CASES = [(3, 64, 8, 6, False, False, True, 32769),
         (3, 32, 8, 6, False, False, True, 257),
         (1, 24, 8, 6, False, False, True, 63),
         (3, 24, 16, 8, False, True, True, 257),
         (1, 32, 16, 8, False, True, True, 63),
         (1, 64, 16, 6, True, True, True, 257),
         (3, 32, 8, 8, True, False, True, 257),
         (3, 64, 8, 6, True, False, True, 1),
         (1, 32, 8, 6, False, False, True, 1),
         (3, 64, 16, 8, False, True, False, 257),
         (1, 24, 8, 6, True, False, False, 63)]
IDS = ["C{}-H{}-F{}-k{}-{}-{}-{}-B{}".format(c, h, f, k, "wf" if wf else "pn", "pgo" if pgo else "id",
                                            "jac" if j else "nojac", b) for c, h, f, k, wf, pgo, j, b in CASES]


@functools.lru_cache(maxsize=None)
def _fixture():
    z = np.load(GOLDEN / "tracking_colour_photo.npz")
    return {k: z[k] for k in z.files}


def _dress(npm, Fc, k, wf, pgo, dtype):
    """The case's options on a map (CPU oracle or its device copy): the same seeded tables on both."""
    g = torch.Generator().manual_seed(1000 + Fc + k)
    dev = npm.neural_points.device
    npm.nn_k, npm.weighted_first, npm.after_pgo = k, wf, pgo
    if Fc != npm.local_color_features.shape[1]:
        rows, grows = npm.local_color_features.shape[0], npm.color_features.shape[0]
        npm.local_color_features = (0.3 * torch.randn(rows, Fc, generator=g)).to(dtype).to(dev)
        npm.color_features = (0.3 * torch.randn(grows, Fc, generator=g)).to(dtype).to(dev)
    if pgo:
        for name in ("local_point_orientations", "point_orientations"):
            q = torch.randn(getattr(npm, name).shape[0], 4, generator=g)
            setattr(npm, name, (q / q.norm(dim=1, keepdim=True)).to(dtype).to(dev))
    return npm


def _queries(st, B, seed):
    """Near the surface, 60 m away, 1.5 voxels outside the wall x = 0 (float32, CPU)."""
    g = torch.Generator().manual_seed(seed)
    pts, voxel = torch.as_tensor(st["neural_points"]), float(st["resolution"])
    x = pts[torch.randint(0, pts.shape[0], (B,), generator=g)] + torch.randn(B, 3, generator=g) * (0.5 * voxel)
    if B >= 63:
        far, wall = B // 10, B // 5      # about a fifth of the wall block finds 1-3 neighbours, the rest none
        x[B - far:] += 60.0
        lo = B - far - wall
        x[lo:B - far, 0] = -1.5 * voxel
        x[lo:B - far, 1:] = torch.rand(wall, 2, generator=g) * torch.tensor([6.0, 3.0])
    return x.float().contiguous()


@functools.lru_cache(maxsize=None)
def _reference(i):
    """(decoder state, queries, fp64 restatement) of case i: computed once, never modified."""
    C, H, Fc, k, wf, pgo, jac, B = CASES[i]
    st = _fixture()
    npm, _ = ref.cpu_map(st)
    _dress(npm, Fc, k, wf, pgo, torch.float64)
    dst = cref.random_decoder(Fc, H, C, seed=50 + i)
    x = _queries(st, B, seed=10 + i)      # a base at which every case's wall block has queries with 1-3 neighbours
    out = cref.colour_query(npm, cref.cpu_colour_decoder(dst), x.double(), want_jac=jac)
    return dst, x, out


class _ColourDec:
    """Duck-typed colour `Decoder` from a `cdec.*` state dict."""

    def __init__(self, st, device="cuda"):
        t = lambda k: torch.as_tensor(np.asarray(st["cdec." + k])).float().to(device)
        n = len([k for k in st if k.startswith("cdec.layers.") and k.endswith(".weight")])
        self.layers = [NS(weight=t(f"layers.{i}.weight"), bias=t(f"layers.{i}.bias")) for i in range(n)]
        self.lout = NS(weight=t("lout.weight"), bias=t("lout.bias"))
        self.use_leaky_relu = False

    def regress_color(self, f):
        h = f
        for l in self.layers:
            h = torch.relu(torch.nn.functional.linear(h, l.weight, l.bias))
        return torch.sigmoid(torch.nn.functional.linear(h, self.lout.weight, self.lout.bias))


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_queries_cover_the_neighbour_cases_and_stay_under_the_kink_cap(i):
    C, H, Fc, k, wf, pgo, jac, B = CASES[i]
    _, x, out = _reference(i)
    assert out.color.shape == (B, C) and (out.jac is None) == (not jac)
    if B >= 63:
        assert int((out.in_topk == 0).sum()) >= B // 10                     # no neighbour
        assert int(((out.in_topk > 0) & (out.in_topk < k)).sum()) >= 2      # fewer than k
        assert int((out.in_topk == k).sum()) >= B // 2
        none = out.in_topk == 0
        if jac:
            assert float(out.jac[none].abs().max()) == 0.0
        if not wf:
            assert float(out.color[none].abs().max()) == 0.0
    flagged = float(out.flagged.double().mean())
    print(f"\n[{IDS[i]}] undecidable ReLU: {int(out.flagged.sum())} of {B} ({100 * flagged:.3f} %)")
    assert flagged <= cref.KINK_CAP


def test_supported_shapes():
    from pings_amd import neural_points as hnp

    npm = NS(config=NS(layer_norm_on=False, query_nn_k=6))
    ok = _ColourDec(cref.random_decoder(8, 64, 3, 0), device="cpu")
    assert hnp.colour_fused_supported(npm, ok)
    assert not hnp.colour_fused_supported(npm, _ColourDec(cref.random_decoder(8, 64, 3, 0, levels=2), device="cpu"))
    assert not hnp.colour_fused_supported(npm, _ColourDec(cref.random_decoder(8, 65, 3, 0), device="cpu"))
    assert not hnp.colour_fused_supported(npm, _ColourDec(cref.random_decoder(8, 64, 4, 0), device="cpu"))
    assert not hnp.colour_fused_supported(npm, _ColourDec(cref.random_decoder(62, 64, 3, 0), device="cpu"))
    assert not hnp.colour_fused_supported(NS(config=NS(layer_norm_on=True, query_nn_k=6)), ok)
    ok.use_leaky_relu = True
    assert not hnp.colour_fused_supported(npm, ok)
    assert not hnp.colour_fused_supported(npm, None)


def test_argument_errors_are_status_codes():
    import ctypes as C

    from pings_amd import _abi, _lib

    L = _lib.lib()
    d = _abi.ColorDecoder(1, 1, 1, 1, 64, 8, 3, 0)
    call = lambda dec, B=4, k=6: L.pings_color_forward(C.byref(dec), 1, 10, 1, None, 0, 1, B, 1, k, 1, None, None)
    assert call(d, B=0) == 0                                   # nothing to do, nothing launched
    for bad in (_abi.ColorDecoder(1, 1, 1, 1, 65, 8, 3, 0), _abi.ColorDecoder(1, 1, 1, 1, 64, 62, 3, 0),
                _abi.ColorDecoder(1, 1, 1, 1, 64, 8, 4, 0), _abi.ColorDecoder(None, 1, 1, 1, 64, 8, 3, 0)):
        assert call(bad) == 1
    assert call(d, k=17) == 1
    assert L.pings_color_forward(C.byref(d), 1, 10, 1, None, 1, 1, 4, 1, 6, 1, None, None) == 1   # after_pgo, no quaternions
    assert L.pings_color_forward(C.byref(d), None, 10, 1, None, 0, 1, 4, 1, 6, 1, None, None) == 1


# ------------------------------------------------------------------ GPU
def _gate(got, want, keep=None):
    got, want = got.detach().cpu().double(), want.double()
    if keep is not None:
        got, want = got[keep], want[keep]
    return float((got - want).abs().max()), GATE * float(want.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_colour_query_matches_the_fp64_restatement(i):
    from pings_amd import neural_points as hnp
    from test_sdf import _gpu_map

    C, H, Fc, k, wf, pgo, jac, B = CASES[i]
    dst, x, want = _reference(i)
    gpu = _dress(_gpu_map(_fixture()), Fc, k, wf, pgo, torch.float32)
    gpu.config.query_nn_k, gpu.config.weighted_first = k, wf
    dec = _ColourDec(dst)
    xg = x.cuda()
    idx = hnp.radius_neighborhood_topk(gpu, xg, bool(gpu.temporal_local_map_on), True, True, True)[0]
    assert idx.shape == (B, k)
    col, J = hnp.color_fused(gpu, dec, xg, idx, need_jac=jac)
    assert col.shape == (B, C) and (J is None) == (not jac)
    assert torch.equal((idx >= 0).sum(dim=1).cpu(), want.in_topk)
    err, tol = _gate(col, want.color)
    print(f"\n[{IDS[i]}] colour {err:.3g} / {tol:.3g}")
    assert err <= tol
    if jac:
        keep = ~want.flagged
        assert float((~keep).double().mean()) <= cref.KINK_CAP
        assert J.shape == (B, C, 3)
        err, tol = _gate(J, want.jac, keep)
        print(f"[{IDS[i]}] jacobian {err:.3g} / {tol:.3g} ({int((~keep).sum())} undecidable left out)")
        assert err <= tol
        col2, none = hnp.color_fused(gpu, dec, xg, idx, need_jac=False)
        assert none is None and float((col2 - col).abs().max()) <= 1e-6     # the other instantiation, same colour


@pytest.mark.gpu
def test_neighbour_rows_of_the_search_and_of_the_sdf_launch_give_bit_equal_colours():
    from pings_amd import neural_points as hnp
    from test_sdf import _Dec, _gpu_map

    st = _fixture()
    gpu = _gpu_map(st)
    dec = _ColourDec({k: st[k] for k in st if k.startswith("cdec.")})
    x = _queries(st, 1025, seed=3).cuda()
    out = hnp.sdf_fused(gpu, _Dec(st), x, need_grad=True, use_only_valid_points=True, need_std=True, want_idx=True)
    assert len(out) == 6 and len(hnp.sdf_fused(gpu, _Dec(st), x, need_grad=True, need_std=True)) == 5
    idx_sdf = out[5]
    idx_knn = hnp.radius_neighborhood_topk(gpu, x, bool(gpu.temporal_local_map_on), True, True, True)[0]
    assert torch.equal(idx_sdf, idx_knn)
    a, b = hnp.color_fused(gpu, dec, x, idx_sdf), hnp.color_fused(gpu, dec, x, idx_knn)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert int((idx_sdf < 0).all(dim=1).sum()) >= 100 and float(a[0].abs().sum()) > 0
