"""The front-fine rank buckets of the occlusion bound (csrc/raster_common.hpp: rank_bucket) on whole frames, against
the bound switched off: the wall scenes of tests/test_occl_buckets.py at gx = 65 (1040 x 16, tile rows across a word
edge of the masks), once with 1,500 + 8,000 Gaussians — 9,500 survivors: log-linear buckets for the first 1,024 ranks,
where every saturating tile stops — and once with 1,500 + 40,000, where the front part ends at rank 4,096 and the
tiles that never saturate keep ranks far into the equally dealt part behind it.

Every output and gradient is bit-equal to PINGS_RASTER_OCCLUSION=0 except `contributions` (the same non-zero terms in
another association: rtol 1e-5, atol 1e-7), every kept list is a prefix of the oracle's that holds all a pixel blended,
and instances are dropped but not all of them."""
import functools

import numpy as np
import pytest
import torch

from oracle import raster_cpu as R
from scenes import oracle_settings
from test_occl_buckets import N_WALL, SIZES, _run, _same_outputs, _wall_scene
from test_raster import _check_list_prefixes
from test_rank_buckets import front, restated

GX, NB = 65, 256
WALLS = {"full": (0.0, 1.0), "left_half": (0.0, 0.45)}


@functools.lru_cache(maxsize=None)
def _reference(surfel, n_small, wall):
    """Scene, oracle geometry and the oracle's full lists, once per scene (never modified)."""
    W, H = SIZES[GX]
    sc = _wall_scene(W, H, surfel, N_WALL, n_small, WALLS[wall])
    so = oracle_settings(sc, torch.float32, "surfel" if surfel else "3dgs", False)
    f = lambda k: sc[k].to(torch.float32)
    geom = R.preprocess(f("means"), f("scales"), f("rot"), so, opacities=f("op"))
    pl, rg = R.bin_and_sort(geom, so)
    return sc, geom, pl, rg


def _ranks(geom):
    """Depth rank of every Gaussian in the (depth, index) order of the depth sort, -1 for a culled one."""
    valid = geom["valid"].numpy()
    idx = np.nonzero(valid)[0]
    depth = geom["pz"].detach().to(torch.float32).numpy()[idx]
    order = idx[np.lexsort((idx, depth))]
    rank = np.full(valid.shape[0], -1, dtype=np.int64)
    rank[order] = np.arange(len(order))
    return rank, len(order)


@pytest.mark.gpu
@pytest.mark.parametrize("wall", list(WALLS))
@pytest.mark.parametrize("n_small", [8000, 40000])
@pytest.mark.parametrize("mode", ["surfel", "3dgs"])
def test_front_fine_buckets_change_no_output_bit(mode, n_small, wall, monkeypatch):
    W, H = SIZES[GX]
    assert (W + 15) // 16 == GX
    sc, geom, pl, rg = _reference(mode == "surfel", n_small, wall)
    off = _run(sc, mode, monkeypatch, {"PINGS_RASTER_OCCLUSION": "0"})
    on = _run(sc, mode, monkeypatch, {})
    assert off["I"] == int(geom["tiles_touched"].sum()) == len(pl)
    assert np.array_equal(off["pl"].cpu().numpy(), pl) and np.array_equal(off["rg"].cpu().numpy(), rg)
    _same_outputs(on, off, exact_contributions=False)
    _check_list_prefixes(on["pl"], on["rg"], on["nc"], dict(point_list=pl, ranges=rg), W, H)
    assert on["I"] == len(on["pl"]) and 0 < on["I"] < off["I"]

    # where the kept ranks lie in the bucket map, and that every tile keeps whole buckets: its last kept instance is
    # the last of its full list in that rank bucket
    rank, nvalid = _ranks(geom)
    fr, fb = front(NB, nvalid)
    assert (fr, fb) == ((1024, 48) if n_small == 8000 else (4096, 80))
    kept = rank[on["pl"].cpu().numpy()]
    assert bool((kept >= 0).all())
    last_kept = np.array([kept[a:b].max() if b > a else -1 for a, b in on["rg"].cpu().numpy()])
    print(f"{mode} {n_small} {wall}: survivors {nvalid}, instances {on['I']} of {off['I']}, last kept rank "
          f"{last_kept.max()}, front part {fr} ranks / {fb} buckets")
    for t, (a, b) in enumerate(rg):
        n = int(on["rg"][t, 1] - on["rg"][t, 0])
        if 0 < n < b - a:
            r_last, r_next = rank[pl[a + n - 1]], rank[pl[a + n]]
            assert restated([r_last], NB, nvalid)[0] < restated([r_next], NB, nvalid)[0], (t, r_last, r_next)
    # a saturating tile stops inside the wall (the nearest N_WALL ranks) or in the bucket that holds the wall's end
    eq = (nvalid - 1) // NB + 1
    if wall == "full":
        assert last_kept.max() < N_WALL + 2 * eq
    else:
        cols = last_kept.reshape(-1, GX)
        assert cols[:, 0].max() < N_WALL + 2 * eq
        assert cols[:, GX - 1].max() >= max(fr, nvalid // 2)     # an open tile keeps ranks of the equally dealt part
