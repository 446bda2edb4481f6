"""The rank-bucket map of the occlusion bound (csrc/raster_common.hpp: rank_bucket), on the host: the map restated
here in Python integers, compared with the library's own function (pings_raster_rank_bucket, which runs the function
the kernels call) for every rank, and the properties the bound and its cost rest on:

  * integer arithmetic only, a function of (r, nb, nvalid) alone;
  * non-decreasing in r, b(0) = 0, b < nb — a monotone partition of the ranks is all the bound needs;
  * in the front part a bucket that starts at rank r is at most max(w0, r / s) ranks wide;
  * no bucket is wider than twice the equal share ceil(nvalid / nb) the earlier map gave every bucket, and no front
    bucket wider than one share.

No GPU: the export is a host loop."""
import ctypes as C

import numpy as np
import pytest

from pings_amd import _lib

LW, LS = 4, 4                       # log2 w0, log2 s (RB_LW, RB_LS)
W0, S = 1 << LW, 1 << LS
NBS = (32, 64, 256)


def front(nb, nvalid):
    """(ranks, buckets) of the front part."""
    if nvalid == 0:
        return 0, 0
    eq = (nvalid - 1) // nb + 1
    J = 0
    if eq >> LW:
        J = min((eq >> LW).bit_length() - 1 + 2, nb >> (LS + 1))
    return (1 << (LW + LS + J - 1) if J else 0), J << LS


def restated(r, nb, nvalid):
    """rank_bucket for an int64 array of ranks 0 <= r < nvalid (Python / numpy integers, no float)."""
    fr, fb = front(nb, nvalid)
    r = np.asarray(r, dtype=np.int64)
    q = r >> LW
    # floor(log2 q) by counting the shifts that leave something: exact, unlike a float log
    e = np.zeros_like(q)
    for sh in range(1, 40):
        e += (q >> sh) != 0
    k = np.maximum(e - LS, 0)
    b_front = np.where(q < S, q, (k << LS) + (q >> k))
    b_behind = fb + (np.maximum(r - fr, 0) * (nb - fb)) // max(nvalid - fr, 1)
    return np.where(r < fr, b_front, np.minimum(b_behind, nb - 1))


def exported(r, nb, nvalid):
    L = _lib.lib()
    r32 = np.ascontiguousarray(r, dtype=np.int32)
    out = np.empty(len(r32), dtype=np.uint32)
    st = L.pings_raster_rank_bucket(r32.ctypes.data_as(C.c_void_p), len(r32), nb, nvalid, out.ctypes.data_as(C.c_void_p))
    _lib.check(st, "pings_raster_rank_bucket")
    return out.astype(np.int64)


def nvalids(nb):
    """0, 1, around w0; around the first rank of the equal part for every number of front sections this nb allows and
    around the survivor counts at which a section is added; the issue's three frame sizes."""
    out = {0, 1, W0 - 1, W0, W0 + 1, 9_500, 332_253, 1 << 24}
    for J in range(1, (nb >> (LS + 1)) + 1):
        fr = 1 << (LW + LS + J - 1)
        out |= {fr - 1, fr, fr + 1}
        width = W0 << max(J - 1, 0)                    # section J - 1 comes in when ceil(nvalid / nb) reaches its width
        out |= {(width - 1) * nb, (width - 1) * nb + 1, (width - 1) * nb + 2}
    return sorted(out)


def ranks_for(nb, nvalid):
    if nvalid <= 1_000_000:
        return np.arange(nvalid, dtype=np.int64)
    # a dense band around every bucket edge of the restated map (edges found by bisection on the monotone map), the
    # front part in full, and both ends
    fr, _ = front(nb, nvalid)
    edges = []
    for b in range(1, nb):
        lo, hi = 0, nvalid - 1              # first rank with bucket >= b
        while lo < hi:
            mid = (lo + hi) // 2
            if int(restated([mid], nb, nvalid)[0]) >= b:
                hi = mid
            else:
                lo = mid + 1
        edges.append(lo)
    band = np.arange(-300, 301, dtype=np.int64)
    r = np.concatenate([np.arange(min(fr + 4096, nvalid), dtype=np.int64)] + [e + band for e in edges] +
                       [np.arange(nvalid - 4096, nvalid, dtype=np.int64)])
    return np.unique(r[(r >= 0) & (r < nvalid)])


@pytest.mark.parametrize("nb", NBS)
def test_rank_bucket_matches_its_restatement_and_keeps_its_properties(nb):
    for nvalid in nvalids(nb):
        if nvalid == 0:
            assert exported([0, 5, -1], nb, 0).tolist() == [0, 0, 0]
            continue
        r = ranks_for(nb, nvalid)
        b = exported(r, nb, nvalid)
        want = restated(r, nb, nvalid)
        assert np.array_equal(b, want), (nb, nvalid, r[np.nonzero(b != want)[0][:5]])
        # b(0) = 0, b < nb, non-decreasing
        assert b[0] == 0 and int(b.max()) < nb and bool((np.diff(b) >= 0).all()), (nb, nvalid)
        if len(r) != nvalid:
            continue
        # widths, where every rank was evaluated: first rank and population of every bucket in use
        eq = (nvalid - 1) // nb + 1
        fr, fb = front(nb, nvalid)
        used, first, width = np.unique(b, return_index=True, return_counts=True)
        assert int(width.max()) <= 2 * eq, (nb, nvalid, int(width.max()), eq)
        in_front = first < fr
        assert bool((used[in_front] < fb).all()) and bool((used[~in_front] >= fb).all())
        assert bool((width[in_front] <= np.maximum(W0, first[in_front] // S)).all()), (nb, nvalid)
        assert bool((width[in_front] <= max(eq, 1)).all()), (nb, nvalid)
        assert fb <= nb // 2 and (fr == 0 or fr < nvalid)
    # depends on (r, nb, nvalid) alone: a second call, the ranks in another order
    r = np.arange(9_500, dtype=np.int64)[::-1]
    assert np.array_equal(exported(r, nb, 9_500), exported(r[::-1], nb, 9_500)[::-1])


@pytest.mark.parametrize("nb", NBS)
def test_widths_at_two_to_the_24_survivors(nb):
    """2^24 survivors: every bucket's first and last rank by bisection on the exported map."""
    nvalid = 1 << 24
    eq = (nvalid - 1) // nb + 1
    fr, fb = front(nb, nvalid)
    one = lambda x: int(exported([x], nb, nvalid)[0])
    starts = []
    for b in range(nb + 1):
        lo, hi = 0, nvalid                  # first rank with bucket >= b (nvalid if none)
        while lo < hi:
            mid = (lo + hi) // 2
            if one(mid) >= b:
                hi = mid
            else:
                lo = mid + 1
        starts.append(lo)
    assert starts[0] == 0 and starts[nb] == nvalid and one(nvalid - 1) == nb - 1
    for b in range(nb):
        w = starts[b + 1] - starts[b]
        assert 0 < w <= 2 * eq, (b, w)
        if starts[b] < fr:
            assert b < fb and w <= max(W0, starts[b] // S) and w <= eq, (b, w)


def test_ranks_outside_the_survivors():
    """A negative rank (a lane without one) gets bucket 0, a rank from nvalid on (a culled Gaussian) the last bucket."""
    assert exported([-1, -7], 256, 1000).tolist() == [0, 0]
    assert exported([1000, 1001, 2_000_000], 256, 1000).tolist() == [255, 255, 255]
    L = _lib.lib()
    assert L.pings_raster_rank_bucket(None, 3, 256, 10, None) == 1 and b"null" in L.pings_last_error()
