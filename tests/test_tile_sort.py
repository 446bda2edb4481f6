"""The rasteriser's tile sort (csrc/tile_sort.hip): a stable radix sort of (tile id, slot) pairs in one or two digit
passes of histogram, scan and scatter.  Its output is fully determined — stable order by the low `bits` bits of the key —
so every check here is exact equality: against torch.sort(stable=True) on the CPU through the direct entry
pings_raster_tile_sort, against the library sort (PINGS_TILE_SORT=l) through the public rasteriser, and against a
second run.  The rank rule of the scatter kernel (block, wave, round, lane) is also emulated on the host, without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

BLOCK, THREADS = 4096, 256      # TS_BLOCK, TS_THREADS of csrc/raster_common.hpp (the GPU tests read B from the library)


def _digits(bits):
    """(shift, width) of every pass"""
    if bits <= 8:
        return [(0, bits)]
    lo = (bits + 1) // 2
    return [(0, lo), (lo, bits - lo)]


def _patterns(n, bits, rng):
    """name -> keys[n] (int64, below 2^bits)"""
    top = (1 << bits) - 1
    lo = _digits(bits)[0][1]
    i = np.arange(n, dtype=np.int64)
    out = {
        "equal": np.full(n, top // 3, dtype=np.int64),
        "random": rng.integers(0, top + 1, n, dtype=np.int64),
        "descending": (n - 1 - i) & top,            # strictly descending up to 2^bits pairs, wrapping beyond
        "top_bins": np.full(n, top, dtype=np.int64),
        # the top bin of one digit, anything in the other
        "top_low_digit": (rng.integers(0, top + 1, n, dtype=np.int64) | ((1 << lo) - 1)) & top,
        "top_high_digit": (rng.integers(0, top + 1, n, dtype=np.int64) | (top & ~((1 << lo) - 1))) & top,
    }
    # what duplicate_kernel emits: rectangle after rectangle on a grid gx wide, each in row-major runs of consecutive ids
    ntiles = top + 1
    gx = max(1, int(round(np.sqrt(ntiles * 16 / 9))))
    gx = min(gx, ntiles)
    gy = max(1, ntiles // gx)
    keys = np.empty(n, dtype=np.int64)
    m = 0
    while m < n:
        w, h = int(rng.integers(1, min(gx, 9) + 1)), int(rng.integers(1, min(gy, 9) + 1))
        x0, y0 = int(rng.integers(0, gx - w + 1)), int(rng.integers(0, gy - h + 1))
        ids = ((y0 + np.arange(h))[:, None] * gx + x0 + np.arange(w)[None, :]).reshape(-1)
        take = min(n - m, ids.size)
        keys[m:m + take] = ids[:take]
        m += take
    assert n == 0 or keys.max() <= top
    out["rectangles"] = keys
    return out


def _stable_sort(keys, bits):
    """(sorted keys, source indices) by torch.sort(stable=True) over the low `bits` bits"""
    k = torch.from_numpy(keys & ((1 << bits) - 1))
    perm = torch.sort(k, stable=True).indices.numpy()
    return keys[perm], perm


# ---------------------------------------------------------------- the rank rule, on the host
def _emulate(keys, bits, block=BLOCK, waves=THREADS // 64):
    """The three launches of every pass, step for step: table[digit][block] of counts, its exclusive scan, and for
    every pair base[digit][block] + its rank by (wave, round, lane) among the block's pairs of the digit."""
    n = keys.size
    vals = np.arange(n, dtype=np.int64)
    per_wave = block // waves
    for shift, width in _digits(bits):
        nbins, nblk = 1 << width, (n + block - 1) // block
        d = (keys >> shift) & (nbins - 1)
        table = np.zeros((nbins, nblk), dtype=np.int64)
        for b in range(nblk):
            table[:, b] = np.bincount(d[b * block:(b + 1) * block], minlength=nbins)
        flat = table.reshape(-1)
        base = (np.cumsum(flat) - flat).reshape(nbins, nblk)
        out_k, out_v = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
        for b in range(nblk):
            wcnt = np.zeros((waves, nbins), dtype=np.int64)
            for w in range(waves):
                s = b * block + w * per_wave
                wcnt[w] = np.bincount(d[s:min(s + per_wave, n)], minlength=nbins) if s < n else 0
            nxt = base[:, b][None, :] + np.cumsum(wcnt, axis=0) - wcnt       # first destination per (wave, digit)
            for w in range(waves):
                for r in range(per_wave // 64):
                    s = b * block + w * per_wave + r * 64
                    if s >= n:
                        break
                    dd = d[s:min(s + 64, n)]
                    below = np.array([(dd[:l] == dd[l]).sum() for l in range(dd.size)])   # same digit in lower lanes
                    dest = nxt[w, dd] + below
                    out_k[dest], out_v[dest] = keys[s:s + dd.size], vals[s:s + dd.size]
                    np.add.at(nxt[w], dd, 1)
        assert (out_v >= 0).all()
        keys, vals = out_k, out_v
    return keys, vals


@pytest.mark.parametrize("bits", [1, 6, 8, 9, 13, 16])
def test_rank_rule_on_the_host_is_a_stable_sort(bits):
    rng = np.random.default_rng(bits)
    for n in (1, 65, BLOCK - 1, BLOCK + 1, 2 * BLOCK + 17):
        pats = _patterns(n, bits, rng)
        for name in ("equal", "random", "rectangles", "top_low_digit"):
            want_k, want_v = _stable_sort(pats[name], bits)
            got_k, got_v = _emulate(pats[name], bits)
            assert np.array_equal(got_k, want_k) and np.array_equal(got_v, want_v), (name, n)


# ---------------------------------------------------------------- the direct entry against torch.sort
GUARD = 64


def _device_sort(L, keys_dev, n, key_bytes, bits, scratch, library):
    """(sorted keys, values) as int64 numpy arrays; the words behind both outputs must stay untouched"""
    from pings_amd import _lib

    kt = torch.int16 if key_bytes == 2 else torch.int32
    ks = torch.full((n + GUARD,), -21846, dtype=kt, device="cuda")
    vs = torch.full((n + GUARD,), -1431655766, dtype=torch.int32, device="cuda")
    _lib.check(L.pings_raster_tile_sort(_lib.ptr(keys_dev), n, key_bytes, bits, _lib.ptr(ks), _lib.ptr(vs),
                                        _lib.ptr(scratch), int(library), _lib.stream_ptr(ks.device)),
               "pings_raster_tile_sort")
    ks, vs = ks.cpu(), vs.cpu()
    assert bool((ks[n:] == -21846).all()) and bool((vs[n:] == -1431655766).all()), "wrote past the outputs"
    ku = ks[:n].numpy().view(np.uint16 if key_bytes == 2 else np.uint32).astype(np.int64)
    return ku, vs[:n].numpy().view(np.uint32).astype(np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("key_bytes,bits", [(2, 1), (2, 6), (2, 8), (2, 9), (2, 13), (2, 16), (4, 13), (4, 20)])
def test_direct_entry_is_torch_stable_sort(key_bytes, bits):
    """Every size at which a block, a wave or a round begins or ends, every key pattern, the project's sort and the
    library's: keys and values equal torch.sort(stable=True)'s, integer for integer, and a second call gives the
    same.  20 bits always take the library path."""
    from pings_amd import _lib

    L = _lib.lib()
    b = C.c_int32(0)
    L.pings_raster_tile_sort_bytes(1, C.byref(b))
    B = b.value
    assert B >= 256 and B % 256 == 0
    rng = np.random.default_rng(100 * key_bytes + bits)
    for n in (0, 1, 63, 64, 65, B - 1, B, B + 1, 2 * B + 17, 40 * B + 5):
        scratch = torch.empty(L.pings_raster_tile_sort_bytes(n, None), dtype=torch.uint8, device="cuda")
        for name, keys in _patterns(n, bits, rng).items():
            want_k, want_v = _stable_sort(keys, bits)
            host = keys.astype(np.uint16).view(np.int16) if key_bytes == 2 else keys.astype(np.uint32).view(np.int32)
            dev = torch.from_numpy(host.copy()).cuda()
            for library in (False, True):
                got_k, got_v = _device_sort(L, dev, n, key_bytes, bits, scratch, library)
                assert np.array_equal(got_k, want_k), (name, n, library, "keys")
                assert np.array_equal(got_v, want_v), (name, n, library, "values")
                again_k, again_v = _device_sort(L, dev, n, key_bytes, bits, scratch, library)
                assert np.array_equal(again_k, got_k) and np.array_equal(again_v, got_v), (name, n, library, "second call")
            assert np.array_equal(dev.cpu().numpy(), host), (name, n, "input changed")


# ---------------------------------------------------------------- through the public rasteriser
def _culled(sc):
    """every Gaussian behind the camera: no instance at all"""
    V = sc["cam"]["viewmatrix"].to(sc["means"].dtype)
    pc = sc["means"] @ V[:3, :3] + V[3, :3]
    pc[:, 2] = -5.0
    sc["means"] = (pc - V[3, :3]) @ torch.linalg.inv(V[:3, :3])
    return sc


def _public_step(sc, mode):
    """forward + backward: every output and gradient, and the sorted list and tile ranges out of the binning blob"""
    import test_raster as TR
    from test_raster_glue import _binning_field, _rast_step

    res = _rast_step(sc, mode, True)
    _, _, fs, radii, per_g = TR._hip_forward(sc, mode, True)
    res["radii"], res["per_gaussian"], res["I"] = radii.cpu(), per_g.cpu(), torch.tensor(fs.I)
    res["ranges"] = _binning_field(fs, "ranges")
    if fs.I > 0:
        res["point_list"] = _binning_field(fs, "point_list")
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["surfel", "3dgs"])
@pytest.mark.parametrize("W,H,P,culled", [(160, 96, 1500, False), (700, 400, 4000, False), (16, 16, 200, False),
                                          (160, 96, 300, True)])
def test_public_path_equals_the_library_sort(W, H, P, culled, mode, monkeypatch):
    """60 tiles (one pass), 1,100 tiles (6 + 5 bits), one tile, and a frame without instances: images, radii,
    contributions, gradients, point_list and ranges of the default build are those of PINGS_TILE_SORT=l and of a
    second default run, bit for bit."""
    from scenes import make_scene

    sc = make_scene(P, W, H, seed=7 + W, surfel=mode == "surfel")
    if culled:
        sc = _culled(sc)
    monkeypatch.delenv("PINGS_TILE_SORT", raising=False)
    a = _public_step(sc, mode)
    a2 = _public_step(sc, mode)
    monkeypatch.setenv("PINGS_TILE_SORT", "l")
    b = _public_step(sc, mode)
    assert a.keys() == a2.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], a2[k]), ("second run", k)
        assert torch.equal(a[k], b[k]), ("library sort", k)
    assert (int(a["I"]) == 0) == culled
    if not culled:
        assert float(a["out0"].abs().sum()) > 0 and int(a["ranges"].max()) == int(a["I"])
