"""Numpy restatement of the device marching cubes (pings_amd/csrc/mc.hip) — the specification of its bits
and of its output order.  fp32 throughout, vectorised over the cells that the surface crosses.

Cell (i, j, k) spans corners (i..i+1, j..j+1, k..k+1); corner c = di + 2 dj + 4 dk.  Edge e = 4a + o1 + 2 o2: axis a,
(o1, o2) the corner bits of the two other axes in increasing axis order.  Vertex key = 4 p + slot, p the grid point's
linear index (i*ny + j)*nz + k, slot 0 the point itself and 1..3 its +x, +y, +z edge.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32


def edge_lo(e: int) -> int:
    a, o1, o2 = e >> 2, e & 1, (e >> 1) & 1
    return (o1 << 1) | (o2 << 2) if a == 0 else o1 | (o2 << 2) if a == 1 else o1 | (o2 << 1)


def edge_of(ca: int, cb: int) -> int:
    lo, a = ca & cb, {1: 0, 2: 1, 4: 2}[ca ^ cb]
    o1 = (lo >> 1) & 1 if a == 0 else lo & 1
    o2 = (lo >> 1) & 1 if a == 2 else (lo >> 2) & 1
    return 4 * a + o1 + 2 * o2


def face_corner(a: int, s: int, m: int) -> int:
    """Corner m of face (a, s), counter-clockwise about the outward normal."""
    u, w = (a + 1) % 3, (a + 2) % 3
    cu = int(m in (1, 2)) if s else int(m in (2, 3))
    cw = int(m in (2, 3)) if s else int(m in (1, 2))
    return (s << a) | (cu << u) | (cw << w)


FACES = []
for _f in range(6):
    _q = [face_corner(_f >> 1, _f & 1, m) for m in range(4)]
    FACES.append((_q, [edge_of(_q[m], _q[(m + 1) % 4]) for m in range(4)]))


def processed(vals: np.ndarray, lowest_mask) -> np.ndarray:
    """skimage's mask read as gating the cell's lowest corner, and all 8 corners finite.
    vals [..., 8] corner values, lowest_mask the mask at each cell's lowest corner (None: every cell)."""
    ok = np.isfinite(vals).all(-1)
    return ok if lowest_mask is None else ok & (lowest_mask != 0)


def _edge_keys(ia, p0, stride, a, v0, v1, level):
    with np.errstate(all="ignore"):
        c = ia.astype(F32) + (level - v0) / (v1 - v0)
    return np.where(c == ia.astype(F32), 4 * p0,
                    np.where(c == (ia + 1).astype(F32), 4 * (p0 + stride), 4 * p0 + 1 + a))


def marching_cubes(volume, level=0.0, mask=None, allow_degenerate=False, gradient_direction="descent"):
    """-> (verts [V,3] float32 in index units, faces [F,3] int64), in the order the device writes them."""
    if gradient_direction not in ("descent", "ascent"):
        raise ValueError(gradient_direction)
    v = np.ascontiguousarray(volume, dtype=F32)
    nx, ny, nz = v.shape
    level = F32(level)
    empty = (np.zeros((0, 3), F32), np.zeros((0, 3), np.int64))
    if min(nx, ny, nz) < 2:
        return empty
    strides = np.array([ny * nz, nz, 1], np.int64)
    cube = [v[c & 1:nx - 1 + (c & 1), (c >> 1) & 1:ny - 1 + ((c >> 1) & 1), (c >> 2) & 1:nz - 1 + ((c >> 2) & 1)]
            for c in range(8)]
    code = np.zeros(cube[0].shape, np.int32)
    for c in range(8):
        code |= (cube[c] < level).astype(np.int32) << c
    cand = (code != 0) & (code != 255)
    ci, cj, ck = np.nonzero(cand)
    vals = np.stack([cube[c][ci, cj, ck] for c in range(8)], -1)
    lm = None if mask is None else np.asarray(mask)[ci, cj, ck]
    keep = processed(vals, lm)
    ci, cj, ck, vals, code = ci[keep], cj[keep], ck[keep], vals[keep], code[ci, cj, ck][keep]
    n = ci.shape[0]
    if n == 0:
        return empty
    ijk = np.stack([ci, cj, ck], -1).astype(np.int64)
    base = (ijk[:, 0] * ny + ijk[:, 1]) * nz + ijk[:, 2]

    keys = np.zeros((n, 12), np.int64)
    cross = np.zeros((n, 12), bool)
    for e in range(12):
        a, lo = e >> 2, edge_lo(e)
        hi = lo | (1 << a)
        cross[:, e] = (((code >> lo) ^ (code >> hi)) & 1) == 1
        bits = np.array([lo & 1, (lo >> 1) & 1, (lo >> 2) & 1], np.int64)
        p0 = base + (bits * strides).sum()
        keys[:, e] = np.where(cross[:, e], _edge_keys(ijk[:, a] + bits[a], p0, strides[a], a, vals[:, lo], vals[:, hi],
                                                      level), 0)

    # segments exit -> entry on every face: nxt[e] = successor edge of crossing edge e
    nxt = np.full((n, 12), -1, np.int64)
    for q, ex in FACES:
        b = [((code >> q[m]) & 1) == 1 for m in range(4)]
        amb = (b[0] == b[2]) & (b[1] == b[3]) & (b[0] != b[1])
        f = [vals[:, q[m]] - level for m in range(4)]
        p02, p13 = f[0] * f[2], f[1] * f[3]
        conn = np.where(b[0], p02 > p13, p13 > p02)
        entry = np.zeros(n, np.int64)
        for m in range(4):
            entry = np.where(~b[m] & b[(m + 1) % 4], m, entry)
        exa = np.array(ex, np.int64)
        for m in range(4):
            ex_m = b[m] & ~b[(m + 1) % 4]
            partner = np.where(amb, np.where(conn, (m + 1) % 4, (m + 3) % 4), entry)
            nxt[ex_m, ex[m]] = exa[partner[ex_m]]

    desc = gradient_direction == "descent"
    todo = cross.copy()
    out_cell, out_ord, out_tri = [], [], []
    count = np.zeros(n, np.int64)
    for s in range(12):
        rows = np.nonzero(todo[:, s])[0]
        if rows.size == 0:
            continue
        r = rows.shape[0]
        e = np.full(r, s, np.int64)
        seq = np.zeros((r, 12), np.int64)
        length = np.zeros(r, np.int64)
        best = np.zeros(r, np.int64)
        bm = np.zeros(r, np.int64)
        active = np.ones(r, bool)
        for step in range(12):      # do { visit e; e = nxt[e] } while (e != s && n < 12)
            ar = np.nonzero(active)[0]
            if ar.size == 0:
                break
            ea = e[ar]
            todo[rows[ar], ea] = False
            kk = keys[rows[ar], ea]
            better = (length[ar] == 0) | (kk < best[ar])
            best[ar] = np.where(better, kk, best[ar])
            bm[ar] = np.where(better, length[ar], bm[ar])
            seq[ar, length[ar]] = ea
            length[ar] += 1
            e[ar] = nxt[rows[ar], ea]
            active[ar] = (e[ar] != s) & (length[ar] < 12)
        for t in range(1, 11):      # fan from the loop's smallest key
            ok = t + 1 < length
            if not ok.any():
                break
            ia = (bm + t) % np.maximum(length, 1)
            ib = (bm + t + 1) % np.maximum(length, 1)
            ka = keys[rows, seq[np.arange(r), ia]]
            kb = keys[rows, seq[np.arange(r), ib]]
            if not allow_degenerate:
                ok &= (ka != best) & (kb != best) & (ka != kb)
            idx = np.nonzero(ok)[0]
            tri = np.stack([best[idx], ka[idx], kb[idx]] if desc else [best[idx], kb[idx], ka[idx]], -1)
            out_cell.append(rows[idx])
            out_ord.append(count[rows[idx]])
            out_tri.append(tri)
            count[rows[idx]] += 1
    if not out_tri:
        return empty
    cell, order, tri = np.concatenate(out_cell), np.concatenate(out_ord), np.concatenate(out_tri)
    tri = tri[np.lexsort((order, cell))]
    if tri.shape[0] == 0:
        return empty

    vkeys = np.unique(tri)
    p, slot = vkeys >> 2, vkeys & 3
    pi, pj, pk = p // (ny * nz), (p // nz) % ny, p % nz
    verts = np.stack([pi, pj, pk], -1).astype(F32)
    flat = v.reshape(-1)
    for a in range(3):
        on = np.nonzero(slot == 1 + a)[0]
        v0, v1 = flat[p[on]], flat[p[on] + strides[a]]
        with np.errstate(all="ignore"):
            verts[on, a] = verts[on, a] + (level - v0) / (v1 - v0)
    faces = np.searchsorted(vkeys, tri).astype(np.int64)
    return verts, faces
