"""fp64 numpy restatement of LiDAR-scan fusion into the sparse TSDF volume (pings_amd/tsdf_ops.py:
TSDFVolume.integrate_points, csrc/tsdf_points.hip), written from the rules and not from the device code.
It adds to tests/tsdf_ref.py: the store order, `dense` and the extraction are `tsdf_ref.Volume`'s.

The rules.  Grid point g owns the half-open cube of edge `voxel` centred at origin + voxel g.  A valid point p (finite,
min_range < r = |p - o| < max_range) gives the ray o + s d, d = (p - o) / r, s in [s0, s1], s1 = r + trunc,
s0 = max(0, r - trunc) or 0 with carving.  It samples every cube it crosses with a positive chord.  At a sample with
centre c: sdf = sign((c - o).(p - c)) |p - c| ("point", sign(0) = +1) or r - (c - o).d ("ray"); it updates iff
sdf > -trunc with t = min(1, sdf / trunc), quantised once as q = rint(t 2^SCALE_BITS) (colours likewise).  Per call and
voxel with n updating samples and exact sums S, C: tsdf <- (tsdf w + S) / (w + n), colour likewise, w <- min(w + n,
max_weight).

A voxel is *marginal* if, in any call, a sample of it
  * has a chord within CHORD_EPS voxel of zero (it may or may not be a sample in fp32); this includes the cubes next to a
    point where the ray crosses two faces, or a face and an end of its segment, within CHORD_EPS of each other,
  * has |sdf + trunc| < SDF_EPS trunc (the update test may flip), or
  * in "point" mode has |(c - o).(p - c)| < DOT_EPS |c - o| |p - c| (the sign may flip: a jump of up to 2 |p - c|).
A block is marginal if only marginal samples name it."""
from __future__ import annotations

import functools
import itertools

import numpy as np

import tsdf_ref as R

B = R.B
SCALE_BITS = 22                                   # PINGS_TSDF_POINTS_SCALE_BITS
SCALE = float(1 << SCALE_BITS)
MAX_POINTS = (1 << 20) - 1                        # PINGS_TSDF_POINTS_MAX
CHORD_EPS, SDF_EPS, DOT_EPS = 1e-3, 1e-4, 1e-5


def ray_samples(o, p, origin, voxel, trunc, carve):
    """The cubes of one ray -> (samples [(g, chord in voxels)], near: the cubes a chord within CHORD_EPS of zero could
    add or remove, r, d).  o, p fp64."""
    v = p - o
    r = float(np.sqrt(v @ v))
    d = v / r
    s0, s1 = (0.0 if carve else max(0.0, r - trunc)), r + trunc
    x0 = (o - origin) / voxel + 0.5               # cube index = floor(x0 + s d / voxel): faces at the integers
    dv = d / voxel
    eps = CHORD_EPS * voxel
    events = [(s0, -1), (s1, -1)]                 # (parameter, axis); the ends of the segment are events too
    for a in range(3):
        if dv[a] == 0.0:
            continue
        xa, xb = sorted((x0[a] + (s0 - eps) * dv[a], x0[a] + (s1 + eps) * dv[a]))
        for m in range(int(np.ceil(xa)), int(np.floor(xb)) + 1):
            events.append(((m - x0[a]) / dv[a], a))
    events.sort()
    cuts = [s0] + [s for s, a in events if a >= 0 and s0 < s < s1] + [s1]
    samples = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        if hi > lo:
            g = np.floor(x0 + 0.5 * (lo + hi) * dv).astype(np.int64)
            samples.append(((int(g[0]), int(g[1]), int(g[2])), (hi - lo) / voxel))
    near = set()
    for (sa, _), (sb, ab) in zip(events[:-1], events[1:]):
        if sb - sa < eps:                         # two events that fp32 may order the other way
            for s in (sa, sb):
                x = x0 + s * dv
                lo, hi = np.floor(x - 2 * CHORD_EPS).astype(np.int64), np.floor(x + 2 * CHORD_EPS).astype(np.int64)
                for c in itertools.product(*[sorted({int(lo[a]), int(hi[a])}) for a in range(3)]):
                    near.add(c)
    return samples, near, r, d


class Volume(R.Volume):
    """`tsdf_ref.Volume` with `integrate_points`; depth views and scans can share it."""

    def integrate_points(self, points, origin, colors=None, space_carving=False, sdf_mode="point", min_range=0.0,
                         max_range=np.inf, max_weight=None):
        """points [N, 3], origin [3], colors [N, 3] as the device receives them (fp32).  -> (touched blocks,
        {g: number of updating samples})."""
        assert sdf_mode in ("point", "ray")
        pts = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
        o = np.asarray(origin, np.float32).astype(np.float64)
        if len(pts) > MAX_POINTS:
            raise ValueError("too many points for the count field")
        if space_carving and not np.isfinite(max_range):
            raise ValueError("space carving needs a finite max_range")
        voxel, trunc = self.voxel_length, self.sdf_trunc
        cols = None if colors is None else np.asarray(colors, np.float32).astype(np.float64)
        acc: dict = {}                            # g -> [n, sum q, sum q colour (3)] in Python integers: exact
        marginal, touched, definite = set(), set(), set()
        with np.errstate(all="ignore"):
            rr = np.sqrt(((pts - o) ** 2).sum(1))
        valid = np.isfinite(pts).all(1) & np.isfinite(rr) & (rr > min_range) & (rr < max_range)
        for i in np.nonzero(valid)[0]:
            p = pts[i]
            samples, near, r, d = ray_samples(o, p, self.origin, voxel, trunc, space_carving)
            marginal |= near
            qc = None if cols is None else [int(np.rint(min(max(c, 0.0), 1.0) * SCALE)) for c in cols[i]]
            for g, chord in samples:
                blk = (g[0] >> 3, g[1] >> 3, g[2] >> 3)
                touched.add(blk)
                if chord < CHORD_EPS:
                    marginal.add(g)
                else:
                    definite.add(blk)
                c = self.origin + voxel * np.array(g, np.float64)
                co, pc = c - o, p - c
                if sdf_mode == "ray":
                    sdf = r - co @ d
                else:
                    dot, dist = co @ pc, float(np.sqrt(pc @ pc))
                    sdf = dist if dot >= 0.0 else -dist
                    if abs(dot) < DOT_EPS * np.sqrt(co @ co) * dist:
                        marginal.add(g)
                if abs(sdf + trunc) < SDF_EPS * trunc:
                    marginal.add(g)
                if not sdf > -trunc:
                    continue
                q = int(np.rint(min(1.0, sdf / trunc) * SCALE))
                a = acc.setdefault(g, [0, 0, [0, 0, 0]])
                a[0] += 1
                a[1] += q
                if qc is not None:
                    for ch in range(3):
                        a[2][ch] += qc[ch]
        before = set(self.slots)
        new = sorted(b for b in touched if b not in self.slots)
        for b in new:
            self.slots[b] = len(self.coords)
            self.coords.append(b)
        n = len(new)
        self.tsdf = np.concatenate([self.tsdf, np.ones((n, B ** 3))])
        self.weight = np.concatenate([self.weight, np.zeros((n, B ** 3))])
        self.color = np.concatenate([self.color, np.zeros((n, B ** 3, 3))])
        self.marginal = np.concatenate([self.marginal, np.zeros((n, B ** 3), bool)])
        cap = np.inf if max_weight is None else float(max_weight)
        for g, (cnt, s, cs) in acc.items():
            slot, l = self.slots[(g[0] >> 3, g[1] >> 3, g[2] >> 3)], (g[0] & 7) << 6 | (g[1] & 7) << 3 | (g[2] & 7)
            w = self.weight[slot, l]
            self.tsdf[slot, l] = (self.tsdf[slot, l] * w + s / SCALE) / (w + cnt)
            if self.has_color and cols is not None:
                self.color[slot, l] = (self.color[slot, l] * w + np.array(cs, np.float64) / SCALE) / (w + cnt)
            self.weight[slot, l] = min(w + cnt, cap)
        for g in marginal:
            blk = (g[0] >> 3, g[1] >> 3, g[2] >> 3)
            if blk in self.slots:
                self.marginal[self.slots[blk], (g[0] & 7) << 6 | (g[1] & 7) << 3 | (g[2] & 7)] = True
            if blk not in definite and blk not in before:
                self.marginal_blocks.add(blk)          # the device may or may not hold it
        return touched, {g: a[0] for g, a in acc.items()}


# ---------------------------------------------------------------------- the scans of the tests' analytic scene
FAN, FAN_CARVED, HALF_ANGLE = (48, 32), (24, 16), 0.42
CARVE_RANGE = 4.5                                 # past every hit of the scene (at most |c| + 1 < 4.2)
BOX = ((-48, -48, -48), (72, 72, 72))             # grid points that hold every block of the scans, the sensors included


def point_color(p):
    """A smooth function of the point, [N, 3] fp32 in [0, 1]."""
    p = np.asarray(p, np.float64)
    return np.stack([0.5 + 0.5 * np.sin(2.1 * p[:, 0]), 0.5 + 0.5 * np.cos(1.7 * p[:, 1]),
                     0.5 + 0.25 * (p[:, 2] + 1.0) * 0.9], -1).clip(0.0, 1.0).astype(np.float32)


def sphere_scan(c, fan=FAN):
    """A fan of fan[0] x fan[1] directions around the line from `c` to the centre of the unit sphere; the exact hits
    rounded to fp32; rays that miss give no point.  -> (points [N, 3] fp32, colours [N, 3] fp32, sensor [3] fp32)."""
    c = np.asarray(c, np.float32).astype(np.float64)          # the sensor as the device receives it
    E = R.look_at_origin(c)
    x, y, z = E[0, :3], E[1, :3], E[2, :3]
    a, b = np.meshgrid(np.linspace(-HALF_ANGLE, HALF_ANGLE, fan[0]), np.linspace(-HALF_ANGLE, HALF_ANGLE, fan[1]))
    D = z + np.tan(a.reshape(-1, 1)) * x + np.tan(b.reshape(-1, 1)) * y
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    bq, cq = D @ c, c @ c - 1.0
    disc = bq * bq - cq
    hit = disc > 0
    s = -bq[hit] - np.sqrt(disc[hit])
    pts = (c + s[:, None] * D[hit]).astype(np.float32)
    return pts, point_color(pts), c.astype(np.float32)


@functools.lru_cache(maxsize=None)
def sphere_scans(carved=False):
    return [sphere_scan(c, FAN_CARVED if carved else FAN) for c in R.CAMERAS]


@functools.lru_cache(maxsize=None)
def sphere_reference(sdf_mode="point", carved=False):
    """The three scans fused once per mode for every test that needs them (treat as read-only): (volume, [(block list
    in slot order, dense(BOX), marginal blocks so far, {g: updating samples of this call}) after each scan])."""
    vol, snaps = Volume(R.VOXEL, R.TRUNC), []
    for pts, col, o in sphere_scans(carved):
        _, counts = vol.integrate_points(pts, o, col, space_carving=carved, sdf_mode=sdf_mode,
                                         max_range=CARVE_RANGE if carved else np.inf)
        snaps.append((list(vol.coords), vol.dense(*BOX), set(vol.marginal_blocks), counts))
    return vol, snaps


def counts_dense(counts, box=BOX):
    """{g: n} -> an int array over the box (every g of the scene lies inside it)."""
    lo = np.asarray(box[0])
    out = np.zeros(tuple(np.asarray(box[1]) - lo), np.int64)
    for g, n in counts.items():
        out[tuple(np.asarray(g) - lo)] = n
    return out
