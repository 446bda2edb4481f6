"""The interior classifier of the wave-per-tile blend kernels (csrc/raster_common.hpp: blend_interior), on the host.

pings_raster_debug_interior runs the function the kernels call.  A pair flagged interior lets the kernels drop the
per-pixel alpha and depth decisions for the record, so the flag has to be SOUND: for every flagged pair a numpy fp64
evaluation of all 256 pixel positions of the tile (positions outside the image included) must satisfy each condition
with at least half the margin the classifier's comment derives:
  * alpha:  power <= -0.25e-6 (half of q_min > 1e-6), opacity * exp(power) >= (1 + 0.0005) / 255, opacity below 0.99;
  * depth:  den < -DEN_EPS - E / 2 with E = 1e-6 (|nx| max|rx| + |ny| max|ry| + |nz|), and
            zlo + m / 2 < q / den < zhi - m / 2 with m = max|d0| (1e-6 + E / |den|_min).
The per-pixel ray (rx, ry) is the kernels' fp32 quotient; everything behind it is fp64.  A classifier that always said
"general" would be sound too, so both classes must occur at least 100 times in the random set, and every constructed
boundary case must come out general."""
import ctypes as C

import numpy as np
import pytest

from pings_amd import _lib

F = np.float32
W, H, FX, FY = 1920, 1080, F(1000.0), F(1000.0)
CXP, CYP = F(0.5) * F(W) - F(0.5), F(0.5) * F(H) - F(0.5)
ALPHA_MAX, ALPHA_MIN, DEN_EPS = F(0.99), F(1.0) / F(255.0), F(1e-6)


def interior_flags(records, origins, cxp=CXP, cyp=CYP, fx=FX, fy=FY):
    """flags[i] of pings_raster_debug_interior for records [n, 16] and tile origins [n, 2] (float32)."""
    rec = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, 16)
    org = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 2)
    assert len(rec) == len(org)
    out = np.zeros(len(rec), dtype=np.uint8)
    st = _lib.lib().pings_raster_debug_interior(rec.ctypes.data_as(C.c_void_p), org.ctypes.data_as(C.c_void_p), len(rec),
                                                float(cxp), float(cyp), float(fx), float(fy),
                                                out.ctypes.data_as(C.c_void_p))
    _lib.check(st, "pings_raster_debug_interior")
    return out.astype(bool)


def record(mx, my, opacity, pz, s1, s2, theta, rz, n, q=None):
    """One record: a footprint with standard deviations s1, s2 (pixels) turned by theta, unit normal n; q defaults to the
    plane through the centre's ray at depth pz."""
    c, s = np.cos(theta), np.sin(theta)
    cx = c * c / s1 ** 2 + s * s / s2 ** 2
    cy = c * s * (1.0 / s1 ** 2 - 1.0 / s2 ** 2)
    cz = s * s / s1 ** 2 + c * c / s2 ** 2
    n = np.asarray(n, dtype=np.float64)
    n = n / np.linalg.norm(n)
    if q is None:
        q = pz * (n[0] * (mx - float(CXP)) / float(FX) + n[1] * (my - float(CYP)) / float(FY) + n[2])
    return np.array([mx, my, opacity, pz, cx, cy, cz, rz, 0.5, 0.5, 0.5, q, n[0], n[1], n[2], 0.0], dtype=np.float32)


def random_pairs(n, seed):
    rng = np.random.default_rng(seed)
    recs, orgs = [], []
    gx, gy = (W + 15) // 16, (H + 15) // 16
    for i in range(n):
        # every eighth pair on the tile row that the image's bottom edge cuts, every sixteenth in its last column
        tx = gx - 1 if i % 16 == 0 else int(rng.integers(0, gx))
        ty = gy - 1 if i % 8 == 0 else int(rng.integers(0, gy))
        X0, Y0 = 16.0 * tx, 16.0 * ty
        ang, dist = rng.uniform(0, 2 * np.pi), rng.uniform(0.0, 400.0)
        mx, my = X0 + 7.5 + dist * np.cos(ang), Y0 + 7.5 + dist * np.sin(ang)
        s1, s2 = np.exp(rng.uniform(np.log(30.0), np.log(600.0), size=2))
        pz = rng.uniform(2.0, 30.0)
        nrm = np.array([rng.normal(0, 0.6), rng.normal(0, 0.6), -1.0])
        rz = pz * 10.0 ** rng.uniform(-3.0, 0.0)
        recs.append(record(mx, my, rng.uniform(0.05, 1.0), pz, s1, s2, rng.uniform(0, np.pi), rz, nrm))
        orgs.append((X0, Y0))
    return np.stack(recs), np.array(orgs, dtype=np.float32)


def constructed_pairs():
    """name -> (record, tile origin): each a boundary the classifier must not call interior."""
    X0, Y0 = 16.0 * 70, 16.0 * 20
    xm, ym = X0 + 7.5, Y0 + 7.5
    big = dict(s1=400.0, s2=300.0, theta=0.3)
    out = {}
    # den = nx rx + nz crosses zero (hence -DEN_EPS) in the tile's middle column: a surfel seen edge-on
    rxm = (xm - float(CXP)) / float(FX)
    out["edge-on"] = (record(xm + 60, ym + 40, 0.6, 5.0, rz=1.0, n=(1.0, 0.0, -rxm), q=-0.05, **big), (X0, Y0))
    # a slanted surfel with a thin depth range: the ray hit leaves [zlo, zhi] right of the centre's column, which is
    # placed left of the tile, then right of it
    slant = (0.9, 0.0, -0.45)
    out["slanted-leaves-right"] = (record(X0 - 40, ym + 30, 0.6, 5.0, rz=0.02, n=slant, **big), (X0, Y0))
    out["slanted-leaves-left"] = (record(X0 + 56, ym + 30, 0.6, 5.0, rz=0.02, n=slant, **big), (X0, Y0))
    out["centre-in-tile"] = (record(xm + 2.5, ym - 3.5, 0.6, 5.0, rz=1.0, n=(0.1, 0.1, -1.0), **big), (X0, Y0))
    above = np.nextafter(ALPHA_MAX, F(2.0))
    for name, o in (("opacity-0.99", ALPHA_MAX), ("opacity-0.99-next", above), ("opacity-1", F(1.0))):
        out[name] = (record(xm + 60, ym + 40, float(o), 5.0, rz=1.0, n=(0.1, 0.1, -1.0), **big), (X0, Y0))
    # alpha = 1/255 where q = 2 ln(255 * 0.6) = 10.06: with s = 20 px that is 63.4 px from the centre, inside the tile
    out["alpha-contour-cuts"] = (record(X0 - 56, ym, 0.6, 5.0, s1=20.0, s2=20.0, theta=0.0, rz=1.0, n=(0.1, 0.1, -1.0)),
                                 (X0, Y0))
    # the tile row the bottom edge cuts (rows 1072 .. 1087, the image ends at 1079): the depth range is left only in
    # the rows below the image, and the alpha contour crosses only there — positions outside the image count
    Yb = 16.0 * ((H + 15) // 16 - 1)
    den_at = lambda row: (0.5 * (row - float(CYP)) / float(FY) - 1.0)       # of the normal (0, 0.5, -1), unnormalised
    out["bottom-edge-depth"] = (record(xm + 60, Yb - 100, 0.6, 5.0, rz=5.0 * (den_at(Yb - 100) / den_at(Yb + 10.5) - 1.0),
                                       n=(0.0, 0.5, -1.0), **big), (X0, Yb))
    out["bottom-edge-alpha"] = (record(xm, Yb + 12.0 - 63.4, 0.6, 5.0, s1=20.0, s2=20.0, theta=0.0, rz=1.0,
                                       n=(0.1, 0.1, -1.0)), (X0, Yb))
    Xr = 16.0 * ((W + 15) // 16 - 1)
    out["right-edge-centre-in-tile"] = (record(Xr + 14.0, ym + 0.5, 0.6, 5.0, rz=1.0, n=(0.1, 0.1, -1.0), **big), (Xr, Y0))
    return out


def fp64_margins(rec, org):
    """For one pair: the smallest slack of each condition over the 256 pixel positions, in units in which the
    assertion is `slack > 0` with HALF the classifier's margin already taken off."""
    r = rec.astype(np.float32)
    mx, my, o, pz, cx, cy, cz, rz = (float(v) for v in r[:8])
    q, nx, ny, nz = float(r[11]), float(r[12]), float(r[13]), float(r[14])
    X0, Y0 = F(org[0]), F(org[1])
    px = X0 + np.arange(16, dtype=np.float32)
    py = Y0 + np.arange(16, dtype=np.float32)
    rx = ((px - CXP) / FX).astype(np.float64)      # the kernels' fp32 quotient
    ry = ((py - CYP) / FY).astype(np.float64)
    PX, PY = np.meshgrid(px.astype(np.float64), py.astype(np.float64))
    RX, RY = np.meshgrid(rx, ry)
    dx, dy = mx - PX, my - PY
    power = -0.5 * (cx * dx * dx + cz * dy * dy) - cy * dx * dy
    alpha = o * np.exp(power)
    den = nx * RX + ny * RY + nz
    mag = abs(nx) * np.abs(rx).max() + abs(ny) * np.abs(ry).max() + abs(nz)
    e_den = 1e-6 * mag
    out = {"opacity": float(ALPHA_MAX) - o if o < float(ALPHA_MAX) else -1.0,
           "power": (-0.25e-6 - power).min(),
           "alpha": (alpha - 1.0005 * float(ALPHA_MIN)).min(),
           "den": (-float(DEN_EPS) - 0.5 * e_den - den).min()}
    if out["den"] > 0:
        d0 = q / den
        m = np.abs(d0).max() * (1e-6 + e_den / np.abs(den).min())
        zlo, zhi = float(F(r[3]) - F(r[7])), float(F(r[3]) + F(r[7]))
        out["zlo"] = (d0 - 0.5 * m - zlo).min()
        out["zhi"] = (zhi - 0.5 * m - d0).min()
    return out


RANDOM = random_pairs(4000, seed=11)


def test_flagged_pairs_satisfy_every_condition_in_fp64_with_half_the_margin():
    recs, orgs = RANDOM
    cons = constructed_pairs()
    recs = np.concatenate([recs, np.stack([v[0] for v in cons.values()])])
    orgs = np.concatenate([orgs, np.array([v[1] for v in cons.values()], dtype=np.float32)])
    flags = interior_flags(recs, orgs)
    bad = []
    for i in np.nonzero(flags)[0]:
        m = fp64_margins(recs[i], orgs[i])
        if len(m) < 6 or min(m.values()) <= 0:
            bad.append((int(i), m))
    assert not bad, bad[:5]


def test_both_classes_occur_in_the_random_set():
    flags = interior_flags(*RANDOM)
    n_int = int(flags.sum())
    print(f"interior {n_int}, general {len(flags) - n_int} of {len(flags)}")
    assert n_int >= 100 and len(flags) - n_int >= 100
    # and on the tiles the image's edges cut
    edge = (RANDOM[1][:, 1] == 16.0 * ((H + 15) // 16 - 1))
    assert int(flags[edge].sum()) >= 20


def test_the_random_set_holds_general_pairs_of_every_kind():
    """The general class of the random set is not one condition's alone: each of the conditions fails, on its own, for
    some pair that passes the others (fp64, no margins)."""
    recs, orgs = RANDOM
    flags = interior_flags(recs, orgs)
    kinds = {"alpha": 0, "depth": 0}
    for i in np.nonzero(~flags)[0][:1500]:
        m = fp64_margins(recs[i], orgs[i])
        alpha_ok = m["opacity"] > 0 and m["power"] > 0 and m["alpha"] > 0
        depth_ok = len(m) == 6 and m["den"] > 0 and m["zlo"] > 0 and m["zhi"] > 0
        if alpha_ok and not depth_ok:
            kinds["depth"] += 1
        if depth_ok and not alpha_ok:
            kinds["alpha"] += 1
    assert kinds["alpha"] >= 20 and kinds["depth"] >= 20, kinds


@pytest.mark.parametrize("name", sorted(constructed_pairs()))
def test_constructed_boundary_cases_are_general(name):
    rec, org = constructed_pairs()[name]
    assert not interior_flags(rec[None], np.array([org], dtype=np.float32))[0]


def test_constructed_cases_are_boundaries_of_the_condition_they_name():
    """Each constructed pair fails in fp64 what its name says and, moved off its boundary, is interior: the cases test
    the classifier's conditions, not an unrelated rejection."""
    cons = constructed_pairs()
    m = fp64_margins(*cons["edge-on"])
    assert m["den"] <= 0
    for k in ("slanted-leaves-right", "slanted-leaves-left", "bottom-edge-depth"):
        m = fp64_margins(*cons[k])
        assert m["den"] > 0 and m["alpha"] > 0 and m["power"] > 0 and min(m["zlo"], m["zhi"]) <= 0, (k, m)
    for k in ("alpha-contour-cuts", "bottom-edge-alpha"):
        m = fp64_margins(*cons[k])
        assert m["alpha"] <= 0 and m["den"] > 0 and m["zlo"] > 0 and m["zhi"] > 0, (k, m)
    for k in ("centre-in-tile", "right-edge-centre-in-tile"):
        assert fp64_margins(*cons[k])["power"] <= 0
    # the opacity cases with an opacity of 0.9 are interior: nothing else about them is a boundary
    rec, org = cons["opacity-1"]
    rec = rec.copy()
    rec[2] = 0.9
    assert interior_flags(rec[None], np.array([org], dtype=np.float32))[0]
    # the bottom-edge cases are interior in the tile row above, which the image holds whole
    for k in ("bottom-edge-depth", "bottom-edge-alpha"):
        rec, org = cons[k]
        assert interior_flags(rec[None], np.array([(org[0], org[1] - 16.0)], dtype=np.float32))[0], k


def test_null_pointers_are_refused():
    L = _lib.lib()
    assert L.pings_raster_debug_interior(None, None, 3, 1.0, 1.0, 1.0, 1.0, None) == 1 and b"null" in L.pings_last_error()
    assert L.pings_raster_debug_interior(None, None, 0, 1.0, 1.0, 1.0, 1.0, None) == 0
