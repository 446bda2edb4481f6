"""fp64 restatement of the odometry loop's `assemble` and `step` from plain arrays, for tests/test_tracker_edges.py.

`assemble` is registration_step (utils/tracker.py:353-605) up to implicit_reg's two GEMMs with the formulas of
tests/tracking_ref.py:step, fed the arrays the kernel sees instead of a query: validity, residual, the three weights,
J = [p x g, g], and the sums  N = sum w J^T J,  g = -sum w r J,  count, sum w, sum |r|, sum w r^2.  Next to every sum of
signed terms it returns the sum of the terms' magnitudes (`S`, `Sg`), the scale of the rounding-error bound of the
tests.  `dtype` is the precision of the per-point quantities (|g|, r, w, J); products and sums are always fp64, so
`dtype=torch.float32` is the reference's own fp32 operator order with an exact accumulation: what the kernel may differ
from the fp64 run by.  `step` is implicit_reg's tail (:649-689) from the 42 numbers [N | g].

`make_inputs` / `edge_rows` build the inputs of the tests; they live here so that the CPU tests check the very arrays
the GPU tests upload.
"""
from types import SimpleNamespace as NS

import numpy as np
import torch

F_NORMALS, F_DIV_GRAD, F_WEIGHTED = 1, 2, 4     # pings_amd._abi.REG_F_*

f32 = lambda v: float(np.float32(v))

# The scalar settings of pings_reg_loop_args, as the fp32 numbers the kernel compares with.  min_grad and max_grad are
# 1.25 * 2^e so that the gradient (0.75, 1, 0) * 2^e sits on them exactly: 0.5625 + 1 = 1.5625 = 1.25^2 without rounding.
SETTINGS = dict(min_grad=0.3125, max_grad=1.25, max_std=f32(0.06), gm_dist=f32(0.3), gm_grad=f32(0.1), lm_lambda=f32(1e-4))

# name -> (flags, GM distance on, GM gradient on): the flag sets of the assemble tests.  F_WEIGHTED (read by the step
# only) is set wherever the reference's w is a tensor: any weight on.
FLAG_SETS = {
    "none": (0, False, False),
    "normals": (F_NORMALS | F_WEIGHTED, False, False),
    "div_grad": (F_DIV_GRAD, False, False),
    "all": (F_NORMALS | F_DIV_GRAD | F_WEIGHTED, True, True),
    "gm_dist": (F_WEIGHTED, True, False),
    "gm_grad": (F_WEIGHTED, False, True),
}

ASSEMBLE_SIZES = (0, 1, 9, 10, 255, 256, 257, 65535, 65536, 65537, 131073)
FULL_GRID_SIZES = (257, 65537)
# (n, flag set, labels non-zero): the full flag grid at two sizes, the richest flag set at the others
ASSEMBLE_CASES = [(n, fs, n == 65536) for n in ASSEMBLE_SIZES for fs in (FLAG_SETS if n in FULL_GRID_SIZES else ("all",))]
NORMAL_EQ_SIZES = (0, 1, 255, 256, 257, 131072, 131073, 262145)


def settings(flagset):
    flags, gd, gg = FLAG_SETS[flagset]
    s = dict(SETTINGS)
    s["flags"] = flags
    if not gd:
        s["gm_dist"] = 0.0
    if not gg:
        s["gm_grad"] = 0.0
    return s


# ---------------------------------------------------------------- inputs
def edge_rows():
    """Rows that sit exactly on the edges of the validity window: (grad[m,3], std[m], mask[m], expected valid[m])."""
    m, M, s = (np.float32(SETTINGS[k]) for k in ("min_grad", "max_grad", "max_std"))
    up = lambda v: np.nextafter(v, np.float32(np.inf))
    dn = lambda v: np.nextafter(v, np.float32(-np.inf))
    ok_std, nan = np.float32(0.5) * s, np.float32(np.nan)
    rows = [
        # |g| at min_grad: equality and the lower neighbour are out (strict >), the upper neighbour is in
        ((m, 0, 0), ok_std, 1, False), ((0, up(m), 0), ok_std, 1, True), ((0, 0, -dn(m)), ok_std, 1, False),
        ((0.75 * m / 1.25, m / 1.25, 0), ok_std, 1, False),
        # |g| at max_grad: equality and the upper neighbour are out (strict <), the lower neighbour is in
        ((-M, 0, 0), ok_std, 1, False), ((0, dn(M), 0), ok_std, 1, True), ((0, 0, up(M)), ok_std, 1, False),
        ((0, M / 1.25, -0.75 * M / 1.25), ok_std, 1, False),
        # std at max_std (strict <)
        ((0, 1, 0), s, 1, False), ((0, 1, 0), dn(s), 1, True), ((0, 1, 0), up(s), 1, False),
        # masked out, NaN gradient, NaN std: `NaN < x` is false
        ((0, 1, 0), ok_std, 0, False), ((0.5, nan, 0.5), ok_std, 1, False), ((0, 1, 0), nan, 1, False),
    ]
    g = np.array([r[0] for r in rows], np.float32)
    return g, np.array([r[1] for r in rows], np.float32), np.array([r[2] for r in rows], np.uint8), \
        np.array([r[3] for r in rows], bool)


def _norm64(g):
    g = g.astype(np.float64)
    return np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])


def make_inputs(n, seed, offset=1000.0, label_nonzero=False, edges=True, all_valid=False):
    """fp32 inputs of `assemble` as numpy arrays: points in a 6 m box around (offset, -offset, offset / 2), gradients of
    random direction with norms over [0.2, 2.5], sdf within 0.1, std around max_std, 85 % of the mask set.  Every drawn
    |g| and std is at least 1e-5 (relative) off its threshold; `edges` puts `edge_rows` at the front and, once more, at
    the very end (the rows of the last grid-stride pass).  `all_valid` (the sizes of a handful of points, where chance
    could leave none valid) draws every row inside the window with its mask set."""
    rng = np.random.default_rng(seed)
    m, M, s = SETTINGS["min_grad"], SETTINGS["max_grad"], SETTINGS["max_std"]
    cur = (rng.uniform(-3.0, 3.0, (n, 3)) + np.array([offset, -offset, 0.5 * offset])).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-12)
    lo, hi, top = (1.1 * m, 0.95 * M, 0.95) if all_valid else (0.2, 2.5, 1.2)
    grad = (d * rng.uniform(lo, hi, (n, 1))).astype(np.float32)
    std = (s * rng.uniform(0.2, top, n)).astype(np.float32)
    for _ in range(100):     # resample what fp32 and fp64 could decide differently
        bad = np.flatnonzero((np.abs(_norm64(grad) - m) < 1e-5 * m) | (np.abs(_norm64(grad) - M) < 1e-5 * M) |
                             (np.abs(std.astype(np.float64) - s) < 1e-5 * s))
        if bad.size == 0:
            break
        grad[bad] = (d[bad] * rng.uniform(lo, hi, (bad.size, 1))).astype(np.float32)
        std[bad] = (s * rng.uniform(0.2, top, bad.size)).astype(np.float32)
    else:
        raise AssertionError("could not move every point off the thresholds")
    mask = (rng.uniform(size=n) < (2.0 if all_valid else 0.85)).astype(np.uint8)
    sdf = rng.uniform(-0.1, 0.1, n).astype(np.float32)
    label = (rng.uniform(-0.02, 0.02, n) if label_nonzero else np.zeros(n)).astype(np.float32)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-12)).astype(np.float32)
    expect = np.zeros(n, bool)
    has_edges = np.zeros(n, bool)
    if edges:
        eg, es, em, ev = edge_rows()
        E = eg.shape[0]
        for head in ([0] if n >= E else []) + ([n - E] if n >= 2 * E else []):
            grad[head:head + E], std[head:head + E], mask[head:head + E] = eg, es, em
            expect[head:head + E], has_edges[head:head + E] = ev, True
    return NS(n=n, cur=cur, sdf=sdf, grad=grad, std=std, mask=mask, label=label, normals=nrm, edge=has_edges,
              edge_valid=expect)


def limit_valid(inp, valid, keep):
    """Clears the mask of every valid row after the first `keep`: exactly `keep` valid points, spread as they were."""
    idx = np.flatnonzero(valid)
    assert idx.size >= keep
    inp.mask = inp.mask.copy()
    inp.mask[idx[keep:]] = 0
    return inp


def make_normal_eq_inputs(n, seed, offset=1000.0):
    """points, grad, residual, weight of `pings_reg_normal_equations` (fp32 numpy)."""
    i = make_inputs(n, seed, offset, edges=False)
    w = np.random.default_rng(seed + 1).uniform(0.0, 1.0, n).astype(np.float32)
    return i.cur, i.grad, i.sdf, w


# ---------------------------------------------------------------- assemble
def _sums(p, g, w, r):
    """The sums over the given rows.  J is computed in the precision of p and g; w, r are fp64."""
    px, py, pz = (p[:, k] for k in range(3))
    gx, gy, gz = (g[:, k] for k in range(3))
    J = torch.stack([py * gz - pz * gy, pz * gx - px * gz, px * gy - py * gx, gx, gy, gz], 1).double()
    p, g = p.double().abs(), g.double().abs()
    px, py, pz = (p[:, k] for k in range(3))
    gx, gy, gz = (g[:, k] for k in range(3))
    Jh = torch.stack([py * gz + pz * gy, pz * gx + px * gz, px * gy + py * gx, gx, gy, gz], 1)
    wJ = w.unsqueeze(1) * J
    return NS(N=wJ.T @ J, g=-(wJ.T @ r), S=(w.unsqueeze(1) * Jh).T @ Jh, Sg=(w * r.abs()).unsqueeze(1).T @ Jh)


def normal_equations(points, grad, res, weight, dtype=torch.float64):
    """N[6,6], g[6] of `pings_reg_normal_equations` and their magnitude sums S[6,6], Sg[6] (fp64)."""
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a))
    o = _sums(t(points).to(dtype), t(grad).to(dtype), t(weight).double(), t(res).double())
    o.Sg = o.Sg.reshape(6)
    return o


def assemble(inp, st, dtype=torch.float64):
    """`inp`: the arrays of make_inputs; `st`: settings(flagset).  Returns valid[n] (bool), count, sum_w, sum_abs_r,
    sum_wr2, N[6,6], g[6], S[6,6], Sg[6], all fp64, unnormalised (the w / (2 mean w) of `F_WEIGHTED` is the step's)."""
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a))
    grad, std = t(inp.grad).to(dtype), t(inp.std).to(dtype)
    thr = lambda k: torch.tensor(st[k], dtype=dtype)     # the settings are fp32 numbers: exact in either precision
    gn = torch.sqrt((grad[:, 0] * grad[:, 0] + grad[:, 1] * grad[:, 1]) + grad[:, 2] * grad[:, 2])
    valid = t(inp.mask).bool() & (gn < thr("max_grad")) & (gn > thr("min_grad")) & (std < thr("max_std"))
    p, g, gn = t(inp.cur).to(dtype)[valid], grad[valid], gn[valid]
    s, lab = t(inp.sdf).to(dtype)[valid], t(inp.label).to(dtype)[valid]
    if st["flags"] & F_DIV_GRAD:
        s = s / gn
    r = s - lab
    w = torch.ones_like(r)
    if st["gm_dist"] > 0:
        w = w * (thr("gm_dist") / (thr("gm_dist") + r * r)) ** 2
    if st["gm_grad"] > 0:
        w = w * (thr("gm_grad") / (thr("gm_grad") + (gn - 1.0) ** 2)) ** 2
    if st["flags"] & F_NORMALS:
        unit = g / (gn.unsqueeze(-1) + 1e-7)
        nr = t(inp.normals).to(dtype)[valid]
        w = w * (0.5 + ((nr[:, 0] * unit[:, 0] + nr[:, 1] * unit[:, 1]) + nr[:, 2] * unit[:, 2]).abs())
    w, r = w.double(), r.double()
    o = _sums(p, g, w, r)
    o.Sg = o.Sg.reshape(6)
    o.valid, o.count = valid, int(valid.sum())
    o.sum_w, o.sum_abs_r, o.sum_wr2 = float(w.sum()), float(r.abs().sum()), float((w * r * r).sum())
    return o


def totals(o):
    """The 32 per-step totals in the kernel's layout: 21 upper-triangle entries of N, g, count, sum w, sum |r|, sum w r^2."""
    iu = np.triu_indices(6)
    return np.concatenate([o.N.numpy()[iu], o.g.numpy(), [o.count, o.sum_w, o.sum_abs_r, o.sum_wr2, 0.0]])


def total_bounds(o):
    """Magnitude sums in the same layout (entries 27..31: the sums themselves, all of positive terms)."""
    iu = np.triu_indices(6)
    return np.concatenate([o.S.numpy()[iu], o.Sg.numpy(), [0.0, o.sum_w, o.sum_abs_r, o.sum_wr2, 0.0]])


# ---------------------------------------------------------------- step
def normal_eq_from_totals(tot, weighted):
    """The 42 floats [N | g] the step kernel solves: the fp64 totals times count / (2 sum w) when weighted, rounded to fp32."""
    tot = np.asarray(tot, np.float64)
    c = tot[27] / (2.0 * tot[28]) if weighted else 1.0
    N = np.zeros((6, 6))
    N[np.triu_indices(6)] = c * tot[:21]
    N = N + np.triu(N, 1).T
    return np.concatenate([N.reshape(36), c * tot[21:27]]).astype(np.float32)


def expmap(v):
    """Rodrigues' formula in fp64 (utils/tracker.py:774-783); a zero vector gives NaN, as there."""
    v = np.asarray(v, np.float64)
    a = np.sqrt(v @ v)
    with np.errstate(invalid="ignore", divide="ignore"):
        x, y, z = v / a
    S = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    return np.eye(3) + S * np.sin(a) + (S @ S) * (1.0 - np.cos(a))


def damped(ng, lm_lambda):
    """N + lambda diag(N) in the precision N arrives in (fp32 from the kernels: `v + lambda * v`), lifted to fp64."""
    ng = np.asarray(ng)
    N = ng[:36].reshape(6, 6).copy()
    d = np.diag_indices(6)
    N[d] = N[d] + ng.dtype.type(lm_lambda) * N[d]
    return N.astype(np.float64)


def step(ng, lm_lambda, T=None):
    """implicit_reg's tail from [N | g] (fp32 or fp64 numpy, 42 numbers): t = solve(damped N, g) in fp64, dT = [expmap(t[:3]) |
    t[3:]], T_new = dT @ T.  Returns NS(t, dT, T, cond) with cond the 2-norm condition number of the damped matrix."""
    A = damped(ng, lm_lambda)
    t = np.linalg.solve(A, np.asarray(ng[36:], np.float64))
    dT = np.eye(4)
    dT[:3, :3], dT[:3, 3] = expmap(t[:3]), t[3:]
    return NS(t=t, dT=dT, T=None if T is None else dT @ np.asarray(T, np.float64), cond=float(np.linalg.cond(A, 2)))


def rot_deg(dT):
    return float(np.degrees(np.arccos(((dT[0, 0] + dT[1, 1]) + dT[2, 2] - 1.0) / 2.0)))


def tran_m(dT):
    return float(np.sqrt((dT[0, 3] * dT[0, 3] + dT[1, 3] * dT[1, 3]) + dT[2, 3] * dT[2, 3]))


def solve_tolerance(cond):
    """Relative error allowed between two fp64 solves of one system: both are backward stable, so each is within
    c * cond_2 * 2^-53 of the exact solution with c a small multiple of the dimension (6) times the pivot growth; 1e3
    covers c for both."""
    return 1e3 * cond * 2.0 ** -52
