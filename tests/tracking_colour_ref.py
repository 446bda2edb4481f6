"""fp64 restatement of the tracker's colour branches, for tests/test_tracking_colour.py and
tests/test_color_query_edges.py.

* `colour_query`: the colour head of Tracker.query_source_points (utils/tracker.py:328-336) on
  oracle.sdf_cpu.NeuralPointMap: sigmoid(MLP.mlp(colour features)), the IDW sum, one autograd pass per channel for the
  Jacobian; and the queries whose Jacobian fp32 cannot decide (a hidden pre-activation within rounding of its kink).
* `step`: registration_step (:353-605) with the photometric term (implicit_color_reg, :692-737) and the
  colour-consistency weight, written like tests/tracking_ref.py:step against an injected query.
* `tracking`: the loop of tests/tracking_ref.py with that step in place of its own.
* `assemble_colour`: the sums of `pings_reg_assemble_color` from plain arrays with their magnitude sums, on top of
  tests/tracker_edges_ref.py, and the rounding counts of the bound.

Bound of `pings_reg_assemble_color` (u = 2^-24; everything relative to magnitude sums, as tests/test_tracker_edges.py).
The geometric term w J_a J_b carries 16 roundings (12 weight chain, 3 cross product, 1 spare).  New:
  intensity   (0.144 c0 + 0.299 c1) + 0.587 c2: each term passes the rounding of its coefficient to fp32, its product
              and at most two additions: 4, relative to I^ = 0.144 |c0| + 0.299 |c1| + 0.587 |c2| (the rows of the
              Jacobian have mixed signs, so I^ and not |I| is the scale).
  PHOTO       an entry of J_c = [p x grad I, grad I]: 4 + 3 (cross product) = 7 relative to its magnitude built from
              grad I^; a term lambda w J_c,a J_c,b: 12 (w) + 14 + 1 (lambda, an fp32 number) = 27; a term
              lambda w r_c J_c,a: r_c = I_pred - I_src has 4 + 1 roundings relative to r^ = I_pred^ + I_src^ (it cancels),
              so 12 + 7 + 5 + 1 = 25 with r^ in the magnitude sum.  28 covers both and the geometric 16.
  CONSIST     d = |I_src - I_pred| has absolute error (4 I_src + 4 I_pred + d) u <= 9 u for colours in [0, 1];
              exp(-d) turns it into a relative error, expf adds its own 2, the product with w 1: 12 more, 16 + 12 = 28
              on every sum that carries w.
  photo_part  sum |r_c|: 5 u sum r^.
So every sum is held to 28 u (+ n 2^-52 for the fp64 accumulation) of its magnitude sum, photo_part to 5 u."""
from types import SimpleNamespace as NS

import numpy as np
import torch
import torch.nn.functional as F

import tracker_edges_ref as E
import tracking_ref as ref
from oracle import sdf_cpu, tracker_cpu

PHOTO, CONSIST = 1, 2            # pings_amd._abi.REG_COLOR_*
COLOUR_ROUNDINGS = 28
PHOTO_PART_ROUNDINGS = 5
KINK_ULPS = 16                   # |pre| below 16 * 2^-24 * (sum |W1| |in| + |b1|): fp32 cannot decide the ReLU
KINK_CAP = 0.005                 # at most 0.5 % of a batch may be undecidable


def cpu_colour_decoder(st, prefix="cdec."):
    p = [torch.as_tensor(np.asarray(st[prefix + k])).double() for k in ("layers.0.weight", "layers.0.bias",
                                                                         "lout.weight", "lout.bias")]
    return sdf_cpu.MLP(*p)


def random_decoder(Fc, H, C, seed, levels=1):
    """Seeded colour decoder with nn.Linear's default init: state dict in the layout of the fixtures' `cdec.*`."""
    torch.manual_seed(seed)
    dims = [Fc + 3] + [H] * levels
    st = {}
    for i in range(levels):
        l = torch.nn.Linear(dims[i], dims[i + 1])
        st[f"cdec.layers.{i}.weight"], st[f"cdec.layers.{i}.bias"] = l.weight.detach().numpy(), l.bias.detach().numpy()
    lo = torch.nn.Linear(H, C)
    st["cdec.lout.weight"], st["cdec.lout.bias"] = lo.weight.detach().numpy(), lo.bias.detach().numpy()
    return st


def colour_query(npm, cdec, x, want_jac=True, query_locally=True):
    """NS(color[B,C], jac[B,C,3] | None, flagged[B] bool, counts[B], valid_in_topk[B]) in the map's precision."""
    xq = x.clone().requires_grad_(True)
    _, cf, w, cnt, _ = npm.query_feature(xq, accumulate_stability=False, query_locally=query_locally,
                                         query_color_feature=True, use_only_valid_points=True)
    pre = F.linear(cf, cdec.W1, cdec.b1)
    col = torch.sigmoid(F.linear(F.relu(pre), cdec.W2, cdec.b2))
    if not npm.weighted_first:
        col = torch.sum(col * w, dim=1)
    margin = KINK_ULPS * 2.0 ** -24 * (F.linear(cf.abs(), cdec.W1.abs()) + cdec.b1.abs())
    flagged = (pre.abs() < margin).reshape(x.shape[0], -1).any(dim=1)
    jac = None
    if want_jac:
        jac = torch.stack([torch.autograd.grad(col[:, c].sum(), xq, retain_graph=True)[0]
                           for c in range(col.shape[1])], 1)
    return NS(color=col.detach(), jac=jac, flagged=flagged.detach(), counts=cnt,
              in_topk=(w.detach().reshape(x.shape[0], -1) > 0).sum(dim=1))


def cpu_query(npm, dec, cdec, bs, nn_k, want_jac):
    def q(points):
        outs = []
        for h in range(0, points.shape[0], bs):
            s, g, m, _, std = tracker_cpu.query_source_points(npm, dec, points[h:h + bs], mask_min_nn_count=nn_k)
            c = colour_query(npm, cdec, points[h:h + bs], want_jac)
            outs.append((s, g, m, std, c.color, c.jac if want_jac else c.color.new_zeros(c.color.shape + (3,))))
        return tuple(torch.cat(t) for t in zip(*outs))
    return q


def intensity(c):
    """color_to_intensity (utils/tools.py:723) on [n,3] or [n,3,3]; the coefficients and their order as written there."""
    return ((0.144 * c[:, 0] + 0.299 * c[:, 1]) + 0.587 * c[:, 2]).unsqueeze(1)


def expmap(v):
    a = v.norm()
    x, y, z = (v / a).tolist()
    S = torch.tensor([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]], dtype=v.dtype, device=v.device)
    return torch.eye(3, dtype=v.dtype, device=v.device) + S * torch.sin(a) + (S @ S) * (1.0 - torch.cos(a))


def solve_colour(points, grad, res, w, colour_grad, colour_res, lam, lm_lambda):
    """implicit_color_reg (utils/tracker.py:692-737): one intensity channel, N = N_geo + lam N_col before damping."""
    J = torch.cat([torch.linalg.cross(points, grad), grad], -1)
    N = J.T @ (w * J)
    g = -(J * w).T @ res
    Jc = torch.cat([torch.linalg.cross(points, colour_grad), colour_grad], -1)
    N = N + lam * (Jc.T @ (w * Jc))
    g = g + lam * (-(Jc * w).T @ colour_res)
    N = N + lm_lambda * torch.diag(torch.diag(N))
    t = torch.linalg.inv(N.double()) @ g.double()
    T = torch.eye(4, dtype=torch.float64, device=points.device)
    T[:3, :3] = expmap(t[:3])
    T[:3, 3] = t[3:]
    return T


def step(query, solve, cfg, points, normals, labels, colours, GM_dist, GM_grad, lm_lambda):
    """One registration step with colours: (dT, valid count, residual mean in cm, valid mask, photometric residual mean
    | None).  query(points) -> (sdf, grad, mask, std, colour[n,C], jac[n,C,3])."""
    sdf, grad, mask, std, col, jac = query(points)
    gnorm = grad.norm(dim=-1)
    max_std = cfg.surface_sample_range_m * cfg.max_sdf_std_ratio
    valid = mask & (gnorm < cfg.reg_max_grad_norm) & (gnorm > cfg.reg_min_grad_norm) & (std < max_std)
    p = points[valid]
    n = p.shape[0]
    if n < 10:
        return torch.eye(4, dtype=torch.float64, device=points.device), n, 0.0, valid, 0.0
    g, gn, s, lab = grad[valid], gnorm[valid], sdf[valid], labels[valid]
    if cfg.reg_dist_div_grad_norm:
        s = s / gn
    r = s - lab
    res_cm = float(r.abs().mean()) * 100.0
    w = torch.ones_like(r)
    weighted = False
    if GM_dist is not None:
        w = w * (GM_dist / (GM_dist + r * r)) ** 2
        weighted = True
    if GM_grad is not None:
        w = w * (GM_grad / (GM_grad + (gn - 1.0) ** 2)) ** 2
        weighted = True
    if normals is not None:
        unit = g / (gn.unsqueeze(-1) + 1e-7)
        w = w * (0.5 + (normals[valid] * unit).sum(dim=1).abs())
        weighted = True
    C = int(cfg.color_channel)
    cs, cp = colours[valid, :C].to(p.dtype), col[valid, :C]
    if C == 3:
        cs, cp = intensity(cs), intensity(cp)
    photo = bool(cfg.photometric_loss_on)
    if photo:
        cj = jac[valid, :C]
        if C == 3:
            cj = intensity(cj)
    elif cfg.consist_wieght_on:          # an elif in the reference: ignored when the photometric term is on
        w = w * torch.exp(-torch.mean((cs - cp).abs(), dim=-1))
        weighted = True
    if weighted:
        w = w / (2.0 * w.mean())
    if not photo:
        return solve(p, g, r, w.unsqueeze(1), lm_lambda), n, res_cm, valid, None
    rc = cp - cs
    dT = solve_colour(p, g, r, w.unsqueeze(1), cj[:, 0], rc[:, 0], float(cfg.photometric_loss_weight), lm_lambda)
    return dT, n, res_cm, valid, float(rc.abs().mean())


def tracking(query, solve, cfg, source_points, init_pose, colours, normals=None, labels=None):
    """tests/tracking_ref.py:tracking with the colour step: (T, valid_flag, trace, photometric residuals)."""
    photo = []

    def colour_step(q, s, cfg_, points, nrm, lab, GMd, GMg, lm):
        dT, n, res, valid, ph = step(q, s, cfg_, points, nrm, lab, colours, GMd, GMg, lm)
        photo.append(ph)
        return dT, n, res, valid

    saved = ref.step
    ref.step = colour_step
    try:
        T, valid, trace = ref.tracking(query, solve, cfg, source_points, init_pose, normals=normals, labels=labels)
    finally:
        ref.step = saved
    return T, valid, trace, photo


# ---------------------------------------------------------------- pings_reg_assemble_color from plain arrays
def make_colours(inp, C, seed, equal_rows=8):
    """Seeded colours in [0, 1], predictions and Jacobian rows for the points of tracker_edges_ref.make_inputs: the first
    `equal_rows` valid-or-not rows predict the measured colour exactly (w_colour = 1), and the first invalid row carries
    NaN colours (they must not reach the sums)."""
    rng = np.random.default_rng(seed)
    n = inp.n
    src = rng.uniform(0.0, 1.0, (n, C)).astype(np.float32)
    pred = np.clip(src + rng.normal(0.0, 0.15, (n, C)), 0.0, 1.0).astype(np.float32)
    jac = rng.normal(0.0, 0.5, (n, C, 3)).astype(np.float32)
    pred[:min(equal_rows, n)] = src[:min(equal_rows, n)]
    return NS(src=src, pred=pred, jac=jac, C=C)


def poison_invalid(col, valid):
    bad = np.flatnonzero(~np.asarray(valid))
    if bad.size:
        col.src[bad[0]] = np.nan
        col.pred[bad[0]] = np.nan
        col.jac[bad[0]] = np.nan
    return bad[:1]


def _i(c, dtype):
    """Intensity of [m,C] or [m,C,3] in `dtype` and its magnitude in fp64."""
    c = torch.as_tensor(np.ascontiguousarray(c))
    if c.shape[1] == 1:
        return c[:, 0].to(dtype), c[:, 0].double().abs()
    v = c.to(dtype)
    a = c.double().abs()
    return (0.144 * v[:, 0] + 0.299 * v[:, 1]) + 0.587 * v[:, 2], (0.144 * a[:, 0] + 0.299 * a[:, 1]) + 0.587 * a[:, 2]


def assemble_colour(inp, col, st, mode, lam, dtype=torch.float64):
    """tracker_edges_ref.assemble with the colour terms: the same fields, plus `photo` = sum |r_c| and `photo_mag` =
    sum (I_pred^ + I_src^).  `lam` is an fp32 number.  Products and sums are fp64, per-point quantities `dtype`."""
    base = E.assemble(inp, st, dtype)
    valid = base.valid
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a))
    grad = t(inp.grad).to(dtype)
    gn = torch.sqrt((grad[:, 0] * grad[:, 0] + grad[:, 1] * grad[:, 1]) + grad[:, 2] * grad[:, 2])[valid]
    p, g = t(inp.cur).to(dtype)[valid], grad[valid]
    s, lab = t(inp.sdf).to(dtype)[valid], t(inp.label).to(dtype)[valid]
    thr = lambda k: torch.tensor(st[k], dtype=dtype)
    if st["flags"] & E.F_DIV_GRAD:
        s = s / gn
    r = s - lab
    w = torch.ones_like(r)
    if st["gm_dist"] > 0:
        w = w * (thr("gm_dist") / (thr("gm_dist") + r * r)) ** 2
    if st["gm_grad"] > 0:
        w = w * (thr("gm_grad") / (thr("gm_grad") + (gn - 1.0) ** 2)) ** 2
    if st["flags"] & E.F_NORMALS:
        unit = g / (gn.unsqueeze(-1) + 1e-7)
        nr = t(inp.normals).to(dtype)[valid]
        w = w * (0.5 + ((nr[:, 0] * unit[:, 0] + nr[:, 1] * unit[:, 1]) + nr[:, 2] * unit[:, 2]).abs())
    v = valid.numpy()
    i_src, m_src = _i(col.src[v], dtype)
    i_pred, m_pred = _i(col.pred[v], dtype)
    rc = i_pred - i_src
    if mode == CONSIST:
        w = w * torch.exp(-(i_src - i_pred).abs())
    w, r, rc = w.double(), r.double(), rc.double()
    o = E._sums(p, g, w, r)
    if mode == PHOTO:
        gi, gm = _i(col.jac[v], dtype)                   # [m,3] each
        wl = w * float(lam)
        px, py, pz = (p[:, k] for k in range(3))
        cx, cy, cz = (gi[:, k] for k in range(3))
        J = torch.stack([py * cz - pz * cy, pz * cx - px * cz, px * cy - py * cx, cx, cy, cz], 1).double()
        pa = p.double().abs()
        px, py, pz = (pa[:, k] for k in range(3))
        cx, cy, cz = (gm[:, k] for k in range(3))
        Jh = torch.stack([py * cz + pz * cy, pz * cx + px * cz, px * cy + py * cx, cx, cy, cz], 1)
        wJ = wl.unsqueeze(1) * J
        o.N = o.N + wJ.T @ J
        o.g = o.g - wJ.T @ rc
        o.S = o.S + (wl.unsqueeze(1) * Jh).T @ Jh
        o.Sg = o.Sg + (wl * (m_pred + m_src)).unsqueeze(1).T @ Jh
    o.Sg = o.Sg.reshape(6)
    o.valid, o.count = valid, int(valid.sum())
    o.sum_w, o.sum_abs_r, o.sum_wr2 = float(w.sum()), float(r.abs().sum()), float((w * r * r).sum())
    o.photo, o.photo_mag = float(rc.abs().sum()), float((m_pred + m_src).sum())
    return o
