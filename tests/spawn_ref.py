"""Helpers of tests/test_spawn_edges.py: the two stages of csrc/spawn.hip in plain fp64, with per-element fp32 bounds.

Reference.  `gather` and `activate` take the arguments of `pings_amd.spawn.gather` / `pings_amd.spawn.activate` and
restate the stages with torch operators in fp64, differentiable by autograd.  `test_spawn_edges.py` pins them to
`oracle/spawn_cpu.spawn_gaussians` (which the reference's G4 vectors pin) to 1e-12.

Bounds.  `gather_v`, `activate_v` and `backward_v` walk the operation sequence of the kernels once more, on pairs
(v, e): v the fp64 value, e a bound on |fp32 result - v|.  Inputs are fp32 numbers, so they start with e = 0.  With
u = 2^-24 one fp32 operation on operands that carry errors gives

    a + b :  e = (ea + eb)(1 + u) + u |v| + tiny                  (tiny = 2^-126: results flushed to zero)
    a * b :  e = (|a| eb + |b| ea + ea eb)(1 + u) + u |v| + tiny
    a / b :  e = (ea + |v| eb) / (|b| - eb) (1 + u) + u |v| + tiny
    f(a)  :  e = L(a, ea)(1 + r) + r |v| + tiny                   L: how far f moves over [a - ea, a + ea]

i.e. the magnitudes of the terms that enter an element times fp32 epsilon, carried through the sequence.  Nothing is
special-cased: for d = g c (1 - t t) at saturated tanh the subtraction 1 - t t carries the absolute error
2 |t| e_t + u t^2 + u |1 - t t| of its operands, about (2 ulps(tanh) + 1) 2^-23 however small 1 - t t is, and the
product turns it into that times |g c|; in the rotation's eps branch e / kNormEps divides the bound of e by 1e-12 as
it divides e.  A multiplication by a sign or by 2 is exact and adds nothing.  Constants of the kernel that are not
fp32 numbers (0.1, 1e-7, 1e-12) carry u |c|.

Accuracy of the device functions (the only numbers here that are not arithmetic):
  * sqrtf and the fp32 division are correctly rounded, u: the library is built with
    -fhip-fp32-correctly-rounded-divide-sqrt (pings_amd/build.py).
  * tanhf: 5 ulp, expf: 3 ulp.  Source: the OpenCL C specification, version 3.0, section 7.4 "Relative error as
    ULPs" (tanh <= 5 ulp, exp <= 3 ulp).  hipcc lowers tanhf / expf to ROCm's device library OCML
    (ROCm-Device-Libs, doc/OCML.md), which is written to that table.  One ulp is 2^-23 relative.

The bounds assume that fp32 and fp64 take the same branches.  `activate_v` returns every decision input with its
distance to the threshold and its bound, so that a test can require distance > bound (or distance == 0 where a value
sits on its threshold exactly in both precisions) instead of excluding elements.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

U = 2.0 ** -24
ULP = 2.0 ** -23
TINY = 2.0 ** -126
TANH_ULP = 5.0      # OpenCL C 3.0 section 7.4: tanh <= 5 ulp (OCML, the device library behind tanhf, follows that table)
EXP_ULP = 3.0       # OpenCL C 3.0 section 7.4: exp <= 3 ulp
K_NORM_EPS, K_THIN, K_RESIDUAL = 1e-12, 1e-7, 0.1     # csrc/spawn.hip: kNormEps, kThin, kResidual


def _d(t):
    return None if t is None else t.detach().double().cpu()


# ---------------------------------------------------------------- fp64 restatement (autograd)
def rotate(q, sgn, v):
    """sgn = -1: R(q)^T v, the reference's apply_quaternion_rotation; sgn = +1: R(q) v."""
    w, u = q[:, :1], sgn * q[:, 1:]
    t = 2.0 * torch.linalg.cross(u, v)
    return v + w * t + torch.linalg.cross(u, t)


def quat_mul(a, b):
    w1, x1, y1, z1 = a.unbind(1)
    w2, x2, y2, z2 = b.unbind(1)
    return torch.stack((w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                        w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2), dim=1)


def gather(geo_feature, color_feature, sel, position, orientation, color, free_mask, cam_origin, xy_only,
           view_concat, dist_concat, fc=None):
    """-> geo_in, col_in, pos, quat, base_color, free, view_dist[n,1] (None without cam_origin), in fp64."""
    n = int(sel.shape[0]) if sel is not None else int(position.shape[0])
    idx = sel.long() if sel is not None else torch.arange(n)
    pos, quat = position.double()[idx], orientation.double()[idx]
    base = None if color is None else color.double()[idx]
    free = None if free_mask is None else free_mask[idx]
    geo_in, col_in = geo_feature.double()[idx], color_feature.double()[idx]
    vdist = None
    if cam_origin is not None:
        v = pos - cam_origin.double().reshape(1, 3)
        if xy_only:
            v = torch.cat((v[:, :2], torch.zeros_like(v[:, 2:])), dim=1)
        vdist = v.norm(dim=1, keepdim=True)
        if dist_concat:
            geo_in = torch.cat((geo_in, vdist), dim=1)
        if view_concat:
            col_in = torch.cat((col_in, rotate(quat, +1.0, v / vdist)), dim=1)
    return geo_in, col_in, pos, quat, base, free, vdist


def activate(xyz_raw, rot_raw, scale_raw, alpha_raw, color_raw, pos, quat, base, dist_ratio, free, *, n, k,
             surfel, color_residual, alpha_filter_on, scale_filter_on, displacement_range, unit_scale, max_scale,
             scale_filter_thr):
    """The fields of `pings_amd.spawn.Spawned` in fp64, plus `keep` [n*k] (the filters' mask before compaction)."""
    nk = n * k
    sd = scale_raw.shape[1] // k
    rep = lambda t: t.double().repeat_interleave(k, dim=0)
    q = rep(quat)
    xyz = rep(pos) + rotate(q, -1.0, displacement_range * torch.tanh(xyz_raw.double().reshape(nk, 3)))
    r = torch.nn.functional.normalize(rot_raw.double().reshape(nk, 4), eps=K_NORM_EPS)
    rot = quat_mul(q, torch.nan_to_num(r, 0, 0))
    s_arg = scale_raw.double()
    if dist_ratio is not None:
        s_arg = s_arg + dist_ratio.double().reshape(n, 1)
    s = torch.clamp(unit_scale * torch.exp(s_arg), max=max_scale).reshape(nk, sd)
    scale = torch.cat((s[:, :2], torch.full((nk, 1), K_THIN, dtype=torch.float64)), dim=1) if surfel else s
    alpha = torch.tanh(alpha_raw.double()).reshape(nk, 1)
    c_raw = color_raw.double().reshape(nk, 3)
    if color_residual:
        color = torch.clamp(rep(base) + K_RESIDUAL * torch.tanh(c_raw), 0.0, 1.0)
    else:
        color = torch.sigmoid(c_raw)
    alpha_all = alpha.clone()
    keep = torch.ones(nk, dtype=torch.bool)
    if alpha_filter_on:
        keep &= alpha.detach().squeeze(1) > 0.0
    if scale_filter_on:
        keep &= (scale.detach() > scale_filter_thr).any(dim=1)
    gfree = None if free is None else free.repeat(k)[keep]      # the reference tiles the mask: Gaussian g <- free[g % n]
    return SimpleNamespace(xyz=xyz[keep], scale=scale[keep], rot=rot[keep], alpha=alpha[keep], color=color[keep],
                           alpha_all=alpha_all, free_mask=gfree, count=int(keep.sum()), keep=keep)


# ---------------------------------------------------------------- (value, bound) arithmetic
class V:
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = torch.as_tensor(v, dtype=torch.float64).detach()
        self.e = torch.zeros_like(self.v) if e is None else e

    @staticmethod
    def const(c):
        """A constant of the kernel that is written in decimal and rounded to fp32 by the compiler."""
        return V(c, torch.tensor(U * abs(c), dtype=torch.float64))

    def exact(self, c):
        """Times a sign or a power of two."""
        return V(self.v * c, self.e * abs(c))

    def __add__(self, o):
        o = _lift(o)
        return _op(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = _lift(o)
        return _op(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return _lift(o) - self

    def __mul__(self, o):
        o = _lift(o)
        return _op(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e)

    __radd__, __rmul__ = __add__, __mul__

    def __truediv__(self, o):
        o = _lift(o)
        v = self.v / o.v
        return _op(v, (self.e + v.abs() * o.e) / (o.v.abs() - o.e))

    def __rtruediv__(self, o):
        return _lift(o) / self

    def where(self, mask, other):
        other = _lift(other)
        return V(torch.where(mask, self.v, other.v), torch.where(mask, self.e, other.e))


def _lift(x):
    return x if isinstance(x, V) else V(x)


def _op(v, e_in, rel=U):
    return V(v, e_in * (1.0 + rel) + rel * v.abs() + TINY)


def v_tanh(a):
    return _op(torch.tanh(a.v), a.e, TANH_ULP * ULP)                    # |tanh'| <= 1


def v_exp(a):
    x = torch.exp(a.v)
    return _op(x, x * torch.expm1(a.e), EXP_ULP * ULP)


def v_sqrt(a):
    s, lo = a.v.sqrt(), (a.v - a.e).clamp_min(0.0).sqrt()
    return _op(s, torch.minimum(a.e.sqrt(), a.e / (s + lo).clamp_min(TINY)))     # both bound |sqrt(x) - sqrt(y)|


def v_max(a, b):
    b = _lift(b)
    return V(torch.maximum(a.v, b.v), torch.maximum(a.e, b.e))


def v_rotate(q, sgn, v):
    """`rotate` of csrc/spawn.hip on lists of V: q = [w, x, y, z], v = [x, y, z]."""
    w, (ux, uy, uz) = q[0], [c.exact(sgn) for c in q[1:]]
    vx, vy, vz = v
    tx, ty, tz = (uy * vz - uz * vy).exact(2.0), (uz * vx - ux * vz).exact(2.0), (ux * vy - uy * vx).exact(2.0)
    return [vx + w * tx + (uy * tz - uz * ty), vy + w * ty + (uz * tx - ux * tz), vz + w * tz + (ux * ty - uy * tx)]


def _cols(t, rows=None):
    t = _d(t) if rows is None else _d(t).reshape(rows, -1)
    return [V(c) for c in t.unbind(1)]


def _stack(vs):
    return torch.stack([x.v for x in vs], dim=1), torch.stack([x.e.expand_as(x.v) for x in vs], dim=1)


def gather_v(sel, position, orientation, cam_origin, xy_only):
    """(value, bound) of view_dist [n, 1] and of the view direction in the neural point's frame [n, 3]."""
    n = int(sel.shape[0]) if sel is not None else int(position.shape[0])
    idx = sel.long().cpu() if sel is not None else torch.arange(n)
    p, q, cam = _cols(_d(position)[idx]), _cols(_d(orientation)[idx]), _d(cam_origin).reshape(3)
    v = [p[c] - V(cam[c]) for c in range(3)]
    if xy_only:
        v[2] = V(torch.zeros(n, dtype=torch.float64))
    dist = v_sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    d = v_rotate(q, +1.0, [c / dist for c in v])
    return (dist.v.reshape(n, 1), dist.e.reshape(n, 1)), _stack(d)


def _scales_v(scale_raw, dist_ratio, n, k, sd, unit_scale):
    """e = unit exp(raw + dr), [n*k] per column."""
    cols = _cols(scale_raw, n * k)
    if dist_ratio is None:
        return [V(unit_scale) * v_exp(c) for c in cols]
    dr = V(_d(dist_ratio).reshape(n).repeat_interleave(k))
    return [V(unit_scale) * v_exp(c + dr) for c in cols]


def _unit_rot_v(rot_raw, nk):
    r = _cols(rot_raw, nk)
    nr = v_sqrt(((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3])
    return r, nr


def activate_v(xyz_raw, rot_raw, scale_raw, alpha_raw, color_raw, pos, quat, base, dist_ratio, free, *, n, k,
               surfel, color_residual, alpha_filter_on, scale_filter_on, displacement_range, unit_scale, max_scale,
               scale_filter_thr):
    """{name: (value, bound)} of xyz, rot, scale, alpha, color for all n*k Gaussians (before compaction), and under
    "decisions" {name: (distance to the threshold, bound)} of every input of a branch the kernels take."""
    nk = n * k
    sd = scale_raw.shape[1] // k
    rep = lambda t: _d(t).repeat_interleave(k, dim=0)
    q = _cols(rep(quat))
    out, dec = {}, {}
    # position
    t = [v_tanh(c) for c in _cols(xyz_raw, nk)]
    o = v_rotate(q, -1.0, [V(displacement_range) * c for c in t])
    out["xyz"] = _stack([pc + oc for pc, oc in zip(_cols(rep(pos)), o)])
    # rotation
    r, nr = _unit_rot_v(rot_raw, nk)
    eps = V.const(K_NORM_EPS)
    dec["rot_eps"] = ((nr.v - K_NORM_EPS).abs(), nr.e + eps.e)
    nrm = v_max(nr, eps)
    nan = torch.isnan(nr.v)
    r = [(c / nrm).where(~nan, 0.0) for c in r]                      # nan_to_num of a row whose norm is NaN
    out["rot"] = _stack([q[0] * r[0] - q[1] * r[1] - q[2] * r[2] - q[3] * r[3],
                         q[0] * r[1] + q[1] * r[0] + q[2] * r[3] - q[3] * r[2],
                         q[0] * r[2] - q[1] * r[3] + q[2] * r[0] + q[3] * r[1],
                         q[0] * r[3] + q[1] * r[2] - q[2] * r[1] + q[3] * r[0]])
    # scale
    e = _scales_v(scale_raw, dist_ratio, n, k, sd, unit_scale)
    s = [c.where(c.v <= max_scale, max_scale) for c in e]
    dec["scale_max"] = tuple(torch.stack(x, dim=1) for x in zip(*[((c.v - max_scale).abs(), c.e) for c in e]))
    if surfel:
        s = s[:2] + [V(torch.full((nk,), K_THIN, dtype=torch.float64), torch.full((nk,), U * K_THIN, dtype=torch.float64))]
    out["scale"] = _stack(s)
    if scale_filter_on:
        cols = s[:2] if surfel else s                               # the thin column is far below any threshold
        dec["scale_thr"] = tuple(torch.stack(x, dim=1) for x in zip(*[((c.v - scale_filter_thr).abs(), c.e)
                                                                      for c in cols]))
    # opacity
    a = v_tanh(V(_d(alpha_raw).reshape(nk)))
    out["alpha"] = (a.v.reshape(nk, 1), a.e.reshape(nk, 1))
    if alpha_filter_on:
        dec["alpha_keep"] = (a.v.abs(), a.e)
    # colour
    if color_residual:
        pre = [bc + V.const(K_RESIDUAL) * v_tanh(c) for bc, c in zip(_cols(rep(base)), _cols(color_raw, nk))]
        dec["color_lo"] = tuple(torch.stack(x, dim=1) for x in zip(*[(c.v.abs(), c.e) for c in pre]))
        dec["color_hi"] = tuple(torch.stack(x, dim=1) for x in zip(*[((c.v - 1.0).abs(), c.e) for c in pre]))
        col = [c.where(c.v >= 0.0, 0.0).where(c.v <= 1.0, 1.0) for c in pre]
    else:
        col = [1.0 / (1.0 + v_exp(V(-c.v))) for c in _cols(color_raw, nk)]
    out["color"] = _stack(col)
    out["decisions"] = dec
    return out


def backward_v(xyz_raw, rot_raw, scale_raw, alpha_raw, color_raw, quat, base, dist_ratio, keep, g, *, n, k, surfel,
               color_residual, displacement_range, unit_scale, max_scale, **_):
    """`backward_kernel` on (value, bound) pairs.  `g` maps xyz / scale / rot / alpha / color / alpha_all to the
    upstream gradient of all n*k Gaussians ([n*k, d], rows of dropped Gaussians are never read) or to None.
    -> {xyz_raw, rot_raw, scale_raw, alpha_raw, color_raw: (value, bound)}, shaped as the raws."""
    nk = n * k
    sd = scale_raw.shape[1] // k
    keep = keep.cpu()
    zero = torch.zeros(nk, dtype=torch.float64)

    def up(name, d):
        t = g.get(name)
        return [V(zero)] * d if t is None else [V(torch.where(keep, c, zero)) for c in _d(t).reshape(nk, d).unbind(1)]

    def done(vs, d):
        v, e = _stack([x.where(keep, 0.0) for x in vs])
        return v.reshape(n, d * k), e.reshape(n, d * k)

    q = _cols(_d(quat).repeat_interleave(k, dim=0))
    out = {}
    # opacity: both terms, and the only one that reaches a dropped Gaussian
    a = v_tanh(V(_d(alpha_raw).reshape(nk)))
    ga_all, ga = g.get("alpha_all"), g.get("alpha")
    terms = ([V(_d(ga_all).reshape(nk))] if ga_all is not None else []) + (up("alpha", 1) if ga is not None else [])
    gsum = terms[0] + terms[1] if len(terms) == 2 else terms[0] if terms else V(zero)
    if len(terms) == 2:     # a dropped Gaussian adds nothing to g_alpha_all: no rounding there
        gsum = gsum.where(keep, terms[0])
    d_a = gsum * (1.0 - a * a)
    out["alpha_raw"] = (d_a.v.reshape(n, k), d_a.e.reshape(n, k))
    # position
    b = v_rotate(q, +1.0, up("xyz", 3)) if g.get("xyz") is not None else [V(zero)] * 3
    t = [v_tanh(c) for c in _cols(xyz_raw, nk)]
    out["xyz_raw"] = done([V(displacement_range) * (1.0 - tc * tc) * bc for tc, bc in zip(t, b)], 3)
    # rotation
    o = up("rot", 4)
    e = [q[0] * o[0] + q[1] * o[1] + q[2] * o[2] + q[3] * o[3], q[0] * o[1] - q[1] * o[0] - q[2] * o[3] + q[3] * o[2],
         q[0] * o[2] + q[1] * o[3] - q[2] * o[0] - q[3] * o[1], q[0] * o[3] - q[1] * o[2] + q[2] * o[1] - q[3] * o[0]]
    r, nr = _unit_rot_v(rot_raw, nk)
    live = nr.v > K_NORM_EPS
    inv = 1.0 / nr.where(live, 1.0)
    u = [c * inv for c in r]
    dot = ((u[0] * e[0] + u[1] * e[1]) + u[2] * e[2]) + u[3] * e[3]
    eps = V.const(K_NORM_EPS)
    out["rot_raw"] = done([((ec - uc * dot) * inv).where(live, ec / eps) for ec, uc in zip(e, u)], 4)
    # scale
    ev = _scales_v(scale_raw, dist_ratio, n, k, sd, unit_scale)
    gs = g.get("scale")
    od = 3 if surfel else sd
    gs = None if gs is None else _d(gs).reshape(nk, od)
    d_s = []
    for c in range(sd):
        has = gs is not None and (not surfel or c < 2)
        go = V(torch.where(keep, gs[:, c], zero)) if has else V(zero)
        d_s.append((go * ev[c]).where(ev[c].v <= max_scale, 0.0))
    out["scale_raw"] = done(d_s, sd)
    # colour
    go, d_c = up("color", 3), []
    for c, raw in enumerate(_cols(color_raw, nk)):
        if color_residual:
            tc = v_tanh(raw)
            pre = V(_d(base).repeat_interleave(k, dim=0)[:, c]) + V.const(K_RESIDUAL) * tc
            d_c.append((go[c] * V.const(K_RESIDUAL) * (1.0 - tc * tc)).where((pre.v >= 0.0) & (pre.v <= 1.0), 0.0))
        else:
            s = 1.0 / (1.0 + v_exp(V(-raw.v)))
            d_c.append(go[c] * s * (1.0 - s))
    out["color_raw"] = done(d_c, 3)
    return out


def worst_ratio(got, ref, E):
    """max |got - ref| / E over the elements (an element with E = 0 has to be exact)."""
    got, ref = _d(got).reshape(ref.shape), ref.detach()
    assert torch.isfinite(got).all()
    if not ref.numel():
        return 0.0
    err = (got - ref).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / E).max())
