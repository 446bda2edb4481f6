"""Gaussian-space loss block of the mapper's joint iteration on the HIP device (csrc/gauss_loss.hip).

`gaussian_losses(mapper, render_pkg, ...)` evaluates what `Mapper.joint_gsdf_mapping` computes inline at
utils/mapper.py:1331-1483 — opacity, opacity entropy, isotropy, area, SDF consistency, SDF-normal consistency and
invalid opacity — without a single host wait: the constraint count, the sample, the valid-gradient count and every
masked mean stay on the device.  The seven values come back un-weighted; the caller keeps the lambdas:

    G = gaussian_losses(self, render_pkg, gs_type=self.config.gs_type, ...)
    opacity_loss = G.opacity * self.config.lambda_opacity          # and so on

The sample is a uniform subset of min(count, bs * gaussian_bs_ratio) constrained Gaussians drawn with device random
keys (the generator's stream, not the reference's CPU `randperm`: the draws differ, the distribution is the same).
Gradients reach the render_pkg tensors, `local_geo_features` and the SDF decoder; the SDF-normal term's gradient
reaches the query points through H_S(x) v (`pings_sdf_hvp_x`).
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _abi, _lib
from . import neural_points as _np

GS_TYPES = {"gaussian_surfel": (2, 3, 2), "3d_gs": (3, 3, 3), "2d_gs": (2, 2, 2)}   # ncols, scale columns, voxel power
F_OPACITY, F_ENT, F_ISO, F_AREA, F_SDF = 1, 2, 4, 8, 16


class GaussianLosses(NamedTuple):
    opacity: torch.Tensor           # -mean(alpha_all[alpha_all < min_alpha]), 0 when no alpha is below
    opacity_ent: torch.Tensor       # opacity_entropy_loss(|alpha_all|)
    isotropic: torch.Tensor         # mean |s - mean_c s| over the sampled scales (:2 or :3 columns)
    area: torch.Tensor              # mean product of the scale columns / voxel^2 (voxel^3 for 3d_gs)
    sdf_cons: torch.Tensor          # mean |S(x) - label| over the valid rows (NaN when none, as torch)
    sdf_normal_cons: torch.Tensor   # mean 1 - <dS/dx / (|dS/dx| + 1e-7), n> over the valid rows
    invalid_opacity: torch.Tensor   # mean alpha of the samples whose unshifted row is not valid (NaN when none)
    counts: torch.Tensor            # float64 [5]: #alpha_all < min_alpha, constraint count, S, valid rows, invalid


def _carve(dev, spec):
    """One allocation for a list of (name, dtype, numel): views aligned to 256 bytes."""
    offs, off = [], 0
    for _, dt, n in spec:
        es = torch.empty((), dtype=dt).element_size()
        offs.append(off)
        off += (n * es + 255) // 256 * 256
    buf = torch.empty(max(off, 256), dtype=torch.uint8, device=dev)
    out = {}
    for (name, dt, n), o in zip(spec, offs):
        es = torch.empty((), dtype=dt).element_size()
        out[name] = buf[o:o + n * es].view(dt)
    return buf, out


def _f32(t):
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    return t if t.is_contiguous() else t.contiguous()


class _Block(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, rot, scale, alpha, alpha_all, feats, W1, b1, W2, b2, st):
        L = _lib.lib()
        dev = xyz.device
        a = st["args"]
        P, cap, R = int(a.P), int(a.cap), int(a.R)
        rows = (1 + R) * cap
        sdf_on = bool(a.flags & F_SDF)
        nnk = st["nnk"]
        spec = [("keys", torch.int32, P), ("part", torch.float64, 1024), ("meta", torch.int32, 8),
                ("idx", torch.int32, cap), ("normal", torch.float32, 3 * cap), ("queries", torch.float32, 3 * rows),
                ("label", torch.float32, rows)]
        if sdf_on:
            spec += [("sdf", torch.float32, rows), ("grad", torch.float32, 3 * rows), ("nn", torch.int64, rows),
                     ("valid", torch.uint8, rows), ("nidx", torch.int64, rows * nnk), ("w", torch.float32, rows * nnk),
                     ("gidx", torch.int64, rows * nnk)]
        buf, B = _carve(dev, spec)
        # the outputs live in a small buffer of their own: a caller holding the losses does not keep the workspace
        res = torch.empty(9, dtype=torch.float64, device=dev)
        B["counts"], B["losses"] = res[:5], res[5:].view(torch.float32)[:7]
        keep = {"xyz": _f32(xyz), "rot": _f32(rot), "scale": _f32(scale), "alpha": _f32(alpha),
                "alpha_all": _f32(alpha_all)}
        for k, t in keep.items():
            setattr(a, k, t.data_ptr() if t.numel() else None)
        for k in ("keys", "part", "meta", "idx", "normal", "queries", "label", "losses", "counts") + \
                (("sdf", "grad", "nn", "valid") if sdf_on else ()):
            setattr(a, k, B[k].data_ptr())
        stream = _lib.stream_ptr(dev)
        _lib.check(L.pings_gauss_loss_select(C.byref(a), stream), "pings_gauss_loss_select")
        _lib.check(L.pings_gauss_loss_prepare(C.byref(a), stream), "pings_gauss_loss_prepare")
        if sdf_on:
            m, dec = st["map"], st["dec"]
            _lib.check(L.pings_sdf_forward(
                C.byref(m.c), C.byref(dec), st["feats_c"].data_ptr(), st["pts"].data_ptr(),
                st["quat"].data_ptr(), None, int(st["after_pgo"]), B["queries"].data_ptr(), rows, B["sdf"].data_ptr(),
                B["grad"].data_ptr(), B["nn"].data_ptr(), None, B["nidx"].data_ptr(), B["w"].data_ptr(), None,
                B["gidx"].data_ptr(), stream), "pings_sdf_forward")
        _lib.check(L.pings_gauss_loss_reduce(C.byref(a), stream), "pings_gauss_loss_reduce")
        ctx.st, ctx.buf, ctx.B, ctx.keep = st, buf, B, keep
        ctx.shapes = [t.shape for t in (xyz, rot, scale, alpha, alpha_all)]
        ctx.need = [t is not None and t.requires_grad for t in (xyz, rot, scale, alpha, alpha_all, feats, W1, b1, W2, b2)]
        # saved for torch's version check: an in-place change to an input before backward raises, as for any node
        ctx.save_for_backward(xyz, rot, scale, alpha, alpha_all, feats, W1, b1, W2, b2)
        ctx.mark_non_differentiable(B["counts"])
        return tuple(B["losses"].unbind(0)) + (B["counts"],)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        L = _lib.lib()
        ctx.saved_tensors                       # raises if an input was modified in place since the forward
        st, B = ctx.st, ctx.B
        a = st["args"]
        gl = grads[:7]
        dev = B["losses"].device
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        g = torch.stack([zero if x is None else x.to(torch.float32) for x in gl])
        P, Na, cap, R = int(a.P), int(a.Na), int(a.cap), int(a.R)
        rows = (1 + R) * cap
        sdf_on = bool(a.flags & F_SDF)
        sc = int(a.scale_cols)
        spec = [("d_xyz", torch.float32, 3 * P), ("d_rot", torch.float32, 4 * P), ("d_scale", torch.float32, sc * P),
                ("d_alpha", torch.float32, P), ("d_alpha_all", torch.float32, Na)]
        feats, dec = st["feats"], st["dec"]
        if sdf_on:
            F, H, nnk = int(dec.feat_dim), int(dec.hidden), st["nnk"]
            nrows = feats.shape[0]
            spec += [("ds", torch.float32, rows), ("v", torch.float32, 3 * rows), ("dn", torch.float32, 3 * rows),
                     ("dq", torch.float32, 3 * rows), ("dF", torch.float32, nrows * F), ("dF2", torch.float32, nrows * F),
                     ("dP", torch.float32, H * (F + 5) + 1), ("dP2", torch.float32, H * (F + 5) + 1),
                     ("scratch", torch.uint8, int(L.pings_sdf_backward_scratch_bytes(rows, nnk, F, H, nrows)))]
        buf, O = _carve(dev, spec)
        if P:
            # the four dense Gaussian gradients lie back to back at the start of the allocation: one memset
            buf[:(O["d_alpha"].data_ptr() - buf.data_ptr()) + P * 4].zero_()
        a.g = g.data_ptr()
        for k in ("d_xyz", "d_rot", "d_scale", "d_alpha", "d_alpha_all") + (("ds", "v", "dn", "dq") if sdf_on else ()):
            setattr(a, k, O[k].data_ptr())
        stream = _lib.stream_ptr(dev)
        gF = gW1 = gb1 = gW2 = gb2 = None
        if sdf_on:
            _lib.check(L.pings_gauss_loss_backward_rows(C.byref(a), stream), "pings_gauss_loss_backward_rows")
            q, s = B["queries"].data_ptr(), O["scratch"].data_ptr()
            f, pts, quat, gpts = st["feats_c"], st["pts"], st["quat"], st["gpts"]
            ap = int(st["after_pgo"])
            if any(ctx.need[5:]):
                P1, P2 = O["dP"].data_ptr(), O["dP2"].data_ptr()
                off = lambda base, k: base + 4 * k
                _lib.check(L.pings_sdf_backward(
                    C.byref(dec), f.data_ptr(), f.shape[0], pts.data_ptr(), quat.data_ptr(), ap, q, rows, nnk,
                    B["nidx"].data_ptr(), B["w"].data_ptr(), O["ds"].data_ptr(), s, O["dF"].data_ptr(), P1,
                    off(P1, H * (F + 3)), off(P1, H * (F + 4)), off(P1, H * (F + 5)), stream), "pings_sdf_backward")
                _lib.check(L.pings_sdf_double_backward(
                    C.byref(dec), f.data_ptr(), f.shape[0], pts.data_ptr(), quat.data_ptr(), gpts.data_ptr(), ap, q,
                    rows, nnk, B["nidx"].data_ptr(), B["gidx"].data_ptr(), B["w"].data_ptr(), O["v"].data_ptr(), s,
                    O["dF2"].data_ptr(), P2, off(P2, H * (F + 3)), off(P2, H * (F + 4)), off(P2, H * (F + 5)), stream),
                    "pings_sdf_double_backward")
                O["dF"].add_(O["dF2"])
                O["dP"].add_(O["dP2"])
                gF = O["dF"].view(nrows, F)
                p = O["dP"]
                gW1, gb1 = p[:H * (F + 3)].view(H, F + 3), p[H * (F + 3):H * (F + 4)]
                gW2, gb2 = p[H * (F + 4):H * (F + 5)].view(1, H), p[H * (F + 5):]
            if ctx.need[0] or ctx.need[1]:
                h = _abi.SdfHvpArgs(dec.W1, dec.b1, dec.W2, dec.b2, H, F, dec.sdf_scale, ap, f.data_ptr(),
                                    pts.data_ptr(), quat.data_ptr(), gpts.data_ptr(), q, rows, nnk, B["nidx"].data_ptr(),
                                    B["gidx"].data_ptr(), O["v"].data_ptr(), O["ds"].data_ptr(), B["grad"].data_ptr(),
                                    O["dq"].data_ptr())
                _lib.check(L.pings_sdf_hvp_x(C.byref(h), stream), "pings_sdf_hvp_x")
            else:
                O["dq"].zero_()
        _lib.check(L.pings_gauss_loss_backward_scatter(C.byref(a), stream), "pings_gauss_loss_backward_scatter")
        s_xyz, s_rot, s_scale, s_alpha, s_all = ctx.shapes
        out = [O["d_xyz"].view(s_xyz), O["d_rot"].view(s_rot), O["d_scale"].view(s_scale), O["d_alpha"].view(s_alpha),
               O["d_alpha_all"].view(s_all), gF, gW1, gb1, gW2, gb2]
        return tuple(t if n else None for t, n in zip(out, ctx.need)) + (None,)


def gaussian_losses(self, render_pkg: dict, *, gs_type: str, opacity: bool = True, opacity_ent: bool = False,
                    isotropic: bool = False, area: bool = True, sdf_consistency: bool = True,
                    generator: Optional[torch.Generator] = None, _sample=None) -> GaussianLosses:
    """The Gaussian-space loss block of `Mapper.joint_gsdf_mapping` (utils/mapper.py:1331-1483).  `self` is the
    Mapper (its `config`, `neural_points` and `sdf_mlp` are read); `render_pkg` is `render(...)`'s dictionary.
    `sdf_consistency` covers the SDF, SDF-normal and invalid-opacity terms (the reference computes the three together
    when lambda_sdf_cons or lambda_sdf_normal_cons is positive).  A disabled term is 0.
    `_sample=(indices [S] int64, randn [R*S])` (tests only) replaces the draws: the sampled Gaussian indices (distinct)
    and the standard normal draws of the shifts in the reference's row order (shift block k, then sample)."""
    if gs_type not in GS_TYPES:
        raise ValueError(f"gaussian_losses: gs_type must be one of {sorted(GS_TYPES)}, got {gs_type!r}")
    cfg = self.config
    xyz, rot, scale, alpha = (render_pkg[k] for k in ("gaussian_xyz", "gaussian_rot", "gaussian_scale",
                                                        "gaussian_alpha"))
    alpha_all = render_pkg.get("alpha_all")
    P = xyz.shape[0]
    ncols, scols, vpow = GS_TYPES[gs_type]
    if scale.dim() != 2 or scale.shape[0] != P or scale.shape[1] != scols:
        raise ValueError(f"gaussian_losses: gaussian_scale must be [{P},{scols}] for {gs_type}, got {tuple(scale.shape)}")
    if rot.shape != (P, 4) or alpha.numel() != P:
        raise ValueError(f"gaussian_losses: gaussian_rot must be [{P},4] and gaussian_alpha [{P},1], got "
                         f"{tuple(rot.shape)} and {tuple(alpha.shape)}")
    if "local_view_gaussian_count" not in render_pkg:
        raise ValueError("gaussian_losses: render_pkg has no local_view_gaussian_count (the reference skips the frame)")
    vis = render_pkg["visibility_filter"][:render_pkg["local_view_gaussian_count"]]
    if vis.numel() != P:
        raise ValueError(f"gaussian_losses: {vis.numel()} local visibility flags for {P} Gaussians")
    contrib = render_pkg.get("contributions")
    contrib = None if contrib is None else _f32(contrib[:P])
    free = render_pkg.get("gaussian_free_mask")
    if free is not None and free.numel() != P:
        raise ValueError(f"gaussian_losses: gaussian_free_mask has {free.numel()} entries for {P} Gaussians")
    if not xyz.is_cuda:
        raise _lib.PingsHipError("gaussian_losses runs on the HIP device only (got a CPU tensor); there is no CPU "
                                 "fallback")
    opacity = bool(opacity and alpha_all is not None)
    opacity_ent = bool(opacity_ent and alpha_all is not None)
    if alpha_all is None:
        alpha_all = torch.zeros(0, dtype=torch.float32, device=xyz.device)
    cap = int(cfg.bs * cfg.gaussian_bs_ratio)
    if cap <= 0:
        raise ValueError(f"gaussian_losses: bs * gaussian_bs_ratio must be positive, got {cap}")
    R = int(cfg.gs_consist_shift_count) if sdf_consistency else 0
    dev = xyz.device
    flags = (F_OPACITY * opacity) | (F_ENT * opacity_ent) | (F_ISO * bool(isotropic)) | (F_AREA * bool(area)) | \
            (F_SDF * bool(sdf_consistency))
    a = _abi.GaussLossArgs(P, alpha_all.numel(), cap, R, ncols, scols, flags, float(cfg.min_alpha),
                           float(cfg.gs_contribution_threshold), float(cfg.gs_consist_shift_range_m),
                           float(cfg.valid_grad_min_thre), float(cfg.valid_grad_max_thre),
                           float(1.0 / cfg.voxel_size_m ** vpow), -1)
    keep = {"vis": vis.detach().to(torch.uint8).contiguous(), "contrib": contrib,
            "free": None if free is None else free.detach().to(torch.uint8).contiguous()}
    a.visible, a.contrib, a.free_mask = (_lib.ptr(keep[k]) for k in ("vis", "contrib", "free"))
    if _sample is not None:
        ids, z = _sample
        S = int(ids.numel())
        if S > cap or (R and z.numel() != R * S):
            raise ValueError(f"gaussian_losses: _sample needs at most {cap} indices and R * S = {R * S} draws")
        keep["inject"] = ids.detach().to(device=dev, dtype=torch.int64).contiguous()
        rz = torch.zeros(max(R, 1), cap, dtype=torch.float32, device=dev)
        if R:
            rz[:, :S] = z.detach().to(device=dev, dtype=torch.float32).view(R, S)
        keep["randn"] = rz
        a.n_inject, a.inject_idx = S, keep["inject"].data_ptr()
    else:
        keep["seed"] = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=dev, generator=generator)
        keep["randn"] = torch.randn(max(R, 1), cap, dtype=torch.float32, device=dev, generator=generator) if R else None
        a.seed = keep["seed"].data_ptr()
    a.randn = _lib.ptr(keep["randn"]) if keep["randn"] is not None else None

    st = {"args": a, "keep": keep, "nnk": 0, "dec": None, "feats": None}
    feats = W1 = b1 = W2 = b2 = None
    if sdf_consistency:
        npm, dec = self.neural_points, self.sdf_mlp
        wf = bool(getattr(getattr(npm, "config", None), "weighted_first", getattr(npm, "weighted_first", False)))
        if not _np.fused_supported(npm, dec) or wf:
            raise NotImplementedError("gaussian_losses: the fused block needs the per-neighbour decoder of the fused SDF "
                                      "kernels (one hidden ReLU level, weighted_first=False, every shipped config)")
        l0, lo = dec.layers[0], dec.lout
        feats, W1, b1, W2, b2 = npm.local_geo_features, l0.weight, l0.bias, lo.weight, lo.bias
        m = _np._map_args(npm, bool(npm.temporal_local_map_on), True, False, True)
        fc, W1c, b1c, W2c, b2c = (_f32(t) for t in (feats, W1, b1, W2, b2))
        st.update(map=m, nnk=int(m.nn_k), feats=feats, feats_c=fc, params=(W1c, b1c, W2c, b2c),
                  dec=_abi.SdfDecoder(W1c.data_ptr(), b1c.data_ptr(), W2c.data_ptr(), b2c.data_ptr(), int(W1c.shape[0]),
                                      int(fc.shape[1]), float(dec.sdf_scale), 0),
                  pts=_f32(npm.local_neural_points), quat=_f32(npm.local_point_orientations),
                  gpts=_f32(npm.neural_points), after_pgo=bool(npm.after_pgo))
        if W1c.shape[1] != fc.shape[1] + 3:
            raise ValueError(f"gaussian_losses: decoder input dim {W1c.shape[1]} != feature dim {fc.shape[1]} + 3")
    outs = _Block.apply(xyz, rot, scale, alpha, alpha_all, st.get("feats_c") if feats is None else feats,
                        W1, b1, W2, b2, st)
    return GaussianLosses(*outs)
