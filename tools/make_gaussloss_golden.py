"""Golden vectors of the mapper's Gaussian-space loss block (utils/mapper.py:1331-1483) from the reference's own helpers.

`rotation2normal` and `quaternion2rotmat` (gaussian_splatting/utils/general_utils.py), `opacity_entropy_loss`
(gaussian_splatting/utils/loss_utils.py) and `get_gradient` (utils/tools.py) are imported from the reference tree;
`Mapper.sdf` is the oracle's restatement (`oracle/sdf_cpu.mapper_sdf`, itself pinned by the `sdf_*.npz` vectors) on the
`sdf_gs_f32` map in float64.  The inline lines of the block are transcribed below with the sample (indices and the
standard normal shift draws) fixed in place of `torch.randperm` / `torch.randn`.  Writes tests/golden/gaussloss_*.npz
with the inputs, the seven terms and the gradients of a weighted sum; tests/test_gauss_losses.py reads only the files.

    python tools/make_gaussloss_golden.py            (needs the reference tree; CPU only)
"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from oracle import ref_shim, sdf_cpu  # noqa: E402

WEIGHTS = [0.7, 1.3, 0.9, 1.1, 2.0, 1.7, 0.6]
CASES = {"surfel_r1": ("gaussian_surfel", 1, True, True, 0), "gs3d_r2": ("3d_gs", 2, False, True, 1),
         "gs2d_r0": ("2d_gs", 0, True, False, 2)}


def helpers():
    ref_shim.load()                      # stubs the reference's non-arithmetic imports, puts the tree on sys.path
    from gaussian_splatting.utils.general_utils import rotation2normal  # type: ignore
    from gaussian_splatting.utils.loss_utils import opacity_entropy_loss  # type: ignore
    from utils.tools import get_gradient  # type: ignore
    return rotation2normal, opacity_entropy_loss, get_gradient


def block(H, cfg, gs_type, alpha_all, local_visible_mask, gaussian_contributions, gaussian_free_mask, gaussian_xyz,
          gaussian_rot, gaussian_scale, gaussian_alpha, sdf, sampled_indices, randn):
    """utils/mapper.py:1331-1483 with every lambda positive, lambdas left out (un-weighted terms)."""
    rotation2normal, opacity_entropy_loss, get_gradient = H
    opacity_loss = 0.0
    constraint_min_alpha = cfg.min_alpha
    masked_alpha_mask = (alpha_all < constraint_min_alpha)
    if torch.sum(masked_alpha_mask) > 0:
        opacity_loss = 0.0 - (alpha_all[masked_alpha_mask]).mean()
    opacity_ent_loss = opacity_entropy_loss(torch.abs(alpha_all))
    constraint_mask = local_visible_mask
    large_alpha_mask = (gaussian_alpha > constraint_min_alpha).squeeze(-1)
    constraint_mask = constraint_mask & large_alpha_mask
    if gaussian_contributions is not None:
        constraint_mask = constraint_mask & (gaussian_contributions > cfg.gs_contribution_threshold)
    if gaussian_free_mask is not None:
        constraint_mask = constraint_mask & (~gaussian_free_mask)
    constraint_count = torch.sum(constraint_mask).item()
    isotropic_loss = area_loss = sdf_consistency_loss = sdf_normal_consistency_loss = 0.0
    invalid_opacity_loss = 0.0
    if constraint_count > 10:
        scaling = gaussian_scale[sampled_indices]
        if gs_type == "3d_gs":
            scaling = scaling[:, :3]
        else:
            scaling = scaling[:, :2]
        isotropic_loss = torch.abs(scaling - scaling.mean(dim=1).view(-1, 1)).mean()
        if gs_type == "3d_gs":
            area_loss = (scaling[:, 0] * scaling[:, 1] * scaling[:, 2]).mean()
            area_loss /= (cfg.voxel_size_m ** 3)
        else:
            area_loss = (scaling[:, 0] * scaling[:, 1]).mean()
            area_loss /= (cfg.voxel_size_m ** 2)
        sampled_guassians_alpha = gaussian_alpha[sampled_indices]
        sampled_guassians_xyz = gaussian_xyz[sampled_indices]
        sampled_guassians_normals = rotation2normal(gaussian_rot[sampled_indices])
        sampled_count = sampled_guassians_xyz.shape[0]
        shift_sample_count = cfg.gs_consist_shift_count
        shift_range = cfg.gs_consist_shift_range_m
        xyz_repeat = sampled_guassians_xyz.repeat(shift_sample_count, 1)
        normals_repeat = sampled_guassians_normals.repeat(shift_sample_count, 1)
        random_shift = (randn - 0.5) * 2.0 * shift_range
        shifted_xyz = xyz_repeat + normals_repeat * random_shift[:, None]
        xyz_all = torch.cat((sampled_guassians_xyz, shifted_xyz), 0)
        normals_all = torch.cat((sampled_guassians_normals, normals_repeat), 0)
        sdf_label_all = torch.cat((torch.zeros(sampled_count, dtype=xyz_all.dtype), random_shift), 0)
        xyz_all.requires_grad_(True)
        sampled_sdf, _, valid_nnk_mask = sdf(xyz_all, min_nn_count=3)
        sdf_grad = get_gradient(xyz_all, sampled_sdf)
        grad_norm = sdf_grad.norm(dim=-1, keepdim=True).squeeze()
        valid_grad_mask = (grad_norm < cfg.valid_grad_max_thre) & (grad_norm > cfg.valid_grad_min_thre) & (valid_nnk_mask)
        valid_grad_mask_no_shift = valid_grad_mask[:sampled_count]
        invalid_opacity_loss = (sampled_guassians_alpha[~valid_grad_mask_no_shift].mean())
        sdf_consistency_loss = torch.abs(sampled_sdf[valid_grad_mask] - sdf_label_all[valid_grad_mask]).mean()
        sdf_grad = sdf_grad / (grad_norm.unsqueeze(-1) + 1e-7)
        gaussian_normal_error = (1.0 - (sdf_grad[valid_grad_mask] * normals_all[valid_grad_mask]).sum(dim=1))
        sdf_normal_consistency_loss = gaussian_normal_error.mean()
    return [opacity_loss, opacity_ent_loss, isotropic_loss, area_loss, sdf_consistency_loss,
            sdf_normal_consistency_loss, invalid_opacity_loss]


def main():
    from test_gauss_losses import _cfg, _ref_mask, _scene, _state

    H = helpers()
    st = _state("gs_f32")
    out_dir = ROOT / "tests" / "golden"
    for name, (gs_type, R, contrib, free, seed) in CASES.items():
        cfg = _cfg(R=R, cap=512)
        pkg = _scene(st, P=600, gs_type=gs_type, seed=seed, contrib=contrib, free=free)
        mask = _ref_mask(pkg, cfg)
        true_idx = torch.where(mask)[0]
        g = torch.Generator().manual_seed(seed + 7)
        S = min(len(true_idx), cfg.bs)
        idx = true_idx[torch.randperm(len(true_idx), generator=g)[:S]]
        z = torch.randn(R * S, generator=g)
        cpu = sdf_cpu.NeuralPointMap(st)
        for k, v in list(vars(cpu).items()):
            if torch.is_tensor(v) and v.dtype == torch.float32:
                setattr(cpu, k, v.double())
        cpu.dtype = torch.float64
        leaves = {k: pkg[k].double().requires_grad_(True) for k in
                  ("gaussian_xyz", "gaussian_rot", "gaussian_scale", "gaussian_alpha", "alpha_all")}
        cpu.local_geo_features = cpu.local_geo_features.clone().requires_grad_(True)
        dec = sdf_cpu.MLP(*(torch.as_tensor(st["dec." + k]).double() for k in
                            ("layers.0.weight", "layers.0.bias", "lout.weight", "lout.bias")), float(st["sdf_scale"]))

        def mapper_sdf(x, min_nn_count=1):        # Mapper.sdf (mapper.py:2273-2289) on the oracle map
            s, cnt = sdf_cpu.mapper_sdf(cpu, dec, x)
            return s, None, cnt >= min_nn_count

        P = pkg["gaussian_xyz"].shape[0]
        vals = block(H, cfg, gs_type, leaves["alpha_all"], pkg["visibility_filter"][:P],
                     pkg["contributions"][:P].double() if contrib else None, pkg["gaussian_free_mask"],
                     leaves["gaussian_xyz"], leaves["gaussian_rot"], leaves["gaussian_scale"], leaves["gaussian_alpha"],
                     mapper_sdf, idx, z.double())
        vals = [torch.as_tensor(v, dtype=torch.float64) for v in vals]
        tot = sum(w * v for w, v in zip(WEIGHTS, vals) if bool(torch.isfinite(v)) and v.requires_grad)
        ins = list(leaves.values()) + [cpu.local_geo_features]
        grads = torch.autograd.grad(tot, ins, allow_unused=True)
        rec = {"gs_type": gs_type, "R": R, "seed": seed, "idx": idx.numpy(), "randn": z.numpy(),
               "values": np.array([float(v.detach()) for v in vals]), "weights": np.array(WEIGHTS),
               "visible": pkg["visibility_filter"][:P].numpy()}
        if contrib:
            rec["contributions"] = pkg["contributions"][:P].numpy()
        if free:
            rec["free_mask"] = pkg["gaussian_free_mask"].numpy()
        for k, t, gr in zip(list(leaves) + ["local_geo_features"], ins, grads):
            if k != "local_geo_features":
                rec[k] = pkg[k].numpy()
            rec["d_" + k] = (torch.zeros_like(t) if gr is None else gr).numpy()
        np.savez_compressed(out_dir / f"gaussloss_{name}.npz", **rec)
        print(name, [round(float(v), 6) for v in vals])


if __name__ == "__main__":
    main()
