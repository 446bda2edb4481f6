"""fp64 restatement of the mapper's Gaussian-space loss block (utils/mapper.py:1331-1483) for the tests of
`pings_amd.gaussian_losses`.  The inline lines are transcribed term for term; the sample (indices and the standard
normal shift draws) is passed in, in place of `torch.randperm` / `torch.randn`.  `sdf(x)` returns (sdf, valid_nnk)
and must be twice differentiable in x (the oracle's `mapper_sdf` on a float64 map)."""
import torch


def quaternion2rotmat(q):                       # gaussian_splatting/utils/general_utils.py:205-213
    r, x, y, z = q.split(1, -1)
    R = torch.stack([
        1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)
    ], -1).reshape([len(q), 3, 3])
    return R


def rotation2normal(q):                         # general_utils.py:199-203
    n = quaternion2rotmat(q)[..., 2]
    return torch.nn.functional.normalize(n)


def opacity_entropy_loss(opacities):            # loss_utils.py:166-169
    opacities = torch.clamp(opacities, min=1e-6, max=1 - 1e-6)
    entropy = -opacities * torch.log(opacities) - (1 - opacities) * torch.log(1 - opacities)
    return entropy.mean()


def get_gradient(inputs, outputs):              # utils/tools.py:409-419
    return torch.autograd.grad(outputs, inputs, torch.ones_like(outputs), create_graph=True, retain_graph=True,
                               only_inputs=True)[0]


def block(cfg, gs_type, alpha_all, local_visible_mask, contributions, free_mask, gaussian_xyz, gaussian_rot,
          gaussian_scale, gaussian_alpha, sdf, sampled_indices, randn, opacity=True, opacity_ent=False,
          isotropic=False, area=True, sdf_consistency=True):
    """Returns the seven un-weighted terms as a list (0.0 for a disabled or gated term)."""
    z = 0.0
    opacity_loss = opacity_ent_loss = z
    m = cfg.min_alpha
    if opacity and alpha_all is not None:
        masked = alpha_all < m
        if torch.sum(masked) > 0:
            opacity_loss = 0.0 - alpha_all[masked].mean()
    if opacity_ent and alpha_all is not None:
        opacity_ent_loss = opacity_entropy_loss(torch.abs(alpha_all))
    mask = local_visible_mask & (gaussian_alpha > m).squeeze(-1)
    if contributions is not None:
        mask = mask & (contributions > cfg.gs_contribution_threshold)
    if free_mask is not None:
        mask = mask & (~free_mask)
    count = int(torch.sum(mask))
    iso = ar = sc = nc = inv = z
    if count > 10:
        scaling = gaussian_scale[sampled_indices]
        if isotropic:
            s = scaling[:, :3] if gs_type == "3d_gs" else scaling[:, :2]
            iso = torch.abs(s - s.mean(dim=1).view(-1, 1)).mean()
        if area:
            if gs_type == "3d_gs":
                ar = (scaling[:, 0] * scaling[:, 1] * scaling[:, 2]).mean() / cfg.voxel_size_m ** 3
            else:
                ar = (scaling[:, 0] * scaling[:, 1]).mean() / cfg.voxel_size_m ** 2
        alpha_s = gaussian_alpha[sampled_indices]
        if sdf_consistency:
            xyz = gaussian_xyz[sampled_indices]
            nrm = rotation2normal(gaussian_rot[sampled_indices])
            K = xyz.shape[0]
            R = cfg.gs_consist_shift_count
            shift = (randn - 0.5) * 2.0 * cfg.gs_consist_shift_range_m
            xs = xyz.repeat(R, 1) + nrm.repeat(R, 1) * shift[:, None]
            x_all = torch.cat((xyz, xs), 0)
            n_all = torch.cat((nrm, nrm.repeat(R, 1)), 0)
            label = torch.cat((torch.zeros(K, dtype=xyz.dtype), shift), 0)
            if not x_all.requires_grad:
                x_all.requires_grad_(True)                          # mapper.py:1444
            s_val, valid_nnk = sdf(x_all)
            g = get_gradient(x_all, s_val)
            gn = g.norm(dim=-1, keepdim=True).squeeze()
            valid = (gn < cfg.valid_grad_max_thre) & (gn > cfg.valid_grad_min_thre) & valid_nnk
            inv = alpha_s[~valid[:K]].mean()
            sc = torch.abs(s_val[valid] - label[valid]).mean()
            gh = g / (gn.unsqueeze(-1) + 1e-7)
            nc = (1.0 - (gh[valid] * n_all[valid]).sum(dim=1)).mean()
    return [opacity_loss, opacity_ent_loss, iso, ar, sc, nc, inv]
