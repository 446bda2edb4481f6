"""numpy fp64 restatement of the reference's camera pose arithmetic — TEST INFRASTRUCTURE ONLY.

`se3_exp` is utils/campose_utils.py:28-76 (both `angle < 1e-5` series branches), `update_pose` :79-98 with the
`CamImage.set_pose` it ends in (gaussian_splatting/utils/cameras.py:207-219), `set_pose` that method alone with a
general inverse.  Inputs are taken as they are (fp32 arrays are widened exactly), everything is computed in fp64 and
every output is rounded to fp32 once; `full_proj_transform` is built from the rounded `world_view_transform`, as the
reference builds it from its fp32 one.
"""
import numpy as np


def skew(x):
    return np.array([[0.0, -x[2], x[1]], [x[2], 0.0, -x[0]], [-x[1], x[0], 0.0]], dtype=np.float64)


def se3_exp(tau):
    tau = np.asarray(tau, dtype=np.float64)
    rho, theta = tau[:3], tau[3:]
    W = skew(theta)
    W2 = W @ W
    angle = np.sqrt(np.sum(theta * theta))
    I = np.eye(3)
    if angle < 1e-5:
        R = I + W + 0.5 * W2
        V = I + 0.5 * W + (1.0 / 6.0) * W2
    else:
        R = I + (np.sin(angle) / angle) * W + ((1.0 - np.cos(angle)) / angle ** 2) * W2
        V = I + W * ((1.0 - np.cos(angle)) / angle ** 2) + W2 * ((angle - np.sin(angle)) / angle ** 3)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = V @ rho
    return T


def _pack(T_cw, center, P):
    wvt = T_cw.T.astype(np.float32)
    fpt = (wvt.astype(np.float64) @ np.asarray(P, dtype=np.float64)).astype(np.float32)
    return dict(world_view_transform=wvt, full_proj_transform=fpt, camera_center=np.asarray(center).astype(np.float32),
                R=np.ascontiguousarray(wvt[:3, :3].T), T=wvt[3, :3].copy())


def set_pose(T_wc, P):
    """T_wc [4,4] camera -> world (any float dtype) -> the five tensors of `CamImage.set_pose`."""
    T_wc = np.asarray(T_wc, dtype=np.float64)
    return _pack(np.linalg.inv(T_wc), T_wc[:3, 3], P)


def update_pose(state, P, rho, theta, threshold=1e-4):
    """state: dict with the five tensors (fp32).  Returns (new state, converged).  |tau| == 0: the state itself, True."""
    tau = np.concatenate([np.asarray(rho, dtype=np.float64), np.asarray(theta, dtype=np.float64)])
    n = np.sqrt(np.sum(tau * tau))
    if n == 0:
        return state, True
    T_cw = np.eye(4)
    T_cw[:3, :3] = np.asarray(state["R"], dtype=np.float64)
    T_cw[:3, 3] = np.asarray(state["T"], dtype=np.float64)
    new = se3_exp(tau) @ T_cw
    center = -new[:3, :3].T @ new[:3, 3]
    return _pack(new, center, P), bool(n < threshold)
