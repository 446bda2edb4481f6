"""`pings_amd.camera_ops`: update_pose / set_pose on the device (csrc/camera.hip) against vectors produced by the
reference's own `CamImage.set_pose` and `update_pose` (tests/golden/campose_steps.npz, tools/make_campose_golden.py) and
against the fp64 restatement tests/campose_ref.py.

Gates: 1e-5 against the fixture (the gate of tests/test_camera.py for this quantity; the reference computes in fp32 and
stays within 3e-6 of the fp64 form on these cases), 1.2e-7 against the restatement fed the same fp32 inputs (one fp32
rounding is at most 2^-24 ~ 6e-8 of the tensor's maximum; the factor 2 covers full_proj_transform, which is built from
an already rounded operand)."""
import types

import numpy as np
import pytest
import torch

import campose_ref as CR
from conftest import rel_err

KEYS = ("world_view_transform", "full_proj_transform", "camera_center", "R", "T")
FIX_TOL = 1e-5
REF_TOL = 1.2e-7


@pytest.fixture(scope="module")
def fix(golden_dir):
    z = np.load(golden_dir / "campose_steps.npz")
    return {k: z[k] for k in z.files}


def _rel(a, b):
    return rel_err(torch.as_tensor(np.asarray(a)), torch.as_tensor(np.asarray(b)))


def _fix_state(fix, b, si=None, step=None):
    if si is None:
        return {k: fix["set_" + k][b] for k in KEYS}
    return {k: fix["step_" + k][b, si, step] for k in KEYS}


class _Cam:
    """The attributes of a `CamImage` that the pose functions touch.  strided=True lays the tensors out the way
    `CamImage.set_pose` leaves them: one T_cw, `world_view_transform` its transposed view, `R` / `T` slices of it,
    `camera_center` a row of another matrix, `projection_matrix` a transposed view."""

    def __init__(self, P, state=None, device="cuda", strided=True):
        self.device = device
        t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32).to(device)
        if strided:
            self.projection_matrix = t(np.ascontiguousarray(np.asarray(P).T)).T
        else:
            self.projection_matrix = t(P)
        self.R = torch.eye(3, device=device)
        self.T = torch.zeros(3, device=device)
        self.world_view_transform = self.full_proj_transform = self.camera_center = None
        self.cam_rot_delta = torch.nn.Parameter(torch.zeros(3, device=device))
        self.cam_trans_delta = torch.nn.Parameter(torch.zeros(3, device=device))
        if state is not None:
            if strided:
                T_cw = t(np.ascontiguousarray(state["world_view_transform"].T))
                self.world_view_transform = T_cw.T
                self.R, self.T = T_cw[:3, :3], T_cw[:3, 3]
                holder = torch.zeros(4, 4, device=device)
                holder[3, :3] = t(state["camera_center"])
                self.camera_center = holder[3, :3]
                self.full_proj_transform = t(np.ascontiguousarray(state["full_proj_transform"].T)).T
            else:
                self.world_view_transform = t(state["world_view_transform"])
                self.R, self.T = t(state["R"]), t(state["T"])
                self.camera_center = t(state["camera_center"])
                self.full_proj_transform = t(state["full_proj_transform"])

    def set_tau(self, tau):
        tau = torch.as_tensor(np.asarray(tau), dtype=torch.float32).to(self.device)
        self.cam_trans_delta.data.copy_(tau[:3])
        self.cam_rot_delta.data.copy_(tau[3:])

    def state(self):
        return {k: getattr(self, k).detach().cpu().numpy().copy() for k in KEYS}


# ------------------------------------------------------------------------------------------------ CPU
def test_restatement_matches_the_reference_fixture(fix):
    P = fix["projection_matrix"]
    worst = 0.0
    for b in range(fix["pose"].shape[0]):
        s = CR.set_pose(fix["pose"][b], P)
        for k in KEYS:
            worst = max(worst, _rel(s[k], fix["set_" + k][b]))
            assert _rel(s[k], fix["set_" + k][b]) <= FIX_TOL, ("set_pose", b, k)
        for si, scale in enumerate(fix["scales"]):
            st = _fix_state(fix, b)
            for i in range(fix["tau"].shape[2]):
                tau = fix["tau"][b, si, i]
                st, flag = CR.update_pose(st, P, tau[:3], tau[3:], float(fix["threshold"]))
                assert flag == bool(fix["flag"][b, si, i]), (b, scale, i)
                for k in KEYS:
                    e = _rel(st[k], fix["step_" + k][b, si, i])
                    worst = max(worst, e)
                    assert e <= FIX_TOL, (b, str(scale), i, k, e)
    print(f"restatement vs fixture: worst rel_err {worst:.3e}")


def test_fixture_covers_both_sides_of_both_thresholds(fix):
    tau = fix["tau"].astype(np.float64)
    n, a = np.linalg.norm(tau, axis=-1), np.linalg.norm(tau[..., 3:], axis=-1)
    assert (n == 0).any() and ((n > 0) & (n < 1e-4)).any() and (n > 1e-4).any()
    assert ((a > 0) & (a < 1e-5)).any() and (a > 1e-5).any() and (a > 2.9).any()
    assert (np.abs(n[n > 0] / 1e-4 - 1) > 0.01).all() and (np.abs(a[a > 0] / 1e-5 - 1) > 0.01).all()
    assert fix["flag"].any() and not fix["flag"].all()


def test_no_cpu_fallback(fix):
    from pings_amd import camera_ops
    from pings_amd._lib import PingsHipError

    cam = _Cam(fix["projection_matrix"], _fix_state(fix, 0), device="cpu")
    cam.set_tau(fix["tau"][0, 5, 0])
    with pytest.raises(PingsHipError):
        camera_ops.update_pose(cam)
    with pytest.raises(PingsHipError):
        camera_ops.set_pose(cam, torch.eye(4, dtype=torch.float64))
    camera_ops.set_pose(cam, None)                       # None is a no-op, as in the reference
    assert cam.cam_trans_delta.abs().max() > 0           # nothing was touched


def test_install_rebinds_both_names_once():
    from pings_amd import camera_ops

    ref_update = lambda camera, converged_threshold=1e-4: True

    class CamCls:
        def set_pose(self, cam_pose):
            return "reference"

    ref_set = CamCls.__dict__["set_pose"]
    mods = [types.ModuleType(n) for n in ("campose_utils", "mapper", "inspect_pings")]
    for m in mods:
        m.update_pose = ref_update
    for _ in range(2):                                   # installing twice changes nothing
        camera_ops.install(*mods, cam_cls=CamCls)
        for m in mods:
            assert m.update_pose is camera_ops.update_pose
            assert m._pings_update_pose_original is ref_update
        assert CamCls.__dict__["set_pose"] is camera_ops.set_pose
        assert CamCls._pings_set_pose_original is ref_set
    camera_ops.uninstall(*mods, cam_cls=CamCls)
    assert all(m.update_pose is ref_update for m in mods) and CamCls.__dict__["set_pose"] is ref_set


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("b", [0, 1, 2])
def test_update_pose_chain_matches_the_reference_fixture(fix, b):
    from pings_amd import camera_ops

    P = fix["projection_matrix"]
    worst = 0.0
    for si, scale in enumerate(fix["scales"]):
        cam = _Cam(P, _fix_state(fix, b))
        for i in range(fix["tau"].shape[2]):
            tau = fix["tau"][b, si, i]
            cam.set_tau(tau)
            before = cam.state()
            flag = camera_ops.update_pose(cam, float(fix["threshold"]))
            assert flag.dtype is torch.bool and flag.dim() == 0 and flag.is_cuda
            assert bool(flag) == bool(fix["flag"][b, si, i]), (str(scale), i)
            after = cam.state()
            for k in KEYS:
                e = _rel(after[k], fix["step_" + k][b, si, i])
                worst = max(worst, e)
                assert e <= FIX_TOL, (str(scale), i, k, e)
            assert not getattr(cam.world_view_transform, "requires_grad") and cam.R.grad_fn is None
            if np.all(tau == 0):                         # pose optimisation off: carried over bit for bit
                for k in KEYS:
                    assert np.array_equal(after[k], before[k]), (str(scale), i, k)
            assert cam.cam_rot_delta.abs().max() == 0 and cam.cam_trans_delta.abs().max() == 0
            # R and T are views of the world_view_transform slice of one block
            assert cam.R.data_ptr() == cam.world_view_transform.data_ptr()
            assert torch.equal(cam.R, cam.world_view_transform[:3, :3].T)
            assert torch.equal(cam.T, cam.world_view_transform[3, :3])
    print(f"kernel vs fixture, base {b}: worst rel_err {worst:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("b", [0, 1, 2])
def test_update_pose_matches_the_restatement_strided_and_contiguous(fix, b):
    """Every fixture step on its own: kernel and restatement start from the fixture's fp32 state before the step."""
    from pings_amd import camera_ops

    P = fix["projection_matrix"]
    worst = 0.0
    for si, scale in enumerate(fix["scales"]):
        for i in range(fix["tau"].shape[2]):
            st = _fix_state(fix, b) if i == 0 else _fix_state(fix, b, si, i - 1)
            tau = fix["tau"][b, si, i]
            want, want_flag = CR.update_pose(st, P, tau[:3], tau[3:], float(fix["threshold"]))
            got = []
            for strided in (True, False):
                cam = _Cam(P, st, strided=strided)
                cam.set_tau(tau)
                flag = camera_ops.update_pose(cam, float(fix["threshold"]))
                assert bool(flag) == want_flag, (str(scale), i)
                got.append(cam.state())
            for k in KEYS:
                e = _rel(got[0][k], want[k])
                worst = max(worst, e)
                assert e <= REF_TOL, (str(scale), i, k, e)
                assert np.array_equal(got[0][k], got[1][k]), (str(scale), i, k)
    print(f"kernel vs restatement, base {b}: worst rel_err {worst:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_set_pose_matches_fixture_and_restatement(fix, dtype):
    from pings_amd import camera_ops

    P = fix["projection_matrix"]
    worst_fix = worst_ref = 0.0
    for b in range(fix["pose"].shape[0]):
        pose = torch.as_tensor(fix["pose"][b]).to(dtype)
        want = CR.set_pose(pose.numpy(), P)
        got = []
        for where, layout in (("cuda", "plain"), ("cpu", "plain"), ("cuda", "transposed")):
            cam = _Cam(P, strided=layout == "transposed")
            inp = pose.to(where)
            if layout == "transposed":
                inp = inp.T.contiguous().T               # the same matrix, read through swapped strides
            camera_ops.set_pose(cam, inp)
            got.append(cam.state())
            assert cam.R.data_ptr() == cam.world_view_transform.data_ptr()
        for k in KEYS:
            ef, er = _rel(got[0][k], fix["set_" + k][b]), _rel(got[0][k], want[k])
            worst_fix, worst_ref = max(worst_fix, ef), max(worst_ref, er)
            # an fp32 pose is already rounded: the fixture saw the fp64 one, so only the fp64 input meets the 1e-5 gate
            # by derivation; the fp32 input is held to it as well (rounding the pose moves the result by ~6e-8)
            assert ef <= FIX_TOL, (b, k, ef)
            assert er <= REF_TOL, (b, k, er)
            assert np.array_equal(got[0][k], got[1][k]) and np.array_equal(got[0][k], got[2][k]), (b, k)
    print(f"set_pose {dtype}: worst rel_err vs fixture {worst_fix:.3e}, vs restatement {worst_ref:.3e}")


@pytest.mark.gpu
def test_set_pose_non_rigid_input_is_the_general_inverse(fix):
    from pings_amd import camera_ops

    P = fix["projection_matrix"]
    pose = fix["pose"][0].copy()
    pose[:3, :3] *= 1.5                                  # uniform scale: invertible, not rigid
    want = CR.set_pose(pose, P)
    cam = _Cam(P)
    camera_ops.set_pose(cam, torch.as_tensor(pose).cuda())
    got = cam.state()
    for k in KEYS:
        assert _rel(got[k], want[k]) <= REF_TOL, k
    # a rigid shortcut (R^T, -R^T t) would be off by the scale squared
    rigid = pose[:3, :3].T
    assert np.abs(got["R"] - rigid).max() > 0.1


@pytest.mark.gpu
def test_set_pose_singular_input_gives_non_finite_outputs(fix):
    from pings_amd import camera_ops

    cam = _Cam(fix["projection_matrix"])
    camera_ops.set_pose(cam, torch.zeros(4, 4, dtype=torch.float64, device="cuda"))
    assert not torch.isfinite(cam.world_view_transform).all()


@pytest.mark.gpu
def test_update_and_set_pose_do_not_wait_for_the_device(fix):
    from pings_amd import _lib, camera_ops

    P = fix["projection_matrix"]
    cam = _Cam(P, _fix_state(fix, 1))
    pose = torch.as_tensor(fix["pose"][1]).cuda()
    tau = torch.as_tensor(fix["tau"][1, 5, 0]).cuda()
    cam.set_tau(fix["tau"][1, 5, 0])
    camera_ops.update_pose(cam)                          # warm-up: loads the library
    torch.cuda.synchronize()
    _lib.sync_counts(reset=True)
    probe = torch.ones(1, device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                # positive control: the mode catches a device-to-host read
            probe.sum().item()
        camera_ops.set_pose(cam, pose)
        cam.cam_trans_delta.data.copy_(tau[:3])
        cam.cam_rot_delta.data.copy_(tau[3:])
        flag = camera_ops.update_pose(cam)
        with pytest.raises(RuntimeError):                # reading the flag is the one wait
            bool(flag)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert _lib.sync_counts() == {}
    assert bool(flag) is False
    want, _ = CR.update_pose(CR.set_pose(fix["pose"][1], P), P, fix["tau"][1, 5, 0][:3], fix["tau"][1, 5, 0][3:])
    assert _rel(cam.state()["world_view_transform"], want["world_view_transform"]) <= REF_TOL


def test_null_pointers_are_a_status_code(fix):
    from pings_amd import _abi, _lib

    L = _lib.lib()
    assert L.pings_camera_update_pose(None, None) == 1 and b"null" in L.pings_last_error()
    assert L.pings_camera_update_pose(_abi.CameraPoseArgs(), None) == 1 and b"null" in L.pings_last_error()
    assert L.pings_camera_set_pose(None, 1, 4, 1, None, 4, 1, None, None) == 1 and b"null" in L.pings_last_error()


@pytest.mark.gpu
def test_render_accepts_a_camera_posed_through_camera_ops():
    """A `Camera` posed by `camera_ops.set_pose` + `update_pose` renders the image of a `Camera` given the same pose
    through its own torch `set_pose`."""
    from pings_amd import camera_ops
    from pings_amd.camera import Camera, se3_exp
    from pings_amd.renderer import render
    from test_render import _scene

    dev = "cuda"
    data, decs, cam, _, _ = _scene(dev)
    pose = torch.linalg.inv(se3_exp(torch.tensor([0.05, -0.03, 0.04, 0.02, -0.015, 0.01], dtype=torch.float64)))
    camera_ops.set_pose(cam, pose)
    with torch.no_grad():
        cam.cam_trans_delta.copy_(torch.tensor([0.02, 0.01, -0.015], device=dev))
        cam.cam_rot_delta.copy_(torch.tensor([-0.01, 0.02, 0.005], device=dev))
    assert not bool(camera_ops.update_pose(cam))
    T_cw = cam.world_view_transform.T.double().cpu()
    other = Camera(160, 96, 140.0, 150.0, 78.3, 49.1, 0.05, 60.0, torch.linalg.inv(T_cw), device=dev)
    assert rel_err(other.world_view_transform, cam.world_view_transform) <= 1e-6
    bg = torch.tensor([0.2, 0.4, 0.6], device=dev)
    kw = dict(view_concat_on=True, learn_color_residual=True)
    with torch.no_grad():
        a = render(cam, None, data, decs, None, bg, **kw)
        b = render(other, None, data, decs, None, bg, **kw)
    assert a is not None and b is not None
    for k in ("render", "surf_depth", "rend_alpha"):
        assert rel_err(a[k], b[k]) <= 1e-5, k
