"""_RasterizeGaussians.backward as autograd drives it (SurfelGaussianRasterizer, 64x48): unused outputs reach it as None,
not as zero tensors autograd fills, and the pose gradients are returned as views of the six floats of d_tau.

A loss on the image alone gives the gradient bits of the same loss with explicit zero upstream gradients for normal,
depth and alpha; theta.grad / rho.grad have shape (3,) and are the halves of the d_tau the C ABI writes for the same
inputs; a second backward accumulates; zeroing theta.grad in place leaves rho.grad alone."""
import pytest
import torch

from scenes import hip_settings
from test_gaussian_passes import FRONT_ONLY, _bits, _run, _scene

NAMES = ("means", "col", "op", "scales", "rot")


def _leaves(sc):
    d = lambda t: t.to(torch.float32).cuda().contiguous().requires_grad_(True)
    leaves = {k: d(sc[k]) for k in NAMES}
    leaves["theta"] = torch.zeros(3, device="cuda", requires_grad=True)
    leaves["rho"] = torch.zeros(3, device="cuda", requires_grad=True)
    return leaves


def _render(sc, leaves):
    from pings_amd import rasterizer as hr

    rast = hr.SurfelGaussianRasterizer(hip_settings(sc, "surfel", FRONT_ONLY))
    m2d = torch.zeros_like(leaves["means"], requires_grad=True)
    return rast(means3D=leaves["means"], means2D=m2d, colors_precomp=leaves["col"], opacities=leaves["op"],
                scales=leaves["scales"], rotations=leaves["rot"], theta=leaves["theta"], rho=leaves["rho"])


@pytest.fixture(scope="module")
def case():
    sc = _scene("small", 257, "s", "surfel")
    g = torch.Generator().manual_seed(21)
    gc = torch.randn(3, sc["H"], sc["W"], generator=g, dtype=torch.float64)
    return sc, gc


@pytest.mark.gpu
def test_unused_outputs_equal_zero_upstream(case):
    sc, gc = case
    a, b = _leaves(sc), _leaves(sc)
    img = _render(sc, a)[0]
    (img * gc.float().cuda()).sum().backward()
    img, nrm, dep, alp, _, _ = _render(sc, b)
    torch.autograd.backward([(img * gc.float().cuda()).sum(), nrm, dep, alp],
                            [None, torch.zeros_like(nrm), torch.zeros_like(dep), torch.zeros_like(alp)])
    for k in a:
        assert a[k].grad is not None and float(a[k].grad.abs().max()) > 0, k
        assert torch.equal(_bits(a[k].grad), _bits(b[k].grad)), k


@pytest.mark.gpu
def test_pose_gradients_are_the_halves_of_d_tau(case):
    sc, gc = case
    leaves = _leaves(sc)
    (_render(sc, leaves)[0] * gc.float().cuda()).sum().backward()
    zeros = lambda c: torch.zeros(c, sc["H"], sc["W"], dtype=torch.float64)
    out, _ = _run(sc, "surfel", (gc, zeros(3), zeros(1), zeros(1)))
    theta, rho = leaves["theta"].grad, leaves["rho"].grad
    assert theta.shape == (3,) and rho.shape == (3,)
    assert torch.equal(_bits(theta), _bits(out["d_tau"][3:])) and torch.equal(_bits(rho), _bits(out["d_tau"][:3]))
    assert torch.equal(_bits(leaves["means"].grad), _bits(out["d_means3D"]))
    # the two are views of one six-float tensor: an in-place edit of one must not reach the other
    rho_before = rho.clone()
    theta.zero_()
    assert int(_bits(leaves["theta"].grad).abs().max()) == 0
    assert torch.equal(_bits(leaves["rho"].grad), _bits(rho_before))


@pytest.mark.gpu
def test_second_backward_accumulates(case):
    sc, gc = case
    leaves = _leaves(sc)
    (_render(sc, leaves)[0] * gc.float().cuda()).sum().backward()
    first = {k: t.grad.clone() for k, t in leaves.items()}
    (_render(sc, leaves)[0] * gc.float().cuda()).sum().backward()
    for k, t in leaves.items():
        assert t.grad.shape == first[k].shape
        assert torch.equal(_bits(t.grad), _bits(first[k] + first[k])), k   # the kernels are bitwise reproducible
