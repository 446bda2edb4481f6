"""Every kernel class `mlp_plan` (csrc/mlp_common.hpp) can choose, against fp64 with per-element bounds, at the edges of
the plan and of the grids.

tests/test_mlp.py runs the shipped decoder shapes; this file runs, for each of the three families, both sides of every
threshold of the plan (forward KS, backward <NS, IB>, workgroup PF_X and <PF_X, PF_G>, the wave-128 <OH, VECX, VECG> and
its alignment fallbacks), row counts around one tile and one workgroup (1, 31, 32, 33, 127, 128, 129) and row counts
beyond the grid caps, where a workgroup or wave takes a second trip through its tile loop (17573 and 33061 rows for the
workgroup kernels' 512 workgroups, 65639 / 32805 for the wave kernels' 65536 / 32768 rows per trip).  Two CPU tests tie
the case lists to the plan: every class signature `mlp_ref.plan` can reach is run at its smallest and largest IN, and the
classes the kernel files instantiate are exactly the ones the plan can reach.

Each fp64 case asserts test_mlp.py's gates (`rel_err` <= 1e-5 on y, <= 1e-4 on gradients) AND |hip - ref| <= E per
element, E from tests/mlp_ref.py (no factor on top), and prints the worst err / E per quantity as a line `EDGE ...`.

Worst err / E per family and quantity on the MI355X: unmeasured.  The GPU cases of this file have not run on a device.
"""
import itertools
import types

import pytest
import torch

import mlp_ref
from conftest import rel_err

SMALL_N = (1, 31, 32, 33, 127, 128, 129)


def _cross(HID, INs, OUTs):
    return [(IN, HID, OUT) for IN, OUT in itertools.product(INs, OUTs)]


# (IN, HID, OUT), every one at every SMALL_N.  IN lists are the two sides of the plan's thresholds.
WG_SHAPES = (
    _cross(32, (1, 9, 10, 11, 20, 21, 36, 37, 63, 64), (1, 3, 32))
    + _cross(64, (1, 20, 21, 36, 37, 40, 41, 64), (2, 20, 31, 32))
    + _cross(64, (36, 37, 40, 41, 64), (1,))          # forward: workgroup kernel, backward: the SDF kernel
    + _cross(96, (1, 30, 31, 36, 37, 60, 61, 64), (1, 8, 32))
    + _cross(128, (33, 40, 41, 63, 64), (1, 24, 32)))
H64O1_SHAPES = _cross(64, (1, 2, 11, 12, 13, 19, 20, 32, 33, 34, 35, 63), (1,))   # 36, 37: in the list above
WAVE_SHAPES = [(IN, 128, OUT) for IN, OUT in (
    (32, 8), (19, 3), (32, 1), (1, 32), (31, 31), (4, 4), (29, 24), (32, 12), (16, 20), (32, 28), (32, 24),
    # the other end (smallest / largest IN) of each <vecw, vecx, OH, vecg> class
    (1, 24), (31, 24), (1, 8), (31, 8), (4, 8), (4, 24), (4, 3), (1, 5), (31, 16))]
SHAPES = WG_SHAPES + H64O1_SHAPES + WAVE_SHAPES

# (N, IN, HID, OUT): one shape per class signature at a row count beyond the grid cap of its kernels
LARGE = (
    [(17573, IN, 32, 3) for IN in (9, 11, 21, 63)]
    + [(17573, IN, 64, 31) for IN in (20, 21, 37, 41)]
    + [(17573, IN, 64, 1) for IN in (36, 37, 41)]
    + [(17573, IN, 96, 8) for IN in (30, 31, 37, 61)]
    + [(17573, IN, 128, 24) for IN in (33, 63)]
    + [(33061, 37, 32, 32), (33061, 21, 64, 2), (33061, 61, 96, 1), (33061, 41, 128, 1)]
    + [(65639, IN, 64, 1) for IN in (11, 12, 13, 32, 35, 64)]
    + [(65639, IN, 128, OUT) for IN, OUT in ((32, 24), (32, 8), (32, 28), (32, 1), (29, 24), (31, 8), (31, 16), (19, 3))])

# double backward (hidden 64, one output): both sides of the <NS, IB> thresholds around one workgroup, and beyond the
# 32768 rows of one trip
DOUBLE = [(N, IN) for IN in (12, 13, 32, 33, 36, 37, 63, 64) for N in (33, 129)] + [(32805, IN) for IN in (11, 35, 64)]

# wave-128 operands one float off a 16-byte boundary: one at a time, then all
MISALIGNED = [("x",), ("gy",), ("W1",), ("W2",), ("x", "gy", "W1", "W2")]
MISALIGNED_SHAPES = [(32, 128, 24), (32, 128, 8)]
MISALIGNED_N = (1, 33, 129)

DETERMINISM = [(17573, 37, 32, 3), (17573, 41, 64, 31), (17573, 61, 96, 8), (17573, 63, 128, 24)]


def _seed(N, IN, HID, OUT):
    return ((N * 67 + IN) * 131 + HID) * 37 + OUT


def _family(IN, HID, OUT):
    s = mlp_ref.plan(IN, HID, OUT)
    return s.fwd if s.fwd == s.bwd else f"{s.fwd}+{s.bwd}"


# ---------------------------------------------------------------- CPU: the case lists against the plan
def test_every_reachable_class_signature_is_run_at_its_smallest_and_largest_input_width():
    span = mlp_ref.reachable_signatures()
    assert len({s.fwd for s in span}) == 3
    have = {}
    for IN, HID, OUT in SHAPES:
        have.setdefault(mlp_ref.plan(IN, HID, OUT), set()).add(IN)
    for sig, (lo, hi) in span.items():
        assert {lo, hi} <= have.get(sig, set()), (sig, lo, hi)
    # beyond the grid caps: every signature once; the double backward on both of its two-block classes and a one-block one
    assert {mlp_ref.plan(IN, HID, OUT) for _, IN, HID, OUT in LARGE} == set(span)
    assert {mlp_ref.plan(IN, 64, 1).h64 for N, IN in DOUBLE if N > 32768} == {(6, 1), (18, 2), (32, 2)}
    assert {mlp_ref.plan(IN, 64, 1).h64 for N, IN in DOUBLE if N <= 129} == {(6, 1), (16, 1), (18, 2), (32, 2)}
    # every <OH, VECX, VECG> body of the wave-128 backward, the alignment fallbacks included
    ran = {mlp_ref.plan(IN, HID, OUT).wave for IN, HID, OUT in WAVE_SHAPES}
    ran |= {mlp_ref.plan(IN, HID, OUT, misaligned=mis).wave for IN, HID, OUT in MISALIGNED_SHAPES for mis in MISALIGNED}
    assert {(oh, vx, vg) for _, vx, oh, vg in ran} == mlp_ref.reachable_classes()["wave128_bwd"]
    assert {vw for vw, _, _, _ in ran} == {True, False}


def test_the_kernel_classes_built_are_the_classes_the_plan_can_reach():
    """`with_class<...>` lists of mlp_wg.hip / mlp_h64o1.hip and the PINGS_BWD_BODY lines of mlp_wave128.hip against the
    restated plan over all 64 x 4 x 32 admitted shapes: a class nobody can ask for is dead code, a class asked for and
    not built is a runtime error."""
    built, reach = mlp_ref.built_classes(), mlp_ref.reachable_classes()
    assert all(built.values())
    assert built == reach


def test_under_one_per_cent_of_the_rows_of_the_small_cases_are_moved_off_the_kink():
    """mlp_ref.make_inputs gates the rows moved per case from 300 rows on; below, one row is more than 1 %, so the
    fraction is taken here over all cases below 300 rows together, with the seeds the GPU tests use."""
    moved = rows = 0
    for IN, HID, OUT in SHAPES:
        for N in SMALL_N:
            moved, rows = moved + mlp_ref.draw_inputs(N, IN, HID, OUT, _seed(N, IN, HID, OUT))[1], rows + N
    for IN, HID, OUT in MISALIGNED_SHAPES:
        for N in MISALIGNED_N:
            moved, rows = moved + mlp_ref.draw_inputs(N, IN, HID, OUT, _seed(N, IN, HID, OUT) + 1)[1], rows + N
    for N, IN in DOUBLE:
        if N < 300:
            moved, rows = moved + mlp_ref.draw_inputs(N, IN, 64, 1, _seed(N, IN, 64, 1) + 2)[1], rows + N
    del TALLY[:]
    for J, N in GROUP_CASES:
        if N < 300:
            _group_inputs(N, GROUPS[J], _group_seed(J, N))
    moved, rows = moved + sum(k for k, _ in TALLY), rows + sum(n for _, n in TALLY)
    assert moved < 0.01 * rows, (moved, rows)


def test_the_restated_plan_at_the_thresholds_mlp_common_states():
    p = mlp_ref.plan
    assert [p(IN, 64, 1).fwd_ks for IN in (11, 12, 19, 20, 35)] == [6, 10, 10, 18, 18] and p(36, 64, 1).fwd == "wg"
    assert [p(IN, 64, 1).h64 for IN in (12, 13, 32, 33, 36, 37, 64)] == [(6, 1), (16, 1), (16, 1), (18, 2), (18, 2),
                                                                       (32, 2), (32, 2)]
    assert [p(IN, 32, 3).fwd_pfx for IN in (10, 11, 20, 21, 36, 37)] == [5, 10, 10, 18, 18, 32]
    assert [p(IN, 128, 8).bwd_pf for IN in (33, 40, 41, 64)] == [(5, 4), (5, 4), (9, 4), (9, 4)]
    assert p(32, 128, 8).wave == (True, True, 4, True) and p(32, 128, 8, misaligned=("gy",)).wave == (True, True, 16, False)
    assert p(32, 128, 24, misaligned=("W2",)).wave == (False, True, 12, True)


# ---------------------------------------------------------------- GPU: first order
def _run_hip(x, W1, b1, W2, b2, gy):
    from pings_amd.mlp import fused_mlp

    ins = [t.cuda().requires_grad_(True) for t in (x, W1, b1, W2, b2)]
    y = fused_mlp(*ins)
    g = torch.autograd.grad(y, ins, gy.cuda())
    return dict(y=y.detach(), gx=g[0], gW1=g[1], gb1=g[2], gW2=g[3], gb2=g[4])


def _check(tag, got, ref):
    """test_mlp.py's gates and the per-element bound for every quantity in `got`; prints the worst err / E of each."""
    worst = {k: mlp_ref.worst_ratio(v, *ref[k]) for k, v in got.items()}
    print("EDGE", tag, " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    for k, v in got.items():
        val, E = ref[k]
        assert tuple(v.shape) == tuple(val.shape), (tag, k)
        assert rel_err(v, val) <= (1e-5 if k == "y" else 1e-4), (tag, k, rel_err(v, val))
        if worst[k] > 1.0:
            at = int(((v.detach().double().cpu() - val).abs() / E).argmax())
            raise AssertionError(f"{tag}: {k} is {worst[k]:.3f} E at flat index {at} of shape {tuple(val.shape)}")


def _first_order_case(N, IN, HID, OUT):
    ins = mlp_ref.make_inputs(N, IN, HID, OUT, _seed(N, IN, HID, OUT))
    _check(f"{_family(IN, HID, OUT)} N={N} IN={IN} HID={HID} OUT={OUT}", _run_hip(*ins), mlp_ref.first_order(*ins))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "in%d-hid%d-out%d" % s)
def test_small_row_counts_match_fp64_within_the_fp32_bounds(shape):
    for N in SMALL_N:
        _first_order_case(N, *shape)


@pytest.mark.gpu
@pytest.mark.parametrize("case", LARGE, ids=lambda s: "n%d-in%d-hid%d-out%d" % s)
def test_second_trips_through_the_tile_loop_match_fp64_within_the_fp32_bounds(case):
    _first_order_case(*case)


def _off_by_one_float(t):
    """The same values as a contiguous view one float into a larger flat buffer: data_ptr() % 16 == 4."""
    flat = torch.empty(t.numel() + 8, dtype=torch.float32, device="cuda")
    v = flat[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("shape", MISALIGNED_SHAPES, ids=lambda s: "in%d-hid%d-out%d" % s)
@pytest.mark.parametrize("mis", MISALIGNED, ids="+".join)
def test_wave128_operands_off_the_16_byte_boundary(shape, mis):
    """A row slice as x, gy, W1 or W2: the kernels' `& 15` fallbacks to scalar loads (and OH = 16 for gy)."""
    from pings_amd import mlp as mlp_mod

    IN, HID, OUT = shape
    for N in MISALIGNED_N:
        ins = mlp_ref.make_inputs(N, IN, HID, OUT, _seed(N, IN, HID, OUT) + 1)
        dev = dict(zip(("x", "W1", "b1", "W2", "b2", "gy"), (t.cuda() for t in ins)))
        for k in mis:
            dev[k] = _off_by_one_float(dev[k])
        for k in ("x", "gy", "W1", "W2"):
            assert mlp_mod._f32c(dev[k]).data_ptr() % 16 == (4 if k in mis else 0), k
        y = mlp_mod.fused_mlp(dev["x"], dev["W1"], dev["b1"], dev["W2"], dev["b2"])
        gx, gW1, gb1, gW2, gb2 = mlp_mod._hip_backward(dev["x"], dev["W1"], dev["b1"], dev["W2"], dev["gy"], True)
        _check(f"wave128-off16({'+'.join(mis)}) N={N} IN={IN} HID={HID} OUT={OUT}",
               dict(y=y, gx=gx, gW1=gW1, gb1=gb1, gW2=gW2, gb2=gb2), mlp_ref.first_order(*ins))


@pytest.mark.gpu
@pytest.mark.parametrize("case", DETERMINISM, ids=lambda s: "n%d-in%d-hid%d-out%d" % s)
def test_workgroup_kernels_give_the_same_bits_twice(case):
    ins = mlp_ref.make_inputs(*case, _seed(*case))
    a, b = _run_hip(*ins), _run_hip(*ins)
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------- GPU: the double backward
@pytest.mark.gpu
@pytest.mark.parametrize("case", DOUBLE, ids=lambda s: "n%d-in%d" % s)
def test_double_backward_classes_match_fp64_within_the_fp32_bounds(case, monkeypatch):
    """The Eikonal composition of test_mlp.py's double-backward test.  The Eikonal term alone reaches W1, W2 and the
    per-row factor s only through `pings_mlp_double_backward` (d_W1, d_W2, d_dy), so those three gradients are the
    kernel's outputs and are held to mlp_ref.double_backward's bounds under the cotangent a = dL/dgx the device itself
    produced; the whole loss is then compared with fp64 autograd under test_mlp.py's gates."""
    from pings_amd import mlp as mlp_mod
    from pings_amd.mlp import fused_mlp

    def no_operator_composition(*_a, **_k):
        raise AssertionError("the recorded backward fell back to torch operators")

    monkeypatch.setattr(mlp_mod, "_torch_backward", no_operator_composition)
    N, IN = case
    x, W1, b1, W2, b2, _ = mlp_ref.make_inputs(N, IN, 64, 1, _seed(N, IN, 64, 1) + 2)
    scale = torch.rand(N, generator=torch.Generator().manual_seed(N + IN)) + 0.5

    def eikonal(xx, p, s, mlp):
        y = mlp(xx, *p).squeeze(1) * s
        gx, = torch.autograd.grad(y.sum(), xx, create_graph=True)
        return ((gx.norm(dim=1) - 1.0) ** 2).mean(), 0.1 * y.abs().mean(), gx

    hip_p = [t.cuda().requires_grad_(True) for t in (W1, b1, W2, b2)]
    xh, sh = x.cuda().requires_grad_(True), scale.cuda().requires_grad_(True)
    eik, rest, gxh = eikonal(xh, hip_p, sh, fused_mlp)
    a, = torch.autograd.grad(eik, gxh, retain_graph=True)
    dW1, dW2, ds = torch.autograd.grad(eik, [hip_p[0], hip_p[2], sh], retain_graph=True)
    tag = f"h64o1-dbl N={N} IN={IN} HID=64 OUT=1"
    first = mlp_ref.first_order(x, W1, b1, W2, b2, scale.reshape(N, 1))
    _check(tag + " (recorded backward)", dict(gx=gxh.detach()), first)
    _check(tag, dict(ggy=ds.reshape(N, 1), gW1=dW1, gW2=dW2), mlp_ref.double_backward(x, a, scale, W1, b1, W2))

    gh = torch.autograd.grad(eik + rest, hip_p + [xh], allow_unused=True)
    ref_p = [t.double().requires_grad_(True) for t in (W1, b1, W2, b2)]
    xr = x.double().requires_grad_(True)
    eik_r, rest_r, gxr = eikonal(xr, ref_p, scale.double(), lambda xx, a_, b_, c_, d_: torch.relu(xx @ a_.T + b_) @ c_.T + d_)
    gr = torch.autograd.grad(eik_r + rest_r, ref_p + [xr], allow_unused=True)
    assert rel_err(eik + rest, eik_r + rest_r) <= 1e-5 and rel_err(gxh, gxr) <= 1e-4
    for name, u, v in zip(["W1", "b1", "W2", "b2", "x"], gh, gr):
        assert rel_err(u, v) <= 1e-4, name


# ---------------------------------------------------------------- GPU: grouped launches
# (IN, OUT) per job, the input each job reads, inputs without a gradient, jobs whose output is left out of the loss
_FIVE = [(32, 24), (32, 32), (32, 24), (32, 8), (19, 24)]      # the shipped spawn decoders
GROUPS = {
    1: dict(shapes=_FIVE[:1], inputs=[0], nograd=set(), unused=set()),
    5: dict(shapes=_FIVE, inputs=[0, 0, 0, 1, 2], nograd={1}, unused={2}),
    8: dict(shapes=_FIVE + [(32, 3), (7, 5), (16, 12)], inputs=[0, 0, 0, 1, 2, 0, 3, 4], nograd={1}, unused={2}),
}


TALLY = []      # (rows moved off the kink, rows) of every group input drawn


def _group_inputs(N, cfg, seed):
    """Inputs, parameters and upstream gradients of a group (fp32, CPU); a shared input is moved off the kink of every
    decoder that reads it."""
    g = torch.Generator().manual_seed(seed)
    width = {}
    for (IN, _), i in zip(cfg["shapes"], cfg["inputs"]):
        assert width.setdefault(i, IN) == IN
    xs = [torch.randn(N, width[i], generator=g) for i in sorted(width)]
    params, ups = [], []
    for IN, OUT in cfg["shapes"]:
        params.append((torch.randn(128, IN, generator=g) / IN ** 0.5, 0.2 * torch.randn(128, generator=g),
                       torch.randn(OUT, 128, generator=g) / 128 ** 0.5, 0.2 * torch.randn(OUT, generator=g)))
        ups.append(torch.randn(N, OUT, generator=g))
    for i, x in enumerate(xs):
        readers = [p for p, j in zip(params, cfg["inputs"]) if j == i]
        moved = mlp_ref.nudge_off_kink(x, torch.cat([p[0] for p in readers]), torch.cat([p[1] for p in readers]))
        mlp_ref.check_moved(moved, N)
        TALLY.append((moved, N))
    return xs, params, ups


GROUP_CASES = [(J, N) for J in sorted(GROUPS) for N in (1, 33, 129, 5017)]


def _group_seed(J, N):
    return 1000 * J + N


def _check_group(tag, cfg, xs, params, ups, ys, gxs, gps, rows):
    """Outputs, input gradients (summed over the jobs that share an input: k - 1 more fp32 additions) and parameter
    gradients of a grouped launch against mlp_ref on the first `rows` rows."""
    refs = []
    for j, (p, i) in enumerate(zip(params, cfg["inputs"])):
        up = ups[j] if j not in cfg["unused"] else torch.zeros_like(ups[j])
        refs.append(mlp_ref.first_order(xs[i][:rows], *p, up[:rows]))
        got = dict(y=ys[j][:rows], gW1=gps[j][0], gb1=gps[j][1], gW2=gps[j][2], gb2=gps[j][3])
        _check(f"{tag} job={j} IN={p[0].shape[1]} OUT={p[2].shape[0]}", got, refs[j])
    for i, gx in gxs.items():
        share = [refs[j]["gx"] for j, k in enumerate(cfg["inputs"]) if k == i]
        val = sum(v for v, _ in share)
        E = sum(e for _, e in share) + mlp_ref.gamma(len(share) - 1) * sum(v.abs() for v, _ in share)
        _check(f"{tag} input={i} shared_by={len(share)}", dict(gx=gx[:rows]), dict(gx=(val, E)))


@pytest.mark.gpu
@pytest.mark.parametrize("J, N", GROUP_CASES)
def test_grouped_launches_match_fp64_within_the_fp32_bounds(J, N):
    """One, five and eight (MAX_JOBS) decoders in one launch each way, against the reference and not against single
    launches: few tiles (the share loop's early exit) and many, a job with OUT = 3, a job whose output the loss leaves
    out, an input that needs no gradient."""
    from pings_amd.mlp import fused_mlp_group, group_supported

    cfg = GROUPS[J]
    xs, params, ups = _group_inputs(N, cfg, _group_seed(J, N))
    dx = [x.cuda().requires_grad_(i not in cfg["nograd"]) for i, x in enumerate(xs)]
    dp = [tuple(t.cuda().requires_grad_(True) for t in p) for p in params]
    assert group_supported([dx[i] for i in cfg["inputs"]], dp)
    ys = fused_mlp_group([dx[i] for i in cfg["inputs"]], dp)
    used = [j for j in range(J) if j not in cfg["unused"]]
    leaves = [x for x in dx if x.requires_grad] + [t for p in dp for t in p]
    grads = torch.autograd.grad([ys[j] for j in used], leaves, [ups[j].cuda() for j in used])
    nx = sum(x.requires_grad for x in dx)
    gxs = dict(zip([i for i, x in enumerate(dx) if x.requires_grad], grads[:nx]))
    gps = [grads[nx + 4 * j:nx + 4 * j + 4] for j in range(J)]
    _check_group(f"wave128-grouped J={J} N={N}", cfg, xs, params, ups, [y.detach() for y in ys], gxs, gps, N)


@pytest.mark.gpu
@pytest.mark.parametrize("n", (77, 300))
def test_grouped_launches_with_rows_counted_on_the_device(n):
    """`fc.n_dev` rows of a capacity of N are decoded: outputs and input gradients of the first n rows and the weight
    gradients of n rows only match the reference of those rows; the forward writes no row from n on."""
    from pings_amd import _abi, _lib
    from pings_amd.mlp import fused_mlp_group

    N = 300
    cfg = dict(shapes=[(32, 24), (19, 3)], inputs=[0, 1], nograd=set(), unused=set())
    xs, params, ups = _group_inputs(N, cfg, 7 + n)
    dx = [x.cuda().requires_grad_(True) for x in xs]
    dp = [tuple(t.cuda().requires_grad_(True) for t in p) for p in params]
    fc = types.SimpleNamespace(n_dev=torch.tensor([n], dtype=torch.int32, device="cuda"), n_sel=n)
    ys = fused_mlp_group(dx, dp, fc)
    grads = torch.autograd.grad(ys, dx + [t for p in dp for t in p], [u.cuda() for u in ups])
    gps = [grads[2 + 4 * j:6 + 4 * j] for j in range(2)]
    _check_group(f"wave128-grouped-dyn n={n} N={N}", cfg, xs, params, ups, [y.detach() for y in ys],
                 {0: grads[0], 1: grads[1]}, gps, n)

    # the same forward on sentinel-filled outputs
    L = _lib.lib()
    sentinel = 12345.0
    outs = [torch.full((N, OUT), sentinel, dtype=torch.float32, device="cuda") for _, OUT in cfg["shapes"]]
    jobs = (_abi.MlpJob * 2)()
    keep = []
    for j, ((IN, OUT), p) in enumerate(zip(cfg["shapes"], dp)):
        x, (W1, b1, W2, b2) = dx[j].detach(), (t.detach() for t in p)
        keep += [x, W1, b1, W2, b2]
        jobs[j] = _abi.MlpJob(x.data_ptr(), IN, OUT, W1.data_ptr(), b1.data_ptr(), W2.data_ptr(), b2.data_ptr(),
                              outs[j].data_ptr(), None, None, None, None, None, None)
    _lib.check(L.pings_mlp_forward_grouped_dyn(jobs, 2, N, fc.n_dev.data_ptr(), _lib.stream_ptr(outs[0].device)),
               "pings_mlp_forward_grouped_dyn")
    for j, y in enumerate(outs):
        assert torch.equal(y[:n], ys[j].detach()[:n]), j
        assert bool((y[n:] == sentinel).all()), j
