"""FusedAdamW on the device against torch.optim.AdamW(foreach=False) on the CPU in fp64, fed the same gradients.

The gate, per tensor and the same for the parameter, exp_avg and exp_avg_sq:

    max|hip - fp64| <= max(4 E, steps * 2^-24 * max|fp64|)

E is the error of stock CPU fp32 AdamW against the same fp64 run, computed here.  The factor 4 allows for the device's
division and square root rounding differently from the host's; the second term is half an ulp per step, for tensors
whose E is small by luck (a 1-element tensor).  A wrong bias correction, beta or decay shows at 1e-4 and above.
"""
import ctypes

import pytest
import torch

from pings_amd import _abi, _lib
from pings_amd.dist import GradBucket
from pings_amd.optim import CHUNK, MAX_JOBS, FusedAdamW

pytestmark = pytest.mark.gpu

STEPS = 12
DEFAULTS = dict(betas=(0.9, 0.99), eps=1e-15)                       # utils/tools.py:361
GROUPS = [dict(lr=0.01, weight_decay=0.0),                          # decoders and feature tables
          dict(lr=0.003),                                           # the camera groups: torch's weight_decay 0.01
          dict(lr=1e-3, weight_decay=0.1, eps=1e-8, betas=(0.8, 0.95))]
KEYS = ("exp_avg", "exp_avg_sq")


class Case:
    """Initial values, group of every tensor and the gradients of every step (fp32, CPU; None: no gradient), with the
    fp64 oracle's final state and the error E of stock CPU fp32 against it."""

    def __init__(self, shapes, steps=STEPS, seed=0, every_third=(), never=(), zero_rows=(), only=None):
        gen = torch.Generator().manual_seed(seed)
        self.steps = steps
        self.init = [0.1 * torch.randn(s, generator=gen) for s in shapes]
        self.group = [i % len(GROUPS) for i in range(len(shapes))]
        self.grads = []
        for s in range(steps):
            row = []
            for i, x in enumerate(self.init):
                if i in never or (i in every_third and s % 3 != 2) or (only and i in only and s not in only[i]):
                    row.append(None)
                    continue
                mag = 10.0 ** (-12.0 * torch.rand(x.shape, generator=gen))          # 1e-12 .. 1
                g = mag * (torch.randint(0, 2, x.shape, generator=gen) * 2 - 1)
                if i in zero_rows:
                    g[torch.rand(x.shape[0], generator=gen) < 0.7] = 0.0
                row.append(g.float())
            self.grads.append(row)
        self.ref = self._final(torch.float64)
        got = self._final(torch.float32)
        self.E = [None if r is None else {k: (got[i][k].double() - r[k]).abs().max().item() if r[k].numel() else 0.0
                                          for k in r if k != "step"} for i, r in enumerate(self.ref)]

    def groups(self, params):
        return [dict(GROUPS[j], params=[p for p, gi in zip(params, self.group) if gi == j], name=f"group_{j}")
                for j in range(len(GROUPS))]

    def _final(self, dtype):
        ps = [torch.nn.Parameter(x.to(dtype, copy=True)) for x in self.init]
        opt = torch.optim.AdamW(self.groups(ps), foreach=False, **DEFAULTS)
        for row in self.grads:
            for p, g in zip(ps, row):
                p.grad = None if g is None else g.to(dtype)
            opt.step()
        self.n_state = len(opt.state)
        return [None if p not in opt.state else
                dict(p=p.detach(), step=opt.state[p]["step"].item(), **{k: opt.state[p][k] for k in KEYS}) for p in ps]

    def gate(self, params, opt):
        assert len(opt.state) == self.n_state
        for i, (p, r) in enumerate(zip(params, self.ref)):
            if r is None:
                assert p not in opt.state and torch.equal(p.detach().cpu(), self.init[i]), i
                continue
            st = opt.state[p]
            assert st["step"].item() == r["step"] and st["step"].device.type == "cpu", i
            for k, got in (("p", p.detach()), ("exp_avg", st["exp_avg"]), ("exp_avg_sq", st["exp_avg_sq"])):
                assert got.shape == r[k].shape
                if not got.numel():
                    continue
                err = (got.double().cpu() - r[k]).abs().max().item()
                bound = max(4 * self.E[i][k], self.steps * 2.0 ** -24 * r[k].abs().max().item())
                print(f"tensor {i} {tuple(got.shape)} {k}: err {err:.3e} E {self.E[i][k]:.3e} bound {bound:.3e}")
                assert err <= bound, (i, tuple(got.shape), k, err, self.E[i][k], bound)


SIZES = [(0,), (1,), (3,), (9,), (63,), (64,), (65,), (255,), (257,), (CHUNK - 1,), (CHUNK,), (CHUNK + 1,),
         (2 * CHUNK + 5,), (4097, 32), (130,), (77,)]


@pytest.fixture(scope="module")
def case():
    # the table (index 13) has 70 % zero rows; tensor 14 has a gradient every third step, tensor 15 never
    return Case(SIZES, every_third=(14,), never=(15,), zero_rows=(13,))


def _device_params(c):
    return [torch.nn.Parameter(x.cuda()) for x in c.init]


def _run(c, params, opt_of, first=0, last=None, set_grad=None):
    """Steps [first, last) with the optimiser `opt_of(step)`."""
    for s in range(first, c.steps if last is None else last):
        opt = opt_of(s)
        for p, g in zip(params, c.grads[s]):
            if set_grad is not None:
                set_grad(p, g)
            else:
                p.grad = None if g is None else g.cuda()
        opt.step()
    return opt


def test_parity_over_12_steps(case):
    ps = _device_params(case)
    opt = FusedAdamW(case.groups(ps), **DEFAULTS)
    _run(case, ps, lambda s: opt)
    assert opt.last_launches == 1
    case.gate(ps, opt)
    assert [g["name"] for g in opt.param_groups] == ["group_0", "group_1", "group_2"]


@pytest.mark.parametrize("off", [1, 2, 3])
def test_misaligned_views(off):
    """Parameters, gradients and both moments at float offset `off` of flat buffers: the scalar path."""
    c = Case([(5,), (257,), (CHUNK + 1,), (2 * CHUNK + 5,), (33, 32)], seed=off, zero_rows=(4,))

    def view(x):
        flat = torch.zeros(x.numel() + 4, device="cuda")
        v = flat[off:off + x.numel()].view(x.shape)
        v.copy_(x)
        assert v.data_ptr() % 16 == 4 * off
        return v

    ps = [torch.nn.Parameter(view(x)) for x in c.init]
    gviews = [view(torch.zeros_like(x)) for x in c.init]
    opt = FusedAdamW(c.groups(ps), **DEFAULTS)
    for p in ps:
        opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": view(torch.zeros_like(p)),
                        "exp_avg_sq": view(torch.zeros_like(p))}
    for p, gv in zip(ps, gviews):
        assert p.data_ptr() % 16 == 4 * off
        p.grad = gv
    _run(c, ps, lambda s: opt, set_grad=lambda p, g: p.grad.copy_(g))
    assert opt.last_launches == 1
    assert all(opt.state[p]["exp_avg"].data_ptr() % 16 == 4 * off for p in ps)
    c.gate(ps, opt)


def test_grad_bucket_views():
    """`GradBucket` hands out gradient views at arbitrary 4-byte offsets of one flat buffer (world size 1)."""
    c = Case([(3,), (64,), (1,), (CHUNK + 1,), (130, 32), (7,)], seed=7)
    ps = _device_params(c)
    bucket = GradBucket(ps)
    assert any(p.grad.data_ptr() % 16 for p in ps)
    opt = FusedAdamW(c.groups(ps), **DEFAULTS)
    for s in range(c.steps):
        bucket.zero()
        if s == 5:
            opt.zero_grad(set_to_none=True)     # the bucket re-attaches its views
            bucket.zero()
        for p, g in zip(ps, c.grads[s]):
            p.grad.copy_(g)
        bucket.finish()
        opt.step()
    bucket.close()
    c.gate(ps, opt)


@pytest.mark.parametrize("n, launches", [(MAX_JOBS + 1, 2), (MAX_JOBS, 1)])
def test_job_table_capacity(n, launches):
    c = Case([(3,)] * n, steps=2, seed=n)
    ps = _device_params(c)
    opt = FusedAdamW(c.groups(ps), **DEFAULTS)
    _run(c, ps, lambda s: opt)
    assert opt.last_launches == launches
    # What can go wrong here is a job that is skipped or that runs with another job's pointers or scalars (the three
    # groups differ in every hyper-parameter), which shows at 1e-4 of the tensor's magnitude and above; two steps of
    # fp32 rounding stay below 1e-6.  So every tensor is held to 1e-5 of its fp64 magnitude, and must have moved.
    assert len(opt.state) == n
    for i, (p, r) in enumerate(zip(ps, c.ref)):
        st = opt.state[p]
        assert st["step"].item() == 2
        for k, got in (("p", p.detach()), ("exp_avg", st["exp_avg"]), ("exp_avg_sq", st["exp_avg_sq"])):
            err = (got.double().cpu() - r[k]).abs().max().item()
            print(f"tensor {i} {k}: err {err:.3e} of {r[k].abs().max().item():.3e}")
            assert err <= 1e-5 * r[k].abs().max().item(), (i, k, err)
        assert not torch.equal(p.detach().cpu(), c.init[i]), i


def test_grid_stride_over_more_items_than_workgroups():
    """2,050 chunks against the 2,048-workgroup cap: the first two workgroups take a second item, the last of them the
    3-element tail, and a 1-element tensor follows in the same launch.  The large tensor has a gradient in two of
    the 12 steps only: its fp64 oracle costs a second per step."""
    c = Case([(2049 * CHUNK + 3,), (1,)], seed=5, only={0: (4, 11)})
    ps = _device_params(c)
    opt = FusedAdamW(c.groups(ps), **DEFAULTS)
    _run(c, ps, lambda s: opt)
    assert opt.last_launches == 1
    c.gate(ps, opt)


def test_a_device_resident_step_moves_to_the_host():
    """A state dict of stock `AdamW(fused=True)` carries `step` on the device; it is read once, then stays on the
    host, so later steps do not wait for the device."""
    c = Case([(5,), (CHUNK + 1,), (3,)], seed=9)
    ps = _device_params(c)
    stock = torch.optim.AdamW(c.groups(ps), fused=True, **DEFAULTS)
    _run(c, ps, lambda s: stock, 0, 4)
    assert all(stock.state[p]["step"].is_cuda for p in ps)
    sd = stock.state_dict()
    for g in sd["param_groups"]:
        g["fused"] = None
    opt = FusedAdamW(c.groups(ps))
    opt.load_state_dict(sd)
    _run(c, ps, lambda s: opt, 4, 5)
    assert all(opt.state[p]["step"].device.type == "cpu" and opt.state[p]["step"].item() == 5 for p in ps)
    grads = [g.cuda() for g in c.grads[5]]
    torch.cuda.set_sync_debug_mode("error")
    try:
        for p, g in zip(ps, grads):
            p.grad = g
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert opt.last_launches == 1 and all(opt.state[p]["step"].item() == 6 for p in ps)


def _joint_layout(rows=257):
    """The joint iteration's groups at small tables: seven decoders of four tensors, ten cameras of six tensors of
    which one camera has gradients, two feature tables.  Returns (groups, live parameters)."""
    gen = torch.Generator().manual_seed(3)

    def par(*shape):
        return torch.nn.Parameter((0.1 * torch.randn(shape, generator=gen)).cuda())

    groups, live = [], []
    for d, (fin, out) in enumerate([(32, 1), (16, 3), (32, 3), (32, 3), (32, 4), (32, 1), (48, 3)]):
        ps = [par(64, fin), par(64), par(out, 64), par(out)]
        groups.append({"params": ps, "lr": 0.01, "weight_decay": 0.0, "name": f"mlp_{d}"})
        live += ps
    for cam in range(10):
        ps = [par(1), par(1), par(3, 3), par(3, 1), par(3), par(3)]
        groups += [{"params": [p], "lr": 0.001, "name": f"cam_{cam}_{k}"} for k, p in enumerate(ps)]
        if cam == 4:
            live += ps
    for name, width in (("geo", 32), ("color", 16)):
        groups.append({"params": [par(rows, width)], "lr": 0.01, "weight_decay": 0.0, "name": name})
        live += groups[-1]["params"]
    return groups, live


def _six_steps():
    groups, live = _joint_layout()
    every = [p for g in groups for p in g["params"]]
    opt = FusedAdamW(groups, **DEFAULTS)
    gen = torch.Generator().manual_seed(11)
    grads = [[torch.randn(p.shape, generator=gen).cuda() for p in live] for _ in range(6)]

    def step(s):
        opt.zero_grad(set_to_none=True)         # fresh gradient blocks every iteration, the reference's way
        for p, g in zip(live, grads[s]):
            p.grad = g
        opt.step()

    step(0)
    torch.cuda.synchronize()
    allocs = torch.cuda.memory_stats()["num_device_alloc"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        for s in range(1, 6):
            step(s)
            assert opt.last_launches == 1
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_stats()["num_device_alloc"] == allocs
    torch.cuda.synchronize()
    assert len(opt.state) == len(live)
    return [p.detach().clone() for p in every] + [opt.state[p][k].clone() for p in live for k in KEYS]


def test_host_behaviour_and_run_to_run_bits():
    a, b = _six_steps(), _six_steps()
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(torch.isfinite(x).all() for x in a)


def test_state_dict_interchange_on_the_device(case):
    """stock -> fused after step 4, fused -> stock after step 8."""
    ps = _device_params(case)
    stock = torch.optim.AdamW(case.groups(ps), **DEFAULTS)
    _run(case, ps, lambda s: stock, 0, 4)
    fused = FusedAdamW(case.groups(ps), lr=1.0, betas=(0.1, 0.1))
    fused.load_state_dict(stock.state_dict())
    _run(case, ps, lambda s: fused, 4, 8)
    assert fused.last_launches == 1
    stock2 = torch.optim.AdamW(case.groups(ps), lr=1.0, betas=(0.1, 0.1))
    stock2.load_state_dict(fused.state_dict())
    _run(case, ps, lambda s: stock2, 8, 12)
    case.gate(ps, stock2)


def test_argument_errors_are_status_codes():
    L = _lib.lib()
    n = ctypes.c_int(-1)
    st = L.pings_adamw_step(None, 1, ctypes.byref(n), None)
    assert st == 1 and b"null job table" in L.pings_last_error() and n.value == 0
    jobs = (_abi.AdamwJob * 2)()
    assert L.pings_adamw_step(jobs, -1, ctypes.byref(n), None) == 1
    assert b"negative job count" in L.pings_last_error()
    jobs[1].n = 5                                   # null pointers with n > 0
    assert L.pings_adamw_step(jobs, 2, ctypes.byref(n), None) == 1
    assert b"null pointer in job" in L.pings_last_error()
    jobs[1].n = -5
    assert L.pings_adamw_step(jobs, 2, None, None) == 1
    jobs[1].n = 0                                   # empty jobs are legal and launch nothing
    n.value = -1
    assert L.pings_adamw_step(jobs, 2, ctypes.byref(n), None) == 0 and n.value == 0
    assert L.pings_adamw_step(None, 0, ctypes.byref(n), None) == 0 and n.value == 0
