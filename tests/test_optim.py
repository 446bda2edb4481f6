"""FusedAdamW off the GPU: the stock path for CPU tensors, state-dict interchange, rejected options, install / uninstall
and the ABI constants.  The kernel itself is tested in test_optim_gpu.py."""
import types

import pytest
import torch

import abi_header as hdr
from pings_amd import _abi
from pings_amd.optim import CHUNK, MAX_JOBS, FusedAdamW, install, uninstall

SHAPES = [(5, 3), (7,), (), (2, 3, 4)]


def _params(seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g, dtype=dtype)) for s in SHAPES]


def _groups(ps):
    return [{"params": ps[:2], "lr": 0.01, "weight_decay": 0.0, "name": "a"},
            {"params": ps[2:], "lr": 0.003, "name": "b"}]


def _set_grads(ps, step, skip=()):
    g = torch.Generator().manual_seed(100 + step)
    for i, p in enumerate(ps):
        p.grad = None if i in skip else torch.randn(p.shape, generator=g, dtype=p.dtype)


def test_cpu_tensors_take_the_stock_path_bit_for_bit():
    a, b = _params(), _params()
    b[1] = torch.nn.Parameter(b[1].detach().double())       # another dtype in the same optimiser
    a[1] = torch.nn.Parameter(a[1].detach().double())
    stock = torch.optim.AdamW(_groups(a), betas=(0.9, 0.99), eps=1e-15, foreach=False)
    fused = FusedAdamW(_groups(b), betas=(0.9, 0.99), eps=1e-15)
    for s in range(5):
        skip = (3,) if s % 2 else ()            # a parameter without a gradient does not advance
        _set_grads(a, s, skip)
        _set_grads(b, s, skip)
        stock.step()
        fused.step()
        assert fused.last_launches == 0
    for x, y in zip(a, b):
        assert torch.equal(x, y)
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(stock.state[x][k], fused.state[y][k]), k
    assert fused.state[b[3]]["step"].item() == 3 and fused.state[b[0]]["step"].item() == 5
    assert fused.state[b[0]]["step"].device.type == "cpu" and fused.state[b[0]]["step"].dtype == torch.float32


def test_non_contiguous_and_sparse_gradients():
    base = torch.randn(4, 6)
    p = torch.nn.Parameter(base.clone().t())                # non-contiguous parameter
    q = torch.nn.Parameter(base.clone().t())
    stock, fused = torch.optim.AdamW([p], foreach=False), FusedAdamW([q])
    for s in range(3):
        p.grad = torch.full_like(p, 0.1 * (s + 1))
        q.grad = torch.full_like(q, 0.1 * (s + 1))
        stock.step()
        fused.step()
    assert torch.equal(p, q)
    q.grad = torch.zeros(6, 4).to_sparse()
    with pytest.raises(RuntimeError, match="sparse"):
        fused.step()


def test_state_dict_round_trips_stock_fused_stock():
    a, b, c, ref = _params(), _params(), _params(), _params()
    opts = [torch.optim.AdamW(_groups(a), betas=(0.9, 0.99), foreach=False), FusedAdamW(_groups(b), betas=(0.5, 0.5)),
            torch.optim.AdamW(_groups(c), betas=(0.5, 0.5), foreach=False)]
    whole = torch.optim.AdamW(_groups(ref), betas=(0.9, 0.99), foreach=False)
    sets = [a, b, c]
    for leg in range(3):
        if leg:
            with torch.no_grad():
                for x, y in zip(sets[leg], sets[leg - 1]):
                    x.copy_(y)
            opts[leg].load_state_dict(opts[leg - 1].state_dict())
        for s in range(2 * leg, 2 * leg + 2):
            _set_grads(sets[leg], s)
            _set_grads(ref, s)
            opts[leg].step()
            whole.step()
    for x, y in zip(c, ref):
        assert torch.equal(x, y)
    sd = opts[1].state_dict()
    assert [g["name"] for g in sd["param_groups"]] == ["a", "b"]
    assert sd["param_groups"][0]["betas"] == (0.9, 0.99)    # loaded hyper-parameters replace the constructor's
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    assert opts[2].state[c[0]]["step"].item() == 6


@pytest.mark.parametrize("kw", [{"amsgrad": True}, {"maximize": True}, {"capturable": True}, {"differentiable": True},
                                {"fused": True}, {"lr": torch.tensor(0.01)}])
def test_rejected_options_raise(kw):
    with pytest.raises(ValueError):
        FusedAdamW(_params(), **kw)


def test_rejected_options_inside_a_group_raise():
    ps = _params()
    with pytest.raises(ValueError, match="amsgrad"):
        FusedAdamW([{"params": ps[:2]}, {"params": ps[2:], "amsgrad": True}])


def _stub_modules(adam=True):
    ps = _params()
    tools = types.ModuleType("stub_tools")

    def setup_optimizer(lr_scale=1.0):
        """the stub's own"""
        groups = [{"params": ps[:2], "lr": 0.01 * lr_scale, "weight_decay": 0.0, "name": "sdf_mlp_param"},
                  {"params": ps[2:], "lr": 0.003, "name": "cam_0_dr"}]
        if adam:
            return torch.optim.AdamW(groups, betas=(0.9, 0.99), eps=1e-15)
        return torch.optim.SGD(groups, momentum=0.9)

    tools.setup_optimizer = setup_optimizer
    mapper = types.ModuleType("stub_mapper")
    mapper.setup_optimizer = setup_optimizer                # `from utils.tools import setup_optimizer`
    return tools, mapper, setup_optimizer, ps


def test_install_wraps_setup_optimizer_and_uninstall_restores_it():
    tools, mapper, orig, ps = _stub_modules()
    install(tools, mapper)
    assert tools.setup_optimizer is not orig and mapper.setup_optimizer is tools.setup_optimizer
    opt = mapper.setup_optimizer(lr_scale=2.0)
    assert type(opt) is FusedAdamW
    want = orig(lr_scale=2.0)
    assert len(opt.param_groups) == 2
    for g, w in zip(opt.param_groups, want.param_groups):
        assert all(x is y for x, y in zip(g["params"], w["params"]))
        assert {k: v for k, v in g.items() if k != "params"} == {k: v for k, v in w.items() if k != "params"}
    assert [g["name"] for g in opt.param_groups] == ["sdf_mlp_param", "cam_0_dr"]
    assert opt.param_groups[0]["lr"] == 0.02 and opt.param_groups[0]["weight_decay"] == 0.0
    assert opt.param_groups[1]["weight_decay"] == 0.01 and opt.param_groups[1]["betas"] == (0.9, 0.99)
    assert opt.param_groups[1]["eps"] == 1e-15
    wrapped = tools.setup_optimizer
    install(tools, mapper)                                  # twice: nothing is wrapped twice
    assert tools.setup_optimizer is wrapped
    uninstall(tools, mapper)
    assert tools.setup_optimizer is orig and mapper.setup_optimizer is orig
    assert type(tools.setup_optimizer()) is torch.optim.AdamW


def test_install_passes_another_optimiser_through():
    tools, mapper, orig, _ = _stub_modules(adam=False)
    install(tools, mapper)
    assert type(tools.setup_optimizer()) is torch.optim.SGD
    uninstall(tools, mapper)
    assert mapper.setup_optimizer is orig


def test_abi_constants_equal_the_header():
    d = hdr.defines()
    assert _abi.ADAMW_MAX_JOBS == d["PINGS_ADAMW_MAX_JOBS"] == MAX_JOBS
    assert _abi.ADAMW_CHUNK == d["PINGS_ADAMW_CHUNK"] == CHUNK
    assert _abi.ABI_VERSION == d["PINGS_ABI_VERSION"]
    import ctypes
    assert ctypes.sizeof(_abi.AdamwJob) * MAX_JOBS + 8 * MAX_JOBS + 8 <= 4096   # job table + prefix + count
