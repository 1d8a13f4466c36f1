"""CPU: the fused optimizers' host side (optim.py) -- constructor defaults and refusals are torch's, and the checkpoints are torch's
format in both directions (the driver saves ``optimizer_state_dict``, /root/reference/dss2_run.py:240-247): the state of a stepped
``torch.optim`` class loads into the fused class and comes out again with the same keys and values; a fresh fused optimizer's export
loads into the torch class.  Stepping itself needs the GPU (tests/test_gpu_optim.py)."""
import copy
import inspect

import pytest
import torch

from conftest import load_pkg

# (fused class, torch class, constructor arguments)
CONFIGS = [
    ("FusedAdam", torch.optim.Adam, {}),
    ("FusedAdam", torch.optim.Adam, dict(weight_decay=0.01, amsgrad=True)),
    ("FusedAdamW", torch.optim.AdamW, dict(weight_decay=0.01)),
    ("FusedRMSprop", torch.optim.RMSprop, {}),
    ("FusedRMSprop", torch.optim.RMSprop, dict(momentum=0.9, centered=True, weight_decay=0.01)),
    ("FusedSGD", torch.optim.SGD, dict(lr=0.1)),
    ("FusedSGD", torch.optim.SGD, dict(lr=0.1, momentum=0.9, dampening=0.1)),
    ("FusedSGD", torch.optim.SGD, dict(lr=0.1, momentum=0.9, nesterov=True, weight_decay=0.01)),
    ("FusedAdamax", torch.optim.Adamax, {}),
]
IDS = [f"{n}-{'-'.join(kw) or 'default'}" for n, _, kw in CONFIGS]


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in [(3,), (2, 4), (1,)]]


def _step_torch(opt, ps, steps, seed=1):
    g = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()


@pytest.mark.parametrize("name,ref", [("FusedAdam", torch.optim.Adam), ("FusedAdamW", torch.optim.AdamW),
                                      ("FusedRMSprop", torch.optim.RMSprop), ("FusedSGD", torch.optim.SGD)])
def test_constructor_defaults_are_torchs(name, ref):
    pkg = load_pkg()
    mine = getattr(pkg.optim, name)
    want = inspect.signature(ref.__init__).parameters
    got = inspect.signature(mine.__init__).parameters
    hyper = {"FusedAdam": ["lr", "betas", "eps", "weight_decay", "amsgrad"], "FusedAdamW": ["lr", "betas", "eps", "weight_decay", "amsgrad"],
             "FusedRMSprop": ["lr", "alpha", "eps", "weight_decay", "momentum", "centered"],
             "FusedSGD": ["lr", "momentum", "dampening", "weight_decay", "nesterov"]}[name]
    assert list(got)[2:2 + len(hyper)] == hyper          # (self, params, then torch's positional order)
    for k in hyper:
        assert got[k].default == want[k].default, (k, got[k].default, want[k].default)
    assert "capturable" in got and got["capturable"].default is False
    opt = mine(_params())
    for k in hyper:
        assert opt.defaults[k] == want[k].default and opt.param_groups[0][k] == want[k].default


@pytest.mark.parametrize("name", ["FusedAdam", "FusedAdamW", "FusedRMSprop", "FusedSGD"])
def test_what_the_kernels_do_not_do_is_refused(name):
    pkg = load_pkg()
    mine = getattr(pkg.optim, name)
    for kw in (dict(maximize=True), dict(foreach=True), dict(fused=True), dict(differentiable=True)):
        with pytest.raises(ValueError, match="not supported"):
            mine(_params(), **kw)
    mine(_params(), maximize=False, foreach=None, fused=None, differentiable=False)       # torch's defaults, spelled out, are fine
    with pytest.raises(ValueError):
        mine(_params(), lr=-1.0)
    with pytest.raises(ValueError, match="fp32 element"):
        mine(_params(), lr=torch.zeros(2))
    with pytest.raises(ValueError, match="fp32 element"):
        mine(_params(), lr=torch.zeros((), dtype=torch.float64))
    if name == "FusedSGD":
        with pytest.raises(ValueError, match="Nesterov"):
            mine(_params(), nesterov=True)
        with pytest.raises(ValueError, match="Nesterov"):
            mine(_params(), nesterov=True, momentum=0.9, dampening=0.1)


def test_stepping_cpu_parameters_is_an_error_not_a_fallback():
    pkg = load_pkg()
    ps = _params()
    for p in ps:
        p.grad = torch.ones_like(p)
    for name in ("FusedAdam", "FusedAdamW", "FusedRMSprop", "FusedSGD", "FusedAdamax"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            getattr(pkg.optim, name)(ps).step()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.optim.clip_grad_norm_(ps, 1.0)


@pytest.mark.parametrize("name,ref,kw", CONFIGS, ids=IDS)
def test_a_torch_checkpoint_round_trips_through_the_fused_class(name, ref, kw):
    pkg = load_pkg()
    ps = _params()
    o_ref = ref(ps, foreach=False, **kw)
    _step_torch(o_ref, ps, 3)
    want = copy.deepcopy(o_ref.state_dict())
    mine = getattr(pkg.optim, name)([torch.nn.Parameter(p.detach().clone()) for p in ps], **kw)
    mine.load_state_dict(copy.deepcopy(want))
    mine.init_state()                                       # (what a recorded step calls first: must keep the loaded state and count)
    got = copy.deepcopy(mine.state_dict())
    assert set(got["state"]) == set(want["state"])
    for i, st in want["state"].items():
        assert set(got["state"][i]) == set(st), (i, set(got["state"][i]), set(st))
        for k, v in st.items():
            assert torch.equal(torch.as_tensor(got["state"][i][k]), torch.as_tensor(v)), (i, k)
    steps = [st["step"] for st in got["state"].values() if "step" in st]
    assert len({s.data_ptr() for s in steps}) == len(steps)                                # independent clones, not the shared tensor
    assert "_step" not in got["param_groups"][0]
    for k in kw:
        assert got["param_groups"][0][k] == want["param_groups"][0][k]
    # ... and back: torch's class loads the re-export and goes on exactly like the optimizer the checkpoint came from
    ps2 = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    o2 = ref(ps2, foreach=False, **kw)
    o2.load_state_dict(got)
    _step_torch(o_ref, ps, 2, seed=5)
    _step_torch(o2, ps2, 2, seed=5)
    assert all(torch.equal(a, b) for a, b in zip(ps, ps2))


@pytest.mark.parametrize("name,ref,kw", CONFIGS, ids=IDS)
def test_a_fresh_fused_optimizer_exports_what_torch_loads(name, ref, kw):
    pkg = load_pkg()
    ps = _params()
    for with_init in (False, True):
        mine = getattr(pkg.optim, name)(ps, **kw)
        if with_init:
            mine.init_state()                               # state tensors exist (for a capture), nothing has been stepped
        sd = copy.deepcopy(mine.state_dict())
        if name != "FusedAdamax":                           # torch's class holds nothing before its first step (Adamax: zeros and step 0, as ever)
            assert sd["state"] == {}, sd["state"]
        ps_a = [torch.nn.Parameter(p.detach().clone()) for p in ps]
        ps_b = [torch.nn.Parameter(p.detach().clone()) for p in ps]
        o_a, o_b = ref(ps_a, foreach=False, **kw), ref(ps_b, foreach=False, **kw)
        o_a.load_state_dict(sd)
        _step_torch(o_a, ps_a, 2)
        _step_torch(o_b, ps_b, 2)
        assert all(torch.equal(a, b) for a, b in zip(ps_a, ps_b))


def test_sgd_keeps_its_step_count_to_itself():
    """torch.optim.SGD has no ``step`` in its state; the fused kernels need one (the first step's buffer is the gradient): it is
    internal, and a loaded momentum buffer counts as stepped."""
    pkg = load_pkg()
    ps = _params()
    o_ref = torch.optim.SGD(ps, lr=0.1, momentum=0.9, dampening=0.1)
    _step_torch(o_ref, ps, 2)
    mine = pkg.optim.FusedSGD([torch.nn.Parameter(p.detach().clone()) for p in ps], lr=0.1, momentum=0.9, dampening=0.1)
    mine.load_state_dict(copy.deepcopy(o_ref.state_dict()))
    mine.init_state()
    assert float(mine.param_groups[0]["_step"]) >= 1.0
    sd = mine.state_dict()
    assert all(set(st) == {"momentum_buffer"} for st in sd["state"].values()) and len(sd["state"]) == len(ps)
    plain = pkg.optim.FusedSGD(_params(), lr=0.1)
    plain.init_state()
    plain.param_groups[0]["_step"] += 3.0                    # as after three steps: still nothing to export without momentum
    assert plain.state_dict()["state"] == {}


def test_schedulers_fill_a_tensor_lr_in_place_and_a_checkpoint_keeps_the_tensor():
    """The recorded launches read the lr TENSOR: torch's schedulers must update it in place (they do: ``fill_``), and loading a
    checkpoint must not swap it for another tensor."""
    pkg = load_pkg()
    for name in ("FusedAdamax", "FusedAdam", "FusedAdamW", "FusedRMSprop", "FusedSGD"):
        lr = torch.tensor(0.5)
        opt = getattr(pkg.optim, name)(_params(), lr=lr)
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
        sched.step()
        sched.step()
        assert opt.param_groups[0]["lr"] is lr and float(lr) == 0.125
        plateau = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, factor=0.5, patience=0)
        plateau.step(1.0)
        plateau.step(2.0)
        assert opt.param_groups[0]["lr"] is lr and float(lr) == 0.0625
        sd = copy.deepcopy(opt.state_dict())
        lr.fill_(7.0)
        opt.load_state_dict(sd)
        assert opt.param_groups[0]["lr"] is lr and float(lr) == 0.0625
