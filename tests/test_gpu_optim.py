"""GPU: the recordable optimizers (optim.FusedAdam / FusedAdamW / FusedRMSprop / FusedSGD, a device-side learning rate, global-norm
gradient clipping) -- the names a user puts into the driver's ``getattr(optim, NAME)`` (/root/reference/dss2_run.py:91-92).

* parity over 5 steps against ``torch.optim`` on the CPU in fp64 (``foreach=False``) for 10 configurations x the 4 launch forms
  (separate gradients / flat bucket x host / device step count), parameters AND state; every run twice with equal bits;
* ``FusedAdamax(lr=tensor)`` = ``FusedAdamax(lr=float)`` bit for bit in all forms; the ``dss2_adamax_step*`` exports (adapters that Python
  no longer calls), driven through ctypes with hand-filled tables, = ``FusedAdamax`` bit for bit, and their refusals;
* a tensor ``lr`` changed between replays of a hipGraph and of a launch plan gives the eager steps with those float rates, bit for bit;
  ``StepLR`` over three ``EpochTrainer`` epochs;
* ``clip_grad_norm_``: norm and scaled gradients against fp64, untouched bits above the norm, both gradient layouts, more tensors than
  one by-value launch carries, equal bits twice, torch's non-finite behaviour, and a verified launch plan with clip + FusedAdam;
* ``EpochTrainer`` / ``GraphedTrainer`` with ``max_grad_norm`` = the eager ``train_epoch`` bit for bit; constructing an ``EpochTrainer``
  leaves EVERY optimizer state tensor as it was."""
import ctypes as C
import importlib

import pytest
import torch

from conftest import PKG_NAME, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REG = {"mu_v": 1e-1, "mu_theta": 1e-1, "lam_v": 1e-4, "lam_p": 1e-8, "lam_pf": 1e-6, "lam_reg": 1e2}
STEPS = 5
SHAPES = [(1,), (3,), (33,), (2049,), (22, 32), (128, 128)] + [(7,)] * 100       # 106 tensors: crosses the 80-descriptor by-value chunk
ZERO_GRAD, TINY_GRAD = 2, 4                                                          # tensor with all-zero gradients / gradients x 1e-6

# (fused class, torch class, arguments).  Tolerance: rel_err < 1e-5 per tensor (the project's number for the Adamax parity,
# tests/test_gpu_round2.py) unless torch's OWN fp32 single-tensor run on the GPU is farther than that from the fp64 run; then
# 4 x torch's error, which the test measures (_reference).  Measured on the MI355X, worst tensor over parameters and state,
# the same in all four forms -- torch fp32 / fused kernels:
#   adam 2.25e-07 / 3.26e-07    adam_wd_amsgrad 2.26e-07 / 2.80e-07    adamw 3.64e-07 / 3.64e-07    rmsprop 1.85e-07 / 1.62e-07
#   rmsprop_mom_centered_wd 2.75e-07 / 2.51e-07    sgd 1.50e-07 / 1.50e-07    sgd_mom_damp 2.17e-07 / 2.62e-07
#   sgd_nesterov_wd 3.09e-07 / 2.45e-07    adamax 1.67e-07 / 3.20e-07    adamax_wd 2.17e-07 / 3.90e-07
# torch is under 1e-5 everywhere, so the default tolerance holds for every configuration.
CONFIGS = {
    "adamax": ("FusedAdamax", "Adamax", {}),
    "adamax_wd": ("FusedAdamax", "Adamax", dict(weight_decay=0.01)),
    "adam": ("FusedAdam", "Adam", {}),
    "adam_wd_amsgrad": ("FusedAdam", "Adam", dict(weight_decay=0.01, amsgrad=True)),
    "adamw": ("FusedAdamW", "AdamW", dict(weight_decay=0.01)),
    "rmsprop": ("FusedRMSprop", "RMSprop", {}),
    "rmsprop_mom_centered_wd": ("FusedRMSprop", "RMSprop", dict(momentum=0.9, centered=True, weight_decay=0.01)),
    "sgd": ("FusedSGD", "SGD", dict(lr=0.1)),
    "sgd_mom_damp": ("FusedSGD", "SGD", dict(lr=0.1, momentum=0.9, dampening=0.1)),
    "sgd_nesterov_wd": ("FusedSGD", "SGD", dict(lr=0.1, momentum=0.9, nesterov=True, weight_decay=0.01)),
}
FORMS = [(False, False), (False, True), (True, False), (True, True)]               # (flat bucket, capturable)
FORM_IDS = ["separate-host", "separate-dev", "flat-host", "flat-dev"]


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module(PKG_NAME)
    p._lib.lib()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return p


_DATA = {}


def _data():
    """Initial parameters and the gradients of every step (fresh N(0,1) draws, so the centered RMSprop variance stays away from
    cancellation), fp32 on the CPU; made once and never modified."""
    if not _DATA:
        g = torch.Generator().manual_seed(7)
        _DATA["p0"] = [torch.randn(s, generator=g) for s in SHAPES]
        grads = []
        for _ in range(STEPS):
            gs = [torch.randn(s, generator=g) for s in SHAPES]
            gs[ZERO_GRAD].zero_()
            gs[TINY_GRAD].mul_(1e-6)
            grads.append(gs)
        _DATA["grads"] = grads
    return _DATA["p0"], _DATA["grads"]


def _collect(opt, ps):
    """Parameters, then every state tensor but the step count, in a fixed order, on the CPU."""
    out = [p.detach().cpu() for p in ps]
    for p in ps:
        st = opt.state.get(p, {})
        out += [st[k].detach().cpu() for k in sorted(st) if k != "step" and torch.is_tensor(st[k])]
    return out


def _run_torch(name, kw, device, dtype, steps=STEPS):
    p0, grads = _data()
    ps = [torch.nn.Parameter(p.to(device=device, dtype=dtype)) for p in p0]
    opt = getattr(torch.optim, name)(ps, foreach=False, **kw)
    for k in range(steps):
        for p, g in zip(ps, grads[k]):
            p.grad = g.to(device=device, dtype=dtype)
        opt.step()
    return _collect(opt, ps)


_REF = {}


def _reference(cfg):
    """(fp64 CPU result, error of torch's own fp32 single-tensor GPU run against it) of a configuration, computed once."""
    if cfg not in _REF:
        _, name, kw = CONFIGS[cfg]
        want = _run_torch(name, kw, "cpu", torch.float64)
        t32 = _run_torch(name, kw, DEV, torch.float32)
        _REF[cfg] = (want, max(rel_err(a, b) for a, b in zip(t32, want)))
    return _REF[cfg]


def _run_fused(pkg, cls, kw, flat, capturable, steps=STEPS, lr=None, data=None):
    p0, grads = data or _data()
    ps = [torch.nn.Parameter(p.to(DEV)) for p in p0]
    kw = dict(kw)
    if lr is not None:
        kw["lr"] = lr
    opt = getattr(pkg.optim, cls)(ps, capturable=capturable, **kw)
    sizes = [p.numel() for p in ps]
    for k in range(steps):
        if flat:
            bucket = torch.cat([g.reshape(-1) for g in grads[k]]).to(DEV)
            for p, g in zip(ps, bucket.split(sizes)):
                p.grad = g.view(p.shape)
        else:
            for p, g in zip(ps, grads[k]):
                p.grad = g.to(DEV)
        opt.step()
    torch.cuda.synchronize()
    assert float(opt.param_groups[0]["_step"]) == steps
    assert opt.table_builds == 1                           # one table for the run, in the form asked for
    assert (len(opt._flat_table) == 1) == flat
    return _collect(opt, ps)


@pytest.mark.parametrize("flat,capturable", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_five_steps_match_torch_fp64_and_repeat_bit_for_bit(pkg, cfg, flat, capturable):
    cls, _, kw = CONFIGS[cfg]
    want, torch_err = _reference(cfg)
    tol = 1e-5 if torch_err <= 1e-5 else 4.0 * torch_err
    got = _run_fused(pkg, cls, kw, flat, capturable)
    assert len(got) == len(want)
    errs = [rel_err(a, b) for a, b in zip(got, want)]
    worst = max(errs)
    print(f"{cfg} {FORM_IDS[FORMS.index((flat, capturable))]}: torch fp32 {torch_err:.2e}, fused {worst:.2e}, tolerance {tol:.1e}")
    for i, e in enumerate(errs):
        assert e < tol, (cfg, i, e, tol)
    again = _run_fused(pkg, cls, kw, flat, capturable)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize("flat,capturable", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adamax_with_a_tensor_lr_equals_the_float_lr_kernels_bit_for_bit(pkg, flat, capturable, wd):
    kw = dict(weight_decay=wd)
    a = _run_fused(pkg, "FusedAdamax", kw, flat, capturable, steps=3, lr=3e-3)
    b = _run_fused(pkg, "FusedAdamax", kw, flat, capturable, steps=3, lr=torch.tensor(3e-3, device=DEV))
    assert len(a) == 3 * len(SHAPES)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), (i, (x - y).abs().max().item())


# ---- the Adamax entry points of the header.  FusedAdamax runs dss2_optim_step*, so nothing in Python calls them any more: here they
#      are called as a C user would, with hand-filled tables in their own 40-byte layouts.
ADAPTER_SHAPES = [(1,), (3,), (33,), (2049,)] + [(7,)] * 96       # 100 tensors: crosses the by-value chunk of 80 (and the 96 of the former Adamax kernel)
ADAPTER_STEPS = 3
ADAPTER_HYPER = (3e-3, 0.9, 0.999, 1e-8, 0.01)                     # lr, beta1, beta2, eps, weight_decay
_ADAPTER = {}


def _adapter_data():
    if "data" not in _ADAPTER:
        g = torch.Generator().manual_seed(11)
        p0 = [torch.randn(s, generator=g) for s in ADAPTER_SHAPES]
        _ADAPTER["data"] = (p0, [[torch.randn(s, generator=g) for s in ADAPTER_SHAPES] for _ in range(ADAPTER_STEPS)])
    return _ADAPTER["data"]


def _adapter_reference(pkg, flat, capturable):
    """FusedAdamax on the same data in the same form (the host and the device form their bias corrections separately), once."""
    if (flat, capturable) not in _ADAPTER:
        lr, b1, b2, eps, wd = ADAPTER_HYPER
        _ADAPTER[flat, capturable] = _run_fused(pkg, "FusedAdamax", dict(betas=(b1, b2), eps=eps, weight_decay=wd), flat, capturable,
                                                steps=ADAPTER_STEPS, lr=lr, data=_adapter_data())
    return _ADAPTER[flat, capturable]


@pytest.mark.parametrize("flat,capturable", FORMS, ids=FORM_IDS)
def test_the_adamax_exports_equal_fused_adamax_bit_for_bit(pkg, flat, capturable):
    L, st = pkg._lib.lib(), pkg._lib.stream_ptr(torch.device(DEV))
    p0, grads = _adapter_data()
    ps = [p.to(DEV) for p in p0]
    avg, inf = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    n, sizes = len(ps), [p.numel() for p in ps]
    step_dev = torch.zeros(1, dtype=torch.float32, device=DEV)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    for k in range(ADAPTER_STEPS):
        if flat:
            bucket = torch.cat(grads[k]).to(DEV)
            offs = [sum(sizes[:i]) for i in range(n)]
            # dss2_adamax_flat_desc: param, grad_off, exp_avg, exp_inf, n
            tab = torch.tensor([[p.data_ptr(), o, m.data_ptr(), u.data_ptr(), p.numel()] for p, o, m, u in zip(ps, offs, avg, inf)],
                               dtype=torch.int64).to(DEV)
            assert tab.shape == (n, 5) and tab.is_contiguous()
            rc = L.dss2_adamax_step_flat(tab.data_ptr(), n, max(sizes), bucket.data_ptr(), *ADAPTER_HYPER, 0 if capturable else k + 1,
                                         step_dev.data_ptr() if capturable else None, counter.data_ptr(), st)
            pkg._lib.check(rc, "dss2_adamax_step_flat")
        else:
            gs = [g.to(DEV) for g in grads[k]]
            tab = (pkg._lib.AdamaxDesc * n)()
            assert C.sizeof(tab) == 40 * n
            for d, p, g, m, u in zip(tab, ps, gs, avg, inf):
                d.param, d.grad, d.exp_avg, d.exp_inf, d.n = p.data_ptr(), g.data_ptr(), m.data_ptr(), u.data_ptr(), p.numel()
            if capturable:
                pkg._lib.check(L.dss2_adamax_step_dev(C.addressof(tab), n, *ADAPTER_HYPER, step_dev.data_ptr(), st), "dss2_adamax_step_dev")
            else:
                pkg._lib.check(L.dss2_adamax_step(C.addressof(tab), n, *ADAPTER_HYPER, k + 1, st), "dss2_adamax_step")
    torch.cuda.synchronize()
    if capturable:
        assert float(step_dev) == ADAPTER_STEPS          # advanced by the launches themselves
        if flat:
            assert int(counter) == 0                     # the last workgroup to arrive left the arrival word at zero for the next launch
    got = [p.cpu() for p in ps] + [t.cpu() for m, u in zip(avg, inf) for t in (m, u)]      # _collect's order: exp_avg, exp_inf per tensor
    want = _adapter_reference(pkg, flat, capturable)
    assert len(got) == len(want) == 3 * n
    for i, (x, y) in enumerate(zip(got, want)):
        assert torch.equal(x, y), (i, (x - y).abs().max().item())


def test_the_adamax_exports_refuse_what_they_refused(pkg):
    L, st = pkg._lib.lib(), pkg._lib.stream_ptr(torch.device(DEV))
    p, g, m, u = (torch.zeros(4, device=DEV) for _ in range(4))
    word = torch.zeros(2, dtype=torch.int32, device=DEV)
    host = (pkg._lib.AdamaxDesc * 1)()
    host[0].param, host[0].grad, host[0].exp_avg, host[0].exp_inf, host[0].n = p.data_ptr(), g.data_ptr(), m.data_ptr(), u.data_ptr(), 4
    holed = (pkg._lib.AdamaxDesc * 1)()
    holed[0].param, holed[0].grad, holed[0].exp_avg, holed[0].n = p.data_ptr(), g.data_ptr(), m.data_ptr(), 4
    flat = torch.tensor([[p.data_ptr(), 0, m.data_ptr(), u.data_ptr(), 4]], dtype=torch.int64).to(DEV)
    H, T, G, SD, CT = ADAPTER_HYPER, flat.data_ptr(), g.data_ptr(), word.data_ptr(), word.data_ptr() + 4
    refused = [
        ("adamax_step: ", lambda: L.dss2_adamax_step(None, 1, *H, 1, st)),                               # null table
        ("adamax_step: ", lambda: L.dss2_adamax_step(C.addressof(host), 1, *H, 0, st)),                  # step < 1
        ("adamax_step: ", lambda: L.dss2_adamax_step(C.addressof(holed), 1, *H, 1, st)),                 # a descriptor without exp_inf
        ("adamax_step_dev: ", lambda: L.dss2_adamax_step_dev(None, 1, *H, SD, st)),
        ("adamax_step_dev: ", lambda: L.dss2_adamax_step_dev(C.addressof(host), 1, *H, None, st)),
        ("adamax_step_flat: ", lambda: L.dss2_adamax_step_flat(None, 1, 4, G, *H, 1, None, None, st)),
        ("adamax_step_flat: ", lambda: L.dss2_adamax_step_flat(T, 1, 4, None, *H, 1, None, None, st)),
        ("adamax_step_flat: ", lambda: L.dss2_adamax_step_flat(T, 65536, 4, G, *H, 1, None, None, st)),  # more rows than a grid has
        ("adamax_step_flat: ", lambda: L.dss2_adamax_step_flat(T, 1, 4, G, *H, -1, SD, CT, st)),
        ("adamax_step_flat: ", lambda: L.dss2_adamax_step_flat(T, 1, 4, G, *H, 0, None, CT, st)),        # step == 0 needs step_dev ...
        ("adamax_step_flat: ", lambda: L.dss2_adamax_step_flat(T, 1, 4, G, *H, 0, SD, None, st)),        # ... and counter
    ]
    for i, (who, call) in enumerate(refused):
        assert call() == 2, i
        assert L.dss2_last_error().decode().startswith(who), (i, L.dss2_last_error())
    torch.cuda.synchronize()
    assert not p.any() and not m.any() and not u.any() and not word.any()      # nothing was launched


# ---- device-side learning rate in recorded steps
MPN_ARGS = (8, 6, 2, 32, 2, 2, 0.0)


def _mpn_step(pkg, n_graphs=4, seed=0):
    torch.manual_seed(seed)
    b = pkg.synthetic.make_batch(["cigre14"], n_graphs, seed=seed, violate=0.3)
    x, ei, ea = b["x"].to(DEV), b["edge_index"].to(DEV), b["edge_attr"].to(DEV)
    st = tuple(s.to(DEV) for s in b["stats"])
    model = pkg.MPN(*MPN_ARGS).to(DEV)
    params = list(model.parameters())
    seen = {}

    def step(opt=None, max_norm=None):
        for p in params:
            p.grad = None
        out = model(x[:, :8], ei, ea[:, :6])
        loss = pkg.gsp_wls_edge(input=x[:, :8], edge_input=ea[:, :6], output=out, x_mean=st[0], x_std=st[1], edge_mean=st[2], edge_std=st[3],
                                edge_index=ei, reg_coefs=REG, num_samples=None, node_param=x[:, 8:], edge_param=ea[:, 6:])
        loss.backward(pkg.data.unit_grad(loss))
        if max_norm is not None:
            seen["norm"] = pkg.optim.clip_grad_norm_(params, max_norm)
        if opt is not None:
            opt.step()
        seen["loss"] = loss
        return loss
    return model, params, step, seen


@pytest.mark.parametrize("how", ["graph", "plan"])
def test_a_tensor_lr_changed_between_replays_gives_the_eager_steps_with_those_rates(pkg, how):
    m1, p1, step1, _ = _mpn_step(pkg)
    m2, p2, step2, _ = _mpn_step(pkg)
    m2.load_state_dict(m1.state_dict())
    lr = torch.tensor(3e-3, device=DEV)
    o1 = pkg.optim.FusedAdam(p1, lr=3e-3, capturable=True)
    o2 = pkg.optim.FusedAdam(p2, lr=lr, capturable=True)
    if how == "graph":
        rec = pkg.graphs.GraphedStep(lambda: step2(o2), warmup=1)          # one real step (the capture itself runs nothing)
        real = 1
    else:
        rec = pkg.graphs.PlannedStep(lambda: step2(o2), warmup=1)          # warm-up + recording: two real steps
        real = 2
    for _ in range(real):
        step1(o1)
    for rate in (3e-3, 1e-3, 0.0):
        lr.fill_(rate)
        o1.param_groups[0]["lr"] = float(lr)                                # (the fp32 value the kernels read)
        before = [p.detach().clone() for p in p2]
        rec.replay()
        step1(o1)
        torch.cuda.synchronize()
        for a, b in zip(p1, p2):
            assert torch.equal(a, b), (rate, (a - b).abs().max().item())
        moved = any(not torch.equal(a, b) for a, b in zip(before, p2))
        assert moved == (rate != 0.0), rate                                 # at 0 the parameters do not move; else the replay trains
    assert float(o2.param_groups[0]["_step"]) == real + 3 and o2.param_groups[0]["lr"] is lr


def _dataset(pkg, S, seed=4):
    full = pkg.synthetic.make_batch(["cigre14"], S, seed=seed, violate=0.2)
    ds = pkg.dataset.DeviceDataset.from_batch(full, device=DEV)
    return ds, tuple(s.to(DEV) for s in full["stats"])


def _twin_models(pkg, seed=1):
    torch.manual_seed(seed)
    m1, m2 = pkg.MPN(*MPN_ARGS).to(DEV), pkg.MPN(*MPN_ARGS).to(DEV)
    m2.load_state_dict(m1.state_dict())
    return m1, m2


def test_step_lr_schedules_the_replayed_epochs(pkg):
    ds, stats = _dataset(pkg, 10)
    m1, m2 = _twin_models(pkg)
    lr = torch.tensor(1e-2, device=DEV)
    o1 = pkg.optim.FusedAdam(m1.parameters(), lr=1e-2, capturable=True)
    o2 = pkg.optim.FusedAdam(m2.parameters(), lr=lr, capturable=True)
    tr = pkg.runner.EpochTrainer(m2, o2, stats, REG, ds, 4, shuffle=False, mode="graph")
    sched = torch.optim.lr_scheduler.StepLR(o2, step_size=1, gamma=0.1)
    rates = []
    for _ in range(3):
        rates.append(float(lr))
        o1.param_groups[0]["lr"] = float(lr)
        pkg.runner.train_epoch(m1, o1, pkg.dataset.DataLoader(ds, batch_size=4, shuffle=False), stats, REG)
        tr.train_epoch()
        sched.step()                                                        # fills the tensor the recorded launches read
        assert o2.param_groups[0]["lr"] is lr
    torch.cuda.synchronize()
    assert rates == pytest.approx([1e-2, 1e-3, 1e-4], rel=1e-6)
    for a, b in zip(m1.parameters(), m2.parameters()):
        assert torch.equal(a, b), (a - b).abs().max().item()


# ---- clipping
CLIP_SHAPES = [(1,), (3,), (33,), (2049,), (22, 32), (128, 128)] + [(7,)] * 200       # 206 tensors: two by-value launches (192 each)


def _clip_grads(flat, seed=3):
    g = torch.Generator().manual_seed(seed)
    gs = [torch.randn(s, generator=g) for s in CLIP_SHAPES]
    gs[ZERO_GRAD].zero_()
    gs[TINY_GRAD].mul_(1e-6)
    ps = [torch.nn.Parameter(torch.zeros(s, device=DEV)) for s in CLIP_SHAPES]
    if flat:
        bucket = torch.cat([x.reshape(-1) for x in gs]).to(DEV)
        for p, x in zip(ps, bucket.split([p.numel() for p in ps])):
            p.grad = x.view(p.shape)
    else:
        for p, x in zip(ps, gs):
            p.grad = x.to(DEV)
    norm64 = torch.cat([x.reshape(-1) for x in gs]).double().norm().item()
    return ps, gs, norm64


@pytest.mark.parametrize("flat", [False, True], ids=["separate", "flat"])
def test_clip_grad_norm_against_fp64(pkg, flat):
    ps, gs, norm64 = _clip_grads(flat)
    # above the norm: the coefficient is 1 and every gradient keeps its bits
    norm = pkg.optim.clip_grad_norm_(ps, 2.0 * norm64)
    assert norm.dtype == torch.float32 and norm.is_cuda and norm.dim() == 0
    assert abs(float(norm) - norm64) <= 1e-6 * norm64, (float(norm), norm64)      # fp64 accumulation, one rounding to fp32
    for p, x in zip(ps, gs):
        assert torch.equal(p.grad.cpu(), x)
    # at half the norm: g * coef
    max_norm = 0.5 * norm64
    norm = pkg.optim.clip_grad_norm_(ps, max_norm)
    assert abs(float(norm) - norm64) <= 1e-6 * norm64
    coef = max_norm / (norm64 + 1e-6)
    for i, (p, x) in enumerate(zip(ps, gs)):
        want = x.double() * coef
        assert bool(((p.grad.cpu().double() - want).abs() <= 1e-6 * want.abs()).all()), i
    first = [p.grad.clone() for p in ps]
    # the same again from the same gradients: equal bits (no float atomics)
    ps2, _, _ = _clip_grads(flat)
    norm2 = pkg.optim.clip_grad_norm_(ps2, max_norm)
    assert torch.equal(norm, norm2) and all(torch.equal(a, p.grad) for a, p in zip(first, ps2))


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_clip_grad_norm_with_a_non_finite_gradient_is_torchs(pkg, bad):
    ps, gs, _ = _clip_grads(flat=False)
    ps[3].grad[5] = bad
    twins = [torch.nn.Parameter(torch.zeros_like(p)) for p in ps]
    for q, p in zip(twins, ps):
        q.grad = p.grad.clone()
    want = torch.nn.utils.clip_grad_norm_(twins, 1.0, error_if_nonfinite=False, foreach=False)
    got = pkg.optim.clip_grad_norm_(ps, 1.0)
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.isinf(got), torch.isinf(want))
    for p, q in zip(ps, twins):
        assert torch.equal(torch.isnan(p.grad), torch.isnan(q.grad)) and torch.equal(torch.isinf(p.grad), torch.isinf(q.grad))


def test_a_launch_plan_carries_clip_and_fused_adam(pkg):
    model, params, step, seen = _mpn_step(pkg)
    lr = torch.tensor(0.0, device=DEV)          # the parameters stand still, so a replay must reproduce loss, clipped gradients and norm
    opt = pkg.optim.FusedAdam(params, lr=lr, capturable=True)
    bare = pkg.graphs.PlannedStep(lambda: step())
    plan = pkg.graphs.PlannedStep(lambda: step(opt, max_norm=1e-3), verify=lambda: [seen["loss"], seen["norm"]] + [p.grad for p in params])
    assert plan.n_launches == bare.n_launches + 3                            # two clipping launches and ONE optimizer launch (flat bucket)
    assert float(seen["norm"]) > 1e-3                                        # (the clip is active)
    done = float(opt.param_groups[0]["_step"])
    assert done == 4.0                                                       # 2 warm-ups, the recording, the verifying replay: the plan steps
    lr.fill_(1e-3)
    before = [p.detach().clone() for p in params]
    plan.replay()
    torch.cuda.synchronize()
    assert float(opt.param_groups[0]["_step"]) == 5.0 and any(not torch.equal(a, b) for a, b in zip(before, params))


# ---- trainers
def _opt_state(opt):
    out = []
    for g in opt.param_groups:
        out.append(g["_step"].detach().clone())
        for p in g["params"]:
            st = opt.state[p]
            out += [st[k].detach().clone() for k in sorted(st) if k != "step"]
    return out


@pytest.mark.parametrize("mode", ["plan", "graph"])
def test_epoch_trainer_with_fused_adam_and_clipping_equals_the_eager_epoch(pkg, mode):
    S, B = 10, 4                                 # two full steps and a remainder of 2
    ds, stats = _dataset(pkg, S)
    m1, m2 = _twin_models(pkg)
    o1 = pkg.optim.FusedAdam(m1.parameters(), lr=3e-3, capturable=True)
    o2 = pkg.optim.FusedAdam(m2.parameters(), lr=3e-3, capturable=True)
    batches = list(pkg.dataset.DataLoader(ds, batch_size=B, shuffle=False))
    assert [b.num_graphs for b in batches] == [4, 4, 2]
    for m, o in ((m1, o1), (m2, o2)):            # one eager step first: the optimizer state the trainer is given is not all zeros
        pkg.runner.train_epoch(m, o, batches[:1], stats, REG, max_grad_norm=1.0)
    before_p = [p.detach().clone() for p in m2.parameters()]
    before_s = _opt_state(o2)
    assert len(before_s) == 1 + 2 * len(before_p) and float(before_s[0]) == 1.0
    tr = pkg.runner.EpochTrainer(m2, o2, stats, REG, ds, B, shuffle=False, mode=mode, max_grad_norm=1.0)
    torch.cuda.synchronize()
    # recording the steps trained on real batches; the trainer restored EVERY state tensor it consumed (exp_avg_sq too)
    assert all(torch.equal(a, b) for a, b in zip(before_p, m2.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(before_s, _opt_state(o2)))
    for _ in range(2):
        # eager: one train_epoch per batch, so every step's loss comes back with its own bits
        want = [pkg.runner.train_epoch(m1, o1, [b], stats, REG, max_grad_norm=1.0) for b in batches]
        tr.train_epoch()
        total, steps = tr.acc.tolist()           # fp64 sum of the steps' fp32 losses, in order
        assert steps == 3.0 and total == sum(want[1:], want[0]), (total, want)
        for a, b in zip(m1.parameters(), m2.parameters()):
            assert torch.equal(a, b), (a - b).abs().max().item()
    assert all(torch.equal(a, b) for a, b in zip(_opt_state(o1), _opt_state(o2)))


def test_graphed_trainer_with_fused_sgd_and_clipping_equals_eager_steps(pkg):
    ds, stats = _dataset(pkg, 4)
    m1, m2 = _twin_models(pkg)
    kw = dict(lr=1e-2, momentum=0.9, dampening=0.1, capturable=True)
    o1, o2 = pkg.optim.FusedSGD(m1.parameters(), **kw), pkg.optim.FusedSGD(m2.parameters(), **kw)
    batch = list(pkg.dataset.DataLoader(ds, batch_size=4, shuffle=False))
    tr = pkg.runner.GraphedTrainer(m2, o2, stats, REG, max_grad_norm=1.0)
    for _ in range(3):                           # the capture's warm-up step (buf = g), then two replays
        want = pkg.runner.train_epoch(m1, o1, batch, stats, REG, max_grad_norm=1.0)
        got = pkg.runner.train_epoch_graphed(tr, batch)
        assert got == want
        for a, b in zip(m1.parameters(), m2.parameters()):
            assert torch.equal(a, b), (a - b).abs().max().item()
