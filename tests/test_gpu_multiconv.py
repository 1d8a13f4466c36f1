"""GPU: MultiConvNet, WrappedMultiConv and ChebConv (the reference's networks.py:737-835 with PyG's ChebConv) on the kernels of
csrc/dss2_cheb.hip, against the reference's own model (tests/golden/case_multiconv_*.npz) and the restatement tests/cheb_oracle.py
in fp64.

Outputs within max(1e-5, 4 x the error of the same restatement run in fp32), max-normalised; parameter, input and edge-weight
gradients within max(max(1e-4, 8 / N), 4 x the fp32 restatement's error) (the convention of test_gpu_gnn_dsse.py): the bound is
measured on the reference arithmetic, never on the code under test, and every error is printed next to it.  Then the smallest shapes
that can go wrong (one node, a path, a star whose arg-max is the hub's degree or an edge, ragged and slab-capped batches, 1 and 3
parallel convs, widths that change), a caller's edge_weight gradient with and without a given lambda_max, dropout with the kernels'
own masks handed to the oracle, bit-identical reruns, the NaN pattern of all-zero weights, a training step as a launch plan and as a
hipGraph, and broken argument structs."""
import ctypes as C
import importlib
import types

import pytest
import torch

import cheb_oracle as cor
from conftest import PKG_NAME, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module(PKG_NAME)


def _note(name, **kv):
    print(f"[multiconv] {name}: " + ", ".join(f"{k} {v}" for k, v in kv.items()))


def _check(name, got, want64, got32, n_nodes, grad):
    """got (GPU) against want64 within the bound the fp32 restatement got32 sets; NaN patterns must agree."""
    got, want64 = got.detach().double().cpu(), want64.detach().double()
    nan = torch.isnan(want64)
    assert torch.equal(torch.isnan(got), nan), name
    if bool(nan.all()):
        return
    g, w, g32 = got[~nan], want64[~nan], got32.detach().double()[~nan]
    floor = max(1e-4, 8.0 / n_nodes) if grad else 1e-5
    if float(w.abs().max()) == 0:
        err, bound = float(g.abs().max()), max(floor * 1e-3, 4 * float(g32.abs().max()))      # an exactly zero gradient (K = 1)
    else:
        err, bound = rel_err(g, w), max(floor, 4 * rel_err(g32, w))
    _note(name, err=f"{err:.3g}", bound=f"{bound:.3g}")
    assert err <= bound, (name, err, bound)


def _oracle_net(sd, t, dtype, masks=None):
    ref = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    x = t["x"].to(dtype).clone().requires_grad_(True)
    out = cor.multiconv(ref, x, t["edge_index"], t["edge_attr"].to(dtype), masks)
    out.backward(t["gout"].to(dtype))
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in ref.items()}
    return out.detach(), grads, x.grad[:, 4:4 + 8]


def _gpu_net(pkg, sd, t, args, seed=None):
    net = pkg.MultiConvNet(*args).to(DEV)
    net.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    x = t["x"].float().to(DEV).requires_grad_(True)
    data = types.SimpleNamespace(x=x, edge_index=t["edge_index"].to(DEV), edge_attr=t["edge_attr"].float().to(DEV))
    if seed is not None:
        torch.manual_seed(seed)
    out = net(data)
    out.backward(t["gout"].float().to(DEV))
    torch.cuda.synchronize()
    assert float(x.grad[:, :4].abs().max()) == 0 and float(x.grad[:, 12:].abs().max()) == 0
    return net, out.detach(), {k: p.grad for k, p in net.named_parameters()}, x.grad[:, 4:12]


@pytest.mark.parametrize("name", cor.GOLDENS)
def test_reference_goldens_on_the_hip_path(pkg, name):
    t, sd, grads, keys, args = cor.load_golden(name)
    N = t["x"].size(0)
    o32, g32, dx32 = _oracle_net(sd, t, torch.float32)
    net, out, g, dx = _gpu_net(pkg, sd, t, args)
    _check(f"{name} out", out, t["out"], o32, N, False)
    for k in keys:
        _check(f"{name} grad {k}", g[k], grads[k], g32[k], N, True)
    if "dx" in t:
        _check(f"{name} dx", dx, t["dx"], dx32, N, True)
    else:
        _, _, dx64 = _oracle_net(sd, t, torch.float64)
        _check(f"{name} dx (fp64 restatement)", dx, dx64, dx32, N, True)


# ---- small shapes against the fp64 restatement ---------------------------------------------------------------------------------------
def _path():
    return 3, torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]])


def _star(out_of_hub):
    hub, leaves = torch.zeros(6, dtype=torch.int64), torch.arange(1, 7)
    return 7, (torch.stack([hub, leaves]) if out_of_hub else torch.stack([leaves, hub]))


def _random(n, e, seed):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, e), generator=g)
    ei[:, 0] = torch.tensor([n - 1, n - 1])          # a self loop
    ei[:, 1] = ei[:, 2]                              # a duplicate
    return n, ei


SHAPES = {
    # name: (graph, widths of the chain, parallel convs, K, weight sign, lambda_max)
    "one_node_no_edge": ((1, torch.zeros(2, 0, dtype=torch.int64)), [3, 4], 1, 2, 1.0, 2.0),
    "one_node_no_edge_nan": ((1, torch.zeros(2, 0, dtype=torch.int64)), [3, 4], 1, 2, 1.0, None),
    "path3": (_path(), [2, 3], 1, 3, 1.0, None),
    "star_out_hub_degree": (_star(True), [4, 4], 2, 3, 1.0, None),
    "star_out_edge": (_star(True), [4, 4], 2, 3, -1.0, None),
    "star_in_leaf_degree": (_star(False), [4, 4], 2, 2, 1.0, None),
    "star_in_edge": (_star(False), [4, 4], 2, 2, -1.0, None),
    "ragged_g8": (_random(37, 90, 1), [5, 8], 2, 3, 1.0, None),
    "ragged_g16": (_random(21, 60, 2), [9, 16], 1, 4, 1.0, None),
    "capped_g32": (_random(2100, 4000, 3), [8, 32], 2, 2, 1.0, None),
    "three_convs_widths": (_random(40, 120, 4), [5, 32, 2], 3, 3, 1.0, None),
    "one_conv_k1": (_random(19, 40, 5), [6, 7], 1, 1, 1.0, None),
    "given_lambda": (_random(33, 80, 6), [4, 6], 1, 3, 1.0, 2.5),
}


def _shape_inputs(name):
    (n, ei), widths, F, K, sign, lam = SHAPES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randn(n, widths[0], generator=g, dtype=torch.float64).float().double()
    ws = [(sign * (0.5 + torch.rand(ei.size(1), generator=g, dtype=torch.float64))).float().double() for _ in range(F)]
    sds = []
    for ci, co in zip(widths[:-1], widths[1:]):
        sd = {}
        for f in range(F):
            sd[f"convs.{f}.bias"] = ((torch.rand(co, generator=g, dtype=torch.float64) - 0.5) * 0.4).float().double()
            for k in range(K):
                sd[f"convs.{f}.lins.{k}.weight"] = ((torch.rand(co, ci, generator=g, dtype=torch.float64) - 0.5) * 0.7).float().double()
        sds.append(sd)
    gout = torch.randn(n, widths[-1], generator=g, dtype=torch.float64).float().double()
    return n, ei, x, ws, sds, gout, F, K, lam


def _shape_oracle(name, dtype):
    n, ei, x, ws, sds, gout, F, K, lam = _shape_inputs(name)
    x = x.to(dtype).requires_grad_(True)
    ws = [w.to(dtype).requires_grad_(True) for w in ws]
    refs = [{k: v.to(dtype).requires_grad_(True) for k, v in sd.items()} for sd in sds]
    h = x
    for l, sd in enumerate(refs):
        h = cor.wrapped(sd, "", h, ei, ws, lam)
        if l < len(refs) - 1:
            h = torch.relu(h)
    h.backward(gout.to(dtype))
    zero = lambda v: v.grad if v.grad is not None else torch.zeros_like(v)      # noqa: E731
    return h.detach(), [{k: zero(v) for k, v in sd.items()} for sd in refs], zero(x), [zero(w) for w in ws]


@pytest.mark.parametrize("name", list(SHAPES))
def test_small_shapes_against_the_fp64_restatement(pkg, name):
    n, ei, x, ws, sds, gout, F, K, lam = _shape_inputs(name)
    o64, g64, dx64, dw64 = _shape_oracle(name, torch.float64)
    o32, g32, dx32, dw32 = _shape_oracle(name, torch.float32)
    xg = x.float().to(DEV).requires_grad_(True)
    wg = [w.float().to(DEV).requires_grad_(True) for w in ws]
    eig = ei.to(DEV)
    mods, h = [], xg
    for l, sd in enumerate(sds):
        ci, co = sd["convs.0.lins.0.weight"].shape[1], sd["convs.0.lins.0.weight"].shape[0]
        if F == 1 and len(sds) == 1:       # the standalone conv
            m = pkg.ChebConv(ci, co, K).to(DEV)
            m.load_state_dict({k[len("convs.0."):]: v.float() for k, v in sd.items()}, strict=True)
            h = m(h, eig, wg[0], lambda_max=lam)
        else:
            assert lam is None
            m = pkg.WrappedMultiConv(F, ci, co, K).to(DEV)
            m.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
            h = m(h, [eig] * F, wg)
        if l < len(sds) - 1:
            h = torch.relu(h)
        mods.append(m)
    h.backward(gout.float().to(DEV))
    torch.cuda.synchronize()
    _check(f"{name} out", h, o64, o32, n, False)
    if bool(torch.isnan(o64).any()):
        return                             # (lambda_max = 0: the output's NaN pattern is what is pinned)
    for l, (m, sd) in enumerate(zip(mods, sds)):
        pre = "" if isinstance(m, pkg.WrappedMultiConv) else "convs.0."
        for k, p in m.named_parameters():
            _check(f"{name} layer {l} grad {k}", p.grad, g64[l][pre + k], g32[l][pre + k], n, True)
    _check(f"{name} dx", xg.grad, dx64, dx32, n, True)
    for f in range(F):
        if ei.size(1):
            _check(f"{name} d edge_weight {f}", wg[f].grad, dw64[f], dw32[f], n, True)


def test_all_zero_edge_weights_give_the_oracles_nan_pattern(pkg):
    n, ei = _random(12, 30, 8)
    x = torch.randn(n, 4, generator=torch.Generator().manual_seed(9), dtype=torch.float64).float().double()
    torch.manual_seed(1)
    m = pkg.ChebConv(4, 5, 3).to(DEV)
    sd = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    want = cor.cheb_conv(x, ei, torch.zeros(ei.size(1), dtype=torch.float64), [sd[f"lins.{k}.weight"] for k in range(3)], sd["bias"])
    got = m(x.float().to(DEV), ei.to(DEV), torch.zeros(ei.size(1), device=DEV))
    assert bool(torch.isnan(want).any())
    assert torch.equal(torch.isnan(got).cpu(), torch.isnan(want))


def test_dropout_masks_of_the_kernels_in_the_oracle_and_bitwise_reruns(pkg):
    t, sd, grads, keys, args = cor.load_golden("multiconv_h16")
    args = args[:-1] + (0.3,)
    N = t["x"].size(0)
    net, out, g, dx = _gpu_net(pkg, sd, t, args, seed=5)
    snap = net._last_snapshot
    masks = [pkg.ops.dropout_mask(snap, 0.3, l + 1, N, w.out_channels).double().cpu() for l, w in enumerate(net.convs[:-1])]
    assert all(0.2 < float((m == 0).double().mean()) < 0.4 for m in masks)
    o64, g64, dx64 = _oracle_net(sd, t, torch.float64, masks)
    o32, g32, dx32 = _oracle_net(sd, t, torch.float32, [m.float() for m in masks])
    _check("dropout out", out, o64, o32, N, False)
    for k in keys:
        _check(f"dropout grad {k}", g[k], g64[k], g32[k], N, True)
    _check("dropout dx", dx, dx64, dx32, N, True)
    net2, out2, g2, dx2 = _gpu_net(pkg, sd, t, args, seed=5)
    assert torch.equal(out, out2) and torch.equal(dx, dx2) and all(torch.equal(g[k], g2[k]) for k in keys)
    net.eval()                             # the reference's nn.Dropout lives in forward: active in eval() too
    torch.manual_seed(5)
    data = types.SimpleNamespace(x=t["x"].float().to(DEV), edge_index=t["edge_index"].to(DEV), edge_attr=t["edge_attr"].float().to(DEV))
    assert torch.equal(net(data).detach(), out)


def test_edge_attr_gradient_is_refused(pkg):
    t, sd, grads, keys, args = cor.load_golden("multiconv_h8")
    net = pkg.MultiConvNet(*args).to(DEV)
    data = types.SimpleNamespace(x=t["x"].float().to(DEV), edge_index=t["edge_index"].to(DEV),
                                 edge_attr=t["edge_attr"].float().to(DEV).requires_grad_(True))
    with pytest.raises(NotImplementedError):
        net(data)


# ---- a training step as a launch plan and as a hipGraph ------------------------------------------------------------------------------
def _step_model(pkg, name="multiconv_k3"):
    t, sd, grads, keys, args = cor.load_golden(name)
    net = pkg.MultiConvNet(*args).to(DEV)
    net.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    data = types.SimpleNamespace(x=t["x"].float().to(DEV), edge_index=t["edge_index"].to(DEV), edge_attr=t["edge_attr"].float().to(DEV))
    gout = t["gout"].float().to(DEV)
    params = list(net.parameters())

    def step(opt=None):
        for p in params:
            p.grad = None
        out = net(data)
        out.backward(gout)
        if opt is not None:
            opt.step()
        return out
    return net, params, step, args


def test_step_launch_count_is_the_documented_formula(pkg):
    """with n layers, F = 2 convs, K terms, H = max(K - 1, 1) and no dropout a step is 2 n H + 5 + ceil(n F K / 16)
    launches of the library."""
    for name in ("multiconv_k3", "multiconv_k1", "multiconv_l1"):
        net, params, step, args = _step_model(pkg, name)
        n, K = len(net.convs), args[5]
        plan = pkg.graphs.PlannedStep(step, warmup=1)
        want = 2 * n * max(K - 1, 1) + 5 + -(-n * 2 * K // 16)
        _note(f"launches {name}", plan=plan.n_launches, formula=want)
        assert plan.n_launches == want


def test_planned_and_graphed_training_steps_equal_eager_steps(pkg):
    nets = [_step_model(pkg) for _ in range(3)]
    opts = [pkg.optim.FusedAdamax(p, lr=1e-3, capturable=True) for _, p, _, _ in nets]
    (_, p_e, step_e, _), (_, p_p, step_p, _), (_, p_g, step_g, _) = nets
    start = [p.detach().clone() for p in p_e]
    for _ in range(5):
        step_e(opts[0])
    plan = pkg.graphs.PlannedStep(lambda: step_p(opts[1]), warmup=1)       # warm-up 1 + recording 1 = 2 real steps
    for _ in range(3):
        plan.replay()
    graph = pkg.graphs.GraphedStep(lambda: step_g(opts[2]), warmup=1)      # 1 warm-up, the capture runs nothing
    for _ in range(4):
        graph.replay()
    torch.cuda.synchronize()
    for a, b, c in zip(p_e, p_p, p_g):
        assert torch.equal(a, b), (a - b).abs().max().item()
        assert torch.equal(a, c), (a - c).abs().max().item()
    assert not any(torch.equal(a, b) for a, b in zip(p_e, start))          # every parameter, edge_trans included, has moved


# ---- broken argument structs ----------------------------------------------------------------------------------------------------------
class _Recorder:
    """Stands in for the loaded library: keeps a copy of the argument struct of every call of the four entry points."""

    def __init__(self, real):
        self.real, self.calls = real, {}

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not name.startswith("dss2_cheb_"):
            return fn

        def call(ref, sm):
            a = ref._obj
            self.calls.setdefault(name, []).append(type(a).from_buffer_copy(a))
            return fn(ref, sm)
        return call


def test_broken_argument_structs_are_refused_before_any_launch(pkg, monkeypatch):
    L = pkg._lib
    real = L.lib()
    rec = _Recorder(real)
    monkeypatch.setattr(L, "lib", lambda: rec)
    t, sd, grads, keys, args = cor.load_golden("multiconv_k3")
    net, out, g, dx = _gpu_net(pkg, sd, t, args)
    monkeypatch.undo()
    assert set(rec.calls) == {"dss2_cheb_edge_forward", "dss2_cheb_edge_backward", "dss2_cheb_forward", "dss2_cheb_backward"}
    buffers = [out, dx] + [g[k] for k in keys]
    before = [b.detach().clone() for b in buffers]
    sm = L.stream_ptr(torch.device(DEV))

    def setf(path, v):
        def mutate(a):
            obj = a
            for p in path[:-1]:
                obj = getattr(obj, p)
            setattr(obj, path[-1], v)
        return mutate

    breaks = {
        "dss2_cheb_forward": [setf(("group",), 7), setf(("lo", "K"), 9), setf(("g", "n_convs"), 5), setf(("hop",), 7), setf(("lo", "y"), None),
                              setf(("has_head",), 1), setf(("g", "n_nodes"), 0)],
        "dss2_cheb_backward": [setf(("group",), 12), setf(("g", "slab"), None), setf(("up", "dv"), None), setf(("g", "n_edges"), 3),
                               setf(("up", "cout"), 33)],
        "dss2_cheb_edge_forward": [setf(("g", "n_convs"), 3), setf(("n_wg",), 0), setf(("hid",), 65), setf(("W1",), None), setf(("g", "dn"), None)],
        "dss2_cheb_edge_backward": [setf(("n_wg",), 257), setf(("dw",), None), setf(("dz1",), None), setf(("g", "n_rows"), -1)],
    }
    for fn, muts in breaks.items():
        for i, mutate in enumerate(muts):
            a = type(rec.calls[fn][-1]).from_buffer_copy(rec.calls[fn][-1])
            mutate(a)
            rc = getattr(real, fn)(C.byref(a), sm)
            msg = (real.dss2_last_error() or b"").decode()
            torch.cuda.synchronize()
            _note(f"refusal {fn} #{i}", rc=rc, msg=repr(msg))
            assert rc != 0, (fn, i)
            assert fn in msg, (fn, i, msg)
            for b, w in zip(buffers, before):
                assert torch.equal(b, w), (fn, i)
