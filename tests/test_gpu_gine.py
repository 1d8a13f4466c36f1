"""GPU: GINEConv and GINE_DSSE (the reference's GIN model, /root/reference/networks.py:71-111) on the kernels of
csrc/dss2_gine.hip, against the fp64 restatement tests/gine_oracle.py.

Outputs and the WLS loss within 1e-5 (max-normalised), parameter gradients within max(1e-4, 8 / N) (the convention of the other
parity tests), each widened to 4x the error of the same restatement run in fp32 where that is larger (see _model_parity); every
bound is printed next to its error.  Gradients are compared over named_parameters(): the shared nn Linear appears once there and
once per conv in the state_dict.  Then structures (self loops, duplicates, a large component, a hub target, no edges, strided
inputs), the standalone layer, NaN inputs, bit-identical reruns, state_dict round trips, the driver line's trajectory against
torch's Adamax on the oracle, GraphedTrainer / EpochTrainer replays equal to the eager steps bit for bit, and launch counts."""
import ctypes as C
import importlib
import io
import json
import os

import numpy as np
import pytest
import torch

import gine_oracle as go
from conftest import GOLDEN, PKG_NAME, golden, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REG = {"mu_v": 1e-1, "mu_theta": 1e-1, "lam_v": 1e-4, "lam_p": 1e-8, "lam_pf": 1e-6, "lam_reg": 1e2}


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module(PKG_NAME)


@pytest.fixture(scope="module")
def oracle():
    import dss2_oracle
    return dss2_oracle


def _note(name, **errs):
    print(f"[gine parity] {name}: " + ", ".join(f"{k} {v:.2e}" if isinstance(v, float) else f"{k} {v}" for k, v in errs.items()))


def _real_batch():
    g = golden("cigre14_real64.npz")
    b = {k: torch.from_numpy(np.ascontiguousarray(g[k])) for k in ("x", "edge_index", "edge_attr")}
    b["stats"] = tuple(torch.from_numpy(g[k]) for k in ("x_mean", "x_std", "edge_mean", "edge_std"))
    return b


def _synthetic(pkg, grids, B, seed=3):
    return pkg.synthetic.make_batch(grids, B, seed=seed)


def _with_self_loop_and_duplicate(b):
    """The batch plus a self loop on node 3 and a second copy of edge 5 (same attributes)."""
    ei, ea = b["edge_index"], b["edge_attr"]
    ei2 = torch.cat([ei, torch.tensor([[3], [3]]), ei[:, 5:6]], 1)
    ea2 = torch.cat([ea, ea[7:8] * 1.5, ea[5:6]], 0)
    return dict(b, edge_index=ei2, edge_attr=ea2)


def _bridged(b, nodes_per_graph):
    """Two graphs joined by one extra edge: a connected component of 2 * nodes_per_graph nodes."""
    ei, ea = b["edge_index"], b["edge_attr"]
    ei2 = torch.cat([ei, torch.tensor([[nodes_per_graph - 1], [nodes_per_graph]])], 1)
    ea2 = torch.cat([ea, ea[:1]], 0)
    return dict(b, edge_index=ei2, edge_attr=ea2)


def _hub(b, n_in=320):
    """The batch plus n_in edges from distinct nodes into node 5 (attributes copied from the first edges, scaled down)."""
    ei, ea = b["edge_index"], b["edge_attr"]
    src = torch.arange(100, 100 + n_in)
    ei2 = torch.cat([ei, torch.stack([src, torch.full_like(src, 5)])], 1)
    ea2 = torch.cat([ea, ea[:n_in] * 0.25], 0)
    return dict(b, edge_index=ei2, edge_attr=ea2)


def _no_edges(b):
    return dict(b, edge_index=torch.zeros(2, 0, dtype=torch.int64), edge_attr=b["edge_attr"][:0])


def _relabelled(b, seed):
    """The same batch with its nodes relabelled and its edges reordered: another summation order for every sum."""
    gen = torch.Generator().manual_seed(seed)
    n, e = b["x"].size(0), b["edge_index"].size(1)
    perm, ep = torch.randperm(n, generator=gen), torch.randperm(e, generator=gen)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(n)
    return dict(b, x=b["x"][perm], edge_index=inv[b["edge_index"]][:, ep], edge_attr=b["edge_attr"][ep])


def _quad(out):
    w = torch.linspace(-1.0, 1.0, out.numel(), dtype=out.dtype, device=out.device).view_as(out)
    return (out * w).sum() + 0.5 * (out ** 2).sum()


def _oracle_run(oracle, b, sd, num_layers, nonlin, loss, dtype, need_dx=False):
    """The restatement at `dtype` on the CPU: (output, loss value, {name: grad}, dx).  The shared nn enters once."""
    x, ei, ea = b["x"].to(dtype), b["edge_index"], b["edge_attr"].to(dtype)
    ref = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in go.unique_params(sd).items()}
    xr = x[:, :8].clone().requires_grad_(need_dx)
    out = go.gine_dsse(xr, ei, ea[:, :6], ref, num_layers, nonlin)
    o = out.detach().clone()
    if loss == "wls":
        st = tuple(s.to(dtype) for s in b["stats"])
        lv = oracle.gsp_wls_edge(input=x[:, :8], edge_input=ea[:, :6], output=out, x_mean=st[0], x_std=st[1], edge_mean=st[2],
                                 edge_std=st[3], edge_index=ei, reg_coefs=REG, num_samples=None, node_param=x[:, 8:],
                                 edge_param=ea[:, 6:])
    else:
        lv = _quad(out)
    lv.backward()
    return o, lv.item(), {k: v.grad for k, v in ref.items()}, xr.grad


def _model_parity(pkg, oracle, name, b, num_layers=8, nonlin="leaky_relu", loss="wls", seed=0, need_dx=False, sd=None, eps=0.0,
                  train_eps=False, per_module=False):
    """GPU against the fp64 restatement.  Bounds: 1e-5 (output, loss) and max(1e-4, 8 / N) (gradients), widened to 4x the error
    of the SAME restatement run in fp32 on the CPU where that is larger (the WLS loss amplifies the output's fp32 rounding; a
    message ReLU gate within rounding of 0 falls either way in fp32 and moves a weight-gradient row).  With the WLS loss the fp32
    gradient error is also taken over a relabelled copy of the batch (another summation order).  ``per_module``: a gradient error
    is normalised by the largest fp64 gradient of its module instead of its own (for a parameter whose gradient nearly cancels)."""
    if sd is None:
        sd = go.random_state_dict(num_layers, eps=eps, seed=seed)
    mine = pkg.GINE_DSSE(8, 32, 2, num_layers, 6, nonlin=nonlin, eps=eps, train_eps=train_eps)
    mine.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    mine = mine.to(DEV)
    o64, l64, g64, dx64 = _oracle_run(oracle, b, sd, num_layers, nonlin, loss, torch.float64, need_dx)
    o32, l32, g32, dx32 = _oracle_run(oracle, b, sd, num_layers, nonlin, loss, torch.float32, need_dx)
    g32r = _oracle_run(oracle, _relabelled(b, 1), sd, num_layers, nonlin, loss, torch.float32)[2] if loss == "wls" else None
    x, eid, ea = b["x"].to(DEV), b["edge_index"].to(DEV), b["edge_attr"].to(DEV)
    xin = x[:, :8]
    if need_dx:
        xin = xin.detach().clone().requires_grad_(True)
    out = mine(xin, eid, ea[:, :6])
    out_plain = out.detach().clone()
    if loss == "wls":
        st = tuple(s.to(DEV) for s in b["stats"])
        l_g = pkg.gsp_wls_edge(input=x[:, :8], edge_input=ea[:, :6], output=out, x_mean=st[0], x_std=st[1], edge_mean=st[2],
                               edge_std=st[3], edge_index=eid, reg_coefs=REG, num_samples=None, node_param=x[:, 8:],
                               edge_param=ea[:, 6:])
    else:
        l_g = _quad(out)
    l_g.backward()
    torch.cuda.synchronize()
    N = x.size(0)
    errs = dict(out=rel_err(out_plain, o64), loss=abs(l_g.item() - l64) / abs(l64))
    fp32 = dict(out=rel_err(o32, o64), loss=abs(l32 - l64) / abs(l64))
    tol = max(1e-4, 8.0 / N)
    bounds = {"out": max(1e-5, 4 * fp32["out"]), "loss": max(1e-5, 4 * fp32["loss"])}
    named = dict(mine.named_parameters())
    assert list(named) == go.parameter_names(num_layers, train_eps), list(named)
    if num_layers == 1:     # no conv: the shared nn exists and gets no gradient, as in the reference
        assert named.pop("nn.weight").grad is None and named.pop("nn.bias").grad is None
    scale = {}
    for k in named:
        mod = k.rsplit(".", 1)[0]
        scale[mod] = max(scale.get(mod, 0.0), g64[k].abs().max().item())

    def err(a, k):
        if not per_module:
            return rel_err(a, g64[k])
        return (a.detach().double().cpu() - g64[k]).abs().max().item() / max(scale[k.rsplit(".", 1)[0]], 1e-30)
    worst, worst_k, ratio = 0.0, None, -1.0
    for k, p in named.items():
        e, e32 = err(p.grad, k), err(g32[k], k)
        if g32r is not None:
            e32 = max(e32, err(g32r[k], k))
        bound = max(tol, 4 * e32)
        assert e < bound, (name, k, e, bound)
        if e / bound > ratio:     # the gradient closest to its bound
            worst, worst_k, ratio, bounds["grad"] = e, k, e / bound, bound
    errs["grad"] = worst
    if need_dx:
        errs["dx"], bounds["dx"] = rel_err(xin.grad, dx64), max(tol, 4 * rel_err(dx32, dx64))
        assert errs["dx"] < bounds["dx"], (errs, bounds)
    _note(name, **{f"{k} (bound)": f"{v:.2e} ({bounds[k]:.2e})" for k, v in errs.items()}, grad_param=worst_k)
    assert errs["out"] < bounds["out"] and errs["loss"] < bounds["loss"], (name, errs, bounds)
    return mine


def test_known_answers(pkg):
    with open(os.path.join(GOLDEN, "gine_known_answers.json")) as fh:
        z = json.load(fh)
    for name, c in z["cases"].items():
        if "model" in c:
            m = pkg.GINE_DSSE(**c["model"])
            sd = {k: torch.tensor(v, dtype=torch.float32) for k, v in c["state_dict"].items()}
        else:
            p = c["params"]
            lin_w = p.get("lin.weight")
            nnl = torch.nn.Linear(len(p["nn.weight"][0]), len(p["nn.weight"]))
            m = pkg.GINEConv(nnl, eps=p["eps"][0], edge_dim=None if lin_w is None else len(lin_w[0]))
            sd = {k: torch.tensor(v, dtype=torch.float32) for k, v in p.items()}
        m.load_state_dict(sd, strict=True)
        m = m.to(DEV)
        x = torch.tensor(c["x"], dtype=torch.float32, device=DEV)
        ei = torch.tensor(c["edge_index"], dtype=torch.int64, device=DEV).view(2, -1)
        ea = torch.tensor(c["edge_attr"], dtype=torch.float32, device=DEV).view(ei.size(1), -1)
        out = m(x, ei, ea)
        want = torch.tensor(c["out"], dtype=torch.float64)
        assert (out.detach().double().cpu() - want).abs().max().item() < 2e-6, (name, out, want)


@pytest.mark.parametrize("case", ["real64", "reswitched", "ober_sub", "mixed", "ober179", "tanh_L2", "relu", "L1", "train_eps",
                                  "dx"])
def test_gine_dsse_parity(pkg, oracle, case):
    kw = {}
    if case == "real64":
        b = _real_batch()
    elif case == "reswitched":
        b = _synthetic(pkg, ["cigre14_reswitched"], 32)
    elif case == "ober_sub":
        b = _synthetic(pkg, ["ober_sub"], 16)
    elif case == "mixed":
        b = _synthetic(pkg, ["cigre14", "cigre14_reswitched"], 48)
    elif case == "ober179":
        b = _synthetic(pkg, ["ober179"], 6)
    elif case == "tanh_L2":
        b, kw = _real_batch(), dict(nonlin="tanh", num_layers=2)
    elif case == "relu":
        b, kw = _synthetic(pkg, ["cigre14"], 64, seed=5), dict(nonlin="relu")
    elif case == "L1":
        b, kw = _real_batch(), dict(num_layers=1)
    elif case == "train_eps":
        b, kw = _synthetic(pkg, ["cigre14"], 64, seed=6), dict(train_eps=True, eps=0.3, num_layers=4)
    else:
        b, kw = _real_batch(), dict(need_dx=True, loss="quad", seed=7)
    _model_parity(pkg, oracle, case, b, **kw)


GINE_GOLDENS = ["gine_real64", "gine_reswitched", "gine_ober", "gine_mixed", "gine_train_eps_l2"]


@pytest.mark.parametrize("name", GINE_GOLDENS)
def test_gine_dsse_parity_reference_goldens(pkg, oracle, name):
    """The cases of tests/golden/make_gine_goldens.py (the reference's GINE_DSSE, float64) with their weights: the GPU against the
    fp64 restatement, which tests/test_gine_cpu.py holds to the reference's outputs and gradients."""
    g = golden(f"case_{name}.npz")
    b = {k: torch.from_numpy(np.ascontiguousarray(g[k])).float() for k in ("x", "edge_attr")}
    b["edge_index"] = torch.from_numpy(g["edge_index"])
    b["stats"] = tuple(torch.from_numpy(g[k]).float() for k in ("x_mean", "x_std", "edge_mean", "edge_std"))
    sd = {k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")}
    _model_parity(pkg, oracle, name, b, num_layers=int(g["num_layers"]), eps=float(g["eps"]), train_eps=bool(g["train_eps"]), sd=sd,
                  per_module=True)


@pytest.mark.parametrize("case", ["self_loop_and_duplicate", "component_above_192", "hub_above_300", "no_edges"])
def test_gine_dsse_parity_structures(pkg, oracle, case):
    if case == "self_loop_and_duplicate":
        _model_parity(pkg, oracle, case, _with_self_loop_and_duplicate(_real_batch()), loss="quad", need_dx=True)
    elif case == "component_above_192":
        _model_parity(pkg, oracle, case, _bridged(_synthetic(pkg, ["ober179"], 2), 179), loss="quad")
    elif case == "hub_above_300":
        _model_parity(pkg, oracle, case, _hub(_real_batch()), loss="quad", need_dx=True)
    else:
        _model_parity(pkg, oracle, case, _no_edges(_real_batch()), loss="quad", need_dx=True, eps=0.2, train_eps=True)


def test_strided_column_slices_equal_contiguous_inputs(pkg):
    b = _real_batch()
    x, ei, ea = b["x"].to(DEV), b["edge_index"].to(DEV), b["edge_attr"].to(DEV)
    assert x.stride(0) > 8 and ea.stride(0) > 6
    torch.manual_seed(3)
    m = pkg.GINE_DSSE(8, 32, 2, 4, 6).to(DEV)
    o1 = m(x[:, :8], ei, ea[:, :6])
    _quad(o1).backward()
    g1 = [p.grad.clone() for p in m.parameters()]
    m.zero_grad()
    o2 = m(x[:, :8].contiguous(), ei, ea[:, :6].contiguous())
    _quad(o2).backward()
    assert torch.equal(o1, o2) and all(torch.equal(a, p.grad) for a, p in zip(g1, m.parameters()))


@pytest.mark.parametrize("cin,cout,edge_dim,eps", [(8, 8, 6, 0.0), (8, 8, None, 0.5), (5, 12, 3, -0.25), (20, 32, 16, 0.1),
                                                   (32, 7, None, 0.0)])
def test_standalone_gineconv(pkg, cin, cout, edge_dim, eps):
    b = _real_batch()
    torch.manual_seed(cin * 100 + cout)
    N, E = b["x"].size(0), b["edge_index"].size(1)
    x64 = torch.randn(N, cin, dtype=torch.float64)
    ea64 = torch.randn(E, edge_dim if edge_dim else cin, dtype=torch.float64)
    conv = pkg.GINEConv(torch.nn.Linear(cin, cout), eps=eps, train_eps=True, edge_dim=edge_dim)
    keys = ["eps", "nn.weight", "nn.bias"] + (["lin.weight", "lin.bias"] if edge_dim else [])
    assert list(conv.state_dict()) == keys
    sd = {k: v.double().clone().requires_grad_(True) for k, v in conv.state_dict().items()}
    conv = conv.to(DEV)
    xr = x64.clone().requires_grad_(True)
    out_r = go.gine(xr, b["edge_index"], ea64, sd["nn.weight"], sd["nn.bias"], sd["eps"], sd.get("lin.weight"), sd.get("lin.bias"))
    xg = x64.float().to(DEV).requires_grad_(True)
    out = conv(xg, b["edge_index"].to(DEV), ea64.float().to(DEV))
    assert out.shape == (N, cout)
    w = torch.linspace(-1, 1, out_r.numel(), dtype=torch.float64).view_as(out_r)
    (out_r * w).sum().backward()
    (out * w.float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    errs = {"out": rel_err(out, out_r), "dx": rel_err(xg.grad, xr.grad)}
    tol = max(1e-4, 8.0 / N)
    for k, p in conv.named_parameters():
        errs[k] = rel_err(p.grad, sd[k].grad)
        assert errs[k] < tol, (k, errs)
    _note(f"GINEConv({cin},{cout},edge_dim={edge_dim},eps={eps}) (bounds: out 1e-5, rest {tol:.1e})", **errs)
    assert errs["out"] < 1e-5 and errs["dx"] < tol, errs


def test_nan_input_stays_in_its_graph(pkg):
    b = _real_batch()
    x = b["x"].clone()
    x[3 * 14 + 2, 1] = float("nan")          # graph 3, bus 2
    sd = go.random_state_dict(8, seed=4)
    want = go.gine_dsse(x[:, :8].double(), b["edge_index"], b["edge_attr"][:, :6].double(), sd, 8)
    m = pkg.GINE_DSSE(8, 32, 2, 8, 6)
    m.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    m = m.to(DEV)
    with torch.no_grad():
        out = m(x.to(DEV)[:, :8], b["edge_index"].to(DEV), b["edge_attr"].to(DEV)[:, :6]).double().cpu()
    nan_w, nan_g = torch.isnan(want), torch.isnan(out)
    assert nan_w.any() and torch.equal(nan_w, nan_g), (nan_w.nonzero(), nan_g.nonzero())
    assert torch.isfinite(out[~nan_g]).all()
    assert (out[~nan_g] - want[~nan_w]).abs().max().item() < 1e-5 * want[~nan_w].abs().max().item()


def test_edge_attr_grad_raises_and_cpu_raises(pkg):
    b = _real_batch()
    m = pkg.GINE_DSSE(8, 32, 2, 3, 6).to(DEV)
    x, ei, ea = b["x"].to(DEV), b["edge_index"].to(DEV), b["edge_attr"].to(DEV)
    with pytest.raises(NotImplementedError):
        m(x[:, :8], ei, ea[:, :6].clone().requires_grad_(True))
    with pytest.raises(ValueError, match="edge_attr"):
        m(x[:, :8], ei, ea[:, :5])
    with pytest.raises(RuntimeError):
        pkg.GINE_DSSE(8, 32, 2, 3, 6)(b["x"][:, :8], b["edge_index"], b["edge_attr"][:, :6])


def _step(pkg, m, b, st):
    for p in m.parameters():
        p.grad = None
    x, ei, ea = b
    out = m(x[:, :8], ei, ea[:, :6])
    loss = pkg.gsp_wls_edge(input=x[:, :8], edge_input=ea[:, :6], output=out, x_mean=st[0], x_std=st[1], edge_mean=st[2],
                            edge_std=st[3], edge_index=ei, reg_coefs=REG, num_samples=None, node_param=x[:, 8:], edge_param=ea[:, 6:])
    loss.backward()
    return out.detach().clone(), loss.detach().clone(), [p.grad.clone() for p in m.parameters()]


def test_two_runs_are_bit_identical_and_state_dict_round_trips(pkg):
    b = _real_batch()
    dev_b = (b["x"].to(DEV), b["edge_index"].to(DEV), b["edge_attr"].to(DEV))
    st = tuple(s.to(DEV) for s in b["stats"])
    sd = go.random_state_dict(8, eps=0.1, seed=2)
    m = pkg.GINE_DSSE(8, 32, 2, 8, 6, train_eps=True)
    m.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    m = m.to(DEV)
    o1, l1, g1 = _step(pkg, m, dev_b, st)
    o2, l2, g2 = _step(pkg, m, dev_b, st)
    assert torch.equal(o1, o2) and torch.equal(l1, l2) and all(torch.equal(a, c) for a, c in zip(g1, g2))
    buf = io.BytesIO()
    torch.save(m.state_dict(), buf)
    buf.seek(0)
    m2 = pkg.GINE_DSSE(8, 32, 2, 8, 6, train_eps=True).to(DEV)
    m2.load_state_dict(torch.load(buf), strict=True)
    assert m2.nn is m2.model.module_0.nn is m2.model.module_12.nn
    o3, l3, g3 = _step(pkg, m2, dev_b, st)
    assert torch.equal(o1, o3) and torch.equal(l1, l3) and all(torch.equal(a, c) for a, c in zip(g1, g3))


def test_driver_line_tracks_the_oracle(pkg, oracle):
    """runner.build_model("GINE_DSSE", HYPER) + FusedAdamax over five eager steps on the real CIGRE batch against the fp64 oracle
    with torch's Adamax from the same weights: the loss trajectories agree and the loss goes down."""
    b = _real_batch()
    torch.manual_seed(0)
    mine = pkg.runner.build_model("GINE_DSSE", pkg.runner.HYPER)
    assert isinstance(mine, pkg.GINE_DSSE) and mine.num_layers == 8 and mine.dim_dense == 32 and mine.edge_dim == 6
    sd = {k: v.double().clone() for k, v in mine.state_dict().items()}
    mine = mine.to(DEV)
    _, l32, _, _ = _oracle_run(oracle, b, sd, 8, "leaky_relu", "wls", torch.float32)
    ref = {k: v.requires_grad_(True) for k, v in go.unique_params(sd).items()}
    o_ref = torch.optim.Adamax([ref[k] for k in go.parameter_names(8)], lr=3e-3)
    o_gpu = pkg.FusedAdamax(mine.parameters(), lr=3e-3)
    dev_b = {"x": b["x"].to(DEV), "edge_index": b["edge_index"].to(DEV), "edge_attr": b["edge_attr"].to(DEV), "num_graphs": 64}
    st = tuple(s.to(DEV) for s in b["stats"])
    x64, ea64, ei = b["x"].double(), b["edge_attr"].double(), b["edge_index"]
    st64 = tuple(s.double() for s in b["stats"])
    l_ref, l_gpu = [], []
    for _ in range(5):
        o_ref.zero_grad()
        out = go.gine_dsse(x64[:, :8], ei, ea64[:, :6], ref, 8)
        lr_ = oracle.gsp_wls_edge(input=x64[:, :8], edge_input=ea64[:, :6], output=out, x_mean=st64[0], x_std=st64[1],
                                  edge_mean=st64[2], edge_std=st64[3], edge_index=ei, reg_coefs=REG, num_samples=None,
                                  node_param=x64[:, 8:], edge_param=ea64[:, 6:])
        lr_.backward()
        o_ref.step()
        l_ref.append(lr_.item())
        l_gpu.append(pkg.runner.train_epoch(mine, o_gpu, [dev_b], st, pkg.runner.REG_COEFS))
    rtol = max(1e-3, 8 * abs(l32 - l_ref[0]) / abs(l_ref[0]))
    print("[gine driver line] gpu", l_gpu, "oracle", l_ref, "rtol", rtol)
    assert l_gpu[-1] < l_gpu[0]
    for a, c in zip(l_gpu, l_ref):
        assert abs(a - c) <= rtol * abs(c), (l_gpu, l_ref, rtol)


@pytest.mark.parametrize("train_eps", [False, True])
def test_graphed_replay_equals_the_eager_step(pkg, train_eps):
    """With train_eps the replays see the eps the optimizer just wrote: the kernels read it from device memory."""
    b = _real_batch()
    x, ei, ea = b["x"].to(DEV), b["edge_index"].to(DEV), b["edge_attr"].to(DEV)
    st = tuple(s.to(DEV) for s in b["stats"])
    torch.manual_seed(1)
    m1 = pkg.GINE_DSSE(8, 32, 2, 8, 6, eps=0.1, train_eps=train_eps).to(DEV)
    m2 = pkg.GINE_DSSE(8, 32, 2, 8, 6, eps=0.1, train_eps=train_eps).to(DEV)
    m2.load_state_dict(m1.state_dict())
    o1 = pkg.FusedAdamax(m1.parameters(), lr=3e-3, capturable=True)
    o2 = pkg.FusedAdamax(m2.parameters(), lr=3e-3, capturable=True)
    tr = pkg.runner.GraphedTrainer(m2, o2, st, REG)
    batch = {"x": x, "edge_index": ei, "edge_attr": ea, "num_graphs": 64}
    want = [pkg.runner.train_epoch(m1, o1, [batch], st, REG) for _ in range(3)]
    got = [float(tr.step(x, ei, ea)) for _ in range(3)]      # the first is the capture's warm-up step, then two replays
    torch.cuda.synchronize()
    for a, c in zip(m1.parameters(), m2.parameters()):
        assert torch.equal(a, c), (a - c).abs().max().item()
    if train_eps:
        assert m2.model.module_0.eps.item() != 0.1
    assert np.allclose(got, want, rtol=1e-6, atol=0), (got, want)


@pytest.mark.parametrize("mode", ["plan", "graph"])
def test_an_epoch_of_replays_equals_the_eager_epoch(pkg, mode):
    full = pkg.synthetic.make_batch(["cigre14"], 150, seed=4, violate=0.2)
    ds = pkg.dataset.DeviceDataset.from_batch(full, device=DEV)
    stats = tuple(s.to(DEV) for s in full["stats"])
    torch.manual_seed(1)
    m1 = pkg.runner.build_model("GINE_DSSE", pkg.runner.HYPER).to(DEV)
    m2 = pkg.runner.build_model("GINE_DSSE", pkg.runner.HYPER).to(DEV)
    m2.load_state_dict(m1.state_dict())
    o1 = pkg.optim.FusedAdamax(m1.parameters(), lr=3e-3, capturable=True)
    o2 = pkg.optim.FusedAdamax(m2.parameters(), lr=3e-3, capturable=True)
    tr = pkg.runner.EpochTrainer(m2, o2, stats, REG, ds, 64, shuffle=False, mode=mode)
    want = []
    for _ in range(2):
        loader = pkg.dataset.DataLoader(ds, batch_size=64, shuffle=False)
        want.append(pkg.runner.train_epoch(m1, o1, loader, stats, REG))
    got = []
    for _ in range(2):
        tr.train_epoch()
        got.append(tr.mean_loss())
    torch.cuda.synchronize()
    for a, c in zip(m1.parameters(), m2.parameters()):
        assert torch.equal(a, c), (a - c).abs().max().item()
    assert np.allclose(got, want, rtol=1e-6, atol=0), (got, want)


def test_launch_counts_of_the_driver_line(pkg):
    """Forward <= 7 launches (one per conv, head fused into the last), backward <= 10 (7 fused conv launches, the head's launch
    folded into the first, the head's weight gradients, the reduction), counted from launch plans."""
    L = pkg._lib
    b = _real_batch()
    x, ei, ea = b["x"].to(DEV), b["edge_index"].to(DEV), b["edge_attr"].to(DEV)
    m = pkg.runner.build_model("GINE_DSSE", pkg.runner.HYPER).to(DEV)
    out = m(x[:, :8], ei, ea[:, :6])         # warm: topology cached
    g = torch.ones_like(out)
    out.backward(g)
    torch.cuda.synchronize()

    def count(fn):
        h = C.c_void_p()
        L.check(L.lib().dss2_plan_begin(C.byref(h)), "plan_begin")
        try:
            r = fn()
        finally:
            L.check(L.lib().dss2_plan_end(h), "plan_end")
        n = int(L.lib().dss2_plan_size(h))
        L.lib().dss2_plan_destroy(h)
        return n, r
    n_fwd, out = count(lambda: m(x[:, :8], ei, ea[:, :6]))
    n_bwd, _ = count(lambda: out.backward(g))
    torch.cuda.synchronize()
    print(f"[gine launches] forward {n_fwd}, backward {n_bwd}")
    assert n_fwd <= 7 and n_bwd <= 10, (n_fwd, n_bwd)
