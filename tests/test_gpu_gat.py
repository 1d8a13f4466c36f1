"""GPU: GATv2Conv and GAT_DSSE (the reference driver's default model, /root/reference/networks.py:113-156 and dss2_run.py:86) on the
kernels of csrc/dss2_gat.hip, against the fp64 restatement tests/gat_oracle.py.

Outputs and the WLS loss within 1e-5 (max-normalised), parameter gradients within max(1e-4, 8 / N) (the convention of the other
parity tests), each widened to 4x the error of the same restatement run in fp32 where that is larger (see _model_parity); the
observed errors and the fp32 restatement's are printed.  Then the training-loop properties: bit-identical reruns, state_dict round trips,
the driver line's trajectory against torch's Adamax on the oracle, GraphedTrainer / EpochTrainer replays equal to the eager
steps bit for bit, and the launch counts of one step."""
import importlib
import io
import json
import os

import numpy as np
import pytest
import torch

import gat_oracle as go
from conftest import GOLDEN, PKG_NAME, golden, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REG = {"mu_v": 1e-1, "mu_theta": 1e-1, "lam_v": 1e-4, "lam_p": 1e-8, "lam_pf": 1e-6, "lam_reg": 1e2}
WORST = {}


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module(PKG_NAME)


@pytest.fixture(scope="module")
def oracle():
    import dss2_oracle
    return dss2_oracle


def _note(name, **errs):
    WORST[name] = errs
    print(f"[gat parity] {name}: " + ", ".join(f"{k} {v:.2e}" if isinstance(v, float) else f"{k} {v}" for k, v in errs.items()))


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


def _relabelled(b, seed):
    """The same batch with its nodes relabelled and its edges reordered: another summation order for every sum."""
    gen = torch.Generator().manual_seed(seed)
    n, e = b["x"].size(0), b["edge_index"].size(1)
    perm, ep = torch.randperm(n, generator=gen), torch.randperm(e, generator=gen)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(n)
    return dict(b, x=b["x"][perm], edge_index=inv[b["edge_index"]][:, ep], edge_attr=b["edge_attr"][ep])


def _oracle_run(oracle, b, sd, num_layers, nonlin, self_loops, loss, dtype, need_dx=False):
    """The restatement at `dtype` on the CPU: (output, loss value, {name: grad}, dx)."""
    x, ei, ea = b["x"].to(dtype), b["edge_index"], b["edge_attr"].to(dtype)
    ref = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    xr = x[:, :8].clone().requires_grad_(need_dx)
    out = go.gat_dsse(xr, ei, ea[:, :6], ref, num_layers, nonlin, add_self_loops=self_loops)
    o = out.detach().clone()
    if loss == "wls":
        st = tuple(s.to(dtype) for s in b["stats"])
        lv = oracle.gsp_wls_edge(input=x[:, :8], edge_input=ea[:, :6], output=out, x_mean=st[0], x_std=st[1], edge_mean=st[2],
                                 edge_std=st[3], edge_index=ei, reg_coefs=REG, num_samples=None, node_param=x[:, 8:],
                                 edge_param=ea[:, 6:])
    else:
        w = torch.linspace(-1.0, 1.0, out.numel(), dtype=dtype).view_as(out)
        lv = (out * w).sum() + 0.5 * (out ** 2).sum()
    lv.backward()
    return o, lv.item(), {k: v.grad for k, v in ref.items()}, xr.grad


def _model_parity(pkg, oracle, name, b, num_layers=8, nonlin="leaky_relu", loss="wls", self_loops=True, seed=0, need_dx=False, sd=None,
                  per_module=False):
    """GPU against the fp64 restatement.  Bounds: 1e-5 (output, loss) and max(1e-4, 8 / N) (gradients), widened to 4x the error
    of the SAME restatement run in fp32 on the CPU where that is larger: the WLS loss amplifies the output's fp32 rounding (on the
    real CIGRE batch the fp32 restatement's loss is off by ~1e-4), and lin_edge's gradient is a sum of softmax-backward terms that
    cancel per target (a near-constant attribute column), so fp32 cannot hold it to 1e-4 of its own maximum either.  With the WLS
    loss the fp32 gradient error is also taken over a relabelled copy of the batch (another summation order): on the real CIGRE
    batch a LeakyReLU gate within ~1e-6 of its kink falls either way under fp32 rounding and moves a gradient row.  (Relabelling
    keeps the loss's row order out of the output comparison: only gradients use it.)  Every effective bound is printed next to
    the error it bounds.  ``sd``: explicit weights (default: go.random_state_dict(num_layers, seed)).  ``per_module``: a gradient
    error is normalised by the largest fp64 gradient of its MODULE (the conv or Linear it belongs to) instead of its own: a
    parameter whose gradient vanishes analytically has no scale of its own (lin_r.bias where every logit of a target lies in
    LeakyReLU's linear part: the softmax is shift-invariant per target, so d x_r = 0 there, and its fp64 gradient is rounding)."""
    if sd is None:
        sd = go.random_state_dict(num_layers, seed=seed)
    mine = pkg.GAT_DSSE(8, 32, 2, num_layers, 6, nonlin=nonlin, self_loops=self_loops)
    mine.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    mine = mine.to(DEV)
    o64, l64, g64, dx64 = _oracle_run(oracle, b, sd, num_layers, nonlin, self_loops, loss, torch.float64, need_dx)
    o32, l32, g32, dx32 = _oracle_run(oracle, b, sd, num_layers, nonlin, self_loops, loss, torch.float32, need_dx)
    _, _, g32r, _ = _oracle_run(oracle, _relabelled(b, 1), sd, num_layers, nonlin, self_loops, "quad" if loss == "quad" else loss,
                                torch.float32) if loss == "wls" else (None, None, None, None)
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
        w = torch.linspace(-1.0, 1.0, out.numel(), dtype=torch.float32, device=DEV).view_as(out)
        l_g = (out * w).sum() + 0.5 * (out ** 2).sum()
    l_g.backward()
    torch.cuda.synchronize()
    N = x.size(0)
    errs = dict(out=rel_err(out_plain, o64), loss=abs(l_g.item() - l64) / abs(l64))
    fp32 = dict(out=rel_err(o32, o64), loss=abs(l32 - l64) / abs(l64))
    tol = max(1e-4, 8.0 / N)
    named = dict(mine.named_parameters())
    bounds = {"out": max(1e-5, 4 * fp32["out"]), "loss": max(1e-5, 4 * fp32["loss"])}
    worst, worst_k, ratio = 0.0, None, -1.0
    scale = {}
    for k in sd:
        mod = k.rsplit(".", 2)[0] if ".lin_" in k else k.rsplit(".", 1)[0]
        scale[mod] = max(scale.get(mod, 0.0), g64[k].abs().max().item())

    def err(a, k):
        if not per_module:
            return rel_err(a, g64[k])
        mod = k.rsplit(".", 2)[0] if ".lin_" in k else k.rsplit(".", 1)[0]
        return (a.detach().double().cpu() - g64[k]).abs().max().item() / max(scale[mod], 1e-30)
    for k in sd:
        e, e32 = err(named[k].grad, k), err(g32[k], k)
        if g32r is not None:      # (a relabelled batch has the same parameter gradients in exact arithmetic)
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
    with open(os.path.join(GOLDEN, "gat_known_answers.json")) as fh:
        z = json.load(fh)
    for name, c in z["cases"].items():
        p = c["params"]
        ed = None if p["We"] is None else len(p["We"][0])
        conv = pkg.GATv2Conv(2, 2, negative_slope=c["slope"], add_self_loops=c["add_self_loops"], edge_dim=ed)
        with torch.no_grad():
            conv.att.copy_(torch.tensor(p["att"]))
            conv.bias.copy_(torch.tensor(p["bias"]))
            conv.lin_l.weight.copy_(torch.tensor(p["Wl"]))
            conv.lin_l.bias.copy_(torch.tensor(p["bl"]))
            conv.lin_r.weight.copy_(torch.tensor(p["Wr"]))
            conv.lin_r.bias.copy_(torch.tensor(p["br"]))
            if ed:
                conv.lin_edge.weight.copy_(torch.tensor(p["We"]))
        conv = conv.to(DEV)
        x = torch.tensor(c["x"], dtype=torch.float32, device=DEV)
        ei = torch.tensor(c["edge_index"], dtype=torch.int64, device=DEV)
        ea = None if c["edge_attr"] is None else torch.tensor(c["edge_attr"], dtype=torch.float32, device=DEV)
        out = conv(x, ei, ea)
        want = torch.tensor(c["out"], dtype=torch.float64)
        assert (out.double().cpu() - want).abs().max().item() < 2e-6, (name, out, want)


@pytest.mark.parametrize("case", ["real64", "reswitched", "ober_sub", "mixed", "ober179", "tanh_L2", "relu", "L1"])
def test_gat_dsse_parity(pkg, oracle, case):
    if case == "real64":
        # the quadratic loss: under the WLS loss the lin_edge gradients of this batch are ill-conditioned in fp32 (the fp32
        # restatement is off by 2e-3 .. 9e-2 of their maximum depending on the summation order); the WLS loss on the real batch is
        # covered by tanh_L2 / L1 here and by test_driver_line_tracks_the_oracle (seed 7: no gate within 6e-6 of its kink)
        b, kw = _real_batch(), dict(seed=7, loss="quad")
    elif case == "reswitched":
        b, kw = _synthetic(pkg, ["cigre14_reswitched"], 32), {}
    elif case == "ober_sub":
        b, kw = _synthetic(pkg, ["ober_sub"], 16), {}
    elif case == "mixed":
        b, kw = _synthetic(pkg, ["cigre14", "cigre14_reswitched"], 48), {}
    elif case == "ober179":
        b, kw = _synthetic(pkg, ["ober179"], 6), {}
    elif case == "tanh_L2":
        b, kw = _real_batch(), dict(nonlin="tanh", num_layers=2)
    elif case == "relu":
        b, kw = _synthetic(pkg, ["cigre14"], 64, seed=5), dict(nonlin="relu")
    else:
        b, kw = _real_batch(), dict(num_layers=1)
    _model_parity(pkg, oracle, case, b, **kw)


GAT_GOLDENS = ["gat_real64", "gat_reswitched", "gat_ober", "gat_mixed", "gat_tanh_l2"]


@pytest.mark.parametrize("name", GAT_GOLDENS)
def test_gat_dsse_parity_reference_goldens(pkg, oracle, name):
    """The cases of tests/golden/make_gat_goldens.py (the reference's GAT_DSSE, float64) with their weights: the GPU against the
    fp64 restatement, which tests/test_gat_cpu.py holds to the reference's outputs (1e-10) and gradients."""
    g = golden(f"case_{name}.npz")
    b = {k: torch.from_numpy(np.ascontiguousarray(g[k])).float() for k in ("x", "edge_attr")}
    b["edge_index"] = torch.from_numpy(g["edge_index"])
    b["stats"] = tuple(torch.from_numpy(g[k]).float() for k in ("x_mean", "x_std", "edge_mean", "edge_std"))
    sd = {k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")}
    _model_parity(pkg, oracle, name, b, num_layers=int(g["num_layers"]), nonlin=str(g["nonlin"]), sd=sd, per_module=True)


@pytest.mark.parametrize("case", ["self_loop_and_duplicate", "component_above_192", "no_self_loops", "strided_dx"])
def test_gat_dsse_parity_structures(pkg, oracle, case):
    if case == "self_loop_and_duplicate":
        _model_parity(pkg, oracle, case, _with_self_loop_and_duplicate(_real_batch()), loss="quad")
    elif case == "component_above_192":
        _model_parity(pkg, oracle, case, _bridged(_synthetic(pkg, ["ober179"], 2), 179), loss="quad")
    elif case == "no_self_loops":      # directed CIGRE batch: bus 0 of every graph is a source only
        _model_parity(pkg, oracle, case, _with_self_loop_and_duplicate(_real_batch()), loss="quad", self_loops=False)
    else:
        _model_parity(pkg, oracle, case, _real_batch(), need_dx=True, seed=7, loss="quad")


@pytest.mark.parametrize("cin,cout,edge_dim,share,loops,bias", [(8, 8, None, False, True, True), (8, 8, 6, True, True, True),
                                                                (5, 12, 3, False, True, True), (20, 32, 16, False, False, True),
                                                                (32, 7, 6, False, True, True), (8, 8, 6, False, True, False)])
def test_standalone_gatv2conv(pkg, cin, cout, edge_dim, share, loops, bias):
    b = _real_batch()
    torch.manual_seed(cin * 100 + cout)
    N, E = b["x"].size(0), b["edge_index"].size(1)
    x64 = torch.randn(N, cin, dtype=torch.float64)
    ea64 = torch.randn(E, edge_dim, dtype=torch.float64) if edge_dim else None
    conv = pkg.GATv2Conv(cin, cout, edge_dim=edge_dim, share_weights=share, add_self_loops=loops, bias=bias)
    with torch.no_grad():
        conv.att.mul_(3.0)
        if bias:
            conv.bias.uniform_(-0.2, 0.2)
    sd = {k: v.double().clone().requires_grad_(True) for k, v in conv.state_dict().items()}
    if share:
        sd["lin_r.weight"], sd["lin_r.bias"] = sd["lin_l.weight"], sd["lin_l.bias"]
    if not bias:      # PyG: bias=False leaves lin_l, lin_r and the conv without biases
        assert not any(k.endswith("bias") for k in sd), list(sd)
    conv = conv.to(DEV)
    xr = x64.clone().requires_grad_(True)
    out_r = go.gatv2(xr, b["edge_index"], ea64, go.conv_params(sd, ""), add_self_loops=loops)
    xg = x64.float().to(DEV).requires_grad_(True)
    out = conv(xg, b["edge_index"].to(DEV), None if ea64 is None else ea64.float().to(DEV))
    w = torch.linspace(-1, 1, out_r.numel(), dtype=torch.float64).view_as(out_r)
    (out_r * w).sum().backward()
    (out * w.float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    errs = {"out": rel_err(out, out_r), "dx": rel_err(xg.grad, xr.grad)}
    tol = max(1e-4, 8.0 / N)
    for k, p in conv.named_parameters():
        errs[k] = rel_err(p.grad, sd[k].grad)
        assert errs[k] < tol, (k, errs)
    _note(f"GATv2Conv({cin},{cout},edge_dim={edge_dim},share={share},loops={loops},bias={bias}) (bounds: out 1e-5, rest {tol:.1e})", **errs)
    assert errs["out"] < 1e-5 and errs["dx"] < tol, errs


def test_edge_attr_grad_raises_and_cpu_raises(pkg):
    b = _real_batch()
    m = pkg.GAT_DSSE(8, 32, 2, 3, 6).to(DEV)
    x, ei, ea = b["x"].to(DEV), b["edge_index"].to(DEV), b["edge_attr"].to(DEV)
    with pytest.raises(NotImplementedError):
        m(x[:, :8], ei, ea[:, :6].clone().requires_grad_(True))
    with pytest.raises(RuntimeError):
        pkg.GAT_DSSE(8, 32, 2, 3, 6)(b["x"][:, :8], b["edge_index"], b["edge_attr"][:, :6])


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
    sd = go.random_state_dict(8, seed=2)
    m = pkg.GAT_DSSE(8, 32, 2, 8, 6)
    m.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    m = m.to(DEV)
    o1, l1, g1 = _step(pkg, m, dev_b, st)
    o2, l2, g2 = _step(pkg, m, dev_b, st)
    assert torch.equal(o1, o2) and torch.equal(l1, l2) and all(torch.equal(a, c) for a, c in zip(g1, g2))
    buf = io.BytesIO()
    torch.save(m.state_dict(), buf)
    buf.seek(0)
    m2 = pkg.GAT_DSSE(8, 32, 2, 8, 6).to(DEV)
    m2.load_state_dict(torch.load(buf), strict=True)
    o3, l3, _ = _step(pkg, m2, dev_b, st)
    assert torch.equal(o1, o3) and torch.equal(l1, l3)


def test_driver_line_tracks_the_oracle(pkg, oracle):
    """runner.build_model("GAT_DSSE", HYPER) + FusedAdamax over five eager steps on the real CIGRE batch against the fp64 oracle
    with torch's Adamax from the same weights: the loss trajectories agree and the loss goes down."""
    b = _real_batch()
    torch.manual_seed(0)
    mine = pkg.runner.build_model("GAT_DSSE", pkg.runner.HYPER)
    assert isinstance(mine, pkg.GAT_DSSE) and mine.num_layers == 8 and mine.dim_dense == 32 and mine.edge_dim == 6
    sd = {k: v.double().clone() for k, v in mine.state_dict().items()}
    mine = mine.to(DEV)
    # the bound: 1e-3, or 8x the first-step loss error of the restatement in fp32: the WLS loss amplifies fp32 output rounding
    # (~1e-4 on this batch at step 0) and the default weights have gates within 1e-6 of their kinks, so the first updates differ
    _, l32, _, _ = _oracle_run(oracle, b, sd, 8, "leaky_relu", True, "wls", torch.float32)
    ref = {k: v.requires_grad_(True) for k, v in sd.items()}
    o_ref = torch.optim.Adamax(list(ref.values()), lr=3e-3)
    o_gpu = pkg.FusedAdamax(mine.parameters(), lr=3e-3)
    dev_b = {"x": b["x"].to(DEV), "edge_index": b["edge_index"].to(DEV), "edge_attr": b["edge_attr"].to(DEV), "num_graphs": 64}
    st = tuple(s.to(DEV) for s in b["stats"])
    x64, ea64, ei = b["x"].double(), b["edge_attr"].double(), b["edge_index"]
    st64 = tuple(s.double() for s in b["stats"])
    l_ref, l_gpu = [], []
    for _ in range(5):
        o_ref.zero_grad()
        out = go.gat_dsse(x64[:, :8], ei, ea64[:, :6], ref, 8)
        lr_ = oracle.gsp_wls_edge(input=x64[:, :8], edge_input=ea64[:, :6], output=out, x_mean=st64[0], x_std=st64[1],
                                  edge_mean=st64[2], edge_std=st64[3], edge_index=ei, reg_coefs=REG, num_samples=None,
                                  node_param=x64[:, 8:], edge_param=ea64[:, 6:])
        lr_.backward()
        o_ref.step()
        l_ref.append(lr_.item())
        l_gpu.append(pkg.runner.train_epoch(mine, o_gpu, [dev_b], st, pkg.runner.REG_COEFS))
    rtol = max(1e-3, 8 * abs(l32 - l_ref[0]) / abs(l_ref[0]))
    print("[gat driver line] gpu", l_gpu, "oracle", l_ref, "rtol", rtol)
    assert l_gpu[-1] < l_gpu[0]
    for a, c in zip(l_gpu, l_ref):
        assert abs(a - c) <= rtol * abs(c), (l_gpu, l_ref, rtol)


def test_graphed_replay_equals_the_eager_step(pkg):
    b = _real_batch()
    x, ei, ea = b["x"].to(DEV), b["edge_index"].to(DEV), b["edge_attr"].to(DEV)
    st = tuple(s.to(DEV) for s in b["stats"])
    torch.manual_seed(1)
    m1 = pkg.runner.build_model("GAT_DSSE", pkg.runner.HYPER).to(DEV)
    m2 = pkg.runner.build_model("GAT_DSSE", pkg.runner.HYPER).to(DEV)
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
    assert np.allclose(got, want, rtol=1e-6, atol=0), (got, want)


@pytest.mark.parametrize("mode", ["plan", "graph"])
def test_an_epoch_of_replays_equals_the_eager_epoch(pkg, mode):
    full = pkg.synthetic.make_batch(["cigre14"], 150, seed=4, violate=0.2)
    ds = pkg.dataset.DeviceDataset.from_batch(full, device=DEV)
    stats = tuple(s.to(DEV) for s in full["stats"])
    torch.manual_seed(1)
    m1 = pkg.runner.build_model("GAT_DSSE", pkg.runner.HYPER).to(DEV)
    m2 = pkg.runner.build_model("GAT_DSSE", pkg.runner.HYPER).to(DEV)
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
    """Forward <= 7 launches (one per conv, head fused into the last), backward <= 2 * 7 + 2, counted from launch plans."""
    import ctypes as C
    L = pkg._lib
    b = _real_batch()
    x, ei, ea = b["x"].to(DEV), b["edge_index"].to(DEV), b["edge_attr"].to(DEV)
    m = pkg.runner.build_model("GAT_DSSE", pkg.runner.HYPER).to(DEV)
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
    print(f"[gat launches] forward {n_fwd}, backward {n_bwd}")
    assert n_fwd <= 7 and n_bwd <= 2 * 7 + 2, (n_fwd, n_bwd)
