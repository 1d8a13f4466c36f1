"""GPU: gnn_dsse (the reference's networks.py:11-69) with GCN2Conv, FAConv and TAGConv on the kernels of csrc/dss2_gnn.hip,
against the reference's own model (tests/golden/case_gnn_*.npz) and the fp64 restatement tests/gnn_oracle.py.

Outputs and the WLS loss within 1e-5 (max-normalised), parameter and input gradients within max(1e-4, 8 / N), each widened to
4x the error of the same restatement run in fp32 where that is larger (the convention of test_gpu_gine.py); every bound is
printed next to its error.  Then node ids outside the batch, structures (a self loop with duplicates, a component above 192 buses, a hub above 300 in-edges,
no edges), the standalone convs, the cached structure, NaN inputs, bit-identical reruns, state_dict round trips, the driver
line's trajectory against torch's Adamax on the oracle, GraphedTrainer / EpochTrainer replays equal to the eager steps bit for
bit, and launch counts."""
import ctypes as C
import importlib
import io

import numpy as np
import pytest
import torch

import gnn_oracle as gor
from conftest import PKG_NAME, golden, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REG = {"mu_v": 1e-1, "mu_theta": 1e-1, "lam_v": 1e-4, "lam_p": 1e-8, "lam_pf": 1e-6, "lam_reg": 1e2}
KINDS = ["gcn2", "fagcn", "tagcn"]


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module(PKG_NAME)


@pytest.fixture(scope="module")
def oracle():
    import dss2_oracle
    return dss2_oracle


def _note(name, **errs):
    print(f"[gnn parity] {name}: " + ", ".join(f"{k} {v}" for k, v in errs.items()))


def _real_batch():
    g = golden("cigre14_real64.npz")
    b = {k: torch.from_numpy(np.ascontiguousarray(g[k])) for k in ("x", "edge_index", "edge_attr")}
    b["stats"] = tuple(torch.from_numpy(g[k]) for k in ("x_mean", "x_std", "edge_mean", "edge_std"))
    return b


def _with_self_loop_and_duplicate(b):
    ei = b["edge_index"]
    return dict(b, edge_index=torch.cat([ei, torch.tensor([[3, 3], [3, 3]]), ei[:, 5:6], ei[:, 5:6]], 1))


def _bridged(b, nodes_per_graph):
    """Graphs 0, 1 and 2 joined by one edge each: a connected component of 3 * nodes_per_graph nodes."""
    ei, n = b["edge_index"], nodes_per_graph
    return dict(b, edge_index=torch.cat([ei, torch.tensor([[n - 1, 2 * n - 1], [n, 2 * n]])], 1))


def _hub(b, n_in=320):
    src = torch.arange(100, 100 + n_in)
    return dict(b, edge_index=torch.cat([b["edge_index"], torch.stack([src, torch.full_like(src, 5)])], 1))


def _no_edges(b):
    return dict(b, edge_index=torch.zeros(2, 0, dtype=torch.int64))


def _model(pkg, kind, num_layers=8, seed=0, **kw):
    torch.manual_seed(seed)
    kw.setdefault("K", 2)
    m = pkg.gnn_dsse(8, 32, 2, num_layers, model=kind, **kw)
    with torch.no_grad():        # non-trivial attention vectors / biases
        for k, p in m.named_parameters():
            if k.endswith("bias") or "att_" in k:
                p.uniform_(-0.5, 0.5)
    return m


def _oracle_run(oracle, b, sd, kw, dtype, need_dx, loss):
    x, ei = b["x"].to(dtype), b["edge_index"]
    ref = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    xr = x[:, :8].clone().requires_grad_(need_dx)
    out = gor.GnnDSSE(ref, **kw)(xr, ei)
    o = out.detach().clone()
    if loss == "wls":
        ea = b["edge_attr"].to(dtype)
        st = tuple(s.to(dtype) for s in b["stats"])
        lv = oracle.gsp_wls_edge(input=x[:, :8], edge_input=ea[:, :6], output=out, x_mean=st[0], x_std=st[1], edge_mean=st[2],
                                 edge_std=st[3], edge_index=ei, reg_coefs=REG, num_samples=None, node_param=x[:, 8:],
                                 edge_param=ea[:, 6:])
    else:
        w = torch.linspace(-1.0, 1.0, out.numel(), dtype=dtype).view_as(out)
        lv = (out * w).sum() + 0.5 * (out ** 2).sum()
    lv.backward()
    return o, lv.item(), {k: v.grad for k, v in ref.items()}, xr.grad


def _parity(pkg, oracle, name, b, kind, num_layers=8, nonlin="leaky_relu", need_dx=True, loss="wls", **kw):
    m = _model(pkg, kind, num_layers, nonlin=nonlin, **kw)
    sd = {k: v.double() for k, v in m.state_dict().items()}
    okw = dict(num_layers=num_layers, model=kind, main_param=kw.get("main_param", 0.1), K=kw.get("K", 2), nonlin=nonlin,
               cached=kw.get("cached", True), add_self_loops=kw.get("add_self_loops", True), normalize=kw.get("normalize", True))
    o64, l64, g64, dx64 = _oracle_run(oracle, b, sd, okw, torch.float64, need_dx, loss)
    o32, l32, g32, dx32 = _oracle_run(oracle, b, sd, okw, torch.float32, need_dx, loss)
    m = m.to(DEV)
    x, ei = b["x"].to(DEV), b["edge_index"].to(DEV)
    xin = x[:, :8].clone().requires_grad_(need_dx)
    out = m(xin, ei)
    out_plain = out.detach().clone()
    if loss == "wls":
        ea = b["edge_attr"].to(DEV)
        st = tuple(s.to(DEV) for s in b["stats"])
        lv = pkg.gsp_wls_edge(input=x[:, :8], edge_input=ea[:, :6], output=out, x_mean=st[0], x_std=st[1], edge_mean=st[2],
                              edge_std=st[3], edge_index=ei, reg_coefs=REG, num_samples=None, node_param=x[:, 8:], edge_param=ea[:, 6:])
    else:
        w = torch.linspace(-1.0, 1.0, out.numel(), dtype=out.dtype, device=DEV).view_as(out)
        lv = (out * w).sum() + 0.5 * (out ** 2).sum()
    lv.backward()
    torch.cuda.synchronize()
    N = x.size(0)
    tol = max(1e-4, 8.0 / N)
    e_out, b_out = rel_err(out_plain, o64), max(1e-5, 4 * rel_err(o32, o64))
    e_loss, b_loss = abs(lv.item() - l64) / abs(l64), max(1e-5, 4 * abs(l32 - l64) / abs(l64))
    worst = (0.0, None, 1.0)
    for k, p in m.named_parameters():
        e, bound = rel_err(p.grad, g64[k]), max(tol, 4 * rel_err(g32[k], g64[k]))
        assert e < bound, (name, k, e, bound)
        worst = max(worst, (e, k, bound), key=lambda t: t[0] / t[2])
    msg = dict(out=f"{e_out:.2e} ({b_out:.2e})", loss=f"{e_loss:.2e} ({b_loss:.2e})", grad=f"{worst[0]:.2e} ({worst[2]:.2e}) {worst[1]}")
    if need_dx:
        e_dx, b_dx = rel_err(xin.grad, dx64), max(tol, 4 * rel_err(dx32, dx64))
        msg["dx"] = f"{e_dx:.2e} ({b_dx:.2e})"
        assert e_dx < b_dx, (name, e_dx, b_dx)
    _note(name, **msg)
    assert e_out < b_out and e_loss < b_loss, (name, e_out, b_out, e_loss, b_loss)
    return m


@pytest.mark.parametrize("kind", KINDS)
def test_parity_real_batch(pkg, oracle, kind):
    _parity(pkg, oracle, f"{kind} real64", _real_batch(), kind)


@pytest.mark.parametrize("case", [
    ("gcn2", dict(shared_weights=False)), ("gcn2", dict(add_self_loops=False)), ("gcn2", dict(normalize=False, main_param=0.3)),
    ("tagcn", dict(K=3, bias=False)), ("tagcn", dict(K=0)), ("tagcn", dict(K=1, normalize=False)), ("fagcn", dict(main_param=0.0)),
    ("fagcn", dict(add_self_loops=False)), ("gcn2", dict(num_layers=2, nonlin="tanh")), ("fagcn", dict(nonlin="relu")),
    ("gcn2", dict(num_layers=1)), ("tagcn", dict(nonlin="tanh", K=4))], ids=lambda c: f"{c[0]}-{c[1]}")
def test_parity_options(pkg, oracle, case):
    kind, kw = case
    kw = dict(kw)
    _parity(pkg, oracle, f"{kind} {kw}", _real_batch(), kind, num_layers=kw.pop("num_layers", 8), nonlin=kw.pop("nonlin", "leaky_relu"),
            loss="quad", **kw)


@pytest.mark.parametrize("name", gor.GOLDENS)
def test_parity_reference_goldens(pkg, oracle, name):
    """The kernels against the reference's own gnn_dsse, WLS loss and backward (tests/golden/make_gnn_goldens.py) on its seeded
    weights: output, loss, every parameter gradient and (where stored) the input gradient."""
    t, params, grads, keys, kw = gor.load_golden(name)
    b = {"x": t["x"], "edge_index": t["edge_index"], "edge_attr": t["edge_attr"],
         "stats": tuple(t[k] for k in ("x_mean", "x_std", "edge_mean", "edge_std"))}
    okw = dict(num_layers=kw["num_layers"], model=kw["model"], main_param=kw["main_param"], K=kw["K"], nonlin=kw["nonlin"],
               add_self_loops=kw["add_self_loops"])
    need_dx = "dx" in t
    o32, l32, g32, dx32 = _oracle_run(oracle, b, params, okw, torch.float32, need_dx, "wls")
    m = pkg.gnn_dsse(8, 32, 2, **kw)
    m.load_state_dict({k: v.float() for k, v in params.items()}, strict=True)
    m = m.to(DEV)
    x, ei, ea = b["x"].float().to(DEV), b["edge_index"].to(DEV), b["edge_attr"].float().to(DEV)
    st = tuple(s.float().to(DEV) for s in b["stats"])
    xin = x[:, :8].clone().requires_grad_(need_dx)
    out = m(xin, ei)
    out_plain = out.detach().clone()
    lv = pkg.gsp_wls_edge(input=x[:, :8], edge_input=ea[:, :6], output=out, x_mean=st[0], x_std=st[1], edge_mean=st[2],
                          edge_std=st[3], edge_index=ei, reg_coefs=REG, num_samples=None, node_param=x[:, 8:], edge_param=ea[:, 6:])
    lv.backward()
    torch.cuda.synchronize()
    tol = max(1e-4, 8.0 / x.size(0))
    l64 = t["loss"].item()
    e_out, b_out = rel_err(out_plain, t["out"]), max(1e-5, 4 * rel_err(o32, t["out"]))
    e_loss, b_loss = abs(lv.item() - l64) / abs(l64), max(1e-5, 4 * abs(l32 - l64) / abs(l64))
    msg = dict(out=f"{e_out:.2e} ({b_out:.2e})", loss=f"{e_loss:.2e} ({b_loss:.2e})")
    assert [k for k, _ in m.named_parameters()] == keys == sorted(grads, key=keys.index)
    for k, p in m.named_parameters():
        e, bound = rel_err(p.grad, grads[k]), max(tol, 4 * rel_err(g32[k], grads[k]))
        assert e < bound, (name, k, e, bound)
    if need_dx:
        e_dx, b_dx = rel_err(xin.grad, t["dx"]), max(tol, 4 * rel_err(dx32, t["dx"]))
        msg["dx"] = f"{e_dx:.2e} ({b_dx:.2e})"
        assert e_dx < b_dx, (name, e_dx, b_dx)
    _note(f"golden {name}", **msg)
    assert e_out < b_out and e_loss < b_loss, (name, e_out, b_out, e_loss, b_loss)


@pytest.mark.parametrize("bad", [-1, "N"])
def test_node_ids_outside_the_batch_raise(pkg, bad):
    b = _real_batch()
    x, ei = b["x"][:, :8].float().to(DEV), b["edge_index"].clone()
    ei[0, 3] = x.size(0) if bad == "N" else bad
    for kind in KINDS:
        m = _model(pkg, kind, cached=False).to(DEV)
        with pytest.raises(ValueError):
            m(x, ei.to(DEV))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("grids", [["cigre14_reswitched"], ["ober_sub"], ["cigre14", "ober_sub"]], ids=["reswitched", "ober", "mixed"])
def test_parity_synthetic(pkg, oracle, kind, grids):
    b = pkg.synthetic.make_batch(grids, 16, seed=3)
    _parity(pkg, oracle, f"{kind} {grids}", b, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("struct", ["loop_dup", "bridged", "hub", "no_edges"])
def test_parity_structures(pkg, oracle, kind, struct):
    if struct in ("loop_dup", "no_edges"):
        b = _real_batch()
    else:
        b = pkg.synthetic.make_batch(["ober_sub"] if struct == "bridged" else ["cigre14"], 32, seed=5)
    if struct == "loop_dup":
        b = _with_self_loop_and_duplicate(b)
    elif struct == "bridged":
        npg = b["x"].size(0) // 32
        b = _bridged(b, npg)
        assert 3 * npg > 192
    elif struct == "hub":
        b = _hub(b)
    else:
        b = _no_edges(b)
    _parity(pkg, oracle, f"{kind} {struct}", b, kind, loss="quad")


def _standalone_check(conv, ref_fn, x, x0, ei, params, with_x0=True):
    xg = x.clone().to(DEV).requires_grad_(True)
    x0g = x0.clone().to(DEV).requires_grad_(True) if with_x0 else None
    out = conv(xg, x0g, ei.to(DEV)) if with_x0 else conv(xg, ei.to(DEV))
    w = torch.linspace(-1, 1, out.numel(), device=DEV).view_as(out)
    (out * w).sum().backward()
    xr = x.double().requires_grad_(True)
    x0r = x0.double().requires_grad_(True)
    pr = [p.detach().double().cpu().requires_grad_(True) for p in params]
    o64 = ref_fn(xr, x0r, pr)
    (o64 * w.cpu().double()).sum().backward()
    assert rel_err(out.detach(), o64.detach()) < 1e-5
    assert rel_err(xg.grad, xr.grad) < 1e-4
    if with_x0:
        assert rel_err(x0g.grad, x0r.grad) < 1e-4
    for p, q in zip(params, pr):
        assert rel_err(p.grad, q.grad) < 1e-4


def test_standalone_convs(pkg):
    b = _with_self_loop_and_duplicate(_real_batch())
    x, ei = b["x"][:, :8].float(), b["edge_index"]
    x0 = torch.randn_like(x)
    N = x.size(0)
    torch.manual_seed(0)
    g = pkg.GCN2Conv(8, alpha=0.2, shared_weights=False).to(DEV)
    st = gor.Structure(ei, N)
    _standalone_check(g, lambda a, a0, p: gor.gcn2(a, a0, st, 0.2, p[0], p[1]), x, x0, ei, [g.weight1, g.weight2])
    f = pkg.FAConv(8, eps=0.3).to(DEV)
    with torch.no_grad():
        f.att_l.weight.uniform_(-1, 1)
        f.att_r.weight.uniform_(-1, 1)
    _standalone_check(f, lambda a, a0, p: gor.fa(a, a0, st, 0.3, p[0], p[1]), x, x0, ei, [f.att_l.weight, f.att_r.weight])
    t = pkg.TAGConv(8, 8, K=3, bias=False).to(DEV)
    assert "bias" not in t.state_dict()
    stn = gor.Structure(ei, N, True, False)
    _standalone_check(t, lambda a, a0, p: gor.tag(a, stn, p), x, x0, ei, [l.weight for l in t.lins], with_x0=False)


def test_cached_structure(pkg):
    b = _real_batch()
    x, ei = b["x"][:, :8].float().to(DEV), b["edge_index"].to(DEV)
    m = _model(pkg, "gcn2", cached=True).to(DEV)
    m_nc = _model(pkg, "gcn2", cached=False).to(DEV)
    out1 = m(x, ei)
    ei2 = ei[:, torch.randperm(ei.size(1), device=DEV)[: ei.size(1) // 2]].contiguous()
    out2 = m(x, ei2)             # same node count, another edge_index: the first structure's result
    assert torch.equal(out1, out2)
    assert not torch.equal(m_nc(x, ei2), out1)
    with pytest.raises(ValueError):
        m(x[:100], ei2[:, (ei2 < 100).all(0)])
    # more nodes: the extra nodes have no edge and no loop (the oracle's cache has the same rule)
    xb = torch.cat([x, x[:5]], 0)
    sd = {k: v.double().cpu() for k, v in m.state_dict().items()}
    ref = gor.GnnDSSE(sd, 8, "gcn2", K=2)
    ref(x.double().cpu(), ei.cpu())
    assert rel_err(m(xb, ei), ref(xb.double().cpu(), ei.cpu())) < 1e-5
    # reset_parameters clears the cache: the next call's edge_index becomes the structure
    for cv in m.model.children():
        if isinstance(cv, pkg.GCN2Conv):
            cv.reset_parameters()
            assert cv._cached_struct is None
    m_nc.load_state_dict(m.state_dict())
    assert torch.equal(m(x, ei2), m_nc(x, ei2))
    assert torch.equal(m(x, ei), m_nc(x, ei2))


@pytest.mark.parametrize("kind", KINDS)
def test_nan_input_stays_in_its_graph(pkg, kind):
    b = pkg.synthetic.make_batch(["cigre14"], 4, seed=1)
    x, ei = b["x"][:, :8].to(DEV).clone(), b["edge_index"].to(DEV)
    x[3, 2] = float("nan")
    m = _model(pkg, kind).to(DEV)
    out = m(x, ei)
    npg = x.size(0) // 4
    assert torch.isnan(out[:npg]).any() and torch.isfinite(out[npg:]).all()


def _step(pkg, m, b, st):
    for p in m.parameters():
        p.grad = None
    x, ei, ea = b
    out = m(x[:, :8], ei)
    loss = pkg.gsp_wls_edge(input=x[:, :8], edge_input=ea[:, :6], output=out, x_mean=st[0], x_std=st[1], edge_mean=st[2],
                            edge_std=st[3], edge_index=ei, reg_coefs=REG, num_samples=None, node_param=x[:, 8:], edge_param=ea[:, 6:])
    loss.backward()
    return out.detach().clone(), loss.detach().clone(), [p.grad.clone() for p in m.parameters()]


@pytest.mark.parametrize("kind", KINDS)
def test_two_runs_are_bit_identical_and_state_dict_round_trips(pkg, kind):
    b = _real_batch()
    dev_b = (b["x"].to(DEV), b["edge_index"].to(DEV), b["edge_attr"].to(DEV))
    st = tuple(s.to(DEV) for s in b["stats"])
    m = _model(pkg, kind).to(DEV)
    o1, l1, g1 = _step(pkg, m, dev_b, st)
    o2, l2, g2 = _step(pkg, m, dev_b, st)
    assert torch.equal(o1, o2) and torch.equal(l1, l2) and all(torch.equal(a, c) for a, c in zip(g1, g2))
    buf = io.BytesIO()
    torch.save(m.state_dict(), buf)
    buf.seek(0)
    m2 = pkg.gnn_dsse(8, 32, 2, 8, K=2, model=kind).to(DEV)
    m2.load_state_dict(torch.load(buf), strict=True)
    o3, l3, g3 = _step(pkg, m2, dev_b, st)
    assert torch.equal(o1, o3) and torch.equal(l1, l3) and all(torch.equal(a, c) for a, c in zip(g1, g3))


@pytest.mark.parametrize("kind", KINDS)
def test_driver_line_tracks_the_oracle(pkg, oracle, kind):
    b = _real_batch()
    torch.manual_seed(0)
    mine = pkg.runner.build_model("gnn_dsse", pkg.runner.HYPER, gnn_model=kind)
    assert isinstance(mine, pkg.gnn_dsse) and mine.num_layers == 8 and mine.K == 2 and mine.cached is False
    sd = {k: v.double().clone() for k, v in mine.state_dict().items()}
    mine = mine.to(DEV)
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
        out = gor.GnnDSSE(ref, 8, kind, K=2, cached=False)(x64[:, :8], ei)
        lr_ = oracle.gsp_wls_edge(input=x64[:, :8], edge_input=ea64[:, :6], output=out, x_mean=st64[0], x_std=st64[1],
                                  edge_mean=st64[2], edge_std=st64[3], edge_index=ei, reg_coefs=REG, num_samples=None,
                                  node_param=x64[:, 8:], edge_param=ea64[:, 6:])
        lr_.backward()
        o_ref.step()
        l_ref.append(lr_.item())
        l_gpu.append(pkg.runner.train_epoch(mine, o_gpu, [dev_b], st, pkg.runner.REG_COEFS))
    print(f"[gnn driver line {kind}] gpu", l_gpu, "oracle", l_ref)
    for a, c in zip(l_gpu, l_ref):
        assert abs(a - c) <= 1e-3 * abs(c), (l_gpu, l_ref)


@pytest.mark.parametrize("kind", KINDS)
def test_graphed_replay_equals_the_eager_step(pkg, kind):
    b = _real_batch()
    x, ei, ea = b["x"].to(DEV), b["edge_index"].to(DEV), b["edge_attr"].to(DEV)
    st = tuple(s.to(DEV) for s in b["stats"])
    torch.manual_seed(1)
    m1 = pkg.runner.build_model("gnn_dsse", pkg.runner.HYPER, gnn_model=kind).to(DEV)
    m2 = pkg.runner.build_model("gnn_dsse", pkg.runner.HYPER, gnn_model=kind).to(DEV)
    m2.load_state_dict(m1.state_dict())
    o1 = pkg.FusedAdamax(m1.parameters(), lr=3e-3, capturable=True)
    o2 = pkg.FusedAdamax(m2.parameters(), lr=3e-3, capturable=True)
    tr = pkg.runner.GraphedTrainer(m2, o2, st, REG)
    batch = {"x": x, "edge_index": ei, "edge_attr": ea, "num_graphs": 64}
    want = [pkg.runner.train_epoch(m1, o1, [batch], st, REG) for _ in range(3)]
    got = [float(tr.step(x, ei, ea)) for _ in range(3)]
    torch.cuda.synchronize()
    for a, c in zip(m1.parameters(), m2.parameters()):
        assert torch.equal(a, c), (a - c).abs().max().item()
    assert np.allclose(got, want, rtol=1e-6, atol=0), (got, want)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", ["plan", "graph"])
def test_an_epoch_of_replays_equals_the_eager_epoch(pkg, mode, kind):
    full = pkg.synthetic.make_batch(["cigre14"], 150, seed=4, violate=0.2)
    ds = pkg.dataset.DeviceDataset.from_batch(full, device=DEV)
    stats = tuple(s.to(DEV) for s in full["stats"])
    torch.manual_seed(1)
    m1 = pkg.runner.build_model("gnn_dsse", pkg.runner.HYPER, gnn_model=kind).to(DEV)
    m2 = pkg.runner.build_model("gnn_dsse", pkg.runner.HYPER, gnn_model=kind).to(DEV)
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


@pytest.mark.parametrize("kind,n_fwd_max,n_bwd_max", [("gcn2", 7, 10), ("fagcn", 7, 10), ("tagcn", 14, 17)])
def test_launch_counts_of_the_driver_line(pkg, kind, n_fwd_max, n_bwd_max):
    L = pkg._lib
    b = _real_batch()
    x, ei = b["x"].to(DEV), b["edge_index"].to(DEV)
    m = pkg.runner.build_model("gnn_dsse", pkg.runner.HYPER, gnn_model=kind).to(DEV)
    out = m(x[:, :8], ei)
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
    n_fwd, out = count(lambda: m(x[:, :8], ei))
    n_bwd, _ = count(lambda: out.backward(g))
    torch.cuda.synchronize()
    print(f"[gnn launches {kind}] forward {n_fwd}, backward {n_bwd}")
    assert n_fwd <= n_fwd_max and n_bwd <= n_bwd_max, (n_fwd, n_bwd)
