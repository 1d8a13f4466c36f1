"""GPU: GATv2Conv with several heads (concatenated and averaged) and GAT_DSSE(heads=H, concat=False) on the kernels of
csrc/dss2_gat.hip, against the fp64 restatement tests/gat_heads_oracle.py and against single-head convs carrying the heads' row
blocks (the path the reference goldens pin).

Bounds, as in tests/test_gpu_gat.py: outputs within 1e-5 (max-normalised), gradients within max(1e-4, 8 / N), each gradient bound
widened to 4x the error of the same restatement run in fp32 on the CPU where that is larger; for the model the output and loss
bounds are widened the same way (_model_parity there).  Every bound is printed beside its error.  Then bit-identical reruns,
launch-plan and hipGraph replays equal to the eager step, the launch counts of one step, and the C entry's refusal."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import gat_heads_oracle as gho
from conftest import PKG_NAME, golden, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REG = {"mu_v": 1e-1, "mu_theta": 1e-1, "lam_v": 1e-4, "lam_p": 1e-8, "lam_pf": 1e-6, "lam_reg": 1e2}
_CACHE = {}


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module(PKG_NAME)


@pytest.fixture(scope="module")
def oracle():
    import dss2_oracle
    return dss2_oracle


def _real_batch():
    if "real" not in _CACHE:
        g = golden("cigre14_real64.npz")
        b = {k: torch.from_numpy(np.ascontiguousarray(g[k])) for k in ("x", "edge_index", "edge_attr")}
        b["stats"] = tuple(torch.from_numpy(g[k]) for k in ("x_mean", "x_std", "edge_mean", "edge_std"))
        _CACHE["real"] = b
    return _CACHE["real"]


def _small_graph(pkg, kind="plain"):
    """The directed 3-graph CIGRE batch: 45 nodes (several workgroups' slab rows at every lane group), bus 0 of every graph
    without an incoming edge.  "loops": plus a self loop on node 3 and a second copy of edge 5."""
    if "small" not in _CACHE:
        _CACHE["small"] = pkg.synthetic.make_batch(["cigre14"], 3, seed=3)["edge_index"]
    ei = _CACHE["small"]
    if kind == "loops":
        ei = torch.cat([ei, torch.tensor([[3], [3]]), ei[:, 5:6]], 1)
    return ei


def _relabelled(b, seed):
    """The same batch with its nodes relabelled and its edges reordered: another summation order for every sum."""
    gen = torch.Generator().manual_seed(seed)
    n, e = b["x"].size(0), b["edge_index"].size(1)
    perm, ep = torch.randperm(n, generator=gen), torch.randperm(e, generator=gen)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(n)
    return dict(b, x=b["x"][perm], edge_index=inv[b["edge_index"]][:, ep], edge_attr=b["edge_attr"][ep])


_KEYS = (("att", "att"), ("bias", "bias"), ("lin_l.weight", "Wl"), ("lin_l.bias", "bl"), ("lin_r.weight", "Wr"), ("lin_r.bias", "br"),
         ("lin_edge.weight", "We"))


def _load(conv, p):
    """The oracle's parameter dict into a conv (shared weights: lin_r is lin_l)."""
    own = conv.state_dict()
    sd = {k: p[n].float().reshape(own[k].shape) for k, n in _KEYS if p.get(n) is not None and k in own}
    conv.load_state_dict(sd, strict=True)
    return conv


def _conv_reference(p, x64, ei, ea64, heads, concat, loops, share, dtype):
    """(out, {state_dict key: grad}, dx) of the restatement at dtype on the CPU, loss sum(out * w)."""
    q = {n: (None if v is None else v.to(dtype).clone().requires_grad_(True)) for n, v in p.items()}
    if share:
        q["Wr"], q["br"] = q["Wl"], q["bl"]
    x = x64.to(dtype).clone().requires_grad_(True)
    out = gho.gatv2_heads(x, ei, None if ea64 is None else ea64.to(dtype), q, heads, concat, add_self_loops=loops)
    w = torch.linspace(-1, 1, out.numel(), dtype=dtype).view_as(out)
    (out * w).sum().backward()
    grads = {k: q[n].grad for k, n in _KEYS if q.get(n) is not None and not (share and n in ("Wr", "br"))}
    return out.detach(), grads, x.grad


CONV_CASES = {
    # name: (cin, C, H, concat, edge_dim, share_weights, add_self_loops, bias, graph)
    "h4_mean_full32": (8, 8, 4, False, 6, False, True, True, "plain"),
    "h4_concat_full32": (8, 8, 4, True, 6, False, True, True, "plain"),
    "h2_g16": (8, 8, 2, True, 6, False, True, True, "plain"),
    "h3_c5_inert_lanes": (5, 5, 3, True, 6, False, True, True, "plain"),
    "h3_c5_mean": (5, 5, 3, False, 3, False, True, True, "plain"),
    "h2_c3_g8": (3, 3, 2, False, 6, False, True, True, "plain"),
    "h4_c2": (8, 2, 4, True, 6, False, True, True, "plain"),
    "no_edge_dim": (8, 8, 2, False, None, False, True, True, "plain"),
    "share_weights": (8, 8, 4, False, 6, True, True, True, "plain"),
    "no_loops_isolated_target": (8, 8, 4, True, 6, False, False, True, "plain"),
    "no_loops_isolated_target_mean": (8, 4, 3, False, 6, False, False, True, "plain"),
    "no_bias": (8, 8, 2, False, 6, False, True, False, "plain"),
    "self_loop_and_duplicate": (8, 8, 4, False, 6, False, True, True, "loops"),
    "self_loop_and_duplicate_concat": (6, 4, 3, True, 16, False, True, True, "loops"),
    "wide_input": (20, 4, 2, True, 6, False, True, True, "plain"),
}


def _conv_case(pkg, name):
    """Everything one conv case needs, computed once: the conv on the GPU, its inputs and the fp64 / fp32 references."""
    if ("conv", name) in _CACHE:
        return _CACHE[("conv", name)]
    cin, c, H, concat, ed, share, loops, bias, kind = CONV_CASES[name]
    ei = _small_graph(pkg, kind)
    N, E = 45, ei.size(1)
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x64 = torch.randn(N, cin, generator=g, dtype=torch.float64)
    ea64 = torch.randn(E, ed, generator=g, dtype=torch.float64) if ed else None
    p = gho.random_conv_params(cin, c, H, concat=concat, ed=ed, bias=bias, seed=len(name))
    if share:
        p["Wr"], p["br"] = p["Wl"], p["bl"]
    conv = _load(pkg.GATv2Conv(cin, c, heads=H, concat=concat, edge_dim=ed, share_weights=share, add_self_loops=loops, bias=bias), p).to(DEV)
    r64 = _conv_reference(p, x64, ei, ea64, H, concat, loops, share, torch.float64)
    r32 = _conv_reference(p, x64, ei, ea64, H, concat, loops, share, torch.float32)
    _CACHE[("conv", name)] = (conv, p, x64, ei, ea64, r64, r32)
    return _CACHE[("conv", name)]


def _run_conv(conv, x64, ei, ea64, w_like):
    for q in conv.parameters():
        q.grad = None
    xg = x64.float().to(DEV).requires_grad_(True)
    out = conv(xg, ei.to(DEV), None if ea64 is None else ea64.float().to(DEV))
    w = torch.linspace(-1, 1, w_like.numel(), dtype=torch.float64).view_as(w_like).float().to(DEV)
    (out * w).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), {k: q.grad.clone() for k, q in conv.named_parameters()}, xg.grad


@pytest.mark.parametrize("name", sorted(CONV_CASES))
def test_multi_head_conv_against_the_oracle(pkg, name):
    conv, p, x64, ei, ea64, (o64, g64, dx64), (o32, g32, dx32) = _conv_case(pkg, name)
    cin, c, H, concat, ed, share, loops, bias, kind = CONV_CASES[name]
    out, grads, dx = _run_conv(conv, x64, ei, ea64, o64)
    assert tuple(out.shape) == (45, H * c if concat else c)
    assert sorted(grads) == sorted(g64), (sorted(grads), sorted(g64))
    tol = max(1e-4, 8.0 / 45)
    report = {"out": (rel_err(out, o64), 1e-5), "dx": (rel_err(dx, dx64), max(tol, 4 * rel_err(dx32, dx64)))}
    for k in g64:
        assert grads[k].shape == g64[k].shape, k
        report[k] = (rel_err(grads[k], g64[k]), max(tol, 4 * rel_err(g32[k], g64[k])))
    print(f"[gat heads conv] {name}: " + ", ".join(f"{k} {e:.2e} (bound {b:.2e})" for k, (e, b) in report.items()))
    for k, (e, b) in report.items():
        assert e < b, (name, k, e, b)
    if not loops:      # the isolated targets (no incoming edge, no self loop): an empty softmax, the bias alone
        indeg = torch.bincount(ei[1], minlength=45)
        assert (indeg == 0).any()
        want = p["bias"].float() if bias else torch.zeros(out.size(1))
        assert torch.equal(out[indeg == 0].cpu(), want.expand(int((indeg == 0).sum()), -1))


@pytest.mark.parametrize("name", ["h4_mean_full32", "h4_concat_full32", "h3_c5_inert_lanes", "h3_c5_mean", "h2_c3_g8", "self_loop_and_duplicate"])
def test_multi_head_conv_is_its_single_head_convs(pkg, name):
    """The multi-head conv against H single-head GATv2Conv carrying its row blocks, on the GPU: concatenated, or averaged with
    the bias added once.  The single-head kernels are the ones the known answers and the reference goldens pin."""
    conv, p, x64, ei, ea64, (o64, g64, _), (_, g32, _) = _conv_case(pkg, name)
    cin, c, H, concat, ed, share, loops, bias, kind = CONV_CASES[name]
    out, grads, dx = _run_conv(conv, x64, ei, ea64, o64)
    singles = []
    for h in range(H):
        hp = gho.head_params(p, h, H, concat)
        if hp["bias"] is None:
            hp["bias"] = torch.zeros(c, dtype=torch.float64)
        singles.append(_load(pkg.GATv2Conv(cin, c, edge_dim=ed, add_self_loops=loops), hp).to(DEV))
    xg = x64.float().to(DEV).requires_grad_(True)
    eid, ea = ei.to(DEV), None if ea64 is None else ea64.float().to(DEV)
    parts = [s(xg, eid, ea) for s in singles]
    mean_bias = p["bias"].float().to(DEV).requires_grad_(True)
    want = torch.cat(parts, 1) if concat else torch.stack(parts).mean(0) + mean_bias
    w = torch.linspace(-1, 1, o64.numel(), dtype=torch.float64).view_as(o64).float().to(DEV)
    (want * w).sum().backward()
    torch.cuda.synchronize()
    tol = max(1e-4, 8.0 / 45)
    rows = lambda k: torch.cat([dict(s.named_parameters())[k].grad.reshape(c, -1) for s in singles]).reshape(grads[k].shape)  # noqa: E731
    report = {"out": (rel_err(out, want), 1e-5), "dx": (rel_err(dx, xg.grad), tol)}
    for k in grads:
        if k == "bias":
            ref = rows(k) if concat else mean_bias.grad
        else:
            ref = rows(k)
        report[k] = (rel_err(grads[k], ref), max(tol, 4 * rel_err(g32[k], g64[k])))
    print(f"[gat heads split] {name}: " + ", ".join(f"{k} {e:.2e} (bound {b:.2e})" for k, (e, b) in report.items()))
    for k, (e, b) in report.items():
        assert e < b, (name, k, e, b)


def _oracle_run(oracle, b, sd, num_layers, heads, nonlin, dtype):
    """The model restatement with the WLS loss at dtype on the CPU: (output, loss value, {name: grad}, dx)."""
    x, ei, ea = b["x"].to(dtype), b["edge_index"], b["edge_attr"].to(dtype)
    ref = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    xr = x[:, :8].clone().requires_grad_(True)
    out = gho.gat_dsse_heads(xr, ei, ea[:, :6], ref, num_layers, heads, nonlin)
    st = tuple(s.to(dtype) for s in b["stats"])
    lv = oracle.gsp_wls_edge(input=x[:, :8], edge_input=ea[:, :6], output=out, x_mean=st[0], x_std=st[1], edge_mean=st[2],
                             edge_std=st[3], edge_index=ei, reg_coefs=REG, num_samples=None, node_param=x[:, 8:], edge_param=ea[:, 6:])
    lv.backward()
    return out.detach().clone(), lv.item(), {k: v.grad for k, v in ref.items()}, xr.grad


def _wls(pkg, b, out):
    x, ei, ea, st = b
    return pkg.gsp_wls_edge(input=x[:, :8], edge_input=ea[:, :6], output=out, x_mean=st[0], x_std=st[1], edge_mean=st[2],
                            edge_std=st[3], edge_index=ei, reg_coefs=REG, num_samples=None, node_param=x[:, 8:], edge_param=ea[:, 6:])


def _dev_batch():
    b = _real_batch()
    return (b["x"].to(DEV), b["edge_index"].to(DEV), b["edge_attr"].to(DEV), tuple(s.to(DEV) for s in b["stats"]))


def _model_check(pkg, oracle, b, sd, num_layers, heads, nonlin):
    """GAT_DSSE(8, 32, 2, L, 6, heads=H, concat=False) with weights sd on batch b against the restatement (see the tests)."""
    mine = pkg.GAT_DSSE(8, 32, 2, num_layers, 6, heads=heads, concat=False, nonlin=nonlin)
    mine.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    mine = mine.to(DEV)
    o64, l64, g64, dx64 = _oracle_run(oracle, b, sd, num_layers, heads, nonlin, torch.float64)
    o32, l32, g32, dx32 = _oracle_run(oracle, b, sd, num_layers, heads, nonlin, torch.float32)
    _, _, g32r, _ = _oracle_run(oracle, _relabelled(b, 1), sd, num_layers, heads, nonlin, torch.float32)
    db = (b["x"].to(DEV), b["edge_index"].to(DEV), b["edge_attr"].to(DEV), tuple(t.to(DEV) for t in b["stats"]))
    xin = db[0][:, :8].detach().clone().requires_grad_(True)
    out = mine(xin, db[1], db[2][:, :6])
    loss = _wls(pkg, db, out)
    loss.backward()
    torch.cuda.synchronize()
    N = db[0].size(0)
    tol = max(1e-4, 8.0 / N)
    report = {"out": (rel_err(out, o64), max(1e-5, 4 * rel_err(o32, o64))),
              "loss": (abs(loss.item() - l64) / abs(l64), max(1e-5, 4 * abs(l32 - l64) / abs(l64))),
              "dx": (rel_err(xin.grad, dx64), max(tol, 4 * rel_err(dx32, dx64)))}
    named = dict(mine.named_parameters())
    assert sorted(named) == sorted(sd)
    for k in sd:
        e32 = max(rel_err(g32[k], g64[k]), rel_err(g32r[k], g64[k]))
        report[k] = (rel_err(named[k].grad, g64[k]), max(tol, 4 * e32))
    print(f"[gat heads model] L={num_layers} H={heads} {nonlin}: " + ", ".join(f"{k} {e:.2e} (bound {bd:.2e})" for k, (e, bd) in report.items()))
    for k, (e, bd) in report.items():
        assert e < bd, (k, e, bd)


@pytest.mark.parametrize("num_layers,heads,nonlin,gain", [(3, 2, "leaky_relu", 1.0), (8, 4, "leaky_relu", 3.0), (3, 4, "tanh", 1.0)])
def test_gat_dsse_head_mean_against_the_oracle(pkg, oracle, num_layers, heads, nonlin, gain):
    """GAT_DSSE(8, 32, 2, L, 6, heads=H, concat=False) + gsp_wls_edge on the 64 real CIGRE graphs: output, loss, every gradient
    and dx, with the bounds of test_gpu_gat._model_parity (the fp32 gradient error also over a relabelled copy of the batch).

    The weights of the L = 8 case carry gain = 3 on lin_l / lin_r (entries up to 1.8).  Every layer averages over a target's
    neighbours and then over the H heads, so with entries up to 0.6 seven layers contract the features until all nodes of a graph
    carry the same row: the attention is then uniform, and the gradients of att, lin_r and lin_edge of the late layers, which
    vanish analytically there (the softmax is shift-invariant per target), are 1e-10 of the other gradients of their conv.  A
    comparison normalised by such a gradient's own maximum measures rounding alone: the restatement in fp32 is off by 5e-2 ..
    2e-1 of it at gain 1 (seeds 0 .. 9), and the kernels, whose backward normalises alpha by the forward's online-softmax sum
    where torch renormalises from scratch, by more (measured at gain 1, seed 9: att, lin_r, lin_edge of convs 4 .. 7 off by 0.1
    .. 180 of their maxima of 1e-10 .. 1e-8, every other gradient, the loss and the output within the bounds).  With gain 3 the
    features keep their spread (the restatement's gradients span 2e1 .. 1e4 and its fp32 run holds them to 1e-5), so the
    comparison tests the arithmetic."""
    _model_check(pkg, oracle, _real_batch(), gho.random_state_dict(num_layers, heads, seed=7, gain=gain), num_layers, heads, nonlin)


def test_gat_dsse_head_mean_reference_golden(pkg, oracle):
    """tests/golden/case_gat_heads4_mean.npz (make_gat_heads_goldens.py: the reference's own GAT_DSSE(heads=4, concat=False,
    num_layers=3), float64) with its weights: the GPU against the fp64 restatement, which tests/test_gat_heads_cpu.py holds to the
    reference's outputs and gradients."""
    g = golden("case_gat_heads4_mean.npz")
    b = {k: torch.from_numpy(np.ascontiguousarray(g[k])).float() for k in ("x", "edge_attr")}
    b["edge_index"] = torch.from_numpy(g["edge_index"])
    b["stats"] = tuple(torch.from_numpy(g[k]).float() for k in ("x_mean", "x_std", "edge_mean", "edge_std"))
    sd = {k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")}
    _model_check(pkg, oracle, b, sd, int(g["num_layers"]), int(g["heads"]), str(g["nonlin"]))


def _step(pkg, m, db):
    for p in m.parameters():
        p.grad = None
    out = m(db[0][:, :8], db[1], db[2][:, :6])
    loss = _wls(pkg, db, out)
    loss.backward()
    return out.detach().clone(), loss.detach().clone(), [p.grad.clone() for p in m.parameters()]


def _driver(pkg, heads, seed=1):
    torch.manual_seed(seed)
    return pkg.runner.build_model("GAT_DSSE", {**pkg.runner.HYPER, "heads": heads}).to(DEV)


def test_two_runs_are_bit_identical(pkg):
    db = _dev_batch()
    m = _driver(pkg, 4)
    o1, l1, g1 = _step(pkg, m, db)
    o2, l2, g2 = _step(pkg, m, db)
    assert torch.equal(o1, o2) and torch.equal(l1, l2) and all(torch.equal(a, c) for a, c in zip(g1, g2))
    conv, p, x64, ei, ea64, (o64, _, _), _ = _conv_case(pkg, "h3_c5_inert_lanes")
    a, b = _run_conv(conv, x64, ei, ea64, o64), _run_conv(conv, x64, ei, ea64, o64)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and all(torch.equal(a[1][k], b[1][k]) for k in a[1])


def test_graphed_replay_equals_the_eager_step(pkg):
    x, ei, ea, st = _dev_batch()
    m1, m2 = _driver(pkg, 4), _driver(pkg, 4)
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


def test_planned_replays_equal_the_eager_epoch(pkg):
    full = pkg.synthetic.make_batch(["cigre14"], 128, seed=4, violate=0.2)
    ds = pkg.dataset.DeviceDataset.from_batch(full, device=DEV)
    stats = tuple(s.to(DEV) for s in full["stats"])
    m1, m2 = _driver(pkg, 2), _driver(pkg, 2)
    m2.load_state_dict(m1.state_dict())
    o1 = pkg.optim.FusedAdamax(m1.parameters(), lr=3e-3, capturable=True)
    o2 = pkg.optim.FusedAdamax(m2.parameters(), lr=3e-3, capturable=True)
    tr = pkg.runner.EpochTrainer(m2, o2, stats, REG, ds, 64, shuffle=False, mode="plan")
    want = pkg.runner.train_epoch(m1, o1, pkg.dataset.DataLoader(ds, batch_size=64, shuffle=False), stats, REG)
    tr.train_epoch()
    got = tr.mean_loss()
    torch.cuda.synchronize()
    for a, c in zip(m1.parameters(), m2.parameters()):
        assert torch.equal(a, c), (a - c).abs().max().item()
    assert np.allclose(got, want, rtol=1e-6, atol=0), (got, want)


def test_launch_counts_do_not_depend_on_the_head_count(pkg):
    L = pkg._lib
    x, ei, ea, _ = _dev_batch()

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

    counts = {}
    for heads in (1, 4):
        m = _driver(pkg, heads)
        out = m(x[:, :8], ei, ea[:, :6])         # warm: topology cached
        g = torch.ones_like(out)
        out.backward(g)
        torch.cuda.synchronize()
        n_fwd, out = count(lambda: m(x[:, :8], ei, ea[:, :6]))
        n_bwd, _ = count(lambda: out.backward(g))
        torch.cuda.synchronize()
        counts[heads] = (n_fwd, n_bwd)
    print(f"[gat heads launches] (forward, backward) by heads: {counts}")
    assert counts[4] == counts[1] and counts[4][0] <= 7 and counts[4][1] <= 2 * 7 + 2, counts


def test_the_c_entry_refuses_more_lanes_than_the_group(pkg):
    """dss2_gat_forward with heads * Cp above the lane group: an error code and a message, and no launch (y keeps its fill)."""
    L = pkg._lib
    N = 4
    f = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)  # noqa: E731
    rowptr = torch.zeros(N + 1, dtype=torch.int32, device=DEV)
    y = torch.full((N, 16), 7.0, dtype=torch.float32, device=DEV)
    a = L.GatArgs()
    g = a.g
    g.rowptr = g.col = g.ent = g.rowptrT = g.colT = g.entT = rowptr.data_ptr()
    g.n_nodes, g.ed, g.add_self_loops, g.slope, g.n_slabs, g.slab_len = N, 0, 1, 0.2, 1, 0
    keep = [f(16, 8), f(16), f(N, 8), f(2, N * 2)]
    d = a.lo
    d.att, d.bias, d.Wl, d.bl, d.Wr, d.br = keep[1].data_ptr(), keep[1].data_ptr(), keep[0].data_ptr(), keep[1].data_ptr(), keep[0].data_ptr(), keep[1].data_ptr()
    d.h, d.ldh, d.y, d.m, d.s = keep[2].data_ptr(), 8, y.data_ptr(), keep[3].data_ptr(), keep[3].data_ptr() + 4 * N * 2
    d.cin, d.cout, d.heads, d.concat = 8, 8, 2, 1
    a.has_lo, a.group = 1, 8                     # 2 heads * 8 lanes in a group of 8
    rc = L.lib().dss2_gat_forward(C.byref(a), L.stream_ptr(torch.device(DEV)))
    msg = L.lib().dss2_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0 and "heads" in msg and "16" in msg, (rc, msg)
    assert torch.equal(y, torch.full_like(y, 7.0))
    d.cout, d.heads = 5, 5                       # Cp = 8: 40 lanes, above every group
    a.group = 32
    assert L.lib().dss2_gat_backward(C.byref(a), L.stream_ptr(torch.device(DEV))) != 0
    assert "heads" in L.lib().dss2_last_error().decode()
