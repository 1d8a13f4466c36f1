"""GPU: the lane-group kernels (csrc/dss2_gat.hip, dss2_gine.hip, dss2_gnn.hip, dss2_lanegroup.{hpp,hip}) over the case table
of tests/lanegroup_cases.py: every lane group (8 / 16 / 32) with partial and full groups and head widths below, at and above it,
batches above the 256-workgroup cap (several trips of the grid-stride loop, partials summed over several nodes, all 256 slab rows)
and the small ends, against the fp64 restatement.

Floors as everywhere in this suite: the output within 1e-5 (max-normalised), every parameter gradient and the input gradient within
max(1e-4, 8 / N); the small ends (N = 1, 3, 33, 2049), where 8 / N would let any gradient pass, are held to 1e-4 instead
(lanegroup_cases.grad_bound).  Nothing is widened: tests/test_lanegroup_cases_cpu.py holds every case's fp32 restatement to a
quarter of these bounds.  Each case prints one ``[lanegroup shapes]`` line with its errors next to the bounds.

Then bit-identical reruns above the cap, ``lanegroup.wgrad`` + ``reduce_slabs`` on their own against G^T X in fp64, argument
structs that the C entry points must refuse before any launch (a valid struct of a real call with one field broken: non-zero
return, the entry point's name in the error text, every buffer of the call keeps its bits), the Python-level refusals, and
a standalone GATv2Conv on a batch without edges, with and without self loops."""
import ctypes as C
import importlib
import types

import pytest
import torch

import lanegroup_cases as lc
from conftest import PKG_NAME, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module(PKG_NAME)


def _run(case, m=None):
    """One forward + backward of the case on the GPU: (model, output, {name: grad}, dx)."""
    x, ei, ea = lc.inputs(case)
    if m is None:
        m = lc.build_model(case).to(DEV)
    for p in m.parameters():
        p.grad = None
    xg = x.float().to(DEV).requires_grad_(True)
    out = lc.call_model(case, m, xg, ei.to(DEV), None if ea is None else ea.float().to(DEV))
    lc.quad(out).backward()
    torch.cuda.synchronize()
    return m, out.detach(), {k: p.grad for k, p in m.named_parameters()}, xg.grad


@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.id)
def test_parity(pkg, case):
    n = lc.structure(case.struct)[1]
    m = lc.build_model(case)
    spec = lc.spec_of(case, m)
    assert spec.group == case.group
    if case.group_name == "cap":        # a later change of the geometry must not turn this into a small-batch test
        assert spec.n_slabs == pkg.lanegroup._MAX_SLABS and n > pkg.lanegroup._MAX_SLABS * (256 // spec.group)
    ref = lc.oracle_run(case, torch.float64)
    _, out, grads, dx = _run(case, m.to(DEV))
    tol = lc.grad_bound(case, n)
    e_out, e_dx = rel_err(out, ref["out"]), rel_err(dx, ref["dx"])
    assert sorted(grads) == sorted(ref["grads"])
    errs = {}
    for k, g in ref["grads"].items():
        if g is None:       # a parameter the model does not use (the shared nn of a GINE model without convs)
            assert grads[k] is None, k
            continue
        assert grads[k] is not None and grads[k].shape == g.shape, k
        errs[k] = rel_err(grads[k], g)
    worst = max(errs, key=errs.get)
    print(f"[lanegroup shapes] {case.id}: G {spec.group}, N {n}, slabs {spec.n_slabs}, out {e_out:.2e} ({lc.OUT_FLOOR:.0e}), "
          f"grad {errs[worst]:.2e} ({tol:.2e}) {worst}, dx {e_dx:.2e} ({tol:.2e})")
    assert e_out < lc.OUT_FLOOR, (case.id, e_out)
    for k, e in errs.items():
        assert e < tol, (case.id, k, e, tol)
    assert e_dx < tol, (case.id, e_dx, tol)


@pytest.mark.parametrize("case", [next(c for c in lc.CAP_CASES if c.family == f and c.group == 32) for f in lc.FAMILIES], ids=lambda c: c.id)
def test_two_runs_above_the_cap_are_bit_identical(case):
    m, o1, g1, dx1 = _run(case)
    g1 = {k: v.clone() for k, v in g1.items()}
    _, o2, g2, dx2 = _run(case, m)
    assert torch.equal(o1, o2) and torch.equal(dx1, dx2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


# ------------------------------------------------------------------------------------------
# lanegroup.wgrad + reduce_slabs on their own
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257, 16500])
@pytest.mark.parametrize("gw,xw", [(32, 32), (1, 32), (32, 1), (7, 20)])
def test_wgrad_and_slab_reduction(pkg, gw, xw, n):
    lg = pkg.lanegroup
    gen = torch.Generator().manual_seed(gw * 1000 + xw * 10 + n)
    Gb = torch.randn(n, gw + 5, generator=gen, dtype=torch.float64)
    Xb = torch.randn(n, xw + 3, generator=gen, dtype=torch.float64)
    G64, X64 = Gb[:, 2:2 + gw], Xb[:, 1:1 + xw]
    want_w, want_b = G64.t() @ X64, G64.sum(0)
    Gd, Xd = Gb.float().to(DEV)[:, 2:2 + gw], Xb.float().to(DEV)[:, 1:1 + xw]
    assert Gd.stride(0) > gw and Xd.stride(0) > xw
    col, tail = 3, 4
    total = col + gw * xw + gw + tail
    tol = 1e-4 if n == 1 else lc.grad_floor(n)       # (one product per entry at n = 1: the 8 / N term has nothing to allow for)
    for n_slabs in (1, 256, n + 3):
        slab = torch.full((n_slabs, total), 7.0, dtype=torch.float32, device=DEV)
        flat = torch.full((total,), -1.0, dtype=torch.float32, device=DEV)
        spec = types.SimpleNamespace(n_slabs=n_slabs, total=total)
        lg.wgrad([(Gd, Gd.stride(0), Xd, Xd.stride(0), gw, xw, col)], slab, spec, n, DEV)
        lg.reduce_slabs([(slab, flat, total, total, n_slabs)], DEV)
        torch.cuda.synchronize()
        # the columns around the job keep their fill in every row: the kernel wrote its own columns only
        assert (slab[:, :col] == 7.0).all() and (slab[:, total - tail:] == 7.0).all()
        chunk = -(-n // n_slabs)
        empty = slab[-(-n // chunk):, col:total - tail]       # workgroups whose chunk lies beyond the last node write zeros
        assert (empty == 0.0).all()
        e_w = rel_err(flat[col:col + gw * xw].view(gw, xw), want_w)
        e_b = rel_err(flat[col + gw * xw:col + gw * xw + gw], want_b)
        print(f"[lanegroup shapes] wgrad ({gw}, {xw}) N {n} slabs {n_slabs}: G^T X {e_w:.2e}, column sums {e_b:.2e} ({tol:.2e})")
        assert e_w < tol and e_b < tol, (n_slabs, e_w, e_b, tol)
        assert rel_err(flat[:col], torch.full((col,), 7.0 * n_slabs)) < 1e-6


# ------------------------------------------------------------------------------------------
# refusals through the C ABI
# ------------------------------------------------------------------------------------------
def _tensors(o, acc):
    if isinstance(o, torch.Tensor):
        if o.is_cuda and o.numel():
            acc.append(o)
    elif isinstance(o, dict):
        for v in o.values():
            _tensors(v, acc)
    elif isinstance(o, (list, tuple)):
        for v in o:
            _tensors(v, acc)
    return acc


def _bits(t):
    return t.detach().contiguous().view(-1).view(torch.int32).clone()


class _Capture:
    """One real forward + backward of a model with every launch's argument struct copied (after the call succeeded), and every
    buffer the calls wrote kept alive: the forward's through the autograd node, the backward's slabs and the gradients."""

    def __init__(self, pkg, monkeypatch, case):
        lg = pkg.lanegroup
        self.calls, slabs = [], []
        launch, reduce = lg._launch, lg.reduce_slabs

        def rec_launch(fn, a, sm, hook, l, hop):
            launch(fn, a, sm, hook, l, hop)
            self.calls.append((fn, type(a).from_buffer_copy(a)))

        def rec_reduce(descs, dev):
            slabs.extend(d[0] for d in descs)
            reduce(descs, dev)

        monkeypatch.setattr(lg, "_launch", rec_launch)
        monkeypatch.setattr(lg, "reduce_slabs", rec_reduce)
        x, ei, ea = lc.inputs(case)
        self.m = lc.build_model(case).to(DEV)
        self.x = x.float().to(DEV).requires_grad_(True)
        self.out = lc.call_model(case, self.m, self.x, ei.to(DEV), None if ea is None else ea.float().to(DEV))
        self.buffers = _tensors(self.out.grad_fn.st, [self.out])
        lc.quad(self.out).backward()
        torch.cuda.synchronize()
        monkeypatch.undo()
        self.buffers += slabs + [p.grad for p in self.m.parameters() if p.grad is not None] + [self.x.grad]
        self.fwd = [a for fn, a in self.calls if fn.endswith("_forward")]
        self.bwd = [a for fn, a in self.calls if fn.endswith("_backward")]

    def copy(self, a):
        return type(a).from_buffer_copy(a)


def _up_is_lo(a):
    a.up = a.lo
    a.has_up = 1


def _set(path, v):
    def f(a):
        *heads, last = path.split(".")
        for h in heads:
            a = getattr(a, h)
        setattr(a, last, v)
    return f


def _breaks(family):
    """(name, pass, base launch, mutation): base "first" / "last" forward launch (conv 0 alone / the last conv with the head),
    "first" backward launch (head + the last conv's local step), "mid" (a source pass with the local step of the conv before)."""
    c_field = {"gat": "lo.cout", "gine": "lo.cin"}.get(family, "lo.c")
    both = [("group_12", "last", _set("group", 12)),
            ("conv_c_above_group", "last", lambda a: _set(c_field, a.group + 1)(a)),
            ("head_dense_33", "last", _set("head.dense", 33)),
            ("head_nout_0", "last", _set("head.nout", 0)),
            ("edge_dim_17", "last", _set("g.ed", 17)),
            ("head_with_source_pass", "last", _up_is_lo),
            ("n_nodes_0", "last", _set("g.n_nodes", 0))]
    out = [(n, "fwd", b, f) for n, b, f in both] + [(n, "bwd", "first", f) for n, _, f in both]
    out += [("source_pass_in_a_forward", "fwd", "first", _up_is_lo),
            ("nothing_to_do", "fwd", "first", _set("has_lo", 0)),
            ("no_slab", "bwd", "first", _set("g.slab", None)),
            ("no_gradient_source", "bwd", "first", _set("has_head", 0))]
    if family == "tagcn":       # K = 2: forward hops 1, 2 per conv, adjoint hops 1, 0
        def no_weight(a):
            a.lo.W[1] = None

        def hop_1_with_buffers(a):
            a.hop, a.rout = 1, a.rin
        out += [("K_5", "fwd", "last", _set("lo.K", 5)), ("K_5", "bwd", "first", _set("lo.K", 5)),
                ("weight_missing", "fwd", "last", no_weight), ("weight_missing", "bwd", "first", no_weight),
                ("hop_0", "fwd", "first", _set("hop", 0)), ("hop_3", "fwd", "first", _set("hop", 3)),
                ("head_on_hop_1", "fwd", "last", _set("hop", 1)),
                ("up_c_is_not_lo_c", "bwd", "mid", lambda a: _set("up.c", a.lo.c - 1)(a)),
                ("local_step_on_adjoint_hop_1", "bwd", "mid", _set("hop", 1)),
                ("local_step_on_adjoint_hop_1_with_buffers", "bwd", "mid", hop_1_with_buffers)]
    return out


_REFUSAL_CASES = {"gat": lc._case("refusal", "gat", (8, 32, 2), "mixed16", num_layers=3, edge_dim=6),
                  "gine": lc._case("refusal", "gine", (8, 32, 2), "mixed16", num_layers=3, edge_dim=6),
                  "tagcn": lc._case("refusal", "tagcn", (8, 32, 2), "mixed16", num_layers=3, K=2)}


@pytest.mark.parametrize("family", list(_REFUSAL_CASES))
def test_broken_argument_structs_are_refused_before_any_launch(pkg, monkeypatch, family):
    L = pkg._lib
    cap = _Capture(pkg, monkeypatch, _REFUSAL_CASES[family])
    entry = {"gat": "dss2_gat", "gine": "dss2_gine"}.get(family, "dss2_gnn")
    sm = L.stream_ptr(torch.device(DEV))
    bases = {("fwd", "first"): cap.fwd[0], ("fwd", "last"): cap.fwd[-1], ("bwd", "first"): cap.bwd[0],
             ("bwd", "mid"): next(a for a in cap.bwd if a.has_up and a.has_lo)}
    assert bases[("fwd", "first")].has_lo and not bases[("fwd", "first")].has_head
    assert bases[("fwd", "last")].has_lo and bases[("fwd", "last")].has_head
    assert bases[("bwd", "first")].has_head and bases[("bwd", "first")].has_lo and not bases[("bwd", "first")].has_up
    # the canary sees a launch: the valid last forward struct, run again, rewrites the output that was wiped before it
    want = cap.out.detach().clone()
    with torch.no_grad():
        cap.out.fill_(123.0)
    L.check(getattr(L.lib(), entry + "_forward")(C.byref(cap.copy(bases[("fwd", "last")])), sm), "valid struct")
    torch.cuda.synchronize()
    assert torch.equal(cap.out.detach(), want)
    before = [_bits(t) for t in cap.buffers]
    seen = set()
    for name, pas, base, mutate in _breaks(family):
        fn = entry + ("_forward" if pas == "fwd" else "_backward")
        a = cap.copy(bases[(pas, base)])
        mutate(a)
        rc = getattr(L.lib(), fn)(C.byref(a), sm)
        msg = (L.lib().dss2_last_error() or b"").decode()
        torch.cuda.synchronize()
        print(f"[lanegroup shapes] refusal {fn} {name}: rc {rc}, {msg!r}")
        assert rc != 0, (fn, name)
        assert fn in msg, (fn, name, msg)
        for t, b in zip(cap.buffers, before):
            assert torch.equal(_bits(t), b), (fn, name)
        seen.add((fn, name))
    assert len(seen) == len(_breaks(family))


# ------------------------------------------------------------------------------------------
# Python-level refusals on GPU tensors
# ------------------------------------------------------------------------------------------
def test_python_level_refusals(pkg):
    lg, Lin = pkg.lanegroup, torch.nn.Linear
    ei, n = lc.structure("mixed16")
    ei = ei.to(DEV)
    x8 = torch.randn(n, 8, device=DEV)
    for build in (lambda: pkg.GAT_DSSE(33, 32, 2, 3, 6), lambda: pkg.GINE_DSSE(33, 32, 2, 3, 6), lambda: pkg.gnn_dsse(33, 32, 2, 3),
                  lambda: pkg.GAT_DSSE(8, 33, 2, 3, 6), lambda: pkg.GINE_DSSE(8, 33, 2, 3, 6), lambda: pkg.gnn_dsse(8, 33, 2, 3),
                  lambda: pkg.gnn_dsse(8, 32, 33, 3), lambda: pkg.GATv2Conv(8, 33), lambda: pkg.GATv2Conv(8, 8, edge_dim=17),
                  lambda: pkg.GINEConv(Lin(33, 8)), lambda: pkg.GCN2Conv(33, 0.1), lambda: pkg.FAConv(33),
                  lambda: pkg.gnn_dsse(8, 32, 2, 3, model="tagcn", K=5)):
        with pytest.raises(ValueError):
            build()

    def gnn_stack(convs, head):
        return lg.SequentialX0(list(convs) + list(head), convs, head, "tanh", pkg.gnn.run_gnn).to(DEV)

    def head(c=8, d=32):
        return [Lin(c, d), Lin(d, 2)]
    with pytest.raises(ValueError, match="head"):        # dense 33 that no constructor saw
        gnn_stack([pkg.GCN2Conv(8, 0.1)], head(8, 33))(x8, x8, ei)
    with pytest.raises(ValueError, match="K = 5"):
        gnn_stack([pkg.TAGConv(8, 8, K=5, bias=False)], head())(x8, x8, ei)
    with pytest.raises(ValueError, match="one kind"):
        gnn_stack([pkg.GCN2Conv(8, 0.1), pkg.FAConv(8)], head())(x8, x8, ei)
    with pytest.raises(ValueError, match="input width"):
        gnn_stack([pkg.GCN2Conv(8, 0.1)], head(12))(x8, x8, ei)
    with pytest.raises(ValueError, match="in_channels must equal out_channels"):
        gnn_stack([pkg.TAGConv(8, 12, K=2, bias=False)], head(12))(x8, x8, ei)
    ea = torch.randn(ei.size(1), 6, device=DEV)
    convs = [pkg.GINEConv(Lin(8, 8), edge_dim=6), pkg.GINEConv(Lin(8, 8), edge_dim=6)]
    h = head()
    with pytest.raises(ValueError, match="share the one nn"):
        lg.Sequential(convs + h, convs, h, "tanh", pkg.gine.run_gine).to(DEV)(x8, ei, ea)
    convs = [pkg.GATv2Conv(8, 8, edge_dim=6)]
    h = head(8, 33)
    with pytest.raises(ValueError, match="head"):
        lg.Sequential(convs + h, convs, h, "tanh", pkg.gat.run_gat).to(DEV)(x8, ei, ea)


@pytest.mark.parametrize("loops", [True, False])
def test_gat_on_a_batch_without_edges(pkg, loops):
    """GATv2 without edges: every node attends to its self loop alone; without self loops the layer gives its bias.  (The table's
    N = 1 case first failed here: run_gat sent E = 0 to the structure build, which refuses it; it now takes lanegroup.NoEdges
    as GINE and gnn_dsse do.)"""
    torch.manual_seed(3)
    conv = pkg.GATv2Conv(5, 12, edge_dim=3, add_self_loops=loops)
    with torch.no_grad():
        conv.bias.uniform_(-0.5, 0.5)
    p = lc.gat_oracle.conv_params({k: v.detach().double().requires_grad_(True) for k, v in conv.state_dict().items()}, "")
    x = torch.randn(4, 5, dtype=torch.float64)
    ei, ea = torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0, 3, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    want = lc.gat_oracle.gatv2(xr, ei, ea, p, 0.2, loops)
    lc.quad(want).backward()
    conv = conv.to(DEV)
    xg = x.float().to(DEV).requires_grad_(True)
    out = conv(xg, ei.to(DEV), ea.float().to(DEV))
    lc.quad(out).backward()
    torch.cuda.synchronize()
    assert rel_err(out, want) < lc.OUT_FLOOR
    if loops:
        assert rel_err(xg.grad, xr.grad) < 1e-4
        named = dict(conv.named_parameters())
        for k, name in (("Wl", "lin_l.weight"), ("bl", "lin_l.bias"), ("bias", "bias")):
            assert rel_err(named[name].grad, p[k].grad) < 1e-4, name
        # a softmax over one self loop is constant: these gradients vanish analytically.  The kernel forms them as alpha (da - T)
        # with T = alpha da, where the lanes' butterfly sums may differ in the last bit, so they are rounding; they have no scale
        # of their own and are held to 1e-4 of the layer's largest gradient (the per-module measure of test_gpu_gat.py)
        scale = max(v.grad.abs().max().item() for v in p.values() if v is not None and v.grad is not None)
        for name in ("att", "lin_r.weight", "lin_r.bias", "lin_edge.weight"):
            assert named[name].grad is not None and named[name].grad.abs().max().item() < 1e-4 * scale, name
    else:
        assert torch.equal(out.detach().cpu(), conv.bias.detach().cpu().expand(4, 12)) and not xg.grad.any()
        assert rel_err(conv.bias.grad, p["bias"].grad) < 1e-4
