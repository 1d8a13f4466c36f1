"""GPU: csrc/dss2_loss.hip -- wls_partials_kernel, wls_grad_kernel, pflow_kernel, the eval_* kernels and vminmax_kernel -- on the graphs of
tests/loss_cases.py: buses of degree 0 and 5 .. 13 (an empty incidence row; up to four rounds of WLS_GB = 4 branches, full and with 1 and
3 live entries, from-end and to-end entries in every round number), parallel branches, a hub across the workgroup boundary, N = 256 and 257,
and a batch beyond 65 536 buses and branches (the strided loops of the evaluation and of vminmax_kernel, the two-launch finish).

Every case (8 layouts x 2 families x 2 output regimes) is held to the fp64 oracle with its max() ties and penalty gates pinned to the
kernel's own choices (loss_cases.pinned_branches): loss, the masked output (exactly), the eight flow columns, d loss / d output over the
batch and graph by graph.  A bound is max(1e-5, 4 x the error of the fp32 ORACLE for that quantity against the fp64 one, same pins): measured
on the reference arithmetic, never on the kernel.  Then what must hold to the bit: copies of a graph give equal rows, 4 x the upstream
gradient gives 4 x the gradient, an output with row stride 4 gives the contiguous one's bits and leaves the other columns alone, two runs
agree, and the fused finish agrees with the two-launch one.

Measured on the MI355X, worst error / bound over the cases of a group (the tests print every error beside its bound; run with -s):
  loss 0.070 (iso_heavy, cigre14, physical)    flows 0.518 (one_wg, cigre14, physical: the line loading)
  gradient over the batch 0.313, graph by graph 0.327 (both n256, ober_sub, physical): no graph needed more than the batch-wide bound
  get_pflow (16 cases) 0.125 (big, cigre14: Q_to)    evaluation metrics (6 cases) 0.055 (one_wg, ober_sub: mae_loading_trafos)
get_pflow's bound also admits ROUNDINGS x 2^-24 x sum |terms| / max |value| of the column (`_flow_budget`): with one branch the fp32 oracle's
error is a single sample of the rounding noise (Q_from of a transformer: 2e-6, at sum |terms| / |Q| = 620; the kernel's sample was 3.5e-5).

Mutations of scratch builds of csrc/dss2_loss.hip (arithmetic only, none kept) and what failed:
  rounds after the first skipped in wls_grad_kernel     -> the gradient of all 32 cases of test_loss_flows_and_gradient_... (error 0.46 .. 0.54)
  the same in wls_partials_kernel                       -> the same 32 cases, at their first step: the skipped branches' flow rows keep the
                                                           sentinel, which `check_pins` refuses as a max() choice that is no near-tie
  gth += dd with the sign fixed                         -> the gradient of the same 32 cases (error 1.2 .. 2.0)
  eval_partials_kernel taking one element per thread    -> test_eval_batch_metrics on `big` only, both families (rmse_v off by 5e-4)
  gscale ignored                                        -> the 4 x property of the same 32 cases

What no test here can see: (1) a reordering of the additions inside one bus's row that keeps fp32 rounding within the bound; (2) the
clamped tail loads of gather_branches (entries beyond a row repeat its last one: loaded, never used -- any in-bounds address gives the
same results); (3) a stale V_lv / V_hv cache after a raw write that is NOT followed by invalidate_vminmax, which is the documented contract.
"""
import copy
import ctypes as C
import importlib

import pytest
import torch

import loss_cases as lc
import dss2_oracle as oracle
import dss2_topology_oracle as topo_oracle
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = lc.case_ids()
IDS = ["-".join(c) for c in CASES]
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module(PKG_NAME)
    p._lib.lib()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return p


_DEVICE = {}


def _dev(c):
    """The case's fp32 device tensors (x, edge_index, edge_attr, stats, output, y), uploaded once."""
    key = (c.layout, c.family, c.regime)
    if key not in _DEVICE:
        _DEVICE[key] = lc.tensors(c, torch.float32, DEV)
    return _DEVICE[key]


def _record(kind, name, errs, bounds):
    parts = " ".join(f"{k}={errs[k]:.2e}/{bounds[k]:.2e}" for k in bounds)
    print(f"[loss-shapes {kind}] {name}: {parts}")


class _RowStride4(torch.autograd.Function):
    """src [N, 2] -> a tensor of the same values with strides (4, 1) that owns its storage, the rest of which holds SENTINEL.  (Not a view:
    autograd refuses a two-output function that modifies a view in place, and the loss returns (loss, output).)"""

    @staticmethod
    def forward(ctx, src):
        n = src.shape[0]
        o = torch.empty_strided((n, 2), (4, 1), dtype=src.dtype, device=src.device)
        torch.as_strided(o, (4 * n - 2,), (1,)).fill_(SENTINEL)
        o.copy_(src)
        return o

    @staticmethod
    def backward(ctx, g):
        return g


def _loss(pkg, x, ei, ea, st, o, **kw):
    return pkg.data.gsp_wls_edge(input=x[:, :8], edge_input=ea[:, :6], output=o, x_mean=st[0], x_std=st[1], edge_mean=st[2],
                                 edge_std=st[3], edge_index=ei, reg_coefs=lc.REG, num_samples=None, node_param=x[:, 8:],
                                 edge_param=ea[:, 6:], **kw)


def _run(pkg, g, scale=None, stride4=False):
    """One forward + backward of the loss: (loss [0-dim], d loss / d output, flows [E, 8], output after the call)."""
    x, ei, ea, st, out, _ = g
    leaf = out.clone().requires_grad_(True)
    o = _RowStride4.apply(leaf) if stride4 else leaf * 1.0
    flows = torch.full((ei.shape[1], 8), SENTINEL, device=DEV)
    loss = _loss(pkg, x, ei, ea, st, o, pflow_out=flows)
    (loss if scale is None else scale * loss).backward()
    return loss.detach().clone(), leaf.grad.clone(), flows, o.detach()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_loss_flows_and_gradient_against_the_pinned_fp64_referee(pkg, case):
    c = lc.build_case(*case)
    g = _dev(c)
    topo = pkg.topology.get_topology(g[1], c.N)
    want = topo_oracle.TopologyOracle(c.ei, c.N)
    assert torch.equal(topo.inc_rowptr.cpu(), want.inc_rowptr) and torch.equal(topo.inc_ent.cpu(), want.inc_ent)
    loss, grad, flows, o_after = _run(pkg, g)
    # output after the call: theta masked in place, nothing else touched
    masked = g[4].clone()
    masked[:, 1] *= 1.0 - g[0][:, 9]
    assert torch.equal(o_after, masked)
    r64 = lc.referee(c, torch.float64, o_after, flows)
    r32 = lc.referee(c, torch.float32, o_after, flows)
    noise = lc.errors(r32.loss, r32.grad, r32.flows, r64, c)
    err = lc.errors(loss.item(), grad, flows, r64, c)
    bounds = {k: lc.bound(v) for k, v in noise.items() if not k.startswith("_")}
    _record("loss", "-".join(case), err, bounds)
    for k, b in bounds.items():
        note = ""
        if k == "grad_per_graph" and err[k] > b:      # the graph's conditioning, for the reader of a failure
            rows = c.graph == err["_worst_graph"]
            note = f"graph {err['_worst_graph']} ({int(rows.sum())} buses): max |ref grad| {r64.grad[rows].abs().max():.3e} of {r64.grad.abs().max():.3e} in the batch"
        assert err[k] <= b, (k, err[k], b, note)
    # bit-exact: a second run; copies of the set; 4 x the upstream gradient
    loss2, grad2, flows2, _ = _run(pkg, g)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2) and torch.equal(flows, flows2)
    if c.layout in lc.COPIED:
        k = lc.COPIED[c.layout]
        fl, gr = flows.view(k, lc.SET_E, 8), grad.view(k, lc.SET_N, 2)
        assert torch.equal(fl, fl[:1].expand_as(fl)) and torch.equal(gr, gr[:1].expand_as(gr))
    loss4, grad4, _, _ = _run(pkg, g, scale=4.0)
    assert torch.equal(loss4, loss) and torch.equal(grad4, 4.0 * grad) and grad.abs().max() > 0


@pytest.mark.parametrize("layout", ["one_wg", "n257_hub", "straddle", "big"])
@pytest.mark.parametrize("family", list(lc.FAMILIES))
def test_row_stride_four_output_gives_the_contiguous_bits(pkg, layout, family):
    c = lc.build_case(layout, family, "physical")
    g = _dev(c)
    x, ei, ea, st, out, _ = g
    loss, grad, flows, o_after = _run(pkg, g)
    loss_s, grad_s, flows_s, o_s = _run(pkg, g, stride4=True)
    assert o_s.stride() == (4, 1)
    assert torch.equal(loss, loss_s) and torch.equal(grad, grad_s) and torch.equal(flows, flows_s) and torch.equal(o_after, o_s)
    gaps = torch.as_strided(o_s, (c.N - 1, 2), (4, 1), 2)
    assert (gaps == SENTINEL).all()
    # a real two-column view of an [N, 4] tensor (no gradient: autograd does not let a two-output function modify a view in place)
    buf = torch.full((c.N, 4), SENTINEL, device=DEV)
    buf[:, 1:3] = out
    with torch.no_grad():
        loss_v = _loss(pkg, x, ei, ea, st, buf[:, 1:3])
    assert torch.equal(loss_v, loss) and torch.equal(buf[:, 1:3], o_after)
    assert (buf[:, 0] == SENTINEL).all() and (buf[:, 3] == SENTINEL).all()


@pytest.mark.parametrize("layout", ["n257_iso", "n257_hub", "straddle", "big"])
def test_fused_finish_and_two_launch_finish_agree_bitwise(pkg, layout):
    """flags.WLS_FUSED_FINISH on, against both finish flags off (up to 16 workgroups WLS_FUSED_FINISH_SMALL alone already fuses, so
    switching only the first would compare the fused finish with itself on the small layouts)."""
    c = lc.build_case(layout, "ober_sub", "physical")
    g = _dev(c)
    keep = pkg.flags.WLS_FUSED_FINISH, pkg.flags.WLS_FUSED_FINISH_SMALL
    try:
        pkg.flags.WLS_FUSED_FINISH, pkg.flags.WLS_FUSED_FINISH_SMALL = True, True
        fused = _run(pkg, g)
        pkg.flags.WLS_FUSED_FINISH, pkg.flags.WLS_FUSED_FINISH_SMALL = False, False
        plain = _run(pkg, g)
        pkg.flags.WLS_FUSED_FINISH, pkg.flags.WLS_FUSED_FINISH_SMALL = False, True
        default = _run(pkg, g)
    finally:
        pkg.flags.WLS_FUSED_FINISH, pkg.flags.WLS_FUSED_FINISH_SMALL = keep
    for a, b, d in zip(fused, plain, default):
        assert torch.equal(a, b) and torch.equal(a, d)


# ------------------------------------------------------------------------------------------------ get_pflow
def _pflow_case(family, E):
    """A path of E branches (every fifth a transformer, the first included), or the `big` layout for E = None."""
    if E is None:
        c = lc.build_case("big", family, "physical")
        x, ei, ea, st, out, y = lc.tensors(c, torch.float64)
        return x, ei, ea, y
    comp = lc.Component(f"PF{E}", E + 1, [(k, k + 1) if k % 3 else (k + 1, k) for k in range(E)], trafos=set(range(0, E, 5)))
    x, ea, _, y = lc.component_data(comp, family, "physical")
    return x.clone(), torch.tensor(comp.edges, dtype=torch.int64).t().contiguous(), ea.clone(), y.clone()


def _flow_budget(y, ei, node_param, edge_param, phase_shift):
    """[E, 8] fp64: for each of get_pflow's quantities the sum of the magnitudes of the terms it is formed from.  P and Q are
    differences of nearly equal terms (at a transformer of the grids sum |terms| / |Q_from| is 600), so an fp32 evaluation -- any
    one, the oracle's as much as the kernel's -- is off by a few 2^-24 of THIS, not of the value; the currents and loadings inherit it
    (hypot is 1-Lipschitz in each argument, the rest are positive factors)."""
    vhv, vlv = node_param[:, 0].max(), node_param[:, 0].min()
    vi, vj, d = y[ei[0], 0], y[ei[1], 0], y[ei[0], 1] - y[ei[1], 1]
    G, B, Gs, Bs, imax = (edge_param[:, k] for k in (0, 1, 2, 3, 6))
    tp = torch.ceil(edge_param[:, 5])
    if not phase_shift:
        d = d - edge_param[:, 5]
    c, s_, kk = torch.cos(d).abs(), torch.sin(d).abs(), vlv ** 2
    cross = vi * vj * (G.abs() * c + B.abs() * s_)
    crossq = vi * vj * (G.abs() * s_ + B.abs() * c)
    bpf, bqf = (cross + (G + Gs / 2).abs() * vi ** 2) * kk, (crossq + (B + Bs / 2).abs() * vi ** 2) * kk
    bpt, bqt = (cross + (G + Gs / 2).abs() * vj ** 2) * kk, (crossq + (B + Bs / 2).abs() * vj ** 2) * kk
    bif = (bpf + bqf) / (vi * vlv * 3 ** 0.5) / (1.0 - tp * (1.0 - vhv / vlv)).abs()
    bit = (bpt + bqt) / (vj * vlv * 3 ** 0.5)
    bll = (1.0 - tp).abs() * torch.maximum(bif, bit) / imax
    blt = tp * torch.maximum(bif * vhv, bit * vlv) / imax
    return torch.stack([bll, blt, bpf, bqf, bpt, bqt, bif, bit], 1)


ROUNDINGS = 8      # fp32 roundings on the way to a flow: the angle difference, sincosf (2 ulp), two products and a sum per bracket, the square, the scale


@pytest.mark.parametrize("E", [1, 256, 257, None], ids=["E1", "E256", "E257", "big"])
@pytest.mark.parametrize("family", list(lc.FAMILIES))
def test_get_pflow_both_phase_shift_senses(pkg, family, E):
    x, ei, ea, y = _pflow_case(family, E)
    assert (torch.ceil(ea[:, 11]) > 0).any() and x[:, 8].min() < x[:, 8].max()
    xd, eid, ead, yd = x.float().to(DEV), ei.to(DEV), ea.float().to(DEV), y.float().to(DEV)
    errs, bounds, got = {}, {}, {}
    for ps in (True, False):
        got[ps] = torch.stack(pkg.data.get_pflow(yd, eid, xd[:, 8:], ead[:, 6:], phase_shift=ps), 1)
        r64 = torch.stack(oracle.get_pflow(y, ei, x[:, 8:], ea[:, 6:], phase_shift=ps), 1)
        r32 = torch.stack(oracle.get_pflow(y.float(), ei, x[:, 8:].float(), ea[:, 6:].float(), phase_shift=ps), 1)
        bud = _flow_budget(y, ei, x[:, 8:], ea[:, 6:], ps)
        assert got[ps].shape == (ei.shape[1], 8) and torch.isfinite(got[ps]).all()
        for k in range(8):
            errs[f"{'shift0' if ps else 'shifted'}.{k}"] = lc.max_rel(got[ps][:, k], r64[:, k])
            # (max over the column: with E = 1 the fp32 oracle's error is ONE sample of the rounding noise, so the budget is part of the bound)
            budget = ROUNDINGS * 2.0 ** -24 * bud[:, k].max().item() / max(r64[:, k].abs().max().item(), 1e-300)
            bounds[f"{'shift0' if ps else 'shifted'}.{k}"] = max(lc.bound(lc.max_rel(r32[:, k], r64[:, k])), budget if r64[:, k].abs().max() > 0 else 0.0)
    _record("get_pflow", f"{family}-{'big' if E is None else E}", errs, bounds)
    for k in bounds:
        assert errs[k] <= bounds[k], (k, errs[k], bounds[k])
    trafo = (torch.ceil(ea[:, 11]) > 0).to(DEV)       # the two senses differ at the transformers and only there
    assert torch.equal(got[True][~trafo], got[False][~trafo])
    assert (got[True][trafo][:, 2] != got[False][trafo][:, 2]).all()


# ------------------------------------------------------------------------------------------------ eval_batch
@pytest.mark.parametrize("layout", ["one_wg", "iso_heavy", "big"])
@pytest.mark.parametrize("family", list(lc.FAMILIES))
def test_eval_batch_metrics(pkg, family, layout):
    c = lc.build_case(layout, family, "physical")
    x, ei, ea, st, out, y = _dev(c)
    x64, ei64, ea64, st64, out64, y64 = lc.tensors(c, torch.float64)
    m64, yh64 = oracle.eval_batch_metrics(out64, y64, x64, ei64, ea64, st64[0], st64[1])
    m32, _ = oracle.eval_batch_metrics(out64.float(), y64.float(), x64.float(), ei64, ea64.float(), st64[0].float(), st64[1].float())
    # what the selections hold: ceil(shift) = 3 makes a transformer's LINE loading (1 - 3) max(I) / imax, negative and non-zero
    t_lines, t_trafos = oracle.get_pflow(y64, ei64, x64[:, 8:], ea64[:, 6:])[:2]
    trafo = torch.ceil(ea64[:, 11]) > 0
    assert trafo.any() and (t_trafos[trafo] != 0).all() and (t_lines[~trafo] != 0).all()
    if family == "ober_sub":
        assert (t_lines[trafo] < 0).all()
    else:
        assert (t_lines[trafo] == 0).all()
    acc = torch.zeros(10, dtype=torch.float64, device=DEV)
    yhat = pkg.data.eval_batch(out, y, x, ei, ea, st[0], st[1], acc)
    once = acc.clone()
    assert torch.allclose(yhat.cpu().double(), yh64, rtol=1e-6, atol=1e-7)
    got = dict(zip(pkg.data.EVAL_METRICS, once.cpu().tolist()))
    errs = {k: abs(got[k] - m64[k]) / abs(m64[k]) for k in m64}
    bounds = {k: max(2e-5, 4.0 * abs(m32[k] - m64[k]) / abs(m64[k])) for k in m64}
    _record("eval", f"{layout}-{family}", errs, bounds)
    for k in m64:
        assert errs[k] <= bounds[k], (k, got[k], m64[k])
    yhat2 = pkg.data.eval_batch(out, y, x, ei, ea, st[0], st[1], acc)       # a second batch into the same accumulator
    assert torch.equal(acc, 2.0 * once) and torch.equal(yhat2, yhat)


# ------------------------------------------------------------------------------------------------ the V_hv / V_lv cache
def test_vminmax_cache_follows_the_tensor(pkg):
    c = lc.build_case("one_wg", "cigre14", "physical")
    x, ei, ea, st, out, y = lc.tensors(c, torch.float32, DEV)       # fresh tensors: cache entries of this test's own
    vlv, vhv = x[:, 8].min().item(), x[:, 8].max().item()

    def run():
        o = out.clone()
        flows = torch.empty(c.E, 8, device=DEV)
        return _loss(pkg, x, ei, ea, st, o, pflow_out=flows).item(), o, flows

    def check(loss, o, flows, x_now):
        c2 = copy.copy(c)
        c2.x = x_now.detach().cpu().double()
        r64, r32 = lc.referee(c2, torch.float64, o, flows), lc.referee(c2, torch.float32, o, flows)
        assert abs(loss - r64.loss) <= lc.bound(abs(r32.loss - r64.loss) / abs(r64.loss)) * abs(r64.loss), (loss, r64.loss)
        for k in range(8):
            assert lc.max_rel(flows[:, k], r64.flows[:, k]) <= lc.bound(lc.max_rel(r32.flows[:, k], r64.flows[:, k])), k
        return r64.loss

    first = run()
    ref1 = check(*first, x)
    assert run()[0] == first[0]                                       # (a cache hit)
    x[:, 8] = torch.where(x[:, 8] == vlv, 0.5 * vlv, x[:, 8])        # through torch: the version counter moves
    second = run()
    ref2 = check(*second, x)
    assert abs(ref2 - ref1) > 1e-2 * abs(ref1)                        # (the change is one a stale cache could not hide)
    new = x.clone()                                                   # (the LOW level again: with transformer flag 1 V_hv cancels out of the loading)
    new[:, 8] = torch.where(x[:, 8] == 0.5 * vlv, 0.25 * vlv, x[:, 8])
    version = x._version
    x.data.copy_(new)                                                 # a raw write: same tensor, same version
    assert x._version == version and x[:, 8].min().item() == 0.25 * vlv
    stale = run()
    assert stale[0] == second[0]                                      # the documented contract: torch's counter saw nothing ...
    pkg.data.invalidate_vminmax(x)                                    # ... and this is what such writers call
    third = run()
    ref3 = check(*third, x)
    assert abs(ref3 - ref2) > 1e-2 * abs(ref2)


# ------------------------------------------------------------------------------------------------ refusals, all on the host
def test_refusals_before_any_launch(pkg):
    c = lc.build_case("one_wg", "cigre14", "wild")
    x, ei, ea, st, out, y = _dev(c)
    N, E = c.N, c.E
    o = out.clone()
    bad_outputs = [torch.zeros(N, 3, device=DEV), torch.zeros(N, 4, device=DEV)[:, ::2], torch.zeros(N, device=DEV)]
    for bo in bad_outputs:
        with pytest.raises(ValueError, match="output must be"):
            _loss(pkg, x, ei, ea, st, bo)
        assert (bo == 0).all()
    for bad in (torch.empty(E, 7, device=DEV), torch.empty(E, 8, device=DEV, dtype=torch.float64), torch.empty(E, 8),
                torch.empty(E, 16, device=DEV)[:, ::2]):
        with pytest.raises(ValueError, match="pflow_out must be"):
            _loss(pkg, x, ei, ea, st, o, pflow_out=bad)
    for bad in (torch.ones(1, dtype=torch.int64, device=DEV), torch.ones(2, dtype=torch.int32, device=DEV), torch.ones(1, dtype=torch.int32)):
        with pytest.raises(ValueError, match="edge_count must be"):
            _loss(pkg, x, ei, ea, st, o, edge_count=bad)
    for k in ("lam_v", "lam_p", "lam_pf", "lam_reg"):
        reg = {q: v for q, v in lc.REG.items() if q != k}
        with pytest.raises(KeyError, match=k):
            pkg.data.gsp_wls_edge(input=x[:, :8], edge_input=ea[:, :6], output=o, x_mean=st[0], x_std=st[1], edge_mean=st[2],
                                  edge_std=st[3], edge_index=ei, reg_coefs=reg, num_samples=None, node_param=x[:, 8:], edge_param=ea[:, 6:])
    assert torch.equal(o, out)                                        # nothing ran: theta is not masked
    for bad in (torch.zeros(10, device=DEV), torch.zeros(9, dtype=torch.float64, device=DEV)):
        with pytest.raises(ValueError, match="acc must be"):
            pkg.data.eval_batch(out, y, x, ei, ea, st[0], st[1], bad)
        assert (bad == 0).all()
    # through the ABI: the size checks come first, so null operands are never looked at
    L, lib = pkg._lib.lib(), pkg._lib
    stream = lib.stream_ptr(torch.device(DEV))
    for n in (0, -1):
        a = lib.WlsArgs()
        a.n_nodes, a.n_edges = n, 5
        assert L.dss2_wls_loss_partials(C.byref(a), stream) == 2 and L.dss2_last_error().decode() == "wls_loss: empty batch"
        assert L.dss2_wls_loss_grad(C.byref(a), stream) == 2 and L.dss2_last_error().decode() == "wls_loss: empty batch"
        assert L.dss2_get_pflow(None, 2, None, 3, None, 7, None, None, n, 5, None, None, 0, stream) == 2
        assert L.dss2_last_error().decode() == "get_pflow: empty batch"
    for n in (1, 0, -1):
        assert L.dss2_eval_batch(None, 2, None, 2, None, 3, None, 7, None, None, n, 5, None, None, None, None, None, None, None, None, stream) == 2
        assert L.dss2_last_error().decode() == "eval_batch: needs at least 2 nodes and 1 edge"
    torch.cuda.synchronize()
