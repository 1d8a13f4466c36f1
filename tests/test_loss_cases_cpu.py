"""CPU: the case table of tests/loss_cases.py is what it says it is -- structure (against TopologyOracle's incidence CSR), live and
idle penalty gates, margins from every threshold, finiteness -- and the mathematics of the loss kernels holds at degree > 4: the numpy
restatement of their node-centric traversal (tests/test_kernel_math_cpu.py) reproduces the fp64 oracle on the hub graphs.  Also the
record of the reference arithmetic's own fp32 error per case, which tests/test_gpu_loss_shapes.py takes its bounds from (run with -s)."""
import collections

import numpy as np
import pytest
import torch

import loss_cases as lc
import dss2_topology_oracle as topo_oracle
from test_kernel_math_cpu import _emulate_wls

CASES = lc.case_ids()
IDS = ["-".join(c) for c in CASES]


def _rows(topo):
    rp, ent = topo.inc_rowptr.numpy(), topo.inc_ent.numpy()
    return lambda i: [(int(en) & 0x7fffffff, int(en) < 0) for en in ent[rp[i]:rp[i + 1]]]


@pytest.mark.parametrize("layout", list(lc.LAYOUTS))
def test_structure(layout):
    c = lc.build_case(layout, "cigre14", "physical")
    N, E, hist = lc.EXPECT[layout]
    assert (c.N, c.E) == (N, E)
    topo = topo_oracle.TopologyOracle(c.ei, c.N)
    deg = (topo.inc_rowptr[1:] - topo.inc_rowptr[:-1]).tolist()
    assert dict(collections.Counter(deg)) == hist
    row = _rows(topo)
    for (k, nm), bus in c.hub_bus.items():
        if nm not in lc.HUB_SPEC:
            continue
        r = row(bus)
        rounds = tuple("".join("T" if to else "F" for _, to in r[k0:k0 + lc.WLS_GB]) for k0 in range(0, len(r), lc.WLS_GB))
        assert rounds == lc.HUB_ROUNDS[nm], (nm, rounds)
        assert len(r) == lc.HUB_SPEC[nm][0] and len(rounds) == -(-len(r) // lc.WLS_GB)
        assert float(c.x[bus, 9]) == (1.0 if nm == lc.SLACK_HUB else 0.0)
        if nm in lc.TRAFO_HUBS:       # a transformer in the named later round
            k0 = lc.WLS_GB * lc.TRAFO_HUBS[nm]
            assert k0 >= lc.WLS_GB and any(torch.ceil(c.ea[e, 11]) > 0 for e, _ in r[k0:k0 + lc.WLS_GB])
    # across the hubs every round number occurs with from-end and with to-end entries, and rounds 1-3 mixed
    seen = collections.defaultdict(set)
    for rounds in lc.HUB_ROUNDS.values():
        for k, s in enumerate(rounds):
            seen[k].add("mixed" if len(set(s)) == 2 else s[0])
            seen[k] |= set(s)
    assert all({"F", "T"} <= seen[k] for k in range(4)) and all("mixed" in seen[k] for k in range(3))
    assert {len(s[-1]) for s in lc.HUB_ROUNDS.values()} == {1, 3, 4}
    # the parallel branches: two and three stored branches between one pair, one of them reversed
    pairs = collections.Counter((min(a, b), max(a, b)) for a, b in c.ei.t().tolist())
    assert {2, 3} <= set(pairs.values())
    for (a, b), n in pairs.items():
        if n > 1 and c.E < 1000:
            dirs = {(int(p), int(q)) for p, q in c.ei.t().tolist() if {p, q} == {a, b}}
            assert dirs == {(a, b), (b, a)}
            rows_ab = c.ea[[k for k, (p, q) in enumerate(c.ei.t().tolist()) if {p, q} == {a, b}]]
            assert len({tuple(r.tolist()) for r in rows_ab}) == n          # different parameters
    # branch-less buses: a slack one and an ordinary one
    iso = torch.tensor(deg) == 0
    assert set(c.x[iso, 9].tolist()) == {0.0, 1.0}
    assert c.x[:, 8].min() < c.x[:, 8].max()
    if layout == "big":
        assert c.N > 65536 and c.E > 65536 and (c.N + lc.LB - 1) // lc.LB > 16
        assert (c.x[:-1, 8] == c.x[:, 8].max()).all() and c.x[-1, 8] < c.x[0, 8]
    if layout == "straddle":
        bus = [b for (k, nm), b in c.hub_bus.items() if nm == "h13" and b == lc.LB - 1]
        assert len(bus) == 1
        others = [int(c.ei[0, e] if to else c.ei[1, e]) for e, to in row(bus[0])]
        assert sum(o >= lc.LB for o in others) >= 12 and any(o < lc.LB for o in others)
    if layout == "n256":
        assert c.N == lc.LB
    if layout == "n257_hub":
        assert deg[-1] == 5 and c.N == lc.LB + 1
    if layout == "n257_iso":
        assert deg[-1] == 0 and c.N == lc.LB + 1
    if layout == "iso_heavy":
        assert c.E < c.N
    if layout == "one_wg":
        assert c.E > c.N
    for fam in lc.FAMILIES:               # rows really are fp32 values
        cc = lc.build_case(layout, fam, "wild")
        for t_ in (cc.x, cc.ea, cc.out, cc.y):
            assert torch.equal(t_.float().double(), t_)
        assert set(torch.ceil(cc.ea[:, 11]).tolist()) == {0.0, lc.FAMILIES[fam]}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gates_and_margins(case):
    c = lc.build_case(*case)
    x, ei, ea, st, out, _ = lc.tensors(c, torch.float64)
    v, dth, load = lc._oracle_quantities(x, ea, out, st, ei)
    margins = (torch.minimum((v - 1.1).abs(), (v - 0.9).abs()).min().item(), (dth - 0.5).abs().min().item(), (load - 1.5).abs().min().item())
    assert min(margins) >= lc.MARGIN, margins
    assert load.abs().max() <= lc.LOAD_CAP * 1.05
    if c.regime != "physical":
        return
    for name, g in (("v > 1.1", v > 1.1), ("v < 0.9", v < 0.9), ("|dtheta| > 0.5", dth > 0.5), ("loading > 1.5", load > 1.5)):
        assert int(g.sum()) >= 3 and int((~g).sum()) >= 3, (name, int(g.sum()), g.numel())
    row = _rows(topo_oracle.TopologyOracle(c.ei, c.N))
    meas = (ea[:, :4] != 0).any(1)
    for (k, nm), bus in c.hub_bus.items():
        r = row(bus)
        for k0 in range(0, len(r), lc.WLS_GB):
            live = r[k0:k0 + lc.WLS_GB]
            assert any(load[e] > 1.5 for e, _ in live), (nm, k0, "no overloaded branch in this round")
            if any(not to for _, to in live):
                assert any(meas[e] for e, to in live if not to), (nm, k0, "no measured from-end branch in this round")
            assert any(meas[e] for e, _ in live)
    assert 0.25 * c.E <= int(meas.sum()) <= 0.75 * c.E


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_finite_and_fp32_record(case):
    """Loss, gradient and flows are finite in fp64 and fp32; prints the fp32 oracle's error against the fp64 one (both with the
    fp64 oracle's own max() choices), the noise scale of the GPU bounds."""
    c = lc.build_case(*case)
    fl64, om64 = lc.oracle_flows(c)
    r64 = lc.referee(c, torch.float64, om64, fl64)
    r32 = lc.referee(c, torch.float32, om64, fl64)
    for r in (r64, r32):
        assert np.isfinite(r.loss) and torch.isfinite(r.grad).all() and torch.isfinite(r.flows).all()
    assert torch.equal(r64.out_after, om64)
    err = lc.errors(r32.loss, r32.grad, r32.flows, r64, c)
    print(f"[loss-cases fp32 oracle vs fp64] {'-'.join(case)}: " + " ".join(f"{k}={v:.2e}" for k, v in err.items() if not k.startswith("_")))
    # the record is a measurement; what it must show is only that fp32 is a usable noise scale at all
    assert err["loss"] < 1e-4 and err["grad"] < 1e-2


@pytest.mark.parametrize("family", list(lc.FAMILIES))
@pytest.mark.parametrize("regime", lc.REGIMES)
def test_kernel_math_at_degree_above_four(family, regime):
    """The kernels' traversal (rounds of a bus's incidence row, both orientations, the from-end's edge term) restated in numpy gives
    the oracle's loss and gradient on the hub graphs at the bounds of tests/test_kernel_math_cpu.py."""
    c = lc.build_case("one_wg", family, regime)
    x, ei, ea, st, out, _ = lc.tensors(c, torch.float64)
    topo = topo_oracle.TopologyOracle(ei, c.N)
    loss, grad, out_after, _ = _emulate_wls(topo, x, ea, out, st, lc.REG)
    leaf = out.clone().requires_grad_(True)
    o = leaf * 1.0
    ref = lc.referee_loss(x, ea, o, st, ei)
    ref.backward()
    assert abs(loss - ref.item()) <= 1e-10 * abs(ref.item())
    np.testing.assert_allclose(out_after, o.detach().numpy(), rtol=0, atol=1e-12)
    gref = leaf.grad.numpy()
    assert np.abs(grad - gref).max() <= 1e-9 * np.abs(gref).max()
    # ... and graph by graph, so that the hub graph's large entries do not stand in for a branch-less bus
    pg = lc.per_graph_rel(torch.from_numpy(grad), leaf.grad, c.graph, c.n_graphs)
    assert pg.max() <= 1e-9, pg
