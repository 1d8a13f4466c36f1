"""GPU: the WLS estimators on batches that MIX bus counts (graph_ptr; nodes_per_graph an upper bound), csrc/dss2_wls_core.hpp's ws_range
in every kernel body, against the per-graph fp64 oracle of tests/wls_mixed_cases.py (every graph solved alone with the batch's V_lv).

Batches (tests/wls_mixed_cases.py): A (bound 33: the four-wave LDS kernel around two-bus and one-bus graphs), B (bound 99: the LDS cap),
C (bound 179, blocked), D (bound 256, the blocked cap), cigre14 + ober_sub and ober_sub + ober179 from synthetic.make_batch; 3 .. 7 graphs.

Bounds, none taken from the kernel (tests/test_wls_mixed_cpu.py measures the oracle's spreads and holds the literals to them): state 5e-7
and objective 1e-6 relative, but on ober_sub + ober179, whose ober179 graph has the oracle's own two summation orders 7.3e-8 apart after
three iterations (8 x that: 5.8e-7) and its objective 2.6e-7 relative apart after one (2.1e-6).  Iterations and status equal the oracle's; at
tol = 1e-6 every decision on A, B and C is compared, none left out (no graph decides within a factor 4 of the tolerance).  The objective
of a one-bus graph is 0 in the oracle (below 1e-20): there the kernel's is held to 1e-12 absolute instead of a relative error.
The robust and bad-data mixes carry one 25 sigma error per graph from synthetic.corrupt_measurements (through graph_ptr; global ids) and
are held to the bounds of tests/test_gpu_wls_robust.py (state 5e-7, q 1e-9 at 8 iterations, objective 1e-6) and
tests/test_gpu_wls_bad_data.py (S 2e-7, rN 1e-4, state_std 3.4e-9, state 5e-7).

Measured on the MI355X (bound in brackets): state 5.96e-8 at worst on A, B, C, D and cigre14 + ober_sub (the fp32 rounding of the output)
[5e-7], objective 2.0e-9 relative (B after one iteration) [1e-6], the one-bus graphs' objective exactly 0; ober_sub + ober179 state
6.0e-8 / 8.5e-8 / 5.9e-8 after 1 / 3 / 8 iterations [5e-7 / 5.8e-7 / 5e-7], objective 1.2e-7 after one [2.1e-6]; iterations, status and
every decision equal to the oracle's.  Robust mixes: state 5.95e-8, q 1.5e-13 [1e-9], objective 8.2e-12; the bad-data mix: removed ids the
oracle's (four of the five injected errors: the fifth sits on a measurement whose rN stays below the threshold), removed_rn 3.2e-11
[1e-4], S 5.7e-10 [2e-7], rN 6.3e-9 [1e-4], state_std 2.7e-12 [3.4e-9].

What must hold to the bit: a uniform batch through graph_ptr = arange(G + 1) n against the same call without it, every field, all four
entries; the graphs of A and of C in reversed order and with max_groups 1, 2 and the default (what a workgroup leaves in LDS or in its
workspace slice when a small graph follows a large one, and the other way round); a graph of A alone; the healthy graphs behind a
failing one, beside refused ones (bound 32: the two n33 graphs end with status 2 and untouched rows), beside an empty one; a hipGraph
and a launch-plan replay.  Every test prints its figures beside the bounds (-s).
"""
import functools
import importlib
import math

import numpy as np
import pytest
import torch

import wls_edge_cases as ec
import wls_large_cases as lc
import wls_mixed_cases as mc
import wls_oracle as wo
import wls_robust_oracle as ro
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Q_BOUND, SENS_BOUND, RN_BOUND, STD_BOUND, S_MIN = 1e-9, 2e-7, 1e-4, 8 * 4.3e-10, 1e-3
ZERO_OBJECTIVE = 1e-12
FIELDS = ("state", "objective", "iterations", "status", "last_step")
PER_GRAPH_ROBUST, PER_GRAPH_BAD_DATA = ("n_downweighted",), ("dof", "chi2_limit", "suspect", "removed", "removed_rn", "n_removed")
LDS_ENTRY, LARGE_ENTRY = "wls_estimate", "wls_estimate_large"
# (batch, entry): A and B through both, the grid mixes through their own
PARITY = [("A", LDS_ENTRY), ("B", LDS_ENTRY), ("cigre_ober", LDS_ENTRY), ("A", LARGE_ENTRY), ("B", LARGE_ENTRY), ("C", LARGE_ENTRY),
          ("D", LARGE_ENTRY), ("ober_ober179", LARGE_ENTRY)]


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module(PKG_NAME)
    p._lib.lib()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return p


def _to_device(b):
    return {k: (tuple(s.to(DEV) for s in v) if k == "stats" else (v.to(DEV) if torch.is_tensor(v) else v)) for k, v in b.items()}


@functools.lru_cache(maxsize=None)
def _device(name):
    return _to_device(mc.batch(name))


def _run(pkg, b, entry=LDS_ENTRY, bound=None, graph_ptr="own", **kw):
    if graph_ptr == "own":
        graph_ptr = b["graph_ptr"]
    return getattr(pkg.estimator, entry)(b["x"], b["edge_index"], b["edge_attr"], *b["stats"], b["nodes_per_graph"] if bound is None else bound,
                                         graph_ptr=graph_ptr, **kw)


def _equal(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


def _per_graph(res, b, g, per_graph=()):
    """Everything a result says about graph g: its state rows and its entries of the per-graph fields."""
    rows, _ = mc.graph_rows(b, g)
    return [res.state[rows]] + [getattr(res, f)[g] for f in FIELDS[1:] + tuple(per_graph)]


def _same_graph(p, q):
    return all(torch.equal(s, t) for s, t in zip(p, q))


def _errors(res, ref):
    st = (res.state.cpu().double() - ref["state"]).abs().max().item()
    got, want = res.objective.cpu(), ref["objective"]
    live = want.abs() > ZERO_OBJECTIVE
    ob = ((got - want).abs() / want.abs())[live].max().item()
    dead = got[~live].abs().max().item() if bool((~live).any()) else 0.0
    return st, ob, dead


# ---- 1. against the per-graph oracle

@pytest.mark.parametrize("max_iter", mc.TRIP_COUNTS)
@pytest.mark.parametrize("name,entry", PARITY)
def test_parity_at_fixed_trip_counts(pkg, name, entry, max_iter):
    sb, ob_bound = mc.state_bound(name, max_iter), mc.objective_bound(name, max_iter)
    ref, b = mc.oracle(name, max_iter, 0.0), _device(name)
    res = _run(pkg, b, entry, max_iter=max_iter, tol=0.0)
    st, ob, dead = _errors(res, ref)
    print(f"[wls mixed parity] {name} {entry} max_iter={max_iter} sizes {b['sizes']}: state {st:.2e}/{sb:.1e} objective {ob:.2e}/{ob_bound:.1e} "
          f"(zero objectives {dead:.1e}/{ZERO_OBJECTIVE:.0e}) iterations {res.iterations.tolist()} status {res.status.tolist()}")
    G = b["num_graphs"]
    assert res.state.shape == (b["x"].shape[0], 2) and res.objective.shape == (G, 2) and res.iterations.shape == (G,) and res.status.shape == (G,)
    assert torch.equal(res.iterations.cpu(), ref["iterations"]) and torch.equal(res.status.cpu(), ref["status"])
    assert bool((res.status == 1).all()) and bool((res.iterations == max_iter).all())
    assert st <= sb, (st, sb)
    assert ob <= ob_bound and dead <= ZERO_OBJECTIVE, (ob, ob_bound, dead)


@pytest.mark.parametrize("name,entry", [(n, e) for n, e in PARITY if n in mc.DECIDED])
def test_every_convergence_decision_matches_the_oracle(pkg, name, entry):
    ref, b = mc.oracle(name, 12, mc.TOL), _device(name)
    res = _run(pkg, b, entry, max_iter=12, tol=mc.TOL)
    st = (res.state.cpu().double() - ref["state"]).abs().max().item()
    print(f"[wls mixed convergence] {name} {entry}: iterations {res.iterations.tolist()} oracle {ref['iterations'].tolist()} status {res.status.tolist()} "
          f"last_step {['%.1e' % v for v in res.last_step.tolist()]} state {st:.2e}/{mc.STATE_BOUND:.0e}")
    assert not bool(wo.undecided(ref, mc.TOL).any())
    assert torch.equal(res.status.cpu(), ref["status"]) and torch.equal(res.iterations.cpu(), ref["iterations"]) and bool((res.status == 0).all())
    assert st <= mc.STATE_BOUND


# ---- 2. uniform batches through graph_ptr: the same bits

def _uniform_ptr(b):
    n = b["nodes_per_graph"]
    return torch.arange(b["x"].shape[0] // n + 1, dtype=torch.int64, device=DEV) * n


@pytest.mark.parametrize("name,entry", [("cigre14", LDS_ENTRY), ("n33", LDS_ENTRY), ("n100", LARGE_ENTRY)])
def test_a_uniform_batch_through_graph_ptr_is_the_plain_call_to_the_bit(pkg, name, entry):
    b = _to_device(lc.batch(name))
    for kw in (dict(max_iter=1, tol=0.0), dict(max_iter=8, tol=0.0), dict(max_iter=12, tol=mc.TOL)):
        plain = _run(pkg, b, entry, graph_ptr=None, **kw)
        for groups in (0, 1, 2):
            res = _run(pkg, b, entry, graph_ptr=_uniform_ptr(b), max_groups=groups, **kw)
            assert _equal(res, plain), (name, entry, kw, groups)


def test_uniform_robust_and_bad_data_through_graph_ptr_to_the_bit(pkg):
    b = _to_device(ro.corrupted("cigre14")[0])              # one error of 25 sigma per graph
    ptr = _uniform_ptr(b)
    kw = dict(max_iter=8, tol=0.0)
    plain = _run(pkg, b, "wls_robust", graph_ptr=None, gamma=3.0, **kw)
    res = _run(pkg, b, "wls_robust", graph_ptr=ptr, gamma=3.0, **kw)
    assert int(plain.n_downweighted.sum()) >= 5 and _equal(res, plain) and len(res) == 8
    plain = _run(pkg, b, "wls_bad_data", graph_ptr=None, threshold=4.0, max_removals=1, **kw)
    res = _run(pkg, b, "wls_bad_data", graph_ptr=ptr, threshold=4.0, max_removals=1, **kw)
    assert plain.n_removed.tolist() == [1] * 5 and len(res) == 16
    for f, p, q in zip(res._fields, res, plain):
        assert torch.equal(p, q), f


# ---- 3. independence of neighbours

@pytest.mark.parametrize("name,entry", [("A", LDS_ENTRY), ("A", LARGE_ENTRY), ("C", LARGE_ENTRY)])
def test_order_and_group_count_do_not_change_a_graphs_bits(pkg, name, entry):
    hb = mc.batch(name)
    b = _device(name)
    G = hb["num_graphs"]
    kw = dict(max_iter=6, tol=mc.TOL)
    base = _run(pkg, b, entry, **kw)
    assert bool((base.status == 0).all())
    order = list(range(G))[::-1]
    back = _to_device(mc.reordered(hb, order))
    for batch, where in ((b, list(range(G))), (back, order)):
        for groups in (1, 2, 0):
            res = _run(pkg, batch, entry, max_groups=groups, **kw)
            for pos, g in enumerate(where):
                assert _same_graph(_per_graph(res, batch, pos), _per_graph(base, b, g)), (name, entry, groups, pos, g)


def test_a_graph_of_a_mix_is_the_graph_alone_to_the_bit(pkg):
    hb, b = mc.batch("A"), _device("A")
    kw = dict(max_iter=6, tol=mc.TOL)
    base = _run(pkg, b, **kw)
    for g in range(hb["num_graphs"]):
        alone = _to_device(mc.reordered(hb, [g]))
        res = _run(pkg, alone, bound=33, **kw)               # the same workgroup width: the bound is 33 here too
        assert res.objective.shape == (1, 2) and _same_graph(_per_graph(res, alone, 0), _per_graph(base, b, g)), g


# ---- 4. a failing graph in front

def test_a_failing_graph_in_front_fails_alone(pkg):
    failing = ec._graph("isolated", ec.IDS["isolated"][ec.FAILING_GRAPH], ec.FAILING_GRAPH)     # its theta_3 pivot is exactly 0
    hb = mc.collate([failing] + [mc.shape_graph(name, k) for name, k in mc.BATCHES["A"]])
    long, b = _to_device(hb), _device("A")
    kw = dict(max_iter=10, tol=mc.TOL)
    base = _run(pkg, b, **kw)
    for entry in (LDS_ENTRY, LARGE_ENTRY):
        ref = _run(pkg, b, entry, **kw)
        res = _run(pkg, long, entry, max_groups=1, **kw)
        print(f"[wls mixed failing] {entry}: status {res.status.tolist()} iterations {res.iterations.tolist()}")
        assert int(res.status[0]) == 2 and int(res.iterations[0]) == 0 and float(res.last_step[0]) == 0.0
        assert torch.equal(res.state[:6], torch.tensor([1.0, 0.0], device=DEV).expand(6, 2))       # a factorisation that failed: the start
        for g in range(b["num_graphs"]):
            assert _same_graph(_per_graph(res, long, g + 1), _per_graph(ref, b, g)), (entry, g)
        assert bool(torch.isfinite(res.objective).all())
    assert bool((base.status == 0).all())


# ---- 5. the guard: a refusal path (ws_range refuses the graph before anything of it touches LDS or memory), not an overrun

def test_graphs_above_the_bound_are_refused_alone(pkg):
    hb, b = mc.batch("A"), _device("A")
    kw = dict(max_iter=6, tol=mc.TOL)
    for entry in (LDS_ENTRY, LARGE_ENTRY):
        full = _run(pkg, b, entry, **kw)
        res = _run(pkg, b, entry, bound=32, **kw)            # (the LDS entry: the one-wave kernel now, LDS for 32 buses)
        print(f"[wls mixed guard] {entry} bound 32: status {res.status.tolist()} iterations {res.iterations.tolist()}")
        for g, n in enumerate(hb["sizes"]):
            rows, _ = mc.graph_rows(hb, g)
            if n == 33:
                assert int(res.status[g]) == 2 and int(res.iterations[g]) == 0 and float(res.last_step[g]) == 0.0
                assert bool((res.objective[g] == 0).all()) and bool((res.state[rows] == 0).all())
            else:
                assert _same_graph(_per_graph(res, b, g), _per_graph(full, b, g)), (entry, g)
    # the blocked kernel with a bound below its largest graph: C at 128 refuses n179t alone
    c = _device("C")
    full, res = _run(pkg, c, LARGE_ENTRY, **kw), _run(pkg, c, LARGE_ENTRY, bound=128, **kw)
    assert res.status.tolist() == [2 if n > 128 else 0 for n in c["sizes"]]
    for g, n in enumerate(c["sizes"]):
        if n <= 128:
            assert _same_graph(_per_graph(res, c, g), _per_graph(full, c, g)), g
    rows, _ = mc.graph_rows(c, c["sizes"].index(179))
    assert bool((res.state[rows] == 0).all())


def test_an_empty_graph_and_a_pointer_outside_the_batch_are_refused_alone(pkg):
    hb, b = mc.batch("A"), _device("A")
    kw = dict(max_iter=6, tol=mc.TOL)
    full = _run(pkg, b, **kw)
    ptr = hb["graph_ptr"].tolist()
    empty = torch.tensor(ptr[:3] + [ptr[3]] + ptr[3:], dtype=torch.int64, device=DEV)           # graph 3 owns no row
    res = _run(pkg, b, graph_ptr=empty, **kw)
    assert res.status.tolist() == [0, 0, 0, 2, 0, 0, 0, 0] and int(res.iterations[3]) == 0 and bool((res.objective[3] == 0).all())
    for g in range(hb["num_graphs"]):
        pos = g if g < 3 else g + 1
        assert torch.equal(res.state, full.state) and all(torch.equal(getattr(res, f)[pos], getattr(full, f)[g]) for f in FIELDS[1:]), g
    # a last offset beyond N, a negative first one: those graphs alone
    N = hb["x"].shape[0]
    beyond = torch.tensor(ptr[:-1] + [N + 1], dtype=torch.int64, device=DEV)
    res = _run(pkg, b, graph_ptr=beyond, **kw)
    assert res.status.tolist() == [0] * 6 + [2] and all(_same_graph(_per_graph(res, b, g), _per_graph(full, b, g)) for g in range(6))
    negative = torch.tensor([-1] + ptr[1:], dtype=torch.int64, device=DEV)
    res = _run(pkg, b, graph_ptr=negative, **kw)
    assert res.status.tolist() == [2] + [0] * 6 and all(_same_graph(_per_graph(res, b, g), _per_graph(full, b, g)) for g in range(1, 7))
    assert bool((res.state[:2] == 0).all())


def test_refused_graphs_of_the_robust_and_the_bad_data_entries(pkg):
    kw = dict(max_iter=8, tol=0.0)
    b = _to_device(mc.corrupted("R_lds")[0])                 # sizes 2, 33, 10, 6, 64
    full, res = _run(pkg, b, "wls_robust", **kw), _run(pkg, b, "wls_robust", bound=33, **kw)
    rows, erows = mc.graph_rows(b, 4)
    assert res.status.tolist() == [1, 1, 1, 1, 2] and int(res.n_downweighted[4]) == 0 and int(res.iterations[4]) == 0
    assert bool((res.state[rows] == 0).all()) and bool((res.bus_q[rows] == 1).all()) and bool((res.edge_q[erows] == 1).all())
    for g in range(4):
        assert _same_graph(_per_graph(res, b, g, PER_GRAPH_ROBUST), _per_graph(full, b, g, PER_GRAPH_ROBUST)), g
        r, e = mc.graph_rows(b, g)
        assert torch.equal(res.bus_q[r], full.bus_q[r]) and torch.equal(res.edge_q[e], full.edge_q[e])
    b = _to_device(mc.corrupted("BD")[0])                    # sizes 10, 33, 2, 64, 6
    more = dict(threshold=4.0, max_removals=2, **kw)
    full, res = _run(pkg, b, "wls_bad_data", **more), _run(pkg, b, "wls_bad_data", bound=33, **more)
    rows, erows = mc.graph_rows(b, 3)
    assert res.status.tolist() == [1, 1, 1, 2, 1] and int(res.iterations[3]) == 0 and bool((res.objective[3] == 0).all())
    assert int(res.dof[3]) == 0 and math.isinf(float(res.chi2_limit[3])) and int(res.suspect[3]) == 0 and int(res.n_removed[3]) == 0
    assert res.removed[3].tolist() == [-1, -1] and res.removed_rn[3].tolist() == [0.0, 0.0]
    for t in (res.state, res.bus_rn, res.bus_sens, res.state_std):
        assert bool((t[rows] == 0).all())
    assert bool((res.edge_rn[erows] == 0).all()) and bool((res.edge_sens[erows] == 0).all())
    for g in (0, 1, 2, 4):
        assert _same_graph(_per_graph(res, b, g, PER_GRAPH_BAD_DATA), _per_graph(full, b, g, PER_GRAPH_BAD_DATA)), g
        r, e = mc.graph_rows(b, g)
        assert torch.equal(res.bus_rn[r], full.bus_rn[r]) and torch.equal(res.edge_sens[e], full.edge_sens[e]) and torch.equal(res.state_std[r], full.state_std[r])


def test_refusals_on_the_host(pkg):
    b = _device("A")
    for bad, what in ((b["graph_ptr"].int(), "int32"), (b["graph_ptr"][:1], "one element"), (b["graph_ptr"].reshape(2, 4), "2-D"),
                      (torch.cat([b["graph_ptr"], b["graph_ptr"]])[::2], "strided")):
        with pytest.raises(ValueError, match="graph_ptr must be"):
            _run(pkg, b, graph_ptr=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _run(pkg, b, graph_ptr=b["graph_ptr"].cpu())
    with pytest.raises(ValueError, match="bound"):
        _run(pkg, b, bound=0)
    # every size refusal goes by the bound
    with pytest.raises(NotImplementedError, match="at most 99 buses per graph, got 100"):
        _run(pkg, b, "wls_bad_data", bound=100)
    with pytest.raises(NotImplementedError, match="at most 99 buses per graph, got 100"):
        _run(pkg, b, LDS_ENTRY, bound=100)
    with pytest.raises(NotImplementedError, match="at most 256 buses per graph, got 257"):
        _run(pkg, b, LARGE_ENTRY, bound=257)
    # N need not be a multiple of the bound (A has 86 rows), and wls_robust routes by it
    res = _run(pkg, b, "wls_robust", bound=40, max_iter=3, tol=0.0)
    big = _run(pkg, b, "wls_robust", bound=100, max_iter=3, tol=0.0)
    assert b["x"].shape[0] % 40 != 0 and bool((res.status == 1).all()) and torch.equal(res.iterations, big.iterations)
    assert (res.state.double() - big.state.double()).abs().max().item() <= 1.2e-7       # (the LDS and the blocked form round one solution)
    # through the ABI: a graph_ptr with n_graphs = 0 is rc 2 before any launch
    import ctypes as C
    L, lib = pkg._lib.lib(), pkg._lib
    a = lib.WlsSolveArgs()
    a.n_nodes, a.n_edges, a.nodes_per_graph, a.max_iter, a.tol = 86, 80, 33, 5, 1e-6
    a.graph_ptr, a.n_graphs = b["graph_ptr"].data_ptr(), 0
    assert L.dss2_wls_solve(C.byref(a), lib.stream_ptr(torch.device(DEV))) == 2 and b"n_graphs" in L.dss2_last_error()
    a.n_graphs = 7
    assert L.dss2_wls_large_groups(C.byref(a)) == 7
    a.max_groups = 3
    assert L.dss2_wls_large_groups(C.byref(a)) == 3
    torch.cuda.synchronize()


# ---- 6. the robust and the bad-data entries on a mix, against their oracles per graph

@pytest.mark.parametrize("name,large", [("R_lds", False), ("R_blocked", True)])
def test_robust_on_a_mix_matches_the_oracle(pkg, name, large):
    hb, ids = mc.corrupted(name)
    ref = mc.robust_oracle(name, 8, 0.0)
    b = _to_device(hb)
    assert (hb["nodes_per_graph"] > pkg.estimator.max_nodes_per_graph()) == large          # large=None routes by the bound
    res = _run(pkg, b, "wls_robust", max_iter=8, tol=0.0, gamma=ro.GAMMA)
    forced = _run(pkg, b, "wls_robust", max_iter=8, tol=0.0, gamma=ro.GAMMA, large=large)
    assert _equal(res, forced)
    st, ob, _ = _errors(res, ref)
    qe = max((res.bus_q.cpu() - ref["bus_q"]).abs().max().item(), (res.edge_q.cpu() - ref["edge_q"]).abs().max().item())
    print(f"[wls mixed robust] {name}: errors at {ids}: state {st:.2e}/{mc.STATE_BOUND:.0e} q {qe:.2e}/{Q_BOUND:.0e} objective {ob:.2e}/{mc.OBJ_BOUND:.0e} "
          f"down-weighted {res.n_downweighted.tolist()} oracle {ref['n_downweighted'].tolist()}")
    assert torch.equal(res.iterations.cpu(), ref["iterations"]) and torch.equal(res.status.cpu(), ref["status"])
    assert st <= mc.STATE_BOUND and qe <= Q_BOUND and ob <= mc.OBJ_BOUND
    assert sum(ro.near_threshold(ref)) == 0
    assert ro.downweighted_ids(dict(bus_q=res.bus_q.cpu(), edge_q=res.edge_q.cpu())) == ro.downweighted_ids(ref)
    assert torch.equal(res.n_downweighted.cpu(), ref["n_downweighted"]) and bool((res.n_downweighted >= 1).all())


def test_bad_data_on_a_mix_removes_what_the_oracle_removes(pkg):
    hb, ids = mc.corrupted("BD")
    ref = mc.bad_data_oracle("BD", 1)
    res = _run(pkg, _to_device(hb), "wls_bad_data", max_iter=8, tol=0.0, threshold=4.0, max_removals=1)
    S = torch.cat([res.bus_sens.cpu().reshape(-1), res.edge_sens.cpu().reshape(-1)])
    rn = torch.cat([res.bus_rn.cpu().reshape(-1), res.edge_rn.cpu().reshape(-1)])
    S0 = torch.cat([ref["bus_sens"].reshape(-1), ref["edge_sens"].reshape(-1)])
    rn0 = torch.cat([ref["bus_rn"].reshape(-1), ref["edge_rn"].reshape(-1)])
    kept, low = S0 >= 2 * S_MIN, S0 < S_MIN / 2
    e_s = (S - S0).abs().max().item()
    e_rn = ((rn - rn0).abs() / rn0.clamp_min(1.0))[kept].max().item()
    e_std = (res.state_std.cpu() - ref["state_std"]).abs().max().item()
    e_st = (res.state.cpu().double() - ref["state"]).abs().max().item()
    e_rem = ((res.removed_rn.cpu() - ref["removed_rn"]).abs() / ref["removed_rn"].clamp_min(1.0)).max().item()
    print(f"[wls mixed bad data] errors at {ids}: removed {res.removed[:, 0].tolist()} oracle {ref['removed'][:, 0].tolist()} rN "
          f"{['%.2f' % v for v in res.removed_rn[:, 0].tolist()]}: removed_rn {e_rem:.2e}/{RN_BOUND:.0e} state {e_st:.2e}/{mc.STATE_BOUND:.0e} "
          f"S {e_s:.2e}/{SENS_BOUND:.0e} rN {e_rn:.2e}/{RN_BOUND:.0e} state_std {e_std:.2e}/{STD_BOUND:.2e}")
    assert torch.equal(res.removed.cpu(), ref["removed"]) and torch.equal(res.n_removed.cpu(), ref["n_removed"])      # global ids
    assert sum(r == i for r, i in zip(res.removed[:, 0].tolist(), ids)) >= 3
    assert torch.equal(res.iterations.cpu(), ref["iterations"]) and torch.equal(res.status.cpu(), ref["status"])
    assert torch.equal(res.dof.cpu(), ref["dof"]) and torch.equal(res.suspect.cpu(), ref["suspect"])
    assert bool((rn[low] == 0).all()) and bool((rn0[low] == 0).all())
    assert e_rem <= RN_BOUND and e_st <= mc.STATE_BOUND and e_s <= SENS_BOUND and e_rn <= RN_BOUND and e_std <= STD_BOUND


# ---- 7. replays

def test_replays_agree_bitwise(pkg):
    b = _device("B")
    kw = dict(max_iter=6, tol=mc.TOL)
    eager = _run(pkg, b, **kw)
    static = dict(b, x=b["x"].clone(), edge_attr=b["edge_attr"].clone(), graph_ptr=b["graph_ptr"].clone())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _run(pkg, static, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = _run(pkg, static, **kw)
    graph.replay()
    torch.cuda.synchronize()
    assert _equal(out, eager)
    with torch.no_grad():
        rec = pkg.graphs.PlannedStep(lambda: _run(pkg, static, **kw))
    rec.replay()
    torch.cuda.synchronize()
    assert _equal(rec.loss, eager)
    # the blocked form, recorded
    c = _device("C")
    eager = _run(pkg, c, LARGE_ENTRY, **kw)
    with torch.no_grad():
        rec = pkg.graphs.PlannedStep(lambda: _run(pkg, c, LARGE_ENTRY, **kw))
    rec.replay()
    torch.cuda.synchronize()
    assert _equal(rec.loss, eager)


# ---- 8. the loader and the runner

def test_a_mixed_dataset_carries_graph_ptr_and_evaluate_wls_solves_it(pkg):
    ds, est = pkg.dataset, pkg.estimator
    full = pkg.synthetic.make_batch(["cigre14", "ober_sub"], 256, seed=0)       # (the driver's way: statistics of a large mixed batch)
    stats = tuple(s.to(DEV) for s in full["stats"])
    parts = [ds.DeviceDataset.from_batch(pkg.synthetic.make_batch([c], 4, seed=6 + k, stats=full["stats"]), device=torch.device(DEV))
             for k, c in enumerate(["cigre14", "ober_sub"])]
    mixed = ds.MixedDataset(parts).shuffled(np.random.default_rng(0))
    assert mixed.n is None
    loader = ds.DataLoader(mixed, batch_size=3, shuffle=False)
    bad = graphs = 0
    for i, batch in enumerate(loader):
        ids = mixed.ids[3 * i:3 * i + 3]
        part = np.searchsorted(mixed.start, ids, side="right") - 1
        want = np.concatenate([[0], np.cumsum([parts[p].n for p in part])])
        assert batch.max_nodes == 70 and batch.graph_ptr.dtype == torch.int64 and batch.graph_ptr.is_contiguous()
        assert batch.graph_ptr.tolist() == want.tolist() and int(batch.graph_ptr[-1]) == batch.x.shape[0]
        res = est.wls_estimate(batch.x, batch.edge_index, batch.edge_attr, *stats, batch.max_nodes, graph_ptr=batch.graph_ptr)
        print(f"[wls mixed loader] batch {i}: graph_ptr {batch.graph_ptr.tolist()} status {res.status.tolist()} iterations {res.iterations.tolist()}")
        bad, graphs = bad + int((res.status != 0).sum()), graphs + res.status.numel()
    assert graphs == 8
    got = pkg.runner.evaluate_wls(loader, stats)
    print(f"[wls mixed evaluate] {got}")
    assert set(got) == set(pkg.data.EVAL_METRICS) | {"wls_mean_iterations", "wls_not_converged"}
    assert all(math.isfinite(v) for v in got.values()) and got["wls_not_converged"] == bad
    assert got == pkg.runner.evaluate_wls(loader, stats, 70)                # (max_nodes wins over nodes_per_graph)
    robust = pkg.runner.evaluate_wls(loader, stats, robust=dict(gamma=3.0))
    assert all(math.isfinite(v) for v in robust.values()) and "wls_downweighted" in robust
    # a same-bus-count MixedDataset is left as it was: no graph_ptr
    same = ds.MixedDataset([parts[0], parts[0]])
    first = next(iter(ds.DataLoader(same, batch_size=3, shuffle=False)))
    assert same.n == 15 and first.graph_ptr is None and first.max_nodes is None
    # a uniform loader: with its graph_ptr (synthetic.make_batch's) and without, the same metrics
    loader_h = [pkg.synthetic.make_batch(["cigre14"], 4, seed=s, stats=full["stats"]) for s in (21, 22)]
    with_ptr = [{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in bb.items() if k != "stats"} for bb in loader_h]
    without = [{k: v for k, v in bb.items() if k != "graph_ptr"} for bb in with_ptr]
    assert pkg.runner.evaluate_wls(with_ptr, stats, 15) == pkg.runner.evaluate_wls(without, stats, 15)
    with pytest.raises(ValueError, match="nodes_per_graph is None"):
        pkg.runner.evaluate_wls(without, stats)
