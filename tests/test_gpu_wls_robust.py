"""GPU: estimator.wls_robust / csrc/dss2_wls_robust.hip (the Huber M-estimator by re-weighted Gauss-Newton, on the LDS kernel and on the
blocked kernel) against the plain estimators, to the bit where the mathematics coincide, and against the fp64 oracle of
tests/wls_robust_oracle.py on batches with one gross error of 25 sigma per graph (`corrupted`), gamma = 3.

Bounds, none taken from the kernel (tests/test_wls_robust_cpu.py measures the spreads and holds the literals below to them):
  state      max(5e-7, 8 x spread), spread = the worst, over four random summation orders of the ORACLE, of |fp32(oracle state) -
             permuted-order state|: 5e-7 everywhere but on ober179 (condition number 2.4e13), see STATE_BOUNDS
  q          max(1e-9, 8 x spread of the oracle's q over the same four orders): Q_BOUND for all cases but ober179 after one iteration
  objective  1e-6 relative (8 x the oracle's spread stays below it)
The margin of 8 is tests/test_gpu_wls_large.py's.  Iterations and status equal the oracle's; the set {q < 1} and n_downweighted equal
the oracle's (no measurement of these cases has |t - gamma| <= 1e-6 gamma in the oracle: asserted, nothing is left out).
ober179 is held to the fixed trip count 14 instead of decisions at a tolerance, for the reason given in tests/test_gpu_wls_large.py.

The batches are tests/wls_cases.py's, wls_edge_cases.py's and wls_large_cases.py's own: three graphs each, cigre14 five, mixed seven, cap one.

Measured on the MI355X (bound in brackets): state 5.96e-8 at worst [5e-7], ober179 after one iteration 3.3e-7 [2.5e-6]; q after one
iteration 3.6e-8 at worst (n128, plain_iters 1 [2.7e-7]; every case at most a quarter of its bound), ober179 7.8e-7 [5.2e-6]; q from three
iterations on 3.1e-13 [1e-9]; objective 1.3e-8 relative, ober179 after one iteration 4.4e-8 [1e-6]; sets, counts, iterations, status and
every decision at tol = 1e-6 equal to the oracle's; the two forms' fp32 states identical but for 5.8e-11 on ober_sub after one iteration;
evaluate_wls: worst metric mae_loading_trafos on cigre14 at 9.0e-6 of the fp64 value [1e-5].

What must hold to the bit: gamma = inf against wls_estimate / wls_estimate_large (all five fields; q = 1, nothing down-weighted); gamma = 3
with plain_iters = max_iter (state, iterations, status, last_step; the Huber cost is at most the plain J); two runs; a graph at positions
0 and 2; max_groups 1 and 2; a failing graph beside healthy ones; hipGraph and launch-plan replays.  Every test prints its errors beside
the bounds (-s).
"""
import ctypes as C
import functools
import importlib
import math

import pytest
import torch

import dss2_oracle
import wls_bad_data_oracle as bo
import wls_cases as wc
import wls_edge_cases as ec
import wls_large_cases as lc
import wls_oracle as wo
import wls_robust_oracle as ro
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAMMA, TOL = 3.0, 1e-6
STATE_FLOOR, Q_FLOOR, OBJ_BOUND, FORMS_AGREEMENT = 5e-7, 1e-9, 1e-6, 1.2e-7
SMALL = ["two_bus", "star10", "ring6_parallel", "n33", "cigre14", "mixed", "ober_sub"]
LDS_CASES = SMALL + ec.SIZES                                 # n32: the largest one-wave size; n64, n65; n99: the LDS cap
LARGE_CASES = SMALL + lc.ALL                                 # + n100, n128, n179t, ober179, cap
PLAIN_ITERS = (0, 1)
FIELDS = ("state", "objective", "iterations", "status", "last_step")


def trip_counts(name):
    return {"cap": (1, 3), "ober179": (1, 3, 8, 14)}.get(name, (1, 3, 8))


# (case, trip count, plain_iters) -> bound where it is not the default; tests/test_wls_robust_cpu.py::test_the_gpu_tests_bounds_cover_the_oracles_spread
# Measured oracle spreads: state at most 6.0e-8 (the fp32 rounding of the output) but on ober179 after one iteration, 2.6e-7 (plain_iters 0)
# and 2.9e-7 (1); q at most 7.9e-13 from three iterations on (one measurement per graph is down-weighted by then) and, after ONE
# iteration, when 2 to 204 measurements per graph are, 2.1e-12 (cigre14) .. 6.8e-8 (n99), 5.4e-7 / 3.9e-7 on ober179.
STATE_BOUNDS = {("ober179", 1, 0): 2.5e-6, ("ober179", 1, 1): 2.8e-6}
Q_BOUND = Q_FLOOR
Q_BOUNDS = {("two_bus", 1, 1): 2.6e-9, ("star10", 1, 1): 2.0e-8, ("ring6_parallel", 1, 0): 1.2e-9, ("ring6_parallel", 1, 1): 6.9e-9,
            ("n33", 1, 0): 7.5e-9, ("n33", 1, 1): 2.1e-7, ("mixed", 1, 0): 5.9e-8, ("mixed", 1, 1): 7.0e-8, ("ober_sub", 1, 0): 2.8e-9,
            ("ober_sub", 1, 1): 1.5e-9, ("n32", 1, 1): 1.2e-9, ("n64", 1, 0): 2.5e-9, ("n64", 1, 1): 4.1e-8, ("n65", 1, 0): 1.2e-9,
            ("n65", 1, 1): 7.9e-9, ("n99", 1, 0): 5.4e-8, ("n99", 1, 1): 6.6e-7, ("n100", 1, 0): 3.9e-8, ("n100", 1, 1): 7.6e-8,
            ("n128", 1, 0): 3.2e-8, ("n128", 1, 1): 2.7e-7, ("n179t", 1, 0): 6.3e-8, ("n179t", 1, 1): 2.7e-7, ("ober179", 1, 0): 5.2e-6,
            ("ober179", 1, 1): 3.8e-6, ("cap", 1, 0): 3.8e-8, ("cap", 1, 1): 4.0e-8}
# Decisions at tol = 1e-6.  The re-weighted iteration converges linearly, so a deciding step within a factor 4 of tol is common: in the
# oracle 4 of 5 graphs of cigre14, 5 of 7 of mixed, all of n99 and cap, one of ring6_parallel.  Those batches are held to the fixed trip
# counts above (like ober179); these ten have 2 such graphs of 30 (one of n33, one of n100), both forms and both LDS kernel widths.
CONVERGENCE_CASES = ["two_bus", "star10", "n33", "ober_sub", "n32", "n64", "n65", "n100", "n128", "n179t"]
CONVERGENCE_GRAPHS = 30


def state_bound(name, it, plain):
    return STATE_BOUNDS.get((name, it, plain), STATE_FLOOR)


def q_bound(name, it, plain):
    return Q_BOUNDS.get((name, it, plain), Q_BOUND)


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module(PKG_NAME)
    p._lib.lib()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return p


def _to_device(b):
    return {k: (tuple(s.to(DEV) for s in v) if k == "stats" else (v.to(DEV) if torch.is_tensor(v) else v)) for k, v in b.items()}


@functools.lru_cache(maxsize=None)
def _device(name, clean=False):
    if clean:
        return _to_device(ec.batch(name) if name in ec.CASES else lc.batch(name))
    return _to_device(ro.corrupted(name)[0])


def _run(pkg, b, entry="wls_robust", **kw):
    return getattr(pkg.estimator, entry)(b["x"], b["edge_index"], b["edge_attr"], *b["stats"], b["nodes_per_graph"], **kw)


def _equal(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


def _q_error(res, ref):
    bus = (res.bus_q.cpu() - ref["bus_q"]).abs().max().item()
    edge = (res.edge_q.cpu() - ref["edge_q"]).abs().max().item() if ref["edge_q"].numel() else 0.0
    return max(bus, edge)


def _ids(res):
    return ro.downweighted_ids(dict(bus_q=res.bus_q.cpu(), edge_q=res.edge_q.cpu()))


# ---- 1. the anchor

@pytest.mark.parametrize("name,large", [("cigre14", False), ("n33", False), ("ober_sub", False), ("ober_sub", True), ("n100", True), ("ober179", True)])
def test_gamma_inf_is_the_plain_estimator_to_the_bit(pkg, name, large):
    b = _device(name)
    plain_entry = "wls_estimate_large" if large else "wls_estimate"
    for kw in (dict(max_iter=1, tol=0.0), dict(max_iter=8, tol=0.0), dict(max_iter=20, tol=TOL)):
        plain = _run(pkg, b, entry=plain_entry, **kw)
        for plain_iters in PLAIN_ITERS:
            res = _run(pkg, b, gamma=float("inf"), plain_iters=plain_iters, large=large, **kw)
            assert isinstance(res, pkg.estimator.WLSRobustResult) and res._fields[:5] == FIELDS
            for f in FIELDS:
                assert torch.equal(getattr(res, f), getattr(plain, f)), (name, large, kw, f)
            assert res.bus_q.dtype == torch.float64 and res.bus_q.shape == (b["x"].shape[0], 4)
            assert res.edge_q.dtype == torch.float64 and res.edge_q.shape == (b["edge_attr"].shape[0], 2)
            assert res.n_downweighted.dtype == torch.int32 and res.n_downweighted.shape == plain.iterations.shape
            assert bool((res.bus_q == 1.0).all()) and bool((res.edge_q == 1.0).all()) and bool((res.n_downweighted == 0).all())
        # gamma = 3 with every iteration plain: the plain iterates, and the Huber cost of the plain solution
        res = _run(pkg, b, gamma=GAMMA, plain_iters=kw["max_iter"], large=large, **kw)
        for f in ("state", "iterations", "status", "last_step"):
            assert torch.equal(getattr(res, f), getattr(plain, f)), (name, large, kw, f)
        assert bool((res.objective <= plain.objective).all())
        print(f"[wls robust anchor] {name} large={large} {kw}: equal to {plain_entry}; with gamma = 3 and plain iterations only "
              f"{int(res.n_downweighted.sum())} measurements have q < 1, cost {res.objective.sum().item():.6g} against J {plain.objective.sum().item():.6g}")


# ---- 2. parity with the oracle at fixed trip counts

def _parity_params():
    out = []
    for large, cases in ((False, LDS_CASES), (True, LARGE_CASES)):
        out += [(name, large, it, plain) for name in cases for it in trip_counts(name) for plain in PLAIN_ITERS]
    return out


@pytest.mark.parametrize("name,large,max_iter,plain_iters", _parity_params())
def test_parity_at_fixed_trip_counts(pkg, name, large, max_iter, plain_iters):
    sb, qb = state_bound(name, max_iter, plain_iters), q_bound(name, max_iter, plain_iters)
    ref = ro.oracle(name, max_iter, 0.0, plain_iters)
    res = _run(pkg, _device(name), max_iter=max_iter, tol=0.0, gamma=GAMMA, plain_iters=plain_iters, large=large)
    st = (res.state.cpu().double() - ref["state"]).abs().max().item()
    ob = ((res.objective.cpu() - ref["objective"]).abs() / ref["objective"].abs()).max().item()
    qe = _q_error(res, ref)
    print(f"[wls robust parity] {name} large={large} max_iter={max_iter} plain_iters={plain_iters}: state {st:.2e}/{sb:.1e} q {qe:.2e}/{qb:.1e} "
          f"objective {ob:.2e}/{OBJ_BOUND:.0e} down-weighted {res.n_downweighted.tolist()} oracle {ref['n_downweighted'].tolist()}")
    assert torch.equal(res.iterations.cpu(), ref["iterations"]) and torch.equal(res.status.cpu(), ref["status"])
    assert bool((res.status == 1).all()) and bool((res.iterations == max_iter).all())
    assert st <= sb, (st, sb)
    assert qe <= qb, (qe, qb)
    assert ob <= OBJ_BOUND, (ob, OBJ_BOUND)
    assert sum(ro.near_threshold(ref)) == 0                   # (nothing may be left out of the next comparison)
    assert _ids(res) == ro.downweighted_ids(ref)
    assert torch.equal(res.n_downweighted.cpu(), ref["n_downweighted"])
    assert bool((res.bus_q > 0).all()) and bool((res.bus_q <= 1).all()) and bool((res.edge_q > 0).all()) and bool((res.edge_q <= 1).all())


# ---- 3. convergence decisions

def test_convergence_decisions_match_the_oracle(pkg):
    total = excluded = 0
    for name in CONVERGENCE_CASES:
        ref = ro.oracle(name, 20, TOL)
        res = _run(pkg, _device(name), max_iter=20, tol=TOL, gamma=GAMMA)
        skip = wo.undecided(ref, TOL)
        total, excluded = total + skip.numel(), excluded + int(skip.sum())
        print(f"[wls robust convergence] {name}: iterations {res.iterations.tolist()} oracle {ref['iterations'].tolist()} status {res.status.tolist()} "
              f"last_step {['%.1e' % v for v in res.last_step.tolist()]} excluded {skip.tolist()}")
        keep = ~skip
        assert torch.equal(res.status.cpu()[keep], ref["status"][keep]) and torch.equal(res.iterations.cpu()[keep], ref["iterations"][keep])
        assert bool((ref["status"] == 0).all())
        n = ro.corrupted(name)[0]["nodes_per_graph"]
        assert (res.state.cpu().double() - ref["state"])[keep.repeat_interleave(n)].abs().max() <= STATE_FLOOR
        assert torch.equal(res.n_downweighted.cpu()[keep], ref["n_downweighted"][keep])
    assert total == CONVERGENCE_GRAPHS and excluded <= 0.1 * total, (excluded, total)


# ---- 4. the two forms

@pytest.mark.parametrize("max_iter", [1, 3, 8])
@pytest.mark.parametrize("name", ["cigre14", "ober_sub", "n33"])
def test_the_two_forms_agree(pkg, name, max_iter):
    b = _device(name)
    kw = dict(max_iter=max_iter, tol=0.0, gamma=GAMMA)
    lds, big = _run(pkg, b, large=False, **kw), _run(pkg, b, large=True, **kw)
    st = (big.state.double() - lds.state.double()).abs().max().item()
    qe = max((big.bus_q - lds.bus_q).abs().max().item(), (big.edge_q - lds.edge_q).abs().max().item())
    qb = q_bound(name, max_iter, 1)
    print(f"[wls robust forms] {name} max_iter={max_iter}: state {st:.2e}/{FORMS_AGREEMENT:.1e} q {qe:.2e}/{qb:.1e}")
    assert torch.equal(big.iterations, lds.iterations) and torch.equal(big.status, lds.status)
    assert torch.equal(big.n_downweighted, lds.n_downweighted)
    assert st <= FORMS_AGREEMENT and qe <= qb


# ---- 5. to the bit

@pytest.mark.parametrize("name,large", [("n33", False), ("n100", True)])
def test_runs_copies_and_group_counts_agree_bitwise(pkg, name, large):
    b = _device(name)
    kw = dict(max_iter=8, tol=TOL, gamma=GAMMA, large=large)
    res = _run(pkg, b, **kw)
    assert bool((res.status == 0).all()) and int(res.n_downweighted.sum()) == 3
    assert _equal(_run(pkg, b, **kw), res)
    for groups in (1, 2):
        assert _equal(_run(pkg, b, max_groups=groups, **kw), res), groups
    # graph 0 again at position 2: its rows come out as at position 0, and as in the plain batch
    n, hb = b["nodes_per_graph"], ro.corrupted(name)[0]
    rows0, erows0 = ec.graph_rows(hb, 0)
    e0 = int(erows0.sum())
    twice = _to_device(dict(hb, x=torch.cat([hb["x"][:2 * n], hb["x"][rows0]]), edge_attr=torch.cat([hb["edge_attr"][:2 * e0], hb["edge_attr"][erows0]])))
    assert torch.equal(hb["edge_index"][:, :e0] + 2 * n, hb["edge_index"][:, 2 * e0:])          # (the three graphs share one structure)
    for groups in (0, 1, 2):
        out = _run(pkg, twice, max_groups=groups, **kw)
        assert torch.equal(out.state[:n], out.state[2 * n:]) and torch.equal(out.state[:2 * n], res.state[:2 * n])
        assert torch.equal(out.bus_q[:n], out.bus_q[2 * n:]) and torch.equal(out.bus_q[:2 * n], res.bus_q[:2 * n])
        assert torch.equal(out.edge_q[:e0], out.edge_q[2 * e0:]) and torch.equal(out.edge_q[:2 * e0], res.edge_q[:2 * e0])
        for f in FIELDS[1:] + ("n_downweighted",):
            assert torch.equal(getattr(out, f)[0], getattr(out, f)[2]) and torch.equal(getattr(out, f)[:2], getattr(res, f)[:2]), f
    if large:     # ... and ober179, whose workgroups own two rows of G per thread, with fewer workgroups than graphs
        ober = _device("ober179")
        assert _equal(_run(pkg, ober, max_iter=3, tol=0.0, max_groups=2), _run(pkg, ober, max_iter=3, tol=0.0))


@pytest.mark.parametrize("large", [False, True])
@pytest.mark.parametrize("name", ec.FAILING)
def test_a_failing_graph_fails_alone(pkg, name, large):
    hb, bad = ec.batch(name), ec.FAILING_GRAPH
    b, healthy = _device(name), _device(ec.HEALTHY[name], clean=True)
    assert ro.corrupted(name)[0] is hb                         # (the failing cases go through as they are)
    n = hb["nodes_per_graph"]
    for plain_iters in PLAIN_ITERS:
        kw = dict(max_iter=10, tol=TOL, gamma=GAMMA, plain_iters=plain_iters, large=large)
        res, want = _run(pkg, b, **kw), _run(pkg, healthy, **kw)
        print(f"[wls robust failing] {name} large={large} plain_iters={plain_iters}: status {res.status.tolist()} iterations {res.iterations.tolist()}")
        assert int(res.status[bad]) == 2 and int(res.iterations[bad]) == 0 and float(res.last_step[bad]) == 0.0
        assert torch.equal(res.state[bad * n:(bad + 1) * n], torch.tensor([1.0, 0.0], device=DEV).expand(n, 2))
        for g in range(hb["num_graphs"]):
            if g == bad:
                continue
            rows, erows = ec.graph_rows(hb, g)
            erows = erows.to(DEV)
            assert torch.equal(res.state[rows], want.state[rows]) and torch.equal(res.bus_q[rows], want.bus_q[rows])
            assert torch.equal(res.edge_q[erows], want.edge_q[erows])
            for f in FIELDS[1:] + ("n_downweighted",):
                assert torch.equal(getattr(res, f)[g], getattr(want, f)[g]), f
            assert int(want.status[g]) == 0


def _static_copy(b):
    return dict(b, x=b["x"].clone(), edge_attr=b["edge_attr"].clone())


@pytest.mark.parametrize("name,large", [("n33", False), ("n100", True)])
def test_replays_agree_bitwise(pkg, name, large):
    b = _device(name)
    n = b["nodes_per_graph"]
    kind = lc.TREES[name] if name in lc.TREES else {}
    other = wc.collate([wc.graph(name, k, **kind) for k in (3, 4, 5)], n)
    assert torch.equal(other["edge_index"].to(DEV), b["edge_index"])
    kw = dict(max_iter=8, tol=TOL, gamma=GAMMA, large=large)
    eager = _run(pkg, b, **kw)
    eager_other = _run(pkg, dict(b, x=other["x"].to(DEV), edge_attr=other["edge_attr"].to(DEV)), **kw)
    assert not torch.equal(eager_other.state, eager.state) and not torch.equal(eager_other.bus_q, eager.bus_q)
    # hipGraph
    static = _static_copy(b)
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
    static["x"].copy_(other["x"])
    static["edge_attr"].copy_(other["edge_attr"])
    graph.replay()
    torch.cuda.synchronize()
    assert _equal(out, eager_other)
    # launch plan
    static = _static_copy(b)
    with torch.no_grad():
        rec = pkg.graphs.PlannedStep(lambda: _run(pkg, static, **kw))
    assert rec.n_launches == 1
    rec.replay()
    torch.cuda.synchronize()
    assert _equal(rec.loss, eager)
    static["x"].copy_(other["x"])
    static["edge_attr"].copy_(other["edge_attr"])
    rec.replay()
    torch.cuda.synchronize()
    assert _equal(rec.loss, eager_other)


# ---- 6. refusals

def test_refusals(pkg):
    est = pkg.estimator
    L, lib = pkg._lib.lib(), pkg._lib
    b, h = _device("n100"), ro.corrupted("n100")[0]
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="gamma must be > 0"):
            _run(pkg, b, gamma=bad)
    for bad in (-1, 0.5):
        with pytest.raises(ValueError, match="plain_iters"):
            _run(pkg, b, plain_iters=bad)
    with pytest.raises(NotImplementedError, match="at most 99 buses per graph, got 100"):
        _run(pkg, b, large=False)
    cap = est.max_nodes_per_graph_large()
    n = cap + 1
    x, ea = torch.zeros(n, 11, device=DEV), torch.zeros(n - 1, 13, device=DEV)
    ei = torch.stack([torch.arange(n - 1, device=DEV), torch.arange(1, n, device=DEV)])
    for large in (None, True):
        with pytest.raises(NotImplementedError, match=f"at most {cap} buses per graph, got {n}"):
            est.wls_robust(x, ei, ea, *b["stats"], n, large=large)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        est.wls_robust(h["x"], h["edge_index"], h["edge_attr"], *h["stats"], 100)
    with pytest.raises(ValueError, match="nodes_per_graph"):
        _run(pkg, dict(b, nodes_per_graph=99))
    with pytest.raises(ValueError, match="max_iter"):
        _run(pkg, b, max_iter=0)
    for bad in (torch.ones(300, 3, device=DEV), torch.ones(299, 2, device=DEV), torch.ones(600, device=DEV)):
        with pytest.raises(ValueError, match="init must be"):
            _run(pkg, b, init=bad)
    # through the ABI: rc 2 and a message, before any launch
    stream = lib.stream_ptr(torch.device(DEV))
    assert L.dss2_wls_robust(None, stream) == 2 and L.dss2_wls_robust_large(None, stream) == 2
    a = lib.WlsRobustArgs()
    a.solve.n_nodes, a.solve.n_edges, a.solve.nodes_per_graph, a.solve.max_iter, a.solve.tol = 300, 297, 100, 5, 1e-6
    a.gamma, a.plain_iters = 3.0, 1
    assert L.dss2_wls_robust(C.byref(a), stream) == 2 and b"100 buses per graph need more than" in L.dss2_last_error()
    assert L.dss2_wls_robust_large(C.byref(a), stream) == 2 and b"workspace is null" in L.dss2_last_error()
    need = L.dss2_wls_large_workspace_bytes(100, L.dss2_wls_large_groups(C.byref(a.solve)))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    a.workspace, a.workspace_bytes = ws.data_ptr(), need - 1
    assert L.dss2_wls_robust_large(C.byref(a), stream) == 2 and b"workspace has" in L.dss2_last_error()
    a.workspace_bytes = need
    assert L.dss2_wls_robust_large(C.byref(a), stream) == 2 and b"wls_robust_large: null argument" in L.dss2_last_error()      # (no tensors)
    a.solve.n_nodes, a.solve.n_edges, a.solve.nodes_per_graph = 30, 27, 10
    assert L.dss2_wls_robust(C.byref(a), stream) == 2 and b"wls_robust: null argument" in L.dss2_last_error()
    # ... with every tensor of the solve in place: the parameters and the three outputs of this entry
    hb = ro.corrupted("star10")[0]
    full = _device("star10")
    good = _run(pkg, full, max_iter=3, tol=0.0)
    topo = pkg.topology.get_topology(full["edge_index"], 30)
    s = a.solve
    keep = [full["x"].contiguous(), full["edge_attr"].contiguous(), *(t.float().contiguous() for t in full["stats"]),
            torch.empty(30, 2, device=DEV), torch.empty(3, 2, dtype=torch.float64, device=DEV), torch.empty(3, dtype=torch.int32, device=DEV),
            torch.empty(3, dtype=torch.int32, device=DEV), torch.empty(3, dtype=torch.float64, device=DEV), torch.empty(130, device=DEV)]
    s.x, s.ldx, s.edge_attr, s.ldea = keep[0].data_ptr(), keep[0].stride(0), keep[1].data_ptr(), keep[1].stride(0)
    s.x_mean, s.x_std, s.edge_mean, s.edge_std = (t.data_ptr() for t in keep[2:6])
    s.efrom, s.eto, s.inc_rowptr, s.inc_ent = (t.data_ptr() for t in (topo.efrom, topo.eto, topo.inc_rowptr, topo.inc_ent))
    s.n_nodes, s.n_edges, s.nodes_per_graph, s.max_iter, s.tol = 30, topo.E, 10, 3, 0.0
    s.w_v = s.w_p = s.w_pf = 1.0
    s.state, s.objective, s.iterations, s.status, s.last_step, s.vminmax = (t.data_ptr() for t in keep[6:])
    for entry in (L.dss2_wls_robust, L.dss2_wls_robust_large):
        for gamma in (0.0, -3.0, float("nan")):
            a.gamma = gamma
            assert entry(C.byref(a), stream) == 2 and b"gamma must be > 0" in L.dss2_last_error()
        a.gamma, a.plain_iters = 3.0, -1
        assert entry(C.byref(a), stream) == 2 and b"plain_iters must be >= 0" in L.dss2_last_error()
        a.plain_iters = 1
        assert entry(C.byref(a), stream) == 2 and b"null argument" in L.dss2_last_error()            # (bus_q, edge_q, n_downweighted)
    bus_q, edge_q, down = torch.empty(30, 4, dtype=torch.float64, device=DEV), torch.ones(hb["edge_attr"].shape[0], 2, dtype=torch.float64, device=DEV), torch.empty(3, dtype=torch.int32, device=DEV)
    a.bus_q, a.edge_q, a.n_downweighted = bus_q.data_ptr(), edge_q.data_ptr(), down.data_ptr()
    a.gamma = float("inf")                                     # +inf is allowed
    assert L.dss2_wls_robust(C.byref(a), stream) == 0
    a.gamma = 3.0
    assert L.dss2_wls_robust(C.byref(a), stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(keep[6], good.state) and torch.equal(bus_q, good.bus_q) and torch.equal(edge_q, good.edge_q) and torch.equal(down, good.n_downweighted)


# ---- 7. the evaluation

@pytest.mark.parametrize("grid,n,graphs", [("ober179", 179, 2), ("cigre14", 15, 3)])
def test_evaluate_wls_robust_scores_the_oracle_states(pkg, grid, n, graphs):
    """runner.evaluate_wls(robust=...) on a loader of two corrupted batches: the ten evaluation metrics against the same metrics computed
    in torch fp64 from the oracle's states, at a fixed trip count of 8; wls_downweighted against the oracle's count."""
    stats_h = (lc.batch("ober179") if grid == "ober179" else wc.grid_batch("cigre14"))["stats"]
    loader_h = []
    for seed in (21, 22):
        bb = pkg.synthetic.make_batch([grid], graphs, seed=seed, stats=stats_h)
        ids = bo.largest_sensitivity_targets(bb["x"], bb["edge_index"], bb["edge_attr"], stats_h, n)
        x2, ea2 = bo.add_gross_errors(bb["x"], bb["edge_attr"], stats_h, ids, ro.SIGMAS)
        loader_h.append(dict(bb, x=x2, edge_attr=ea2))
    loader = [{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in bb.items() if k != "stats"} for bb in loader_h]
    stats = tuple(s.to(DEV) for s in stats_h)
    got = pkg.runner.evaluate_wls(loader, stats, n, max_iter=8, tol=0.0, robust=dict(gamma=GAMMA))
    want = {k: 0.0 for k in pkg.data.EVAL_METRICS}
    zero, one = torch.zeros(8, dtype=torch.float64), torch.ones(8, dtype=torch.float64)
    down = 0
    for bb in loader_h:
        ref = ro.solve_huber(bb["x"], bb["edge_index"], bb["edge_attr"], stats_h, n, max_iter=8, tol=0.0, gamma=GAMMA)
        assert sum(ro.near_threshold(ref)) == 0
        down += int(ref["n_downweighted"].sum())
        m, _ = dss2_oracle.eval_batch_metrics(ref["state"], bb["y"].double(), bb["x"].double(), bb["edge_index"], bb["edge_attr"].double(), zero, one)
        for k in want:
            want[k] += m[k] / 2
    for k in pkg.data.EVAL_METRICS:
        err = abs(got[k] - want[k]) / abs(want[k])
        print(f"[wls robust evaluate] {grid} {k}: {got[k]:.8g} against {want[k]:.8g}: {err:.2e}/1e-05")
    print(f"[wls robust evaluate] {grid}: wls_downweighted {got['wls_downweighted']} against {down}")
    assert set(got) == set(pkg.data.EVAL_METRICS) | {"wls_mean_iterations", "wls_not_converged", "wls_downweighted"}
    assert got["wls_mean_iterations"] == 8.0 and got["wls_not_converged"] == 2 * graphs
    assert got["wls_downweighted"] == down and down >= 2 * graphs
    for k in pkg.data.EVAL_METRICS:
        assert abs(got[k] - want[k]) <= 1e-5 * abs(want[k]), (k, got[k], want[k])
    with pytest.raises(ValueError, match="bad_data and robust"):
        pkg.runner.evaluate_wls(loader, stats, n, bad_data=dict(threshold=3.0), robust=dict(gamma=GAMMA))
    assert math.isfinite(got["wls_mean_iterations"])
