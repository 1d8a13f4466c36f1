"""GPU: estimator.wls_estimate_large / csrc/dss2_wls_large.hip (the gain matrix in global memory, blocked Cholesky) against the fp64 oracle
of tests/wls_oracle.py on the batches of tests/wls_large_cases.py -- trees of 100, 128 and 179 buses, ober179, one graph at the cap of
256 buses -- and on every batch of tests/wls_cases.py (small graphs through the large kernel), three graphs each.

Bounds, none taken from the kernel.  State: max(5e-7, 8 x spread), spread = the worst, over four random summation orders of the ORACLE,
of |fp32(oracle state) - permuted-order state| (tests/test_wls_large_cpu.py measures it and holds the literals below to it):
  trees and the cap graph, every trip count   spread <= 6.0e-8                        bound 5e-7
  ober179, 1 / 3 / 8 / 14 iterations          spread 2.9e-7 .. 3.1e-7 / 8.4e-8 .. 1.0e-7 / 5.9e-8 / 6.0e-8 (two machines' BLAS orders)
                                              bound 2.5e-6 / 8.2e-7 / 5e-7 / 5e-7   (condition number 2.4e13, first step 0.64)
  wls_cases' batches                          the existing 5e-7
Objective 1e-6 relative (oracle spread at most 3.6e-8, ober179 after one iteration).  Iterations and status equal.  Against
estimator.wls_estimate (the LDS kernel) on cigre14, ober_sub and n33: state within 1.2e-7, twice the fp32 rounding of the output -- both
round one fp64 solution.  runner.evaluate_wls: the ten metrics within 1e-5 relative of the fp64 metrics of the oracle's states.
ober179's Gauss-Newton converges linearly (steps shrinking by 0.3 .. 0.7: deciding steps 8.7e-7, 2.9e-7, 5.2e-7 at iterations 12, 9, 14,
every one within a factor 4 of tol = 1e-6), so it is held to a fourth fixed trip count, 14, not to decisions at a tolerance.

Measured on the MI355X (bound in brackets): trees and the cap graph 5.96e-8 at worst (the fp32 rounding of the output) [5e-7], objective
1.3e-8 relative (n100, one iteration) [1e-6]; ober179 3.14e-7 / 5.96e-8 / 5.93e-8 / 5.93e-8 after 1 / 3 / 8 / 14 iterations [2.5e-6 /
8.2e-7 / 5e-7 / 5e-7], objective 6.8e-8 after one iteration; wls_cases' batches 5.96e-8; iterations and status equal everywhere, every
decision at tol = 1e-6 equal to the oracle's (star10's excluded graph included); against the LDS kernel the fp32 states are identical;
from the oracle's solution on n128 one update of 5.0e-8 .. 5.9e-8; evaluate_wls on ober179: worst metric rmse_v at 3.2e-7 of the fp64 value.

What must hold to the bit: two runs; a graph at positions 0 and 2 of a batch; max_groups 1 and 2 against the default; a failing graph in
front (status 2, no update, its start state) leaves the other graphs' rows alone; a hipGraph replay and a launch-plan replay against
the eager call, also after the static inputs were overwritten with another batch.  Every test prints its errors beside the bounds (-s).
"""
import ctypes as C
import functools
import importlib

import pytest
import torch

import dss2_oracle
import wls_cases as wc
import wls_edge_cases as ec
import wls_large_cases as lc
import wls_oracle as wo
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL_BOUND, OBJ_BOUND, TOL, LDS_AGREEMENT = 5e-7, 1e-6, 1e-6, 1.2e-7
# (case, trip count) -> state bound; tests/test_wls_large_cpu.py::test_the_gpu_tests_bounds_cover_the_oracles_spread
STATE_BOUNDS = {(name, it): 5e-7 for name in lc.SIZES for it in (1, 3, 8)}
STATE_BOUNDS.update({("cap", 1): 5e-7, ("cap", 3): 5e-7, ("ober179", 1): 2.5e-6, ("ober179", 3): 8.2e-7, ("ober179", 8): 5e-7, ("ober179", 14): 5e-7})
CONVERGENCE_CASES = wc.ALL_BATCHES + lc.SIZES
FIELDS = ("state", "objective", "iterations", "status", "last_step")


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
    return _to_device(lc.batch(name))


def _run(pkg, b, entry="wls_estimate_large", **kw):
    return getattr(pkg.estimator, entry)(b["x"], b["edge_index"], b["edge_attr"], *b["stats"], b["nodes_per_graph"], **kw)


def _errors(res, ref):
    st = (res.state.cpu().double() - ref["state"]).abs().max().item()
    ob = ((res.objective.cpu() - ref["objective"]).abs() / ref["objective"].abs()).max().item()
    return st, ob


def _equal(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("name,max_iter", sorted(STATE_BOUNDS) + [(name, it) for name in wc.ALL_BATCHES for it in (1, 3, 8)])
def test_parity_at_fixed_trip_counts(pkg, name, max_iter):
    bound = STATE_BOUNDS.get((name, max_iter), SMALL_BOUND)
    ref = lc.oracle(name, max_iter, 0.0)
    res = _run(pkg, _device(name), max_iter=max_iter, tol=0.0)
    st, ob = _errors(res, ref)
    print(f"[wls large parity] {name} max_iter={max_iter}: state {st:.2e}/{bound:.1e} objective {ob:.2e}/{OBJ_BOUND:.0e} "
          f"iterations {res.iterations.tolist()} status {res.status.tolist()}")
    assert res.state.dtype == torch.float32 and res.objective.dtype == torch.float64 and res.objective.shape == (ref["objective"].shape[0], 2)
    assert res.iterations.dtype == torch.int32 and res.status.dtype == torch.int32 and res.last_step.dtype == torch.float64
    assert torch.equal(res.iterations.cpu(), ref["iterations"]) and torch.equal(res.status.cpu(), ref["status"])
    assert bool((res.status == 1).all()) and bool((res.iterations == max_iter).all())
    assert st <= bound, (st, bound)
    assert ob <= OBJ_BOUND, (ob, OBJ_BOUND)
    step = ((res.last_step.cpu() - ref["last_step"]).abs() / ref["last_step"]).max().item()
    print(f"[wls large parity] {name} max_iter={max_iter}: last_step relative difference {step:.2e}")


def test_convergence_decisions_match_the_oracle(pkg):
    total = excluded = 0
    for name in CONVERGENCE_CASES:
        ref = lc.oracle(name, 20, TOL)
        res = _run(pkg, _device(name), max_iter=20, tol=TOL)
        skip = wo.undecided(ref, TOL)
        total, excluded = total + skip.numel(), excluded + int(skip.sum())
        print(f"[wls large convergence] {name}: iterations {res.iterations.tolist()} oracle {ref['iterations'].tolist()} status {res.status.tolist()} "
              f"last_step {['%.1e' % v for v in res.last_step.tolist()]} excluded {skip.tolist()}")
        keep = ~skip
        assert torch.equal(res.status.cpu()[keep], ref["status"][keep]) and torch.equal(res.iterations.cpu()[keep], ref["iterations"][keep])
        assert bool((ref["status"] == 0).all())
        assert (res.state.cpu().double() - ref["state"])[keep.repeat_interleave(lc.batch(name)["nodes_per_graph"])].abs().max() <= SMALL_BOUND
    assert total == 36 and excluded <= 0.1 * total, (excluded, total)


@pytest.mark.parametrize("max_iter", [1, 3, 8])
@pytest.mark.parametrize("name", ["cigre14", "ober_sub", "n33"])
def test_agreement_with_the_lds_kernel(pkg, name, max_iter):
    b = _device(name)
    lds = _run(pkg, b, entry="wls_estimate", max_iter=max_iter, tol=0.0)
    res = _run(pkg, b, max_iter=max_iter, tol=0.0)
    st = (res.state.double() - lds.state.double()).abs().max().item()
    ob = ((res.objective - lds.objective).abs() / lds.objective.abs()).max().item()
    print(f"[wls large against lds] {name} max_iter={max_iter}: state {st:.2e}/{LDS_AGREEMENT:.1e} objective {ob:.2e} relative")
    assert torch.equal(res.iterations, lds.iterations) and torch.equal(res.status, lds.status)
    assert st <= LDS_AGREEMENT, (st, LDS_AGREEMENT)


def test_runs_copies_and_group_counts_agree_bitwise(pkg):
    b = _device("n100")
    kw = dict(max_iter=6, tol=TOL)
    res = _run(pkg, b, **kw)
    assert bool((res.status == 0).all())
    assert _equal(_run(pkg, b, **kw), res)
    for groups in (1, 2):
        assert _equal(_run(pkg, b, max_groups=groups, **kw), res), groups
    # graph 0 again at position 2: its rows come out as at position 0, and as in the plain batch
    g = [wc.graph("n100", k, **lc.TREES["n100"]) for k in (0, 1, 0)]
    twice = _to_device(wc.collate(g, 100))
    for groups in (0, 1, 2):
        out = _run(pkg, twice, max_groups=groups, **kw)
        assert torch.equal(out.state[:100], out.state[200:]) and torch.equal(out.state[:200], res.state[:200])
        for f in FIELDS[1:]:
            assert torch.equal(getattr(out, f)[0], getattr(out, f)[2]) and torch.equal(getattr(out, f)[:2], getattr(res, f)[:2]), f
    # ... and ober179, whose workgroups own two rows of G per thread, with fewer workgroups than graphs
    ober = _device("ober179")
    assert _equal(_run(pkg, ober, max_iter=3, tol=0.0, max_groups=2), _run(pkg, ober, max_iter=3, tol=0.0))


def test_a_failing_graph_in_front_fails_alone(pkg):
    hb = lc.batch("n100")
    b, behind = _device("n100"), _to_device(ec.preceded_by_failing_graph(hb))
    kw = dict(max_iter=10, tol=TOL)
    res = _run(pkg, b, **kw)
    for groups in (0, 1, 2):
        long = _run(pkg, behind, max_groups=groups, **kw)
        print(f"[wls large failing] max_groups={groups}: status {long.status.tolist()} iterations {long.iterations.tolist()}")
        assert int(long.status[0]) == 2 and int(long.iterations[0]) == 0 and float(long.last_step[0]) == 0.0
        assert torch.equal(long.state[:100], torch.tensor([1.0, 0.0], device=DEV).expand(100, 2))
        assert torch.equal(long.state[100:], res.state)
        for f in FIELDS[1:]:
            assert torch.equal(getattr(long, f)[1:], getattr(res, f)), f
        assert bool(torch.isfinite(long.objective).all())


def _static_copy(b):
    return dict(b, x=b["x"].clone(), edge_attr=b["edge_attr"].clone())


def test_replays_agree_bitwise(pkg):
    b = _device("n100")
    other = wc.collate([wc.graph("n100", k, **lc.TREES["n100"]) for k in (3, 4, 5)], 100)
    assert torch.equal(other["edge_index"], lc.batch("n100")["edge_index"])
    kw = dict(max_iter=6, tol=TOL)
    eager = _run(pkg, b, **kw)
    eager_other = _run(pkg, dict(b, x=other["x"].to(DEV), edge_attr=other["edge_attr"].to(DEV)), **kw)
    assert not torch.equal(eager_other.state, eager.state)
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


def test_warm_start_from_the_solution(pkg):
    flat = lc.oracle("n128", 20, TOL)
    res = _run(pkg, _device("n128"), init=flat["state"].float().to(DEV), max_iter=20, tol=TOL)
    st = (res.state.cpu().double() - flat["state"]).abs().max().item()
    print(f"[wls large warm] n128 from the solution: iterations {res.iterations.tolist()} last_step {['%.1e' % v for v in res.last_step.tolist()]} "
          f"state {st:.2e}/{SMALL_BOUND:.0e}")
    assert bool((res.status == 0).all()) and bool((res.iterations == 1).all()) and bool((res.last_step < TOL).all())
    assert st <= SMALL_BOUND


def test_refusals(pkg):
    est = pkg.estimator
    L, lib = pkg._lib.lib(), pkg._lib
    cap = est.max_nodes_per_graph_large()
    assert cap == lc.CAP
    n = cap + 1
    x, ea = torch.zeros(n, 11, device=DEV), torch.zeros(n - 1, 13, device=DEV)
    ei = torch.stack([torch.arange(n - 1, device=DEV), torch.arange(1, n, device=DEV)])
    b, h = _device("n100"), lc.batch("n100")
    with pytest.raises(NotImplementedError, match=f"at most {cap} buses per graph, got {n}"):
        est.wls_estimate_large(x, ei, ea, *b["stats"], n)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        est.wls_estimate_large(h["x"], h["edge_index"], h["edge_attr"], *h["stats"], 100)
    with pytest.raises(ValueError, match="nodes_per_graph"):
        _run(pkg, dict(b, nodes_per_graph=99))
    with pytest.raises(ValueError, match="max_iter"):
        _run(pkg, b, max_iter=0)
    for bad in (torch.ones(300, 3, device=DEV), torch.ones(299, 2, device=DEV), torch.ones(600, device=DEV)):
        with pytest.raises(ValueError, match="init must be"):
            _run(pkg, b, init=bad)
    # through the ABI: rc 2 and a message, before any launch
    stream = lib.stream_ptr(torch.device(DEV))
    a = lib.WlsLargeArgs()
    a.solve.n_nodes, a.solve.n_edges, a.solve.nodes_per_graph, a.solve.max_iter, a.solve.tol = n, n - 1, n, 5, 1e-6
    assert L.dss2_wls_solve_large(C.byref(a), stream) == 2 and f"{n} buses".encode() in L.dss2_last_error()
    a.solve.n_nodes, a.solve.nodes_per_graph = 201, 100
    assert L.dss2_wls_solve_large(C.byref(a), stream) == 2 and b"multiple" in L.dss2_last_error()
    a.solve.n_nodes = 300
    assert L.dss2_wls_solve_large(C.byref(a), stream) == 2 and b"workspace is null" in L.dss2_last_error()
    need = L.dss2_wls_large_workspace_bytes(100, L.dss2_wls_large_groups(C.byref(a.solve)))
    assert need == 3 * L.dss2_wls_large_workspace_bytes(100, 1) > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    a.workspace, a.workspace_bytes = ws.data_ptr(), need - 1
    assert L.dss2_wls_solve_large(C.byref(a), stream) == 2 and b"workspace has" in L.dss2_last_error()
    a.workspace_bytes = need
    assert L.dss2_wls_solve_large(C.byref(a), stream) == 2 and b"null argument" in L.dss2_last_error()      # (the tensors are still missing)
    assert L.dss2_wls_solve_large(None, stream) == 2
    torch.cuda.synchronize()


def test_evaluate_wls_scores_the_oracle_states_on_ober179(pkg):
    """runner.evaluate_wls on a loader of two ober179 batches (it picks wls_estimate_large above 99 buses): the ten evaluation metrics
    against the same metrics computed in torch fp64 from the oracle's states, at a fixed trip count of 8."""
    stats_h = lc.batch("ober179")["stats"]
    loader_h = [pkg.synthetic.make_batch(["ober179"], 2, seed=s, stats=stats_h) for s in (21, 22)]
    loader = [{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in bb.items() if k != "stats"} for bb in loader_h]
    stats = _device("ober179")["stats"]
    got = pkg.runner.evaluate_wls(loader, stats, 179, max_iter=8, tol=0.0)
    want = {k: 0.0 for k in pkg.data.EVAL_METRICS}
    zero, one = torch.zeros(8, dtype=torch.float64), torch.ones(8, dtype=torch.float64)
    for bb in loader_h:
        ref = wo.solve(bb["x"], bb["edge_index"], bb["edge_attr"], stats_h, 179, max_iter=8, tol=0.0)
        m, _ = dss2_oracle.eval_batch_metrics(ref["state"], bb["y"].double(), bb["x"].double(), bb["edge_index"], bb["edge_attr"].double(), zero, one)
        for k in want:
            want[k] += m[k] / 2
    for k in pkg.data.EVAL_METRICS:
        err = abs(got[k] - want[k]) / abs(want[k])
        print(f"[wls large evaluate] {k}: {got[k]:.8g} against {want[k]:.8g}: {err:.2e}/1e-05")
    assert set(got) == set(pkg.data.EVAL_METRICS) | {"wls_mean_iterations", "wls_not_converged"}
    assert got["wls_mean_iterations"] == 8.0 and got["wls_not_converged"] == 4
    for k in pkg.data.EVAL_METRICS:
        assert abs(got[k] - want[k]) <= 1e-5 * abs(want[k]), (k, got[k], want[k])
    with pytest.raises(NotImplementedError, match="at most 99 buses per graph, got 179"):
        pkg.runner.evaluate_wls(loader, stats, 179, bad_data=dict(threshold=3.0))
