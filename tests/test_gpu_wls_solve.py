"""GPU: estimator.wls_estimate / csrc/dss2_wls_solve.hip against the fp64 oracle of tests/wls_oracle.py on the batches of
tests/wls_cases.py -- cigre14 (5 graphs), cigre14 mixed with cigre14_reswitched (7), ober_sub (3: the multi-wave kernel), and the
hand-built shapes two_bus, star10 (a hub of degree 9), ring6_parallel (a doubled branch) and n33 (66 states, just over one wave),
three graphs each.

Bounds (set by the issue from two fp64 implementations that differ in summation order and factorisation, never from the kernel):
state within 5e-7 absolute (8 x the 6e-8 the two differed by after fp32 rounding), objective within 1e-6 relative (prototype 1.5e-8),
iterations and status equal.  Every test prints its errors beside the bounds (run with -s).

Measured on the MI355X, worst case over the seven batches and the three trip counts (bound in brackets):
  state 5.96e-8 (n33, 3 iterations; the fp32 rounding of the output, 2^-24 at 1.0) [5e-7]
  objective 4.6e-9 relative (mixed, 1 iteration; 2.9e-9 on n33, 1.8e-9 on star10, all after the first iteration) [1e-6]
  iterations and status equal everywhere; at tol = 1e-6 every decision equals the oracle's, the one excluded graph (star10, deciding
  step 5.1e-7) included; from the oracle's solution one update of 2.8e-8 .. 6.0e-8, state within 5.95e-8
  runner.evaluate_wls: worst metric mae_loading_trafos at 6.2e-6 of the fp64 value [1e-5] (the fp32 evaluation kernels' own error)

What must hold to the bit: two runs; copies of a graph in one batch; a batch with one graph's measurements masked leaves the other
graphs' rows alone (that graph ends with status 2, no update, the state of its start); a cap on the number of workgroups (the grid
strides over the graphs); a hipGraph replay and a launch-plan replay, also after the static inputs were overwritten with another batch.
"""
import functools
import importlib

import pytest
import torch

import dss2_oracle
import wls_cases as wc
import wls_oracle as wo
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STATE_BOUND, OBJ_BOUND, TOL = 5e-7, 1e-6, 1e-6


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module(PKG_NAME)
    p._lib.lib()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return p


@functools.lru_cache(maxsize=None)
def _host(name):
    return wc.any_batch(name)


@functools.lru_cache(maxsize=None)
def _device(name):
    b = _host(name)
    return {k: (tuple(s.to(DEV) for s in v) if k == "stats" else (v.to(DEV) if torch.is_tensor(v) else v)) for k, v in b.items()}


@functools.lru_cache(maxsize=None)
def _oracle(name, max_iter, tol):
    b = _host(name)
    return wo.solve(b["x"], b["edge_index"], b["edge_attr"], b["stats"], b["nodes_per_graph"], max_iter=max_iter, tol=tol)


def _init_near_truth(name):
    y = _host(name)["y"].double().clone()
    y[:, 0] += 0.01
    return y.float()


def _run(pkg, b, **kw):
    return pkg.estimator.wls_estimate(b["x"], b["edge_index"], b["edge_attr"], *b["stats"], b["nodes_per_graph"], **kw)


def _errors(res, ref):
    st = (res.state.cpu().double() - ref["state"]).abs().max().item()
    ob = ((res.objective.cpu() - ref["objective"]).abs() / ref["objective"].abs()).max().item()
    return st, ob


def _equal(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("max_iter", [1, 3, 8])
@pytest.mark.parametrize("name", wc.ALL_BATCHES)
def test_parity_at_fixed_trip_counts(pkg, name, max_iter):
    ref = _oracle(name, max_iter, 0.0)
    res = _run(pkg, _device(name), max_iter=max_iter, tol=0.0)
    st, ob = _errors(res, ref)
    print(f"[wls parity] {name} max_iter={max_iter}: state {st:.2e}/{STATE_BOUND:.0e} objective {ob:.2e}/{OBJ_BOUND:.0e} "
          f"iterations {res.iterations.tolist()} status {res.status.tolist()}")
    assert res.state.dtype == torch.float32 and res.objective.dtype == torch.float64 and res.objective.shape == (ref["objective"].shape[0], 2)
    assert res.iterations.dtype == torch.int32 and res.status.dtype == torch.int32 and res.last_step.dtype == torch.float64
    assert torch.equal(res.iterations.cpu(), ref["iterations"]) and torch.equal(res.status.cpu(), ref["status"])
    assert bool((res.status == 1).all()) and bool((res.iterations == max_iter).all())
    assert st <= STATE_BOUND, (st, STATE_BOUND)
    assert ob <= OBJ_BOUND, (ob, OBJ_BOUND)
    step = ((res.last_step.cpu() - ref["last_step"]).abs() / ref["last_step"]).max().item()
    print(f"[wls parity] {name} max_iter={max_iter}: last_step relative difference {step:.2e}")


def test_convergence_decisions_match_the_oracle(pkg):
    total = excluded = 0
    for name in wc.ALL_BATCHES:
        ref = _oracle(name, 12, TOL)
        res = _run(pkg, _device(name), max_iter=12, tol=TOL)
        skip = wo.undecided(ref, TOL)
        total, excluded = total + skip.numel(), excluded + int(skip.sum())
        print(f"[wls convergence] {name}: iterations {res.iterations.tolist()} oracle {ref['iterations'].tolist()} status {res.status.tolist()} "
              f"last_step {['%.1e' % v for v in res.last_step.tolist()]} excluded {skip.tolist()}")
        keep = ~skip
        assert torch.equal(res.status.cpu()[keep], ref["status"][keep]) and torch.equal(res.iterations.cpu()[keep], ref["iterations"][keep])
        assert bool((ref["status"] == 0).all())
        assert (res.state.cpu().double() - ref["state"])[keep.repeat_interleave(_host(name)["nodes_per_graph"])].abs().max() <= STATE_BOUND
    assert excluded <= 0.1 * total, (excluded, total)


@pytest.mark.parametrize("name", wc.ALL_BATCHES)
def test_warm_starts(pkg, name):
    b = _device(name)
    flat = _oracle(name, 12, TOL)
    # from the oracle's solution: one update, below the tolerance
    init = flat["state"].float().to(DEV)
    res = _run(pkg, b, init=init, max_iter=12, tol=TOL)
    st = (res.state.cpu().double() - flat["state"]).abs().max().item()
    print(f"[wls warm] {name}: from the solution: iterations {res.iterations.tolist()} last_step {['%.1e' % v for v in res.last_step.tolist()]} state {st:.2e}/{STATE_BOUND:.0e}")
    assert bool((res.status == 0).all()) and bool((res.iterations == 1).all())
    assert st <= STATE_BOUND
    # from the labels + 0.01 in V: no more updates than from the flat start, on every graph
    near = _run(pkg, b, init=_init_near_truth(name).to(DEV), max_iter=12, tol=TOL)
    cold = _run(pkg, b, max_iter=12, tol=TOL)
    print(f"[wls warm] {name}: near the labels {near.iterations.tolist()} flat {cold.iterations.tolist()}")
    assert bool((near.status == 0).all()) and bool((near.iterations <= cold.iterations).all())
    # a strided init (two columns of a wider tensor) and slack angles that are not 0 in it: same bits as the clean one
    wide = torch.full((init.shape[0], 5), 7.0, device=DEV)
    wide[:, 1:3] = init
    wide[:, 2] += 0.3 * (b["x"][:, 9] != 0)
    again = _run(pkg, b, init=wide[:, 1:3], max_iter=12, tol=TOL)
    assert _equal(again, res)


def test_a_graph_without_measurements_fails_alone(pkg):
    b = _device("cigre14")
    n = b["nodes_per_graph"]
    assert b["num_graphs"] == 5
    six = pkg.synthetic.tile_real_batch(_host("cigre14"), 2)
    keep_e = int((six["edge_index"][0] < 6 * n).sum())
    x, ei, ea = six["x"][:6 * n].clone().to(DEV), six["edge_index"][:, :keep_e].to(DEV), six["edge_attr"][:keep_e].clone().to(DEV)
    assert bool((ei < 6 * n).all())
    whole = pkg.estimator.wls_estimate(x, ei, ea, *b["stats"], n, max_iter=12, tol=TOL)
    xm, eam = x.clone(), ea.clone()
    xm[2 * n:3 * n, :8] = 0.0
    eam[(ei[0] >= 2 * n) & (ei[0] < 3 * n), :4] = 0.0
    init = torch.stack([torch.full((6 * n,), 0.98, device=DEV), torch.full((6 * n,), -0.01, device=DEV) * (x[:, 9] == 0)], 1)
    for start in (None, init):
        ref = pkg.estimator.wls_estimate(x, ei, ea, *b["stats"], n, init=start, max_iter=12, tol=TOL)
        res = pkg.estimator.wls_estimate(xm, ei, eam, *b["stats"], n, init=start, max_iter=12, tol=TOL)
        print(f"[wls masked] status {res.status.tolist()} iterations {res.iterations.tolist()}")
        assert res.status.tolist() == [0, 0, 2, 0, 0, 0] and int(res.iterations[2]) == 0 and float(res.last_step[2]) == 0.0
        want = torch.tensor([1.0, 0.0], device=DEV).expand(n, 2) if start is None else start[2 * n:3 * n]
        assert torch.equal(res.state[2 * n:3 * n], want)
        others = torch.ones(6, dtype=torch.bool, device=DEV)
        others[2] = False
        rows = others.repeat_interleave(n)
        assert torch.equal(res.state[rows], ref.state[rows]) and torch.equal(res.objective[others], ref.objective[others])
        assert torch.equal(res.iterations[others], ref.iterations[others]) and torch.equal(res.last_step[others], ref.last_step[others])
        assert bool(torch.isfinite(res.objective).all())
    assert bool((whole.status == 0).all())


def _first_graphs(b, k):
    n = b["nodes_per_graph"]
    e = int((b["edge_index"][0] < k * n).sum())
    assert bool((b["edge_index"][:, :e] < k * n).all()) and bool((b["edge_index"][:, e:] >= k * n).all())
    return dict(b, x=b["x"][:k * n], edge_index=b["edge_index"][:, :e], edge_attr=b["edge_attr"][:e], y=b["y"][:k * n], num_graphs=k)


def test_copies_agree_bitwise_and_the_grid_strides(pkg):
    four = _first_graphs(_host("mixed"), 4)
    n = four["nodes_per_graph"]
    big = pkg.synthetic.tile_real_batch(four, 75)
    assert big["num_graphs"] == 300
    dev = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in big.items()}
    dev["stats"] = _device("mixed")["stats"]
    res = _run(pkg, dev, max_iter=8, tol=0.0)
    for t, rows in ((res.state, 4 * n), (res.objective, 4), (res.iterations, 4), (res.status, 4), (res.last_step, 4)):
        v = t.reshape(75, rows, -1)
        assert torch.equal(v, v[:1].expand_as(v))
    ref = wo.solve(four["x"], four["edge_index"], four["edge_attr"], four["stats"], n, max_iter=8, tol=0.0)
    st = (res.state[:4 * n].cpu().double() - ref["state"]).abs().max().item()
    ob = ((res.objective[:4].cpu() - ref["objective"]).abs() / ref["objective"].abs()).max().item()
    print(f"[wls copies] state {st:.2e}/{STATE_BOUND:.0e} objective {ob:.2e}/{OBJ_BOUND:.0e}")
    assert st <= STATE_BOUND and ob <= OBJ_BOUND
    # fewer workgroups than graphs: each strides over several graphs, same bits
    for groups in (1, 7, 299):
        assert _equal(_run(pkg, dev, max_iter=8, tol=0.0, max_groups=groups), res)
    # ... and in the multi-wave kernel
    ober = _device("ober_sub")
    assert _equal(_run(pkg, ober, max_iter=3, tol=0.0, max_groups=2), _run(pkg, ober, max_iter=3, tol=0.0))


def _static_copy(b):
    return dict(b, x=b["x"].clone(), edge_attr=b["edge_attr"].clone())


@pytest.mark.parametrize("name", ["cigre14", "ober_sub"])
def test_two_runs_and_replays_agree_bitwise(pkg, name):
    grids, B, seed, n = wc.GRID_BATCHES[name]
    b = _device(name)
    other = pkg.synthetic.make_batch(grids, B, seed=seed + 100, stats=_host(name)["stats"])
    kw = dict(max_iter=6, tol=TOL)
    eager = _run(pkg, b, **kw)
    assert _equal(_run(pkg, b, **kw), eager)
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


def test_refusals(pkg):
    b = _device("cigre14")
    h = _host("cigre14")
    big = pkg.synthetic.make_batch(["ober179"], 1, seed=0)
    with pytest.raises(NotImplementedError, match=str(pkg.estimator.max_nodes_per_graph())):
        pkg.estimator.wls_estimate(big["x"].to(DEV), big["edge_index"].to(DEV), big["edge_attr"].to(DEV), *[s.to(DEV) for s in big["stats"]], 179)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.estimator.wls_estimate(h["x"], h["edge_index"], h["edge_attr"], *h["stats"], 15)
    with pytest.raises(ValueError, match="nodes_per_graph"):
        _run(pkg, dict(b, nodes_per_graph=14))
    with pytest.raises(ValueError, match="nodes_per_graph"):
        _run(pkg, dict(b, nodes_per_graph=0))
    with pytest.raises(ValueError, match="max_iter"):
        _run(pkg, b, max_iter=0)
    with pytest.raises(ValueError, match="tol"):
        _run(pkg, b, tol=-1.0)
    for bad in (torch.ones(75, 3, device=DEV), torch.ones(74, 2, device=DEV), torch.ones(150, device=DEV)):
        with pytest.raises(ValueError, match="init must be"):
            _run(pkg, b, init=bad)
    # through the ABI: rc 2 and a message, before any launch
    import ctypes as C
    L, lib = pkg._lib.lib(), pkg._lib
    a = lib.WlsSolveArgs()
    a.n_nodes, a.n_edges, a.nodes_per_graph, a.max_iter, a.tol = 179, 178, 179, 5, 1e-6
    assert L.dss2_wls_solve(C.byref(a), lib.stream_ptr(torch.device(DEV))) == 2 and b"LDS" in L.dss2_last_error()
    a.n_nodes, a.nodes_per_graph = 31, 15
    assert L.dss2_wls_solve(C.byref(a), lib.stream_ptr(torch.device(DEV))) == 2 and b"multiple" in L.dss2_last_error()
    assert L.dss2_wls_solve(None, lib.stream_ptr(torch.device(DEV))) == 2
    torch.cuda.synchronize()


def test_evaluate_wls_scores_the_oracle_states(pkg):
    """runner.evaluate_wls on a loader of two batches: the ten evaluation metrics against the same metrics computed in torch fp64 from
    the oracle's states."""
    stats_h = _host("cigre14")["stats"]
    loader_h = [pkg.synthetic.make_batch(["cigre14"], 4, seed=s, stats=stats_h) for s in (21, 22)]
    loader = [{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in bb.items() if k != "stats"} for bb in loader_h]
    got = pkg.runner.evaluate_wls(loader, _device("cigre14")["stats"], 15)
    want = {k: 0.0 for k in pkg.data.EVAL_METRICS}
    its = []
    zero, one = torch.zeros(8, dtype=torch.float64), torch.ones(8, dtype=torch.float64)
    for bb in loader_h:
        ref = wo.solve(bb["x"], bb["edge_index"], bb["edge_attr"], stats_h, 15, max_iter=10, tol=TOL)
        its += ref["iterations"].tolist()
        m, _ = dss2_oracle.eval_batch_metrics(ref["state"], bb["y"].double(), bb["x"].double(), bb["edge_index"], bb["edge_attr"].double(), zero, one)
        for k in want:
            want[k] += m[k] / 2
    for k in pkg.data.EVAL_METRICS:
        err = abs(got[k] - want[k]) / abs(want[k])
        print(f"[wls evaluate] {k}: {got[k]:.8g} against {want[k]:.8g}: {err:.2e}/1e-05")
    print(f"[wls evaluate] mean iterations {got['wls_mean_iterations']:.3f} (oracle {sum(its) / len(its):.3f}), not converged {got['wls_not_converged']}")
    assert set(got) == set(pkg.data.EVAL_METRICS) | {"wls_mean_iterations", "wls_not_converged"}
    for k in pkg.data.EVAL_METRICS:
        assert abs(got[k] - want[k]) <= 1e-5 * abs(want[k]), (k, got[k], want[k])
    assert got["wls_not_converged"] == 0
    # the hybrid: a model's output as the start
    torch.manual_seed(0)
    model = pkg.MPN(8, 6, 2, 32, 1, 2, 0.0).to(DEV)
    warm = pkg.runner.evaluate_wls(loader, _device("cigre14")["stats"], 15, model=model, max_iter=12)
    print(f"[wls evaluate] from an untrained MPN: mean iterations {warm['wls_mean_iterations']:.3f}, not converged {warm['wls_not_converged']}, rmse_v {warm['rmse_v']:.4g}")
    assert warm["wls_mean_iterations"] >= 1.0
