"""GPU: estimator.wls_estimate_banded / csrc/dss2_wls_banded.hpp (the blocked kernel on a band of the gain matrix, buses numbered by
estimator.band_order) against the fp64 oracle of tests/wls_oracle.py on the batches of tests/wls_banded_cases.py.

Bounds, none taken from the kernel (tests/wls_banded_cases.py): the state within wls_large_cases.state_bound(spread) -- 8 x the oracle's
own spread over four summation orders, never below 5e-7 --, the objective within 1e-6 relative, iterations and statuses equal to the
oracle's (at tol = 1e-6 a graph whose deciding step lies within a factor 4 of tol is left out, wls_oracle.undecided, as in every WLS test
here).  Against the dense kernels on sizes both serve: within twice the bound.

What must hold to the bit: two runs; max_groups = 1 against the default; a graph alone against the same graph inside a batch; a hipGraph
replay and a launch-plan replay against the eager call with a given `order`, also after the static inputs were overwritten; the graphs
beside one that does not fit its declared band.  Every test prints its errors beside the bounds (-s).
"""
import ctypes as C
import functools
import importlib

import pytest
import torch

import dss2_oracle
import wls_banded_cases as bc
import wls_cases as wc
import wls_oracle as wo
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-6
FIELDS = ("state", "objective", "iterations", "status", "last_step")
BEYOND = ["n257", "n320", "radial300"]


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
    return _to_device(bc.batch(name))


def _order(pkg, b, **kw):
    return pkg.estimator.band_order(b["edge_index"], b["nodes_per_graph"], num_nodes=b["x"].size(0), **kw)


def _run(pkg, b, entry="wls_estimate_banded", **kw):
    return getattr(pkg.estimator, entry)(b["x"], b["edge_index"], b["edge_attr"], *b["stats"], b["nodes_per_graph"], **kw)


def _equal(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


def _parity(tag, res, name, max_iter, tol=0.0):
    """The five outputs against the oracle's; returns the state bound."""
    ref, bound = bc.oracle(name, max_iter, tol), bc.bound(name, max_iter, tol)
    n = bc.batch(name)["nodes_per_graph"]
    keep = ~wo.undecided(ref, tol)
    rows = keep.repeat_interleave(n)
    st = (res.state.cpu().double() - ref["state"])[rows].abs().max().item()
    ob = ((res.objective.cpu() - ref["objective"]).abs() / ref["objective"].abs())[keep].max().item()
    print(f"[wls banded {tag}] {name} max_iter={max_iter} tol={tol:g}: state {st:.2e}/{bound:.1e} objective {ob:.2e}/{bc.OBJ_BOUND:.0e} "
          f"iterations {res.iterations.tolist()} oracle {ref['iterations'].tolist()} status {res.status.tolist()} left out {(~keep).tolist()}")
    assert res.state.dtype == torch.float32 and res.state.shape == ref["state"].shape and res.objective.dtype == torch.float64
    assert res.iterations.dtype == torch.int32 and res.status.dtype == torch.int32 and res.last_step.dtype == torch.float64
    assert int(keep.sum()) >= max(1, keep.numel() - 1)
    assert torch.equal(res.iterations.cpu()[keep], ref["iterations"][keep]) and torch.equal(res.status.cpu()[keep], ref["status"][keep])
    assert st <= bound, (st, bound)
    assert ob <= bc.OBJ_BOUND, (ob, bc.OBJ_BOUND)
    return bound


@pytest.mark.parametrize("max_iter", [1, 3, 8])
@pytest.mark.parametrize("name", BEYOND)
def test_parity_beyond_the_dense_cap(pkg, name, max_iter):
    assert bc.batch(name)["nodes_per_graph"] > pkg.estimator.max_nodes_per_graph_large()
    res = _run(pkg, _device(name), max_iter=max_iter, tol=0.0)
    _parity("parity", res, name, max_iter)
    assert bool((res.status == 1).all()) and bool((res.iterations == max_iter).all())


@pytest.mark.parametrize("name", BEYOND)
def test_convergence_decisions_beyond_the_dense_cap(pkg, name):
    _parity("convergence", _run(pkg, _device(name), max_iter=8, tol=TOL), name, 8, TOL)


@pytest.mark.parametrize("name", ["cigre14", "mixed", "ober_sub", "n100", "ober179", "cap"])
def test_sizes_both_forms_serve(pkg, name):
    b = _device(name)
    res = _run(pkg, b, max_iter=8, tol=0.0)
    bound = _parity("both", res, name, 8)
    dense = "wls_estimate" if b["nodes_per_graph"] <= pkg.estimator.max_nodes_per_graph() else "wls_estimate_large"
    other = _run(pkg, b, entry=dense, max_iter=8, tol=0.0)
    st = (res.state.double() - other.state.double()).abs().max().item()
    print(f"[wls banded both] {name}: against {dense} {st:.2e}/{2 * bound:.1e}")
    assert st <= 2 * bound and torch.equal(res.iterations, other.iterations) and torch.equal(res.status, other.status)


def test_band_edges(pkg):
    """One 70-bus graph with the band forced to the minimum, around one and two blocks, and dense as a band."""
    b = _device("ober70")
    least = _order(pkg, b).half_bandwidth
    assert least < 15
    for hb in (least, 15, 16, 17, 31, 32, 33, 2 * 70 - 1):
        res = _run(pkg, b, max_iter=8, tol=0.0, order=_order(pkg, b, half_bandwidth=hb))
        _parity(f"edges hb={hb}", res, "ober70", 8)


def test_a_numbering_without_a_band(pkg):
    """The randomly relabelled tree as it comes (an identity order: hb near dense) and through Cuthill-McKee."""
    b = _device("relabelled257")
    ident, cm = _order(pkg, b, identity=True), _order(pkg, b)
    print(f"[wls banded unordered] hb {ident.half_bandwidth} as it comes, {cm.half_bandwidth} ordered")
    assert cm.half_bandwidth < 64 and 300 < ident.half_bandwidth
    for o in (ident, cm):
        _parity(f"unordered hb={o.half_bandwidth}", _run(pkg, b, max_iter=8, tol=0.0, order=o), "relabelled257", 8)


@pytest.mark.parametrize("max_iter", [1, 3, 8])
def test_star_of_41_buses(pkg, max_iter):
    b = _device("star41")
    assert _order(pkg, b).half_bandwidth == 81
    _parity("star", _run(pkg, b, max_iter=max_iter, tol=0.0), "star41", max_iter)


def test_mixed_topologies_in_one_batch(pkg):
    b = _device("mixed8")
    o = _order(pkg, b)
    assert o.n_orderings == 2
    _parity("mixed", _run(pkg, b, max_iter=8, tol=0.0, order=o), "mixed8", 8)


def test_runs_group_counts_and_batch_positions_agree_bitwise(pkg):
    b = _device("n257")
    kw = dict(max_iter=5, tol=TOL)
    res = _run(pkg, b, **kw)
    assert _equal(_run(pkg, b, **kw), res)
    assert _equal(_run(pkg, b, max_groups=1, **kw), res)
    alone = _to_device(wc.collate([wc.graph("n257", 1, **bc.TREES["n257"])], 257))
    out = _run(pkg, alone, **kw)
    assert torch.equal(out.state, res.state[257:])
    for f in FIELDS[1:]:
        assert torch.equal(getattr(out, f)[0], getattr(res, f)[1]), f


def _static_copy(b):
    return dict(b, x=b["x"].clone(), edge_attr=b["edge_attr"].clone())


def test_replays_with_a_given_order_agree_bitwise(pkg):
    b = _device("n257")
    other = wc.collate([wc.graph("n257", k, **bc.TREES["n257"]) for k in (2, 3)], 257)
    assert torch.equal(other["edge_index"], bc.batch("n257")["edge_index"])
    order = _order(pkg, b)
    kw = dict(max_iter=5, tol=TOL, order=order)
    eager = _run(pkg, b, **kw)
    eager_other = _run(pkg, dict(b, x=other["x"].to(DEV), edge_attr=other["edge_attr"].to(DEV)), **kw)
    assert not torch.equal(eager_other.state, eager.state) and _equal(eager, _run(pkg, b, max_iter=5, tol=TOL))
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
    # launch plan: the gathers of x and of the state are launches of the library, and replay with the solve
    static = _static_copy(b)
    with torch.no_grad():
        rec = pkg.graphs.PlannedStep(lambda: _run(pkg, static, **kw))
    rec.replay()
    torch.cuda.synchronize()
    assert _equal(rec.loss, eager)
    static["x"].copy_(other["x"])
    static["edge_attr"].copy_(other["edge_attr"])
    rec.replay()
    torch.cuda.synchronize()
    assert _equal(rec.loss, eager_other)


def test_refusals_and_the_band_guard(pkg):
    est, lib = pkg.estimator, pkg._lib
    L = lib.lib()
    b = _device("n257")
    # hb above the cap of (n, hb)
    cap = est.band_max_half_bandwidth(257)
    with pytest.raises(NotImplementedError, match=f"hb of at most {cap} states, got hb = {cap + 1}"):
        _run(pkg, b, order=_order(pkg, b, half_bandwidth=cap + 1))
    _run(pkg, b, max_iter=1, order=_order(pkg, b, half_bandwidth=cap))
    with pytest.raises(ValueError, match="order was made for"):
        _run(pkg, _device("n320"), order=_order(pkg, b))
    # a band one block too small for ONE graph of three: the star in the caller's numbering needs Wb = 5 (its last leaf's rows, in block
    # row 5, reach column 0); hb = 64 declares 4.  That graph: status 2, no iteration, its init; the chains beside it: the correct call's bits.
    g = _device("guard41")
    good = _order(pkg, g, identity=True)
    assert good.half_bandwidth == 81
    init = torch.stack([torch.linspace(0.98, 1.02, 123, device=DEV), torch.linspace(-0.01, 0.01, 123, device=DEV)], 1)
    init[g["x"][:, 9] != 0, 1] = 0.0
    kw = dict(max_iter=6, tol=TOL, init=init)
    want = _run(pkg, g, order=good, **kw)
    assert bool((want.status != 2).all())
    # (the call's workspace, three slices, is put in its place beforehand: poisoned, with a poisoned page behind the bytes the call declares)
    need = est.band_workspace_bytes(41, 64, 3)
    ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    est._WORKSPACES[(g["x"].device, need)] = ws
    short = _run(pkg, g, order=good._replace(half_bandwidth=64), **kw)
    torch.cuda.synchronize()
    del est._WORKSPACES[(g["x"].device, need)]
    # nothing of the graph that does not fit was assembled -- its slice is untouched -- and nothing was written behind the workspace;
    # the chains' slices were used
    assert bool((ws[need // 3:2 * need // 3] == 0xA5).all()) and bool((ws[need:] == 0xA5).all())
    assert not bool((ws[:need // 3] == 0xA5).all()) and not bool((ws[2 * need // 3:need] == 0xA5).all())
    print(f"[wls banded guard] status {short.status.tolist()} iterations {short.iterations.tolist()} against {want.status.tolist()} {want.iterations.tolist()}")
    assert int(short.status[1]) == 2 and int(short.iterations[1]) == 0 and float(short.last_step[1]) == 0.0
    assert torch.equal(short.state[41:82], init[41:82]) and bool(torch.isfinite(short.objective).all())
    for k in (0, 2):
        assert torch.equal(short.state[41 * k:41 * k + 41], want.state[41 * k:41 * k + 41])
        for f in FIELDS[1:]:
            assert torch.equal(getattr(short, f)[k], getattr(want, f)[k]), (f, k)
    # through the ABI: rc 2 and a message, before any launch
    stream = lib.stream_ptr(torch.device(DEV))
    a = lib.WlsLargeArgs()
    a.solve.n_nodes, a.solve.n_edges, a.solve.nodes_per_graph, a.solve.max_iter, a.solve.tol = 514, 512, 257, 5, 1e-6
    assert a.solve.half_bandwidth == 0
    assert L.dss2_wls_solve_large(C.byref(a), stream) == 2 and b"257 buses" in L.dss2_last_error() and b"at most 256" in L.dss2_last_error()
    a.solve.half_bandwidth = cap + 1
    assert L.dss2_wls_solve_large(C.byref(a), stream) == 2 and f"half-bandwidth of {cap + 1}".encode() in L.dss2_last_error()
    a.solve.half_bandwidth = -1
    assert L.dss2_wls_solve_large(C.byref(a), stream) == 2 and b"half_bandwidth" in L.dss2_last_error()
    a.solve.half_bandwidth = 19
    assert L.dss2_wls_solve_large(C.byref(a), stream) == 2 and b"workspace is null" in L.dss2_last_error()
    need = est.band_workspace_bytes(257, 19, 2)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    a.workspace, a.workspace_bytes = ws.data_ptr(), need - 1
    assert L.dss2_wls_solve_large(C.byref(a), stream) == 2 and f"need {need}".encode() in L.dss2_last_error()
    a.workspace_bytes = need
    assert L.dss2_wls_solve_large(C.byref(a), stream) == 2 and b"null argument" in L.dss2_last_error()      # (the Python formula is the C side's; the tensors are missing)
    ptr = torch.tensor([0, 257, 514], device=DEV)
    a.solve.graph_ptr, a.solve.n_graphs = ptr.data_ptr(), 2
    assert L.dss2_wls_solve_large(C.byref(a), stream) == 2 and b"graph_ptr" in L.dss2_last_error()
    torch.cuda.synchronize()


def test_evaluate_wls_routes_above_256_buses(pkg):
    h = bc.batch("radial300")
    b = _device("radial300")
    loader = [{k: v for k, v in b.items() if k != "stats"}]
    with pytest.raises(NotImplementedError, match="at most 256 buses per graph, got 300"):
        pkg.runner.evaluate_wls(loader, b["stats"], 300, max_iter=8, tol=0.0)
    got = pkg.runner.evaluate_wls(loader, b["stats"], 300, max_iter=8, tol=0.0, banded="auto")
    ref = bc.oracle("radial300", 8, 0.0)
    zero, one = torch.zeros(8, dtype=torch.float64), torch.ones(8, dtype=torch.float64)
    want, _ = dss2_oracle.eval_batch_metrics(ref["state"], h["y"].double(), h["x"].double(), h["edge_index"], h["edge_attr"].double(), zero, one)
    assert got["wls_mean_iterations"] == 8.0 and got["wls_not_converged"] == 2
    for k in pkg.data.EVAL_METRICS:
        err = abs(got[k] - want[k]) / abs(want[k])
        print(f"[wls banded evaluate] {k}: {got[k]:.8g} against {want[k]:.8g}: {err:.2e}/1e-05")
        assert err <= 1e-5, (k, got[k], want[k])
