"""GPU: estimator.wls_bad_data_large -- the blocked form of the bad-data kernel (csrc/dss2_wls_bad_data.hip with workspace != NULL,
csrc/dss2_wls_large_invert.hpp) -- against the fp64 oracle of tests/wls_bad_data_oracle.py on the batches of tests/wls_large_cases.py:
n100, n128, n179t, ober179 (three graphs each) and cap (one graph of 256 buses).

Every bound, and every list of graphs whose removals are compared, comes from tests/test_wls_bad_data_large_cpu.py, which measures them
in the oracle alone (never from the kernel), at tol = 0 and 8 iterations per solve:
  bus_sens, edge_sens   cpu.bounds(name)[0]: 2e-7 absolute on the trees (tests/test_gpu_wls_bad_data.py's), 8 x the fp64 routes' own
                        spread on ober179 (condition number 2.4e13: 1.4e-5)
  rN, removed_rn        the S bound at the floor, sens / (2 s_min), in units of max(rN, 1), where the oracle's S >= 2 s_min; measurements
                        with S inside [s_min / 2, 2 s_min] are left out (at most 10 % at s_min = 1e-4, which the clean comparison passes;
                        the CPU file asserts it), below s_min / 2 both sides give exactly 0
  state_std             cpu.bounds(name)[1]: 3.44e-9 on the trees, 8 x the routes' spread on ober179 (1.6e-6)
  dof, suspect, iterations, status   equal;  chi2_limit 1e-12 relative
  state                 wls_large_cases.state_bound(the oracle's spread over summation orders), as tests/test_gpu_wls_large.py has it
  sum S - dof           1e-6 on the trees (on ober179 the routes' own spread in S, times 1236 measurements, does not allow it)
A removal is compared on the graphs the CPU file lists as clear: 11 of 13 with one error (n100 graph 1 and ober179 graph 2 are run, and
their identity is not compared), n179t, ober179 graphs 0 and 1 and cap with three.  Every test prints its errors beside the bounds (-s).
"""
import ctypes as C
import functools
import importlib
import math

import pytest
import torch

import test_wls_bad_data_large_cpu as cpu
import wls_bad_data_oracle as bo
import wls_cases as wc
import wls_large_cases as lc
import wls_mixed_cases as mc
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXED = cpu.FIXED
SOLVE_FIELDS = ("state", "objective", "iterations", "status", "last_step")
PER_GRAPH = ("objective", "iterations", "status", "last_step", "dof", "chi2_limit", "suspect", "removed_rn", "n_removed")
BUS_ROWS, EDGE_ROWS = ("state", "bus_rn", "bus_sens", "state_std"), ("edge_rn", "edge_sens")
FORMS_STATE_BOUND = 1.2e-7           # two forms round one fp64 solution to fp32: one ulp at 1 p.u. (tests/test_gpu_wls_mixed.py's figure)


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


def _run(pkg, b, entry="wls_bad_data_large", **kw):
    if "graph_ptr" in b and "graph_ptr" not in kw:
        kw["graph_ptr"] = b["graph_ptr"]
    kw.setdefault("nodes_per_graph", b["nodes_per_graph"])
    n = kw.pop("nodes_per_graph")
    return getattr(pkg.estimator, entry)(b["x"], b["edge_index"], b["edge_attr"], *b["stats"], n, **kw)


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))


def _with_ptr(hb):
    """A uniform host batch with the keys of tests/wls_mixed_cases.py's batches (graph_ptr, edge_ptr, sizes), for mc.reordered."""
    if "graph_ptr" in hb and "edge_ptr" in hb:
        return hb
    n = hb["nodes_per_graph"]
    ptr = hb["graph_ptr"].tolist() if "graph_ptr" in hb else list(range(0, hb["x"].shape[0] + 1, n))
    src = hb["edge_index"][0]
    eptr = [int((src < p).sum()) for p in ptr]
    G = len(ptr) - 1
    assert all(bool(((src[eptr[g]:eptr[g + 1]] >= ptr[g]) & (src[eptr[g]:eptr[g + 1]] < ptr[g + 1])).all()) for g in range(G)), "branches are grouped by graph"
    return dict(hb, graph_ptr=torch.tensor(ptr, dtype=torch.int64), edge_ptr=eptr, sizes=[q - p for p, q in zip(ptr, ptr[1:])], num_graphs=G)


def _graph_view(res, hb, g):
    """Everything a result says about graph g of a batch with the keys of _with_ptr, ids made local to the graph."""
    rows, erows = mc.graph_rows(hb, g)
    N, n = hb["x"].shape[0], hb["sizes"][g]
    ids = res.removed[g].cpu()
    local = torch.where(ids < 0, ids, torch.where(ids < 4 * N, ids - 4 * rows.start, ids - 4 * N - 2 * erows.start + 4 * n))
    return ([getattr(res, f)[rows].cpu() for f in BUS_ROWS] + [getattr(res, f)[erows].cpu() for f in EDGE_ROWS] +
            [getattr(res, f)[g].cpu() for f in PER_GRAPH] + [local])


def _compare_measurements(res, ref, s_min, rows=slice(None), erows=slice(None)):
    """Worst errors of S and rN (the latter in units of max(rN, 1), where the oracle's S >= 2 s_min) against the oracle."""
    S = torch.cat([res.bus_sens.cpu()[rows].reshape(-1), res.edge_sens.cpu()[erows].reshape(-1)])
    rn = torch.cat([res.bus_rn.cpu()[rows].reshape(-1), res.edge_rn.cpu()[erows].reshape(-1)])
    S0 = torch.cat([ref["bus_sens"][rows].reshape(-1), ref["edge_sens"][erows].reshape(-1)])
    rn0 = torch.cat([ref["bus_rn"][rows].reshape(-1), ref["edge_rn"][erows].reshape(-1)])
    kept, low = S0 >= 2 * s_min, S0 < s_min / 2
    assert bool((rn[low] == 0).all()) and bool((rn0[low] == 0).all())
    assert torch.equal(S == 0, S0 == 0)             # inactive measurements: exactly 0 on both sides
    return (S - S0).abs().max().item(), ((rn - rn0).abs() / rn0.clamp_min(1.0))[kept].max().item(), int((~kept & ~low).sum())


# ---- 1. clean data

@pytest.mark.parametrize("name", lc.ALL)
def test_clean_data_match_the_oracle_and_the_solve_is_wls_estimate_large(pkg, name):
    hb, b, ref = lc.batch(name), _device(name), cpu.clean(name)
    res = _run(pkg, b, s_min=cpu.S_MIN_CMP, **FIXED)
    plain = _run(pkg, b, "wls_estimate_large", **FIXED)
    for f in SOLVE_FIELDS:
        assert torch.equal(getattr(res, f), getattr(plain, f)), (name, f)
    sens, std = cpu.bounds(name)
    rn_b = cpu.rn_bound(name, cpu.S_MIN_CMP)
    e_s, e_rn, left_out = _compare_measurements(res, ref, cpu.S_MIN_CMP)
    e_std = (res.state_std.cpu() - ref["state_std"]).abs().max().item()
    e_lim = ((res.chi2_limit.cpu() - ref["chi2_limit"]).abs() / ref["chi2_limit"]).max().item()
    n, G = hb["nodes_per_graph"], hb["x"].shape[0] // hb["nodes_per_graph"]
    trace = res.bus_sens.reshape(G, -1).sum(1).index_add(0, b["edge_index"][0] // n, res.edge_sens.sum(1)).cpu()
    e_tr = (trace - res.dof.cpu().double()).abs().max().item()
    print(f"[bad-data large clean] {name}: S {e_s:.2e}/{sens:.2e} rN {e_rn:.2e}/{rn_b:.2e} state_std {e_std:.2e}/{std:.2e} chi2_limit {e_lim:.1e}/1e-12 "
          f"sum S - dof {e_tr:.1e}{'/1e-6' if name in cpu.TREES else ''} dof {res.dof.tolist()} suspect {res.suspect.tolist()} left out {left_out}")
    assert res.bus_rn.shape == (hb["x"].shape[0], 4) and res.edge_sens.shape == (hb["edge_attr"].shape[0], 2) and res.removed.shape == (G, 1)
    assert torch.equal(res.dof.cpu(), ref["dof"]) and torch.equal(res.suspect.cpu(), ref["suspect"])
    assert torch.equal(res.iterations.cpu(), ref["iterations"]) and torch.equal(res.status.cpu(), ref["status"])
    assert bool((res.n_removed == 0).all()) and bool((res.removed == -1).all())
    assert e_s <= sens and e_rn <= rn_b and e_std <= std and e_lim <= 1e-12
    if name in cpu.TREES:
        assert e_tr <= 1e-6
    assert bool((res.state_std[:, 1][b["x"][:, 9] != 0] == 0).all())


# ---- 2. gross errors

def _removals(pkg, name, ranks, graphs):
    hb, targets = cpu.corrupted(name, ranks)
    ref = cpu.removal_oracle(name, ranks)
    res = _run(pkg, _to_device(hb), **cpu.REMOVAL_KW[ranks])
    n = hb["nodes_per_graph"]
    ok = torch.tensor([g in graphs for g in range(len(ref["decisions"]))])
    assert [bool(v) for v in ok] == [bool(d) and g in graphs for g, d in enumerate(cpu.decided(ref))], "the CPU file's list of clear graphs"
    rows, erows = ok.repeat_interleave(n), ok[hb["edge_index"][0] // n]
    bound_st = lc.state_bound(cpu.removal_state_spread(name, ranks)[ok].max().item())
    rn_b = cpu.rn_bound(name, 1e-3)                  # (the default s_min)
    e_st = (res.state.cpu().double() - ref["state"])[rows].abs().max().item()
    e_rem = ((res.removed_rn.cpu() - ref["removed_rn"]).abs() / ref["removed_rn"].clamp_min(1.0))[ok].max().item()
    print(f"[bad-data large {len(ranks)} error(s)] {name}: targets {targets} removed {res.removed.tolist()} n_removed {res.n_removed.tolist()} compared {ok.tolist()}: "
          f"removed_rn {e_rem:.2e}/{rn_b:.2e} state {e_st:.2e}/{bound_st:.2e} iterations {res.iterations.tolist()} suspect {res.suspect.tolist()}")
    assert torch.equal(res.removed.cpu()[ok], ref["removed"][ok]) and torch.equal(res.n_removed.cpu()[ok], ref["n_removed"][ok])
    assert torch.equal(res.iterations.cpu()[ok], ref["iterations"][ok]) and torch.equal(res.status.cpu()[ok], ref["status"][ok])
    assert e_rem <= rn_b and e_st <= bound_st
    # the graphs left out ran too: no failure, a finite state
    assert bool((res.status != 2).all()) and bool(torch.isfinite(res.state).all()) and bool(torch.isfinite(res.objective).all())
    N = hb["x"].shape[0]
    for g in torch.nonzero(ok).flatten().tolist():           # a removed measurement is inactive in the final solve
        for t in res.removed[g, :int(res.n_removed[g])].tolist():
            got = res.bus_sens.reshape(-1)[t] if t < 4 * N else res.edge_sens.reshape(-1)[t - 4 * N]
            assert float(got) == 0.0


@pytest.mark.parametrize("name", lc.ALL)
def test_one_gross_error_per_graph_is_removed(pkg, name):
    G = len(lc.GRAPHS.get(name, (0, 1, 2)))
    _removals(pkg, name, (0,), [g for g in range(G) if (name, g) not in cpu.ONE_ERROR_LEFT_OUT])


@pytest.mark.parametrize("name", list(cpu.THREE_ERRORS))
def test_three_gross_errors_per_graph_are_removed_in_the_oracles_order(pkg, name):
    _removals(pkg, name, (0, 1, 2), cpu.THREE_ERRORS[name])


# ---- 3. the two forms on grids both serve

@functools.lru_cache(maxsize=None)
def _small_corrupted(name):
    b = wc.any_batch(name)
    targets = bo.largest_sensitivity_targets(b["x"], b["edge_index"], b["edge_attr"], b["stats"], b["nodes_per_graph"])
    x2, ea2 = bo.add_gross_errors(b["x"], b["edge_attr"], b["stats"], targets)
    return dict(b, x=x2, edge_attr=ea2), targets


@pytest.mark.parametrize("name", ["cigre14", "ober_sub", "n33"])
def test_both_forms_agree_on_small_grids(pkg, name):
    hb, targets = _small_corrupted(name)
    b = _to_device(hb)
    kw = dict(threshold=4.0, max_removals=3, **FIXED)
    lds, blocked = _run(pkg, b, "wls_bad_data", **kw), _run(pkg, b, **kw)
    e_st = (lds.state - blocked.state).abs().max().item()
    e_s = max((lds.bus_sens - blocked.bus_sens).abs().max().item(), (lds.edge_sens - blocked.edge_sens).abs().max().item())
    print(f"[bad-data large both forms] {name}: targets {targets} removed {blocked.removed[:, 0].tolist()} state {e_st:.2e}/{FORMS_STATE_BOUND:.1e} S {e_s:.2e}/{cpu.SENS_BOUND:.0e}")
    assert torch.equal(lds.removed, blocked.removed) and torch.equal(lds.n_removed, blocked.n_removed) and bool((blocked.n_removed >= 1).all())
    assert torch.equal(lds.iterations, blocked.iterations) and torch.equal(lds.status, blocked.status) and torch.equal(lds.dof, blocked.dof)
    assert e_st <= FORMS_STATE_BOUND and e_s <= cpu.SENS_BOUND


# ---- 4. reproducibility

def _static_copy(b):
    return dict(b, x=b["x"].clone(), edge_attr=b["edge_attr"].clone())


def test_runs_positions_group_caps_and_a_failing_graph_agree_bitwise(pkg):
    hb = _with_ptr(cpu.corrupted("n179t")[0])
    b = _to_device({k: v for k, v in hb.items() if k != "graph_ptr"})
    kw = dict(threshold=4.0, max_removals=2, max_iter=6, tol=1e-6)
    base = _run(pkg, b, **kw)
    assert bool((base.n_removed == 1).all()) and bool((base.status == 0).all())
    assert _equal(_run(pkg, b, **kw), base)
    for groups in (1, 2):
        assert _equal(_run(pkg, b, max_groups=groups, **kw), base)
    # the graphs in another order (through graph_ptr): every graph's outputs are its own
    order = [2, 0, 1]
    moved = mc.reordered(hb, order)
    res = _run(pkg, _to_device(moved), **kw)
    for pos, g in enumerate(order):
        assert _equal(_graph_view(res, moved, pos), _graph_view(base, hb, g)), g
    # a failing graph in front, on ONE workgroup: a NaN reading makes graph 0's first pivot test fail; the others are untouched
    x = b["x"].clone()
    x[0, 0] = float("nan")
    res = _run(pkg, dict(b, x=x), max_groups=1, **kw)
    print(f"[bad-data large failing] status {res.status.tolist()} iterations {res.iterations.tolist()} n_removed {res.n_removed.tolist()}")
    assert int(res.status[0]) == 2 and int(res.iterations[0]) == 0 and int(res.n_removed[0]) == 0 and int(res.suspect[0]) == 0
    n = hb["nodes_per_graph"]
    assert bool((res.state_std[:n] == 0).all()) and bool((res.bus_sens[:n] == 0).all()) and bool((res.bus_rn[:n] == 0).all())
    for g in (1, 2):
        assert _equal(_graph_view(res, hb, g), _graph_view(base, hb, g)), g


def test_replays_agree_bitwise(pkg):
    b, other = _to_device(cpu.corrupted("n100")[0]), _device("n100")
    kw = dict(threshold=4.0, max_removals=2, max_iter=6, tol=1e-6)
    eager, eager_other = _run(pkg, b, **kw), _run(pkg, other, **kw)
    assert bool((eager.n_removed == 1).all()) and bool((eager_other.n_removed == 0).all()) and not torch.equal(eager.state, eager_other.state)
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


# ---- 5. batches that mix bus counts

@functools.lru_cache(maxsize=None)
def _mix(pkg):
    """cigre14, ober_sub and ober179 in one batch (179, 70, 70 and 15 buses; every graph has the batch's V_lv), one gross error per graph."""
    hb = pkg.synthetic.make_batch(["cigre14", "ober_sub", "ober179"], 4, seed=0)
    hb = _with_ptr(dict(hb, nodes_per_graph=179))
    assert sorted(hb["sizes"]) == [15, 70, 70, 179] and len({float(hb["x"][p:q, 8].min()) for p, q in zip(hb["graph_ptr"][:-1], hb["graph_ptr"][1:])}) == 1
    bad, ids = pkg.synthetic.corrupt_measurements(hb, per_graph=1, sigmas=25.0, seed=3)
    return dict(hb, x=bad["x"], edge_attr=bad["edge_attr"]), ids


def test_a_graph_of_a_mix_is_the_graph_alone_and_one_above_the_bound_is_refused_alone(pkg):
    hb, ids = _mix(pkg)
    b = _to_device(hb)
    kw = dict(threshold=4.0, max_removals=2, **FIXED)
    base = _run(pkg, b, **kw)
    print(f"[bad-data large mix] sizes {hb['sizes']} injected {ids[:, 0].tolist()} removed {base.removed.tolist()} status {base.status.tolist()} dof {base.dof.tolist()}")
    assert bool((base.status == 1).all()) and base.objective.shape == (4, 2)
    for g in range(4):
        alone = mc.reordered(hb, [g])
        res = _run(pkg, _to_device(alone), **kw)             # (the same bound: 179)
        assert _equal(_graph_view(res, alone, 0), _graph_view(base, hb, g)), g
    res = _run(pkg, b, nodes_per_graph=70, **kw)
    for g, n in enumerate(hb["sizes"]):
        rows, erows = mc.graph_rows(hb, g)
        if n > 70:
            assert int(res.status[g]) == 2 and int(res.iterations[g]) == 0 and bool((res.objective[g] == 0).all())
            assert int(res.dof[g]) == 0 and math.isinf(float(res.chi2_limit[g])) and int(res.suspect[g]) == 0 and int(res.n_removed[g]) == 0
            assert res.removed[g].tolist() == [-1, -1] and res.removed_rn[g].tolist() == [0.0, 0.0]
            for t in (res.state, res.bus_rn, res.bus_sens, res.state_std):
                assert bool((t[rows] == 0).all())
            assert bool((res.edge_rn[erows] == 0).all()) and bool((res.edge_sens[erows] == 0).all())
        else:
            assert _equal(_graph_view(res, hb, g), _graph_view(base, hb, g)), g


# ---- 6. refusals

def test_refusals(pkg):
    L, lib, est = pkg._lib.lib(), pkg._lib, pkg.estimator
    stream = lib.stream_ptr(torch.device(DEV))
    buf = torch.zeros(4096, dtype=torch.float64, device=DEV)
    a = lib.WlsBadDataArgs()
    s = a.solve
    for f in ("x", "edge_attr", "x_mean", "x_std", "edge_mean", "edge_std", "efrom", "eto", "inc_rowptr", "inc_ent", "state", "objective",
              "iterations", "status", "last_step", "vminmax"):
        setattr(s, f, buf.data_ptr())
    for f in ("dof", "chi2_limit", "suspect", "removed", "removed_rn", "n_removed", "bus_rn", "bus_sens", "edge_rn", "edge_sens", "state_std"):
        setattr(a, f, buf.data_ptr())
    s.ldx, s.ldea, s.n_nodes, s.n_edges, s.nodes_per_graph, s.max_iter, s.tol = 11, 13, 100, 99, 100, 5, 1e-6
    a.threshold, a.s_min, a.z_p, a.max_removals = 3.0, 1e-3, 1.64, 1
    # every refusal below comes before any launch: the pointers above are never read
    need = L.dss2_wls_large_workspace_bytes(100, L.dss2_wls_large_groups(C.byref(s)))
    assert need == 8 * cpu.graph_doubles(200)
    assert L.dss2_wls_bad_data(C.byref(a), stream) == 2 and b"LDS" in L.dss2_last_error() and b"100 buses" in L.dss2_last_error()    # no workspace: the LDS form
    a.workspace, a.workspace_bytes = buf.data_ptr(), need - 8
    assert L.dss2_wls_bad_data(C.byref(a), stream) == 2 and b"workspace has" in L.dss2_last_error()
    a.workspace, a.workspace_bytes = buf.data_ptr(), 0
    assert L.dss2_wls_bad_data(C.byref(a), stream) == 2 and b"workspace has" in L.dss2_last_error()
    a.workspace, a.workspace_bytes = buf.data_ptr() + 8, need
    assert L.dss2_wls_bad_data(C.byref(a), stream) == 2 and b"aligned" in L.dss2_last_error()
    a.workspace = buf.data_ptr()
    a.threshold = 0.0
    assert L.dss2_wls_bad_data(C.byref(a), stream) == 2 and b"threshold" in L.dss2_last_error()
    a.threshold = 3.0
    s.n_nodes, s.n_edges, s.nodes_per_graph = 257, 256, 257
    assert L.dss2_wls_bad_data(C.byref(a), stream) == 2 and b"at most 256" in L.dss2_last_error()
    torch.cuda.synchronize()
    x, ei, ea = torch.zeros(257, 11, device=DEV), torch.zeros(2, 256, dtype=torch.int64, device=DEV), torch.zeros(256, 13, device=DEV)
    stats = _device("n100")["stats"]
    with pytest.raises(NotImplementedError, match="at most 256 buses per graph, got 257"):
        est.wls_bad_data_large(x, ei, ea, *stats, 257)
    with pytest.raises(ValueError, match="threshold"):
        _run(pkg, _device("n100"), threshold=0.0)


# ---- 7. the runner

def test_evaluate_wls_takes_the_large_form_on_request(pkg):
    loader, stats, injected = [], None, 0
    for seed in (21, 22):
        hb = pkg.synthetic.make_batch(["ober179"], 2, seed=seed, stats=stats)
        stats = hb["stats"] if stats is None else stats
        bad, ids = pkg.synthetic.corrupt_measurements(dict(hb, nodes_per_graph=179), per_graph=1, sigmas=25.0, seed=seed)
        injected += ids.numel()
        loader.append({k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in bad.items() if k not in ("stats", "graph_ptr")})
    dstats = tuple(s.to(DEV) for s in stats)
    got = pkg.runner.evaluate_wls(loader, dstats, 179, bad_data=dict(threshold=4.0, max_removals=3, large=True))
    print(f"[bad-data large evaluate] removed {got['wls_removed']} ({injected} injected) suspect {got['wls_suspect']} not converged {got['wls_not_converged']} rmse_v {got['rmse_v']:.4g}")
    assert set(got) == set(pkg.data.EVAL_METRICS) | {"wls_mean_iterations", "wls_not_converged", "wls_suspect", "wls_removed"}
    assert len(pkg.data.EVAL_METRICS) == 10 and got["wls_removed"] > 0 and all(math.isfinite(got[k]) for k in pkg.data.EVAL_METRICS)
    auto = pkg.runner.evaluate_wls(loader, dstats, 179, bad_data=dict(threshold=4.0, max_removals=3, large="auto"))
    assert auto == got
    for kw in (dict(threshold=4.0, max_removals=3), dict(threshold=4.0, max_removals=3, large=False)):
        with pytest.raises(NotImplementedError, match="at most 99 buses per graph, got 179"):
            pkg.runner.evaluate_wls(loader, dstats, 179, bad_data=kw)
    small = wc.any_batch("cigre14")
    sl = [{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in small.items() if k != "stats"}]
    sst = tuple(s.to(DEV) for s in small["stats"])
    assert pkg.runner.evaluate_wls(sl, sst, 15, bad_data=dict(threshold=4.0, large="auto")) == pkg.runner.evaluate_wls(sl, sst, 15, bad_data=dict(threshold=4.0))
