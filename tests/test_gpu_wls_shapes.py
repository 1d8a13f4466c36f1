"""GPU: estimator.wls_estimate and estimator.wls_bad_data (csrc/dss2_wls_core.hpp, dss2_wls_solve.hip, dss2_wls_bad_data.hip) against
the fp64 oracles on the inputs of tests/wls_edge_cases.py: the kernels' size limits (32, 64, 65 and 99 buses, 100 refused, one bus
without a branch) and measurement sets the grids never produce (theta readings away from the slack, no slack, two slacks, a slack at the
last bus, every flow measured, weights clamped at 0, a self loop and a tripled branch, an isolated bus, weights other than (1, 1, 1),
a failure at an interior pivot, non-finite inputs, the arg-max won by a thread of wave 1, five removals in 64 slots, an exact tie).

Bounds: those of tests/test_gpu_wls_solve.py and tests/test_gpu_wls_bad_data.py, unchanged -- state 5e-7, objective 1e-6 relative,
S 2e-7, rN 1e-4 max(rN, 1) where the oracle's S >= 2 s_min, state_std 3.44e-9, chi2_limit 1e-12 relative; status, iterations, dof and
suspect equal.  tests/test_wls_edge_cases_cpu.py holds two fp64 routes of the oracle to one eighth of each on every case here.
Every test prints its errors beside the bounds (run with -s).

Measured on the MI355X, worst per case (bounds in brackets; the state error is the fp32 rounding of the output, 2^-24 at 1.0):
                     state, 1 / 3 / 8 iterations    objective   S         rN        state_std
                     [5e-7]                         [1e-6]      [2e-7]    [1e-4]    [3.44e-9]
  n32                5.9e-08 / 5.9e-08 / 5.9e-08    1.6e-10     5.0e-11   2.2e-09   6.5e-14
  n64                5.8e-08 / 5.8e-08 / 5.8e-08    2.9e-09     3.0e-10   3.4e-08   1.1e-12
  n65                5.7e-08 / 5.9e-08 / 5.8e-08    4.2e-10     1.2e-10   9.3e-09   2.4e-13
  n99                5.9e-08 / 5.9e-08 / 5.7e-08    5.4e-09     1.7e-08   1.1e-06   3.5e-10
  pmu                5.9e-08 / 5.6e-08 / 5.9e-08    1.0e-07     8.0e-09   2.0e-08   1.4e-10
  pmu_star           5.7e-08 / 5.8e-08 / 5.8e-08    9.3e-10     3.6e-10   1.3e-08   2.4e-12
  no_slack           5.7e-08 / 5.8e-08 / 5.8e-08    1.6e-09     3.8e-09   1.4e-07   1.4e-11
  two_slack          5.1e-08 / 5.2e-08 / 5.2e-08    5.7e-10     1.3e-10   4.1e-09   3.5e-13
  slack_last         6.0e-08 / 5.9e-08 / 5.9e-08    8.5e-10     8.8e-10   2.2e-08   1.9e-12
  all_flows          5.3e-08 / 5.6e-08 / 5.7e-08    4.3e-09     2.0e-09   2.8e-07   1.3e-12
  clamped            4.8e-08 / 5.9e-08 / 5.9e-08    1.3e-08     2.9e-09   1.8e-08   9.7e-12
  multigraph         5.6e-08 / 5.9e-08 / 5.9e-08    7.2e-11     3.0e-11   7.5e-10   1.1e-14
  isolated_pmu       5.0e-08 / 4.2e-08 / 4.2e-08    1.1e-09     1.6e-09   2.5e-08   1.2e-11
  tie                5.8e-08 / 5.2e-08 / 5.4e-08    9.6e-11     3.4e-12   1.3e-11   4.9e-15
  star10_weighted    5.8e-08 / 5.5e-08 / 5.5e-08    6.5e-08     1.8e-08   1.2e-07   2.5e-10
  cigre14_weighted   5.7e-08 / 5.9e-08 / 6.0e-08    1.2e-10     3.2e-11   2.4e-11   4.4e-13
  (objective: the worst is after the first iteration everywhere.)  Status, iterations, dof, suspect and chi2_limit (<= 1.8e-16) equal on
  every case; at tol = 1e-6 every decision equals the oracle's, the 3 of 50 graphs left out included; 290 of 3062 active measurements
  have S within a factor 2 of s_min and are left out of the rN comparison.
  n99, one +25 sigma error per graph (P of bus 0; P flow of branch 88, from-end 70; Q of bus 89): each is the first and only removal,
      removed_rn 4.9e-11 [1e-4], state 5.9e-8 [5e-7], after the removal S 2.4e-8 [2e-7] and rN 1.4e-6 [1e-4]
  n33, five errors on graph 2, max_removals = 64: the oracle's five ids in its order, removed_rn 6.2e-9, state 6.0e-8, S 1.0e-8, rN 4.1e-7
  tie: both flows' rows bit-equal, the smaller id removed, rN within 2.0e-13 relative of the oracle's
  n1:  v within 5.2e-8 of the reading [2^-24], S within 2e-16 of 0, state_std = w^-1/2 to the bit
"""
import ctypes as C
import functools
import importlib

import pytest
import torch

import wls_bad_data_oracle as bo
import wls_edge_cases as ec
import wls_oracle as wo
from conftest import PKG_NAME
from test_gpu_wls_bad_data import _compare_measurements, _decided      # the existing comparison rules, as they are

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STATE_BOUND, OBJ_BOUND, TOL = 5e-7, 1e-6, 1e-6
SENS_BOUND, RN_BOUND, STD_BOUND = 2e-7, 1e-4, 8 * 4.3e-10
FIXED = dict(max_iter=8, tol=0.0)
SOLVE_FIELDS = ("state", "objective", "iterations", "status", "last_step")
PER_BUS, PER_EDGE = ("state", "bus_rn", "bus_sens", "state_std"), ("edge_rn", "edge_sens")
ALL = slice(None)


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
    return _to_device(ec.batch(name))


def _estimate(pkg, b, **kw):
    return pkg.estimator.wls_estimate(b["x"], b["edge_index"], b["edge_attr"], *b["stats"], b["nodes_per_graph"], **kw)


def _bad_data(pkg, b, **kw):
    return pkg.estimator.wls_bad_data(b["x"], b["edge_index"], b["edge_attr"], *b["stats"], b["nodes_per_graph"], **kw)


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))


def _errors(res, ref, rows=ALL, graphs=ALL):
    st = (res.state.cpu().double() - ref["state"])[rows].abs().max().item()
    ob = ((res.objective.cpu() - ref["objective"]).abs() / ref["objective"].abs())[graphs].max().item()
    return st, ob


# ---- wls_estimate ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iter", [1, 3, 8])
@pytest.mark.parametrize("name", ec.SOLVABLE)
def test_parity_at_fixed_trip_counts(pkg, name, max_iter):
    ref = ec.oracle_solve(name, max_iter, 0.0)
    b, w = _device(name), ec.weights_of(name)
    res = _estimate(pkg, b, max_iter=max_iter, tol=0.0, weights=w)
    st, ob = _errors(res, ref)
    print(f"[wls shapes parity] {name} max_iter={max_iter}: state {st:.2e}/{STATE_BOUND:.0e} objective {ob:.2e}/{OBJ_BOUND:.0e} "
          f"iterations {res.iterations.tolist()} status {res.status.tolist()}")
    assert torch.equal(res.iterations.cpu(), ref["iterations"]) and torch.equal(res.status.cpu(), ref["status"])
    assert bool((res.status == 1).all()) and bool((res.iterations == max_iter).all())
    assert st <= STATE_BOUND, (st, STATE_BOUND)
    assert ob <= OBJ_BOUND, (ob, OBJ_BOUND)
    # the same input through the other entry: the five solve fields to the bit
    other = _bad_data(pkg, b, max_iter=max_iter, tol=0.0, weights=w)
    for f in SOLVE_FIELDS:
        assert torch.equal(getattr(other, f), getattr(res, f)), f


def test_convergence_decisions_match_the_oracle(pkg):
    total = excluded = 0
    for name in ec.SOLVABLE:
        ref = ec.oracle_solve(name, 12, TOL)
        b, w = _device(name), ec.weights_of(name)
        res = _estimate(pkg, b, max_iter=12, tol=TOL, weights=w)
        skip = wo.undecided(ref, TOL)
        total, excluded = total + skip.numel(), excluded + int(skip.sum())
        print(f"[wls shapes convergence] {name}: iterations {res.iterations.tolist()} oracle {ref['iterations'].tolist()} status {res.status.tolist()} "
              f"last_step {['%.1e' % v for v in res.last_step.tolist()]} excluded {skip.tolist()}")
        keep = ~skip
        assert torch.equal(res.status.cpu()[keep], ref["status"][keep]) and torch.equal(res.iterations.cpu()[keep], ref["iterations"][keep])
        assert bool((ref["status"] == 0).all())
        assert (res.state.cpu().double() - ref["state"])[keep.repeat_interleave(b["nodes_per_graph"])].abs().max() <= STATE_BOUND
        other = _bad_data(pkg, b, max_iter=12, tol=TOL, weights=w)
        for f in SOLVE_FIELDS:
            assert torch.equal(getattr(other, f), getattr(res, f)), (name, f)
    print(f"[wls shapes convergence] {excluded} of {total} graphs decide within a factor 4 of tol and are left out")
    assert excluded <= 0.1 * total, (excluded, total)


# ---- wls_bad_data on clean data -------------------------------------------------------------------------------------------------
def test_bad_data_parity_on_clean_data(pkg):
    near = active = 0
    for name in ec.SOLVABLE:
        ref, b = ec.oracle_clean(name), ec.batch(name)
        dev = _device(name)
        res = _bad_data(pkg, dev, weights=ec.weights_of(name), **FIXED)
        e_s, e_rn, left_out = _compare_measurements(res, ref, ALL, ALL)
        e_std = (res.state_std.cpu() - ref["state_std"]).abs().max().item()
        e_lim = ((res.chi2_limit.cpu() - ref["chi2_limit"]).abs() / ref["chi2_limit"]).max().item()
        e_st = (res.state.cpu().double() - ref["state"]).abs().max().item()
        n, G = b["nodes_per_graph"], b["num_graphs"]
        trace = res.bus_sens.reshape(G, -1).sum(1).index_add(0, dev["edge_index"][0] // n, res.edge_sens.sum(1)).cpu()
        e_tr = (trace - res.dof.cpu().double()).abs().max().item()
        near, active = near + left_out, active + int((ref["bus_sens"] != 0).sum()) + int((ref["edge_sens"] != 0).sum())
        print(f"[bad-data shapes parity] {name}: S {e_s:.2e}/{SENS_BOUND:.0e} rN {e_rn:.2e}/{RN_BOUND:.0e} state_std {e_std:.2e}/{STD_BOUND:.2e} chi2_limit {e_lim:.1e}/1e-12 "
              f"state {e_st:.2e}/{STATE_BOUND:.0e} sum S - dof {e_tr:.1e}/1e-6 dof {res.dof.tolist()} suspect {res.suspect.tolist()} left out {left_out}")
        assert torch.equal(res.dof.cpu(), ref["dof"]) and torch.equal(res.suspect.cpu(), ref["suspect"])
        assert torch.equal(res.iterations.cpu(), ref["iterations"]) and torch.equal(res.status.cpu(), ref["status"])
        assert e_s <= SENS_BOUND and e_rn <= RN_BOUND and e_std <= STD_BOUND and e_lim <= 1e-12 and e_st <= STATE_BOUND and e_tr <= 1e-6
        assert bool((res.state_std[:, 1][dev["x"][:, 9] != 0] == 0).all())
        # inactive measurements: exactly 0 on both sides (an active one may have S = 0 up to rounding: the isolated bus's readings)
        _, R, _, eR = wo.denormalised(b["x"], b["edge_attr"], b["stats"])
        for got, want, off in ((res.bus_sens.cpu(), ref["bus_sens"], R <= 0), (res.edge_sens.cpu(), ref["edge_sens"], eR <= 0)):
            assert bool((got[off] == 0).all()) and bool((want[off] == 0).all()) and bool((got[~off] != 0).any())
        assert bool((res.n_removed == 0).all()) and bool((res.removed == -1).all())
    # dof from the measurements that are active and the states that are free (star10: 26 measurements, 20 states)
    dof = lambda name: _bad_data(pkg, _device(name), **FIXED).dof.tolist()
    assert dof("clamped") == [27 - 3 - 19] * 3 and dof("no_slack") == [29 - 20] * 3 and dof("two_slack") == [18 - 10] * 3
    print(f"[bad-data shapes parity] {near} of {active} active measurements have S within a factor 2 of s_min and are left out of the rN comparison")
    assert near <= 0.1 * active


# ---- graphs that fail ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.FAILING)
def test_a_failing_graph_fails_alone(pkg, name):
    b, healthy = _device(name), _device(ec.HEALTHY[name])
    n, g = b["nodes_per_graph"], ec.FAILING_GRAPH
    rows, erows = ec.graph_rows(b, g)
    others = torch.ones(3, dtype=torch.bool, device=DEV)
    others[g] = False
    orow, oedge = others.repeat_interleave(n), ~erows
    init = torch.stack([torch.full((3 * n,), 0.98, device=DEV), torch.full((3 * n,), -0.01, device=DEV) * (b["x"][:, 9] == 0)], 1)
    kw = dict(threshold=4.0, max_removals=2, max_iter=12, tol=TOL)
    ref_o = bo.bad_data(*ec.args(ec.batch(name)), **kw)
    for start in (None, init):
        want = torch.tensor([1.0, 0.0], device=DEV).expand(n, 2) if start is None else start[rows]
        res, ok = _estimate(pkg, b, init=start, max_iter=12, tol=TOL), _estimate(pkg, healthy, init=start, max_iter=12, tol=TOL)
        print(f"[wls shapes failing] {name}: wls_estimate status {res.status.tolist()} iterations {res.iterations.tolist()} objective of the failing graph {res.objective[g].tolist()}")
        assert res.status.tolist() == [0, 2, 0] and int(res.iterations[g]) == 0 and float(res.last_step[g]) == 0.0
        assert torch.equal(res.state[rows], want) and ok.status.tolist() == [0, 0, 0]
        assert torch.equal(res.state[orow], ok.state[orow])
        for f in SOLVE_FIELDS[1:]:
            assert torch.equal(getattr(res, f)[others], getattr(ok, f)[others]), f
        assert bool(torch.isfinite(res.objective[others]).all())
        res, ok = _bad_data(pkg, b, init=start, **kw), _bad_data(pkg, healthy, init=start, **kw)
        print(f"[wls shapes failing] {name}: wls_bad_data status {res.status.tolist()} dof {res.dof.tolist()} suspect {res.suspect.tolist()} n_removed {res.n_removed.tolist()}")
        assert res.status.tolist() == [0, 2, 0] and int(res.iterations[g]) == 0 and int(res.n_removed[g]) == 0 and bool((res.removed[g] == -1).all())
        assert torch.equal(res.state[rows], want)
        for t in (res.bus_rn[rows], res.bus_sens[rows], res.state_std[rows], res.edge_rn[erows], res.edge_sens[erows]):
            assert bool((t == 0).all())
        for f in res._fields:
            sel = orow if f in PER_BUS else (oedge if f in PER_EDGE else others)
            assert torch.equal(getattr(res, f)[sel], getattr(ok, f)[sel]), f
            assert not bool(torch.isnan(getattr(res, f)[sel].double()).any()), f
        if start is None:
            assert torch.equal(res.dof.cpu(), ref_o["dof"]) and torch.equal(res.suspect.cpu(), ref_o["suspect"]) and torch.equal(res.status.cpu(), ref_o["status"])


# ---- removals -------------------------------------------------------------------------------------------------------------------
def _compare_removals(res, ref, hb):
    ok = _decided(ref, 4.0)
    n = hb["nodes_per_graph"]
    rows, erows = ok.repeat_interleave(n), ok[hb["edge_index"][0] // n]
    e_st = (res.state.cpu().double() - ref["state"])[rows].abs().max().item()
    e_rem = ((res.removed_rn.cpu() - ref["removed_rn"]).abs() / ref["removed_rn"].clamp_min(1.0))[ok].max().item()
    e_s, e_rn, _ = _compare_measurements(res, ref, rows, erows)
    return ok, e_st, e_rem, e_s, e_rn


def test_the_arg_max_is_won_in_either_wave(pkg):
    hb, ids, ref = ec.cross_wave()
    clean = ec.oracle_clean("n99")
    res = _bad_data(pkg, _to_device(hb), threshold=4.0, max_removals=2, **FIXED)
    ok, e_st, e_rem, e_s, e_rn = _compare_removals(res, ref, hb)
    back = (res.state.cpu().double() - clean["state"]).abs().max().item()
    print(f"[bad-data shapes waves] injected {ids} removed {res.removed[:, 0].tolist()} rN {['%.2f' % v for v in res.removed_rn[:, 0].tolist()]} n_removed {res.n_removed.tolist()} "
          f"decided {ok.tolist()}: removed_rn {e_rem:.2e}/{RN_BOUND:.0e} state {e_st:.2e}/{STATE_BOUND:.0e} after the removal S {e_s:.2e}/{SENS_BOUND:.0e} "
          f"rN {e_rn:.2e}/{RN_BOUND:.0e}; from the solve of the clean data WITH the measurement {back:.2e}")
    assert bool(ok.all()) and ref["removed"][:, 0].tolist() == ids
    assert res.removed[:, 0].tolist() == ids and res.n_removed.tolist() == [1, 1, 1] and bool((res.removed[:, 1] == -1).all())
    assert torch.equal(res.iterations.cpu(), ref["iterations"]) and torch.equal(res.dof.cpu(), ref["dof"]) and torch.equal(res.suspect.cpu(), ref["suspect"])
    assert e_rem <= RN_BOUND and e_st <= STATE_BOUND and e_s <= SENS_BOUND and e_rn <= RN_BOUND
    N = hb["x"].shape[0]
    for t in ids:
        assert float(res.bus_sens.reshape(-1)[t] if t < 4 * N else res.edge_sens.reshape(-1)[t - 4 * N]) == 0.0


def test_five_removals_in_64_slots(pkg):
    hb, ids, ref = ec.five_errors()
    g = ec.FIVE_ERRORS_GRAPH
    b = _to_device(hb)
    res = _bad_data(pkg, b, threshold=4.0, max_removals=64, **FIXED)
    ok, e_st, e_rem, e_s, e_rn = _compare_removals(res, ref, hb)
    print(f"[bad-data shapes five] injected {ids} removed {res.removed[g, :6].tolist()} oracle {ref['removed'][g, :6].tolist()} rN {['%.2f' % v for v in res.removed_rn[g, :6].tolist()]} "
          f"removed_rn {e_rem:.2e}/{RN_BOUND:.0e} state {e_st:.2e}/{STATE_BOUND:.0e} S {e_s:.2e}/{SENS_BOUND:.0e} rN {e_rn:.2e}/{RN_BOUND:.0e}")
    assert bool(ok.all()) and res.removed.shape == (3, 64) and res.removed_rn.shape == (3, 64)
    assert res.n_removed.tolist() == [5 if k == g else 0 for k in range(3)]
    assert torch.equal(res.removed.cpu(), ref["removed"]) and res.removed[g, :5].tolist() == ref["removed"][g, :5].tolist()
    assert bool((res.removed[g, 5:] == -1).all()) and bool((res.removed_rn[g, 5:] == 0.0).all()) and bool((res.removed_rn[g, :5] > 4.0).all())
    assert torch.equal(res.iterations.cpu(), ref["iterations"]) and torch.equal(res.dof.cpu(), ref["dof"]) and torch.equal(res.suspect.cpu(), ref["suspect"])
    assert e_rem <= RN_BOUND and e_st <= STATE_BOUND and e_s <= SENS_BOUND and e_rn <= RN_BOUND
    five = _bad_data(pkg, b, threshold=4.0, max_removals=5, **FIXED)
    assert five.removed.shape == (3, 5)
    for f in res._fields:
        got, want = getattr(five, f), getattr(res, f)
        assert torch.equal(got, want[:, :5] if f in ("removed", "removed_rn") else want), f


def test_an_exact_tie_goes_to_the_smaller_id(pkg):
    hb, ids, ref = ec.tied()
    b = _to_device(hb)
    first = _bad_data(pkg, b, **FIXED)
    res = _bad_data(pkg, b, threshold=4.0, max_removals=1, **FIXED)
    for k, (lo, hi) in enumerate(ids):
        rn, S = first.edge_rn[2 * k:2 * k + 2], first.edge_sens[2 * k:2 * k + 2]
        winner, best, second = ref["decisions"][k][0]
        e = abs(float(rn[0, 1]) - best) / best
        print(f"[bad-data shapes tie] graph {k}: rN {rn.tolist()} S {S.tolist()} removed {int(res.removed[k, 0])} of {lo}, {hi}; oracle {best:.12g}, {second:.12g}: {e:.2e}/{RN_BOUND:.0e}")
        assert torch.equal(rn[0], rn[1]) and torch.equal(S[0], S[1])
        assert float(rn[0, 1]) == float(torch.cat([first.bus_rn[2 * k:2 * k + 2].reshape(-1), rn.reshape(-1)]).max()) > 4.0
        assert int(res.removed[k, 0]) == lo < hi and int(res.n_removed[k]) == 1
        assert winner in (lo, hi) and abs(best - second) <= 1e-9 * best and e <= RN_BOUND
        assert float(res.removed_rn[k, 0]) == float(rn[0, 1])


# ---- the limits -----------------------------------------------------------------------------------------------------------------
def test_limits_and_refusals(pkg):
    est = pkg.estimator
    L, lib = pkg._lib.lib(), pkg._lib
    cap = 160 * 1024
    assert est.max_nodes_per_graph() == 99
    assert (L.dss2_wls_solve_lds_bytes(99), L.dss2_wls_bad_data_lds_bytes(99)) == (162496, 162816)
    assert L.dss2_wls_bad_data_lds_bytes(99) <= cap < L.dss2_wls_solve_lds_bytes(100) < L.dss2_wls_bad_data_lds_bytes(100)
    x, ea = torch.zeros(100, 11, device=DEV), torch.zeros(99, 13, device=DEV)
    ei = torch.stack([torch.arange(99, device=DEV), torch.arange(1, 100, device=DEV)])
    stats = _device("n99")["stats"]
    for entry in (est.wls_estimate, est.wls_bad_data):
        with pytest.raises(NotImplementedError, match="at most 99 buses per graph, got 100"):
            entry(x, ei, ea, *stats, 100)
    stream = lib.stream_ptr(torch.device(DEV))
    a = lib.WlsSolveArgs()
    a.n_nodes, a.n_edges, a.nodes_per_graph, a.max_iter, a.tol = 100, 99, 100, 5, 1e-6
    assert L.dss2_wls_solve(C.byref(a), stream) == 2 and b"LDS" in L.dss2_last_error() and b"100 buses" in L.dss2_last_error()
    b = lib.WlsBadDataArgs()
    b.solve.n_nodes, b.solve.n_edges, b.solve.nodes_per_graph, b.solve.max_iter, b.solve.tol = 100, 99, 100, 5, 1e-6
    assert L.dss2_wls_bad_data(C.byref(b), stream) == 2 and b"LDS" in L.dss2_last_error() and b"100 buses" in L.dss2_last_error()
    torch.cuda.synchronize()


def _shifted(removed, bus_shift, edge_shift, first_edge_id):
    return torch.where(removed < 0, removed, torch.where(removed < first_edge_id, removed + bus_shift, removed + edge_shift))


@pytest.mark.parametrize("name", ["n32", "n99"])
def test_bit_exact_properties_at_the_limits(pkg, name):
    """Two runs, one workgroup striding over all graphs (rem and the slack flags reused), and the batch behind a graph that fails."""
    if name == "n99":
        hb = ec.cross_wave()[0]
    else:
        h = ec.batch(name)
        x2, ea2 = bo.add_gross_errors(h["x"], h["edge_attr"], h["stats"], bo.largest_sensitivity_targets(*ec.args(h)))
        hb = dict(h, x=x2, edge_attr=ea2)
    b, behind = _to_device(hb), _to_device(ec.preceded_by_failing_graph(hb))
    n, N, E0 = hb["nodes_per_graph"], hb["x"].shape[0], int(ec.graph_rows(hb, 0)[1].sum())
    # wls_estimate
    kw = dict(max_iter=10, tol=TOL)
    res = _estimate(pkg, b, **kw)
    assert _equal(_estimate(pkg, b, **kw), res) and _equal(_estimate(pkg, b, max_groups=1, **kw), res) and bool((res.status == 0).all())
    for groups in (0, 1):
        long = _estimate(pkg, behind, max_groups=groups, **kw)
        assert int(long.status[0]) == 2 and torch.equal(long.state[n:], res.state)
        for f in SOLVE_FIELDS[1:]:
            assert torch.equal(getattr(long, f)[1:], getattr(res, f)), f
    # wls_bad_data, with removals
    kw = dict(threshold=4.0, max_removals=2, max_iter=10, tol=TOL)
    res = _bad_data(pkg, b, **kw)
    print(f"[bad-data shapes bits] {name}: n_removed {res.n_removed.tolist()} removed {res.removed[:, 0].tolist()}")
    assert bool((res.n_removed >= 1).all()) and bool((res.status == 0).all())
    assert _equal(_bad_data(pkg, b, **kw), res) and _equal(_bad_data(pkg, b, max_groups=1, **kw), res)
    for groups in (0, 1):
        long = _bad_data(pkg, behind, max_groups=groups, **kw)
        assert int(long.status[0]) == 2 and int(long.n_removed[0]) == 0
        for f in res._fields:
            got = getattr(long, f)
            got = got[n:] if f in PER_BUS else (got[E0:] if f in PER_EDGE else got[1:])
            want = _shifted(res.removed, 4 * n, 4 * n + 2 * E0, 4 * N) if f == "removed" else getattr(res, f)
            assert torch.equal(got, want), f


def test_one_bus_graphs_without_branches(pkg):
    """E = 0 for the whole batch: no edge array exists.  The answer is known: v = the V reading after one update, theta = 0 (the slack),
    one measurement for one free state."""
    hb = ec.batch("n1")
    b = _device("n1")
    assert b["edge_index"].shape == (2, 0) and b["edge_attr"].shape == (0, 13)
    Z, R = (t[:, 0] for t in wo.denormalised(hb["x"], hb["edge_attr"], hb["stats"])[:2])
    one = _estimate(pkg, b, max_iter=1, tol=0.0)
    e_v = (one.state[:, 0].cpu().double() - Z).abs().max().item()
    print(f"[wls shapes one bus] v against the reading {e_v:.2e}/{2.0 ** -24:.2e} objective {one.objective.tolist()}")
    assert e_v <= 2.0 ** -24 and bool((one.state[:, 1] == 0).all()) and one.iterations.tolist() == [1, 1, 1] and one.status.tolist() == [1, 1, 1]
    assert float(one.objective.abs().max()) <= 1e-20
    done = _estimate(pkg, b, max_iter=5, tol=TOL)
    assert done.status.tolist() == [0, 0, 0] and done.iterations.tolist() == [2, 2, 2] and torch.equal(done.state, one.state)
    res = _bad_data(pkg, b, max_iter=1, tol=0.0, threshold=4.0, max_removals=2)
    e_std = ((res.state_std[:, 0].cpu() - R.rsqrt()).abs() * R.sqrt()).max().item()
    print(f"[bad-data shapes one bus] dof {res.dof.tolist()} chi2_limit {res.chi2_limit.tolist()} S {res.bus_sens[:, 0].tolist()} state_std relative {e_std:.1e}/1e-12")
    for f in SOLVE_FIELDS:
        assert torch.equal(getattr(res, f), getattr(one, f)), f
    assert res.dof.tolist() == [0, 0, 0] and bool(torch.isinf(res.chi2_limit).all()) and res.suspect.tolist() == [0, 0, 0]
    assert res.n_removed.tolist() == [0, 0, 0] and bool((res.removed == -1).all()) and bool((res.bus_rn == 0).all())
    assert float(res.bus_sens.abs().max()) <= 1e-15 and e_std <= 1e-12 and bool((res.state_std[:, 1] == 0).all())
    assert res.edge_rn.shape == (0, 2) and res.edge_sens.shape == (0, 2)


def test_the_incidence_lists_a_self_loop_twice(pkg):
    """What ws_accumulate_row's comment says of a branch from a bus to itself: the incidence CSR lists it as a from-end and as a to-end."""
    b = _device("multigraph")
    topo = pkg.topology.get_topology(b["edge_index"], b["x"].shape[0])
    rp, ent = topo.inc_rowptr.cpu().tolist(), topo.inc_ent.cpu()
    row = ent[rp[2]:rp[3]].tolist()
    loop = ec.SELF_LOOP
    assert row.count(loop) == 1 and row.count(loop - 2 ** 31) == 1, row
    assert rp[5] == 2 * 7 and [rp[k + 1] - rp[k] for k in range(5)] == [1, 2, 4, 4, 3]
