"""CPU: what tests/test_gpu_wls_mixed.py rests on, from the fp64 oracles alone and from the header; nothing here runs a kernel.

  * every graph of the batches A, B and C of tests/wls_mixed_cases.py converges in the per-graph oracle (batch V_lv, flat start,
    tol = 1e-6, max_iter = 12) in 2 .. 6 iterations, and NONE has its deciding step within a factor 4 of the tolerance: the GPU test
    compares every decision on them, none left out.  If this ever fails the batch is to be changed, not the rule.
  * the bounds of the GPU test.  A, B and cigre14 + ober_sub are held to the project's 5e-7 (state) and 1e-6 relative (objective): two
    summation orders of the oracle (perm_seed 1 .. 4 against none) differ by at most an eighth of each, as in
    tests/test_wls_edge_cases_cpu.py.  C, D and ober_sub + ober179 are held to wls_large_cases.state_bound(spread), spread = the worst
    over perm_seed 1 .. 4 of |fp32(oracle state) - permuted-order state| (tests/test_wls_large_cpu.py's rule, margin 8), and to
    max(1e-6, 8 x the objective's relative spread); wls_mixed_cases forms both from the oracle where the test runs, so the margin of 8 is
    there by construction, and this test holds the spreads themselves to a ceiling.
    Measured (run with -s): A, B, cigre14 + ober_sub: fp64 state spread at most 7.7e-9 (B after one iteration), objective at most
    3.5e-9 relative; C and D: spread at most 6.0e-8 at every trip count (the fp32 rounding of the output), so 5e-7, objective at most
    3.5e-9; ober_sub + ober179: state 5.9e-8, 7.3e-8, 6.0e-8 after 1, 3, 8 iterations, so 5e-7, 5.8e-7, 5e-7; objective 2.6e-7
    relative after one iteration (the ober179 graph's bus part; condition number 2.4e13), so 2.1e-6 there, 1.7e-8 after three.
  * the robust and the bad-data mixes: the gross errors are where synthetic.corrupt_measurements says (global ids), the bad-data oracle
    finds at least three of the five and decides every removal clearly, no measurement of the robust mixes has t within 1e-6 gamma of gamma, and the
    oracle's q over four summation orders stays within an eighth of the 1e-9 the GPU test uses at 8 iterations.
  * dss2_wls_solve_args' two new fields, graph_ptr and n_graphs, in the ctypes mirrors of all four argument structs against the header.
"""
import ctypes

import pytest
import torch

import wls_bad_data_oracle as bo
import wls_mixed_cases as mc
import wls_oracle as wo
import wls_robust_oracle as ro
from conftest import load_pkg

Q_BOUND, SENS_BOUND, RN_BOUND, STD_BOUND, S_MIN, LEAD = 1e-9, 2e-7, 1e-4, 8 * 4.3e-10, 1e-3, 1e-3


def test_the_batches_are_what_their_names_say():
    for name in mc.FIXED:
        b = mc.batch(name)
        assert b["nodes_per_graph"] == mc.BOUNDS[name] == max(b["sizes"]) and len(set(b["sizes"])) > 1 and 3 <= b["num_graphs"] <= 8
        assert b["graph_ptr"].tolist()[-1] == b["x"].shape[0] and b["edge_ptr"][-1] == b["edge_attr"].shape[0]
    assert mc.batch("A")["sizes"] == [2, 33, 1, 10, 1, 33, 6] and mc.batch("B")["sizes"] == [64, 2, 99, 1, 10]
    assert mc.batch("C")["sizes"] == [2, 100, 1, 33, 179, 99, 128] and mc.batch("D")["sizes"] == [256, 2, 100]
    assert sorted(set(mc.batch("cigre_ober")["sizes"])) == [15, 70] and sorted(set(mc.batch("ober_ober179")["sizes"])) == [70, 179]
    assert mc.batch("cigre_ober")["num_graphs"] == 6 and mc.batch("ober_ober179")["num_graphs"] == 4
    # n1 alone would be solved at 110 kV: the batch's V_lv is 3 kV
    b = mc.batch("A")
    x, _, _, n, _ = mc.cut(b, 2)
    assert n == 1 and float(x[0, 8]) == 110.0 and float(mc.batch_kk(b)) == 9.0
    # a reordered batch holds the same graphs
    r = mc.reordered(b, list(range(b["num_graphs"]))[::-1])
    assert r["sizes"] == b["sizes"][::-1] and torch.equal(mc.cut(r, 0)[0], mc.cut(b, 6)[0]) and torch.equal(mc.cut(r, 5)[1], mc.cut(b, 1)[1])


@pytest.mark.parametrize("name", mc.DECIDED)
def test_every_graph_converges_and_none_is_undecided(name):
    res = mc.oracle(name, 12, mc.TOL)
    u = wo.undecided(res, mc.TOL)
    print(f"[wls mixed convergence] {name}: iterations {res['iterations'].tolist()} last steps {['%.1e' % v for v in res['last_step'].tolist()]} "
          f"undecided {u.tolist()}")
    assert bool((res["status"] == 0).all()) and not bool(u.any())
    assert 2 <= int(res["iterations"].min()) and int(res["iterations"].max()) <= 6


@pytest.mark.parametrize("name", mc.ALL)
def test_the_gpu_tests_bounds_cover_the_oracles_spread(name):
    for it in mc.TRIP_COUNTS:
        ref = mc.oracle(name, it, 0.0)
        assert bool((ref["status"] == 1).all()) and bool((ref["iterations"] == it).all())
        rounded, exact, obj = mc.spreads(name, it)
        sb, ob = mc.state_bound(name, it), mc.objective_bound(name, it)
        print(f"[wls mixed bounds] {name} {it} iterations: fp64 spread {exact:.2e}, against the fp32 state {rounded:.2e}: state bound {sb:.2e}; "
              f"objective spread {obj:.2e} relative: bound {ob:.2e}")
        if name in mc.SPREAD_BOUNDED:
            assert sb == max(5e-7, 8.0 * rounded) and ob == max(1e-6, 8.0 * obj)
            assert sb <= 1e-6 and ob <= 4e-6, (name, it, rounded, obj)      # (an oracle this far apart from itself would referee nothing)
        else:
            assert sb == mc.STATE_BOUND == 5e-7 and exact <= sb / 8, (name, it, exact)
            assert ob == mc.OBJ_BOUND == 1e-6 and obj <= ob / 8, (name, it, obj)


def test_a_one_bus_graph_has_a_zero_objective_in_the_oracle():
    """(the relative objective error of the GPU test is taken over the graphs whose objective is not 0)"""
    ref = mc.oracle("A", 3, 0.0)
    for g in (2, 4):
        assert float(ref["objective"][g].abs().max()) < 1e-20


@pytest.mark.parametrize("name", ["R_lds", "R_blocked"])
def test_the_robust_mixes_are_clear_of_the_threshold(name):
    hb, ids = mc.corrupted(name)
    assert len(ids) == hb["num_graphs"] and len(set(ids)) == len(ids)
    ref = mc.robust_oracle(name, 8, 0.0)
    assert sum(ro.near_threshold(ref)) == 0 and bool((ref["n_downweighted"] >= 1).all())
    spread = st = obj = 0.0
    for seed in (1, 2, 3, 4):
        other = mc.robust_oracle(name, 8, 0.0, seed)
        spread = max(spread, (ref["bus_q"] - other["bus_q"]).abs().max().item(), (ref["edge_q"] - other["edge_q"]).abs().max().item())
        st = max(st, (ref["state"] - other["state"]).abs().max().item())
        obj = max(obj, ((ref["objective"] - other["objective"]).abs() / ref["objective"].abs().clamp_min(1e-300)).max().item())
        assert ro.downweighted_ids(other) == ro.downweighted_ids(ref)
    print(f"[wls mixed robust] {name}: errors at {ids}, down-weighted {ref['n_downweighted'].tolist()}: q spread {spread:.2e}/{Q_BOUND / 8:.2e} "
          f"state {st:.2e}/{mc.STATE_BOUND / 8:.2e} objective {obj:.2e}/{mc.OBJ_BOUND / 8:.2e}")
    assert spread <= Q_BOUND / 8 and st <= mc.STATE_BOUND / 8 and obj <= mc.OBJ_BOUND / 8


def test_the_bad_data_mix_removes_the_injected_errors_clearly():
    hb, ids = mc.corrupted("BD")
    ref = mc.bad_data_oracle("BD", 1)
    print(f"[wls mixed bad data] errors at {ids}: removed {ref['removed'][:, 0].tolist()} rN {['%.2f' % v for v in ref['removed_rn'][:, 0].tolist()]} "
          f"decisions {[[(w, round(a, 3), round(s, 3)) for w, a, s in d] for d in ref['decisions']]}")
    assert hb["nodes_per_graph"] <= 99
    # (a random active measurement may be a critical one, whose error no test can see: what counts is that the kernel removes what the
    #  oracle removes, and that most of the errors are found)
    found = [r == i for r, i in zip(ref["removed"][:, 0].tolist(), ids)]
    assert sum(found) >= 3 and all(r in (i, -1) or ref["n_removed"][g] == 1 for g, (r, i) in enumerate(zip(ref["removed"][:, 0].tolist(), ids)))
    for dec in ref["decisions"]:
        for _, best, second in dec:
            assert abs(best - 4.0) >= LEAD * 4.0 and (best <= 4.0 or best - second >= LEAD * best)
    # two fp64 routes to S, rN and state_std at the final state, as tests/test_wls_edge_cases_cpu.py has them
    for g in range(hb["num_graphs"]):
        x, ei, ea, n, _ = mc.cut(hb, g)
        gr = wo.graphs_of(x, ei, ea, hb["stats"], n)[0]
        N = hb["x"].shape[0]                # the removed measurement's row among the graph's own: 4 i + k, then 4 n + 2 e + k
        m = ids[g] - 4 * int(hb["graph_ptr"][g]) if ids[g] < 4 * N else 4 * n + ids[g] - 4 * N - 2 * hb["edge_ptr"][g]
        if int(ref["n_removed"][g]):
            gr.w = gr.w.clone()
            gr.w[m] = 0.0
        rows, _ = mc.graph_rows(hb, g)
        u = ref["state"][rows].reshape(-1)
        S, std = bo.sens_qr(gr, u)
        S2, std2 = bo.sens_normal(gr, u)
        rn, rn2 = bo.normalized_residuals(gr, u, S, S_MIN), bo.normalized_residuals(gr, u, S2, S_MIN)
        kept = (gr.w > 0) & (S >= 2 * S_MIN)
        e_s, e_std = (S - S2).abs().max().item(), (std - std2).abs().max().item()
        e_rn = ((rn - rn2).abs() / rn.clamp_min(1.0))[kept].max().item()
        print(f"[wls mixed bad data] graph {g}: S {e_s:.2e}/{SENS_BOUND / 8:.2e} state_std {e_std:.2e}/{STD_BOUND / 8:.2e} rN {e_rn:.2e}/{RN_BOUND / 8:.2e}")
        assert e_s <= SENS_BOUND / 8 and e_std <= STD_BOUND / 8 and e_rn <= RN_BOUND / 8, (g, e_s, e_std, e_rn)


def test_struct_layout_of_the_two_new_fields_matches_the_header():
    """Where the two fields sit in the mirror and that all three nested structs embed it at offset 0 (tests/test_abi_cpu.py holds every
    field of the four to the header)."""
    lib = load_pkg()._lib
    S = lib.WlsSolveArgs
    assert [f for f, _ in S._fields_][-2:] == ["graph_ptr", "n_graphs"] and S.n_graphs.offset == S.graph_ptr.offset + 8
    assert S.graph_ptr.offset == S.max_groups.offset + 8 and ctypes.sizeof(S) == S.n_graphs.offset + 8
    for cls in (lib.WlsBadDataArgs, lib.WlsLargeArgs, lib.WlsRobustArgs):
        assert cls._fields_[0] == ("solve", S) and cls.solve.offset == 0


def test_the_python_side_takes_graph_ptr_everywhere():
    import inspect
    pkg = load_pkg()
    est = pkg.estimator
    hb = mc.batch("A")
    # the keyword is taken by all four (its absence would be a TypeError): with CPU tensors the call gets as far as the device check
    for fn in (est.wls_estimate, est.wls_estimate_large, est.wls_robust, est.wls_bad_data):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(hb["x"], hb["edge_index"], hb["edge_attr"], *hb["stats"], 33, graph_ptr=hb["graph_ptr"])
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(hb["x"], hb["edge_index"], hb["edge_attr"], *hb["stats"], nodes_per_graph=33, max_iter=3, graph_ptr=hb["graph_ptr"])
        with pytest.raises(TypeError):
            fn(hb["x"], hb["edge_index"], hb["edge_attr"], *hb["stats"], 33, graph_ptrs=hb["graph_ptr"])
        assert "graph_ptr" in fn.__doc__ and fn.__name__ in ("wls_estimate", "wls_estimate_large", "wls_robust", "wls_bad_data")
        assert "graph_ptr" not in inspect.signature(fn).parameters        # the pinned parameter lists stand (tests/test_wls_bad_data_cpu.py)
    assert inspect.signature(est.wls_estimate_large) == inspect.signature(est.wls_estimate)
    assert inspect.signature(pkg.runner.evaluate_wls).parameters["nodes_per_graph"].default is None
    b = pkg.dataset.Batch(None, None, None, None, 0)
    assert b.graph_ptr is None and b.max_nodes is None
