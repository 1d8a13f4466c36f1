"""CPU: facts about the inputs of tests/wls_edge_cases.py that tests/test_gpu_wls_shapes.py rests on, all from the fp64 oracles
(tests/wls_oracle.py, tests/wls_bad_data_oracle.py); nothing here runs the product's kernels.

  * every solvable case converges (status 0 at tol = 1e-6); `isolated`, `nan_p` and `inf_w` fail on graph 1 alone
  * the GPU tests reuse the bounds of test_gpu_wls_solve.py and test_gpu_wls_bad_data.py: for every new case two fp64 routes -- two
    summation orders of the solve (perm_seed), the QR and the normal-equation route to the sensitivities -- differ by at most one
    eighth of each bound (figures below, printed with -s)
  * at most 10 % of the graphs decide within a factor 4 of tol, at most 10 % of the active measurements have S within a factor 2 of
    s_min, at most 10 % of the graphs of the removal tests decide a removal by less than 1e-3
  * every measurement-set case moves the oracle's outputs by at least 100 x the bound when its feature is taken out of the inputs

Measured here (worst over the cases; bound / 8 in brackets):
  state, two summation orders        1.9e-9 after 1 iteration (n99), 1.8e-11 after 3, 4.5e-14 after 8          [6.25e-8]
  objective, two summation orders    1.6e-8 relative after 1 iteration (n99), 2.0e-10 after 3 and after 8      [1.25e-7]
  S, QR against normal equations     7.1e-9 (no_slack)                                                          [2.5e-8]
  state_std                          2.4e-10 (n99)                                                              [4.3e-10]
  rN where S >= 2 s_min              3.5e-7 in units of max(rN, 1) (no_slack)                                   [1.25e-5]
  decisions within a factor 4 of tol 3 of 50 graphs;  S within a factor 2 of s_min: 290 of 3068 active measurements;  removals decided
  by less than 1e-3: 0 of 6 graphs (an exact tie apart: the two tied rN of `tie` agree to all twelve printed digits)
Two cases were changed to get there, not the bounds: n64 with wls_cases' two V readings and two flows had state_std routes 8.0e-10
apart (graph 0), so n32, n64 and n65 measure V at three buses and a flow on every sixth branch; `clamped` had S routes 3.5e-8 apart
with one of its two V readings clamped away, so it measures V at a third bus.
"""
import pytest
import torch

import wls_bad_data_oracle as bo
import wls_cases as wc
import wls_edge_cases as ec
import wls_oracle as wo

TOL, S_MIN, LEAD = 1e-6, 1e-3, 1e-3
# the bounds of the two existing GPU files
STATE_BOUND, OBJ_BOUND, SENS_BOUND, RN_BOUND, STD_BOUND = 5e-7, 1e-6, 2e-7, 1e-4, 8 * 4.3e-10


def test_the_existing_batches_did_not_move():
    """graph() grew keyword hooks: with their defaults it still draws what it drew (the fp64 sums of x and edge_attr of every batch,
    pinned from the version before the hooks; the full batches were compared once with torch.equal)."""
    want = {"two_bus": (386.00504800863564, 29.958735043135675), "star10": (534.995175778924, 128.80786351222196),
            "ring6_parallel": (474.1487321422901, 121.71589269959509), "n33": (972.2300294168526, 33.653423323059776)}
    for name, sums in want.items():
        b = wc.batch(name)
        assert (float(b["x"].double().sum()), float(b["edge_attr"].double().sum())) == sums, name


def test_shapes_are_what_their_names_say():
    for name, n in (("n32", 32), ("n64", 64), ("n65", 65), ("n99", 99)):
        nb, edges, meas = ec.CASES[name]["shape"]
        deg = ec.degrees(name)
        assert nb == n and len(edges) == n - 1 and deg.min() >= 1, name
        assert 0 < sum(a > b for a, b in edges) < len(edges), "orientation is mixed"
        assert (deg >= 3).sum() >= 3, "laterals"
    L = ec.CASES["n99"]["shape"]
    deg = ec.degrees("n99")
    assert ec.HUB >= 64 and deg[ec.HUB] == 13 and deg.max() == 13 and (deg[88:] == 1).all()
    assert all(ec.HUB in L[1][k - 1] for k in range(88, 99))
    assert L[1][ec.HUB_BRANCH][0] == ec.HUB and ec.HUB_BRANCH in L[2]
    b = ec.batch("n99")
    assert int((b["x"][:99, 0] != 0).sum()) == 3
    b = ec.batch("n1")
    assert b["x"].shape == (3, 11) and b["edge_index"].shape == (2, 0) and b["edge_attr"].shape == (0, 13) and b["edge_index"].dtype == torch.int64
    assert bool((b["x"][:, 0] != 0).all()) and bool((b["x"][:, 2:8] == 0).all()) and bool((b["x"][:, 9] == 1).all())
    for name in ("pmu", "pmu_star"):
        b = ec.batch(name)
        n = b["nodes_per_graph"]
        th = (b["x"][:n, 2] != 0) & (b["x"][:n, 3] != 0)
        assert th.nonzero().flatten().tolist() == list(range(3, n, 3)) and 2 * ec.batch("pmu")["nodes_per_graph"] > 64 >= 2 * ec.batch("pmu_star")["nodes_per_graph"]
    b = ec.batch("no_slack")
    assert bool((b["x"][:, 9] == 0).all()) and (b["x"][:10, 3] != 0).nonzero().flatten().tolist() == [0, 4, 8]
    assert (ec.batch("two_slack")["x"][:6, 9] != 0).nonzero().flatten().tolist() == [0, 5]
    assert (ec.batch("slack_last")["x"][:33, 9] != 0).nonzero().flatten().tolist() == [32]
    assert bool((ec.batch("all_flows")["edge_attr"][:, :4] != 0).all())
    # clamped: the three weights are below 0 after de-normalisation from the fp32 input, every other one is in [1e2, 1e6]
    b = ec.batch("clamped")
    raw = _raw_weights(b)
    neg = [(raw[0][9, 0], "V"), (raw[0][4, 2], "P"), (raw[1][3, 0], "flow")]
    assert all(float(v) < -1e3 for v, _ in neg) and int((raw[0] < 0).sum()) == 3 * 2 and int((raw[1] < 0).sum()) == 3
    assert bool(((raw[0] <= 0) | ((raw[0] >= 99.0) & (raw[0] <= 1.01e6))).all())
    # multigraph
    n, edges, meas = ec.CASES["multigraph"]["shape"]
    assert edges[ec.SELF_LOOP] == (2, 2) and [edges[k] for k in ec.TRIPLE] == [(3, 4), (3, 4), (4, 3)] and meas == list(range(7))
    b = ec.batch("multigraph")
    assert bool((b["edge_attr"][:, :4] != 0).all()) and len({tuple(r) for r in b["edge_attr"][list(ec.TRIPLE), 6:10].tolist()}) == 3
    # isolated: bus 3 has no branch; the two batches differ in graph 1's theta reading alone
    assert ec.degrees("isolated_pmu")[ec.ISOLATED_BUS] == 0
    a, b = ec.batch("isolated_pmu"), ec.batch("isolated")
    diff = (a["x"] != b["x"]).nonzero().tolist()
    assert diff == [[6 + ec.ISOLATED_BUS, 2], [6 + ec.ISOLATED_BUS, 3]] and torch.equal(a["edge_attr"], b["edge_attr"])
    # tie: two identical stored branches
    b = ec.batch("tie")
    assert b["edge_index"][:, :2].tolist() == [[0, 0], [1, 1]] and torch.equal(b["edge_attr"][0::2], b["edge_attr"][1::2])
    # non-finite inputs: one entry of graph 1
    s = ec.batch("star10")
    for name, (row, col), test in (("nan_p", (10 + 4, 4), torch.isnan), ("inf_w", (10 + 9, 1), torch.isinf)):
        b = ec.batch(name)
        bad = ~torch.isfinite(b["x"])
        assert bad.nonzero().tolist() == [[row, col]] and bool(test(b["x"][row, col])) and torch.equal(b["x"][~bad], s["x"][~bad])
        assert torch.equal(b["edge_attr"], s["edge_attr"])


def _raw_weights(b):
    """De-normalised weights WITHOUT the clamp at 0: ([N, 4], [E, 2]) fp64."""
    xm, xs, em, es = (s.double() for s in b["stats"])
    r, er = b["x"].double()[:, 1:8:2], b["edge_attr"].double()[:, 1:4:2]
    return (r * xs[1:8:2] + xm[1:8:2]) * (r != 0), (er * es[1:4:2] + em[1:4:2]) * (er != 0)


def test_every_case_converges_and_the_failing_graphs_fail_alone():
    total = close = 0
    for name in ec.SOLVABLE:
        res = ec.oracle_solve(name, 12, TOL)
        u = wo.undecided(res, TOL)
        total, close = total + u.numel(), close + int(u.sum())
        print(f"[edge-cases convergence] {name}: iterations {res['iterations'].tolist()} last steps {['%.1e' % v for v in res['last_step'].tolist()]} undecided {u.tolist()}")
        assert bool((res["status"] == 0).all()), name
    print(f"[edge-cases convergence] {close} of {total} graphs decide within a factor 4 of tol")
    assert close <= 0.1 * total
    for name in ec.FAILING:
        res = ec.oracle_solve(name, 12, TOL)
        ok = ec.oracle_solve(ec.HEALTHY[name], 12, TOL)
        assert res["status"].tolist() == [0, 2, 0] and int(res["iterations"][1]) == 0, name
        n = ec.batch(name)["nodes_per_graph"]
        assert torch.equal(res["state"][n:2 * n], torch.tensor([1.0, 0.0], dtype=torch.float64).expand(n, 2))
        others = torch.tensor([True, False, True]).repeat_interleave(n)
        assert torch.equal(res["state"][others], ok["state"][others]) and bool((ok["status"] == 0).all())


def test_the_isolated_bus_fails_at_an_interior_pivot():
    b = ec.batch("isolated")
    gr = wo.graphs_of(*ec.args(b))[ec.FAILING_GRAPH]
    u = torch.zeros(12, dtype=torch.float64)
    u[0::2] = 1.0
    Gm, _ = gr.normal_equations(u)
    p = 2 * ec.ISOLATED_BUS + 1
    assert float(Gm[p, p]) == 0.0 and bool((Gm[p] == 0).all()) and 0 < p < 11
    assert int(torch.linalg.cholesky_ex(Gm)[1]) == p + 1 and bool((Gm.diagonal()[:p] > 0).all())


def test_one_bus_without_branches_has_a_known_answer():
    b = ec.batch("n1")
    Z = wo.denormalised(b["x"], b["edge_attr"], b["stats"])[0]
    res = bo.bad_data(*ec.args(b), max_iter=1, tol=0.0)
    assert torch.equal(res["state"][:, 0], Z[:, 0]) and bool((res["state"][:, 1] == 0).all())
    assert res["dof"].tolist() == [0, 0, 0] and bool(torch.isinf(res["chi2_limit"]).all()) and res["suspect"].tolist() == [0, 0, 0]
    assert res["iterations"].tolist() == [1, 1, 1] and bool((res["bus_rn"] == 0).all())
    assert float(res["bus_sens"][:, 0].abs().max()) < 1e-15 and float(res["objective"].abs().max()) < 1e-20


def test_two_fp64_routes_agree_within_an_eighth_of_every_bound():
    worst = {}

    def note(key, value, name):
        if value > worst.get(key, (-1.0, ""))[0]:
            worst[key] = (value, name)

    for name in ec.SOLVABLE:
        b = ec.batch(name)
        n = b["nodes_per_graph"]
        for it in (1, 3, 8):
            a, p = ec.oracle_solve(name, it, 0.0), ec.oracle_solve(name, it, 0.0, 5)
            st = (a["state"] - p["state"]).abs().max().item()
            ob = ((a["objective"] - p["objective"]).abs() / a["objective"].abs()).max().item()
            print(f"[edge-cases routes] {name} {it} iterations: state {st:.2e}/{STATE_BOUND / 8:.2e} objective {ob:.2e}/{OBJ_BOUND / 8:.2e}")
            note(f"state after {it}", st, name)
            note(f"objective after {it}", ob, name)
            assert st <= STATE_BOUND / 8 and ob <= OBJ_BOUND / 8, (name, it, st, ob)
        state = ec.oracle_clean(name)["state"]
        for g, gr in enumerate(wo.graphs_of(*ec.args(b), weights=ec.weights_of(name))):
            u = state[g * n:(g + 1) * n].reshape(-1)
            S, std = bo.sens_qr(gr, u)
            S2, std2 = bo.sens_normal(gr, u)
            rn, rn2 = bo.normalized_residuals(gr, u, S, S_MIN), bo.normalized_residuals(gr, u, S2, S_MIN)
            kept = (gr.w > 0) & (S >= 2 * S_MIN)
            e_s, e_std = (S - S2).abs().max().item(), (std - std2).abs().max().item()
            e_rn = ((rn - rn2).abs() / rn.clamp_min(1.0))[kept].max().item()
            print(f"[edge-cases routes] {name} graph {g}: S {e_s:.2e}/{SENS_BOUND / 8:.2e} state_std {e_std:.2e}/{STD_BOUND / 8:.2e} rN {e_rn:.2e}/{RN_BOUND / 8:.2e}")
            note("S", e_s, name)
            note("state_std", e_std, name)
            note("rN", e_rn, name)
            assert e_s <= SENS_BOUND / 8 and e_std <= STD_BOUND / 8 and e_rn <= RN_BOUND / 8, (name, g, e_s, e_std, e_rn)
    for key, (value, name) in worst.items():
        print(f"[edge-cases routes] worst {key}: {value:.2e} ({name})")


def test_few_sensitivities_fall_close_to_s_min():
    near = active = 0
    for name in ec.SOLVABLE:
        res, b = ec.oracle_clean(name), ec.batch(name)
        S = torch.cat([res["bus_sens"].reshape(-1), res["edge_sens"].reshape(-1)])
        act = sum(int((gr.w > 0).sum()) for gr in wo.graphs_of(*ec.args(b), weights=ec.weights_of(name)))
        close = int(((S >= S_MIN / 2) & (S <= 2 * S_MIN)).sum())
        print(f"[edge-cases s_min] {name}: {close} of {act} active measurements have S within a factor 2 of s_min; dof {res['dof'].tolist()}")
        near, active = near + close, active + act
    print(f"[edge-cases s_min] {near} of {active} in all")
    assert near <= 0.1 * active


def test_dof_counts_active_measurements_and_free_states():
    dof = lambda name: ec.oracle_clean(name)["dof"].tolist()
    # star10: V at 2 buses, P and Q at 10, 2 flows on 2 branches = 26 measurements, 19 free states
    assert dof("star10_weighted") == [7] * 3
    assert dof("clamped") == [7 + 1 - 3] * 3                 # V at a third bus; three weights clamped to 0: not active
    assert dof("no_slack") == [26 + 3 - 20] * 3              # theta at three buses, no state held
    assert dof("pmu_star") == [7 + 3] * 3
    assert dof("two_slack") == [2 + 12 + 4 - (12 - 2)] * 3   # ring6_parallel: 18 measurements, two angles held
    assert dof("slack_last") == [7] * 3 and dof("all_flows") == [2 + 12 + 14 - 11] * 3
    assert dof("isolated_pmu") == [3 + 1 + 12 + 4 - 11] * 3 and dof("tie") == [2 + 4 + 4 - 3] * 3
    assert dof("n99") == [3 + 198 + 4 - 197] * 3


def _decided(dec, threshold=4.0):
    return all(abs(best - threshold) >= LEAD * threshold and (best <= threshold or best - second >= LEAD * best) for _, best, second in dec)


def test_the_removal_cases_decide_clearly():
    graphs = left_out = 0
    hb, ids, res = ec.cross_wave()
    assert res["removed"][:, 0].tolist() == ids and res["n_removed"].tolist() == [1, 1, 1]
    assert ids[2] // 4 % 99 >= 64 and ids[0] // 4 % 99 < 64 and ids[1] >= 4 * 297 and ec.CASES["n99"]["shape"][1][(ids[1] - 4 * 297) // 2 % 98][0] >= 64
    graphs, left_out = graphs + 3, left_out + sum(not _decided(d) for d in res["decisions"])
    hb, ids, res = ec.five_errors()
    g = ec.FIVE_ERRORS_GRAPH
    print(f"[edge-cases removals] five errors at {ids}: removed {res['removed'][g, :6].tolist()} rN {['%.2f' % v for v in res['removed_rn'][g, :6].tolist()]}")
    assert res["n_removed"].tolist() == [5 if k == g else 0 for k in range(3)] and res["removed"].shape == (3, 64)
    assert all(_decided(d) for d in res["decisions"])
    graphs += 3
    hb, ids, res = ec.tied()
    for k, dec in enumerate(res["decisions"]):
        winner, best, second = dec[0]
        print(f"[edge-cases removals] tie graph {k}: ids {ids[k]} winner {winner} rN {best:.12g} runner-up {second:.12g}")
        assert winner in ids[k] and abs(best - second) <= 1e-9 * best and best > 4.0
    # ... and behind the pair the third is far away (at the removal; the oracle's own final rN are of the state after it)
    first = bo.bad_data(*ec.args(hb), max_removals=0, **ec.REMOVAL)
    for k in range(3):
        pair = first["edge_rn"][2 * k:2 * k + 2, 1]
        rest = torch.cat([first["bus_rn"][2 * k:2 * k + 2].reshape(-1), first["edge_rn"][2 * k:2 * k + 2, 0]]).max()
        assert float(pair.min()) - float(rest) >= LEAD * float(pair.min())
    print(f"[edge-cases removals] {left_out} of {graphs} graphs decide a removal by less than 1e-3")
    assert left_out <= 0.1 * graphs


def _moved(a, b):
    """How far two oracle results are apart, in units of the bounds: the state and the objective."""
    if a["status"].tolist() != b["status"].tolist():
        return float("inf")
    st = (a["state"] - b["state"]).abs().max().item() / STATE_BOUND
    ob = ((a["objective"].sum(1) - b["objective"].sum(1)).abs() / a["objective"].sum(1).abs()).max().item() / OBJ_BOUND
    return max(st, ob)


@pytest.mark.parametrize("name", ec.MEASUREMENT_SETS + ec.WEIGHTED)
def test_each_case_discriminates(name):
    """The oracle without the case's feature is at least 100 bounds away: a kernel that ignored the feature could not pass."""
    with_it = ec.oracle_solve(name, 8, 0.0)
    if name == "clamped":                                   # the weights as they are, below 0 included
        b = ec.batch(name)
        gs = wo.graphs_of(*ec.args(b))
        R, eR = _raw_weights(b)
        for g, gr in enumerate(gs):
            rows, _ = ec.graph_rows(b, g)
            gr.w = torch.cat([R[rows].reshape(-1), eR[gr.edges].reshape(-1)])
            assert int((gr.w < 0).sum()) == 3
        without = wo.solve(None, None, None, None, b["nodes_per_graph"], max_iter=8, tol=0.0, graphs=gs)
    else:
        b, weights = ec.without_feature(name)
        without = wo.solve(*ec.args(b), max_iter=8, tol=0.0, weights=weights)
    moved = _moved(with_it, without)
    print(f"[edge-cases discriminate] {name}: the oracle without the feature is {moved:.3g} bounds away (status {without['status'].tolist()})")
    assert moved >= 100.0
