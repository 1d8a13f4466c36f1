"""CPU: the fp64 oracle of the bad-data estimator (tests/wls_bad_data_oracle.py) held to the facts the GPU tests rely on, on all seven
batches of tests/wls_cases.py (27 graphs, 10 iterations, tol = 0) -- and the host side of estimator.wls_bad_data that needs no GPU.

Two fp64 routes to the sensitivities -- the leverages of a QR of sqrt(W) H (the oracle's) and the normal equations with cholesky_inverse
(the kernel's mathematics), the second also with the measurements entering G in random orders -- measured here (run with -s):
  S          2.0e-8 absolute at worst in the same order (n33 graph 2), 3.6e-8 in random orders     the GPU test holds the kernel to 2e-7
  state_std  4.24e-10 absolute at worst (n33, a random order; 2.4e-10 in the same order)            the GPU test holds the kernel to
             8 x STATE_STD_ROUTES = 3.44e-9
  rN         3.8e-4 relative where S is about 1e-6: that is why s_min exists; 2.0e-7 at worst, in units of max(rN, 1), where S >= 2 s_min
"""
import functools
import inspect

import pytest
import torch

import wls_bad_data_oracle as bo
import wls_cases as wc
import wls_oracle as wo
from conftest import load_pkg

S_MIN = 1e-3
STATE_STD_ROUTES = 4.3e-10     # the worst state_std difference between the fp64 routes (measured 4.24e-10), rounded up; asserted below


@functools.lru_cache(maxsize=None)
def _batch(name):
    return wc.any_batch(name)


def _args(b):
    return b["x"], b["edge_index"], b["edge_attr"], b["stats"], b["nodes_per_graph"]


@functools.lru_cache(maxsize=None)
def _clean(name):
    return bo.bad_data(*_args(_batch(name)), max_iter=10, tol=0.0, threshold=4.0, max_removals=3)


def _per_graph_sum(res, b):
    n, ei = b["nodes_per_graph"], b["edge_index"]
    G = b["x"].shape[0] // n
    s = res["bus_sens"].reshape(G, -1).sum(1)
    return s.index_add(0, ei[0] // n, res["edge_sens"].sum(1))


def test_sensitivities_sum_to_the_degrees_of_freedom():
    dofs = {}
    for name in wc.ALL_BATCHES:
        res = _clean(name)
        tr = _per_graph_sum(res, _batch(name))
        err = (tr - res["dof"].double()).abs().max().item()
        print(f"[bad-data trace] {name}: dof {res['dof'].tolist()} sum S - dof {err:.2e}")
        assert err < 1e-9
        dofs[name] = sorted(set(res["dof"].tolist()))
    assert dofs == {"cigre14": [11], "mixed": [11], "ober_sub": [24], "two_bus": [5], "star10": [7], "ring6_parallel": [7], "n33": [7]}


def test_two_fp64_routes_and_summation_orders_agree():
    worst = {"S": 0.0, "S_same_order": 0.0, "std": 0.0, "rn_all": 0.0, "rn_kept": 0.0}
    smallest, below, active = 1.0, [], 0
    for name in wc.ALL_BATCHES:
        b = _batch(name)
        n = b["nodes_per_graph"]
        gs = wo.graphs_of(*_args(b))
        state = _clean(name)["state"]
        for g, gr in enumerate(gs):
            u = state[g * n:(g + 1) * n].reshape(-1)
            S, std = bo.sens_qr(gr, u)
            rn = bo.normalized_residuals(gr, u, S, 1e-12)
            act = gr.w > 0
            smallest = min(smallest, float(S[act].min()))
            below.append(int((S[act] < S_MIN).sum()))
            active += int(act.sum())
            gen = torch.Generator().manual_seed(5 + g)
            for perm in (None, torch.randperm(gr.z.shape[0], generator=gen), torch.randperm(gr.z.shape[0], generator=gen)):
                S2, std2 = bo.sens_normal(gr, u, perm)
                rn2 = bo.normalized_residuals(gr, u, S2, 1e-12)
                rel = (rn - rn2).abs() / rn.clamp_min(1.0)
                kept = act & (S >= 2 * S_MIN)
                worst["S"] = max(worst["S"], float((S - S2).abs().max()))
                if perm is None:
                    worst["S_same_order"] = max(worst["S_same_order"], float((S - S2).abs().max()))
                worst["std"] = max(worst["std"], float((std - std2).abs().max()))
                worst["rn_all"] = max(worst["rn_all"], float(((rn - rn2).abs() / rn.clamp_min(1e-300))[act & (S > 0) & (S2 > 0)].max()))
                worst["rn_kept"] = max(worst["rn_kept"], float(rel[kept].max()))
    print(f"[bad-data routes] S {worst['S_same_order']:.2e} (measurements in their own order) {worst['S']:.2e} (and in random orders) state_std {worst['std']:.2e} rN relative, every active measurement {worst['rn_all']:.2e}, "
          f"where S >= 2 s_min {worst['rn_kept']:.2e} (in units of max(rN, 1)); smallest S {smallest:.2e}; below s_min per graph {min(below)} .. {max(below)}")
    assert worst["S_same_order"] <= 2.5e-8           # the issue measured 2.0e-8: 8 x that, 2e-7, is the kernel's bound
    assert worst["S"] <= 1e-7                        # another summation order of G stays within half of that bound
    assert worst["std"] <= STATE_STD_ROUTES
    assert worst["rn_kept"] <= worst["S"] / (2 * 2 * S_MIN) * 1.01      # the S difference at the floor, halved by the square root
    assert 1e-6 < smallest < 1e-5 and min(below) == 0 and max(below) <= 22


def test_few_sensitivities_fall_close_to_s_min():
    """The GPU test leaves measurements with S inside [s_min / 2, 2 s_min] out of the rN comparison: at most 10 % of the active ones."""
    near = active = 0
    for name in wc.ALL_BATCHES:
        res, b = _clean(name), _batch(name)
        S = torch.cat([res["bus_sens"].reshape(-1), res["edge_sens"].reshape(-1)])
        gs = wo.graphs_of(*_args(b))
        active += sum(int((gr.w > 0).sum()) for gr in gs)
        near += int(((S >= S_MIN / 2) & (S <= 2 * S_MIN)).sum())
    print(f"[bad-data s_min] {near} of {active} active measurements have S within a factor 2 of s_min")
    assert near <= 0.1 * active


def test_clean_data_lose_nothing_at_threshold_4():
    worst = (0.0, None)
    for name in wc.ALL_BATCHES:
        res = _clean(name)
        assert res["n_removed"].tolist() == [0] * len(res["decisions"]) and bool((res["removed"] == -1).all())
        for g, dec in enumerate(res["decisions"]):
            assert len(dec) == 1
            worst = max(worst, (dec[0][1], (name, g)))
    print(f"[bad-data clean] largest rN {worst[0]:.3f} at {worst[1]}")
    assert worst[1] == ("mixed", 2) and abs(worst[0] - 3.62) < 0.01


def test_one_gross_error_per_graph_is_the_first_and_only_removal():
    graphs = close = 0
    for name in wc.ALL_BATCHES:
        b = _batch(name)
        targets = bo.largest_sensitivity_targets(*_args(b))
        x2, ea2 = bo.add_gross_errors(b["x"], b["edge_attr"], b["stats"], targets)
        res = bo.bad_data(x2, b["edge_index"], ea2, b["stats"], b["nodes_per_graph"], max_iter=10, tol=0.0, threshold=4.0, max_removals=3)
        leads = [(d[0][1] - d[0][2]) / d[0][1] for d in res["decisions"]]
        print(f"[bad-data one error] {name}: targets {targets} removed {res['removed'][:, 0].tolist()} rN {['%.2f' % v for v in res['removed_rn'][:, 0].tolist()]} "
              f"leads {['%.1e' % v for v in leads]} final max rN {['%.2f' % d[-1][1] for d in res['decisions']]}")
        assert res["removed"][:, 0].tolist() == targets and res["n_removed"].tolist() == [1] * len(targets)
        for g, dec in enumerate(res["decisions"]):
            # with the error gone the largest rN is back in the clean data's range (at most 3.62 there)
            assert len(dec) == 2 and dec[-1][1] < 3.7
            graphs, close = graphs + 1, close + (leads[g] < 1e-3)
    print(f"[bad-data one error] {close} of {graphs} graphs decide by less than 1e-3")
    assert graphs == 27 and close <= 0.1 * graphs


def test_ober_sub_largest_sensitivity_is_a_decoupled_slack_angle():
    b = _batch("ober_sub")
    res = _clean("ober_sub")
    n = b["nodes_per_graph"]
    for g in range(3):
        S = res["bus_sens"][g * n:(g + 1) * n]
        i, k = divmod(int(S.argmax()), 4)
        assert k == 1 and float(S.max()) == 1.0 and float(b["x"][g * n + i, 9]) != 0.0
        assert bo.largest_sensitivity_targets(*_args(b))[g] != 4 * (g * n + i) + 1


def test_struct_layout_matches_the_header():
    """The solve's block is embedded unchanged, at offset 0 (tests/test_abi_cpu.py holds every field to the header)."""
    lib = load_pkg()._lib
    cls = lib.WlsBadDataArgs
    assert cls._fields_[0] == ("solve", lib.WlsSolveArgs) and cls.solve.offset == 0


def test_lds_helper_admits_every_bus_count_the_solve_serves():
    pkg = load_pkg()
    L = pkg._lib.lib()
    cap = 160 * 1024
    for n in (15, 70):
        assert L.dss2_wls_solve_lds_bytes(n) < L.dss2_wls_bad_data_lds_bytes(n) <= cap
    assert L.dss2_wls_bad_data_lds_bytes(179) > cap and L.dss2_wls_bad_data_lds_bytes(0) == 0
    assert L.dss2_wls_bad_data_lds_bytes(pkg.estimator.max_nodes_per_graph()) <= cap
    assert "dss2_wls_bad_data" in pkg._lib.EXPORTED_SYMBOLS and "dss2_wls_bad_data_lds_bytes" in pkg._lib.EXPORTED_SYMBOLS


def test_host_refusals_and_unchanged_signatures():
    pkg = load_pkg()
    b = _batch("cigre14")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.estimator.wls_bad_data(b["x"], b["edge_index"], b["edge_attr"], *b["stats"], 15)
    sig = inspect.signature(pkg.runner.evaluate_wls)
    assert list(sig.parameters) == ["loader", "stats", "nodes_per_graph", "model", "bad_data", "solver_kw"]
    assert sig.parameters["bad_data"].default is None and sig.parameters["model"].default is None
    est = inspect.signature(pkg.estimator.wls_estimate)
    assert list(est.parameters) == ["x", "edge_index", "edge_attr", "x_mean", "x_std", "edge_mean", "edge_std", "nodes_per_graph", "init", "max_iter",
                                    "tol", "weights", "max_groups"]
    bad = inspect.signature(pkg.estimator.wls_bad_data)
    assert list(bad.parameters)[:12] == list(est.parameters)[:12]
    assert {k: bad.parameters[k].default for k in ("threshold", "max_removals", "confidence", "s_min", "max_groups")} == \
        {"threshold": 3.0, "max_removals": 0, "confidence": 0.95, "s_min": 1e-3, "max_groups": 0}
    assert pkg.WLSBadDataResult._fields[:5] == pkg.WLSResult._fields


def test_corrupt_measurements_moves_active_measurements_by_the_given_sigmas():
    pkg = load_pkg()
    b = _batch("cigre14")
    out, ids = pkg.synthetic.corrupt_measurements(b, per_graph=2, sigmas=25.0, seed=3)
    again, ids2 = pkg.synthetic.corrupt_measurements(b, per_graph=2, sigmas=25.0, seed=3)
    assert torch.equal(ids, ids2) and torch.equal(out["x"], again["x"]) and ids.shape == (5, 2) and ids.dtype == torch.int32
    Z0, R0, eZ0, eR0 = wo.denormalised(b["x"], b["edge_attr"], b["stats"])
    Z1, R1, eZ1, eR1 = wo.denormalised(out["x"], out["edge_attr"], b["stats"])
    assert torch.equal(R0, R1) and torch.equal(eR0, eR1)
    z0, z1, w = torch.cat([Z0.reshape(-1), eZ0.reshape(-1)]), torch.cat([Z1.reshape(-1), eZ1.reshape(-1)]), torch.cat([R0.reshape(-1), eR0.reshape(-1)])
    moved = torch.nonzero(z0 != z1).flatten()
    assert sorted(moved.tolist()) == sorted(ids.reshape(-1).tolist())
    N = b["x"].shape[0]
    graph_of = torch.where(ids < 4 * N, ids // 4 // 15, b["edge_index"][0][((ids - 4 * N) // 2).clamp_min(0)] // 15)
    assert torch.equal(graph_of, torch.arange(5)[:, None].expand(5, 2))
    sig = ((z1 - z0) * w.sqrt())[moved]
    assert bool((w[moved] > 0).all()) and float((sig - 25.0).abs().max()) < 1e-2      # (the fp32 rounding of the normalised entry)
