"""CPU: what tests/test_gpu_wls_robust.py relies on, without a GPU.

(a) the ctypes mirror of dss2_wls_robust_args against the header, the exported entries, wls_robust's signature and the refusals
    that need no device;
(b) the oracle of tests/wls_robust_oracle.py against tests/wls_oracle.py where the two must coincide exactly (gamma = inf; every iteration
    plain), and on uncorrupted batches at gamma = 3 (nothing is down-weighted, the plain solution within 2e-7);
(c) what the Huber estimator is for: on cigre14, ober_sub, n33 and ober179 with one gross error of 25 sigma per graph the converged set
    {q < 1} is exactly the corrupted measurements, and the state's error against the clean solution is below half of plain WLS's
    (measured: 0.18, 0.11, 0.11, 0.13 of it);
(d) no active measurement of any GPU-test case has |t - gamma| <= 1e-6 gamma in the oracle at the trip counts the GPU tests use: the
    sets {q < 1} can be compared without exceptions;
(e) the bounds of the GPU test, measured in the oracle alone: per (case, trip count, plain_iters) the worst, over perm_seed 1 .. 4, of
    |fp32(state) - state with the measurements entering G in a permuted order|, of |q - q'| and of the objective's relative difference.
    The literals the GPU test uses must cover max(floor, 8 x spread) and must not be looser than that by more than half;
(f) the corrupted batches of the GPU test's convergence cases converge in the oracle, and at most 10 % of their graphs decide within a
    factor 4 of tol = 1e-6 (the re-weighted iteration converges linearly: the batches where most graphs do are left to fixed trip counts).
"""
import ctypes
import inspect

import pytest
import torch

import test_gpu_wls_robust as gpu_test
import wls_edge_cases as ec
import wls_large_cases as lc
import wls_oracle as wo
import wls_robust_oracle as ro
from conftest import load_pkg

TABLE = ["cigre14", "ober_sub", "n33", "ober179"]


def test_struct_layout_matches_the_header():
    """The solve's block at offset 0 and what follows it (tests/test_abi_cpu.py holds every field to the header)."""
    lib = load_pkg()._lib
    cls = lib.WlsRobustArgs
    assert cls._fields_[0] == ("solve", lib.WlsSolveArgs) and cls.solve.offset == 0
    assert ctypes.sizeof(cls) == ctypes.sizeof(lib.WlsSolveArgs) + 56


def test_host_side():
    pkg = load_pkg()
    lib, est = pkg._lib, pkg.estimator
    for name in ("dss2_wls_robust", "dss2_wls_robust_large"):
        assert name in lib.EXPORTED_SYMBOLS
    assert pkg.wls_robust is est.wls_robust and pkg.WLSRobustResult is est.WLSRobustResult
    assert est.WLSRobustResult._fields == est.WLSResult._fields + ("bus_q", "edge_q", "n_downweighted")
    plain, robust = inspect.signature(est.wls_estimate).parameters, inspect.signature(est.wls_robust).parameters
    assert list(robust) == list(plain)[:-1] + ["gamma", "plain_iters", "large", "max_groups"]
    assert (robust["gamma"].default, robust["plain_iters"].default, robust["large"].default, robust["max_iter"].default) == (3.0, 1, None, 20)
    b = ro.corrupted("n33")[0]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        est.wls_robust(b["x"], b["edge_index"], b["edge_attr"], *b["stats"], 33)
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError, match="gamma must be > 0"):
            est.wls_robust(b["x"], b["edge_index"], b["edge_attr"], *b["stats"], 33, gamma=bad)
    with pytest.raises(ValueError, match="plain_iters"):
        est.wls_robust(b["x"], b["edge_index"], b["edge_attr"], *b["stats"], 33, plain_iters=-1)
    with pytest.raises(ValueError, match="bad_data and robust"):
        pkg.runner.evaluate_wls([], b["stats"], 33, bad_data=dict(threshold=3.0), robust=dict(gamma=3.0))


@pytest.mark.parametrize("name", ["star10", "cigre14", "n33"])
def test_the_oracle_is_the_plain_one_where_nothing_is_reweighted(name):
    b = ro.corrupted(name)[0]
    for kw in (dict(max_iter=3, tol=0.0), dict(max_iter=20, tol=1e-6)):
        plain = wo.solve(*ec.args(b), **kw)
        for perm_seed in (None, 3):
            ref = wo.solve(*ec.args(b), perm_seed=perm_seed, **kw)
            flat = ro.solve_huber(*ec.args(b), gamma=float("inf"), plain_iters=0, perm_seed=perm_seed, **kw)
            for f in ("state", "objective", "iterations", "status", "last_step"):
                assert torch.equal(flat[f], ref[f]), (name, kw, f)
            assert flat["steps"] == ref["steps"]
            assert bool((flat["bus_q"] == 1).all()) and bool((flat["edge_q"] == 1).all()) and bool((flat["n_downweighted"] == 0).all())
        late = ro.solve_huber(*ec.args(b), gamma=ro.GAMMA, plain_iters=kw["max_iter"], **kw)
        for f in ("state", "iterations", "status", "last_step"):
            assert torch.equal(late[f], plain[f]), (name, kw, f)
        assert bool((late["objective"] <= plain["objective"]).all()) and int(late["n_downweighted"].sum()) >= b["num_graphs"]
        assert (late["gamma"], late["plain_iters"], late["perm_seed"]) == (ro.GAMMA, kw["max_iter"], None) and len(late["t"]) == b["num_graphs"]


@pytest.mark.parametrize("name", ["cigre14", "ober_sub", "n33"])
def test_clean_data_are_not_downweighted_at_gamma_3(name):
    plain = lc.oracle(name, 20, 1e-6)
    ref = ro.oracle(name, 20, 1e-6, clean=True)
    diff = (ref["state"] - plain["state"]).abs().max().item()
    print(f"[wls robust clean] {name}: n_downweighted {ref['n_downweighted'].tolist()} largest t {max(float(t.max()) for t in ref['t']):.2f} "
          f"state against plain WLS {diff:.1e}/2e-07")
    assert bool((ref["status"] == 0).all()) and bool((ref["n_downweighted"] == 0).all())
    assert bool((ref["bus_q"] == 1).all()) and bool((ref["edge_q"] == 1).all())
    assert diff <= 2e-7                                        # (both stop within tol of one solution)
    assert (ref["objective"] - plain["objective"]).abs().max() <= 1e-6 * plain["objective"].abs().max()


@pytest.mark.parametrize("name", TABLE)
def test_one_gross_error_per_graph_is_found_and_its_effect_more_than_halved(name):
    b, ids = ro.corrupted(name)
    clean = lc.oracle(name, 20, 1e-6)
    plain = wo.solve(*ec.args(b), max_iter=20, tol=1e-6)
    ref = ro.oracle(name, 20, 1e-6)
    assert bool((clean["status"] == 0).all()) and bool((plain["status"] == 0).all()) and bool((ref["status"] == 0).all())
    e_plain = (plain["state"] - clean["state"]).abs().max().item()
    e_huber = (ref["state"] - clean["state"]).abs().max().item()
    print(f"[wls robust table] {name}: iterations plain {plain['iterations'].tolist()} huber {ref['iterations'].tolist()}; state error against "
          f"the clean solution plain {e_plain:.1e} huber {e_huber:.1e} ({e_huber / e_plain:.2f})")
    assert ro.downweighted_ids(ref) == sorted(ids) and ref["n_downweighted"].tolist() == [1] * b["num_graphs"]
    assert e_huber < 0.5 * e_plain


def _gpu_cases():
    names = list(dict.fromkeys(gpu_test.LDS_CASES + gpu_test.LARGE_CASES))
    return [(name, it, plain) for name in names for it in gpu_test.trip_counts(name) for plain in gpu_test.PLAIN_ITERS]


def test_the_gpu_cases_are_what_the_issue_lists():
    assert gpu_test.LDS_CASES == ["two_bus", "star10", "ring6_parallel", "n33", "cigre14", "mixed", "ober_sub", "n32", "n64", "n65", "n99"]
    assert gpu_test.LARGE_CASES == gpu_test.LDS_CASES[:7] + ["n100", "n128", "n179t", "ober179", "cap"]
    assert gpu_test.trip_counts("cap") == (1, 3) and gpu_test.trip_counts("ober179") == (1, 3, 8, 14) and gpu_test.trip_counts("n99") == (1, 3, 8)
    assert gpu_test.GAMMA == ro.GAMMA == 3.0 and gpu_test.PLAIN_ITERS == (0, 1)
    assert [ro.corrupted(name)[0]["num_graphs"] for name in ("mixed", "cap", "cigre14", "n99", "ober179")] == [7, 1, 5, 3, 3]
    for key in list(gpu_test.STATE_BOUNDS) + list(gpu_test.Q_BOUNDS):
        assert key in _gpu_cases(), key


@pytest.mark.parametrize("name", list(dict.fromkeys(gpu_test.LDS_CASES + gpu_test.LARGE_CASES)))
def test_the_gpu_tests_bounds_cover_the_oracles_spread(name):
    for it in gpu_test.trip_counts(name):
        for plain in gpu_test.PLAIN_ITERS:
            ref = ro.oracle(name, it, 0.0, plain)
            assert bool((ref["status"] == 1).all()) and bool((ref["iterations"] == it).all())
            # (d) nothing sits on the threshold, and after the first iteration the weight path is exercised widely
            assert sum(ro.near_threshold(ref)) == 0, (name, it, plain)
            assert bool((ref["n_downweighted"] >= 1).all())
            if it >= 3:
                assert ref["n_downweighted"].tolist() == [1 + (name == "mixed" and g == 2) for g in range(ref["n_downweighted"].numel())]
            spread = qs = obj = 0.0
            for seed in (1, 2, 3, 4):
                other = ro.oracle(name, it, 0.0, plain, seed)
                spread = max(spread, (ref["state"].float().double() - other["state"]).abs().max().item())
                qs = max(qs, (ref["bus_q"] - other["bus_q"]).abs().max().item(), (ref["edge_q"] - other["edge_q"]).abs().max().item())
                obj = max(obj, ((ref["objective"] - other["objective"]).abs() / ref["objective"].abs()).max().item())
                assert ro.downweighted_ids(other) == ro.downweighted_ids(ref)
            s_lit, s_meas = gpu_test.state_bound(name, it, plain), max(gpu_test.STATE_FLOOR, 8.0 * spread)
            q_lit, q_meas = gpu_test.q_bound(name, it, plain), max(gpu_test.Q_FLOOR, 8.0 * qs)
            print(f"[wls robust bounds] {name} {it} iterations, plain_iters {plain}: state spread {spread:.2e} -> {s_meas:.2e}, the GPU test uses "
                  f"{s_lit:.2e}; q spread {qs:.2e} -> {q_meas:.2e}, uses {q_lit:.2e}; objective spread {obj:.2e} relative / {gpu_test.OBJ_BOUND:.0e}; "
                  f"down-weighted {ref['n_downweighted'].tolist()}")
            assert s_meas <= s_lit <= 1.5 * s_meas, (name, it, plain, spread, s_lit)
            assert q_meas <= q_lit <= 1.5 * q_meas, (name, it, plain, qs, q_lit)
            assert 8.0 * obj <= gpu_test.OBJ_BOUND == 1e-6
    assert gpu_test.STATE_FLOOR == lc.state_bound(0.0) == 5e-7 and gpu_test.Q_FLOOR == 1e-9


def test_the_corrupted_batches_converge_and_few_graphs_are_undecided():
    total = out = 0
    for name in gpu_test.CONVERGENCE_CASES:
        ref = ro.oracle(name, 20, gpu_test.TOL)
        skip = wo.undecided(ref, gpu_test.TOL)
        total, out = total + skip.numel(), out + int(skip.sum())
        print(f"[wls robust convergence] {name}: iterations {ref['iterations'].tolist()} last steps {['%.1e' % v for v in ref['last_step'].tolist()]} "
              f"undecided {skip.tolist()} down-weighted {ref['n_downweighted'].tolist()}")
        assert bool((ref["status"] == 0).all()), name
        assert sum(ro.near_threshold(ref)) == 0
    assert "ober179" not in gpu_test.CONVERGENCE_CASES and set(gpu_test.CONVERGENCE_CASES) & set(lc.SIZES) and set(gpu_test.CONVERGENCE_CASES) & set(ec.SIZES)
    assert total == gpu_test.CONVERGENCE_GRAPHS == 30 and 0 < out <= 0.1 * total, (out, total)
