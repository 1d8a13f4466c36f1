"""CPU: the fp64 oracle of the WLS state estimator (tests/wls_oracle.py) pinned from several sides, the cases the GPU tests rest on
(tests/wls_cases.py), and the host-side facts of the new entry point (struct layout, LDS helper).

The oracle's measurement function is tied to oracle/dss2_oracle.py's gsp_wls_edge -- the function the reference goldens pin -- through
the objective; its analytic Jacobian to autograd; the Gauss-Newton iteration to known answers (noise-free measurements recomputed in
fp64 from the labels) and to the 64 real CIGRE samples.  Figures measured here (fp64, this file's batches):
  objective against gsp_wls_edge       equal to all twelve printed digits (cigre14, ober_sub)
  Jacobian against autograd            <= 2.7e-16 of the largest entry
  noise-free, flat start               4 to 5 iterations; with tol = 1e-7 the state ends 2e-15 (cigre14), 5e-15 (mixed), 1e-14 (ober_sub) from the labels
  real CIGRE samples                   3 to 4 iterations at tol = 1e-6; max |dV| 0.0116 p.u., max |dtheta| 0.0078 rad against pandapower's labels
  hand-built shapes                    3 to 4 iterations at tol = 1e-6
  permuted measurement order           state changes by <= 9e-15 after 8 iterations
  decisions within a factor 4 of tol   1 of 27 graphs
"""
import os

import numpy as np
import pytest
import torch

import dss2_oracle
import wls_cases as wc
import wls_oracle as wo
from conftest import GOLDEN, load_pkg

F64 = torch.float64
TOL = 1e-6


def _solve(b, **kw):
    return wo.solve(b["x"], b["edge_index"], b["edge_attr"], b["stats"], b["nodes_per_graph"], **kw)


@pytest.mark.parametrize("name", ["cigre14", "ober_sub"])
def test_objective_equals_the_reference_pinned_loss(name):
    """weights = (lam_v, lam_p, lam_pf), lam_reg = 0: sum_g objective[g, 0] / N + sum_g objective[g, 1] / E is gsp_wls_edge's value at
    the same state (normalised for it)."""
    b = wc.grid_batch(name)
    reg = dict(dss2_oracle.DEFAULT_REG_COEFS, lam_reg=0.0)
    res = _solve(b, max_iter=2, tol=0.0, weights=(reg["lam_v"], reg["lam_p"], reg["lam_pf"]))
    x, ea = b["x"].to(F64), b["edge_attr"].to(F64)
    st = tuple(s.to(F64) for s in b["stats"])
    out = torch.stack([(res["state"][:, 0] - st[0][0]) / st[1][0], res["state"][:, 1]], 1)
    want = dss2_oracle.gsp_wls_edge(input=x[:, :8], edge_input=ea[:, :6], output=out, x_mean=st[0], x_std=st[1], edge_mean=st[2],
                                    edge_std=st[3], edge_index=b["edge_index"], reg_coefs=reg, num_samples=None, node_param=x[:, 8:],
                                    edge_param=ea[:, 6:]).item()
    got = (res["objective"][:, 0].sum() / x.shape[0] + res["objective"][:, 1].sum() / ea.shape[0]).item()
    print(f"[wls-oracle objective] {name}: {got:.12e} against {want:.12e}")
    assert want > 0
    assert abs(got - want) <= 1e-9 * want


@pytest.mark.parametrize("name", wc.ALL_BATCHES)
def test_analytic_jacobian_equals_autograd(name):
    b = wc.any_batch(name)
    gen = torch.Generator().manual_seed(7)
    for gr in wo.graphs_of(b["x"], b["edge_index"], b["edge_attr"], b["stats"], b["nodes_per_graph"])[:2]:
        u = torch.zeros(2 * gr.n, dtype=F64)
        u[0::2] = 1.0 + 0.05 * torch.randn(gr.n, dtype=F64, generator=gen)
        u[1::2] = 0.1 * torch.randn(gr.n, dtype=F64, generator=gen)
        H = wo.jacobian(u, gr.f, gr.t, gr.par, gr.kk)
        A = torch.autograd.functional.jacobian(lambda q: wo.h_flat(q, gr.f, gr.t, gr.par, gr.kk), u)
        err = (H - A).abs().max().item() / A.abs().max().item()
        print(f"[wls-oracle jacobian] {name}: {err:.2e}")
        assert err <= 1e-10


@pytest.mark.parametrize("name", list(wc.GRID_BATCHES))
def test_noise_free_measurements_give_back_the_state(name):
    """Measurements recomputed in fp64 from the labels: a flat start reaches the labels within 1e-6 in at most 6 iterations."""
    b = wc.grid_batch(name)
    if name == "mixed":
        assert len({int(((b["edge_index"][0] // 15) == g).sum()) for g in range(7)}) == 2, "the mixed batch holds one structure only"
    gs = wo.graphs_of(b["x"], b["edge_index"], b["edge_attr"], b["stats"], b["nodes_per_graph"])
    y = b["y"].to(F64)
    n = b["nodes_per_graph"]
    for g, gr in enumerate(gs):
        assert bool((y[g * n:(g + 1) * n, 1][gr.slack] == 0).all())
        gr.z = wo.h_flat(y[g * n:(g + 1) * n].reshape(-1), gr.f, gr.t, gr.par, gr.kk)
    res = _solve(b, max_iter=6, tol=1e-7, graphs=gs)
    err = (res["state"] - y).abs().max().item()
    print(f"[wls-oracle noise-free] {name}: error {err:.2e} after {res['iterations'].tolist()} iterations")
    assert err <= 1e-6 and bool((res["status"] == 0).all())


def test_real_cigre_samples_converge():
    z = np.load(os.path.join(GOLDEN, "cigre14_real64.npz"))
    t = lambda k: torch.from_numpy(z[k])
    res = wo.solve(t("x"), t("edge_index"), t("edge_attr"), tuple(t(k) for k in ("x_mean", "x_std", "edge_mean", "edge_std")), 15,
                   max_iter=6, tol=TOL)
    print(f"[wls-oracle real] iterations {sorted(set(res['iterations'].tolist()))}, max |dV| {(res['state'][:, 0] - t('y')[:, 0]).abs().max():.4f}, "
          f"max |dtheta| {(res['state'][:, 1] - t('y')[:, 1]).abs().max():.4f}")
    assert bool((res["status"] == 0).all()) and int(res["iterations"].max()) <= 6


@pytest.mark.parametrize("name", list(wc.SHAPES))
def test_hand_built_shapes_converge(name):
    b = wc.batch(name)
    n, edges, _ = wc.SHAPES[name]
    assert b["x"].shape == (3 * n, 11) and b["edge_index"].shape == (2, 3 * len(edges))
    w = wo.denormalised(b["x"], b["edge_attr"], b["stats"])
    assert all(bool(((r == 0) | ((r >= 99.0) & (r <= 1.01e6))).all()) for r in (w[1], w[3])), "weights outside [1e2, 1e6]"
    res = _solve(b, max_iter=8, tol=TOL)
    print(f"[wls-oracle shapes] {name}: iterations {res['iterations'].tolist()}")
    assert bool((res["status"] == 0).all())


def test_shapes_are_what_their_names_say():
    deg = lambda name: np.bincount(np.array(wc.SHAPES[name][1]).reshape(-1), minlength=wc.SHAPES[name][0])
    assert deg("star10")[0] == 9 and (deg("star10")[1:] == 1).all()
    ring = wc.SHAPES["ring6_parallel"][1]
    assert (1, 2) in ring and (2, 1) in ring and (deg("ring6_parallel") >= 2).all()
    n33 = wc.SHAPES["n33"]
    assert n33[0] == 33 and len(n33[1]) == 32 and 2 * n33[0] > 64 and deg("n33").max() == 3


def test_summation_order_moves_the_state_by_less_than_1e_7():
    for name in ("cigre14", "ober_sub", "star10"):
        b = wc.any_batch(name)
        a = _solve(b, max_iter=8, tol=0.0)
        p = _solve(b, max_iter=8, tol=0.0, perm_seed=5)
        d = (a["state"] - p["state"]).abs().max().item()
        print(f"[wls-oracle order] {name}: {d:.2e}")
        assert d < 1e-7


def test_few_decisions_fall_close_to_the_tolerance():
    """The GPU convergence test compares status and iteration counts except where the oracle's deciding step is within a factor 4 of
    tol: with these seeds that is at most 10 % of the graphs."""
    total = close = 0
    for name in wc.ALL_BATCHES:
        res = _solve(wc.any_batch(name), max_iter=12, tol=TOL)
        u = wo.undecided(res, TOL)
        total, close = total + u.numel(), close + int(u.sum())
        assert bool((res["status"] == 0).all())
    print(f"[wls-oracle decisions] {close} of {total} graphs decide within a factor 4 of tol")
    assert close >= 1 and close <= 0.1 * total


def test_a_graph_without_measurements_fails_cleanly():
    b = wc.grid_batch("cigre14")
    x, ea = b["x"].clone(), b["edge_attr"].clone()
    x[30:45, :8] = 0.0
    ea[(b["edge_index"][0] // 15) == 2, :4] = 0.0
    res = wo.solve(x, b["edge_index"], ea, b["stats"], 15, max_iter=8, tol=TOL)
    assert res["status"].tolist() == [0, 0, 2, 0, 0]
    assert int(res["iterations"][2]) == 0 and bool((res["state"][30:45, 0] == 1).all()) and bool((res["state"][30:45, 1] == 0).all())


def test_lds_helper_admits_the_grids_and_refuses_179_buses():
    pkg = load_pkg()
    L = pkg._lib.lib()
    cap = 160 * 1024
    assert 0 < L.dss2_wls_solve_lds_bytes(15) <= cap and L.dss2_wls_solve_lds_bytes(70) <= cap
    assert L.dss2_wls_solve_lds_bytes(70) >= 140 * 141 // 2 * 8           # the packed gain matrix alone
    assert L.dss2_wls_solve_lds_bytes(179) > cap
    assert pkg.estimator.max_nodes_per_graph() == max(n for n in range(1, 200) if L.dss2_wls_solve_lds_bytes(n) <= cap)
    assert 70 <= pkg.estimator.max_nodes_per_graph() < 179
