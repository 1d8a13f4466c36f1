"""CPU: what tests/test_gpu_wls_bad_data_large.py relies on, without a GPU -- estimator.wls_bad_data_large, the blocked form of the
bad-data kernel (csrc/dss2_wls_bad_data.hip, csrc/dss2_wls_large_invert.hpp), on the batches of tests/wls_large_cases.py: n100, n128,
n179t (three graphs each), ober179 (three) and cap (one graph of 256 buses); 13 graphs.

(a) csrc/dss2_wls_large_invert.hpp's inversion schedule restated in numpy ON ITS STORAGE LAYOUT (wl_row_off's block rows; the two passes
    over block rows of 16; the panel Pt[q][k] and the diagonal block in LDS; the owner of a column; the rows a sum runs over), against
    LAPACK's potri at 200, 256, 358 and 512 states and at 15, 16, 17 and 33.  Every entry outside the stored triangle (the part of a
    diagonal block above the diagonal, the b row, the padding rows) and the panel start as NaN: a read of any of them would show.
    Bound: 8 x the difference between two fp64 summation orders of the same inverse from the same L (potri against
    (L^-1)^T (L^-1) by triangular solves), entry (i, j) in units of sqrt(Sigma_ii Sigma_jj) -- measured 5e-16 .. 4.4e-14 for the two
    orders, 9e-16 .. 4.8e-14 for the schedule against potri (a fifth to a seventh of the bound).  (With the factorisation in another elimination order as well the two routes differ by
    1e-10 .. 9e-10 at condition numbers of 2e11 .. 4e11: that is the scale of what the GPU tests below compare, not of this test.)
(b) the fixtures of the GPU tests, measured in the fp64 oracle (tests/wls_bad_data_oracle.py) alone and printed (run with -s):
    * the share of active measurements with S inside [s_min / 2, 2 s_min], which the rN comparison leaves out: at most 10 % per case at
      s_min = 1e-4 (2.7 %, 3.0 %, 3.6 %, 1.7 %, 4.2 % on n100, n128, n179t, ober179, cap; at the default 1e-3 it is 11.5 .. 15 % on the
      trees, which is why the comparisons pass s_min = 1e-4);
    * the spread of three fp64 routes to S and state_std -- the QR's leverages, the normal equations, the normal equations with the
      measurements entering G in permuted orders: on the trees at most 4.6e-9 and 2.4e-11 absolute, so the constants of
      tests/test_gpu_wls_bad_data.py hold (SENS_BOUND 2e-7, STD_BOUND 3.44e-9); on ober179 (condition number 2.4e13) up to 1.8e-6 and
      2.0e-7, so the bounds there are max(the constant, 8 x the spread measured here) -- `bounds(name)`, imported by the GPU test;
      the rN bound follows as there: the S bound at the floor, sens / (2 s_min), in units of max(rN, 1);
    * one +25 sigma error per graph at the measurement of largest S (threshold 4, max_removals 3, the default s_min, 8 iterations, tol 0):
      the oracle removes exactly the target, with every arg-max 1e-3 away from the threshold and every removal leading its runner-up by
      1e-3 (test_gpu_wls_bad_data.py's _decided), on 11 of the 13 graphs; n100 graph 1 (a near-tie, lead 2e-7) and ober179 graph 2
      (lead 3.4e-4) are the two left out, and exactly these;
    * three errors (ranks 0, 1, 2; max_removals 5): all three targets removed, every decision clear, on n179t, ober179 graphs 0 and 1, cap.
(c) the host side that needs no GPU.
"""
import ctypes
import functools
import inspect

import numpy as np
import pytest
import torch

import wls_bad_data_oracle as bo
import wls_edge_cases as we
import wls_large_cases as lc
import wls_oracle as wo
from conftest import load_pkg
from test_wls_large_cpu import NB, TILE, graph_doubles, row_off

FIXED = dict(max_iter=8, tol=0.0)
S_MIN_CMP = 1e-4                     # the s_min of the comparisons against the oracle
SENS_BOUND, STD_BOUND, LEAD = 2e-7, 8 * 4.3e-10, 1e-3          # tests/test_gpu_wls_bad_data.py's
TREES = ("n100", "n128", "n179t", "cap")
ONE_ERROR_LEFT_OUT = [("n100", 1), ("ober179", 2)]
THREE_ERRORS = {"n179t": (0, 1, 2), "ober179": (0, 1), "cap": (0,)}


# ---- (a) the inversion schedule

def blocked_invert(L):
    """Sigma = (L L^T)^-1 by wl_invert's steps on wl_invert's arrays: A (the workspace slice), Pt (the panel, [16][S]), Ld, invd.  The
    owners of the columns j run side by side here (one outer product per row k): per (q, j) the sum over k is the kernel's, k ascending,
    over exactly the columns j < 16 (k / 16 + 1) the kernel's loop over block rows reaches.  Returns (Sigma, barriers)."""
    ns = L.shape[0]
    A = np.full(graph_doubles(ns), np.nan)
    for r in range(ns):
        A[row_off(r):row_off(r) + r + 1] = L[r, :r + 1]
    S = (ns + 1 + TILE - 1) // TILE * TILE
    last = (ns - 1) // NB
    lanes = np.arange(NB)
    barriers = 1
    for sweep in (0, 1):
        for i0 in range(0, ns, NB):
            w, bi = min(NB, ns - i0), i0 // NB
            st, rows = NB * (bi + 1), row_off(i0)
            Pt = np.full((NB, S), np.nan)
            barriers += 2
            if sweep == 0:
                for q in range(NB):
                    Pt[q, :i0] = A[rows + q * st:rows + q * st + i0] if q < w else 0.0
                Ld = np.eye(NB)
                for q in range(w):
                    Ld[q, :q + 1] = A[rows + q * st + i0:rows + q * st + i0 + q + 1]
                invd = 1.0 / np.diag(Ld)
            else:
                for k in range(i0, ns):
                    v = A[row_off(k) + i0:row_off(k) + i0 + NB]
                    Pt[:, k] = np.where((lanes < w) & (i0 + lanes <= k), v, 0.0)
            J = i0 + w
            kend, kb1 = (i0, bi) if sweep == 0 else (ns, last + 1)
            T = np.zeros((NB, J))
            for kb in range(0 if sweep == 0 else bi, kb1):
                jmax = min(J, NB * (kb + 1))              # (pass 0: the columns j whose loop starts at j / 16 <= kb)
                for k in range(kb * NB, min(kend, kb * NB + NB)):
                    x = A[row_off(k):row_off(k) + jmax]
                    x = np.where(np.arange(jmax) <= k, x, 0.0)
                    assert k < S and np.isfinite(Pt[:, k]).all(), "the panel is read where it was not written"
                    T[:, :jmax] += Pt[:, k][:, None] * x[None, :]
            if sweep == 0:
                T = -T
                for c in range(w):
                    T[:, i0 + c] = 0.0
                    T[c, i0 + c] = 1.0
                for q in range(NB):
                    T[q] *= invd[q]
                    T[q + 1:] -= Ld[q + 1:, q][:, None] * T[q][None, :]
            for q in range(w):
                jn = min(J, i0 + q + 1)
                A[rows + q * st:rows + q * st + jn] = T[q, :jn]
    Sg = np.zeros((ns, ns))
    for r in range(ns):
        Sg[r, :r + 1] = A[row_off(r):row_off(r) + r + 1]
        above = A[row_off(r) + r + 1:row_off(r) + NB * (r // NB + 1)]
        assert np.isnan(above).all(), "an entry above the diagonal was written"
    assert np.isnan(A[row_off(ns):]).all(), "the b row or a padding row was written"
    assert np.isfinite(Sg).all()
    return Sg + np.tril(Sg, -1).T, barriers


@functools.lru_cache(maxsize=None)
def _gain(name):
    gr = wo.graphs_of(*we.args(lc.batch(name)))[0]
    u = torch.zeros(2 * gr.n, dtype=torch.float64)
    u[0::2] = 1.0
    return gr.normal_equations(u)[0].numpy()


@pytest.mark.parametrize("name,ns", [("n100", 200), ("n128", 256), ("n179t", 358), ("cap", 512), ("n100", NB - 1), ("n100", NB), ("n100", NB + 1),
                                     ("n100", 2 * NB + 1)])
def test_blocked_inversion_restated_on_the_kernels_layout(name, ns):
    G = _gain(name)[:ns, :ns]                       # (a leading block of a positive definite matrix is one)
    assert G.shape == (ns, ns)
    L = np.linalg.cholesky(G)
    mine, barriers = blocked_invert(L)
    Lt = torch.from_numpy(L)
    ref = torch.cholesky_inverse(Lt).numpy()                       # LAPACK potri
    X = torch.linalg.solve_triangular(Lt, torch.eye(ns, dtype=torch.float64), upper=False)
    other = (X.T @ X).numpy()                                      # the same inverse from the same L, summed in another order
    d = np.sqrt(np.diag(ref))
    scale = d[:, None] * d[None, :]
    spread = (np.abs(other - ref) / scale).max()
    err = (np.abs(mine - ref) / scale).max()
    bound = 8.0 * spread
    print(f"[bad-data large inversion] {name} ns={ns}: schedule - potri {err:.1e} / {bound:.1e} (8 x the two orders' {spread:.1e}), "
          f"condition number {np.linalg.cond(G):.1e}, {barriers} barriers")
    assert spread > 0.0 and err <= bound
    assert barriers == 4 * ((ns + NB - 1) // NB) + 1
    assert np.array_equal(mine, mine.T)


# ---- (b) the fixtures of the GPU tests

def args(b):
    return b["x"], b["edge_index"], b["edge_attr"], b["stats"], b["nodes_per_graph"]


@functools.lru_cache(maxsize=None)
def clean(name):
    """The oracle on the data as they are, at the comparisons' s_min."""
    return bo.bad_data(*args(lc.batch(name)), s_min=S_MIN_CMP, **FIXED)


@functools.lru_cache(maxsize=None)
def corrupted(name, ranks=(0,)):
    """+25 sigma at the measurements of the largest S (one per rank and graph): (host batch, targets per rank)."""
    b = lc.batch(name)
    targets = [bo.largest_sensitivity_targets(*args(b), rank=r) for r in ranks]
    x2, ea2 = bo.add_gross_errors(b["x"], b["edge_attr"], b["stats"], [t for per_rank in targets for t in per_rank])
    return dict(b, x=x2, edge_attr=ea2), targets


REMOVAL_KW = {(0,): dict(threshold=4.0, max_removals=3, **FIXED), (0, 1, 2): dict(threshold=4.0, max_removals=5, **FIXED)}


@functools.lru_cache(maxsize=None)
def removal_oracle(name, ranks=(0,), perm_seed=None):
    return bo.bad_data(*args(corrupted(name, ranks)[0]), perm_seed=perm_seed, **REMOVAL_KW[ranks])


def decided(ref, threshold=4.0):
    """tests/test_gpu_wls_bad_data.py's rule: every arg-max LEAD away from the threshold, every removal LEAD ahead of its runner-up."""
    out = []
    for dec in ref["decisions"]:
        ok = True
        for _, best, second in dec:
            ok = ok and abs(best - threshold) >= LEAD * threshold and (best <= threshold or best - second >= LEAD * best)
        out.append(ok)
    return out


@functools.lru_cache(maxsize=None)
def removal_state_spread(name, ranks=(0,)):
    """Per graph: the worst, over perm_seed 1 and 2, of |fp32(final state) - final state with G summed in a permuted order| (as
    tests/test_wls_large_cpu.py measures the plain solve's, there over four seeds: every figure here is 6e-8 at most, so
    wls_large_cases.state_bound gives its floor of 5e-7 either way); only meaningful where the graph's decisions are clear."""
    ref = removal_oracle(name, ranks)
    n = lc.batch(name)["nodes_per_graph"]
    worst = torch.zeros(len(ref["decisions"]), dtype=torch.float64)
    for seed in (1, 2):
        other = removal_oracle(name, ranks, seed)
        worst = torch.maximum(worst, (ref["state"].float().double() - other["state"]).abs().reshape(-1, 2 * n).max(1).values)
    return worst


@functools.lru_cache(maxsize=None)
def route_spread(name):
    """(S, state_std): the worst absolute difference between the QR route and the normal equations, the latter in the measurements' own
    order and in two permuted ones, at the oracle's state of the clean data."""
    b = lc.batch(name)
    n = b["nodes_per_graph"]
    state = clean(name)["state"]
    e_s = e_std = 0.0
    for g, gr in enumerate(wo.graphs_of(*args(b))):
        u = state[g * n:(g + 1) * n].reshape(-1)
        S, std = bo.sens_qr(gr, u)
        gen = torch.Generator().manual_seed(5 + g)
        for perm in (None, torch.randperm(gr.z.shape[0], generator=gen), torch.randperm(gr.z.shape[0], generator=gen)):
            S2, std2 = bo.sens_normal(gr, u, perm)
            e_s, e_std = max(e_s, float((S - S2).abs().max())), max(e_std, float((std - std2).abs().max()))
    return e_s, e_std


def bounds(name):
    """(S bound, state_std bound) of a case: the constants of tests/test_gpu_wls_bad_data.py, or 8 x the fp64 routes' own spread where
    that is larger (ober179).  Never from the kernel."""
    e_s, e_std = route_spread(name)
    return max(SENS_BOUND, 8.0 * e_s), max(STD_BOUND, 8.0 * e_std)


def rn_bound(name, s_min):
    """The S bound at the floor, as tests/test_gpu_wls_bad_data.py derives it: in units of max(rN, 1), where the oracle's S >= 2 s_min."""
    return bounds(name)[0] / (2.0 * s_min)


@pytest.mark.parametrize("name", lc.ALL)
def test_few_sensitivities_fall_close_to_s_min(name):
    res = clean(name)
    S = torch.cat([res["bus_sens"].reshape(-1), res["edge_sens"].reshape(-1)])
    active = sum(int((gr.w > 0).sum()) for gr in wo.graphs_of(*args(lc.batch(name))))
    near = int(((S >= S_MIN_CMP / 2) & (S <= 2 * S_MIN_CMP)).sum())
    print(f"[bad-data large s_min] {name}: {near} of {active} active measurements ({100.0 * near / active:.1f} %) have S within a factor 2 of {S_MIN_CMP:.0e}")
    assert near <= 0.1 * active
    assert bool((res["status"] == 1).all()) and bool((res["iterations"] == FIXED["max_iter"]).all()) and bool((res["n_removed"] == 0).all())


@pytest.mark.parametrize("name", lc.ALL)
def test_fp64_routes_spread_gives_the_bounds(name):
    e_s, e_std = route_spread(name)
    sens, std = bounds(name)
    print(f"[bad-data large routes] {name}: S {e_s:.2e} state_std {e_std:.2e} between the fp64 routes -> bounds {sens:.2e}, {std:.2e}; "
          f"rN bound at s_min = {S_MIN_CMP:.0e}: {rn_bound(name, S_MIN_CMP):.2e}")
    assert sens == max(SENS_BOUND, 8.0 * e_s) and std == max(STD_BOUND, 8.0 * e_std)
    if name in TREES:
        assert 8.0 * e_s <= SENS_BOUND and 8.0 * e_std <= STD_BOUND and (sens, std) == (SENS_BOUND, STD_BOUND)
    else:
        assert e_s <= 1e-5 and e_std <= 1e-6          # (ober179: 1.8e-6 and 2.0e-7 measured; an order of magnitude more would be another problem)


def test_one_error_per_graph_which_graphs_decide_clearly():
    left_out = []
    for name in lc.ALL:
        hb, (targets,) = corrupted(name)
        ref = removal_oracle(name)
        ok = decided(ref)
        leads = [(d[0][1] - d[0][2]) / d[0][1] for d in ref["decisions"]]
        print(f"[bad-data large one error] {name}: targets {targets} removed {ref['removed'][:, 0].tolist()} rN {['%.2f' % v for v in ref['removed_rn'][:, 0].tolist()]} "
              f"leads {['%.1e' % v for v in leads]} decided {ok} state spread {['%.1e' % v for v in removal_state_spread(name).tolist()]}")
        for g, good in enumerate(ok):
            if good:
                assert ref["removed"][g].tolist() == [targets[g], -1, -1] and int(ref["n_removed"][g]) == 1
            else:
                left_out.append((name, g))
    assert left_out == ONE_ERROR_LEFT_OUT


def test_three_errors_per_graph_are_all_removed_clearly():
    for name, graphs in THREE_ERRORS.items():
        hb, targets = corrupted(name, (0, 1, 2))
        ref = removal_oracle(name, (0, 1, 2))
        ok = decided(ref)
        print(f"[bad-data large three errors] {name}: targets {targets} removed {ref['removed'].tolist()} decided {ok} "
              f"state spread {['%.1e' % v for v in removal_state_spread(name, (0, 1, 2)).tolist()]}")
        for g in graphs:
            assert ok[g] and int(ref["n_removed"][g]) == 3
            assert sorted(ref["removed"][g, :3].tolist()) == sorted(t[g] for t in targets) and ref["removed"][g, 3:].tolist() == [-1, -1]


# ---- (c) the host side

def test_struct_mirror_has_the_workspace_at_its_end():
    lib = load_pkg()._lib
    cls = lib.WlsBadDataArgs
    assert cls._fields_[0] == ("solve", lib.WlsSolveArgs) and cls.solve.offset == 0
    assert cls._fields_[-2:] == [("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_uint64)]
    assert cls.workspace.offset == cls.state_std.offset + 8 and ctypes.sizeof(cls) == cls.workspace_bytes.offset + 8
    zero = cls()
    assert zero.workspace is None and zero.workspace_bytes == 0      # (a zero-initialised block selects the LDS form)


def test_python_side_without_a_gpu(monkeypatch):
    pkg = load_pkg()
    est = pkg.estimator
    # the size refusal comes after every ValueError and before anything touches the device: with the device check out of the way a
    # host batch reaches it (and nothing beyond it)
    cap = est.max_nodes_per_graph_large()
    with monkeypatch.context() as m:
        m.setattr(est, "_require_gpu", lambda *tensors: None)
        x, ea, ei = torch.zeros(cap + 1, 11), torch.zeros(cap, 13), torch.zeros(2, cap, dtype=torch.int64)
        stats = lc.batch("n100")["stats"]
        with pytest.raises(NotImplementedError, match=f"at most {cap} buses per graph, got {cap + 1}"):
            est.wls_bad_data_large(x, ei, ea, *stats, cap + 1)
        with pytest.raises(NotImplementedError, match=f"at most {cap} buses per graph, got {cap + 1}"):
            est.wls_bad_data_large(x, ei, ea, *stats, cap + 1, graph_ptr=torch.tensor([0, cap + 1]))
        with pytest.raises(NotImplementedError, match="at most 99 buses per graph, got 100"):
            est.wls_bad_data(x[:100], ei, ea, *stats, 100)
    assert pkg.wls_bad_data_large is est.wls_bad_data_large and "wls_bad_data_large" in pkg.__all__
    assert inspect.signature(est.wls_bad_data_large) == inspect.signature(est.wls_bad_data)
    assert "graph_ptr" not in inspect.signature(est.wls_bad_data_large).parameters
    b = lc.batch("n100")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        est.wls_bad_data_large(b["x"], b["edge_index"], b["edge_attr"], *b["stats"], 100)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        est.wls_bad_data_large(b["x"], b["edge_index"], b["edge_attr"], *b["stats"], 100, graph_ptr=torch.tensor([0, 100, 200, 300]))


def test_evaluate_wls_refuses_an_unknown_large():
    pkg = load_pkg()
    stats = lc.batch("n33")["stats"]
    for bad in ("nonsense", None, 1, "Auto"):
        with pytest.raises(ValueError, match="large"):
            pkg.runner.evaluate_wls([], stats, 33, bad_data=dict(threshold=3.0, large=bad))
    given = dict(threshold=3.0, large="auto")
    pkg.runner.evaluate_wls([], stats, 33, bad_data=given)
    assert given == dict(threshold=3.0, large="auto")                # (the caller's dict is not the one the key is taken off)
