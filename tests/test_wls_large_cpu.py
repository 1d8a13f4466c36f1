"""CPU: what tests/test_gpu_wls_large.py relies on, without a GPU.

(a) the ctypes mirror of dss2_wls_large_args against the header, and the host arithmetic of the entry's queries;
(b) the bounds of the GPU test, measured in the fp64 oracle alone: per case and trip count the worst, over perm_seed 1 .. 4, of
    |fp32(state of wls_oracle.solve) - state with the measurements entering G in a permuted order|; the bound is
    max(5e-7, 8 x spread) (wls_large_cases.state_bound).  The literals the GPU test uses must cover what is measured here and must not
    be looser than that by more than half.  Measured (run with -s): trees and the cap graph at most 6.0e-8 at every trip count, so
    5e-7; ober179 2.9e-7 .. 3.1e-7, 8.4e-8 .. 1.0e-7, 5.9e-8, 6.0e-8 after 1, 3, 8, 14 iterations (condition number 2.4e13, first
    step 0.64; the ranges are two machines' BLAS summation orders), so 2.5e-6, 8.2e-7, 5e-7, 5e-7; the objective's spread at most
    3.6e-8 relative (ober179, one iteration; 8 x that is below the 1e-6 bound);
(c) csrc/dss2_wls_large.hip's blocked factorisation restated in numpy ON ITS STORAGE LAYOUT (wl_row_off, the 16-column blocks, the
    transposed panel with its stride, the 8 x 8 tiles with their triangular numbering and both store paths, the blocked back
    substitution), against numpy.linalg.cholesky / solve on the oracle's G at 200, 256 and 358 states and at 15, 16 and 17: the index
    arithmetic at block and tile edges, before anything runs on a GPU.  The panel starts as NaN, as uninitialised LDS may: a tile
    entry stored without being inside the triangle would show.
"""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

import test_gpu_wls_large as gpu_test
import wls_large_cases as lc
import wls_oracle as wo
from conftest import load_pkg

NB, TILE = 16, 8


def test_struct_layout_matches_the_header():
    """The solve's block at offset 0 and what follows it (tests/test_abi_cpu.py holds every field to the header)."""
    lib = load_pkg()._lib
    cls = lib.WlsLargeArgs
    assert cls._fields_[0] == ("solve", lib.WlsSolveArgs) and cls.solve.offset == 0
    assert ctypes.sizeof(cls) == ctypes.sizeof(lib.WlsSolveArgs) + 16


def row_off(r):
    R = r // NB
    return NB * NB * (R * (R + 1) // 2) + (r % NB) * NB * (R + 1)


def graph_doubles(ns):
    nbr = (ns + NB) // NB
    return NB * NB * (nbr * (nbr + 1) // 2)


def test_queries_and_host_side():
    pkg = load_pkg()
    L, lib, est = pkg._lib.lib(), pkg._lib, pkg.estimator
    cap = L.dss2_wls_large_max_nodes()
    assert cap == est.max_nodes_per_graph_large() == lc.CAP and cap >= 256
    for name in ("dss2_wls_solve_large", "dss2_wls_large_workspace_bytes", "dss2_wls_large_groups", "dss2_wls_large_max_nodes",
                 "dss2_wls_large_lds_bytes"):
        assert name in lib.EXPORTED_SYMBOLS
    # the workspace is the layout of the restatement below, per workgroup; rows never overlap and the last one ends inside
    for n in (1, 2, 7, 8, 15, 70, 99, 100, 128, 179, cap):
        ns = 2 * n
        assert L.dss2_wls_large_workspace_bytes(n, 1) == 8 * graph_doubles(ns)
        assert L.dss2_wls_large_workspace_bytes(n, 37) == 37 * 8 * graph_doubles(ns)
        ends = [row_off(r) + NB * (r // NB + 1) for r in range(ns + 1)]
        assert all(row_off(r + 1) == ends[r] for r in range(ns)) and ends[-1] <= graph_doubles(ns)
        assert all(r < NB * (r // NB + 1) for r in range(ns + 1))
        assert 0 < L.dss2_wls_large_lds_bytes(n) <= 160 * 1024
    assert 2 * L.dss2_wls_large_lds_bytes(cap) <= 160 * 1024
    assert L.dss2_wls_large_workspace_bytes(cap + 1, 1) == 0 and L.dss2_wls_large_workspace_bytes(0, 1) == 0
    assert L.dss2_wls_large_workspace_bytes(15, 0) == 0 and L.dss2_wls_large_lds_bytes(cap + 1) == 0
    # the grid: one workgroup per graph up to the library's 512, max_groups honoured, 0 for arguments the entry refuses
    a = lib.WlsSolveArgs()
    a.nodes_per_graph = 179
    for graphs, max_groups, want in ((3, 0, 3), (3, 2, 2), (1024, 0, 512), (1024, 7, 7), (1024, 4096, 512)):
        a.n_nodes, a.max_groups = 179 * graphs, max_groups
        assert L.dss2_wls_large_groups(ctypes.byref(a)) == want
    a.n_nodes = 179 * 3 + 1
    assert L.dss2_wls_large_groups(ctypes.byref(a)) == 0
    a.n_nodes, a.nodes_per_graph = (cap + 1) * 2, cap + 1
    assert L.dss2_wls_large_groups(ctypes.byref(a)) == 0 and L.dss2_wls_large_groups(None) == 0
    # Python: the signature of wls_estimate, no CPU fallback
    assert inspect.signature(est.wls_estimate_large) == inspect.signature(est.wls_estimate)
    assert pkg.wls_estimate_large is est.wls_estimate_large
    b = lc.batch("n100")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        est.wls_estimate_large(b["x"], b["edge_index"], b["edge_attr"], *b["stats"], 100)


def _trip_counts(name):
    return sorted(it for (case, it) in gpu_test.STATE_BOUNDS if case == name)


@pytest.mark.parametrize("name", lc.ALL)
def test_the_gpu_tests_bounds_cover_the_oracles_spread(name):
    assert _trip_counts(name) == {"cap": [1, 3], "ober179": [1, 3, 8, 14]}.get(name, [1, 3, 8])
    for it in _trip_counts(name):
        ref = lc.oracle(name, it, 0.0)
        assert bool((ref["status"] == 1).all()) and bool((ref["iterations"] == it).all())
        spread = obj = 0.0
        for seed in (1, 2, 3, 4):
            other = lc.oracle(name, it, 0.0, seed)
            spread = max(spread, (ref["state"].float().double() - other["state"]).abs().max().item())
            obj = max(obj, ((ref["objective"] - other["objective"]).abs() / ref["objective"].abs()).max().item())
        literal, measured = gpu_test.STATE_BOUNDS[(name, it)], lc.state_bound(spread)
        print(f"[wls large bounds] {name} {it} iterations: spread {spread:.2e} -> bound {measured:.2e}, the GPU test uses {literal:.2e}; "
              f"objective spread {obj:.2e} relative / {gpu_test.OBJ_BOUND:.0e}")
        assert measured <= literal <= 1.5 * measured, (name, it, spread, literal)
        assert 8.0 * obj <= gpu_test.OBJ_BOUND == 1e-6


def test_the_trees_converge_in_four_iterations_and_few_graphs_are_undecided():
    total = out = 0
    for name in gpu_test.CONVERGENCE_CASES:
        ref = lc.oracle(name, 20, gpu_test.TOL)
        skip = wo.undecided(ref, gpu_test.TOL)
        total, out = total + skip.numel(), out + int(skip.sum())
        assert bool((ref["status"] == 0).all()), name
        if name in lc.SIZES:
            print(f"[wls large convergence] {name}: iterations {ref['iterations'].tolist()} last steps {['%.1e' % v for v in ref['last_step'].tolist()]} "
                  f"undecided {skip.tolist()}")
            assert ref["iterations"].tolist() == [4, 4, 4]
    assert total == 36 and out <= 0.1 * total, (out, total)


# ---- (c) the blocked factorisation of csrc/dss2_wls_large.hip on its storage layout

def blocked_solve(G, b):
    """(L [ns, ns], y, du, ok) by the kernel's steps on the kernel's arrays: A (the workspace slice), Pt (the transposed panel), Ld, invd."""
    ns = len(b)
    A = np.zeros(graph_doubles(ns))
    for r in range(ns):
        A[row_off(r):row_off(r) + r + 1] = G[r, :r + 1]
    A[row_off(ns):row_off(ns) + ns] = b
    S = (ns + 1 + TILE - 1) // TILE * TILE
    Pt = np.full((NB, S), np.nan)
    ok = True
    for j0 in range(0, ns, NB):
        w = min(NB, ns - j0)
        j1 = j0 + w
        # a. the diagonal block, lane i holds row i
        D = np.zeros((NB, NB))
        for i in range(w):
            D[i, :i + 1] = A[row_off(j0 + i) + j0:row_off(j0 + i) + j0 + i + 1]
        for j in range(NB):
            d = D[j, j]
            good = d > 0 and math.isfinite(d)
            if j < w:
                ok = ok and good
            s = math.sqrt(d) if good else 1.0
            D[j + 1:, j] /= s
            D[j, j] = s
            for k in range(j + 1, NB):
                D[k:, k] -= D[k:, j] * D[k, j]
        Ld = np.zeros((NB, NB))
        for i in range(w):
            Ld[i, :i + 1] = D[i, :i + 1]
            A[row_off(j0 + i) + j0:row_off(j0 + i) + j0 + i + 1] = D[i, :i + 1]
        invd = 1.0 / np.diag(D)
        assert (invd[w:] == 1.0).all()
        # b. the panel, the b row included: 16 entries of each row, whatever the block's width
        for i in range(j1, ns + 1):
            x = A[row_off(i) + j0:row_off(i) + j0 + NB].copy()
            for j in range(NB):
                x[j] *= invd[j]
                x[j + 1:] -= x[j] * Ld[j + 1:, j]
            A[row_off(i) + j0:row_off(i) + j0 + NB] = x
            Pt[:, i] = x
        # c. the trailing update on 8 x 8 tiles of the lower triangle of tiles
        if j1 < ns:
            ntr = (ns + 1 - j1 + TILE - 1) // TILE
            for p in range(ntr * (ntr + 1) // 2):
                ti = int((math.sqrt(8.0 * p + 1.0) - 1.0) * 0.5)
                while ti * (ti + 1) // 2 > p:
                    ti -= 1
                while (ti + 1) * (ti + 2) // 2 <= p:
                    ti += 1
                tj = p - ti * (ti + 1) // 2
                i0, c0 = j1 + TILE * ti, j1 + TILE * tj
                assert i0 + TILE <= S and c0 + TILE <= S
                with np.errstate(invalid="ignore"):
                    acc = Pt[:, i0:i0 + TILE].T @ Pt[:, c0:c0 + TILE]
                if tj < ti and i0 + TILE - 1 <= ns:
                    for q in range(TILE):
                        A[row_off(i0 + q) + c0:row_off(i0 + q) + c0 + TILE] -= acc[q]
                else:
                    for q in range(TILE):
                        i = i0 + q
                        for c in range(TILE):
                            if i <= ns and c0 + c <= i and c0 + c < ns:
                                A[row_off(i) + c0 + c] -= acc[q, c]
    assert np.isfinite(A).all()
    L = np.zeros((ns, ns))
    for r in range(ns):
        L[r, :r + 1] = A[row_off(r):row_off(r) + r + 1]
    y = A[row_off(ns):row_off(ns) + ns].copy()
    # the blocked back substitution
    du = y.copy()
    for j0 in range((ns - 1) // NB * NB, -1, -NB):
        w = min(NB, ns - j0)
        for j in range(w - 1, -1, -1):
            xj = du[j0 + j] * (1.0 / A[row_off(j0 + j) + j0 + j])
            du[j0 + j] = xj
            for k in range(j):
                du[j0 + k] -= A[row_off(j0 + j) + j0 + k] * xj
        for c in range(j0):
            for j in range(w):
                du[c] -= A[row_off(j0 + j) + c] * du[j0 + j]
    return L, y, du, ok


def _normal_equations(name):
    gr = wo.graphs_of(*lc.we.args(lc.batch(name)))[0]
    u = torch.zeros(2 * gr.n, dtype=torch.float64)
    u[0::2] = 1.0
    Gm, b = gr.normal_equations(u)
    return Gm.numpy(), b.numpy()


@pytest.mark.parametrize("name,ns", [("n100", 200), ("n128", 256), ("n179t", 358), ("n100", NB - 1), ("n100", NB), ("n100", NB + 1),
                                     ("n100", 2 * NB + TILE), ("n100", 2 * NB + TILE + 1)])
def test_blocked_factorisation_restated_on_the_kernels_layout(name, ns):
    G, b = _normal_equations(name)
    G, b = G[:ns, :ns], b[:ns]                      # (a leading block of a positive definite matrix is one)
    assert G.shape == (ns, ns)
    L, y, du, ok = blocked_solve(G, b)
    assert ok
    Lref = np.linalg.cholesky(G)
    # both factorisations are backward stable: entries agree to a few ulps of the row's scale times the growth a Cholesky allows
    scale = np.sqrt(np.diag(G))[:, None]
    err_L = (np.abs(L - Lref) / scale).max()
    resid = np.abs(L @ L.T - G).max() / np.abs(G).max()
    ref_du = np.linalg.solve(G, b)
    cond = np.linalg.cond(G)
    err_du = np.abs(du - ref_du).max() / np.abs(ref_du).max()
    back = np.abs(G @ du - b).max() / (np.abs(G).max() * np.abs(du).max() + np.abs(b).max())
    err_y = np.abs(y - np.linalg.solve(Lref, b)).max() / np.abs(y).max()
    print(f"[wls large restatement] {name} ns={ns}: L {err_L:.1e} residual {resid:.1e} y {err_y:.1e} du {err_du:.1e} (cond {cond:.1e}) backward {back:.1e}")
    assert resid <= 1e-13 and back <= 1e-13
    assert err_L <= 1e-6 and err_y <= 1e-6                       # (an index slip moves entries by their own size)
    assert err_du <= 100.0 * cond * np.finfo(float).eps
    assert np.array_equal(np.triu(L, 1), np.zeros_like(L))
