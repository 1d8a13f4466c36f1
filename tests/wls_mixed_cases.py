"""Batches that MIX bus counts for the WLS estimators' graph_ptr path, shared by tests/test_wls_mixed_cpu.py (which holds every one of
them to facts in the fp64 oracles) and tests/test_gpu_wls_mixed.py.

A batch is a list of (shape, graph number): graphs out of tests/wls_cases.py's generator -- its own shapes, tests/wls_edge_cases.py's
n1, n64 and n99, tests/wls_large_cases.py's trees -- collated one after the other with wls_cases' statistics; `graph_ptr` holds the
row offsets, `sizes` the bus counts, `nodes_per_graph` the BOUND (the largest bus count), `edge_ptr` the offsets of the graphs' stored
branches (a graph's branches are contiguous, in the generator's order).

  A    bound 33: the wide (four-wave) LDS kernel with two-bus and one-bus graphs inside it
  B    bound 99: the LDS cap
  C    bound 179: the blocked kernel, sizes from 1 to 179 in one launch
  D    bound 256: the blocked kernel's cap next to a two-bus graph
  cigre_ober, ober_ober179    synthetic.make_batch on two grids of different bus counts (15 + 70: LDS; 70 + 179: blocked)
  R_lds, R_blocked, BD        the robust and the bad-data mixes: no n1 (every graph has a 3 kV bus, so the oracles of those two, which
                              take V_lv from the graph they are given, see the batch's V_lv), one gross error of 25 sigma per graph
                              placed by synthetic.corrupt_measurements (global ids, through graph_ptr)

The oracle is tests/wls_oracle.py's `solve`, run PER GRAPH on the graph's cut of the batch with kk = V_lv^2 from the WHOLE batch's
minimum of x[:, 8] -- the estimator's rule (n1 alone would give 110 kV instead of 3).  Results are concatenated in batch order.
"""
import functools

import numpy as np
import torch

import wls_bad_data_oracle as bo
import wls_cases as wc
import wls_edge_cases as ec
import wls_large_cases as lc
import wls_oracle as wo
import wls_robust_oracle as ro

F64 = torch.float64

BATCHES = {
    "A": [("two_bus", 0), ("n33", 0), ("n1", 0), ("star10", 0), ("n1", 1), ("n33", 1), ("ring6_parallel", 0)],
    "B": [("n64", 0), ("two_bus", 0), ("n99", 0), ("n1", 0), ("star10", 0)],
    "C": [("two_bus", 0), ("n100", 0), ("n1", 0), ("n33", 0), ("n179t", 0), ("n99", 0), ("n128", 0)],
    "D": [("cap", 0), ("two_bus", 1), ("n100", 1)],
    "R_lds": [("two_bus", 0), ("n33", 0), ("star10", 0), ("ring6_parallel", 0), ("n64", 0)],
    "R_blocked": [("two_bus", 0), ("n100", 0), ("n33", 0), ("n128", 0)],
    "BD": [("star10", 0), ("n33", 0), ("two_bus", 0), ("n64", 0), ("ring6_parallel", 0)],
}
BOUNDS = {"A": 33, "B": 99, "C": 179, "D": 256, "R_lds": 64, "R_blocked": 128, "BD": 64}
GRID_MIXES = {"cigre_ober": (["cigre14", "ober_sub"], 6, 1), "ober_ober179": (["ober_sub", "ober179"], 4, 2)}
FIXED = ["A", "B", "C", "D"]
DECIDED = ["A", "B", "C"]                 # every graph converges and none decides within a factor 4 of tol = 1e-6 (the CPU test asserts it)
ALL = FIXED + list(GRID_MIXES)
LDS = ["A", "B", "cigre_ober"]            # bound <= 99: wls_estimate serves them (and wls_estimate_large does too)
SPREAD_BOUNDED = ["C", "D", "ober_ober179"]   # state bound = wls_large_cases.state_bound(oracle spread); elsewhere the project's 5e-7
TRIP_COUNTS = (1, 3, 8)
STATE_BOUND, OBJ_BOUND, TOL = 5e-7, 1e-6, 1e-6
CORRUPT_SEED = 9                          # (of seeds 0 .. 11 the one whose errors every graph of both robust mixes down-weights, and whose removals are all clear)
PERM_SEEDS = (1, 2, 3, 4)


@functools.lru_cache(maxsize=None)
def spreads(name, it):
    """The oracle's own spread over summation orders at a fixed trip count: the worst, over PERM_SEEDS, of (|fp32(state) - permuted-order
    state| -- tests/test_wls_large_cpu.py's measure --, |state - permuted-order state| in fp64, the objective's relative difference)."""
    ref = oracle(name, it, 0.0)
    rounded = exact = obj = 0.0
    for seed in PERM_SEEDS:
        other = oracle(name, it, 0.0, seed)
        rounded = max(rounded, (ref["state"].float().double() - other["state"]).abs().max().item())
        exact = max(exact, (ref["state"] - other["state"]).abs().max().item())
        live = ref["objective"].abs() > 1e-12
        obj = max(obj, ((ref["objective"] - other["objective"]).abs() / ref["objective"].abs())[live].max().item())
    return rounded, exact, obj


def state_bound(name, it):
    """The project's 5e-7; on C, D and ober_sub + ober179 wls_large_cases.state_bound of the oracle's spread (the same floor, or 8 x the
    spread), formed from the oracle where the test runs -- no literal to go stale with a BLAS's summation order.  Measured: only the
    ober179 graph of ober_sub + ober179 (condition number 2.4e13) leaves the floor, 7.3e-8 after three iterations: 5.8e-7."""
    return lc.state_bound(spreads(name, it)[0]) if name in SPREAD_BOUNDED else STATE_BOUND


def objective_bound(name, it):
    """1e-6 relative; on C, D and ober_sub + ober179 by the same rule, max(1e-6, 8 x the oracle's spread).  Measured: the same graph's bus
    part after ONE iteration is 2.6e-7 apart between two summation orders of the oracle: 2.1e-6 there, the floor everywhere else."""
    return max(OBJ_BOUND, 8.0 * spreads(name, it)[2]) if name in SPREAD_BOUNDED else OBJ_BOUND


def shape_graph(name, k):
    """Graph number k of a shape of wls_cases, wls_edge_cases (n1, n64, n99) or wls_large_cases (the trees)."""
    if name in wc.SHAPES:
        return wc.graph(name, k)
    if name in lc.TREES:
        return wc.graph(name, k, **lc.TREES[name])
    return wc.graph(name, k, **ec.CASES[name])


def collate(graphs):
    """wls_cases.collate for graphs of different sizes: the same normalisation and fp32 rounding, rows and branches one graph after the
    other; plus graph_ptr, edge_ptr, sizes and the bound."""
    xs, eas, ys, eis, ptr, eptr = [], [], [], [], [0], [0]
    for x, ea, y, ed in graphs:
        xn, ean = x.copy(), ea.copy()
        xn[:, :8] = np.where(x[:, :8] != 0, (x[:, :8] - wc.X_MEAN) / wc.X_STD, 0.0)
        ean[:, :6] = np.where(ea[:, :6] != 0, (ea[:, :6] - wc.E_MEAN) / wc.E_STD, 0.0)
        assert ((xn[:, :8] != 0) == (x[:, :8] != 0)).all() and ((ean[:, :4] != 0) == (ea[:, :4] != 0)).all()
        xs.append(xn); eas.append(ean); ys.append(y); eis.append(ed.T.reshape(2, -1) + ptr[-1])
        ptr.append(ptr[-1] + x.shape[0]); eptr.append(eptr[-1] + ea.shape[0])
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(np.concatenate(a))).float()
    stats = tuple(torch.from_numpy(s).float() for s in (wc.X_MEAN, wc.X_STD, wc.E_MEAN, wc.E_STD))
    sizes = [b - a for a, b in zip(ptr, ptr[1:])]
    return {"x": f32(xs), "edge_index": torch.from_numpy(np.ascontiguousarray(np.concatenate(eis, 1))).long(), "edge_attr": f32(eas),
            "y": f32(ys), "stats": stats, "nodes_per_graph": max(sizes), "num_graphs": len(graphs),
            "graph_ptr": torch.tensor(ptr, dtype=torch.int64), "edge_ptr": eptr, "sizes": sizes}


def from_list(items):
    return collate([shape_graph(name, k) for name, k in items])


@functools.lru_cache(maxsize=None)
def batch(name):
    """The host batch of a name of BATCHES or GRID_MIXES."""
    if name in BATCHES:
        b = from_list(BATCHES[name])
        assert b["nodes_per_graph"] == BOUNDS[name]
        return b
    from conftest import load_pkg
    grids, B, seed = GRID_MIXES[name]
    b = load_pkg().synthetic.make_batch(grids, B, seed=seed)
    ptr = b["graph_ptr"].tolist()
    sizes = [q - p for p, q in zip(ptr, ptr[1:])]
    assert len(set(sizes)) == 2, "the seed must draw both grids"
    src = b["edge_index"][0]
    eptr = [int((src < p).sum()) for p in ptr]
    assert all(bool(((src[eptr[g]:eptr[g + 1]] >= ptr[g]) & (src[eptr[g]:eptr[g + 1]] < ptr[g + 1])).all()) for g in range(B)), "branches are grouped by graph"
    return dict(b, nodes_per_graph=max(sizes), sizes=sizes, edge_ptr=eptr)


def cut(b, g):
    """Graph g of a batch as a batch of its own (local bus numbers): x, edge_index, edge_attr, its bus count and its stored branches' ids."""
    lo, hi = int(b["graph_ptr"][g]), int(b["graph_ptr"][g + 1])
    ei = b["edge_index"]
    sel = torch.nonzero((ei[0] >= lo) & (ei[0] < hi)).flatten()
    assert bool(((ei[1, sel] >= lo) & (ei[1, sel] < hi)).all()), "an edge crosses graphs"
    return b["x"][lo:hi], ei[:, sel] - lo, b["edge_attr"][sel], hi - lo, sel


def batch_kk(b):
    """V_lv^2 of the WHOLE batch, in fp64 from the fp32 input: what every graph of it is solved with."""
    return b["x"].double()[:, 8].min() ** 2


def oracle_graphs(b, weights=(1.0, 1.0, 1.0)):
    """One wls_oracle.Graph per graph of the batch, on the graph's cut, with the batch's kk."""
    kk, out = batch_kk(b), []
    for g in range(b["num_graphs"]):
        x, ei, ea, n, _ = cut(b, g)
        Z, R, eZ, eR = wo.denormalised(x, ea, b["stats"])
        out.append(wo.Graph(0, n, x.double(), ei, ea.double(), Z, R, eZ, eR, kk, weights))
    return out


def _joined(b, parts):
    """Per-graph results of wls_oracle.solve (or solve_huber) in batch order as one result."""
    out = {k: torch.cat([p[k] for p in parts]) for k in ("state", "objective", "iterations", "status", "last_step")}
    out["steps"] = [p["steps"][0] for p in parts]
    return out


def solve(b, max_iter, tol, perm_seed=None):
    return _joined(b, [wo.solve(None, None, None, None, gr.n, max_iter=max_iter, tol=tol, perm_seed=perm_seed, graphs=[gr])
                       for gr in oracle_graphs(b)])


@functools.lru_cache(maxsize=None)
def oracle(name, max_iter, tol, perm_seed=None):
    """The per-graph oracle of a batch: computed once, shared, never modified."""
    return solve(batch(name), max_iter, tol, perm_seed)


def reordered(b, order):
    """The graphs of a collated batch of this module in another order (a list of graph numbers; graphs may be left out or repeated)."""
    xs, eas, ys, eis, ptr, eptr = [], [], [], [], [0], [0]
    for g in order:
        x, ei, ea, n, sel = cut(b, g)
        lo = int(b["graph_ptr"][g])
        xs.append(x); eas.append(ea); ys.append(b["y"][lo:lo + n]); eis.append(ei + ptr[-1])
        ptr.append(ptr[-1] + n); eptr.append(eptr[-1] + int(sel.numel()))
    sizes = [q - p for p, q in zip(ptr, ptr[1:])]
    return dict(b, x=torch.cat(xs), edge_attr=torch.cat(eas), y=torch.cat(ys), edge_index=torch.cat(eis, 1), num_graphs=len(order),
                graph_ptr=torch.tensor(ptr, dtype=torch.int64), edge_ptr=eptr, sizes=sizes, nodes_per_graph=b["nodes_per_graph"])


def graph_rows(b, g):
    """(row slice, stored-branch slice) of graph g."""
    return slice(int(b["graph_ptr"][g]), int(b["graph_ptr"][g + 1])), slice(b["edge_ptr"][g], b["edge_ptr"][g + 1])


# ---- the robust and the bad-data mixes: one gross error per graph

@functools.lru_cache(maxsize=None)
def corrupted(name):
    """(host batch with +25 sigma on one active measurement per graph, ids [G] -- GLOBAL ids, placed through graph_ptr)."""
    from conftest import load_pkg
    b = batch(name)
    assert all(float(b["x"][int(p):int(q), 8].min()) == wc.V_LV for p, q in zip(b["graph_ptr"][:-1], b["graph_ptr"][1:])), "every graph needs a 3 kV bus"
    hb, ids = load_pkg().synthetic.corrupt_measurements(b, per_graph=1, sigmas=ro.SIGMAS, seed=CORRUPT_SEED)
    return hb, ids[:, 0].tolist()


def global_id(b, g, n, local):
    """A measurement id of graph g's cut (4 i + k, 4 n + 2 e + k, local numbers) as the batch's id."""
    N = b["x"].shape[0]
    if local < 0:
        return local
    if local < 4 * n:
        return 4 * int(b["graph_ptr"][g]) + local
    return 4 * N + 2 * b["edge_ptr"][g] + (local - 4 * n)


@functools.lru_cache(maxsize=None)
def robust_oracle(name, max_iter, tol, perm_seed=None, gamma=ro.GAMMA, plain_iters=1):
    """wls_robust_oracle.solve_huber per graph of corrupted(name), joined: solve's fields, bus_q [N, 4], edge_q [E, 2], n_downweighted, t."""
    hb, _ = corrupted(name)
    parts = []
    for g, gr in enumerate(oracle_graphs(hb)):
        _, _, ea, n, _ = cut(hb, g)
        parts.append(ro.solve_huber(None, None, ea, None, n, max_iter=max_iter, tol=tol, perm_seed=perm_seed, graphs=[gr], gamma=gamma,
                                    plain_iters=plain_iters))
    out = _joined(hb, parts)
    out["bus_q"], out["edge_q"] = torch.cat([p["bus_q"] for p in parts]), torch.cat([p["edge_q"] for p in parts])
    out["n_downweighted"], out["t"] = torch.cat([p["n_downweighted"] for p in parts]), [p["t"][0] for p in parts]
    return out


@functools.lru_cache(maxsize=None)
def bad_data_oracle(name, max_removals, threshold=4.0, perm_seed=None):
    """wls_bad_data_oracle.bad_data per graph of corrupted(name) (8 iterations, tol = 0), joined, ids made global."""
    hb, _ = corrupted(name)
    parts = []
    for g in range(hb["num_graphs"]):
        x, ei, ea, n, _ = cut(hb, g)
        parts.append(bo.bad_data(x, ei, ea, hb["stats"], n, max_iter=8, tol=0.0, threshold=threshold, max_removals=max_removals, perm_seed=perm_seed))
    out = {k: torch.cat([p[k] for p in parts]) for k in parts[0] if k != "decisions"}
    out["removed"] = torch.tensor([[global_id(hb, g, hb["sizes"][g], int(v)) for v in p["removed"][0].tolist()] for g, p in enumerate(parts)],
                                  dtype=torch.int32)
    out["decisions"] = [[(global_id(hb, g, hb["sizes"][g], w), best, second) for w, best, second in p["decisions"][0]] for g, p in enumerate(parts)]
    return out
