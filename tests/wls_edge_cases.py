"""Inputs for the WLS estimator's kernels at their size limits and on measurement sets the grids never produce, shared by
tests/test_wls_edge_cases_cpu.py (which holds every one of them to facts in the fp64 oracle) and tests/test_gpu_wls_shapes.py.
Everything comes out of tests/wls_cases.py's generator (`graph` with its keyword hooks, 3 kV level, fp64 rounded to fp32 once); three
graphs per case.

Sizes -- radial trees with a few laterals, branch orientation mixed as in n33; n32, n64 and n65 measure V at three buses and a flow on
every sixth branch (with wls_cases' two and two, n64's two fp64 routes to state_std were more than an eighth of the bound apart):
  n32    64 states: the last size of the one-wave kernel, every lane owns a row
  n64    the buses fill wave 0 of the bad-data pass exactly;  n65: the first bus owned by wave 1
  n99    the largest size either entry serves: a hub of degree 13 at bus 70 whose leaves are the last buses (88 .. 98), V measured
         at buses 0, 50 and 98, one flow measured on branch 88 = (70, 89), whose from-end is owned by a thread of wave 1
  n1     one bus, no branch, E = 0 for the whole batch, V the only measurement
Measurement sets:
  pmu, pmu_star   theta measured at every third non-slack bus, on n33 (66 states: the four-wave kernel) and on star10 (one wave)
  no_slack        star10 without a slack flag, theta measured at buses 0, 4 and 8
  two_slack       ring6_parallel with slack flags at buses 0 and 5;  slack_last: n33 whose only slack is bus 32
  all_flows       ring6_parallel with P and Q flow measured on all seven stored branches
  clamped         star10 with V measured at bus 5 too and three weights that de-normalise below 0: V at bus 9, P at bus 4, P flow of
                  branch 3
  multigraph      five buses, a self loop at bus 2 (with a shunt of its own, so that it carries power), the branch 3 - 4 stored three
                  times (twice as (3, 4), once as (4, 3), each with its own parameters), flows measured on all seven
  isolated_pmu    six buses, bus 3 without a branch, its V and theta measured: solvable
  isolated        the same batch with bus 3's theta reading taken away in graph 1: that graph's theta_3 pivot (pivot 7 of 12) is exactly 0
  tie             two buses joined by two stored branches with identical parameters, orientation, flow measurements and weights
Variants of wls_cases' own batches: WEIGHTS on star10 and cigre14; star10 with a NaN in one P measurement of graph 1 (`nan_p`), and with
an infinite V weight in graph 1 (`inf_w`).

Graph numbers: `IDS` picks, per case, three graphs among the first twelve so that, over all cases, at most 10 % of the graphs decide
within a factor 4 of tol = 1e-6 in the fp64 oracle, at most 10 % of the active measurements have S within a factor 2 of s_min (a tree
with P and Q at every bus and little else has about 12 % there), and two fp64 routes of the oracle stay within an eighth of every bound
(n99's graphs 2, 3, 5 and 8 do not).  tests/test_wls_edge_cases_cpu.py checks all three.
"""
import functools

import numpy as np
import torch

import wls_bad_data_oracle as bo
import wls_cases as wc
import wls_oracle as wo

WEIGHTS = (0.37, 2.5, 11.0)


def _tree(n, laterals, leaves_of=None):
    """A chain 0 .. with laterals {first bus of the lateral: the bus it hangs off}; leaves_of = (hub, first leaf): every bus from the
    first leaf on hangs off the hub.  Orientation as in wls_cases._n33."""
    parent = {k: k - 1 for k in range(1, n)}
    parent.update(laterals)
    if leaves_of is not None:
        parent.update({k: leaves_of[0] for k in range(leaves_of[1], n)})
    return [((parent[k], k) if k % 4 else (k, parent[k])) for k in range(1, n)]


_STAR10, _RING6, _N33 = wc.SHAPES["star10"], wc.SHAPES["ring6_parallel"], wc.SHAPES["n33"]
_MULTI = (5, [(0, 1), (2, 1), (2, 2), (2, 3), (3, 4), (3, 4), (4, 3)], list(range(7)))
_ISOLATED = (6, [(0, 1), (2, 1), (2, 4), (4, 5)], [0, 2])
SELF_LOOP, TRIPLE = 2, (4, 5, 6)                      # stored branches of `multigraph`
ISOLATED_BUS, FAILING_GRAPH = 3, 1
NEGATIVE_WEIGHTS = [("x", 9, 1, -4.0e4), ("x", 4, 5, -3.0e3), ("ea", 3, 1, -2.0e3)]
HUB, HUB_BRANCH = 70, 88

# name -> shape (n, edges, measured branches), graph()'s hooks, and hooks of single graphs {position in the batch: hooks}
CASES = {
    "n32": dict(shape=(32, _tree(32, {18: 1, 22: 2, 25: 5}), list(range(0, 31, 6))), v_at=(0, 16, 31)),
    "n64": dict(shape=(64, _tree(64, {18: 1, 40: 5, 52: 30}), list(range(0, 63, 6))), v_at=(0, 32, 63)),
    "n65": dict(shape=(65, _tree(65, {18: 1, 40: 5, 52: 30, 60: 44}), list(range(0, 64, 6))), v_at=(0, 32, 64)),
    "n99": dict(shape=(99, _tree(99, {30: 3, 55: 20, 80: 60}, leaves_of=(HUB, 88)), [0, HUB_BRANCH]), v_at=(0, 50, 98)),
    "n1": dict(shape=(1, [], []), v_at=(0,), pq_at=()),
    "pmu": dict(shape=_N33, theta_at=tuple(range(3, 33, 3))),
    "pmu_star": dict(shape=_STAR10, theta_at=(3, 6, 9)),
    "no_slack": dict(shape=_STAR10, slack=(), theta_at=(0, 4, 8)),
    "two_slack": dict(shape=_RING6, slack=(0, 5)),
    "slack_last": dict(shape=_N33, slack=(32,)),
    "all_flows": dict(shape=(_RING6[0], _RING6[1], list(range(7)))),
    "clamped": dict(shape=_STAR10, v_at=(0, 5, 9), put=NEGATIVE_WEIGHTS),
    "multigraph": dict(shape=_MULTI, par_set={SELF_LOOP: (4.0, -6.0, 0.5, 0.3)}),
    "isolated_pmu": dict(shape=_ISOLATED, v_at=(0, ISOLATED_BUS, 5), theta_at=(ISOLATED_BUS,)),
    "isolated": dict(shape=_ISOLATED, v_at=(0, ISOLATED_BUS, 5), theta_at=(ISOLATED_BUS,), seed_as="isolated_pmu",
                     single={FAILING_GRAPH: dict(put=[("x", ISOLATED_BUS, 2, 0.0), ("x", ISOLATED_BUS, 3, 0.0)])}),
    "tie": dict(shape=(2, [(0, 1), (0, 1)], [0]), same_as={1: 0}),
    "nan_p": dict(shape=_STAR10, seed_as="star10", single={FAILING_GRAPH: dict(put=[("x", 4, 4, float("nan"))])}),
    "inf_w": dict(shape=_STAR10, seed_as="star10", single={FAILING_GRAPH: dict(put=[("x", 9, 1, float("inf"))])}),
}
SIZES = ["n32", "n64", "n65", "n99"]
MEASUREMENT_SETS = ["pmu", "pmu_star", "no_slack", "two_slack", "slack_last", "all_flows", "clamped", "multigraph", "isolated_pmu"]
WEIGHTED = ["star10_weighted", "cigre14_weighted"]
SOLVABLE = SIZES + MEASUREMENT_SETS + ["tie"] + WEIGHTED           # every graph converges in the oracle
FAILING = ["isolated", "nan_p", "inf_w"]                            # graph FAILING_GRAPH ends with status 2, the others converge
# the healthy twin of a failing batch: the same graphs without the one graph's defect
HEALTHY = {"isolated": "isolated_pmu", "nan_p": "star10", "inf_w": "star10"}

IDS = {name: (0, 1, 2) for name in CASES}
IDS.update(n32=(2, 3, 6), n64=(4, 7, 8), n65=(4, 5, 7), n99=(0, 7, 11), pmu=(3, 5, 6), pmu_star=(0, 2, 3), two_slack=(1, 2, 3), slack_last=(6, 7, 10),
           all_flows=(1, 2, 3), tie=(0, 1, 3))


def weights_of(name):
    return WEIGHTS if name in WEIGHTED else (1.0, 1.0, 1.0)


def _graph(name, k, pos):
    kw = dict(CASES[name])
    kw.update(kw.pop("single", {}).get(pos, {}))
    return wc.graph(kw.pop("seed_as", name), k, **kw)


@functools.lru_cache(maxsize=None)
def batch(name):
    """The batch of a case, or of wls_cases (any of its names; `<name>_weighted` is that name's batch, to be solved with WEIGHTS)."""
    if name not in CASES:
        return wc.any_batch(name[:-len("_weighted")] if name.endswith("_weighted") else name)
    return wc.collate([_graph(name, k, pos) for pos, k in enumerate(IDS[name])], CASES[name]["shape"][0])


def args(b):
    return b["x"], b["edge_index"], b["edge_attr"], b["stats"], b["nodes_per_graph"]


@functools.lru_cache(maxsize=None)
def oracle_solve(name, max_iter, tol, perm_seed=None):
    return wo.solve(*args(batch(name)), max_iter=max_iter, tol=tol, weights=weights_of(name), perm_seed=perm_seed)


@functools.lru_cache(maxsize=None)
def oracle_clean(name):
    """The bad-data oracle on the case's data as they are: 8 iterations, tol = 0, no removals."""
    return bo.bad_data(*args(batch(name)), max_iter=8, tol=0.0, weights=weights_of(name))


def graph_rows(b, g):
    """(node rows, stored-edge mask) of graph g of a batch."""
    n = b["nodes_per_graph"]
    return slice(g * n, (g + 1) * n), (b["edge_index"][0] >= g * n) & (b["edge_index"][0] < (g + 1) * n)


def without_feature(name):
    """(batch, weights) of a measurement-set case or a weighted variant with its feature taken out of the INPUTS: theta readings away
    from the slack dropped, the slack put back to bus 0 alone, only wls_cases' own flows kept, the self loop removed, unit weights.
    (`clamped` has no such input: its test hands the oracle the weights as they are.)"""
    b = batch(name)
    n, x, ea, ei = b["nodes_per_graph"], b["x"].clone(), b["edge_attr"].clone(), b["edge_index"]
    local = torch.arange(x.shape[0]) % n
    if name in ("pmu", "pmu_star", "isolated_pmu"):
        x[:, 2:4] = 0.0
    elif name in ("no_slack", "two_slack", "slack_last"):
        x[:, 9] = (local == 0).float()
    elif name == "all_flows":
        keep = torch.tensor([k % 7 in _RING6[2] for k in range(ea.shape[0])])
        ea[~keep, :4] = 0.0
    elif name == "multigraph":
        keep = torch.tensor([k % 7 != SELF_LOOP for k in range(ea.shape[0])])
        ea, ei = ea[keep], ei[:, keep]
    else:
        assert name in WEIGHTED, name
        return b, (1.0, 1.0, 1.0)
    return dict(b, x=x, edge_attr=ea, edge_index=ei), weights_of(name)


def preceded_by_failing_graph(b):
    """The batch with one more graph in front: a copy of graph 0 without any measurement (it fails at pivot 0)."""
    n = b["nodes_per_graph"]
    rows, erows = graph_rows(b, 0)
    x0, ea0, ei0 = b["x"][rows].clone(), b["edge_attr"][erows].clone(), b["edge_index"][:, erows]
    x0[:, :8] = 0.0
    ea0[:, :4] = 0.0
    return dict(b, x=torch.cat([x0, b["x"]]), edge_attr=torch.cat([ea0, b["edge_attr"]]), y=torch.cat([b["y"][rows], b["y"]]),
                edge_index=torch.cat([ei0, b["edge_index"] + n], 1), num_graphs=b["num_graphs"] + 1)


def degrees(name):
    n, edges, _ = CASES[name]["shape"]
    return np.bincount(np.array(edges, dtype=np.int64).reshape(-1), minlength=n)


REMOVAL = dict(max_iter=8, tol=0.0, threshold=4.0)
# n99: graph 0 carries its gross error at P of bus 0, graph 1 at the P flow of HUB_BRANCH (from-end 70), graph 2 at Q of bus 89, the last
# two owned by threads of wave 1.  (Most injections of a tree have a small S: these are bus measurements of large S on either side of
# bus 64, and every removal leads its runner-up by at least 4e-3 in the oracle.)
CROSS_WAVE_BUS_HIGH, CROSS_WAVE_BUS_LOW = 89, 0
FIVE_ERRORS_GRAPH = 2


@functools.lru_cache(maxsize=None)
def cross_wave():
    """n99 with one gross error of +25 sigma per graph: (host batch, ids, the oracle's result with max_removals = 2)."""
    b = batch("n99")
    N, e = b["x"].shape[0], len(CASES["n99"]["shape"][1])
    ids = [4 * (0 * 99 + CROSS_WAVE_BUS_LOW) + 2, 4 * N + 2 * (1 * e + HUB_BRANCH), 4 * (2 * 99 + CROSS_WAVE_BUS_HIGH) + 3]
    x2, ea2 = bo.add_gross_errors(b["x"], b["edge_attr"], b["stats"], ids)
    hb = dict(b, x=x2, edge_attr=ea2)
    return hb, ids, bo.bad_data(*args(hb), max_removals=2, **REMOVAL)


@functools.lru_cache(maxsize=None)
def five_errors():
    """wls_cases' n33 batch with five gross errors on graph 2, at the five largest sensitivities: (host batch, ids, the oracle's result
    with max_removals = 64)."""
    b = batch("n33")
    ids = [bo.largest_sensitivity_targets(*args(b), rank=r)[FIVE_ERRORS_GRAPH] for r in range(5)]
    x2, ea2 = bo.add_gross_errors(b["x"], b["edge_attr"], b["stats"], ids)
    hb = dict(b, x=x2, edge_attr=ea2)
    return hb, ids, bo.bad_data(*args(hb), max_removals=64, **REMOVAL)


@functools.lru_cache(maxsize=None)
def tied():
    """`tie` with a gross error on the Q flow of both stored branches of every graph: (host batch, ids [G][2], the oracle's result with
    max_removals = 1)."""
    b = batch("tie")
    N = b["x"].shape[0]
    ids = [[4 * N + 2 * (2 * g) + 1, 4 * N + 2 * (2 * g + 1) + 1] for g in range(b["num_graphs"])]
    x2, ea2 = bo.add_gross_errors(b["x"], b["edge_attr"], b["stats"], [i for pair in ids for i in pair])
    hb = dict(b, x=x2, edge_attr=ea2)
    return hb, ids, bo.bad_data(*args(hb), max_removals=1, **REMOVAL)
