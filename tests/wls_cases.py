"""Small hand-built graphs for the WLS state estimator, shared by tests/test_wls_oracle_cpu.py (which holds every shape to convergence in
the fp64 oracle) and tests/test_gpu_wls_solve.py.

  two_bus          n = 2, one branch: the smallest gain matrix (4 states, one of them a slack angle)
  star10           a hub of degree 9 (its injection's Jacobian row has 20 non-zeros), branches stored in both orientations
  ring6_parallel   a ring of six buses with one branch doubled, the copy stored the other way round with its own parameters
  n33              a radial feeder of 33 buses with three laterals: 66 states, just over one wave (the multi-wave kernel at its smallest)

Each graph has a random true state (a voltage profile falling along the tree from the slack bus), V measured at two buses, P and Q at
every bus, one or two branch flows, weights drawn log-uniformly from [1e2, 1e6] and gaussian noise of standard deviation weight^-1/2.
The voltage level (V_LV = 3 kV: flows scale with V_LV^2) puts the gain matrices' condition numbers at 6e7 .. 4e11, the bundled grids'
own range (3e11 .. 3e12) at its upper end: at 10 kV they reach 5e13 and two summation orders of the fp64 ORACLE differ by 3.5e-6 in the
objective after one iteration, more than the bound the estimator is held to; at 3 kV by 6e-8.
Everything is drawn in fp64 and normalised with fixed, non-trivial statistics, then rounded to fp32 once: the oracle and the kernel read
the same numbers.  `batch(name)` collates three graphs of one shape with different states and measurements.

`graph` takes keyword hooks (another shape, slack buses, theta readings, raw entries written last ...) for tests/wls_edge_cases.py; with
their defaults it draws what it always drew, and `collate` makes a batch of any list of its graphs.

`grid_batch(name)`: the batches of the bundled grids the GPU tests use (synthetic.make_batch; the only thing taken from the product).
Their seeds are chosen so that, at tol = 1e-6, at most 10 % of the graphs of all batches together take a deciding step within a
factor 4 of the tolerance in the fp64 oracle (tests/test_wls_oracle_cpu.py checks it).
"""
import zlib

import numpy as np
import torch


def _ring6_parallel():
    return 6, [(0, 1), (1, 2), (2, 3), (4, 3), (4, 5), (5, 0), (2, 1)], [0, 6]


def _star10():
    return 10, [((0, k) if k % 2 else (k, 0)) for k in range(1, 10)], [0, 3]


def _n33():
    parent = {k: k - 1 for k in range(1, 33)}
    parent[18], parent[22], parent[25] = 1, 2, 5          # three laterals
    return 33, [((parent[k], k) if k % 4 else (k, parent[k])) for k in range(1, 33)], [0, 17]


SHAPES = {"two_bus": (2, [(0, 1)], [0]), "star10": _star10(), "ring6_parallel": _ring6_parallel(), "n33": _n33()}

# (mean, std) of the 8 node and the first 6 edge feature columns: arbitrary, fixed, away from every measured value
X_MEAN = np.array([0.51, 3.0e3, 0.013, 2.0e3, 0.21, 5.0e3, -0.17, 4.0e3])
X_STD = np.array([0.37, 7.0e4, 0.11, 3.0e4, 1.9, 6.0e4, 1.3, 8.0e4])
E_MEAN = np.array([0.33, 6.0e3, -0.29, 2.5e3, 0.0, 0.0])
E_STD = np.array([2.3, 9.0e4, 1.7, 5.0e4, 1.0, 1.0])
V_LV, V_HV = 3.0, 110.0


def _flows(v, th, f, t, par, kk):
    G, B, Gs, Bs = par.T
    vi, vj, d = v[f], v[t], th[f] - th[t]
    c, s = np.cos(d), np.sin(d)
    pf = (-vi * vj * (G * c + B * s) + (G + Gs / 2) * vi ** 2) * kk
    qf = (vi * vj * (-G * s + B * c) - (B + Bs / 2) * vi ** 2) * kk
    pt = (-vi * vj * (G * c - B * s) + (G + Gs / 2) * vj ** 2) * kk
    qt = (vi * vj * (G * s + B * c) - (B + Bs / 2) * vj ** 2) * kk
    return pf, qf, pt, qt


def graph(name, k=0, *, shape=None, slack=(0,), v_at=None, theta_at=(), pq_at=None, par_set=None, same_as=None, put=()):
    """Raw (un-normalised) x [n, 11], edge_attr [e, 13], y [n, 2], edges [e, 2] of graph number k of a shape, fp64.

    The keyword hooks are tests/wls_edge_cases.py's; with their defaults every draw and every number is what it was without them.
      shape      (n, edges, measured branches) in place of SHAPES[name]; a bus no branch reaches gets a state of its own
      slack      the buses whose slack flag is set (their true angle is 0: the profile is shifted to the first, the others are set)
      v_at       the buses whose V is measured (default: 0 and n - 1);  theta_at: those whose theta is measured
      pq_at      the buses whose P and Q are measured (default: all)
      par_set    {branch: (G, B, Gs, Bs)};  same_as {branch: branch}: parameters and flow measurement copied from another branch
      put        [("x" | "ea", row, column, raw value)] written last -- a negative weight, a NaN, an Inf
    Whatever the hooks need beyond the draws of the plain graph comes from a second generator."""
    n, edges, meas_branches = SHAPES[name] if shape is None else shape
    rng = np.random.default_rng(zlib.crc32(f"wls/{name}/{k}".encode()))
    extra = np.random.default_rng(zlib.crc32(f"wls/{name}/{k}/hooks".encode()))
    e = len(edges)
    f, t = np.array([a for a, _ in edges], dtype=np.int64), np.array([b for _, b in edges], dtype=np.int64)
    # the state: bus 0 is the slack; voltage and angle fall along the tree (a ring's closing branch just joins two such values)
    v, th = np.zeros(n), np.zeros(n)
    v[0] = rng.uniform(1.0, 1.04)
    seen = {0}
    grew = True
    while len(seen) < n and grew:
        grew = False
        for a, b in edges:
            for p, c in ((a, b), (b, a)):
                if p in seen and c not in seen:
                    v[c] = v[p] - rng.uniform(0.0, 0.004)
                    th[c] = th[p] - rng.uniform(0.0, 0.004)
                    seen.add(c)
                    grew = True
    for c in sorted(set(range(n)) - seen):                  # (a bus without a path to bus 0)
        v[c], th[c] = extra.uniform(0.97, 1.03), -extra.uniform(0.0, 0.02)
    if tuple(slack) != (0,) and len(slack):
        th = th - th[slack[0]]
        th[list(slack)] = 0.0
    par = np.stack([rng.uniform(1.0, 20.0, e), -rng.uniform(1.0, 20.0, e), np.zeros(e), rng.uniform(0.0, 2e-3, e)], 1)
    for b, row in (par_set or {}).items():
        par[b] = row
    for b, src in (same_as or {}).items():
        par[b] = par[src]
    pf, qf, pt, qt = _flows(v, th, f, t, par, V_LV ** 2)
    p, q = np.zeros(n), np.zeros(n)
    np.add.at(p, t, -pt); np.add.at(p, f, -pf)
    np.add.at(q, t, -qt); np.add.at(q, f, -qf)

    def weight(size, gen=rng):
        return 10.0 ** gen.uniform(2.0, 6.0, size)

    x = np.zeros((n, 11))
    wv = weight(n)
    for i in ((0, n - 1) if v_at is None else v_at):       # V at two buses
        x[i, 0], x[i, 1] = v[i] + rng.normal() / np.sqrt(wv[i]), wv[i]
    wp, wq = weight(n), weight(n)
    x[:, 4], x[:, 5] = p + rng.normal(size=n) / np.sqrt(wp), wp
    x[:, 6], x[:, 7] = q + rng.normal(size=n) / np.sqrt(wq), wq
    if pq_at is not None:
        x[sorted(set(range(n)) - set(pq_at)), 4:8] = 0.0
    for i in theta_at:
        w = weight(None, extra)
        x[i, 2], x[i, 3] = th[i] + extra.normal() / np.sqrt(w), w
    x[:, 8] = V_LV
    x[0, 8] = V_HV
    x[list(slack), 9] = 1.0
    ea = np.zeros((e, 13))
    for b in meas_branches:
        w = weight(2)
        ea[b, 0], ea[b, 1] = pf[b] + rng.normal() / np.sqrt(w[0]), w[0]
        ea[b, 2], ea[b, 3] = qf[b] + rng.normal() / np.sqrt(w[1]), w[1]
    for b, src in (same_as or {}).items():
        ea[b, :4] = ea[src, :4]
    ea[:, 4:6] = par[:, :2]
    ea[:, 6:10] = par
    ea[:, 10] = 1.0
    ea[:, 12] = 0.4
    for which, row, col, value in put:
        (x if which == "x" else ea)[row, col] = value
    return x, ea, np.stack([v, th], 1), np.stack([f, t], 1).reshape(e, 2)


# the graph numbers of a shape's batch (see the module docstring: star10 keeps one graph -- number 2 -- whose deciding step is within
# a factor 4 of tol = 1e-6, so that the convergence test's exclusion is exercised)
GRAPH_IDS = {name: (0, 1, 2) for name in SHAPES}


def collate(graphs, n):
    """Graphs (the tuples `graph` returns, n buses each) as one batch in the layout of synthetic.make_batch: x [N, 11],
    edge_index [2, E], edge_attr [E, 13] (normalised, fp32), y [N, 2], stats, nodes_per_graph."""
    xs, eas, ys, eis = [], [], [], []
    for pos, (x, ea, y, ed) in enumerate(graphs):
        xn, ean = x.copy(), ea.copy()
        xn[:, :8] = np.where(x[:, :8] != 0, (x[:, :8] - X_MEAN) / X_STD, 0.0)
        ean[:, :6] = np.where(ea[:, :6] != 0, (ea[:, :6] - E_MEAN) / E_STD, 0.0)
        assert ((xn[:, :8] != 0) == (x[:, :8] != 0)).all() and ((ean[:, :4] != 0) == (ea[:, :4] != 0)).all()
        xs.append(xn); eas.append(ean); ys.append(y); eis.append(ed.T + pos * n)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(np.concatenate(a))).float()
    stats = tuple(torch.from_numpy(s).float() for s in (X_MEAN, X_STD, E_MEAN, E_STD))
    return {"x": f32(xs), "edge_index": torch.from_numpy(np.ascontiguousarray(np.concatenate(eis, 1))).long(), "edge_attr": f32(eas),
            "y": f32(ys), "stats": stats, "nodes_per_graph": n, "num_graphs": len(graphs)}


def batch(name, ids=None):
    """The collated batch of a shape: its graphs number GRAPH_IDS[name] (or `ids`)."""
    ids = GRAPH_IDS[name] if ids is None else ids
    return collate([graph(name, k) for k in ids], SHAPES[name][0])


# name -> (grids, graphs, seed, buses per graph)
GRID_BATCHES = {"cigre14": (["cigre14"], 5, 1, 15), "mixed": (["cigre14", "cigre14_reswitched"], 7, 13, 15), "ober_sub": (["ober_sub"], 3, 2, 70)}
ALL_BATCHES = list(GRID_BATCHES) + list(SHAPES)


def grid_batch(name):
    from conftest import load_pkg
    grids, B, seed, n = GRID_BATCHES[name]
    b = load_pkg().synthetic.make_batch(grids, B, seed=seed)
    b["nodes_per_graph"] = n
    return b


def any_batch(name):
    return grid_batch(name) if name in GRID_BATCHES else batch(name)
