"""fp64 oracle of estimator.wls_robust (csrc/dss2_wls_robust.hip): the Huber M-estimator on the measurement model of tests/wls_oracle.py,
solved by iteratively re-weighted Gauss-Newton.  torch on the CPU, dense Jacobian, LAPACK Cholesky; it imports nothing from the product.

Measurement i has the weight w_i = c_k R_i^-1 of wls_oracle.Graph, the residual r_i = z_i - h_i(u) and t_i = sqrt(w_i) |r_i| at the
current iterate.  Its factor q_i is gamma / t_i where weighting is on (iteration number >= plain_iters) and t_i > gamma, else 1 (so a
NaN keeps 1, and so does a weight of 0).  An iteration is wls_oracle.solve's with w_i q_i in place of w_i in G and b; H, r and q come
from the same iterate.  Start, slack handling, failure, decision and statuses are solve's.  At the final state, with weighting on:
q per measurement, the count of q < 1 per graph and the Huber cost sum_i rho(t_i), rho = t^2 (= w r^2, solve's term) where
not t > gamma and 2 gamma t - gamma^2 above, split into bus part and branch part like solve's objective.

`corrupted(name)`: the batch of a case with one gross error of +25 sigma per graph on the measurement of largest residual sensitivity
(wls_bad_data_oracle.largest_sensitivity_targets, add_gross_errors); the three FAILING cases of wls_edge_cases go through as they are.
"""
import functools

import torch

import wls_bad_data_oracle as bo
import wls_edge_cases as ec
import wls_large_cases as lc
import wls_oracle as wo
from wls_oracle import Graph, h_flat, jacobian          # noqa: F401  (the pieces this oracle is built from)

F64 = torch.float64
GAMMA, SIGMAS = 3.0, 25.0


def scaled_residuals(gr, u):
    """(r, t) of graph gr at state u: r = z - h(u), t = sqrt(w) |r|."""
    r = gr.z - h_flat(u, gr.f, gr.t, gr.par, gr.kk)
    return r, gr.w.sqrt() * r.abs()


def factors(t, gamma):
    return torch.where(t > gamma, gamma / t, torch.ones_like(t))


def huber_cost(gr, u, gamma):
    """(bus part, branch part, q, t) at state u with weighting on."""
    r, t = scaled_residuals(gr, u)
    j = torch.where(t > gamma, 2.0 * gamma * t - gamma * gamma, gr.w * r * r)
    return j[:gr.n_bus_rows].sum(), j[gr.n_bus_rows:].sum(), factors(t, gamma), t


def solve_huber(x, edge_index, edge_attr, stats, nodes_per_graph, init=None, max_iter=20, tol=1e-6, weights=(1.0, 1.0, 1.0), perm_seed=None,
                graphs=None, gamma=GAMMA, plain_iters=1):
    """The estimator of the module docstring.  Returns wls_oracle.solve's dict (state [N, 2] fp64, objective [G, 2] = the Huber cost,
    iterations, status, last_step, steps) plus gamma, plain_iters, perm_seed, bus_q [N, 4], edge_q [E, 2] (1 for an edge of no graph),
    n_downweighted [G] int32 and t: per graph the [4 n + 2 e] scaled residuals at the final state (bus-major, then the graph's branches)."""
    gs = graphs if graphs is not None else wo.graphs_of(x, edge_index, edge_attr, stats, nodes_per_graph, weights)
    n, B = nodes_per_graph, len(gs)
    E = max([int(gr.edges.max()) + 1 for gr in gs if gr.edges.numel()] + [0]) if edge_attr is None else edge_attr.shape[0]
    out = dict(state=torch.zeros(B * n, 2, dtype=F64), objective=torch.zeros(B, 2, dtype=F64), iterations=torch.zeros(B, dtype=torch.int32),
               status=torch.zeros(B, dtype=torch.int32), last_step=torch.zeros(B, dtype=F64), steps=[], gamma=gamma, plain_iters=plain_iters,
               perm_seed=perm_seed, bus_q=torch.ones(B * n, 4, dtype=F64), edge_q=torch.ones(E, 2, dtype=F64),
               n_downweighted=torch.zeros(B, dtype=torch.int32), t=[])
    gen = torch.Generator().manual_seed(perm_seed) if perm_seed is not None else None
    for g, gr in enumerate(gs):
        u = torch.zeros(2 * n, dtype=F64)
        if init is None:
            u[0::2] = 1.0
        else:
            i0 = init.detach().cpu().to(F64)[g * n:(g + 1) * n]
            u[0::2], u[1::2] = i0[:, 0], i0[:, 1]
        u[1::2] = torch.where(gr.slack, torch.zeros(n, dtype=F64), u[1::2])
        st, its, last, hist = 1, 0, 0.0, []
        w_full = gr.w
        for it in range(max_iter):
            perm = torch.randperm(gr.z.shape[0], generator=gen) if gen is not None else None
            if it >= plain_iters:
                gr.w = w_full * factors(scaled_residuals(gr, u)[1], gamma)
            try:
                Gm, b = gr.normal_equations(u, perm)
            finally:
                gr.w = w_full
            if not bool(torch.isfinite(Gm).all()):
                st = 2
                break
            L, info = torch.linalg.cholesky_ex(Gm)
            if int(info) != 0 or not bool(torch.isfinite(L).all()):
                st = 2
                break
            du = torch.cholesky_solve(b[:, None], L)[:, 0]
            if not bool(torch.isfinite(du).all()):
                st = 2
                break
            u = u + du
            its += 1
            last = float(du.abs().max())
            hist.append(last)
            if last < tol:
                st = 0
                break
        rows = slice(g * n, (g + 1) * n)
        out["state"][rows, 0], out["state"][rows, 1] = u[0::2], u[1::2]
        jb, je, q, t = huber_cost(gr, u, gamma)
        out["objective"][g, 0], out["objective"][g, 1] = jb, je
        out["iterations"][g], out["status"][g], out["last_step"][g] = its, st, last
        out["bus_q"][rows] = q[:4 * n].reshape(n, 4)
        out["edge_q"][gr.edges] = q[4 * n:].reshape(-1, 2)
        out["n_downweighted"][g] = int((q < 1.0).sum())
        out["steps"].append(hist)
        out["t"].append(t)
    return out


def near_threshold(ref, gamma=GAMMA, rel=1e-6):
    """Per graph the number of measurements whose t lies within rel * gamma of gamma: another fp64 implementation may put them on the
    other side."""
    return [int(((t - gamma).abs() <= rel * gamma).sum()) for t in ref["t"]]


def downweighted_ids(ref):
    """The measurement ids (4 i + k per bus, 4 N + 2 e + k per stored branch) with q < 1, ascending."""
    N = ref["bus_q"].shape[0]
    bus = torch.nonzero(ref["bus_q"].reshape(-1) < 1.0).flatten()
    edge = torch.nonzero(ref["edge_q"].reshape(-1) < 1.0).flatten() + 4 * N
    return torch.cat([bus, edge]).tolist()


@functools.lru_cache(maxsize=None)
def corrupted(name):
    """(host batch, ids): the batch of a case of wls_cases, wls_edge_cases or wls_large_cases with +25 sigma on one measurement per graph;
    a FAILING case comes back as it is, with no ids."""
    b = ec.batch(name) if name in ec.CASES else lc.batch(name)
    if name in ec.FAILING:
        return b, []
    ids = bo.largest_sensitivity_targets(*ec.args(b))
    x2, ea2 = bo.add_gross_errors(b["x"], b["edge_attr"], b["stats"], ids, SIGMAS)
    return dict(b, x=x2, edge_attr=ea2), ids


@functools.lru_cache(maxsize=None)
def oracle(name, max_iter, tol, plain_iters=1, perm_seed=None, gamma=GAMMA, clean=False):
    """solve_huber on corrupted(name) (clean: on the case's batch as it is): computed once, shared, never modified."""
    b = (ec.batch(name) if name in ec.CASES else lc.batch(name)) if clean else corrupted(name)[0]
    return solve_huber(*ec.args(b), max_iter=max_iter, tol=tol, plain_iters=plain_iters, perm_seed=perm_seed, gamma=gamma)
