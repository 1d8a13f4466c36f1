"""fp64 oracle of estimator.wls_bad_data (csrc/dss2_wls_bad_data.hip): the solve of tests/wls_oracle.py, then residual sensitivities,
normalized residuals, the chi-square test and the removal of the largest normalized residual, with re-solves from the current state.
It imports torch and wls_oracle only.

Sensitivities come from a QR of sqrt(W) H (slack-angle columns dropped): S_i = 1 - |Q_i|^2, the leverage form -- deliberately NOT the
kernel's route, which inverts the gain matrix.  state_std = row norms of R^-1 of the same QR.  `sens_normal` is the second fp64 route
(normal equations, cholesky_inverse) that tests/test_wls_bad_data_cpu.py compares the first with.

A measurement is active if its weight c_k R^-1 is above 0 and it has not been removed.  rN_i = |z_i - h_i(u)| sqrt(w_i / S_i) where
S_i >= s_min, 0 below.  The largest rN (ties: the smallest id) is removed if it exceeds `threshold` and fewer than max_removals are gone.
Ids: 4 i + k for bus i (global row), 4 N + 2 e + k for stored branch e.
"""
import torch

import wls_oracle as wo

F64 = torch.float64


def _free_columns(gr):
    keep = torch.ones(2 * gr.n, dtype=torch.bool)
    keep[2 * torch.nonzero(gr.slack).flatten() + 1] = False
    return keep


def sens_qr(gr, u):
    """(S [m] with 0 where inactive, state_std [2 n] with 0 at slack angles) of graph gr at state u with its current weights."""
    keep = _free_columns(gr)
    H = wo.jacobian(u, gr.f, gr.t, gr.par, gr.kk)[:, keep]
    Q, R = torch.linalg.qr(gr.w.sqrt()[:, None] * H)
    S = (1.0 - (Q * Q).sum(1)) * (gr.w > 0)
    Rinv = torch.linalg.solve_triangular(R, torch.eye(R.shape[0], dtype=F64), upper=True)
    std = torch.zeros(2 * gr.n, dtype=F64)
    std[keep] = (Rinv * Rinv).sum(1).sqrt()
    return S, std


def sens_normal(gr, u, perm=None):
    """The same two from the normal equations: Sigma = (H^T W H)^-1 by Cholesky, S_i = 1 - w_i h_i Sigma h_i^T.  perm: the order in which
    the measurements enter G."""
    keep = _free_columns(gr)
    Gm, _ = gr.normal_equations(u, perm)
    Sigma = torch.cholesky_inverse(torch.linalg.cholesky(Gm))
    H = wo.jacobian(u, gr.f, gr.t, gr.par, gr.kk) * keep
    S = (1.0 - gr.w * ((H @ Sigma) * H).sum(1)) * (gr.w > 0)
    return S, Sigma.diagonal().sqrt() * keep


def normalized_residuals(gr, u, S, s_min):
    r = gr.z - wo.h_flat(u, gr.f, gr.t, gr.par, gr.kk)
    ok = (gr.w > 0) & (S >= s_min)
    return torch.where(ok, r.abs() * (gr.w / S.clamp_min(s_min)).sqrt(), torch.zeros_like(r))


def chi2_limit(dof, z_p):
    if dof <= 0:
        return float("inf")
    c = 2.0 / (9.0 * dof)
    return dof * (1.0 - c + z_p * c ** 0.5) ** 3


def global_id(gr, g, N, m):
    """Local measurement row m of graph number g -> the id of the module docstring."""
    if m < gr.n_bus_rows:
        return 4 * g * gr.n + m
    j, k = divmod(m - gr.n_bus_rows, 2)
    return 4 * N + 2 * int(gr.edges[j]) + k


def bad_data(x, edge_index, edge_attr, stats, nodes_per_graph, init=None, max_iter=10, tol=1e-6, weights=(1.0, 1.0, 1.0), threshold=3.0,
             max_removals=0, confidence=0.95, s_min=1e-3, perm_seed=None, sens=sens_qr):
    """The estimator of the module docstring.  Returns a dict with the fields of WLSBadDataResult (state fp64) plus
    decisions: per graph a list of (winner id, winner rN, runner-up rN), one per arg-max taken (the last one is the decision to stop)."""
    gs = wo.graphs_of(x, edge_index, edge_attr, stats, nodes_per_graph, weights)
    n, B, N, E = nodes_per_graph, len(gs), x.shape[0], edge_attr.shape[0]
    slots = max(max_removals, 1)
    z_p = float(torch.special.ndtri(torch.tensor(float(confidence), dtype=F64)))
    out = dict(state=torch.zeros(N, 2, dtype=F64), objective=torch.zeros(B, 2, dtype=F64), iterations=torch.zeros(B, dtype=torch.int32),
               status=torch.zeros(B, dtype=torch.int32), last_step=torch.zeros(B, dtype=F64), dof=torch.zeros(B, dtype=torch.int32),
               chi2_limit=torch.zeros(B, dtype=F64), suspect=torch.zeros(B, dtype=torch.int32),
               removed=torch.full((B, slots), -1, dtype=torch.int32), removed_rn=torch.zeros(B, slots, dtype=F64),
               n_removed=torch.zeros(B, dtype=torch.int32), bus_rn=torch.zeros(N, 4, dtype=F64), edge_rn=torch.zeros(E, 2, dtype=F64),
               bus_sens=torch.zeros(N, 4, dtype=F64), edge_sens=torch.zeros(E, 2, dtype=F64), state_std=torch.zeros(N, 2, dtype=F64),
               decisions=[])
    for g, gr in enumerate(gs):
        cur = None if init is None else init.detach().cpu().to(F64)[g * n:(g + 1) * n]
        its, last, nrem, decisions = 0, 0.0, 0, []
        S = rn = std = None
        for _ in range(max_removals + 1):
            res = wo.solve(None, None, None, None, n, init=cur, max_iter=max_iter, tol=tol, perm_seed=perm_seed, graphs=[gr])
            cur, status = res["state"], int(res["status"][0])
            its += int(res["iterations"][0])
            if int(res["iterations"][0]) > 0:
                last = float(res["last_step"][0])
            if status == 2:
                S = rn = std = None
                break
            u = cur.reshape(-1)
            S, std = sens(gr, u)
            rn = normalized_residuals(gr, u, S, s_min)
            best = rn.max()
            m = int(torch.nonzero(rn == best).flatten()[0])
            runner_up = torch.cat([rn[:m], rn[m + 1:]]).max() if rn.numel() > 1 else torch.tensor(0.0)
            decisions.append((global_id(gr, g, N, m), float(best), float(runner_up)))
            if not (float(best) > threshold and nrem < max_removals):
                break
            out["removed"][g, nrem], out["removed_rn"][g, nrem] = global_id(gr, g, N, m), best
            nrem += 1
            gr.w = gr.w.clone()
            gr.w[m] = 0.0
        rows = slice(g * n, (g + 1) * n)
        out["state"][rows] = cur
        jb, je = gr.objective(cur.reshape(-1))
        out["objective"][g, 0], out["objective"][g, 1] = jb, je
        out["iterations"][g], out["status"][g], out["last_step"][g], out["n_removed"][g] = its, status, last, nrem
        dof = int((gr.w > 0).sum()) - int(_free_columns(gr).sum())
        out["dof"][g], out["chi2_limit"][g] = dof, chi2_limit(dof, z_p)
        out["suspect"][g] = int(float(jb + je) > chi2_limit(dof, z_p))
        if S is not None:
            out["bus_sens"][rows], out["bus_rn"][rows] = S[:4 * n].reshape(n, 4), rn[:4 * n].reshape(n, 4)
            out["edge_sens"][gr.edges], out["edge_rn"][gr.edges] = S[4 * n:].reshape(-1, 2), rn[4 * n:].reshape(-1, 2)
            out["state_std"][rows] = std.reshape(n, 2)
        out["decisions"].append(decisions)
    return out


def largest_sensitivity_targets(x, edge_index, edge_attr, stats, nodes_per_graph, rank=0, max_iter=10):
    """Per graph the id of the active measurement with the (rank + 1)-th largest S among those whose Jacobian row (slack-angle columns
    dropped) is not zero, at the solution of the data as they are (flat start, max_iter iterations, tol = 0).  A slack bus's theta
    reading has S = 1 exactly and is decoupled from the state: it is no target."""
    gs = wo.graphs_of(x, edge_index, edge_attr, stats, nodes_per_graph)
    res = wo.solve(x, edge_index, edge_attr, stats, nodes_per_graph, max_iter=max_iter, tol=0.0, graphs=gs)
    n, N, ids = nodes_per_graph, x.shape[0], []
    for g, gr in enumerate(gs):
        u = res["state"][g * n:(g + 1) * n].reshape(-1)
        S, _ = sens_qr(gr, u)
        H = wo.jacobian(u, gr.f, gr.t, gr.par, gr.kk)[:, _free_columns(gr)]
        S = torch.where((gr.w > 0) & (H.abs().sum(1) > 0), S, torch.full_like(S, -1.0))
        ids.append(global_id(gr, g, N, int(torch.argsort(S, descending=True, stable=True)[rank])))
    return ids


def add_gross_errors(x, edge_attr, stats, ids, sigmas=25.0):
    """Copies of x and edge_attr (fp32) with +sigmas / sqrt(w) added, in physical units, to the measurements `ids`."""
    xm, xs, em, es = (s.detach().cpu().to(F64) for s in stats)
    x2, ea2 = x.detach().cpu().clone(), edge_attr.detach().cpu().clone()
    N = x.shape[0]
    for mid in ids:
        t, mean, std, (row, k) = (x2, xm, xs, divmod(mid, 4)) if mid < 4 * N else (ea2, em, es, divmod(mid - 4 * N, 2))
        w = float(t[row, 2 * k + 1]) * float(std[2 * k + 1]) + float(mean[2 * k + 1])
        assert float(t[row, 2 * k + 1]) != 0.0 and w > 0.0, "not an active measurement"
        z = float(t[row, 2 * k]) * float(std[2 * k]) + float(mean[2 * k]) + sigmas / w ** 0.5
        t[row, 2 * k] = (z - float(mean[2 * k])) / float(std[2 * k])
        assert float(t[row, 2 * k]) != 0.0
    return x2, ea2
