"""fp64 oracle of the batched WLS state estimator (csrc/dss2_wls_solve.hip, estimator.wls_estimate): torch on the CPU, dense Jacobian,
LAPACK Cholesky.  It imports nothing from the product.

Measurement model (the reference's gsp_wls_edge, data.py:397-409): per bus z = (V, theta, P_inj, Q_inj) = x[:, 0:8:2] with weights
R^-1 = x[:, 1:8:2], per stored branch (P_from, Q_from) = edge_attr[:, 0:4:2] with weights edge_attr[:, 1:4:2]; every entry de-normalised
in fp64 from the fp32 input, double(z) * double(std) + double(mean), where the normalised entry is non-zero and 0 elsewhere; a
de-normalised weight below 0 counts as 0 (the reference would use it as it is).  h(u) = (v, theta, p_inj, q_inj) per bus and
(p_from, q_from) per branch (data.py:370-376, 428-435) with shift = 0 and V_lv the batch minimum of vn_kv = x[:, 8].  The state
u = (v, theta) is physical (p.u., rad), laid out (v_0, theta_0, v_1, theta_1, ...) per graph.

Per graph J(u) = sum_buses sum_k c_k R^-1 (Z - h)^2 + sum_branches sum_k w_pf R_edge^-1 (edge_Z - h_edge)^2, c = (w_v, w_v, w_p, w_p).
Gauss-Newton from `init` or from v = 1, theta = 0, slack angles (x[:, 9] != 0) held at 0:  G = H^T W H, b = H^T W r, the slack angles'
rows and columns replaced by the identity and their b by 0, Cholesky (a pivot <= 0 or not finite, or a step that is not finite: status 2,
the state stays), u += du, max |du| < tol: status 0; status 1 = max_iter reached.
"""
import torch

F64 = torch.float64


def denormalised(x, edge_attr, stats):
    """(Z [N, 4], R [N, 4], eZ [E, 2], eR [E, 2]) in fp64 from the fp32 (or fp64-held-fp32) inputs."""
    xm, xs, em, es = (s.detach().cpu().to(F64) for s in stats)
    x, ea = x.detach().cpu().to(F64), edge_attr.detach().cpu().to(F64)
    z, r = x[:, 0:8:2], x[:, 1:8:2]
    Z = (z * xs[0:8:2] + xm[0:8:2]) * (z != 0)
    R = (r * xs[1:8:2] + xm[1:8:2]) * (r != 0)
    ez, er = ea[:, 0:4:2], ea[:, 1:4:2]
    eZ = (ez * es[0:4:2] + em[0:4:2]) * (ez != 0)
    eR = (er * es[1:4:2] + em[1:4:2]) * (er != 0)
    return Z, R.clamp_min(0.0), eZ, eR.clamp_min(0.0)


def h_of(u, f, t, par, kk):
    """Measurement function of one graph: (h_bus [n, 4], h_edge [e, 2]).  u [2 n]; f, t [e] local from / to buses; par [e, 4] =
    G, B, Gs, Bs; kk = V_lv^2.  The branch equations are data.py:370-376 as written there."""
    v, th = u[0::2], u[1::2]
    n = v.shape[0]
    G, B, Gs, Bs = par[:, 0], par[:, 1], par[:, 2], par[:, 3]
    vi, vj, d = v[f], v[t], th[f] - th[t]
    c, s = torch.cos(d), torch.sin(d)
    pf = (-vi * vj * (G * c + B * s) + (G + Gs / 2) * vi ** 2) * kk
    qf = (vi * vj * (-G * s + B * c) - (B + Bs / 2) * vi ** 2) * kk
    pt = (-vi * vj * (G * c - B * s) + (G + Gs / 2) * vj ** 2) * kk
    qt = (vi * vj * (G * s + B * c) - (B + Bs / 2) * vj ** 2) * kk
    zero = torch.zeros(n, dtype=u.dtype)
    p_i = -zero.index_add(0, t, pt) - zero.index_add(0, f, pf)
    q_i = -zero.index_add(0, t, qt) - zero.index_add(0, f, qf)
    return torch.stack([v, th, p_i, q_i], 1), torch.stack([pf, qf], 1)


def h_flat(u, f, t, par, kk):
    """h as one vector: bus-major (V, theta, P, Q) rows, then (p_from, q_from) per branch -- the row order of `jacobian`."""
    hb, he = h_of(u, f, t, par, kk)
    return torch.cat([hb.reshape(-1), he.reshape(-1)])


def jacobian(u, f, t, par, kk):
    """Analytic dense Jacobian [4 n + 2 e, 2 n] of h_flat."""
    v, th = u[0::2], u[1::2]
    n, e = v.shape[0], f.shape[0]
    G, B, Gs, Bs = par[:, 0], par[:, 1], par[:, 2], par[:, 3]
    gg, bb = G + Gs / 2, B + Bs / 2
    vi, vj, d = v[f], v[t], th[f] - th[t]
    c, s = torch.cos(d), torch.sin(d)
    vv = vi * vj
    a1, a2, a3, a4 = G * c + B * s, -G * s + B * c, G * c - B * s, G * s + B * c
    # derivatives with respect to (v_i, theta_i, v_j, theta_j)
    dpf = [(-vj * a1 + 2 * gg * vi) * kk, -vv * a2 * kk, -vi * a1 * kk, vv * a2 * kk]
    dqf = [(vj * a2 - 2 * bb * vi) * kk, -vv * a1 * kk, vi * a2 * kk, vv * a1 * kk]
    dpt = [-vj * a3 * kk, vv * a4 * kk, (-vi * a3 + 2 * gg * vj) * kk, -vv * a4 * kk]
    dqt = [vj * a4 * kk, vv * a3 * kk, (vi * a4 - 2 * bb * vj) * kk, -vv * a3 * kk]
    H = torch.zeros(4 * n + 2 * e, 2 * n, dtype=u.dtype)
    idx = torch.arange(n)
    H[4 * idx, 2 * idx] = 1.0
    H[4 * idx + 1, 2 * idx + 1] = 1.0
    cols = [2 * f, 2 * f + 1, 2 * t, 2 * t + 1]
    k = torch.arange(e)
    for q in range(4):
        H.index_put_((4 * f + 2, cols[q]), -dpf[q], accumulate=True)
        H.index_put_((4 * t + 2, cols[q]), -dpt[q], accumulate=True)
        H.index_put_((4 * f + 3, cols[q]), -dqf[q], accumulate=True)
        H.index_put_((4 * t + 3, cols[q]), -dqt[q], accumulate=True)
        H.index_put_((4 * n + 2 * k, cols[q]), dpf[q], accumulate=True)
        H.index_put_((4 * n + 2 * k + 1, cols[q]), dqf[q], accumulate=True)
    return H


class Graph:
    """One graph's slice of a batch: local edges, parameters, measurements, weights."""

    def __init__(self, g, n, x, ei, ea, Z, R, eZ, eR, kk, weights):
        lo, hi = g * n, (g + 1) * n
        sel = torch.nonzero((ei[0] >= lo) & (ei[0] < hi)).flatten()
        assert bool(((ei[1, sel] >= lo) & (ei[1, sel] < hi)).all()), "an edge crosses graphs"
        self.edges = sel
        self.f, self.t = ei[0, sel] - lo, ei[1, sel] - lo
        self.par = ea[sel, 6:10].to(F64)
        self.kk, self.n = kk, n
        self.slack = x[lo:hi, 9] != 0
        w_v, w_p, w_pf = weights
        c = torch.tensor([w_v, w_v, w_p, w_p], dtype=F64)
        self.z = torch.cat([Z[lo:hi].reshape(-1), eZ[sel].reshape(-1)])
        self.w = torch.cat([(R[lo:hi] * c).reshape(-1), (eR[sel] * w_pf).reshape(-1)])
        self.n_bus_rows = 4 * n

    def objective(self, u):
        r = self.z - h_flat(u, self.f, self.t, self.par, self.kk)
        j = self.w * r * r
        return j[:self.n_bus_rows].sum(), j[self.n_bus_rows:].sum()

    def normal_equations(self, u, perm=None):
        H = jacobian(u, self.f, self.t, self.par, self.kk)
        r = self.z - h_flat(u, self.f, self.t, self.par, self.kk)
        w = self.w
        if perm is not None:
            H, r, w = H[perm], r[perm], w[perm]
        Gm = (H * w[:, None]).t() @ H
        b = H.t() @ (w * r)
        s = 2 * torch.nonzero(self.slack).flatten() + 1
        Gm[s, :] = 0.0
        Gm[:, s] = 0.0
        Gm[s, s] = 1.0
        b[s] = 0.0
        return Gm, b


def graphs_of(x, edge_index, edge_attr, stats, nodes_per_graph, weights=(1.0, 1.0, 1.0)):
    x64, ea64 = x.detach().cpu().to(F64), edge_attr.detach().cpu().to(F64)
    ei = edge_index.detach().cpu()
    N, n = x64.shape[0], nodes_per_graph
    assert N % n == 0
    Z, R, eZ, eR = denormalised(x64, ea64, stats)
    kk = x64[:, 8].min() ** 2
    return [Graph(g, n, x64, ei, ea64, Z, R, eZ, eR, kk, weights) for g in range(N // n)]


def solve(x, edge_index, edge_attr, stats, nodes_per_graph, init=None, max_iter=10, tol=1e-6, weights=(1.0, 1.0, 1.0), perm_seed=None,
          graphs=None):
    """The estimator of the module docstring.  Returns a dict: state [N, 2] fp64, objective [G, 2], iterations [G], status [G],
    last_step [G], and steps: per graph the list of max |du| of every factorised iteration (the applied ones).  perm_seed: the measurements
    enter the normal equations in a random order (a different summation order, same mathematics).  graphs: the list `graphs_of` built,
    with measurements a test has replaced (the noise-free known answer)."""
    gs = graphs if graphs is not None else graphs_of(x, edge_index, edge_attr, stats, nodes_per_graph, weights)
    n, B = nodes_per_graph, len(gs)
    state = torch.zeros(B * n, 2, dtype=F64)
    objective = torch.zeros(B, 2, dtype=F64)
    iterations = torch.zeros(B, dtype=torch.int32)
    status = torch.zeros(B, dtype=torch.int32)
    last_step = torch.zeros(B, dtype=F64)
    steps = []
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
        for _ in range(max_iter):
            perm = torch.randperm(gr.z.shape[0], generator=gen) if gen is not None else None
            Gm, b = gr.normal_equations(u, perm)
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
        state[g * n:(g + 1) * n, 0], state[g * n:(g + 1) * n, 1] = u[0::2], u[1::2]
        jb, je = gr.objective(u)
        objective[g, 0], objective[g, 1] = jb, je
        iterations[g], status[g], last_step[g] = its, st, last
        steps.append(hist)
    return dict(state=state, objective=objective, iterations=iterations, status=status, last_step=last_step, steps=steps)


def undecided(res, tol, factor=4.0):
    """Graphs whose deciding step -- the last one the oracle took -- lies within `factor` of tol: another fp64 implementation may decide
    the other way there.  [G] bool."""
    out = []
    for hist in res["steps"]:
        out.append(bool(hist) and tol > 0 and tol / factor <= hist[-1] <= tol * factor)
    return torch.tensor(out)
