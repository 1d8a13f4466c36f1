"""The classical weighted-least-squares state estimator on the measurement model of ``gsp_wls_edge``: the baseline a learned
estimator is compared with, and the polish after it (a few Gauss-Newton steps from the model's output).

    wls_estimate(x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, nodes_per_graph,
                 init=None, max_iter=10, tol=1e-6, weights=(1.0, 1.0, 1.0)) -> WLSResult

Inputs are those of ``data.eval_batch`` -- the full node tensor [N, 11], the full edge tensor [E, 13], the four statistics -- plus the
bus count of a graph: graph g owns rows [g n, (g + 1) n), edges never cross graphs, per-graph edge counts may differ.  The state is
physical, (v in p.u., theta in rad), the convention of ``eval_batch``'s ``yhat``.  Everything inside is fp64 (the gain matrix of these
grids has condition number 3e11 .. 3e12: an fp32 Cholesky meets non-positive pivots at the first iteration); one HIP
launch per solve, csrc/dss2_wls_solve.hip.  No CPU fallback, no host read-back, recordable into a hipGraph or a launch plan.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence

import torch

from . import _lib
from .data import _vec
from .networks import _F32, _require_gpu, _rows, _stream
from .topology import get_topology

_LDS_CAP = 160 * 1024
STATUS_CONVERGED, STATUS_MAX_ITER, STATUS_FAILED = 0, 1, 2


class WLSResult(NamedTuple):
    state: torch.Tensor          # [N, 2] fp32: v (p.u.), theta (rad)
    objective: torch.Tensor      # [G, 2] fp64: bus part and branch part of J at the final fp64 state
    iterations: torch.Tensor     # [G] int32: updates applied
    status: torch.Tensor         # [G] int32: 0 converged (max |du| < tol), 1 max_iter reached, 2 factorisation failed (state of the previous iterate)
    last_step: torch.Tensor      # [G] fp64: max |du| of the last update applied


_MAX_NODES = []


def max_nodes_per_graph() -> int:
    """The largest bus count of a graph whose gain matrix, right-hand side and state fit into the LDS of a CU."""
    if not _MAX_NODES:
        L = _lib.lib()
        n = 1
        while L.dss2_wls_solve_lds_bytes(n + 1) <= _LDS_CAP:
            n += 1
        _MAX_NODES.append(n)
    return _MAX_NODES[0]


def wls_estimate(x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, nodes_per_graph: int,
                 init: Optional[torch.Tensor] = None, max_iter: int = 10, tol: float = 1e-6,
                 weights: Sequence[float] = (1.0, 1.0, 1.0), max_groups: int = 0) -> WLSResult:
    """Gauss-Newton on J_g(u) = sum_buses sum_k c_k R^-1 (Z - h)^2 + sum_branches sum_k w_pf R_edge^-1 (edge_Z - h_edge)^2 per graph,
    c = (w_v, w_v, w_p, w_p), ``weights`` = (w_v, w_p, w_pf): (1, 1, 1) is the classical WLS, (lam_v, lam_p, lam_pf) the training
    loss's relative weighting.  Start: ``init`` [N, 2] (physical), or flat (v = 1, theta = 0); theta at slack buses is 0 and stays 0.
    ``tol = 0`` never stops early.  ``max_groups`` > 0 caps the number of workgroups (they stride over the graphs)."""
    _require_gpu(x, edge_index, edge_attr)
    n = int(nodes_per_graph)
    N = x.size(0)
    if n < 1 or N == 0 or N % n != 0:
        raise ValueError(f"x has {N} rows: not a positive multiple of nodes_per_graph = {nodes_per_graph}")
    if int(max_iter) < 1:
        raise ValueError("max_iter must be at least 1")
    if not tol >= 0:
        raise ValueError("tol must be >= 0")
    if len(weights) != 3:
        raise ValueError("weights = (w_v, w_p, w_pf)")
    if x.dim() != 2 or x.size(1) < 10 or edge_attr.dim() != 2 or edge_attr.size(1) < 10:
        raise ValueError("x must be the full [N, 11] node tensor and edge_attr the full [E, 13] edge tensor")
    if init is not None:
        _require_gpu(init)
        if init.dim() != 2 or tuple(init.shape) != (N, 2):
            raise ValueError(f"init must be [N, 2] = ({N}, 2), got {tuple(init.shape)}")
    if n > max_nodes_per_graph():
        raise NotImplementedError(f"wls_estimate keeps a graph's gain matrix in LDS: at most {max_nodes_per_graph()} buses per graph, "
                                  f"got {n}")
    dev = x.device
    x2, ldx = _rows(x)
    ea2, ldea = _rows(edge_attr)
    topo = get_topology(edge_index, N)
    G = N // n
    a = _lib.WlsSolveArgs()
    a.x, a.ldx, a.edge_attr, a.ldea = x2.data_ptr(), ldx, ea2.data_ptr(), ldea
    stats = (_vec(x_mean, 8, dev), _vec(x_std, 8, dev), _vec(edge_mean, 4, dev), _vec(edge_std, 4, dev))
    a.x_mean, a.x_std, a.edge_mean, a.edge_std = (s.data_ptr() for s in stats)
    a.efrom, a.eto, a.inc_rowptr, a.inc_ent = (t.data_ptr() for t in (topo.efrom, topo.eto, topo.inc_rowptr, topo.inc_ent))
    a.n_nodes, a.n_edges, a.nodes_per_graph, a.max_iter, a.tol = N, topo.E, n, int(max_iter), float(tol)
    a.w_v, a.w_p, a.w_pf = (float(w) for w in weights)
    keep = None
    if init is not None:
        keep, ld_init = _rows(init.detach())
        a.init, a.ld_init = keep.data_ptr(), ld_init
    res = WLSResult(torch.empty(N, 2, dtype=_F32, device=dev), torch.empty(G, 2, dtype=torch.float64, device=dev),
                    torch.empty(G, dtype=torch.int32, device=dev), torch.empty(G, dtype=torch.int32, device=dev),
                    torch.empty(G, dtype=torch.float64, device=dev))
    a.state, a.objective, a.iterations, a.status, a.last_step = (t.data_ptr() for t in res)
    vmm = torch.empty(130, dtype=_F32, device=dev)
    a.vminmax, a.max_groups = vmm.data_ptr(), int(max_groups)
    _lib.check(_lib.lib().dss2_wls_solve(C.byref(a), _stream(x)), "dss2_wls_solve")
    return res
