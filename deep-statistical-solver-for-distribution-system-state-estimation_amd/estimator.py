"""The classical weighted-least-squares state estimator on the measurement model of ``gsp_wls_edge``: the baseline a learned
estimator is compared with, and the polish after it (a few Gauss-Newton steps from the model's output).

    wls_estimate(x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, nodes_per_graph,
                 init=None, max_iter=10, tol=1e-6, weights=(1.0, 1.0, 1.0)) -> WLSResult

Inputs are those of ``data.eval_batch`` -- the full node tensor [N, 11], the full edge tensor [E, 13], the four statistics -- plus the
bus count of a graph: graph g owns rows [g n, (g + 1) n), edges never cross graphs, per-graph edge counts may differ.  The state is
physical, (v in p.u., theta in rad), the convention of ``eval_batch``'s ``yhat``.  Everything inside is fp64 (the gain matrix of these
grids has condition number 3e11 .. 3e12: an fp32 Cholesky meets non-positive pivots at the first iteration); one HIP
launch per solve, csrc/dss2_wls_solve.hip.  No CPU fallback, no host read-back, recordable into a hipGraph or a launch plan.
It keeps the gain matrix in LDS and serves up to ``max_nodes_per_graph()`` = 99 buses per graph.

    wls_estimate_large(... same arguments ...) -> WLSResult

The same estimator for up to ``max_nodes_per_graph_large()`` = 256 buses per graph (ober179): the gain matrix in a workspace in global
memory, a blocked Cholesky, csrc/dss2_wls_large.hip.

    band_order(edge_index, nodes_per_graph, half_bandwidth=None, num_nodes=None, identity=False) -> BandOrder
    wls_estimate_banded(... same arguments ..., order=None) -> WLSResult

The same estimator beyond 256 buses per graph (feeders of 300, 1000 buses): the buses are numbered for a small bandwidth of the gain
matrix on the host, once per structure (``band_order``: Cuthill-McKee), and the blocked kernel runs on the band alone,
csrc/dss2_wls_banded.hpp.  ``num_nodes`` counts buses behind the last branch (one-bus graphs at the end of a batch); ``identity`` keeps the
caller's numbering and only measures its half-bandwidth.  Equal-size graphs; no ``graph_ptr``.

    wls_bad_data_banded(... wls_bad_data_large's arguments ..., order=None) -> WLSBadDataResult
    wls_robust_banded(... wls_robust's arguments without ``large`` ..., order=None) -> WLSRobustResult

The two answers to gross errors (below) on the banded kernel, beyond 256 buses.  The bad-data test reads the covariance only at its
diagonal and between buses within two branches of each other; those entries of the inverse lie inside the band and follow from the banded
factor by the selected-inverse recurrence, in place (csrc/dss2_wls_banded_invert.hpp) -- no dense inverse.  Results come back in the
caller's bus order, ``removed`` in the caller's ids.

    wls_bad_data(... same inputs ..., threshold=3.0, max_removals=0, confidence=0.95, s_min=1e-3) -> WLSBadDataResult

The rest of the classical estimator on the same solve and in the same single launch (csrc/dss2_wls_bad_data.hip): the chi-square test
on J, residual sensitivities and normalized residuals, removal of the largest one followed by a re-solve, the state's standard deviation.
It inverts the gain matrix in LDS: up to 99 buses per graph.

    wls_bad_data_large(... same arguments ...) -> WLSBadDataResult

The same test for up to ``max_nodes_per_graph_large()`` = 256 buses per graph (ober179), small graphs included: the blocked kernels of
``wls_estimate_large``, the gain matrix inverted in place on its block rows in the workspace.  Opt-in: ``wls_bad_data`` keeps its limit.

    wls_robust(... same inputs ..., gamma=3.0, plain_iters=1, large=None) -> WLSRobustResult

The second classical answer to gross errors, for every bus count up to 256: the Huber M-estimator by iteratively re-weighted
Gauss-Newton on the kernels of ``wls_estimate`` and ``wls_estimate_large`` (csrc/dss2_wls_robust.hip).  No covariance, one launch.

Batches that mix bus counts: the five dense functions take the keyword ``graph_ptr`` (``_public`` at the end of the module adds it: the parameter lists
above are pinned by callers and tests, and ``inspect.signature`` goes on reporting them), a contiguous int64 device tensor [G + 1] of row offsets (what
``synthetic.make_batch`` returns for a list of grids and ``dataset.MixedDataset`` puts on its batches).  Graph g then owns rows
[graph_ptr[g], graph_ptr[g + 1]) and ``nodes_per_graph`` is an UPPER BOUND on a graph's bus count, known on the host: the kernel choice,
LDS, workspace and every size refusal go by it, N need not be a multiple of it, and outputs per graph are [G, ...].  Nothing is read back:
the kernel checks every graph against the bound and against [0, N), and a graph that fails the check ends with status 2, 0 iterations,
objective 0 and no row written (its rows of ``state`` and of the per-measurement outputs keep the value they were allocated with: 0, and
1 for the q factors), while the others are solved.  Measurement ids stay global (4 i + k for row i of x, 4 N + 2 e + k for stored branch
e), and V_lv is the minimum of vn_kv over the WHOLE batch, as the training loss has it.
"""
from __future__ import annotations

import ctypes as C
import functools
import inspect
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


_EDGELESS = {}                   # (device, N) -> the all-zero incidence row pointer of a batch without branches


def _incidence(edge_index: torch.Tensor, N: int):
    """((efrom, eto, inc_rowptr, inc_ent) as device addresses, the stored edge count).  A batch without any branch (one-bus graphs) has
    no Topology: every bus's incidence range is empty, and the kernels touch no edge array then.  Like a Topology, the row pointer is
    kept (a recorded launch replays with its address)."""
    if edge_index.dim() == 2 and edge_index.size(0) == 2 and edge_index.size(1) == 0:
        key = (edge_index.device, N)
        if key not in _EDGELESS:
            _EDGELESS[key] = torch.zeros(N + 1, dtype=torch.int32, device=edge_index.device)
        return (None, None, _EDGELESS[key].data_ptr(), None), 0
    topo = get_topology(edge_index, N)
    return tuple(t.data_ptr() for t in (topo.efrom, topo.eto, topo.inc_rowptr, topo.inc_ent)), topo.E


def _wls_estimate(x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, nodes_per_graph: int,
                 init: Optional[torch.Tensor] = None, max_iter: int = 10, tol: float = 1e-6,
                 weights: Sequence[float] = (1.0, 1.0, 1.0), max_groups: int = 0,
                 graph_ptr: Optional[torch.Tensor] = None) -> WLSResult:
    """Gauss-Newton on J_g(u) = sum_buses sum_k c_k R^-1 (Z - h)^2 + sum_branches sum_k w_pf R_edge^-1 (edge_Z - h_edge)^2 per graph,
    c = (w_v, w_v, w_p, w_p), ``weights`` = (w_v, w_p, w_pf): (1, 1, 1) is the classical WLS, (lam_v, lam_p, lam_pf) the training
    loss's relative weighting.  Start: ``init`` [N, 2] (physical), or flat (v = 1, theta = 0); theta at slack buses is 0 and stays 0.
    ``tol = 0`` never stops early.  ``max_groups`` > 0 caps the number of workgroups (they stride over the graphs).
    ``graph_ptr`` [G + 1] (int64, device): the batch mixes bus counts, graph g owns rows [graph_ptr[g], graph_ptr[g + 1]) and
    ``nodes_per_graph`` is an upper bound on a graph's bus count (the module docstring: the bound, the ids, V_lv)."""
    return _solve(None, _LDS, x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, nodes_per_graph, init, max_iter, tol, weights,
                  max_groups, graph_ptr=graph_ptr)


def max_nodes_per_graph_large() -> int:
    """The largest bus count of a graph ``wls_estimate_large`` serves."""
    return int(_lib.lib().dss2_wls_large_max_nodes())


_WORKSPACES = {}                 # (device, bytes) -> the gain matrices' workspace of wls_estimate_large, kept (a recorded launch replays
                                 # with its address); calls on one stream run one after the other, and no call needs its contents


def _wls_estimate_large(x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, nodes_per_graph: int,
                       init: Optional[torch.Tensor] = None, max_iter: int = 10, tol: float = 1e-6,
                       weights: Sequence[float] = (1.0, 1.0, 1.0), max_groups: int = 0,
                       graph_ptr: Optional[torch.Tensor] = None) -> WLSResult:
    """``wls_estimate`` -- the same inputs, iteration, result and decisions -- for graphs of up to ``max_nodes_per_graph_large()``
    buses, small ones included: the gain matrix lives in a workspace in global memory (one slice per workgroup, allocated once per
    device and size) and is factorised in blocks, csrc/dss2_wls_large.hip.  Still one launch per solve, recordable.
    ``graph_ptr`` as for ``wls_estimate``: with it ``nodes_per_graph`` is an upper bound, and the workspace is sized by the bound."""
    return _solve(None, _BLOCKED, x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, nodes_per_graph, init, max_iter, tol, weights,
                  max_groups, graph_ptr=graph_ptr)


def _solve_block(a, x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, nodes_per_graph, init, max_iter, tol, weights,
                 max_groups, refuse_size, check_own=None, graph_ptr=None):
    """Validates the arguments every estimator here shares and fills ``a``, the ``WlsSolveArgs`` of its launch -- outputs included.
    The caller's own checks run at their place among these: ``check_own()`` (its ValueErrors) after the scalars', ``refuse_size(n)``
    (its NotImplementedError) after every ValueError.  Returns (keep, out, N, E, G): ``keep`` is what ``a`` points into and nothing
    else holds -- the row views, the statistics vectors, the kept ``init``, the vminmax buffer -- to be held until the launch has been
    issued; ``out`` is the WLSResult of fresh tensors that ``a`` writes.  With a ``graph_ptr`` n is the bound, G its length less one,
    and ``state`` is zero-filled (a graph the kernel refuses writes no row)."""
    _require_gpu(x, edge_index, edge_attr)
    n = int(nodes_per_graph)
    N = x.size(0)
    if graph_ptr is not None:
        _require_gpu(graph_ptr)
        if graph_ptr.dtype != torch.int64 or graph_ptr.dim() != 1 or graph_ptr.numel() < 2 or not graph_ptr.is_contiguous():
            raise ValueError("graph_ptr must be a contiguous 1-D int64 tensor of at least 2 elements (G + 1 row offsets)")
        if n < 1 or N == 0:
            raise ValueError(f"with a graph_ptr nodes_per_graph = {nodes_per_graph} is the bound on a graph's bus count: at least 1, "
                             f"and x must have rows")
    elif n < 1 or N == 0 or N % n != 0:
        raise ValueError(f"x has {N} rows: not a positive multiple of nodes_per_graph = {nodes_per_graph}")
    if int(max_iter) < 1:
        raise ValueError("max_iter must be at least 1")
    if not tol >= 0:
        raise ValueError("tol must be >= 0")
    if len(weights) != 3:
        raise ValueError("weights = (w_v, w_p, w_pf)")
    if check_own is not None:
        check_own()
    if x.dim() != 2 or x.size(1) < 10 or edge_attr.dim() != 2 or edge_attr.size(1) < 10:
        raise ValueError("x must be the full [N, 11] node tensor and edge_attr the full [E, 13] edge tensor")
    if init is not None:
        _require_gpu(init)
        if init.dim() != 2 or tuple(init.shape) != (N, 2):
            raise ValueError(f"init must be [N, 2] = ({N}, 2), got {tuple(init.shape)}")
    refuse_size(n)
    dev = x.device
    x2, ldx = _rows(x)
    ea2, ldea = _rows(edge_attr)
    incidence, E = _incidence(edge_index, N)
    G = N // n if graph_ptr is None else graph_ptr.numel() - 1
    if graph_ptr is not None:
        a.graph_ptr, a.n_graphs = graph_ptr.data_ptr(), G
    a.x, a.ldx, a.edge_attr, a.ldea = x2.data_ptr(), ldx, ea2.data_ptr(), ldea
    stats = (_vec(x_mean, 8, dev), _vec(x_std, 8, dev), _vec(edge_mean, 4, dev), _vec(edge_std, 4, dev))
    a.x_mean, a.x_std, a.edge_mean, a.edge_std = (s.data_ptr() for s in stats)
    a.efrom, a.eto, a.inc_rowptr, a.inc_ent = incidence
    a.n_nodes, a.n_edges, a.nodes_per_graph, a.max_iter, a.tol = N, E, n, int(max_iter), float(tol)
    a.w_v, a.w_p, a.w_pf = (float(w) for w in weights)
    kept_init = None
    if init is not None:
        kept_init, ld_init = _rows(init.detach())
        a.init, a.ld_init = kept_init.data_ptr(), ld_init
    out = WLSResult((torch.empty if graph_ptr is None else torch.zeros)(N, 2, dtype=_F32, device=dev), torch.empty(G, 2, dtype=torch.float64, device=dev),
                    torch.empty(G, dtype=torch.int32, device=dev), torch.empty(G, dtype=torch.int32, device=dev),
                    torch.empty(G, dtype=torch.float64, device=dev))
    a.state, a.objective, a.iterations, a.status, a.last_step = (t.data_ptr() for t in out)
    vmm = torch.empty(130, dtype=_F32, device=dev)
    a.vminmax, a.max_groups = vmm.data_ptr(), int(max_groups)
    return (x2, ea2, stats, kept_init, vmm), out, N, E, G


class _Huber(NamedTuple):        # the kinds of a solve beside the plain one (None), as the caller passed them: _solve checks them
    gamma: float
    plain_iters: int


class _BadData(NamedTuple):
    threshold: float
    max_removals: int
    confidence: float
    s_min: float


_LDS, _BLOCKED, _BANDED = "lds", "blocked", "banded"   # the storage forms
_PUBLIC_SUFFIX = {_LDS: "", _BLOCKED: "_large", _BANDED: "_banded"}     # of the public functions that run on a form (for messages)
_ENTRY_SUFFIX = {_LDS: "", _BLOCKED: "_large", _BANDED: "_large"}       # of the C entries of the solve and the Huber solve (the banded form enters through the blocked one's)


def _workspace(dev, need):
    """(address, bytes) of the kept workspace of ``need`` bytes on ``dev``."""
    if (dev, need) not in _WORKSPACES:
        _WORKSPACES[(dev, need)] = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    return _WORKSPACES[(dev, need)].data_ptr(), need


def _robust_outputs(args, solved, N, E, G, dev, ones):
    """The WLSRobustResult around ``solved`` that ``args`` writes.  ``ones``: a graph may write no row (``graph_ptr``)."""
    f64 = torch.float64
    res = WLSRobustResult(*solved, bus_q=(torch.ones if ones else torch.empty)(N, 4, dtype=f64, device=dev),
                          edge_q=torch.ones(E, 2, dtype=f64, device=dev),        # (an edge that leaves its graph is never written)
                          n_downweighted=torch.empty(G, dtype=torch.int32, device=dev))
    args.bus_q, args.edge_q, args.n_downweighted = (t.data_ptr() for t in res[5:])
    return res


def _bad_data_outputs(args, solved, N, E, G, dev, slots, zeros):
    """The WLSBadDataResult around ``solved`` that ``args`` writes.  ``zeros``: a graph may write no row (a refused one under
    ``graph_ptr``, one outside its band)."""
    f64, i32 = torch.float64, torch.int32
    new = lambda *shape, dtype=f64: torch.empty(*shape, dtype=dtype, device=dev)
    rows = (lambda *shape: torch.zeros(*shape, dtype=f64, device=dev)) if zeros else new
    res = WLSBadDataResult(
        *solved,
        dof=new(G, dtype=i32), chi2_limit=new(G), suspect=new(G, dtype=i32), removed=new(G, slots, dtype=i32), removed_rn=new(G, slots),
        n_removed=new(G, dtype=i32), bus_rn=rows(N, 4),
        edge_rn=torch.zeros(E, 2, dtype=f64, device=dev),       # (an edge that leaves its graph is never written)
        bus_sens=rows(N, 4), edge_sens=torch.zeros(E, 2, dtype=f64, device=dev), state_std=rows(N, 2))
    (args.dof, args.chi2_limit, args.suspect, args.removed, args.removed_rn, args.n_removed, args.bus_rn, args.edge_rn, args.bus_sens,
     args.edge_sens, args.state_std) = (t.data_ptr() for t in res[5:])
    return res


def _solve(kind, storage, x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, nodes_per_graph, init, max_iter, tol, weights,
           max_groups, graph_ptr=None, order=None):
    """The one road from the public functions to the library.  ``kind``: None (the plain solve -> WLSResult), a ``_Huber``
    (-> WLSRobustResult) or a ``_BadData`` (-> WLSBadDataResult).  ``storage``: ``_LDS`` (the gain matrix packed in LDS), ``_BLOCKED``
    (block rows in a workspace) or ``_BANDED`` (band rows in a workspace, on the graph relabelled by ``order``; None computes it here,
    which reads ``edge_index`` back); None lets the Huber solve choose between the first two by the bus count."""
    from .ops import gather_rows
    huber, bad = isinstance(kind, _Huber), isinstance(kind, _BadData)
    if huber:                    # (refused before anything else is looked at)
        kind = _Huber(float(kind.gamma), kind.plain_iters)
        if not kind.gamma > 0:
            raise ValueError("gamma must be > 0")
        if int(kind.plain_iters) != kind.plain_iters or kind.plain_iters < 0:
            raise ValueError("plain_iters must be an integer >= 0")
        if storage is None:
            storage = _BLOCKED if int(nodes_per_graph) > max_nodes_per_graph() else _LDS
    banded = storage == _BANDED
    who = f"wls_robust (large={storage == _BLOCKED})" if huber and not banded else \
        ("wls_robust" if huber else "wls_bad_data" if bad else "wls_estimate") + _PUBLIC_SUFFIX[storage]
    hb = 0
    if banded:
        if order is None:
            _require_gpu(x, edge_index, edge_attr)
            order = band_order(edge_index, nodes_per_graph, num_nodes=x.size(0))
        nodes_per_graph, hb = int(nodes_per_graph), int(order.half_bandwidth)

    def check_own():
        if bad:
            if not kind.threshold > 0:
                raise ValueError("threshold must be > 0")
            if int(kind.max_removals) != kind.max_removals or not 0 <= kind.max_removals <= 64:
                raise ValueError("max_removals must be an integer in 0 .. 64")
            if not 0 < kind.confidence < 1:
                raise ValueError("confidence must be in (0, 1)")
            if not 0 < kind.s_min < 1:
                raise ValueError("s_min must be in (0, 1)")
        if banded and (order.nodes_per_graph != nodes_per_graph or order.perm.numel() != x.size(0) or order.edge_index.shape != edge_index.shape):
            raise ValueError(f"order was made for {order.perm.numel()} buses in graphs of {order.nodes_per_graph} and "
                             f"{order.edge_index.size(1)} edges, not for this batch")

    def refuse_size(n):
        if banded:
            if band_lds_bytes(n, hb, bad) > _lib.WLS_BAND_LDS_BYTES:
                raise NotImplementedError(f"{who} keeps a band's panel and the state in LDS: at {n} buses per graph a "
                                          f"half-bandwidth hb of at most {band_max_half_bandwidth(n, bad)} states, got hb = {hb}")
        elif storage == _BLOCKED:
            if n > max_nodes_per_graph_large():
                raise NotImplementedError(f"{who} keeps a block column's panel of the gain matrix in LDS: at most "
                                          f"{max_nodes_per_graph_large()} buses per graph, got {n}")
        elif (_lib.lib().dss2_wls_bad_data_lds_bytes(n) > _LDS_CAP) if bad else n > max_nodes_per_graph():
            raise NotImplementedError(f"{who} keeps a graph's gain matrix in LDS: at most {max_nodes_per_graph()} buses per graph, got {n}")

    # the one place that picks the struct: plain LDS -> the solve block itself; every other form carries it as .solve
    args = _lib.WlsBadDataArgs() if bad else _lib.WlsRobustArgs() if huber else _lib.WlsSolveArgs() if storage == _LDS else _lib.WlsLargeArgs()
    a = getattr(args, "solve", args)
    # (on the band too the checks run on the caller's tensors; the rows are gathered once they have passed)
    keep, res, N, E, G = _solve_block(a, x, order.edge_index if banded else edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std,
                                      nodes_per_graph, init, max_iter, tol, weights, max_groups, refuse_size, check_own, graph_ptr=graph_ptr)
    n, dev = a.nodes_per_graph, x.device
    L = _lib.lib()
    if banded:
        xp = gather_rows(x, order.perm)
        a.x, a.ldx, a.half_bandwidth = xp.data_ptr(), xp.stride(0), hb
        ip = None
        if init is not None:
            ip = gather_rows(init.detach(), order.perm)
            a.init, a.ld_init = ip.data_ptr(), ip.stride(0)
        keep = (keep, xp, ip)
        args.workspace, args.workspace_bytes = _workspace(dev, band_workspace_bytes(n, hb, band_groups(G, max_groups)))
    elif storage == _BLOCKED:    # (kept by (device, bytes): a recorded launch replays with its address; in the bad-data struct a non-null workspace selects the forms on rows)
        args.workspace, args.workspace_bytes = _workspace(dev, int(L.dss2_wls_large_workspace_bytes(n, L.dss2_wls_large_groups(C.byref(a)))))
    per_bus = ()                 # the outputs per bus beside the state: on the band they come back in the kernel's order
    if huber:
        res = _robust_outputs(args, res, N, E, G, dev, ones=graph_ptr is not None)
        args.gamma, args.plain_iters = kind.gamma, int(kind.plain_iters)
        per_bus = ("bus_q",)
    elif bad:
        res = _bad_data_outputs(args, res, N, E, G, dev, max(int(kind.max_removals), 1), zeros=banded or graph_ptr is not None)
        args.threshold, args.max_removals, args.s_min = float(kind.threshold), int(kind.max_removals), float(kind.s_min)
        args.z_p = float(torch.special.ndtri(torch.tensor(float(kind.confidence), dtype=torch.float64)))   # (a host scalar from a Python float: no read-back)
        if banded:
            args.bus_label = order.perm.data_ptr()          # (the caller's row of the kernel's row k: for `removed` alone)
        per_bus = ("bus_rn", "bus_sens", "state_std")
    name = "dss2_wls_bad_data" if bad else ("dss2_wls_robust" if huber else "dss2_wls_solve") + _ENTRY_SUFFIX[storage]
    _lib.check(getattr(L, name)(C.byref(args), _stream(x)), name)
    del keep                     # (held until here: the launch has been issued)
    if banded:
        res = res._replace(state=gather_rows(res.state, order.inverse), **{f: _gather_f64(getattr(res, f), order.inverse) for f in per_bus})
    return res


class WLSRobustResult(NamedTuple):
    state: torch.Tensor          # as in WLSResult
    objective: torch.Tensor      # [G, 2] fp64: bus part and branch part of the Huber cost at the final fp64 state
    iterations: torch.Tensor
    status: torch.Tensor
    last_step: torch.Tensor
    bus_q: torch.Tensor          # [N, 4] fp64: the weight factors of (V, theta, P, Q) at the final state, 1 where not down-weighted
    edge_q: torch.Tensor         # [E, 2] fp64: of (P_from, Q_from)
    n_downweighted: torch.Tensor  # [G] int32: measurements with q < 1


def _wls_robust(x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, nodes_per_graph: int,
               init: Optional[torch.Tensor] = None, max_iter: int = 20, tol: float = 1e-6,
               weights: Sequence[float] = (1.0, 1.0, 1.0), gamma: float = 3.0, plain_iters: int = 1,
               large: Optional[bool] = None, max_groups: int = 0, graph_ptr: Optional[torch.Tensor] = None) -> WLSRobustResult:
    """The Huber M-estimator on ``wls_estimate``'s measurement model, by iteratively re-weighted Gauss-Newton: with w_i = c_k R^-1 the
    weight of measurement i, r_i its residual and t_i = sqrt(w_i) |r_i| at the current iterate, every iteration from number
    ``plain_iters`` on (counted from 0) is ``wls_estimate``'s with w_i q_i in place of w_i, q_i = gamma / t_i where t_i > gamma and
    1 elsewhere; the first ``plain_iters`` are plain (the default, 1, moves a flat start next to the solution before residuals are
    judged).  Start, slack angles, failure, decision, statuses and ``max_groups`` are ``wls_estimate``'s, and ``gamma = inf`` gives its
    result to the bit.  Reported at the final state: the Huber cost (t^2 up to gamma, 2 gamma t - gamma^2 above), every q, and the count
    of q < 1 per graph.  ``large`` None: the LDS kernel up to ``max_nodes_per_graph()`` buses, the blocked kernel above (up to
    ``max_nodes_per_graph_large()``); True / False force one.  gamma = 3 is the default for a reason: at 1.5, on ober179 (condition
    number 2.4e13), three to four measurements per graph are down-weighted and the state is worse than plain WLS.
    ``graph_ptr`` as for ``wls_estimate``: ``nodes_per_graph`` is then an upper bound, and ``large`` None routes by the bound."""
    return _solve(_Huber(gamma, plain_iters), None if large is None else _BLOCKED if large else _LDS, x, edge_index, edge_attr, x_mean, x_std,
                  edge_mean, edge_std, nodes_per_graph, init, max_iter, tol, weights, max_groups, graph_ptr=graph_ptr)


class WLSBadDataResult(NamedTuple):
    state: torch.Tensor          # as in WLSResult; of the final solve
    objective: torch.Tensor      # [G, 2] fp64: J at the final state with the removed measurements' weights at 0
    iterations: torch.Tensor     # [G] int32: updates applied, summed over all solves
    status: torch.Tensor         # [G] int32: of the final solve; 2 if any factorisation failed
    last_step: torch.Tensor      # [G] fp64
    dof: torch.Tensor            # [G] int32: active measurements - free states
    chi2_limit: torch.Tensor     # [G] fp64: Wilson-Hilferty quantile of chi2(dof) at `confidence`; +inf for dof <= 0
    suspect: torch.Tensor        # [G] int32: J > chi2_limit
    removed: torch.Tensor        # [G, max(max_removals, 1)] int32: ids in the order of removal, -1 in unused slots
    removed_rn: torch.Tensor     # [G, max(max_removals, 1)] fp64: their normalized residuals at removal
    n_removed: torch.Tensor      # [G] int32
    bus_rn: torch.Tensor         # [N, 4] fp64: normalized residuals of (V, theta, P, Q) at the final solve, 0 where inactive
    edge_rn: torch.Tensor        # [E, 2] fp64: of (P_from, Q_from)
    bus_sens: torch.Tensor       # [N, 4] fp64: residual sensitivities S_i = w_i Omega_ii
    edge_sens: torch.Tensor      # [E, 2] fp64
    state_std: torch.Tensor      # [N, 2] fp64: sqrt(diag (H^T W H)^-1), 0 at slack angles


def _wls_bad_data(x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, nodes_per_graph: int,
                 init: Optional[torch.Tensor] = None, max_iter: int = 10, tol: float = 1e-6,
                 weights: Sequence[float] = (1.0, 1.0, 1.0), threshold: float = 3.0, max_removals: int = 0,
                 confidence: float = 0.95, s_min: float = 1e-3, max_groups: int = 0,
                 graph_ptr: Optional[torch.Tensor] = None, large: bool = False) -> WLSBadDataResult:
    """``wls_estimate`` followed, inside the same launch, by the chi-square test, the largest-normalized-residual test and up to
    ``max_removals`` removals, each followed by a re-solve from the current state.  A measurement is active if its weight
    c_k R^-1 is above 0 and it has not been removed; S_i = 1 - w_i h_i Sigma h_i^T, rN_i = |z_i - h_i(u)| sqrt(w_i / S_i) where
    S_i >= ``s_min`` and 0 below it (critical measurements).  The largest rN above ``threshold`` is removed (ties: the smallest id).
    Ids: 4 i + k for bus i (row of x), k in V, theta, P, Q; 4 N + 2 e + k for stored branch e, k in P_from, Q_from.
    With ``max_removals = 0`` the first five fields are ``wls_estimate``'s, bit for bit.
    ``graph_ptr`` as for ``wls_estimate``: ``nodes_per_graph`` is then an upper bound (a bound above 99 is refused as 100 buses are),
    and the ids -- ``removed`` among them -- stay the global ones above.
    ``large`` (``wls_bad_data_large``): the blocked form, up to ``max_nodes_per_graph_large()`` buses, with ``wls_estimate_large``'s workspace."""
    return _solve(_BadData(threshold, max_removals, confidence, s_min), _BLOCKED if large else _LDS, x, edge_index, edge_attr, x_mean, x_std,
                  edge_mean, edge_std, nodes_per_graph, init, max_iter, tol, weights, max_groups, graph_ptr=graph_ptr)


def _wls_bad_data_large(x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, nodes_per_graph: int,
                       init: Optional[torch.Tensor] = None, max_iter: int = 10, tol: float = 1e-6,
                       weights: Sequence[float] = (1.0, 1.0, 1.0), threshold: float = 3.0, max_removals: int = 0,
                       confidence: float = 0.95, s_min: float = 1e-3, max_groups: int = 0,
                       graph_ptr: Optional[torch.Tensor] = None) -> WLSBadDataResult:
    """``wls_bad_data`` -- the same inputs, rounds, result and decisions -- for graphs of up to ``max_nodes_per_graph_large()`` buses,
    small ones included: the solves are ``wls_estimate_large``'s (its five outputs to the bit with ``max_removals = 0``), and the gain
    matrix is inverted in place on its block rows in ``wls_estimate_large``'s workspace, csrc/dss2_wls_bad_data.hip.  Still one launch,
    recordable.  Against ``wls_bad_data`` on a graph both serve the sums run in another order: equal to rounding, not to the bit.
    ``graph_ptr`` as for ``wls_estimate``: with it ``nodes_per_graph`` is an upper bound, and the workspace is sized by the bound."""
    return _wls_bad_data(x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, nodes_per_graph, init, max_iter, tol, weights, threshold,
                         max_removals, confidence, s_min, max_groups, graph_ptr=graph_ptr, large=True)


# ---- beyond 256 buses: the banded form of the blocked kernel on a reordered grid (csrc/dss2_wls_banded.hpp) -------------------------

class BandOrder(NamedTuple):
    """What ``band_order`` found for one batch structure; ``wls_estimate_banded(order=...)`` solves the relabelled batch with it."""
    perm: torch.Tensor           # [N] int32: row k of the relabelled batch is row perm[k] of the caller's (x, init are gathered by it)
    inverse: torch.Tensor        # [N] int32: the caller's row i is row inverse[i] of the relabelled batch (the state is gathered by it)
    edge_index: torch.Tensor     # [2, E]: the caller's edge list with both endpoints relabelled; stored order and orientation kept
    topology: object             # the relabelled edge list's Topology (its incidence CSR is the kernel's); None for a CPU edge list
    half_bandwidth: int          # hb in states: >= r - c over every non-zero G[r, c] of every graph, relabelled
    nodes_per_graph: int
    n_orderings: int             # distinct topologies ordered (graphs with equal relative edge lists share one)


def _cuthill_mckee(n, adj):
    """Reverse Cuthill-McKee of a graph of n buses (adj: sorted neighbour lists): order[k] = the bus numbered k.  Every component is
    numbered breadth-first from a pseudo-peripheral bus, neighbours by ascending degree; every tie goes to the lower bus index."""
    deg = [len(a) for a in adj]

    def levels(root):
        seen, level, out = {root}, [root], []
        while level:
            out.append(level)
            nxt = []
            for u in level:
                for v in adj[u]:
                    if v not in seen:
                        seen.add(v)
                        nxt.append(v)
            level = nxt
        return out

    done, order = [False] * n, []
    for seed in sorted(range(n), key=lambda v: (deg[v], v)):
        if done[seed]:
            continue
        root, lv = seed, levels(seed)
        while True:              # pseudo-peripheral: move to the lowest-degree bus of the last level while that deepens the levels
            far = min(lv[-1], key=lambda v: (deg[v], v))
            lv2 = levels(far)
            if len(lv2) <= len(lv):
                break
            root, lv = far, lv2
        done[root] = True
        queue, head = [root], 0
        while head < len(queue):
            for v in sorted(adj[queue[head]], key=lambda v: (deg[v], v)):
                if not done[v]:
                    done[v] = True
                    queue.append(v)
            head += 1
        order.extend(queue)
    return order[::-1]


def _two_hop_bandwidth(adj, label):
    """max |label[i] - label[j]| over the buses i, j within two branches of each other (the pattern of G), in buses."""
    bw = 0
    for i, a in enumerate(adj):
        reach = set(a)
        for j in a:
            reach.update(adj[j])
        if reach:
            bw = max(bw, max(abs(label[i] - label[j]) for j in reach))
    return bw


def band_half_bandwidth(bandwidth_buses: int) -> int:
    """hb in states for a 2-hop bandwidth in buses: bus i has the states 2 i and 2 i + 1."""
    return 2 * int(bandwidth_buses) + 1


def band_blocks(half_bandwidth: int) -> int:
    """Wb: the block columns a block row keeps left of its diagonal block."""
    return -(-int(half_bandwidth) // _lib.WLS_BAND_BLOCK)


def band_lds_bytes(nodes_per_graph: int, half_bandwidth: int, bad_data: bool = False) -> int:
    """The LDS of a workgroup of the banded kernel: wb_lds_bytes of csrc/dss2_wls_banded.hpp (the C side checks the same formula).
    ``bad_data``: of ``wls_bad_data_banded``'s, which keeps its fixed block (the arg-max's per-wave results, the removal list) behind it."""
    nb, n = _lib.WLS_BAND_BLOCK, int(nodes_per_graph)
    solve = (nb * (nb * band_blocks(half_bandwidth) + 8) + nb * nb + nb + 4 * n) * 8 + 16 + (n + 15) // 16 * 16
    return solve + (_lib.WLS_BAND_BAD_DATA_BYTES if bad_data else 0)


def band_groups(n_graphs: int, max_groups: int = 0) -> int:
    g = min(int(n_graphs), _lib.WLS_BAND_GROUPS)
    return min(g, int(max_groups)) if max_groups > 0 else g


def band_workspace_bytes(nodes_per_graph: int, half_bandwidth: int, groups: int) -> int:
    """One slice per workgroup: ceil(2 n / 16) block rows of 16 rows of 16 (Wb + 1) doubles, and the right-hand side behind them."""
    nb = _lib.WLS_BAND_BLOCK
    block_rows = -(-2 * int(nodes_per_graph) // nb)
    return int(groups) * block_rows * (nb * nb * (band_blocks(half_bandwidth) + 1) + nb) * 8


def band_max_half_bandwidth(nodes_per_graph: int, bad_data: bool = False) -> int:
    """The largest hb the banded kernel serves at this bus count (0: the bus count itself is beyond the LDS); ``bad_data``: the
    bad-data form's, whose fixed block in LDS comes off the same cap."""
    if band_lds_bytes(nodes_per_graph, 0, bad_data) > _lib.WLS_BAND_LDS_BYTES:
        return 0
    spare = (_lib.WLS_BAND_LDS_BYTES - band_lds_bytes(nodes_per_graph, 0, bad_data)) // (8 * _lib.WLS_BAND_BLOCK * _lib.WLS_BAND_BLOCK)
    return max(spare, 0) * _lib.WLS_BAND_BLOCK


def band_order(edge_index: torch.Tensor, nodes_per_graph: int, half_bandwidth: Optional[int] = None,
               num_nodes: Optional[int] = None, identity: bool = False) -> BandOrder:
    """Numbers the buses of every graph for a small bandwidth of the gain matrix (reverse Cuthill-McKee on the branch graph; G couples the
    buses within two branches) and returns the ``BandOrder`` that ``wls_estimate_banded`` solves with.  Host work, once per structure:
    ``edge_index`` is read back ONCE here, and nothing is read back per solve.  Graph g owns the buses [g n, (g + 1) n); graphs with equal
    relative edge lists share one ordering.  ``half_bandwidth`` may raise hb above what the numbering needs (ValueError below it);
    ``num_nodes`` counts buses behind the last branch (default: the last bus an edge names, rounded up to whole graphs);
    ``identity`` keeps the caller's numbering and only measures its hb."""
    n = int(nodes_per_graph)
    if n < 1 or edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise ValueError("band_order: edge_index must be [2, E] and nodes_per_graph at least 1")
    ei = edge_index.detach().cpu().numpy()         # the one read-back
    E = ei.shape[1]
    N = int(num_nodes) if num_nodes is not None else (-(-(int(ei.max()) + 1) // n) * n if E else n)
    if N < 1 or N % n != 0 or (E and (int(ei.min()) < 0 or int(ei.max()) >= N)):
        raise ValueError(f"band_order: {N} buses are not whole graphs of {n}, or an edge names a bus outside them")
    G = N // n
    gid = ei[0] // n
    if E and (ei[1] // n != gid).any():
        raise ValueError("band_order: an edge crosses graphs")
    by_graph = gid.argsort(kind="stable")
    starts = [0] * (G + 1)
    for g in gid.tolist():
        starts[g + 1] += 1
    for g in range(G):
        starts[g + 1] += starts[g]
    new_of_old = [0] * N
    orderings, bw = {}, 0
    for g in range(G):
        rel = ei[:, by_graph[starts[g]:starts[g + 1]]] - g * n
        key = rel.tobytes()
        if key not in orderings:
            adj = [set() for _ in range(n)]
            for f, t in rel.T.tolist():
                if f != t:
                    adj[f].add(t)
                    adj[t].add(f)
            adj = [sorted(a) for a in adj]
            order = list(range(n)) if identity else _cuthill_mckee(n, adj)
            label = [0] * n
            for k, old in enumerate(order):
                label[old] = k
            orderings[key] = (label, _two_hop_bandwidth(adj, label))
        label, b = orderings[key]
        bw = max(bw, b)
        for i in range(n):
            new_of_old[g * n + i] = g * n + label[i]
    hb = band_half_bandwidth(bw)
    if half_bandwidth is not None:
        if int(half_bandwidth) < hb:
            raise ValueError(f"band_order: half_bandwidth = {half_bandwidth} is below the {hb} states this numbering needs")
        hb = int(half_bandwidth)
    dev = edge_index.device
    inverse = torch.tensor(new_of_old, dtype=torch.int64)
    perm = torch.empty_like(inverse)
    perm[inverse] = torch.arange(N)
    relabelled = inverse[torch.from_numpy(ei).long()].to(edge_index.dtype).to(dev)
    topo = get_topology(relabelled, N) if relabelled.is_cuda and E else None
    return BandOrder(perm.int().to(dev), inverse.int().to(dev), relabelled, topo, hb, n, len(orderings))


def _gather_f64(t: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """``gather_rows`` of an fp64 [N, k] tensor: its rows travel as 2 k fp32 words each, which the gather copies as they are."""
    from .ops import gather_rows
    return gather_rows(t.view(_F32), idx).view(torch.float64)


def wls_estimate_banded(x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, nodes_per_graph: int,
                        init: Optional[torch.Tensor] = None, max_iter: int = 10, tol: float = 1e-6,
                        weights: Sequence[float] = (1.0, 1.0, 1.0), max_groups: int = 0,
                        order: Optional[BandOrder] = None) -> WLSResult:
    """``wls_estimate_large`` -- the same inputs, iteration, result and decisions -- without its cap of 256 buses, for grids whose gain
    matrix is a band once the buses are numbered for it (radial feeders, sparse meshes): the blocked kernel on rows that keep a band of
    G, csrc/dss2_wls_banded.hpp.  ``order``: ``band_order(edge_index, nodes_per_graph, num_nodes=N)`` of this structure; None computes it
    here, which reads ``edge_index`` back.  With a given ``order`` nothing is read back and every launch is the library's (two or three
    row gathers around the solve): recordable into a hipGraph or a launch plan.  The kernel solves the relabelled graph; ``x`` and
    ``init`` rows go in and the state comes out in the caller's bus order, ``edge_attr`` is used as it is.  Equal-size graphs whose
    topologies may differ.  NotImplementedError where (n, hb) needs more LDS than a workgroup has (``band_max_half_bandwidth(n)``).
    Not served here: ``graph_ptr`` batches.  The Huber form is ``wls_robust_banded``, bad-data detection ``wls_bad_data_banded`` (the
    covariance is wanted between buses within two branches of each other only -- inside the band, where the selected inverse gives it)."""
    return _solve(None, _BANDED, x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, nodes_per_graph, init, max_iter, tol, weights,
                  max_groups, order=order)


def wls_robust_banded(x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, nodes_per_graph: int,
                      init: Optional[torch.Tensor] = None, max_iter: int = 20, tol: float = 1e-6,
                      weights: Sequence[float] = (1.0, 1.0, 1.0), gamma: float = 3.0, plain_iters: int = 1,
                      max_groups: int = 0, order: Optional[BandOrder] = None) -> WLSRobustResult:
    """``wls_robust`` -- the same weighting, iteration, result and decisions -- beyond 256 buses per graph: the banded kernel of
    ``wls_estimate_banded`` with the Huber weighting on the row owners' walk (``gamma = inf`` gives ``wls_estimate_banded``'s five
    outputs to the bit).  ``order``, the bus order of inputs and outputs (``bus_q`` comes back in the caller's; ``edge_q`` is per stored
    edge), the cap on (n, hb) and the refusals are ``wls_estimate_banded``'s; with a given ``order`` nothing is read back."""
    return _solve(_Huber(gamma, plain_iters), _BANDED, x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, nodes_per_graph, init,
                  max_iter, tol, weights, max_groups, order=order)


def wls_bad_data_banded(x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, nodes_per_graph: int,
                        init: Optional[torch.Tensor] = None, max_iter: int = 10, tol: float = 1e-6,
                        weights: Sequence[float] = (1.0, 1.0, 1.0), threshold: float = 3.0, max_removals: int = 0,
                        confidence: float = 0.95, s_min: float = 1e-3, max_groups: int = 0,
                        order: Optional[BandOrder] = None) -> WLSBadDataResult:
    """``wls_bad_data_large`` -- the same rounds, result and decisions -- beyond 256 buses per graph, on the banded kernel of
    ``wls_estimate_banded`` (its five outputs to the bit with ``max_removals = 0``).  The test reads the covariance at its diagonal and
    between buses within two branches of each other: positions inside the band, which the selected inverse of the banded factor gives in
    place (csrc/dss2_wls_banded_invert.hpp) -- no dense inverse.  ``order`` and the bus order of inputs and outputs are
    ``wls_estimate_banded``'s: ``state``, ``bus_rn``, ``bus_sens`` and ``state_std`` come back in the caller's order, the edge outputs
    are per stored edge, and ``removed`` holds the caller's ids.  The kernel compares ids as it numbers the buses: a TIE in rN goes to
    the smallest relabelled id, not to the caller's smallest.  NotImplementedError above ``band_max_half_bandwidth(n, bad_data=True)``.
    A graph with a non-zero outside the band of ``order``: status 2, 0 iterations, objective 0, its start as its state, dof 0, no removal,
    per-measurement outputs 0.  With a given ``order`` nothing is read back and every launch is the library's: recordable."""
    return _solve(_BadData(threshold, max_removals, confidence, s_min), _BANDED, x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std,
                  nodes_per_graph, init, max_iter, tol, weights, max_groups, order=order)


def _public(impl):
    """The public form of an estimator function: the parameters it has always had -- what ``inspect.signature`` reports, and what callers
    and tests have pinned -- plus the keyword ``graph_ptr`` of the module docstring, which the wrapper takes off before the call and
    hands to ``impl``, the same function with ``graph_ptr`` as its last parameter.  Without it the call is the old one, untouched."""
    def deco(fn):
        sig = inspect.signature(fn)

        @functools.wraps(fn)
        def call(*args, graph_ptr=None, **kw):
            if graph_ptr is None:
                return fn(*args, **kw)
            bound = sig.bind(*args, **kw)
            return impl(*bound.args, **bound.kwargs, graph_ptr=graph_ptr)
        call.__doc__ = impl.__doc__
        return call
    return deco


@_public(_wls_estimate)
def wls_estimate(x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, nodes_per_graph: int,
                 init: Optional[torch.Tensor] = None, max_iter: int = 10, tol: float = 1e-6,
                 weights: Sequence[float] = (1.0, 1.0, 1.0), max_groups: int = 0) -> WLSResult:
    return _wls_estimate(x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, nodes_per_graph, init, max_iter, tol, weights, max_groups)


@_public(_wls_estimate_large)
def wls_estimate_large(x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, nodes_per_graph: int,
                       init: Optional[torch.Tensor] = None, max_iter: int = 10, tol: float = 1e-6,
                       weights: Sequence[float] = (1.0, 1.0, 1.0), max_groups: int = 0) -> WLSResult:
    return _wls_estimate_large(x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, nodes_per_graph, init, max_iter, tol, weights,
                               max_groups)


@_public(_wls_robust)
def wls_robust(x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, nodes_per_graph: int,
               init: Optional[torch.Tensor] = None, max_iter: int = 20, tol: float = 1e-6,
               weights: Sequence[float] = (1.0, 1.0, 1.0), gamma: float = 3.0, plain_iters: int = 1,
               large: Optional[bool] = None, max_groups: int = 0) -> WLSRobustResult:
    return _wls_robust(x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, nodes_per_graph, init, max_iter, tol, weights, gamma,
                       plain_iters, large, max_groups)


@_public(_wls_bad_data)
def wls_bad_data(x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, nodes_per_graph: int,
                 init: Optional[torch.Tensor] = None, max_iter: int = 10, tol: float = 1e-6,
                 weights: Sequence[float] = (1.0, 1.0, 1.0), threshold: float = 3.0, max_removals: int = 0,
                 confidence: float = 0.95, s_min: float = 1e-3, max_groups: int = 0) -> WLSBadDataResult:
    return _wls_bad_data(x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, nodes_per_graph, init, max_iter, tol, weights, threshold,
                         max_removals, confidence, s_min, max_groups)


@_public(_wls_bad_data_large)
def wls_bad_data_large(x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, nodes_per_graph: int,
                       init: Optional[torch.Tensor] = None, max_iter: int = 10, tol: float = 1e-6,
                       weights: Sequence[float] = (1.0, 1.0, 1.0), threshold: float = 3.0, max_removals: int = 0,
                       confidence: float = 0.95, s_min: float = 1e-3, max_groups: int = 0) -> WLSBadDataResult:
    return _wls_bad_data_large(x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, nodes_per_graph, init, max_iter, tol, weights,
                               threshold, max_removals, confidence, s_min, max_groups)
