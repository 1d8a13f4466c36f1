"""The reference's third model family, ``gnn_dsse`` (/root/reference/networks.py:11-69), with PyG's GCN2Conv and FAConv, on the
HIP kernels of csrc/dss2_gnn.hip.  TAGConv is networks.TAGConv; inside ``gnn_dsse`` it runs on the same kernels.

    GCN2Conv(channels, alpha, theta=None, layer=None, shared_weights=True, cached=False, add_self_loops=True, normalize=True)
    FAConv(channels, eps=0.1, dropout=0.0, cached=False, add_self_loops=True, normalize=True)
    gnn_dsse(dim_feat, dim_dense, dim_out, num_layers, nonlin='leaky_relu', main_param=0.1, K=3, bias=True, dropout=0.,
             theta=None, shared_weights=True, cached=True, add_self_loops=True, normalize=True, model='gcn2')

P is PyG's gcn_norm propagation (j = edge_index[0] the source, i = edge_index[1] the target): with add_self_loops, every self
loop in the list is dropped and each node gets one loop of weight 1 (add_remaining_self_loops); deg is counted at the target,
w_e = deg_j^-1/2 deg_i^-1/2.  TAGConv uses it without self loops; normalize=False (GCN2, TAG) is weight 1 on every edge.

    GCN2   out = ((1 - alpha) P h + alpha x_0) @ weight1          (shared_weights=False: ((1 - alpha) P h) @ weight1 + (alpha x_0) @ weight2)
    FA     out_i = sum_{e: j->i} tanh(att_l.h_j + att_r.h_i) w_e h_j  (+ eps x_0,i when eps != 0)
    TAG    out = sum_{k=0..K} (P^k h) @ lins[k].weight^T + bias

``gnn_dsse.model`` is ``lanegroup.SequentialX0`` with children ``module_{i}``; its forward is ONE autograd node on the launch
schedule of lanegroup.py, every launch through the library (so the step records into launch plans and hipGraphs):

    forward    GCN2 / FA: one launch per conv; TAG: K per conv (hops 1..K-1 write P^k h, hop K forms the sum); the head Linears
               run in the last launch
    backward   head backward + the local step of the last conv, then per conv its source pass (TAG: K adjoint hops) with the
               local step of the conv before fused into the last; one launch of the head's weight gradients; one slab reduction

``cached=True`` (GCN2, FA; PyG's meaning) keeps the normalised structure of the FIRST forward and reuses it for every later call,
whatever edge_index it is given: with more nodes the extra nodes have no edge and no loop.  With fewer nodes than that structure
references PyG fails with an index error; here ValueError.  ``reset_parameters()`` clears the cache.  So a cached model cannot run a
loader whose last batch is smaller, in the reference either; the driver wiring (runner.build_model) builds cached=False.

Refused (ValueError): widths over the limits (channels <= 32, head <= 32, TAG K <= 4), ``theta`` (PyG cannot build it without
``layer``), FAConv ``dropout > 0``, ``return_attention_weights`` and ``normalize=False``, an ``edge_weight``, CPU tensors and node ids
outside [0, N).  No bipartite inputs.
"""
from __future__ import annotations

import functools
from typing import Optional

import torch
import torch.nn as nn

from . import _lib, lanegroup
from .lanegroup import MAX_CHANNELS, MAX_DENSE
from .lanegroup import glorot as _glorot
from .ops import _ptr, _rows
from .topology import get_topology

_F32 = torch.float32
MAX_K = _lib.GNN_MAX_K
_check_width = functools.partial(lanegroup.check_width, "gnn_dsse")


class _CachedStructure:
    """The structure of the first forward (``cached=True``).  Cleared by ``reset_parameters``."""

    def _structure(self, edge_index, n, mode):
        if not self.cached or mode == 0:
            return _structure(edge_index, n, mode)
        if self._cached_struct is None:
            self._cached_struct = _structure(edge_index, n, mode)
        return _resized(self._cached_struct, n)


class GCN2Conv(_CachedStructure, nn.Module):
    """PyG ``GCN2Conv`` on the HIP kernels.  Parameters ``weight1 [C, C]`` (and ``weight2`` without shared weights), used as
    ``x @ weight1``; no bias.  ``forward(x, x_0, edge_index, edge_weight=None)``."""

    def __init__(self, channels: int, alpha: float, theta: Optional[float] = None, layer: Optional[int] = None,
                 shared_weights: bool = True, cached: bool = False, add_self_loops: bool = True, normalize: bool = True, **kwargs):
        super().__init__()
        _check_width("channels", channels, MAX_CHANNELS)
        if theta is not None or layer is not None:
            raise ValueError("GCN2Conv: theta / layer (the initial-residual identity mapping) are not supported; PyG itself "
                             "cannot build theta without layer")
        self.channels, self.alpha, self.beta = channels, float(alpha), 1.0
        self.cached, self.normalize, self.add_self_loops = cached, normalize, add_self_loops
        self._cached_struct = None
        self.weight1 = nn.Parameter(torch.empty(channels, channels))
        self.weight2 = None if shared_weights else nn.Parameter(torch.empty(channels, channels))
        self.reset_parameters()

    def reset_parameters(self) -> None:
        _glorot(self.weight1)
        if self.weight2 is not None:
            _glorot(self.weight2)
        self._cached_struct = None

    def _mode(self) -> int:
        return 0 if not self.normalize else (2 if self.add_self_loops else 1)

    def forward(self, x, x_0, edge_index, edge_weight=None):
        if edge_weight is not None:
            raise ValueError("GCN2Conv: edge_weight is not supported")
        return run_gnn([self], None, "none", x, x_0, edge_index)


class FAConv(_CachedStructure, nn.Module):
    """PyG ``FAConv`` on the HIP kernels.  Parameters ``att_l.weight``, ``att_r.weight`` ``[1, C]`` (no bias); no weight matrix.
    ``forward(x, x_0, edge_index, edge_weight=None)``."""

    def __init__(self, channels: int, eps: float = 0.1, dropout: float = 0.0, cached: bool = False, add_self_loops: bool = True,
                 normalize: bool = True, **kwargs):
        super().__init__()
        _check_width("channels", channels, MAX_CHANNELS)
        if dropout > 0:
            raise ValueError("FAConv: attention dropout is not supported (dropout must be 0)")
        if not normalize:
            raise ValueError("FAConv: normalize=False is not supported (PyG asserts on it without an edge_weight)")
        self.channels, self.eps, self.dropout = channels, float(eps), dropout
        self.cached, self.add_self_loops, self.normalize = cached, add_self_loops, normalize
        self._cached_struct = None
        self.att_l = nn.Linear(channels, 1, bias=False)
        self.att_r = nn.Linear(channels, 1, bias=False)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        self.att_l.reset_parameters()
        self.att_r.reset_parameters()
        self._cached_struct = None

    def _mode(self) -> int:
        return 2 if self.add_self_loops else 1

    def forward(self, x, x_0, edge_index, edge_weight=None, return_attention_weights=None):
        if edge_weight is not None:
            raise ValueError("FAConv: edge_weight is not supported")
        if return_attention_weights:
            raise ValueError("FAConv: return_attention_weights is not supported")
        return run_gnn([self], None, "none", x, x_0, edge_index)


class gnn_dsse(nn.Module):
    """/root/reference/networks.py:11-69: ``num_layers - 1`` convs of one kind, each followed by the (shared) nonlinearity, then
    Linear(dim_feat, dim_dense) and Linear(dim_dense, dim_out).  ``forward(x, edge_index)``; every conv sees x as x_0."""

    def __init__(self, dim_feat, dim_dense, dim_out, num_layers, nonlin="leaky_relu", main_param=0.1, K=3, bias=True, dropout=0.,
                 theta=None, shared_weights=True, cached=True, add_self_loops=True, normalize=True, model="gcn2"):
        super().__init__()
        from .networks import TAGConv
        self.channels = dim_feat
        self.main_param = main_param
        self.dim_out = dim_out
        self.K = K
        self.dropout = dropout
        self.bias = bias
        self.theta = theta
        self.num_layers = num_layers
        self.shared_weights = shared_weights
        self.cached = cached
        self.normalize = normalize
        self.add_self_loops = add_self_loops
        self.nonlin = lanegroup.nonlin_module(nonlin)
        _check_width("dim_feat", dim_feat, MAX_CHANNELS)
        _check_width("dim_dense", dim_dense, MAX_DENSE)
        _check_width("dim_out", dim_out, MAX_DENSE)
        if num_layers < 1:
            raise ValueError(f"num_layers = {num_layers}: at least 1 (the two Linears)")
        layers, convs = [], []
        for _ in range(num_layers - 1):
            if model == "gcn2":
                conv = GCN2Conv(channels=dim_feat, alpha=main_param, theta=theta, shared_weights=shared_weights, cached=cached,
                                normalize=normalize, add_self_loops=add_self_loops)
            elif model == "fagcn":
                conv = FAConv(channels=dim_feat, eps=main_param, dropout=dropout, cached=cached, normalize=normalize,
                              add_self_loops=add_self_loops)
            elif model == "tagcn":
                conv = TAGConv(in_channels=dim_feat, out_channels=dim_feat, K=K, bias=bias, normalize=normalize)
            else:
                raise ValueError("invalid model type")
            convs.append(conv)
            layers += [conv, self.nonlin]
        if model not in ("gcn2", "fagcn", "tagcn"):
            raise ValueError("invalid model type")
        if model == "gcn2" and theta is not None:
            raise ValueError("gnn_dsse: theta is not supported (PyG's GCN2Conv cannot build it without layer)")
        if model == "tagcn" and not 0 <= K <= MAX_K:
            raise ValueError(f"gnn_dsse: K = {K}: the tagcn kernels take 0 <= K <= {MAX_K}")
        head = [nn.Linear(dim_feat, dim_dense), nn.Linear(dim_dense, dim_out)]
        self.model = lanegroup.SequentialX0(layers + head, convs, head, nonlin, run_gnn)

    def forward(self, x, edge_index):
        x_0 = x
        return self.model(x, x_0, edge_index)


# ------------------------------------------------------------------------------------------
# structure: CSR by target and by source, gcn_norm's deg^-1/2
# ------------------------------------------------------------------------------------------
class _Structure:
    """One structure with its deg^-1/2 for one mode (0 weight 1, 1 gcn_norm, 2 gcn_norm with remaining self loops).  ``ref_n``:
    the node count its entries reference (every node with loops, else the largest node id + 1)."""

    def __init__(self, topo, dis, mode, ref_n):
        self.topo, self.dis, self.mode, self.ref_n = topo, dis, mode, ref_n
        self.N, self.E = topo.N, topo.E      # (the structure is built with double=False: the edges as given)
        self.rowptr, self.col, self.ent = topo.rowptr, topo.col, topo.ent
        self.rowptrT, self.colT, self.entT = topo.rowptrT, topo.colT, topo.entT
        self.loops = int(mode == 2)
        self._sized = {}


_NO_EDGES = {}


def _structure(edge_index, n, mode):
    dev = edge_index.device
    if edge_index.size(1) == 0:
        key = (dev.index, n)
        topo = _NO_EDGES.get(key)
        if topo is None:
            topo = _NO_EDGES[key] = lanegroup.NoEdges(n, dev)
    else:
        topo = get_topology(edge_index, n, double=False)
        topo.stats()       # (cached per structure) raises on node ids outside [0, N) before a kernel reads them
    cache = topo._gnn_structures
    st = cache.get(mode)
    if st is None:
        dis = torch.empty(n, dtype=_F32, device=dev)
        _lib.check(_lib.lib().dss2_gnn_dis(topo.rowptr.data_ptr(), topo.col.data_ptr(), n, mode, dis.data_ptr(),
                                           _lib.stream_ptr(dev)), "dss2_gnn_dis")
        ref_n = n if mode == 2 else (int(edge_index.max()) + 1 if edge_index.size(1) else 0)
        st = cache[mode] = _Structure(topo, dis, mode, ref_n)
    return st


class _Resized:
    """A cached structure seen by a batch of another node count: rows beyond its nodes are empty, with dis = 0 (no loop)."""

    def __init__(self, st, n):
        self.N, self.E, self.loops, self.mode = n, st.E, st.loops, st.mode
        self.col, self.ent, self.colT, self.entT = st.col, st.ent, st.colT, st.entT
        if n >= st.N:
            pad = n - st.N
            self.rowptr = torch.cat([st.rowptr, st.rowptr[-1:].expand(pad)])
            self.rowptrT = torch.cat([st.rowptrT, st.rowptrT[-1:].expand(pad)])
            self.dis = torch.cat([st.dis, st.dis.new_zeros(pad)])
        else:
            self.rowptr, self.rowptrT, self.dis = st.rowptr[:n + 1], st.rowptrT[:n + 1], st.dis[:n]


def _resized(st, n):
    if n == st.N:
        return st
    if n < st.ref_n:
        raise ValueError(f"the cached structure (cached=True) references {st.ref_n} nodes and this batch has {n}: PyG fails "
                         "here with an index error; build the model with cached=False or call reset_parameters()")
    hit = st._sized.get(n)
    if hit is None:
        hit = st._sized[n] = _Resized(st, n)
    return hit


# ------------------------------------------------------------------------------------------
# the fused route
# ------------------------------------------------------------------------------------------
def _kind(cv):
    from .networks import TAGConv
    if isinstance(cv, GCN2Conv):
        return _lib.GNN_GCN2
    if isinstance(cv, FAConv):
        return _lib.GNN_FA
    if isinstance(cv, TAGConv):
        return _lib.GNN_TAG
    raise ValueError(f"gnn stack: {type(cv).__name__} is not a GCN2Conv, FAConv or TAGConv")


def _conv_params(cv, kind):
    if kind == _lib.GNN_GCN2:
        return [cv.weight1, cv.weight2]
    if kind == _lib.GNN_FA:
        return [cv.att_l.weight, cv.att_r.weight]
    return [cv.bias] + [l.weight for l in cv.lins]


def _conv_mode(cv, kind):
    if kind == _lib.GNN_TAG:
        return 1 if cv.normalize else 0
    return cv._mode()


class _Spec(lanegroup.Spec):
    """Kind, width, hop count, slab layout and launch geometry of one conv stack (+ head)."""

    def __init__(self, convs, head, nonlin, n_nodes):
        kinds = {_kind(cv) for cv in convs}
        if len(kinds) > 1:
            raise ValueError("gnn stack: every conv must be of one kind")
        self.kind = kinds.pop() if kinds else 0
        C = 0
        if convs:
            if self.kind == _lib.GNN_TAG:
                if any(cv.in_channels != cv.out_channels for cv in convs):
                    raise ValueError("gnn stack: TAGConv in_channels must equal out_channels on these kernels")
                C = convs[0].in_channels
                if any(cv.in_channels != C for cv in convs):
                    raise ValueError("gnn stack: every conv must have the same width")
            else:
                C = convs[0].channels
                if any(cv.channels != C for cv in convs):
                    raise ValueError("gnn stack: every conv must have the same width")
        if convs and head and head[0].in_features != C:
            raise ValueError("gnn head: its input width must be the convs' width")
        self.c = C
        self.K = convs[0].K if convs and self.kind == _lib.GNN_TAG else 0
        if self.kind == _lib.GNN_TAG:
            if any(cv.K != self.K for cv in convs):
                raise ValueError("gnn stack: every TAGConv must have the same K")
            if not 0 <= self.K <= MAX_K:
                raise ValueError(f"TAGConv K = {self.K}: these kernels take 0 <= K <= {MAX_K}")
        self.shared = self.kind != _lib.GNN_GCN2 or all(cv.weight2 is None for cv in convs)
        if self.kind == _lib.GNN_GCN2 and any(cv.weight2 is None for cv in convs) and not self.shared:
            raise ValueError("gnn stack: mixed shared_weights")
        self.modes = [_conv_mode(cv, self.kind) for cv in convs]
        self.params = [cv.alpha if self.kind == _lib.GNN_GCN2 else (cv.eps if self.kind == _lib.GNN_FA else 0.0) for cv in convs]
        CC = C * C
        cols = {_lib.GNN_GCN2: CC * (1 if self.shared else 2), _lib.GNN_FA: 2 * C, _lib.GNN_TAG: C + (self.K + 1) * CC}.get(self.kind, 0)
        self.n_ps = {_lib.GNN_GCN2: 2, _lib.GNN_FA: 2, _lib.GNN_TAG: self.K + 2}.get(self.kind, 0)
        # TAG: hops 1..K-1 write P^k h and hop K forms the sum; the adjoint runs r_k = g_k + P^T r_{k+1} for k = K-1..0
        self.fwd_hops = tuple(range(1, self.K + 1)) or (0,)
        self.bwd_hops = tuple(range(self.K - 1, -1, -1)) or (0,)
        super().__init__("gnn_dsse", convs, head, nonlin, n_nodes, [C] if convs else [], [cols] * len(convs))


def _check_inputs(x, x_0, edge_index, params):
    for t in (x, x_0, edge_index, *params):
        if t is not None and not t.is_cuda:
            raise ValueError("gnn_dsse: the HIP kernels need GPU tensors (there is no CPU path)")
    for t in (x, x_0, *params):
        if t is not None and t.dtype != _F32:
            raise ValueError(f"gnn_dsse: the kernels compute in float32; got {t.dtype}")
    lanegroup.check_x(x, edge_index, int64=True)


def run_gnn(convs, head, nonlin, x, x_0, edge_index):
    ps = [t for cv in convs for t in _conv_params(cv, _kind(cv))]
    _check_inputs(x, x_0, edge_index, [t for t in ps if t is not None])
    spec = _Spec(convs, head, nonlin, x.size(0))
    lanegroup.check_columns(x, spec)
    if x_0 is x or spec.kind == _lib.GNN_TAG or not convs:
        x0 = None          # the x_0 path goes into x's gradient inside the kernels (TAG and the head have none)
    else:
        if x_0.dim() != 2 or x_0.size(0) != x.size(0) or x_0.size(1) != spec.c:
            raise ValueError(f"x_0 must be [N, {spec.c}]")
        x0 = x_0
    N = x.size(0)
    if N == 0:
        raise ValueError("gnn_dsse: empty batch")
    sts = [cv._structure(edge_index, N, m) if spec.kind != _lib.GNN_TAG else _structure(edge_index, N, m)
           for cv, m in zip(convs, spec.modes)]
    if not convs:
        st = None
    else:
        st = sts[0]
        if any(s is not st for s in sts):
            raise ValueError("gnn stack: the convs see different structures (a cached structure of one conv only); call "
                             "reset_parameters() on every conv")
    hps = [p for m in head for p in (m.weight, m.bias)] if head else []
    return _GnnFn.apply(x, x0, st, spec, *ps, *hps)


def _graph(st, spec, N, slab=None):
    g = _lib.GnnGraph()
    if st is not None:
        lanegroup.fill_csr(g, st)
        g.dis, g.loops = st.dis.data_ptr(), st.loops
    g.n_nodes, g.nonlin = N, spec.nonlin
    g.slab, g.n_slabs, g.slab_len = _ptr(slab), spec.n_slabs, spec.total
    return g


class _GnnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, x0, st, spec, *ps):
        N, dev, C, K, n = x.size(0), x.device, spec.c, spec.K, len(spec.convs)
        x, ldx = _rows(x)
        x0_sep = x0 is not None
        if x0 is not None:
            x0, ldx0 = _rows(x0)
        else:
            x0, ldx0 = x, ldx
        cps, hps = ps[:n * spec.n_ps], ps[n * spec.n_ps:]

        def extra(l):
            if spec.kind == _lib.GNN_GCN2:
                return {"u": torch.empty(N, C, dtype=_F32, device=dev)}
            if spec.kind == _lib.GNN_TAG and K:
                return {"u": torch.empty(K, N, C, dtype=_F32, device=dev)}
            return {}

        states, hs = lanegroup.state_chain(x, ldx, [C] * n, extra)

        def conv_into(d, l, bufs=None):
            d.kind, d.K, d.c, d.slab_off = spec.kind, K, C, spec.offs[l]
            w = cps[l * spec.n_ps:(l + 1) * spec.n_ps]
            if spec.kind == _lib.GNN_TAG:
                d.bias = _ptr(w[0])
                for m in range(K + 1):
                    d.W[m] = _ptr(w[1 + m])
            else:
                d.W[0], d.W[1] = _ptr(w[0]), _ptr(w[1])
            d.h, d.ldh = hs[l][0].data_ptr(), hs[l][1]
            d.x0, d.ldx0 = x0.data_ptr(), ldx0
            d.param = spec.params[l]
            d.y, d.u = states[l]["y"].data_ptr(), _ptr(states[l].get("u"))
            if bufs is not None:
                d.d, d.se, d.sn, d.part = (_ptr(bufs.get(k)) for k in ("d", "se", "sn", "part"))

        def hook(a, l, hop):
            a.hop = hop

        hst, out = lanegroup.forward(spec, _graph(st, spec, N), _lib.GnnArgs, "dss2_gnn_forward", conv_into, x, ldx, hps, hook)
        if out is None:
            out = states[-1]["y"]
        ctx.save_for_backward(x, x0)
        ctx.st = (st, spec, ldx, states, hps, hst, conv_into, x0_sep)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, x0 = ctx.saved_tensors
        st, spec, ldx, states, hps, hst, conv_fwd, sep_x0 = ctx.st
        N, dev, C, K, n, head = x.size(0), gout.device, spec.c, spec.K, len(spec.convs), spec.head
        gout, ldgo = _rows(gout)
        slab = torch.empty(spec.n_slabs * spec.total, dtype=_F32, device=dev)
        flat = torch.empty(spec.total, dtype=_F32, device=dev)
        need_dx = ctx.needs_input_grad[0]
        dx = torch.empty(N, x.size(1), dtype=_F32, device=dev) if need_dx else None
        need_x0 = sep_x0 and ctx.needs_input_grad[1]
        has_x0 = n and spec.kind != _lib.GNN_TAG and (need_x0 or (need_dx and not sep_x0))
        dx0 = torch.empty(N, C, dtype=_F32, device=dev) if has_x0 else None
        fused_x0 = dx0 is not None and not sep_x0
        E = st.E if st is not None else 0
        bufs = []
        for _ in range(min(n, 2)):
            b = {}
            if spec.kind == _lib.GNN_TAG:
                b["d"] = torch.empty(K + 1, N, C, dtype=_F32, device=dev)
            else:
                b["d"] = torch.empty(N, C, dtype=_F32, device=dev)
            if spec.kind == _lib.GNN_FA:
                b["se"] = torch.empty(max(E, 1), dtype=_F32, device=dev)
                b["sn"] = torch.empty(N, dtype=_F32, device=dev)
                b["part"] = torch.empty(N, C, dtype=_F32, device=dev)
            bufs.append(b)
        rbuf = [torch.empty(N, C, dtype=_F32, device=dev) for _ in range(2)] if (spec.kind == _lib.GNN_TAG and K > 1) else None

        def conv_into(d, l):
            conv_fwd(d, l, bufs[l % 2])

        def hook(a, l, hop):
            a.hop = hop
            if l == n:                  # the first launch: with a conv, its local step starts the x_0 gradient
                if n:
                    a.dx0_first, a.dx0 = 1, _ptr(dx0)
                return
            if spec.kind == _lib.GNN_TAG and K:
                a.rin = bufs[l % 2]["d"].data_ptr() + 4 * K * N * C if hop == K - 1 else rbuf[(hop + 1) % 2].data_ptr()
                a.rout = rbuf[hop % 2].data_ptr() if hop > 0 else None
            if hop == 0 and (l > 0 or fused_x0):        # the local step of conv l - 1 adds to it; conv 0's folds it into dx
                a.dx0 = _ptr(dx0)

        lanegroup.backward(spec, _graph(st, spec, N, slab), _lib.GnnArgs, "dss2_gnn_backward", conv_into, gout, ldgo, hps, hst, dx,
                           hook)
        # the head's outer-product weight gradients, then ONE fixed-order reduction
        if head:
            lanegroup.wgrad(lanegroup.head_wgrad_jobs(spec, states, x, ldx, hst, gout, ldgo), slab, spec, N, dev)
        lanegroup.reduce_slabs([(slab, flat, spec.total, spec.total, spec.n_slabs)], dev)
        grads, CC = [], C * C
        for l in range(n):
            o = spec.offs[l]
            if spec.kind == _lib.GNN_GCN2:
                grads += [flat[o:o + CC].view(C, C), None if spec.shared else flat[o + CC:o + 2 * CC].view(C, C)]
            elif spec.kind == _lib.GNN_FA:
                grads += [flat[o:o + C].view(1, C), flat[o + C:o + 2 * C].view(1, C)]
            else:
                grads.append(flat[o:o + C] if spec.convs[l].bias is not None else None)
                grads += [flat[o + C + m * CC:o + C + (m + 1) * CC].view(C, C) for m in range(K + 1)]
        grads += lanegroup.head_grads(spec, flat)
        return lanegroup.backward_result(ctx, dx, grads, dx0 if need_x0 else None)
