"""Drop-in for the hot-path classes of the reference's ``networks.py``, on hand-written HIP kernels.

Same names, constructor arguments, ``forward(x, edge_index, edge_attr)`` signatures and
``state_dict`` keys as /root/reference/networks.py:159-388:

    EdgeAggregation(dim_featn, dim_feate, dim_hid, dim_out)            networks.py:159-209
    MPN / SkipMPN(dim_featn, dim_feate, dim_out, dim_hid, n_gnn_layers, K, dropout_rate)
                                                                       networks.py:212-338
    PFN / SkipPFN(..., L)                                              networks.py:340-388
    TAGConv(in_channels, out_channels, K)       PyG's operator as used at networks.py:230-234

All compute runs in libdss2_hip.so (include/dss2_hip.h) through ctypes; tensors must be fp32 on a
gfx950 device.  There is no CPU or eager-PyTorch fallback: CPU tensors raise.

Preserved reference behaviour: concat order [x_i | x_j | edge_attr]; first-edge-only
``is_directed``; reverse edges with edge_attr columns 0 and 2 negated; no self loops; dropout
applied in ``eval()`` too (a fresh nn.Dropout is built inside forward, networks.py:268); ReLU after
dropout; no activation after the last conv; SkipMPN's residual.
"""
from __future__ import annotations

import ctypes as C
import os as _os
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .topology import LDS_LIMIT, Topology, get_topology

_F32 = torch.float32

from . import flags as FL
from .ops import (_DROP_PARAMS, _dropout_params, _ncg, _ptr, _reduce, _require_gpu, _round16, _round8, _rows, _stream, _wgrad_per_cu, _wgrad_tiles, chain16_supported, chain_f16_supported, chain_gate_words, chain_edge_supported, chain_head_supported, chain_head_wgrad_supported, chain_supported, csr_axpy, dropout_mask, dropout_snapshot, edge_bwd, edge_fwd, gather_rows, gemm16_supported, gemm_plan, gemm_prop, gemm_prop_chain, is_narrow, finish_weights, prep_weights, reduce_pending, segment_sum, wgrad, wgrad_batched)
from .plans import (_DESC_DTYPE, _FoldPlan, _MatView, _PackPlan, _SG_DTYPE, _as_view, _pack_table, _sg, _sg_table, _small_gemm)
from .route import BlockRoute, block_route, use_global_path


# ------------------------------------------------------------------------------------------
# functional pieces (raw tensors in, raw tensors out); used by the autograd Functions below
# ------------------------------------------------------------------------------------------
def _edge_tiled(ts, N: int = 0):
    """(tiled, n_slabs) of an edge MLP on the tile set ``ts``: forward and backward run the tile kernels together or not at all (the
    backward recomputes the forward's gates) -- where the entry tables of BOTH directions exist; else the row-per-wave kernels on the
    CSR (general graphs: hub nodes beyond the ELL width, on either side).  n_slabs: the backward's slabs over ``N`` nodes."""
    tiled = ts.ell_ent_tiles is not None and ts.ellT_ent_tiles is not None and FL.EDGE_TILE_KERNELS
    return tiled, (min(ts.ntiles, 512) if tiled else int(min(512, max(1, (N + 15) // 16))))


def _edge_aggr_forward(topo, x, ldx, ea, ldea, W1, b1, b2, pack_w2_fwd, hid, hout, fn, fe, second_linear=True, need_dx=False):
    """need_dx: the backward will be asked for the gradient w.r.t. x (the library then picks the forward whose gates that backward recomputes exactly)."""
    N = topo.N
    S = torch.empty(N, hid, dtype=_F32, device=W1.device)
    edge_fwd(topo, _edge_tiled(topo.tiling)[0], x, ldx, ea, ldea, W1, b1, S, hid, fn, fe, need_dx)
    if not second_linear:   # folded into the consumer (see _FoldPlan)
        return S, None
    x0 = torch.empty(N, hout, dtype=_F32, device=W1.device)
    # second Linear of the edge MLP after the (linear) aggregation: sum_e (W2 h_e + b2) = W2 S + deg b2
    gemm_prop(topo, S, hid, hid, pack_w2_fwd, 1, hout, x0, bias=b2, rowscale=topo.deg)
    return S, x0


def _edge_aggr_backward(topo, gx0, x, ldx, ea, ldea, W1, b1, S, pack_w2_bwd, hid, hout, fn, fe, g_w1, g_w2, need_dx,
                        pack_dx=None, dS=None, pending=None, dx_add=None):
    """g_w1: flat [hid*(2fn+fe) + hid] <- dW1, db1;  g_w2: flat [hout*hid + hout] <- dW2, db2.
    With ``dS`` given (second Linear folded into the consumer) gx0 / g_w2 are not used.
    pack_dx = (W1[:, :fn] packed, W1[:, fn:2fn] packed[, both stacked along k]); dx_add [N, fn] is added to the result
    (the skip connection's gradient).  Returns dx [N, fn] or None."""
    N, ts = topo.N, topo.tiling
    if dS is None:
        wgrad(topo, gx0, hout, S, hid, 1, g_w2, rowscale=topo.deg, pending=pending)
        dS = torch.empty(N, hid, dtype=_F32, device=gx0.device)
        gemm_prop(topo, gx0, gx0.stride(0), hout, pack_w2_bwd, 1, hid, dS)
    gx0 = dS
    dev = dS.device
    stride = hid * (2 * fn + fe) + hid
    tiled, n_slabs = _edge_tiled(ts, N)
    slab = torch.empty(n_slabs * stride, dtype=_F32, device=dev)
    # U0 = sum of dz over incoming edges (x enters as x_i), U1 over outgoing edges (as x_j).  Side by side in one [N, 2 hid]
    # buffer when the K = 2 hid tile fits LDS: dx is then ONE GEMM [U0 | U1] [W1[:, :fn] ; W1[:, fn:2fn]]
    merged = bool(need_dx and pack_dx is not None and len(pack_dx) > 2 and pack_dx[2] is not None and FL.DX_MERGE and
                  gemm_plan(ts, 1, 2 * hid, fn, graph=(0, 0)).sizing_lds <= LDS_LIMIT)
    if not need_dx:
        U = u0 = u1 = None
        ldu = hid
    elif merged:
        U = torch.empty(N, 2 * hid, dtype=_F32, device=dev)
        u0, u1, ldu = U, U[:, hid:], 2 * hid
    else:
        U = torch.empty(2, N, hid, dtype=_F32, device=dev)
        u0, u1, ldu = U[0], U[1], hid

    # over the incoming edges (dW1 | db1 slabs, U0), then -- transposed -- the outgoing ones (U1)
    edge_bwd(topo, tiled, x, ldx, ea, ldea, W1, b1, dS, slab, n_slabs, u0, ldu, hid, fn, fe, False)
    _reduce(slab, 0, n_slabs, stride, g_w1, stride, pending)
    if not need_dx:
        return None
    edge_bwd(topo, tiled, x, ldx, ea, ldea, W1, b1, dS, None, n_slabs, u1, ldu, hid, fn, fe, True)
    dx = torch.empty(N, fn, dtype=_F32, device=dev)
    if merged:
        gemm_prop(topo, U, 2 * hid, 2 * hid, pack_dx[2], 1, fn, dx, add_src=dx_add,
                  add_ld=(dx_add.stride(0) if dx_add is not None else 0))
        return dx
    # two K = hid -> fn GEMMs on the tile kernel (the two W1 blocks are packed in place by the module's pack launch), the
    # second adding the first through the residual epilogue
    dx0 = torch.empty(N, fn, dtype=_F32, device=dev)
    gemm_prop(topo, u0, hid, hid, pack_dx[0], 1, fn, dx0)
    gemm_prop(topo, u1, hid, hid, pack_dx[1], 1, fn, dx, add_src=dx0, add_ld=fn)
    return dx if dx_add is None else dx + dx_add


def _dx_views(W1, hid, fn, fe):
    """W1[:, :fn] (x enters as x_i) and W1[:, fn:2fn] (as x_j) as in-place blocks for the pack kernel: each alone, and
    both as one group (packed stacked along k for the merged dx GEMM, see _edge_aggr_backward)."""
    ld = 2 * fn + fe
    a, b = _MatView(W1, hid, fn, ld, 0), _MatView(W1, hid, fn, ld, fn)
    return [[a], [b], [a, b]]


def _tagconv_forward(topo, h, pack_fwd, bias, nmat, hin, hout, dmask=None, relu=False, add_src=None, add_ld=0,
                     prebias=None, pre_rowscale=None, drop=None, b_format=0):
    out = torch.empty(topo.N, hout, dtype=_F32, device=h.device)
    # (a folded bias or in-kernel dropout needs the general kernel: dss2_gemm_prop refuses them on a narrow launch, include/dss2_hip.h)
    narrow = is_narrow(nmat, hout) and prebias is None and (drop is None or drop[2] == 0)
    gemm_prop(topo, h, h.stride(0), hin, pack_fwd, nmat, hout, out, bias=bias, dmask=dmask, relu=relu,
              add_src=add_src, add_ld=add_ld, narrow_h=(hout if narrow else 0),
              prebias=prebias, pre_rowscale=pre_rowscale, drop=drop, b_format=b_format)
    return out


def _tagconv_forward_global(topo, h, pack_fwd, bias, nmat, hin, hout, relu=False, add_src=None, add_ld=0, drop=None):
    """TAGConv for graphs beyond the LDS-resident tiles (> 192 nodes): ONE plain tile GEMM X [W_0|..|W_K]^T, then K
    propagation hops in global memory in Horner order, the last one carrying the epilogue.  ``pack_fwd`` is the stacked
    layout of _PackPlan(stacked=True)."""
    N, dev = topo.N, h.device
    out = torch.empty(N, hout, dtype=_F32, device=dev)
    if nmat == 1:
        gemm_prop(topo, h, h.stride(0), hin, pack_fwd, 1, hout, out, bias=bias, relu=relu, add_src=add_src, add_ld=add_ld, drop=drop)
        return out
    wcat = nmat * hout
    Gc = torch.empty(N, (wcat + 3) // 4 * 4, dtype=_F32, device=dev)
    gemm_prop(topo, h, h.stride(0), hin, pack_fwd, 1, wcat, Gc)
    T = Gc[:, (nmat - 1) * hout:]
    for m in range(nmat - 2, -1, -1):
        blk = Gc[:, m * hout:(m + 1) * hout]
        if m > 0:
            csr_axpy(topo, T, blk, hout, add=blk)          # in place: T_m = G_m + A_hat T_{m+1}
            T = blk
        else:
            csr_axpy(topo, T, out, hout, add=blk, bias=bias, relu=relu, add_src=add_src, add_ld=add_ld, drop=drop)
    return out


def _tagconv_backward_global(topo, g, h, pack_bwd, nmat, hin, hout, g_flat, relu_src=None, need_dh=True, pending=None, drop=None):
    """Backward of _tagconv_forward_global.  Z = [g | A^T g | .. | (A^T)^K g] (K hops in global memory); then
    dW_m = Z_m^T h and db as ONE weight-gradient launch on the stacked Z, dh = Z [W_0; ..; W_K] as ONE plain GEMM."""
    N, dev = topo.N, g.device
    if nmat == 1:
        Z, wcat = g, hout
    else:
        wcat = nmat * hout
        Z = torch.empty(N, (wcat + 3) // 4 * 4, dtype=_F32, device=dev)
        if Z.size(1) != wcat:
            Z[:, wcat:].zero_()
        Z[:, :hout].copy_(g)
        for m in range(1, nmat):
            csr_axpy(topo, Z[:, (m - 1) * hout:], Z[:, m * hout:], hout, transposed=True)
    wgrad(topo, Z, wcat, h, hin, 1, g_flat, pending=pending, out_len=wcat * hin + hout)
    if not need_dh:
        return None
    dh = torch.empty(N, hin, dtype=_F32, device=dev)
    gemm_prop(topo, Z, Z.stride(0), wcat, pack_bwd, 1, hin, dh, relu_src=relu_src, drop=drop)
    return dh


def _tagconv_backward(topo, g, h, pack_bwd, nmat, hin, hout, g_flat, relu_src=None, dmask=None, need_dh=True,
                      rowscale2=None, defer_wgrad=False, pending=None, drop=None, b_format=0):
    """g: gradient w.r.t. the conv's pre-activation output [N, hout] (already masked).
    g_flat <- [dW_0..dW_K, db]; returns dh (masked by relu_src / dmask of the PREVIOUS layer)."""
    if not defer_wgrad:      # (deferred: the caller batches this layer's weight gradient with its siblings, wgrad_batched)
        wgrad(topo, g, hout, h, hin, nmat, g_flat, rowscale2=rowscale2, pending=pending)
    if not need_dh:
        return None
    dh = torch.empty(topo.N, hin, dtype=_F32, device=g.device)
    if is_narrow(nmat, hout) and rowscale2 is None:   # narrow gradient rows: propagate g on the input side, one stacked GEMM
        gemm_prop(topo, g, g.stride(0), nmat * hout, pack_bwd, 1, hin, dh, relu_src=relu_src, dmask=dmask,
                  transposed=True, prop_in=nmat - 1, drop=drop)
    else:
        gemm_prop(topo, g, g.stride(0), hout, pack_bwd, nmat, hin, dh, relu_src=relu_src, dmask=dmask, transposed=True,
                  drop=drop, b_format=b_format)
    return dh


# ------------------------------------------------------------------------------------------
# modules
# ------------------------------------------------------------------------------------------
class _GatherFn(torch.autograd.Function):
    """x_j = x[edge_index[0]] (by_source) / x_i = x[edge_index[1]] of PyG's propagate; the backward of a gather is the
    segmented sum over the CSR grouped by that end."""

    @staticmethod
    def forward(ctx, x, topo, by_source):
        ctx.topo, ctx.by_source, ctx.n = topo, by_source, x.size(0)
        return gather_rows(x, topo.efrom if by_source else topo.eto)

    @staticmethod
    def backward(ctx, g):
        t = ctx.topo
        rp, perm = (t.rowptrT, t.permT) if ctx.by_source else (t.rowptr, t.perm)
        return segment_sum(g.contiguous(), rp, perm, ctx.n), None, None


class _SegmentSumFn(torch.autograd.Function):
    """aggr='add': out[i] = sum of the messages of the edges whose target is i; backward = gather by target."""

    @staticmethod
    def forward(ctx, msg, topo):
        ctx.topo = topo
        return segment_sum(msg, topo.rowptr, topo.perm, topo.N)

    @staticmethod
    def backward(ctx, g):
        return gather_rows(g.contiguous(), ctx.topo.eto), None


class MessagePassing(nn.Module):
    """PyG's ``MessagePassing(aggr='add')`` base class as the reference uses it (networks.py:7,159,164,206), on the HIP
    gather / segmented-sum kernels: ``propagate(edge_index, **kwargs)`` gathers every ``foo_j`` / ``foo_i`` parameter of
    ``message()`` from ``kwargs['foo']`` at the source / target end of each edge (flow='source_to_target'), passes other
    parameters through by name, ignores keyword arguments ``message()`` does not name (which is why the ``norm`` of
    networks.py:206 is dead), sums the messages per target node (``dim_size`` = rows of the gathered tensor) and calls
    ``update()``.  Differentiable.  ``edge_index`` is used exactly as given.  ``EdgeAggregation.forward`` does not come
    through here -- it runs the fused edge-MLP kernels -- but ``EdgeAggregation.propagate`` works and gives the same
    numbers (tests), as does any user subclass with its own ``message``."""

    def __init__(self, aggr: str = "add", flow: str = "source_to_target", node_dim: int = 0):
        super().__init__()
        if aggr != "add":
            raise NotImplementedError("only aggr='add' is built")
        if flow != "source_to_target" or node_dim != 0:
            raise NotImplementedError("only flow='source_to_target', node_dim=0 are built (the reference's defaults)")
        self.aggr, self.flow, self.node_dim = aggr, flow, node_dim

    def message(self, x_j):
        return x_j

    def update(self, aggr_out):
        return aggr_out

    def propagate(self, edge_index, size=None, **kwargs):
        import inspect
        _require_gpu(edge_index)
        params = inspect.signature(self.message).parameters
        n_nodes = None if size is None else int(size if isinstance(size, int) else size[1])
        for name in params:
            if name.endswith(("_i", "_j")) and torch.is_tensor(kwargs.get(name[:-2])):
                n_nodes = int(kwargs[name[:-2]].size(0)) if n_nodes is None else n_nodes
        if n_nodes is None:
            raise ValueError("propagate: cannot infer the number of nodes (pass size= or a *_i / *_j message argument)")
        topo = get_topology_asis(edge_index, n_nodes)
        args = {}
        for name, prm in params.items():
            base = name[:-2] if name.endswith(("_i", "_j")) else None
            if base is not None and base in kwargs:
                t = kwargs[base]
                if not torch.is_tensor(t):
                    args[name] = t
                    continue
                _require_gpu(t)
                flat = t if t.dim() == 2 else t.reshape(t.size(0), -1)
                if t.is_floating_point():
                    g = _GatherFn.apply(flat, topo, name.endswith("_j"))
                else:       # index / flag tensors: plain device gather, nothing to differentiate
                    g = flat.index_select(0, (topo.efrom if name.endswith("_j") else topo.eto).long())
                args[name] = g if t.dim() == 2 else g.reshape((topo.E,) + tuple(t.shape[1:]))
            elif name in kwargs:
                args[name] = kwargs[name]
            elif prm.default is inspect.Parameter.empty and prm.kind not in (prm.VAR_KEYWORD, prm.VAR_POSITIONAL):
                raise TypeError(f"propagate: message() needs '{name}' but it was not passed")
        msg = self.message(**args)
        _require_gpu(msg)
        m2 = msg if msg.dim() == 2 else msg.reshape(msg.size(0), -1)
        if m2.size(0) != topo.E:
            raise ValueError(f"message() returned {m2.size(0)} rows for {topo.E} edges")
        out = _SegmentSumFn.apply(m2.contiguous(), topo)
        return self.update(out if msg.dim() == 2 else out.reshape((n_nodes,) + tuple(msg.shape[1:])))


class TAGConv(nn.Module):
    """PyG TAGConv(in, out, K, bias=True, normalize=True) on the fused HIP kernel.
    state_dict keys: ``bias`` (not with bias=False), ``lins.k.weight`` (k = 0..K).  bias=False runs on gnn.py's kernels
    (in == out <= 32, K <= 4); normalize=False is taken only inside gnn_dsse (ValueError standalone)."""

    def __init__(self, in_channels: int, out_channels: int, K: int = 3, bias: bool = True, normalize: bool = True):
        super().__init__()
        if K < 0:
            raise ValueError("TAGConv: K >= 0")
        # K <= 3: the fused tile GEMM + Horner kernels (templated on K + 1 <= 4 matrices); K > 3: ONE plain tile GEMM
        # X [W_0 | .. | W_K]^T and K propagation hops in global memory (the path of graphs beyond the LDS-resident tiles)
        self.in_channels, self.out_channels, self.K = in_channels, out_channels, K
        self.normalize = normalize
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_channels))
        else:
            self.register_parameter("bias", None)
        self.lins = nn.ModuleList([nn.Linear(in_channels, out_channels, bias=False) for _ in range(K + 1)])
        self._plan = None

    def _weights(self):
        return [l.weight for l in self.lins]

    def forward(self, x: torch.Tensor, edge_index: torch.Tensor) -> torch.Tensor:
        if not self.normalize:
            raise ValueError("TAGConv: normalize=False is supported only inside gnn_dsse(model='tagcn')")
        if self.bias is None:
            from .gnn import run_gnn
            return run_gnn([self], None, "none", x, x, edge_index)
        _require_gpu(x, edge_index)
        topo = get_topology_asis(edge_index, x.size(0))
        return _TAGConvFn.apply(x, topo, self, None, self.bias, *self._weights())


def _post_spec(mod, post, dev):
    """(relu, snapshot or None, p) of the 'dropout, then ReLU' that follows a layer inside a per-layer stack (``post``: None / False =
    nothing follows, True = ReLU, a rate = dropout then ReLU)."""
    if not post:
        return False, None, 0.0
    p = 0.0 if post is True else float(post)
    snap = dropout_snapshot(mod, dev) if p > 0.0 else None
    mod._last_dropout = (snap, p)
    return True, snap, p


def _gate(g: torch.Tensor, y: torch.Tensor, snap, p: float) -> torch.Tensor:
    out = torch.empty_like(y)
    g = g.contiguous()
    _lib.check(_lib.lib().dss2_gate_grad(g.data_ptr(), y.data_ptr(), out.data_ptr(), y.size(0), y.size(1),
                                         (snap.data_ptr() if snap is not None else None), 1, float(p), 1, _stream(y)),
               "dss2_gate_grad")
    return out


class _TAGConvFn(torch.autograd.Function):
    """One TAGConv as an autograd node.  ``post`` (see _post_spec): the "dropout, then ReLU" that follows it inside a Multi* stack
    or the general-width MPN loop, fused into the layer's epilogue; its gradient is one dss2_gate_grad launch."""

    @staticmethod
    def forward(ctx, x, topo, mod, post, bias, *ws):
        x = x.contiguous()
        hin, hout, nmat = mod.in_channels, mod.out_channels, mod.K + 1
        glob = use_global_path(topo, nmat)
        if mod._plan is None or mod._plan.device != x.device or mod._plan.stacked != glob:
            mod._plan = _PackPlan([list(ws)], x.device, stacked=glob)
        plan = mod._plan
        ctx.ver = plan.refresh()
        if not glob:
            topo.lds_check(nmat, _round8(hin), _ncg(hout))
        relu, snap, p = _post_spec(mod, post, x.device)
        out = (_tagconv_forward_global if glob else _tagconv_forward)(topo, x, plan.fwd[0], bias, nmat, hin, hout, relu=relu,
                                                                      drop=((snap, p, 1) if snap is not None else None))
        # (an un-gated output is not saved: gsp_wls_edge masks the model output IN PLACE, data.py:413, and a saved tensor must
        #  not change under autograd)
        ctx.save_for_backward(x, out if relu else None)
        ctx.meta = (topo, mod, relu, snap, p, glob)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, y = ctx.saved_tensors
        topo, mod, relu, snap, p, glob = ctx.meta
        plan = mod._plan
        if plan.version != ctx.ver:
            plan.refresh()
        hin, hout, nmat = mod.in_channels, mod.out_channels, mod.K + 1
        g = _gate(gout, y, snap, p) if relu else gout.contiguous()
        flat = torch.empty(nmat * hout * hin + hout, dtype=_F32, device=g.device)
        if plan.stacked != glob:
            raise RuntimeError("the module's weight layouts changed between forward and backward")
        dh = (_tagconv_backward_global if glob else _tagconv_backward)(
            topo, g, x, plan.bwd[0], nmat, hin, hout, flat, need_dh=ctx.needs_input_grad[0])
        gw = [flat[m * hout * hin:(m + 1) * hout * hin].view(hout, hin) for m in range(nmat)]
        return (dh, None, None, None, flat[nmat * hout * hin:], *gw)


def _run_tagconv(conv: TAGConv, x, topo):
    """``conv`` inside a per-layer stack (MultiMPN, MPN._forward_general), which has set ``conv._post``."""
    return _TAGConvFn.apply(x, topo, conv, conv._post, conv.bias, *conv._weights())


class EdgeAggregation(MessagePassing):
    """/root/reference/networks.py:159-209 on HIP.  ``forward`` takes the edge list AS GIVEN
    (the reference's MPN hands it the already doubled list)."""

    def __init__(self, dim_featn, dim_feate, dim_hid, dim_out):
        super().__init__(aggr="add")
        self.dim_featn, self.dim_feate, self.dim_hid, self.dim_out = dim_featn, dim_feate, dim_hid, dim_out
        self.edge_aggr = nn.Sequential(nn.Linear(dim_featn * 2 + dim_feate, dim_hid), nn.ReLU(),
                                       nn.Linear(dim_hid, dim_out))
        self._plan = None
        self._gplan, self._post = None, None      # (state of the general path, multi._EdgeAggrGeneralFn)

    def fused_dims(self) -> bool:
        """The fused edge-MLP kernels are built for the reference's data (8 node / 6 edge features, networks.py:170) and
        dim_hid <= 256; every other width runs the general path: AB = X [W1a; W1b]^T as one tile GEMM, then per edge
        relu(A[i] + B[src] + W1c ea + b1) summed per target (ops.edge_combine_fwd / _bwd), then the second Linear."""
        return self.dim_featn == 8 and self.dim_feate == 6 and self.dim_hid <= 256

    def message(self, x_i, x_j, edge_attr):
        """networks.py:176-181, the reference expression.  ``forward`` does not call it (the fused kernels evaluate the same
        arithmetic with the second Linear moved behind the aggregation); it serves ``propagate`` and subclasses."""
        return self.edge_aggr(torch.cat([x_i, x_j, edge_attr], dim=-1))

    def forward(self, x, edge_index, edge_attr):
        _require_gpu(x, edge_index, edge_attr)
        _no_edge_attr_grad(edge_attr)
        topo = get_topology_asis(edge_index, x.size(0))
        lin1, lin2 = self.edge_aggr[0], self.edge_aggr[2]
        if not self.fused_dims():
            from .multi import _EdgeAggrGeneralFn, _check_general_dims
            _check_general_dims(self)
            return _EdgeAggrGeneralFn.apply(x, edge_attr, topo, self, lin1.weight, lin1.bias, lin2.weight, lin2.bias)
        return _EdgeAggrFn.apply(x, edge_attr, topo, self, lin1.weight, lin1.bias, lin2.weight, lin2.bias)


class _EdgeAggrFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ea, topo, mod, W1, b1, W2, b2):
        x, ldx = _rows(x)
        ea, ldea = _rows(ea)
        if mod._plan is None or mod._plan.device != x.device:
            mod._plan = _PackPlan([[W2]] + _dx_views(W1, mod.dim_hid, mod.dim_featn, mod.dim_feate), x.device, stacked_groups=(3,))
        ctx.ver = mod._plan.refresh()
        topo.lds_check(1, _round8(mod.dim_hid), _ncg(mod.dim_out))
        S, x0 = _edge_aggr_forward(topo, x, ldx, ea, ldea, W1, b1, b2, mod._plan.fwd[0], mod.dim_hid, mod.dim_out,
                                   mod.dim_featn, mod.dim_feate, need_dx=ctx.needs_input_grad[0])
        ctx.save_for_backward(x, ea, S, W1, b1)
        ctx.topo, ctx.mod, ctx.ld = topo, mod, (ldx, ldea)
        return x0

    @staticmethod
    def backward(ctx, g):
        x, ea, S, W1, b1 = ctx.saved_tensors
        mod, topo = ctx.mod, ctx.topo
        if mod._plan.version != ctx.ver:
            mod._plan.refresh()
        hid, hout, fn, fe = mod.dim_hid, mod.dim_out, mod.dim_featn, mod.dim_feate
        g = g.contiguous()
        g1 = torch.empty(hid * (2 * fn + fe) + hid, dtype=_F32, device=g.device)
        g2 = torch.empty(hout * hid + hout, dtype=_F32, device=g.device)
        dx = _edge_aggr_backward(topo, g, x, ctx.ld[0], ea, ctx.ld[1], W1, b1, S, mod._plan.bwd[0], hid, hout, fn, fe,
                                 g1, g2, ctx.needs_input_grad[0], pack_dx=tuple(mod._plan.bwd[1:4]))
        nc = 2 * fn + fe
        return (dx, None, None, None, g1[:hid * nc].view(hid, nc), g1[hid * nc:], g2[:hout * hid].view(hout, hid),
                g2[hout * hid:])


def _no_edge_attr_grad(edge_attr: torch.Tensor) -> None:
    """The kernels produce gradients for the parameters and (when asked) for x, never for edge_attr (the reference's edge
    features are data: dss2_run.py:138).  Asking for one must not silently return None."""
    if edge_attr.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("the DSS2 HIP path does not differentiate with respect to edge_attr (edge features are inputs "
                                  "of the reference's training loop, dss2_run.py:138); detach() it")


def get_topology_asis(edge_index: torch.Tensor, num_nodes: int) -> Topology:
    """Topology of an edge list used exactly as given (standalone EdgeAggregation / TAGConv / propagate)."""
    return get_topology(edge_index, num_nodes, double=False)


class _FlatLayout(NamedTuple):
    offs: List[int]        # segment l of the flat buffer is [offs[l], offs[l + 1])
    sizes: List[int]       # the pieces in storage order ...
    shapes: list           # ... their matrix shapes (None: a vector) ...
    order: List[int]       # ... and the order of MPN._params() over them

    def views(self, flat: torch.Tensor) -> List[torch.Tensor]:
        """Parameter gradients as views into ``flat``, in the order of MPN._params(): one split call for all pieces."""
        parts = flat.split(self.sizes)
        return [parts[i] if self.shapes[i] is None else parts[i].view(self.shapes[i]) for i in self.order]


class MPN(nn.Module):
    """/root/reference/networks.py:212-273 on HIP (one autograd node for the whole block)."""

    skip = False

    def __init__(self, dim_featn, dim_feate, dim_out, dim_hid, n_gnn_layers, K, dropout_rate):
        super().__init__()
        self.dim_featn, self.dim_feate, self.dim_out, self.dim_hid = dim_featn, dim_feate, dim_out, dim_hid
        self.n_gnn_layers, self.K, self.dropout_rate = n_gnn_layers, K, dropout_rate
        if self.skip and dim_out != dim_featn:
            raise ValueError("SkipMPN needs dim_out == dim_featn (networks.py:336)")
        self.edge_aggr = EdgeAggregation(dim_featn, dim_feate, dim_hid, dim_hid)
        self.convs = nn.ModuleList()
        for l in range(n_gnn_layers):
            self.convs.append(TAGConv(dim_hid, dim_out if l == n_gnn_layers - 1 else dim_hid, K=K))
        self._plan = None
        self._fold = None

    # -- reference helpers kept for API parity (networks.py:236-258); not used by forward()
    def is_directed(self, edge_index):
        from .topology import reference_is_directed
        return reference_is_directed(edge_index)

    def undirect_graph(self, edge_index, edge_attr):
        if self.is_directed(edge_index):
            edge_index = torch.cat([edge_index, torch.stack([edge_index[1, :], edge_index[0, :]], dim=0)], dim=1)
            edge_attr = torch.cat([edge_attr, torch.cat([-edge_attr[:, 0:1], edge_attr[:, 1:2], -edge_attr[:, 2:3],
                                                         edge_attr[:, 3:]], dim=1)], dim=0)
        return edge_index, edge_attr

    def _params(self) -> List[torch.Tensor]:
        lin1, lin2 = self.edge_aggr.edge_aggr[0], self.edge_aggr.edge_aggr[2]
        ps = [lin1.weight, lin1.bias, lin2.weight, lin2.bias]
        for c in self.convs:
            ps.append(c.bias)
            ps.extend(l.weight for l in c.lins)
        return ps

    def _layout(self) -> "_FlatLayout":
        """The block's flat gradient buffer, described once (the dimensions are fixed at construction): segments [W1 | b1],
        [W2 | b2], [conv l: W_0 .. W_K | bias], and the pieces that become the views returned to autograd."""
        lay = self.__dict__.get("_flat_layout")
        if lay is None:
            hid, nc, nmat, L = self.dim_hid, 2 * self.dim_featn + self.dim_feate, self.K + 1, self.n_gnn_layers
            pieces = [(hid * nc, (hid, nc)), (hid, None), (hid * hid, (hid, hid)), (hid, None)]      # W1, b1, W2, b2
            order, offs = [0, 1, 2, 3], [0, hid * nc + hid, hid * nc + hid + hid * hid + hid]
            for l in range(L):
                hout = self.dim_out if l == L - 1 else hid
                base = len(pieces)
                pieces += [(hout * hid, (hout, hid))] * nmat + [(hout, None)]                       # stored [W_0..W_K | bias]
                order += [base + nmat] + list(range(base, base + nmat))                              # _params(): bias first
                offs.append(offs[-1] + nmat * hout * hid + hout)
            lay = self.__dict__["_flat_layout"] = _FlatLayout(offs, [sz for sz, _ in pieces], [sh for _, sh in pieces], order)
        return lay

    def _flat_offsets(self):
        """Element offsets of the segments of the flat gradient buffer (a list of ints)."""
        return self._layout().offs

    def _conv_params(self, ps):
        """``ps`` (the order of _params()) -> per conv (bias, W_0 .. W_K)."""
        n = self.K + 2
        return [ps[4 + l * n: 4 + (l + 1) * n] for l in range(self.n_gnn_layers)]

    def forward(self, x, edge_index, edge_attr):
        _require_gpu(x, edge_index, edge_attr)
        _no_edge_attr_grad(edge_attr)
        topo = get_topology(edge_index, x.size(0))
        if not self.edge_aggr.fused_dims():
            return self._forward_general(x, edge_attr, topo)
        from . import stack as _stack
        dims = _stack.route(self, [self], topo)
        if dims is not None:          # dim_hid 32, K 2: the whole-stack kernels (one launch forward, one backward)
            return _stack.run(self, [self], dims, topo, x, edge_attr)
        return _MPNFn.apply(x, edge_attr, topo, self, *self._params())

    def _forward_general(self, x, edge_attr, topo):
        """networks.py:260-273 for input widths other than (8, 6) (or dim_hid > 256): the same layer loop out of the
        per-layer autograd nodes of multi.py -- general edge aggregation, TAGConv with the fused "dropout, then ReLU"
        epilogue -- instead of the fused block.  Correct for every width the kernels take; not the tuned path."""
        from .multi import _EdgeAggrGeneralFn, _check_general_dims
        ea_mod = self.edge_aggr
        _check_general_dims(ea_mod)
        lin1, lin2 = ea_mod.edge_aggr[0], ea_mod.edge_aggr[2]
        ea_mod._post = None
        h = _EdgeAggrGeneralFn.apply(x, edge_attr, topo, ea_mod, lin1.weight, lin1.bias, lin2.weight, lin2.bias)
        last = len(self.convs) - 1
        for i, conv in enumerate(self.convs):
            conv._post = None if i == last else (float(self.dropout_rate) if self.dropout_rate > 0 else True)
            h = _run_tagconv(conv, h, topo)
        return x + h if self.skip else h


class SkipMPN(MPN):
    """/root/reference/networks.py:275-338: MPN + ``input_x + x``."""

    skip = True


def _ensure_plans(mod, topo, dev, ps, rt: BlockRoute):
    """(pack plan, fold plan or None) of an MPN block in the weight space of route ``rt``, created on first use / when that changes."""
    L, nmat, hid = mod.n_gnn_layers, mod.K + 1, mod.dim_hid
    W1, b1, W2, b2 = ps[0:4]
    conv_ps = mod._conv_params(ps)
    if (mod._plan is None or mod._plan.device != dev or not _plans_match(mod, rt)):
        offs = mod._flat_offsets()
        mod._fold = _FoldPlan(W2, b2, conv_ps[0][1:], dev, int(offs[1]), int(offs[2])) if rt.fold else None
        conv_groups = [list(cp[1:]) for cp in conv_ps]
        if rt.fold:   # conv 0 is packed from the folded weights
            conv_groups[0] = [_MatView(mod._fold.Wf[m], conv_ps[0][1].shape[0], hid, hid, 0, dep=True) for m in range(nmat)]
        mod._plan = _PackPlan([[W2]] + conv_groups + _dx_views(W1, hid, mod.dim_featn, mod.dim_feate), dev, stacked=rt.glob,
                              stacked_groups=(L + 3,), bf16_groups=rt.b16, f16=rt.f16)
    if mod._fold is not None:
        mod._fold.params = (W2, b2, list(conv_ps[0][1:]))
    return mod._plan, mod._fold


def _plans_match(mod, rt: BlockRoute) -> bool:
    """The module's plans are those of route ``rt`` (a forward on another topology or under other flags rebuilds them)."""
    plan = mod._plan
    return ((mod._fold is not None) == rt.fold and plan.stacked == rt.glob and tuple(sorted(plan.fwd16)) == rt.b16
            and plan.f16 == rt.f16)


class _BlockMeta(NamedTuple):
    """What one forward call of a block hands to its backward besides the saved tensors."""
    route: BlockRoute
    ldx: int
    ldea: int
    n_acts: int
    drop: tuple          # (snapshot or None, p, first mask id of the block)
    ver: int             # version of the pack plan the forward ran on
    act_bits: dict       # index into the activations -> sign-bit words of that activation (route.gw > 0)


def _mpn_forward(mod, topo, x, ea, ps, stack=None, need_dx=False):
    """One MPN block forward on raw tensors.  ``stack`` (a _StackRun, PFN / SkipPFN): the routes were computed and the weight
    packing, the fold and the dropout snapshot done for all blocks of the stack, in one launch each.
    Returns (out, tensors to keep for backward, _BlockMeta)."""
    x, ldx = _rows(x)
    ea, ldea = _rows(ea)
    dev = x.device
    L, nmat, hid = mod.n_gnn_layers, mod.K + 1, mod.dim_hid
    W1, b1, W2, b2 = ps[0:4]
    conv_ps = mod._conv_params(ps)   # (bias, W_0..W_K)
    rt = block_route(mod, topo, need_dx, False) if stack is None else stack.route_of(mod)
    ntiles = topo.tiling.ntiles
    plan, fold = _ensure_plans(mod, topo, dev, ps, rt)
    if stack is None:
        ver = plan.refresh(fold)      # (fold + packing: one launch)
    else:
        ver = plan.version
    if not rt.glob:
        topo.lds_check(nmat, _round8(hid), _ncg(hid))
    if rt.edge:      # the forward chain computes S itself and writes it for the backward
        S = h = torch.empty(topo.N, hid, dtype=_F32, device=dev)
    else:
        S, h = _edge_aggr_forward(topo, x, ldx, ea, ldea, W1, b1, b2, plan.fwd[0], hid, hid, mod.dim_featn, mod.dim_feate,
                                  second_linear=fold is None, need_dx=need_dx)
    if fold is not None:
        h = S            # conv 0 consumes the aggregated hidden directly
    acts = [h]
    act_bits = {}
    p = float(mod.dropout_rate)
    # dropout is active regardless of .training (a fresh nn.Dropout is built inside forward, networks.py:268).  The
    # masks are not tensors: the epilogues regenerate them from (snapshot, layer id) in forward and backward.
    if p <= 0.0:
        snap, base = None, 0
    elif stack is not None:
        snap, base = stack.snapshot, stack.drop_base(mod)
    else:
        snap, base = dropout_snapshot(mod, dev), 0
    mod._last_dropout, mod._drop_base = (snap, p), base

    def drop_id(l):            # mask applied to conv l's output (none after the last conv)
        return base + l + 1 if (snap is not None and l < L - 1) else 0

    first = rt.n_chain         # first layer with a launch of its own
    if rt.n_chain:
        # the hid -> hid layers 0 .. L-2 as ONE chained launch (activation tile stays in LDS between layers)
        layers = []
        # the chain also writes the sign bits of its outputs; the data-gradient chain reads those instead of the
        # activations for its ReLU gates (dss2_chain_layer.y_bits / gate_bits)
        for l in range(rt.n_chain):
            out_l = torch.empty(topo.N, hid, dtype=_F32, device=dev)
            layers.append(dict(Bp=(plan.fwd16[1 + l] if rt.use16 else plan.fwd[1 + l]), Y=out_l, bias=conv_ps[l][0], relu=True,
                               drop_id=drop_id(l), prebias=(fold.bf if (fold is not None and l == 0) else None)))
            if rt.gw:      # (inside autograd.Function.forward grad mode is off: always written; 1/32 of a layer output)
                act_bits[len(acts)] = layers[-1]["y_bits"] = torch.empty(ntiles * rt.gw, dtype=torch.int64, device=dev)
            acts.append(out_l)
        h, head = acts[-1], None
        if rt.head:      # the narrow last layer inside the same launch (the tile is still in the waves' registers)
            h, first = torch.empty(topo.N, mod.dim_out, dtype=_F32, device=dev), L
            head = dict(W=list(conv_ps[L - 1][1:1 + nmat]), nout=mod.dim_out, Y=h, bias=conv_ps[L - 1][0],
                        add_src=(x if mod.skip else None), add_ld=ldx)
            if rt.edge:
                head["edge"] = dict(x=x, ldx=ldx, ea=ea, ldea=ldea, W1=W1, b1=b1, S=S)
        gemm_prop_chain(topo, acts[0], hid, nmat, layers, pre_rowscale=(topo.deg_pows if fold is not None else None),
                        drop=((snap, p) if snap is not None else None), b_format=(2 if (rt.use16 and rt.f16) else int(rt.use16)), head=head)
    for l in range(first, L):
        last = l == L - 1
        hout = mod.dim_out if last else hid
        kw = dict(relu=not last, add_src=(x if (last and mod.skip) else None), add_ld=ldx,
                  drop=((snap, p, drop_id(l)) if snap is not None else None))
        if rt.glob:
            h = _tagconv_forward_global(topo, h, plan.fwd[1 + l], conv_ps[l][0], nmat, hid, hout, **kw)
        else:
            pre = (fold.bf, topo.deg_pows) if (fold is not None and l == 0) else (None, None)
            g16 = rt.g16[l]      # tall tiles: bf16x6 per layer
            h = _tagconv_forward(topo, h, (plan.fwd16[1 + l] if g16 else plan.fwd[1 + l]), conv_ps[l][0], nmat, hid, hout,
                                 prebias=pre[0], pre_rowscale=pre[1], b_format=int(g16), **kw)
        if not last:
            acts.append(h)
    return h, [x, ea, S] + acts, _BlockMeta(rt, ldx, ldea, len(acts), (snap, p, base), ver, act_bits)


class _BlockBackward(NamedTuple):
    """The state the sections of one block's backward share."""
    mod: nn.Module
    topo: Topology
    rt: BlockRoute
    meta: _BlockMeta
    plan: _PackPlan
    fold: Optional[_FoldPlan]
    S: torch.Tensor
    acts: list
    ps: Sequence[torch.Tensor]
    flat: torch.Tensor
    offs: List[int]
    pending: Optional[list]

    def seg(self, l: int, l1: Optional[int] = None) -> torch.Tensor:
        """Conv l's segment [W_0..W_K | bias] of the flat buffer (through conv l1's)."""
        return self.flat[self.offs[2 + l]:self.offs[3 + (l if l1 is None else l1)]]

    def drop_of(self, l: int):
        """The mask that was applied to conv l's output: (snapshot, p, id) or None."""
        snap, p, base = self.meta.drop
        return (snap, p, base + l + 1) if (snap is not None and l >= 0) else None


def _mpn_backward(mod, topo, saved, ps, meta, gout, need_dx, flat=None, pending=None):
    """Backward of _mpn_forward along the route the forward stored in ``meta``.  Standalone (flat is None): allocates the block's
    flat gradient buffer, runs its slab reductions and the fold's chain rule, calls the all-reduce hook.  Inside a stack: ``flat``
    is the block's slice of the stack's buffer and every slab reduction is only recorded in ``pending``; the caller runs them
    (and the chain rule of all folds) in one launch each after the last block.  Returns (dx, parameter gradients as views into
    flat, whether the fold's chain rule is due)."""
    rt = meta.route
    x, ea, S = saved[0:3]
    standalone = flat is None
    plan, fold = mod._plan, mod._fold
    if not _plans_match(mod, rt):      # (another forward, on another topology or under other flags, rebuilt them in between)
        raise RuntimeError("DSS2_FOLD_W2 / the module's plan changed between forward and backward")
    if plan.version != meta.ver:
        plan.refresh(fold)   # weights are checked unchanged by autograd's saved-tensor versioning
    # one flat gradient buffer; parameter gradients are returned as views into it
    lay = mod._layout()
    if standalone:
        flat = torch.empty(lay.offs[-1], dtype=_F32, device=gout.device)
    if rt.bwd_chain and pending is None:
        pending = []         # the chained route's slab reductions run in ONE launch at the end (always so inside a stack)
    c = _BlockBackward(mod, topo, rt, meta, plan, fold, S, list(saved[3:3 + meta.n_acts]), ps, flat, lay.offs, pending)
    g = gout.contiguous()
    edge = dict(x=x, ldx=meta.ldx, ea=ea, ldea=meta.ldea, W1=ps[0], b1=ps[1])
    d_in, deferred = _bwd_chained(c, g, edge) if rt.bwd_chain else _bwd_layers(c, g)
    _bwd_deferred_wgrads(c, deferred)
    dx = None
    if not rt.bwd_edge:      # (else done inside the data-gradient chain; no input gradient asked for)
        fn, fe, L, hid = mod.dim_featn, mod.dim_feate, mod.n_gnn_layers, mod.dim_hid
        dx = _edge_aggr_backward(topo, (None if rt.fold else d_in), x, meta.ldx, ea, meta.ldea, ps[0], ps[1], S, plan.bwd[0], hid, hid,
                                 fn, fe, flat[lay.offs[0]:lay.offs[1]], flat[lay.offs[1]:lay.offs[2]], need_dx,
                                 pack_dx=tuple(plan.bwd[1 + L:4 + L]), dS=(d_in if rt.fold else None),
                                 pending=pending, dx_add=(gout if (need_dx and mod.skip) else None))
    if standalone:
        # all slab reductions of the block in one launch, then the chain rule of the fold (it needs the reduced gfold)
        if rt.fold:
            fold._check()
        finish_weights(pending if pending is not None else [], (fold.bwd_tab if rt.fold else None), flat, gout.device)
        hook = getattr(mod, "_grad_bucket_hook", None)
        if hook is not None:      # data-parallel: all-reduce the flat bucket once (parallel.py)
            hook(flat)
    return dx, lay.views(flat), rt.fold


def _bwd_chained(c: _BlockBackward, g, edge):
    """The last layer, then the data gradients of layers L-2 .. 0 as ONE chained launch; with the route's fused forms the head's
    data and weight gradients and the edge MLP's backward (``edge``: its inputs) ride in that launch.  Returns (gradient w.r.t.
    conv 0's input -- dS when folded --, the layers (l, gradient, input) whose weight gradients are still due)."""
    mod, topo, rt, plan, acts, pending = c.mod, c.topo, c.rt, c.plan, c.acts, c.pending
    L, nmat, hid, nout = mod.n_gnn_layers, mod.K + 1, mod.dim_hid, mod.dim_out
    dev, ntiles = g.device, topo.tiling.ntiles
    snap, p_drop, base = c.meta.drop
    l = L - 1
    head = head_wg = edge_slab = None
    if rt.bwd_head:
        # the head's input tile is computed from the dim_out-wide upstream gradient (dss2_gemm_prop_chain_head, mode 2) ...
        if rt.bwd_head_wgrad:
            # ... and its weight gradient from the same staging (it holds the hop results and the head's input rows): one slab
            # per tile, summed with the step's other slabs
            hw_len = nmat * nout * hid + nout
            hw_stride = (hw_len + 3) & ~3      # (16-byte lanes in the reduction)
            head_wg = torch.empty(ntiles * hw_stride, dtype=_F32, device=dev)
        else:      # the narrow weight-gradient launch re-reads the activation
            _tagconv_backward(topo, g, acts[l], plan.bwd[1 + l], nmat, hid, nout, c.seg(l), need_dh=False, pending=pending)
        dr = c.drop_of(l - 1)
        head = dict(W=list(c.ps[4 + l * (nmat + 1) + 1:4 + (l + 1) * (nmat + 1)]), nout=nout, G=g, gate=acts[l],
                    Xout=torch.empty(topo.N, hid, dtype=_F32, device=dev), drop_id=(dr[2] if dr is not None else 0),
                    wg_slab=head_wg, wg_stride=(hw_stride if head_wg is not None else 0))
        if rt.bwd_edge:
            # conv 0's input gradient never leaves the chip: one dW1 | db1 slab per tile
            e_stride = c.offs[1] - c.offs[0]
            edge_slab = torch.empty(ntiles * e_stride, dtype=_F32, device=dev)
            head["edge"] = dict(edge, slab=edge_slab)
        g_top = head["Xout"]
    else:
        g_top = _tagconv_backward(topo, g, acts[l], plan.bwd[1 + l], nmat, hid, nout, c.seg(l),
                                  relu_src=acts[l], drop=c.drop_of(l - 1), pending=pending)
    gl = [None] * (L - 1)                   # gl[l]: gradient w.r.t. layer l's pre-activation output
    gl[L - 2] = g_top
    layers = []
    for l in range(L - 2, -1, -1):
        out_l = torch.empty(topo.N, hid, dtype=_F32, device=dev)
        layers.append(dict(Bp=(plan.bwd16[1 + l] if rt.bwd_use16 else plan.bwd[1 + l]), Y=out_l, relu_src=(acts[l] if l > 0 else None),
                           gate_bits=(c.meta.act_bits.get(l) if (l > 0 and rt.bwd_use16) else None),
                           drop_id=(base + l if (l > 0 and snap is not None) else 0)))      # mask of conv l-1: id (l-1)+1
        if l > 0:
            gl[l - 1] = out_l
    gemm_prop_chain(topo, (None if rt.bwd_head else g_top), hid, nmat, layers, transposed=True,
                    drop=((snap, p_drop) if snap is not None else None), b_format=(2 if (rt.bwd_use16 and rt.f16) else int(rt.bwd_use16)),
                    head=head)
    if head_wg is not None:
        _reduce(head_wg, 0, ntiles, hw_stride, c.seg(L - 1), hw_len, pending)
    if edge_slab is not None:
        _reduce(edge_slab, 0, ntiles, e_stride, c.flat[c.offs[0]:c.offs[1]], e_stride, pending)
    if rt.bwd_join:
        # the folded conv 0 (input S, extra scaled bias sums) and the plain layers 1 .. L-2 in ONE launch
        wgrad_batched(topo, gl, hid, [c.S] + acts[1:L - 1], hid, nmat, c.seg(1, L - 2),
                      first_rowscale2=topo.deg_pows, first_out=c.fold.gfold, pending=pending)
    elif rt.fold:
        wgrad(topo, gl[0], hid, c.S, hid, nmat, c.fold.gfold, rowscale2=topo.deg_pows, pending=pending)
    return layers[-1]["Y"], [(l, gl[l], acts[l]) for l in range(L - 1) if rt.bwd_defer[l]]


def _bwd_layers(c: _BlockBackward, g):
    """Layers L-1 .. 0 one launch each.  Returns as _bwd_chained."""
    mod, topo, rt, plan, acts, pending = c.mod, c.topo, c.rt, c.plan, c.acts, c.pending
    L, nmat, hid = mod.n_gnn_layers, mod.K + 1, mod.dim_hid
    deferred = []
    for l in range(L - 1, -1, -1):
        hout = mod.dim_out if l == L - 1 else hid
        g16 = rt.bwd_g16[l]
        Bp = plan.bwd16[1 + l] if g16 else plan.bwd[1 + l]
        # the data gradient's epilogue applies the ReLU / dropout mask of the layer BELOW (its output is acts[l])
        below = dict(relu_src=(acts[l] if l > 0 else None), drop=c.drop_of(l - 1))
        if l == 0 and rt.fold:
            # folded conv 0: weight gradient w.r.t. Wf / bf into the plan's buffer, data gradient is dS;
            # one small-GEMM launch then writes dW_m, conv0.bias, dW2, db2 into the flat buffer
            wgrad(topo, g, hout, c.S, hid, nmat, c.fold.gfold, rowscale2=topo.deg_pows, pending=pending)
            dS = torch.empty(topo.N, hid, dtype=_F32, device=g.device)
            gemm_prop(topo, g, g.stride(0), hout, Bp, nmat, hid, dS, transposed=True, b_format=int(g16))
            g = dS
        elif rt.glob:
            g = _tagconv_backward_global(topo, g, acts[l], Bp, nmat, hid, hout, c.seg(l), pending=pending, **below)
        else:
            if rt.bwd_defer[l]:
                deferred.append((l, g, acts[l]))
            g = _tagconv_backward(topo, g, acts[l], Bp, nmat, hid, hout, c.seg(l), defer_wgrad=rt.bwd_defer[l], pending=pending,
                                  b_format=int(g16), **below)
    return g, deferred[::-1]


def _bwd_deferred_wgrads(c: _BlockBackward, deferred):
    """Weight gradients of the hid -> hid layers ``deferred`` (ascending): independent of each other, so one launch (and one slab
    reduction) covers up to 8 consecutive layers; their segments in the flat buffer are contiguous."""
    hid, nmat = c.mod.dim_hid, c.mod.K + 1
    for c0 in range(0, len(deferred), 8):
        chunk = deferred[c0:c0 + 8]
        out = c.seg(chunk[0][0], chunk[-1][0])
        if len(chunk) == 1:
            wgrad(c.topo, chunk[0][1], hid, chunk[0][2], hid, nmat, out, pending=c.pending)
        else:
            wgrad_batched(c.topo, [t[1] for t in chunk], hid, [t[2] for t in chunk], hid, nmat, out, pending=c.pending)


class _MPNFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ea, topo, mod, *ps):
        out, saved, meta = _mpn_forward(mod, topo, x, ea, ps, need_dx=ctx.needs_input_grad[0])
        ctx.save_for_backward(*saved, *ps)
        ctx.meta = (topo, mod, meta, len(saved))
        return out

    @staticmethod
    def backward(ctx, gout):
        topo, mod, meta, n_saved = ctx.meta
        saved = ctx.saved_tensors
        dx, grads, _ = _mpn_backward(mod, topo, saved[:n_saved], saved[n_saved:], meta, gout, ctx.needs_input_grad[0])
        return (dx, None, None, None, *grads)


class _StackPlan:
    """What the blocks of a PFN / SkipPFN stack share per step: ONE small-GEMM launch folding every block's second Linear,
    ONE pack launch for every block's weights, ONE dropout snapshot (layer ids offset per block), ONE flat gradient buffer
    (block b at base[b]), ONE slab-reduction launch and ONE chain-rule launch for all folds.  The merged descriptor tables
    are rebuilt only when a parameter or plan buffer moves."""

    DROP_STRIDE = 64      # dropout mask ids of block b: b * DROP_STRIDE + layer + 1

    def __init__(self, blocks, device):
        self.blocks, self.device = list(blocks), device
        sizes = [int(m._flat_offsets()[-1]) for m in self.blocks]
        self.base = [0]
        for s in sizes:
            self.base.append(self.base[-1] + s)
        self.total = self.base[-1]
        self.key = None
        self.fold_fwd = self.fold_bwd = self.pack_tab = None
        self.table_builds = 0

    def refresh(self, topo, params, routes):
        plans = [_ensure_plans(m, topo, self.device, ps, rt) for m, ps, rt in zip(self.blocks, params, routes)]
        key = tuple((id(p), id(f), p.pointers(), f.pointers() if f is not None else None) for p, f in plans)
        if key != self.key:
            fwd, bwd, recs, max_elems = [], [], [], 0
            for b, (p, f) in enumerate(plans):
                if f is not None:
                    f_, b_ = f.records(self.base[b])
                    fwd += f_
                    bwd += b_
                recs += p.records()
                max_elems = max(max_elems, p.max_elems)
            self.fold_fwd = _sg_table(fwd, self.device) if fwd else None
            self.fold_bwd = _sg_table(bwd, self.device) if bwd else None
            t, cnt, n_dep = _pack_table(recs, self.device)
            self.pack_tab = (t, cnt, max_elems, n_dep)
            self.key = key
            self.table_builds += 1
        prep_weights(self.fold_fwd, self.pack_tab, self.device)      # every block's fold, then every block's packing: one launch each
        for p, _ in plans:
            p.version += 1


class _StackRun:
    """Per-forward state of a stack (what one call's blocks and its backward share)."""

    def __init__(self, plan: _StackPlan, snapshot, routes):
        self.plan, self.snapshot, self.routes = plan, snapshot, routes

    def route_of(self, mod) -> BlockRoute:
        return self.routes[self.plan.blocks.index(mod)]

    def drop_base(self, mod) -> int:
        return self.plan.blocks.index(mod) * _StackPlan.DROP_STRIDE


class _PFNFn(torch.autograd.Function):
    """All blocks of a PFN / SkipPFN as ONE autograd node: the per-block housekeeping launches (fold, pack, dropout state,
    slab reductions, chain rule of the folds, gradient all-reduce) run once per stack, and every gradient of the stack is
    complete when the node returns -- with blocking collectives.  (parallel.attach_grad_allreduce(async_op=True) returns views of
    a bucket whose all-reduce is still in flight: sound only while every .grad is None, so its hook falls back to the blocking
    collective when gradients are already in place.)"""

    @staticmethod
    def forward(ctx, x, ea, topo, pfn, n_per_block, *ps):
        blocks = list(pfn.mpns)
        dev = x.device
        bounds = np.concatenate([[0], np.cumsum(n_per_block)])
        params = [ps[bounds[b]:bounds[b + 1]] for b in range(len(blocks))]
        sp = pfn._stack_plan
        if sp is None or sp.device != dev:
            sp = pfn._stack_plan = _StackPlan(blocks, dev)
        need_dx = [bi > 0 or ctx.needs_input_grad[0] for bi in range(len(blocks))]
        routes = [block_route(m, topo, nd, True) for m, nd in zip(blocks, need_dx)]
        sp.refresh(topo, params, routes)
        snap = dropout_snapshot(pfn, dev) if float(pfn.dropout_rate) > 0.0 else None
        run = _StackRun(sp, snap, routes)
        saved, metas, counts = [], [], []
        for bi, (m, bp) in enumerate(zip(blocks, params)):
            x, sv, meta = _mpn_forward(m, topo, x, ea, bp, stack=run, need_dx=need_dx[bi])
            saved += sv
            metas.append(meta)
            counts.append(len(sv))
        ctx.save_for_backward(*saved, *ps)
        ctx.meta = (topo, pfn, metas, counts, bounds)
        return x

    @staticmethod
    def backward(ctx, gout):
        topo, pfn, metas, counts, bounds = ctx.meta
        blocks = list(pfn.mpns)
        sp = pfn._stack_plan
        st = ctx.saved_tensors
        n_saved = sum(counts)
        saved, ps = st[:n_saved], st[n_saved:]
        dev = gout.device
        flat = torch.empty(sp.total, dtype=_F32, device=dev)
        pending, grads_all, any_fold = [], [None] * len(blocks), False
        sbounds = np.concatenate([[0], np.cumsum(counts)])
        g = gout
        for b in range(len(blocks) - 1, -1, -1):
            m = blocks[b]
            need_dx = b > 0 or ctx.needs_input_grad[0]
            g, grads_all[b], fl = _mpn_backward(m, topo, saved[sbounds[b]:sbounds[b + 1]], ps[bounds[b]:bounds[b + 1]], metas[b],
                                                g, need_dx, flat=flat[sp.base[b]:sp.base[b + 1]],
                                                pending=pending)
            any_fold = any_fold or fl
        if any_fold and sp.fold_bwd is None:
            raise RuntimeError("the stack's fold tables are missing")
        finish_weights(pending, (sp.fold_bwd if any_fold else None), flat, dev)
        hook = getattr(blocks[0], "_grad_bucket_hook", None)
        if hook is not None:      # data-parallel: ONE all-reduce for the whole stack's bucket
            hook(flat)
        return (g, None, None, None, None, *[t_ for gr in grads_all for t_ in gr])


class PFN(nn.Module):
    """/root/reference/networks.py:340-363: L chained MPN blocks on the same edge inputs."""

    inner = MPN

    def __init__(self, dim_featn, dim_feate, dim_out, dim_hid, n_gnn_layers, K, dropout_rate, L):
        super().__init__()
        self.dim_featn, self.dim_feate, self.dim_out, self.dim_hid = dim_featn, dim_feate, dim_out, dim_hid
        self.n_gnn_layers, self.K, self.dropout_rate, self.L = n_gnn_layers, K, dropout_rate, L
        self.mpns = nn.ModuleList()
        for l in range(L):
            if l == L - 1:
                self.mpns.append(MPN(dim_featn, dim_feate, dim_out, dim_hid, n_gnn_layers, K, dropout_rate))
            else:
                self.mpns.append(self.inner(dim_featn, dim_feate, dim_featn, dim_hid, n_gnn_layers, K, dropout_rate))
        self._stack_plan = None

    def forward(self, x, edge_index, edge_attr):
        _require_gpu(x, edge_index, edge_attr)
        _no_edge_attr_grad(edge_attr)
        if not FL.STACK_NODE or self.n_gnn_layers + 1 >= _StackPlan.DROP_STRIDE or not self.mpns[0].edge_aggr.fused_dims():
            for m in self.mpns:
                x = m(x, edge_index, edge_attr)
            return x
        topo = get_topology(edge_index, x.size(0))
        from . import stack as _stack
        blocks = list(self.mpns)
        dims = _stack.route(self, blocks, topo)
        if dims is not None:          # the reference driver's own model line: ONE launch for all blocks of the stack
            return _stack.run(self, blocks, dims, topo, x, edge_attr)
        params = [m._params() for m in self.mpns]
        return _PFNFn.apply(x, edge_attr, topo, self, tuple(len(p) for p in params), *[t_ for p in params for t_ in p])


class SkipPFN(PFN):
    """/root/reference/networks.py:365-388: SkipMPN blocks, last one a plain MPN."""

    inner = SkipMPN


# the reference driver's default model (networks.py:113-156), defined in gat.py on its own kernels
from .gat import GATv2Conv, GAT_DSSE  # noqa: E402,F401
# the reference's GIN model (networks.py:71-111), defined in gine.py on its own kernels
from .gine import GINEConv, GINE_DSSE  # noqa: E402,F401
# the reference's GCN2 / FA / TAG model (networks.py:11-69), defined in gnn.py on its own kernels
from .gnn import GCN2Conv, FAConv, gnn_dsse  # noqa: E402,F401
# the reference's parallel-ChebConv model (networks.py:737-835), defined in cheb.py on its own kernels
from .cheb import ChebConv, WrappedMultiConv, MultiConvNet  # noqa: E402,F401
