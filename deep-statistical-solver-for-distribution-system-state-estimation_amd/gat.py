"""GATv2 and the reference's default model, ``GAT_DSSE`` (/root/reference/networks.py:113-156), on the HIP kernels of
csrc/dss2_gat.hip.

    GATv2Conv(in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0, add_self_loops=True,
              edge_dim=None, fill_value='mean', bias=True, share_weights=False)     PyG's layer, same parameter names
    GAT_DSSE(dim_feat, dim_dense, dim_out, num_layers, edge_dim, heads=1, concat=True, slope=0.2, self_loops=True,
             dropout=0., nonlin='leaky_relu', model='gat')                          the reference's signature and attributes

``GAT_DSSE.model`` is a look-alike of PyG's ``Sequential`` (``lanegroup.Sequential``) with children ``module_{i}``: conv k is
``module_{2k}``, the shared nonlinearity sits at every ``module_{2k+1}``, the two Linears follow; so the ``state_dict`` keys are
the reference's.  Its forward is ONE autograd node (``_GATFn``) on the launch schedule of lanegroup.py: one launch per conv
forward (the head Linears fused into the last one), per layer one fused backward launch (source pass of layer l + target pass of
layer l - 1), one batched weight-gradient launch and one slab reduction.  Every launch goes through the library, so the step
records into launch plans and hipGraphs.

The semantics are PyG 2.3-2.6's ``GATv2Conv`` / ``softmax`` / ``add_self_loops`` / ``Sequential`` (torch_geometric is not a
dependency; they are pinned by tests/golden/gat_known_answers.json and the fp64 restatements tests/gat_oracle.py and
tests/gat_heads_oracle.py).

Heads.  ``GATv2Conv(heads=H)`` with ``concat=True`` (output ``[N, H * C]``) or ``concat=False`` (the mean over the heads,
``[N, C]``, the bias added after it).  A lane of the kernels' lane group is (head h, channel c) at ``h * Cp + c`` with ``Cp`` the
per-head channels ``C`` rounded up to a power of two, so the supported range is ``H * Cp <= 32`` (and ``in_channels <= 32``): 1 to
4 heads at the driver's 8 channels.  ``GAT_DSSE(heads > 1)`` with convs needs ``concat=False``: every conv maps ``channels ->
channels`` and the first Linear takes ``dim_hidden = channels`` columns, so a concatenated output of ``heads * channels`` columns
fits neither (the reference fails with a shape error in ``forward``); it is refused at construction with a ``ValueError``.

Not provided (ValueError): ``heads * Cp > 32``, attention dropout > 0, fill_value other than 'mean', bipartite (tuple) inputs,
return_attention_weights.  No gradient with respect to edge_attr; no CPU path.
"""
from __future__ import annotations

import functools
import math
from typing import List, Optional

import torch
import torch.nn as nn

from . import _lib, lanegroup
from .lanegroup import MAX_CHANNELS, MAX_DENSE, MAX_EDGE_DIM
from .lanegroup import glorot as _glorot
from .ops import _ptr, _require_gpu, _rows
from .topology import get_topology

_F32 = torch.float32


def _fan_in_uniform(t: torch.Tensor, fan_in: int) -> None:
    b = 1.0 / math.sqrt(fan_in) if fan_in > 0 else 0.0
    with torch.no_grad():
        t.uniform_(-b, b)


_check_width = functools.partial(lanegroup.check_width, "GAT")


def lane_channels(out_channels: int, heads: int) -> int:
    """The lanes one conv's output side takes in the lane group: C with one head, H * Cp (Cp = C rounded up to a power of two)
    with several."""
    if heads == 1:
        return out_channels
    return heads * (1 << (out_channels - 1).bit_length())


class GATv2Conv(nn.Module):
    """PyG ``GATv2Conv`` on the HIP kernels.  ``state_dict`` keys, with H heads of C channels: ``att [1, H, C]``, ``bias [H * C]``
    (``[C]`` with ``concat=False``), ``lin_l.{weight [H * C, in], bias}``, ``lin_r.{weight, bias}`` (the same module as lin_l with
    share_weights), ``lin_edge.weight [H * C, edge_dim]`` (with edge_dim); rows ``h * C .. h * C + C - 1`` belong to head h.  Edges
    are used as given (not doubled); with add_self_loops the input's self loops are dropped and one per node is added with the
    mean of its incoming edges' attributes (0 without any)."""

    def __init__(self, in_channels, out_channels: int, heads: int = 1, concat: bool = True, negative_slope: float = 0.2,
                 dropout: float = 0.0, add_self_loops: bool = True, edge_dim: Optional[int] = None, fill_value="mean",
                 bias: bool = True, share_weights: bool = False, **kwargs):
        super().__init__()
        if isinstance(in_channels, (tuple, list)):
            raise ValueError("GATv2Conv: bipartite (tuple) in_channels are not supported")
        if not isinstance(heads, int) or isinstance(heads, bool) or heads < 1:
            raise ValueError(f"GATv2Conv: heads = {heads!r}; a positive integer")
        if dropout > 0:
            raise ValueError(f"GATv2Conv: attention dropout = {dropout}; only dropout = 0 is supported")
        if not (isinstance(fill_value, str) and fill_value == "mean"):
            raise ValueError(f"GATv2Conv: fill_value = {fill_value!r}; only 'mean' is supported")
        _check_width("in_channels", in_channels, MAX_CHANNELS)
        _check_width("out_channels", out_channels, MAX_CHANNELS)
        if edge_dim is not None:
            _check_width("edge_dim", edge_dim, MAX_EDGE_DIM)
        if lane_channels(out_channels, heads) > MAX_CHANNELS:
            raise ValueError(f"GATv2Conv: heads = {heads} of out_channels = {out_channels} take {lane_channels(out_channels, heads)} "
                             f"lanes (heads * out_channels rounded up to a power of two); the GAT kernels have {MAX_CHANNELS}")
        concat = bool(concat)
        self.in_channels, self.out_channels, self.heads, self.concat = in_channels, out_channels, heads, concat
        self.negative_slope, self.dropout, self.add_self_loops = float(negative_slope), float(dropout), bool(add_self_loops)
        self.edge_dim, self.fill_value, self.share_weights = edge_dim, fill_value, bool(share_weights)
        self.att = nn.Parameter(torch.empty(1, heads, out_channels))
        if bias:
            self.bias = nn.Parameter(torch.empty(heads * out_channels if concat else out_channels))
        else:
            self.register_parameter("bias", None)
        self.lin_l = nn.Linear(in_channels, heads * out_channels, bias=bias)
        self.lin_r = self.lin_l if share_weights else nn.Linear(in_channels, heads * out_channels, bias=bias)
        self.lin_edge = nn.Linear(edge_dim, heads * out_channels, bias=False) if edge_dim is not None else None
        self.reset_parameters()

    def reset_parameters(self) -> None:
        """GATv2Conv.reset_parameters: glorot weights and att, Linear biases U(+-1/sqrt(in)), conv bias zeros."""
        for lin in ([self.lin_l] if self.share_weights else [self.lin_l, self.lin_r]):
            _glorot(lin.weight)
            if lin.bias is not None:
                _fan_in_uniform(lin.bias, self.in_channels)
        if self.lin_edge is not None:
            _glorot(self.lin_edge.weight)
        _glorot(self.att)
        if self.bias is not None:
            with torch.no_grad():
                self.bias.zero_()

    @property
    def out_columns(self) -> int:
        """Columns of the output: H * C concatenated, C as the head mean."""
        return self.heads * self.out_channels if self.concat else self.out_channels

    def _slots(self) -> List[Optional[torch.Tensor]]:
        """The 7 kernel slots (att, bias, W_l, b_l, W_r, b_r, W_e) in the slab's column order."""
        return [self.att, self.bias, self.lin_l.weight, self.lin_l.bias, self.lin_r.weight, self.lin_r.bias,
                None if self.lin_edge is None else self.lin_edge.weight]

    def forward(self, x, edge_index, edge_attr=None, return_attention_weights=None):
        if isinstance(x, (tuple, list)):
            raise ValueError("GATv2Conv: bipartite (tuple) inputs are not supported")
        if return_attention_weights:
            raise ValueError("GATv2Conv: return_attention_weights is not supported")
        if self.lin_edge is None:
            edge_attr = None
        elif edge_attr is None:
            raise ValueError("GATv2Conv: edge_dim is set, so forward needs edge_attr")
        return run_gat([self], None, "none", x, edge_index, edge_attr)


class GAT_DSSE(nn.Module):
    """/root/reference/networks.py:113-156: ``num_layers - 1`` GATv2Conv(dim_feat -> dim_feat) layers, each followed by the
    (shared) nonlinearity, then Linear(dim_feat, dim_dense) and Linear(dim_dense, dim_out)."""

    def __init__(self, dim_feat, dim_dense, dim_out, num_layers, edge_dim, heads=1, concat=True, slope=0.2, self_loops=True,
                 dropout=0., nonlin="leaky_relu", model="gat"):
        super().__init__()
        self.dim_out = dim_out
        self.num_layers = num_layers
        self.dim_feat = dim_feat
        self.dim_dense = dim_dense
        self.edge_dim = edge_dim
        self.dim_hidden = dim_feat
        self.channels = dim_feat
        self.heads = heads
        self.concat = concat
        self.slope = slope
        self.dropout = dropout
        self.loop = self_loops
        self.nonlin = lanegroup.nonlin_module(nonlin)
        if model != "gat":
            raise ValueError("invalid model type")
        if num_layers < 1:
            raise ValueError(f"num_layers = {num_layers}: at least 1 (the two Linears)")
        if isinstance(heads, int) and heads > 1 and concat and num_layers > 1:
            # (every conv is channels -> channels and the first Linear takes dim_hidden = channels columns: the reference's
            # forward fails on the heads * channels columns of a concatenated output)
            raise ValueError(f"GAT_DSSE: heads = {heads} with concat=True gives {heads} * {dim_feat} columns, which fit neither "
                             f"the next conv nor Linear(dim_hidden, dim_dense); pass concat=False (the head mean)")
        _check_width("dim_feat", dim_feat, MAX_CHANNELS)
        _check_width("dim_dense", dim_dense, MAX_DENSE)
        _check_width("dim_out", dim_out, MAX_DENSE)
        layers, convs = [], []
        for _ in range(num_layers - 1):
            conv = GATv2Conv(self.channels, self.channels, heads=heads, concat=concat, negative_slope=slope, dropout=dropout,
                             add_self_loops=self_loops, edge_dim=edge_dim)
            convs.append(conv)
            layers += [conv, self.nonlin]
        head = [nn.Linear(self.dim_hidden, dim_dense), nn.Linear(dim_dense, dim_out)]
        self.model = lanegroup.Sequential(layers + head, convs, head, nonlin, run_gat)

    def forward(self, x, edge_index, edge_attr):
        return self.model(x, edge_index, edge_attr)


# ------------------------------------------------------------------------------------------
# the fused route
# ------------------------------------------------------------------------------------------
class _Spec(lanegroup.Spec):
    """Dimensions, slab layout and launch geometry of one conv stack (+ head)."""

    def __init__(self, convs, head, nonlin, n_nodes):
        c0 = convs[0] if convs else None
        self.ed = (c0.edge_dim or 0) if c0 is not None else 0
        self.loops = int(c0.add_self_loops) if c0 is not None else 1
        self.slope = float(c0.negative_slope) if c0 is not None else 0.2
        self.heads = c0.heads if c0 is not None else 1
        self.concat = c0.concat if c0 is not None else True
        for cv in convs:
            if (cv.edge_dim or 0) != self.ed or int(cv.add_self_loops) != self.loops or float(cv.negative_slope) != self.slope:
                raise ValueError("GAT stack: every conv must share edge_dim, add_self_loops and negative_slope")
            if cv.heads != self.heads or cv.concat != self.concat:
                raise ValueError("GAT stack: every conv must share heads and concat")
        if head and convs and self.heads > 1 and self.concat:
            raise ValueError("GAT stack: the head Linears after concatenated heads are not supported; pass concat=False")
        # the lane group covers a conv's input channels and the lanes of its heads; slab columns in parameter order:
        # att[w], bias[out columns], lin_l.weight[w][cin], lin_l.bias[w], lin_r.weight[w][cin], lin_r.bias[w], lin_edge.weight[w][ed]
        widths = [w for cv in convs for w in (cv.in_channels, lane_channels(cv.out_channels, cv.heads))]
        cols = [3 * w + cv.out_columns + 2 * w * cv.in_channels + w * self.ed for cv in convs for w in (cv.heads * cv.out_channels,)]
        super().__init__("GAT", convs, head, nonlin, n_nodes, widths, cols)


def _slots(convs, head) -> List[Optional[torch.Tensor]]:
    ps = []
    for cv in convs:
        ps += cv._slots()
    if head:
        ps += [head[0].weight, head[0].bias, head[1].weight, head[1].bias]
    return ps


def run_gat(convs, head, nonlin, x, edge_index, edge_attr):
    _require_gpu(x, edge_index, edge_attr)
    if edge_attr is not None:
        from .networks import _no_edge_attr_grad
        _no_edge_attr_grad(edge_attr)
    lanegroup.check_x(x, edge_index, int64=True)
    if x.size(0) == 0:
        raise ValueError("GAT: empty batch")
    if edge_index.size(1) == 0:
        topo = lanegroup.NoEdges(x.size(0), x.device)       # every node attends to its self loop alone (without loops: the bias)
    else:
        topo = get_topology(edge_index, x.size(0), double=False)
        topo.stats()       # (cached per structure) raises on node ids outside [0, N) before a kernel reads them
    spec = _Spec(convs, head, nonlin, x.size(0))
    lanegroup.check_columns(x, spec)
    if spec.ed:
        if edge_attr is None or edge_attr.dim() != 2 or edge_attr.size(1) != spec.ed or edge_attr.size(0) != edge_index.size(1):
            raise ValueError(f"edge_attr must be [E, {spec.ed}]")
    else:
        edge_attr = None
    return _GATFn.apply(x, edge_attr, topo, spec, *_slots(convs, head))


def _graph(topo, spec, ea, ldea, slab=None):
    g = _lib.GatGraph()
    lanegroup.fill_csr(g, topo)
    g.ea, g.ldea = _ptr(ea), ldea
    g.n_nodes, g.ed, g.add_self_loops, g.slope, g.nonlin = topo.N, spec.ed, spec.loops, spec.slope, spec.nonlin
    g.slab, g.n_slabs, g.slab_len = _ptr(slab), spec.n_slabs, spec.total
    return g


def _conv(d, cv, ps7, h, ldh, st, off):
    d.att, d.bias, d.Wl, d.bl, d.Wr, d.br, d.We = (_ptr(t) for t in ps7)
    d.h, d.ldh = h.data_ptr(), ldh
    d.y, d.m, d.s = st["y"].data_ptr(), st["ms"].data_ptr(), st["ms"].data_ptr() + 4 * st["ms"].size(1)
    for k in ("dxl", "dxr", "dedge", "dself"):
        if k in st:
            setattr(d, k, st[k].data_ptr())
    d.cin, d.cout, d.slab_off, d.heads, d.concat = cv.in_channels, cv.out_channels, off, cv.heads, int(cv.concat)


class _GATFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ea, topo, spec, *ps):
        N, dev = topo.N, x.device
        x, ldx = _rows(x)
        ldea = 0
        if ea is not None:
            ea, ldea = _rows(ea)
        convs, n = spec.convs, len(spec.convs)
        states, hs = lanegroup.state_chain(x, ldx, [cv.out_columns for cv in convs],
                                           lambda l: {"ms": torch.empty(2, N * convs[l].heads, dtype=_F32, device=dev)})

        def conv_into(d, l):
            _conv(d, convs[l], ps[7 * l:7 * l + 7], hs[l][0], hs[l][1], states[l], spec.offs[l])

        hst, out = lanegroup.forward(spec, _graph(topo, spec, ea, ldea), _lib.GatArgs, "dss2_gat_forward", conv_into, x, ldx,
                                     ps[7 * n:])
        if out is None:
            out = states[-1]["y"]
        # internal buffers live on ctx (never handed out, except the last conv's y of a head-less stack, whose backward does
        # not read it: the standalone layer has no nonlinearity)
        ctx.save_for_backward(x, ea)      # (autograd's version check covers the inputs the backward reads)
        ctx.st = (topo, spec, ldx, ldea, states, hs, hst, ps)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, ea = ctx.saved_tensors
        topo, spec, ldx, ldea, states, hs, hst, ps = ctx.st
        N, dev, E = topo.N, gout.device, topo.E
        gout, ldgo = _rows(gout)
        convs, head = spec.convs, spec.head
        n = len(convs)
        slab = torch.empty(spec.n_slabs, spec.total, dtype=_F32, device=dev)
        flat = torch.empty(spec.total, dtype=_F32, device=dev)
        cmax = max([cv.heads * cv.out_channels for cv in convs] or [1])      # d x_l, d x_r and the per-edge terms: every head's row
        pp = [(torch.empty(E, cmax, dtype=_F32, device=dev), torch.empty(N, cmax, dtype=_F32, device=dev)) for _ in range(2 if n > 1 else 1)]
        for l, cv in enumerate(convs):
            st = states[l]
            st["dxl"] = torch.empty(N, cv.heads * cv.out_channels, dtype=_F32, device=dev)
            st["dxr"] = torch.empty(N, cv.heads * cv.out_channels, dtype=_F32, device=dev)
            st["dedge"], st["dself"] = pp[l % len(pp)]
        dx = torch.empty(N, x.size(1), dtype=_F32, device=dev) if ctx.needs_input_grad[0] else None

        def conv_into(d, l):
            _conv(d, convs[l], ps[7 * l:7 * l + 7], hs[l][0], hs[l][1], states[l], spec.offs[l])

        # head backward (or the output gradient) + target pass of the last conv, then per conv l its source pass fused with the
        # target pass of conv l - 1; the last one writes dx
        lanegroup.backward(spec, _graph(topo, spec, ea, ldea, slab), _lib.GatArgs, "dss2_gat_backward", conv_into, gout, ldgo,
                           ps[7 * n:], hst, dx)
        # outer-product weight gradients of every layer, then ONE fixed-order reduction of the slab
        jobs = []
        for l, cv in enumerate(convs):
            w, ci, off = cv.heads * cv.out_channels, cv.in_channels, spec.offs[l] + cv.out_columns
            h, ldh = hs[l]
            jobs.append((states[l]["dxl"], w, h, ldh, w, ci, off + w))
            jobs.append((states[l]["dxr"], w, h, ldh, w, ci, off + 2 * w + w * ci))
        if head:
            jobs += lanegroup.head_wgrad_jobs(spec, states, x, ldx, hst, gout, ldgo)
        lanegroup.wgrad(jobs, slab, spec, N, dev)
        lanegroup.reduce_slabs([(slab, flat, spec.total, spec.total, spec.n_slabs)], dev)
        grads = []
        for l, cv in enumerate(convs):
            w, ci, ed, off = cv.heads * cv.out_channels, cv.in_channels, spec.ed, spec.offs[l]
            sizes = [w, cv.out_columns, w * ci, w, w * ci, w, w * ed]
            parts, o = [], off
            for sz in sizes:
                parts.append(flat[o:o + sz])
                o += sz
            for t, gpart in zip(ps[7 * l:7 * l + 7], parts):
                grads.append(None if t is None else gpart.view(t.shape))
        grads += lanegroup.head_grads(spec, flat)
        return lanegroup.backward_result(ctx, dx, grads)
