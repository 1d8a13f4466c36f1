"""The lane-group route that ``gat.py`` (GAT_DSSE), ``gine.py`` (GINE_DSSE) and ``gnn.py`` (gnn_dsse) share, on
csrc/dss2_lanegroup.{hpp,hip}.

The three models run one node per lane group of 8 / 16 / 32 lanes, fuse the two head Linears into the last conv's launches,
write their weight-gradient partials to the rows of a slab and reduce it once.  Here: the width limits, the ``Sequential``
look-alikes, the input checks, the CSR of the graph struct, the convs' state chain, the head's descriptor, slab columns and
gradients, the launch schedule of the forward and of the backward, the head's outer-product weight gradients and the slab
reduction.  Each model keeps its convs: their slab columns, state buffers, descriptor and conv-gradient slicing.

The launch schedule, with ``n`` convs.  A conv takes one launch per hop: ``spec.fwd_hops`` in the forward, ``spec.bwd_hops`` in
the backward, both ``(0,)`` except for gnn_dsse's TAGConv (forward hops 1..K, adjoint hops K-1..0; hop 0 alone with K = 0):

    forward    conv 0, ..., conv n - 1, one launch per hop, the head in the last hop of conv n - 1; with n = 0 one launch of the
               head alone on x
    backward   head backward (or the output gradient) + the node-local pass of conv n - 1, then per l = n - 1 .. 0 the source
               pass of conv l, one launch per hop; its last hop carries the node-local pass of conv l - 1, or (l = 0) writes dx

A model that has fields of its own in the args of a launch passes ``hook(args, l, hop)``, called before every launch with the
conv l the launch runs (forward) or takes the source pass of (backward; l = n in the first backward launch).  Only gnn_dsse does.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Sequence

import torch
import torch.nn as nn

from . import _lib
from .ops import _ptr

_F32 = torch.float32
MAX_CHANNELS = 32        # conv input / output channels and the head's input width (lane group of 8 / 16 / 32 lanes)
MAX_EDGE_DIM = 16
MAX_DENSE = 32           # head widths dim_dense and dim_out
_MAX_SLABS = 256
_NONLIN = {"none": 0, "leaky_relu": 1, "relu": 2, "tanh": 3}


def check_width(model: str, name: str, v: int, limit: int) -> None:
    if not isinstance(v, int) or v < 1 or v > limit:
        raise ValueError(f"{name} = {v}: the {model} kernels take 1 <= {name} <= {limit}")


def glorot(t: torch.Tensor) -> None:
    """PyG's glorot: uniform(-a, a), a = sqrt(6 / (fan_in + fan_out)) over the last two dimensions."""
    a = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    with torch.no_grad():
        t.uniform_(-a, a)


def nonlin_module(nonlin: str) -> nn.Module:
    """The ``*_DSSE`` constructors' ``nonlin`` argument as a module."""
    if nonlin == "relu":
        return nn.ReLU()
    if nonlin == "tanh":
        return nn.Tanh()
    if nonlin == "leaky_relu":
        return nn.LeakyReLU()
    raise ValueError("invalid activation type")


class Sequential(nn.Module):
    """Stand-in for PyG's ``Sequential('x, edge_index, edge_attr', [...])`` as the ``*_DSSE`` models build it: children
    ``module_{i}`` in the list's order (the naming is PyG's and not pinned by a test against PyG itself).  ``forward`` runs the
    model's fused route, ``run(convs, head, nonlin, x, edge_index, edge_attr)``."""

    def __init__(self, modules: Sequence[nn.Module], convs: Sequence[nn.Module], head: Sequence[nn.Linear], nonlin: str, run):
        super().__init__()
        for i, m in enumerate(modules):
            self.add_module(f"module_{i}", m)
        self.__dict__["_convs"], self.__dict__["_head"], self.__dict__["_nonlin"] = list(convs), list(head), nonlin
        self.__dict__["_run"] = run

    def forward(self, x, edge_index, edge_attr):
        return self._run(self._convs, self._head, self._nonlin, x, edge_index, edge_attr)


class SequentialX0(Sequential):
    """``Sequential('x, x_0, edge_index', [...])`` as ``gnn_dsse`` builds it: the same children and naming, called with the
    model input ``x_0`` beside ``x``; ``forward`` runs ``run(convs, head, nonlin, x, x_0, edge_index)``."""

    def forward(self, x, x_0, edge_index):
        return self._run(self._convs, self._head, self._nonlin, x, x_0, edge_index)


def head_dims(head):
    """(c, dense, nout) of the two head Linears."""
    return head[0].in_features, head[0].out_features, head[1].out_features


class Spec:
    """The shared half of a model's spec: lane group, slab count and the head's slab columns.  The model checks its convs, then
    passes their channel widths and the slab columns each conv takes; the convs' columns come first, the head's follow."""

    fwd_hops = bwd_hops = (0,)       # the hops of one conv's launches (see the module docstring)

    def __init__(self, model, convs, head, nonlin, n_nodes, widths, conv_cols):
        self.convs, self.head = convs, head
        self.nonlin = _NONLIN[nonlin]
        widths = list(widths)
        self.x_cols = widths[0] if widths else head[0].in_features      # the model input's width
        if head:
            widths.append(head[0].in_features)
            if head[0].out_features > MAX_DENSE or head[1].out_features > MAX_DENSE or head[1].in_features != head[0].out_features:
                raise ValueError(f"{model} head: widths up to {MAX_DENSE}")
        if max(widths) > MAX_CHANNELS:
            raise ValueError(f"{model}: channel width {max(widths)} above the limit {MAX_CHANNELS}")
        self.group = 8 if max(widths) <= 8 else (16 if max(widths) <= 16 else 32)
        self.offs, off = [], 0
        for cols in conv_cols:
            self.offs.append(off)
            off += cols
        self.head_off = off
        if head:
            c, d, o = head_dims(head)
            off += d * c + d + o * d + o
        self.total = off
        self.n_slabs = max(1, min(_MAX_SLABS, -(-n_nodes // (256 // self.group))))


class NoEdges:
    """The CSR of an edge-less batch (Topology refuses E = 0)."""

    def __init__(self, n, dev):
        self.N, self.E = n, 0
        self.rowptr = self.rowptrT = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        self.col = self.ent = self.colT = self.entT = self.rowptr
        self._gnn_structures = {}      # (gnn._structure: as on a Topology)


def check_x(x, edge_index=None, int64=False):
    """The shapes of x and (where the model does not leave it to Topology) of edge_index."""
    if x.dim() != 2:
        raise ValueError("x must be [N, C]")
    if edge_index is None:
        return
    if edge_index.dim() != 2 or edge_index.size(0) != 2 or (int64 and edge_index.dtype != torch.int64):
        raise ValueError("edge_index must be an int64 tensor [2, E]" if int64 else "edge_index must be [2, E]")


def check_columns(x, spec):
    if x.size(1) != spec.x_cols:
        raise ValueError(f"x has {x.size(1)} columns, the model takes {spec.x_cols}")


def fill_csr(g, topo):
    """The CSR by target and by source of a graph struct."""
    g.rowptr, g.col, g.ent = topo.rowptr.data_ptr(), topo.col.data_ptr(), topo.ent.data_ptr()
    g.rowptrT, g.colT, g.entT = topo.rowptrT.data_ptr(), topo.colT.data_ptr(), topo.entT.data_ptr()


def state_chain(x, ldx, widths, extra):
    """The convs' buffers and inputs: states[l] = {"y": [N, widths[l]], **extra(l)}; hs[l] = (conv l's input, its row stride),
    x for conv 0 and the y before it for the others."""
    states, hs = [], []
    h, ldh = x, ldx
    for l, w in enumerate(widths):
        st = {"y": torch.empty(x.size(0), w, dtype=_F32, device=x.device), **extra(l)}
        states.append(st)
        hs.append((h, ldh))
        h, ldh = st["y"], w
    return states, hs


def _head_into(d, head, hps, hst):
    d.W1, d.b1, d.W2, d.b2 = (t.data_ptr() for t in hps)
    d.c, d.dense, d.nout = head_dims(head)
    d.z1 = hst["z1"].data_ptr()


def _launch(fn, a, sm, hook, l, hop):
    if hook is not None:
        hook(a, l, hop)
    _lib.check(getattr(_lib.lib(), fn)(C.byref(a), sm), fn)


def forward(spec, g, Args, fn, conv_into, x, ldx, hps, hook=None):
    """The forward launches (``fn`` the model's forward entry point, ``conv_into(desc, l)`` fills conv l's descriptor).
    Returns the head's buffers and the model's output (the last conv's y without a head)."""
    sm, N, dev = _lib.stream_ptr(x.device), g.n_nodes, x.device
    head, n, hops = spec.head, len(spec.convs), spec.fwd_hops
    hst, out = {}, None
    if head:
        _, d, o = head_dims(head)
        hst["z1"] = torch.empty(N, d, dtype=_F32, device=dev)
        out = torch.empty(N, o, dtype=_F32, device=dev)
    for l in range(n):
        for hop in hops:
            a = Args()
            a.g, a.group, a.has_lo = g, spec.group, 1
            conv_into(a.lo, l)
            if head and l == n - 1 and hop == hops[-1]:
                a.has_head = 1
                _head_into(a.head, head, hps, hst)
                a.head.out, a.head.ldo = out.data_ptr(), out.stride(0)
            _launch(fn, a, sm, hook, l, hop)
    if n == 0:
        a = Args()
        a.g, a.group, a.has_head = g, spec.group, 1
        _head_into(a.head, head, hps, hst)
        a.head.hin, a.head.ldhin = x.data_ptr(), ldx
        a.head.out, a.head.ldo = out.data_ptr(), out.stride(0)
        _launch(fn, a, sm, hook, 0, 0)
    return hst, out


def backward(spec, g, Args, fn, conv_into, gout, ldgo, hps, hst, dx, hook=None):
    """The backward launches up to the model input's gradient, written to dx (or dropped when dx is None).  The head's hidden
    gradient goes to hst["dz1"]."""
    sm, N, dev = _lib.stream_ptr(gout.device), g.n_nodes, gout.device
    head, n, hops = spec.head, len(spec.convs), spec.bwd_hops
    dh = _ptr(dx)
    a = Args()
    a.g, a.group = g, spec.group
    if head:
        hst["dz1"] = torch.empty(N, head[0].out_features, dtype=_F32, device=dev)
        a.has_head = 1
        _head_into(a.head, head, hps, hst)
        a.head.gout, a.head.ldgo, a.head.dz1 = gout.data_ptr(), ldgo, hst["dz1"].data_ptr()
    else:
        a.gy, a.ldgy = gout.data_ptr(), ldgo
    if n:
        a.has_lo = 1
        conv_into(a.lo, n - 1)
    else:
        a.dh, a.dh_cols = dh, spec.x_cols                   # no conv: the head reads the model input
    _launch(fn, a, sm, hook, n, 0)
    for l in range(n - 1, -1, -1):
        for hop in hops:
            a = Args()
            a.g, a.group, a.has_up = g, spec.group, 1
            conv_into(a.up, l)
            if hop == hops[-1]:
                if l > 0:
                    a.has_lo = 1
                    conv_into(a.lo, l - 1)
                else:
                    a.dh, a.dh_cols = dh, spec.x_cols       # conv 0's input is the model input
            _launch(fn, a, sm, hook, l, hop)


def head_wgrad_jobs(spec, states, x, ldx, hst, gout, ldgo):
    """The head's two outer-product jobs (see wgrad): W1, b1 from dz1 and the head input, W2, b2 from gout and z1."""
    c, d, o = head_dims(spec.head)
    hin, ldhin = (states[-1]["y"], c) if spec.convs else (x, ldx)
    return [(hst["dz1"], d, hin, ldhin, d, c, spec.head_off), (gout, ldgo, hst["z1"], d, o, d, spec.head_off + d * c + d)]


def wgrad(jobs, slab, spec, n_nodes, dev):
    """Outer-product weight gradients into the slab, batched by dss2_lanegroup_wgrad.  A job (G, ldg, X, ldx, gw, xw, col)
    writes sum_n G[n][o] X[n][k] to columns col + o * xw + k and sum_n G[n][o] to col + gw * xw + o."""
    L, sm, M = _lib.lib(), _lib.stream_ptr(dev), _lib.LANEGROUP_WGRAD_MAX_JOBS
    for j0 in range(0, len(jobs), M):
        w = _lib.LanegroupWgradArgs()
        chunk = jobs[j0:j0 + M]
        for jd, (Gm, ldg, Xm, ldxm, gw, xw, col) in zip(w.jobs, chunk):
            jd.G, jd.ldg, jd.X, jd.ldx, jd.gw, jd.xw, jd.col = Gm.data_ptr(), ldg, Xm.data_ptr(), ldxm, gw, xw, col
        w.slab, w.n_nodes, w.n_slabs, w.slab_len, w.n_jobs = slab.data_ptr(), n_nodes, spec.n_slabs, spec.total, len(chunk)
        _lib.check(L.dss2_lanegroup_wgrad(C.byref(w), sm), "dss2_lanegroup_wgrad")


def head_grads(spec, flat):
    """The head's four gradients, views of the reduced slab row."""
    if not spec.head:
        return []
    c, d, o = head_dims(spec.head)
    h = spec.head_off
    return [flat[h:h + d * c].view(d, c), flat[h + d * c:h + d * c + d],
            flat[h + d * c + d:h + d * c + d + o * d].view(o, d), flat[h + d * c + d + o * d:spec.total]]


def reduce_slabs(descs, dev):
    """ONE fixed-order reduction: for every (slab, out, stride, len, n_slabs), out[:len] = the sum of the slab's n_slabs rows."""
    rd = (_lib.ReduceDesc * len(descs))()
    for r, (slab, out, stride, ln, n_slabs) in zip(rd, descs):
        r.slab, r.out, r.stride, r.len, r.n_slabs = slab.data_ptr(), out.data_ptr(), stride, ln, n_slabs
    _lib.check(_lib.lib().dss2_reduce_slabs_multi(rd, len(descs), _lib.stream_ptr(dev)), "dss2_reduce_slabs_multi")


def backward_result(ctx, dx, grads, dx0=None):
    """The autograd Function's return value for forward(ctx, x, ea or x0, topo, spec, *ps): no gradient for a parameter that
    does not need one."""
    grads = [gr if ctx.needs_input_grad[4 + k] else None for k, gr in enumerate(grads)]
    return (dx, dx0, None, None, *grads)
