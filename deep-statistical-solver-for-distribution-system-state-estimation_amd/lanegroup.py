"""The lane-group route that ``gat.py`` (GAT_DSSE) and ``gine.py`` (GINE_DSSE) share, on csrc/dss2_lanegroup.{hpp,hip}.

Both models run one node per lane group of 8 / 16 / 32 lanes, fuse the two head Linears into the last conv's launches, write
their weight-gradient partials to the rows of a slab and reduce it once.  Here: the width limits, the ``Sequential``
look-alike, the head's descriptor, slab columns and gradients, the launch schedule of the forward and of the backward, and
the head's outer-product weight gradients.  Each model keeps its convs: their slab columns, state buffers, descriptor and
conv-gradient slicing.

The launch schedule, with ``n`` convs:

    forward    conv 0, ..., conv n - 1 (+ head), one launch each; with n = 0 one launch of the head alone on x
    backward   head backward (or the output gradient) + the node-local pass of conv n - 1, then per l = n - 1 .. 0 the source
               pass of conv l + the node-local pass of conv l - 1; the last one writes dx
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import torch
import torch.nn as nn

from . import _lib

_F32 = torch.float32
MAX_CHANNELS = 32        # conv input / output channels and the head's input width (lane group of 8 / 16 / 32 lanes)
MAX_EDGE_DIM = 16
MAX_DENSE = 32           # head widths dim_dense and dim_out
_MAX_SLABS = 256
_NONLIN = {"none": 0, "leaky_relu": 1, "relu": 2, "tanh": 3}


def check_width(model: str, name: str, v: int, limit: int) -> None:
    if not isinstance(v, int) or v < 1 or v > limit:
        raise ValueError(f"{name} = {v}: the {model} kernels take 1 <= {name} <= {limit}")


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

    def __init__(self, model, convs, head, nonlin, n_nodes, widths, conv_cols):
        self.convs, self.head = convs, head
        self.nonlin = _NONLIN[nonlin]
        widths = list(widths)
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


def _head_into(d, head, hps, hst):
    d.W1, d.b1, d.W2, d.b2 = (t.data_ptr() for t in hps)
    d.c, d.dense, d.nout = head_dims(head)
    d.z1 = hst["z1"].data_ptr()


def forward(spec, g, Args, fn, conv_into, x, ldx, hps):
    """The forward launches (``fn`` the model's forward entry point, ``conv_into(desc, l)`` fills conv l's descriptor).
    Returns the head's buffers and its output (None without a head)."""
    L, sm, N, dev = _lib.lib(), _lib.stream_ptr(x.device), g.n_nodes, x.device
    head, n = spec.head, len(spec.convs)
    hst, out = {}, None
    if head:
        _, d, o = head_dims(head)
        hst["z1"] = torch.empty(N, d, dtype=_F32, device=dev)
        out = torch.empty(N, o, dtype=_F32, device=dev)
    for l in range(n):
        a = Args()
        a.g, a.group, a.has_lo = g, spec.group, 1
        conv_into(a.lo, l)
        if head and l == n - 1:
            a.has_head = 1
            _head_into(a.head, head, hps, hst)
            a.head.out, a.head.ldo = out.data_ptr(), out.stride(0)
        _lib.check(getattr(L, fn)(C.byref(a), sm), fn)
    if n == 0:
        a = Args()
        a.g, a.group, a.has_head = g, spec.group, 1
        _head_into(a.head, head, hps, hst)
        a.head.hin, a.head.ldhin = x.data_ptr(), ldx
        a.head.out, a.head.ldo = out.data_ptr(), out.stride(0)
        _lib.check(getattr(L, fn)(C.byref(a), sm), fn)
    return hst, out


def backward(spec, g, Args, fn, conv_into, gout, ldgo, hps, hst, dx):
    """The backward launches up to the model input's gradient, written to dx (or dropped when dx is None).  The head's hidden
    gradient goes to hst["dz1"]."""
    L, sm, N, dev = _lib.lib(), _lib.stream_ptr(gout.device), g.n_nodes, gout.device
    head, n = spec.head, len(spec.convs)
    dh = dx.data_ptr() if dx is not None else None
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
        a.dh, a.dh_cols = dh, head[0].in_features       # no conv: the head reads the model input
    _lib.check(getattr(L, fn)(C.byref(a), sm), fn)
    for l in range(n - 1, -1, -1):
        a = Args()
        a.g, a.group, a.has_up = g, spec.group, 1
        conv_into(a.up, l)
        if l > 0:
            a.has_lo = 1
            conv_into(a.lo, l - 1)
        else:
            a.dh, a.dh_cols = dh, a.up.cin                  # conv 0's input is the model input
        _lib.check(getattr(L, fn)(C.byref(a), sm), fn)


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


def backward_result(ctx, dx, grads):
    """The autograd Function's return value for forward(ctx, x, ea, topo, spec, *ps): no gradient for a parameter that does
    not need one."""
    grads = [gr if ctx.needs_input_grad[4 + k] else None for k, gr in enumerate(grads)]
    return (dx, None, None, None, *grads)
