"""GINE and the reference's GIN model, ``GINE_DSSE`` (/root/reference/networks.py:71-111), on the HIP kernels of
csrc/dss2_gine.hip.

    GINEConv(nn, eps=0., train_eps=False, edge_dim=None)          PyG's layer, same parameter names; nn must be a torch.nn.Linear
    GINE_DSSE(dim_feat, dim_dense, dim_out, num_layers, edge_dim, nn='mlp', nonlin='leaky_relu', eps=0., train_eps=False,
              model='gine')                                        the reference's signature and attributes

One layer (j = edge_index[0] the source, i = edge_index[1] the target, edges as given: no doubling, no self loops added or
removed, duplicates kept):  out_i = nn(sum_{e: j->i} relu(h_j + lin(ea_e)) + (1 + eps) h_i).  Without edge_dim the message is
relu(h_j + ea_e) and edge_attr must be [E, nn.in_features] (PyG's rule).

``GINE_DSSE`` builds ONE ``Linear(dim_feat, dim_feat)`` (``self.nn``) and hands the same object to every conv, as the reference
does: ``state_dict()`` lists it once per owner (``nn.*`` and ``model.module_{2k}.nn.*``), ``parameters()`` once, and its gradient is
the sum over the layers.  ``model`` is ``lanegroup.Sequential`` with children ``module_{i}`` (as in gat.py).  Its forward is
ONE autograd node (``_GINEFn``) on the launch schedule of lanegroup.py: one launch per conv forward (the head Linears fused into
the last one), one fused backward launch per conv (source pass of conv l + node-local step of conv l - 1), one launch for the
head's weight gradients and one fixed-order slab reduction.  Every launch goes through the library, so the step records into launch plans and hipGraphs.

One intended deviation: the reference's constructor argument ``nn='mlp'`` shadows ``torch.nn``, so its ``nonlin='relu'`` and
``nonlin='tanh'`` raise (``'mlp'.ReLU()``); here they build ``torch.nn.ReLU`` / ``torch.nn.Tanh`` as the argument names say.  The
default ``leaky_relu`` is the reference's model exactly.

Not provided (ValueError): an ``nn`` other than one Linear, bipartite (tuple) inputs, a missing edge_attr, widths over the limits.
No gradient with respect to edge_attr; no CPU path.
"""
from __future__ import annotations

import functools
from typing import List, Optional

import torch
import torch.nn as nn

from . import _lib, lanegroup
from .lanegroup import MAX_CHANNELS, MAX_DENSE, MAX_EDGE_DIM
from .ops import _ptr, _require_gpu, _rows
from .topology import get_topology

_F32 = torch.float32
_check_width = functools.partial(lanegroup.check_width, "GINE")


class GINEConv(nn.Module):
    """PyG ``GINEConv`` with ``nn`` one ``torch.nn.Linear`` on the HIP kernels.  ``state_dict`` keys in PyG's order: ``eps [1]``
    (a buffer, or a Parameter with train_eps), ``nn.{weight, bias}``, ``lin.{weight [in, edge_dim], bias [in]}`` (with edge_dim)."""

    def __init__(self, nn: torch.nn.Module, eps: float = 0.0, train_eps: bool = False, edge_dim: Optional[int] = None, **kwargs):
        super().__init__()
        if type(nn) is not torch.nn.Linear:
            raise ValueError(f"GINEConv: nn must be one torch.nn.Linear (got {type(nn).__name__}); other modules are not supported")
        _check_width("nn.in_features", nn.in_features, MAX_CHANNELS)
        _check_width("nn.out_features", nn.out_features, MAX_CHANNELS)
        if nn.bias is None:
            raise ValueError("GINEConv: nn must have a bias")
        if edge_dim is not None:
            _check_width("edge_dim", edge_dim, MAX_EDGE_DIM)
        self.nn = nn
        self.initial_eps = eps
        if train_eps:
            self.eps = torch.nn.Parameter(torch.empty(1))
        else:
            self.register_buffer("eps", torch.empty(1))
        self.edge_dim = edge_dim
        self.lin = torch.nn.Linear(edge_dim, nn.in_features) if edge_dim is not None else None
        self.reset_parameters()

    def reset_parameters(self) -> None:
        """PyG: reset(nn), eps = initial_eps, lin.reset_parameters() (PyG's Linear initialises as torch's)."""
        self.nn.reset_parameters()
        with torch.no_grad():
            self.eps.fill_(self.initial_eps)
        if self.lin is not None:
            self.lin.reset_parameters()

    def forward(self, x, edge_index, edge_attr=None, size=None):
        if isinstance(x, (tuple, list)):
            raise ValueError("GINEConv: bipartite (tuple) inputs are not supported")
        if size is not None:
            raise ValueError("GINEConv: size (bipartite graphs) is not supported")
        if edge_attr is None:
            raise ValueError("GINEConv: forward needs edge_attr")
        return run_gine([self], None, "none", x, edge_index, edge_attr)


class GINE_DSSE(nn.Module):
    """/root/reference/networks.py:71-111: ``num_layers - 1`` GINEConv layers sharing ONE Linear(dim_feat, dim_feat), each
    followed by the (shared) nonlinearity, then Linear(dim_feat, dim_dense) and Linear(dim_dense, dim_out)."""

    def __init__(self, dim_feat, dim_dense, dim_out, num_layers, edge_dim, nn="mlp", nonlin="leaky_relu", eps=0., train_eps=False,
                 model="gine"):
        super().__init__()
        self.dim_out = dim_out
        self.num_layers = num_layers
        self.dim_feat = dim_feat
        self.dim_dense = dim_dense
        self.eps = eps
        self.train_eps = train_eps
        self.edge_dim = edge_dim
        self.dim_hidden = dim_feat
        _check_width("dim_feat", dim_feat, MAX_CHANNELS)
        _check_width("dim_dense", dim_dense, MAX_DENSE)
        _check_width("dim_out", dim_out, MAX_DENSE)
        if edge_dim is not None:
            _check_width("edge_dim", edge_dim, MAX_EDGE_DIM)
        if num_layers < 1:
            raise ValueError(f"num_layers = {num_layers}: at least 1 (the two Linears)")
        if nn == "mlp":
            self.nn = torch.nn.Linear(in_features=self.dim_feat, out_features=self.dim_hidden)
        else:
            raise ValueError("invalid nn type")
        # (the reference calls nn.ReLU() / nn.Tanh() on the string argument here; see the module docstring)
        self.nonlin = lanegroup.nonlin_module(nonlin)
        if model != "gine":
            raise ValueError("invalid model type")
        layers, convs = [], []
        for _ in range(num_layers - 1):
            conv = GINEConv(nn=self.nn, eps=self.eps, train_eps=self.train_eps, edge_dim=self.edge_dim)
            convs.append(conv)
            layers += [conv, self.nonlin]
        head = [torch.nn.Linear(self.dim_hidden, self.dim_dense), torch.nn.Linear(self.dim_dense, self.dim_out)]
        self.model = lanegroup.Sequential(layers + head, convs, head, nonlin, run_gine)

    def forward(self, x, edge_index, edge_attr):
        return self.model(x, edge_index, edge_attr)


# ------------------------------------------------------------------------------------------
# the fused route
# ------------------------------------------------------------------------------------------
def _up4(v: int) -> int:
    return (v + 3) // 4 * 4


class _Spec(lanegroup.Spec):
    """Dimensions, slab layout and launch geometry of one conv stack (+ head)."""

    def __init__(self, convs, head, nonlin, n_nodes):
        self.nn = convs[0].nn if convs else None
        self.ed = (convs[0].edge_dim or 0) if convs else 0
        for cv in convs:
            if cv.nn is not self.nn:
                raise ValueError("GINE stack: every conv must share the one nn Linear")
            if (cv.edge_dim or 0) != self.ed:
                raise ValueError("GINE stack: every conv must have the same edge_dim")
        self.cin = self.nn.in_features if convs else 0
        self.cout = self.nn.out_features if convs else 0
        if len(convs) > 1 and self.cin != self.cout:
            raise ValueError("GINE stack: a shared nn between layers needs in_features == out_features")
        if convs and head and head[0].in_features != self.cout:
            raise ValueError("GINE head: its input width must be the convs' output width")
        # main slab row: per conv eps[1] (+ lin.weight [cin][ed], lin.bias [cin]), then the head; the shared nn's per-conv partials
        # go to a second slab [n_slabs][n_convs][nn_len]
        cols = [1 + (self.cin * self.ed + self.cin if self.ed else 0)] * len(convs)
        super().__init__("GINE", convs, head, nonlin, n_nodes, [self.cin, self.cout] if convs else [], cols)
        self.nn_len = self.cout * self.cin + self.cout


def _slots(convs, head) -> List[Optional[torch.Tensor]]:
    """[nn.weight, nn.bias] (when there is a conv), per conv [eps, lin.weight, lin.bias], the head's four."""
    ps = []
    if convs:
        ps += [convs[0].nn.weight, convs[0].nn.bias]
    for cv in convs:
        ps += [cv.eps, None if cv.lin is None else cv.lin.weight, None if cv.lin is None else cv.lin.bias]
    if head:
        ps += [head[0].weight, head[0].bias, head[1].weight, head[1].bias]
    return ps


def run_gine(convs, head, nonlin, x, edge_index, edge_attr):
    _require_gpu(x, edge_index, edge_attr, *[cv.eps for cv in convs])
    if convs:
        from .networks import _no_edge_attr_grad
        if edge_attr is None:
            raise ValueError("GINE: forward needs edge_attr")
        _no_edge_attr_grad(edge_attr)
    lanegroup.check_x(x, edge_index)
    if edge_index.size(1) == 0:
        topo = lanegroup.NoEdges(x.size(0), x.device)       # every GINE layer is then nn((1 + eps) h)
    else:
        topo = get_topology(edge_index, x.size(0), double=False)
        topo.stats()       # (cached per structure) raises on node ids outside [0, N) before a kernel reads them
    spec = _Spec(convs, head, nonlin, x.size(0))
    lanegroup.check_columns(x, spec)
    if convs:
        w = spec.ed if spec.ed else spec.cin
        if edge_attr.dim() != 2 or edge_attr.size(1) != w or edge_attr.size(0) != edge_index.size(1):
            raise ValueError(f"edge_attr must be [E, {w}]" + ("" if spec.ed else " (without edge_dim: [E, nn.in_features])"))
    else:
        edge_attr = None
    return _GINEFn.apply(x, edge_attr, topo, spec, *_slots(convs, head))


def _graph(topo, spec, ea, ldea, slab=None, nslab=None):
    g = _lib.GineGraph()
    lanegroup.fill_csr(g, topo)
    g.ea, g.ldea = _ptr(ea), ldea
    g.n_nodes, g.ed, g.nonlin = topo.N, spec.ed, spec.nonlin
    g.slab, g.n_slabs, g.slab_len = _ptr(slab), spec.n_slabs, spec.total
    g.nslab, g.nslab_len = _ptr(nslab), spec.nn_len * len(spec.convs)
    return g


def _conv(d, spec, ps, l, h, ldh, st, dz=None):
    d.Wn, d.bn = _ptr(ps[0]), _ptr(ps[1])
    d.eps, d.We, d.be = (_ptr(t) for t in ps[2 + 3 * l:5 + 3 * l])
    d.h, d.ldh = h.data_ptr(), ldh
    d.y, d.z = st["y"].data_ptr(), st["z"].data_ptr()
    d.dz = _ptr(dz)
    d.cin, d.cout, d.slab_off, d.nn_off = spec.cin, spec.cout, spec.offs[l], l * spec.nn_len


class _GINEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ea, topo, spec, *ps):
        N, dev = topo.N, x.device
        x, ldx = _rows(x)
        ldea = 0
        if ea is not None:
            ea, ldea = _rows(ea)
        n = len(spec.convs)
        states, hs = lanegroup.state_chain(x, ldx, [spec.cout] * n, lambda l: {"z": torch.empty(N, spec.cin, dtype=_F32, device=dev)})

        def conv_into(d, l):
            _conv(d, spec, ps, l, hs[l][0], hs[l][1], states[l])

        hst, out = lanegroup.forward(spec, _graph(topo, spec, ea, ldea), _lib.GineArgs, "dss2_gine_forward", conv_into, x, ldx,
                                     ps[2 + 3 * n:] if n else ps)
        if out is None:
            out = states[-1]["y"]
        # internal buffers live on ctx (never handed out, except the last conv's y of a head-less stack, whose backward does
        # not read it: the standalone layer has no nonlinearity)
        ctx.save_for_backward(x, ea)
        ctx.st = (topo, spec, ldx, ldea, states, hs, hst, ps)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, ea = ctx.saved_tensors
        topo, spec, ldx, ldea, states, hs, hst, ps = ctx.st
        N, dev = topo.N, gout.device
        gout, ldgo = _rows(gout)
        head, n = spec.head, len(spec.convs)
        main = _up4(spec.n_slabs * spec.total)
        buf = torch.empty(main + spec.n_slabs * n * spec.nn_len, dtype=_F32, device=dev)
        slab, nslab = buf[:main], buf[main:]
        flat = torch.empty(_up4(spec.total) + spec.nn_len, dtype=_F32, device=dev)
        fnn = flat[_up4(spec.total):]
        dzs = [torch.empty(N, spec.cin, dtype=_F32, device=dev) for _ in range(min(n, 2))]
        dx = torch.empty(N, x.size(1), dtype=_F32, device=dev) if ctx.needs_input_grad[0] else None

        def conv_into(d, l):
            _conv(d, spec, ps, l, hs[l][0], hs[l][1], states[l], dzs[l % 2])

        # head backward (or the output gradient) + the node-local step of the last conv, then per conv l its source pass fused
        # with the node-local step of conv l - 1; the last one writes dx
        lanegroup.backward(spec, _graph(topo, spec, ea, ldea, slab, nslab), _lib.GineArgs, "dss2_gine_backward", conv_into, gout,
                           ldgo, ps[2 + 3 * n:] if n else ps, hst, dx)
        # the head's outer-product weight gradients, then ONE fixed-order reduction of both slabs
        if head:
            lanegroup.wgrad(lanegroup.head_wgrad_jobs(spec, states, x, ldx, hst, gout, ldgo), slab, spec, N, dev)
        descs = [(slab, flat, spec.total, spec.total, spec.n_slabs)]
        if n:
            descs.append((nslab, fnn, spec.nn_len, spec.nn_len, spec.n_slabs * n))
        lanegroup.reduce_slabs(descs, dev)
        grads = []
        if n:
            ci, co = spec.cin, spec.cout
            grads += [fnn[:co * ci].view(co, ci), fnn[co * ci:co * ci + co]]
            for l in range(n):
                off, ed = spec.offs[l], spec.ed
                grads.append(flat[off:off + 1])
                grads += [flat[off + 1:off + 1 + ci * ed].view(ci, ed), flat[off + 1 + ci * ed:off + 1 + ci * ed + ci]] if ed else [None, None]
        grads += lanegroup.head_grads(spec, flat)
        return lanegroup.backward_result(ctx, dx, grads)
