"""The reference's ``MultiConvNet`` and ``WrappedMultiConv`` (/root/reference/networks.py:737-835) with PyG's ``ChebConv``
(2.3 - 2.6, ``normalization=None``), on the HIP kernels of csrc/dss2_cheb.hip.

    ChebConv(in_channels, out_channels, K, normalization=None, bias=True)
    WrappedMultiConv(num_convs, in_channels, out_channels, K)
    MultiConvNet(dim_featn, dim_feate, dim_out, dim_hid, n_gnn_layers, K, dropout_rate)

ChebConv, with j = edge_index[0] the source and i = edge_index[1] the target of edge e and w_e its weight (ones without one):
self loops are dropped, deg_i is the sum of w over the edges LEAVING i, the Laplacian entries are -w_e and deg_i, and

    lambda_max = 2 * max over every -w_e and every deg_i of the call           (when it is not given)
    what_e = 2 (-w_e) / lambda_max,   d_i = 2 deg_i / lambda_max - 1           (+inf after the division -> 0; 0 / 0 stays NaN)
    (A t)_i = d_i t_i + sum_{e: j->i} what_e t_j,   T_0 = x, T_1 = A x, T_k = 2 A T_{k-1} - T_{k-2}
    out = sum_{k<K} lins[k](T_k) + bias

``lambda_max`` is ONE scalar per call: the graphs of a batch are coupled through it (the largest entry of any graph scales all of
them), as in the reference, which never passes ``batch``.  A model's output for a graph therefore depends on the batch it is in, and a
shard of a batch does not compute what the batch computes: no sharded data-parallel use.

``MultiConvNet`` runs ``edge_trans`` (Linear(2, dim_hid), ReLU, Linear(dim_hid, 2)) on ``edge_attr[:, :2]``, adds the result to those
two columns, and uses column f as the edge weight of conv f of every layer; the graph is doubled by the reference's first-edge rule
(the reversed edges carry the same attribute rows).  Dropout and ReLU follow every layer but the last; the reference builds
``nn.Dropout`` inside ``forward``, so dropout is active in ``eval()`` too, and so it is here.

Gradients reach every parameter -- ``edge_trans`` through the edge weights, the degrees and ``lambda_max`` -- and x, and for the
standalone ``ChebConv`` / ``WrappedMultiConv`` the caller's ``edge_weight``.  ``max()`` hands its gradient to the arg-max entry; on an
exact tie torch splits it evenly over the tied entries, these kernels give it to the first one (edges in list order, then nodes).  The
two directions of a doubled edge tie exactly and share one attribute row, which makes the two rules agree there.

A model forward is ONE autograd node on the launch schedule of lanegroup.py, every launch through the library (so a step records into
launch plans and hipGraphs), with n layers, K terms and H = max(K - 1, 1) hop launches per layer:

    forward    the edge weights (dss2_cheb_edge_forward), [the dropout state], n H hop launches
    backward   the output gradient + the local step of the last layer, n H adjoint hops (the last of a layer carries the local step
               of the layer below, or writes dx), the edge weights' backward, the edge MLP's and the lins' weight gradients
               (dss2_lanegroup_wgrad: 1 + ceil(n F K / 16) launches), one slab reduction

T_1 .. T_{K-1} of every conv are SAVED by the forward for the backward (F (K - 1) N cin floats per layer), not recomputed.

Refused (ValueError): ``normalization`` other than None, ``batch`` with a per-graph ``lambda_max``, channel widths above 32, K outside
1..4, more than 4 parallel convs, edge_index lists that are not one structure; ``data.edge_attr.requires_grad`` on MultiConvNet
(NotImplementedError); CPU tensors (RuntimeError: there is no CPU path).

With ``lambda_max`` equal to 0 or not finite the output is what the reference computes (NaN where it has NaN), but the gradients are
unspecified: torch gives the ``+inf -> 0`` replacement a zero derivative, the edge backward divides by ``lambda_max`` without a guard.
"""
from __future__ import annotations

import ctypes as C
import functools

import torch
import torch.nn as nn

from . import _lib, lanegroup, ops
from .lanegroup import MAX_CHANNELS
from .ops import _ptr, _rows
from .topology import get_topology, reference_is_directed

_F32 = torch.float32
MAX_K, MAX_CONVS = _lib.CHEB_MAX_K, _lib.CHEB_MAX_CONVS
_check_width = functools.partial(lanegroup.check_width, "ChebConv")


class ChebConv(nn.Module):
    """PyG ``ChebConv`` on the HIP kernels.  Parameters ``bias [out]`` (zeros) and ``lins.{k}.weight [out, in]`` (glorot), k < K.
    ``forward(x, edge_index, edge_weight=None, batch=None, lambda_max=None)``; a float or 0-d tensor ``lambda_max`` is used as given
    and carries no gradient."""

    def __init__(self, in_channels: int, out_channels: int, K: int, normalization=None, bias: bool = True, **kwargs):
        super().__init__()
        if normalization is not None:
            raise ValueError(f"ChebConv: normalization={normalization!r} is not supported (the reference builds it with None)")
        _check_width("in_channels", in_channels, MAX_CHANNELS)
        _check_width("out_channels", out_channels, MAX_CHANNELS)
        _check_width("K", K, MAX_K)
        self.in_channels, self.out_channels, self.normalization = in_channels, out_channels, normalization
        self.lins = nn.ModuleList([nn.Linear(in_channels, out_channels, bias=False) for _ in range(K)])
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    @property
    def K(self) -> int:
        return len(self.lins)

    def reset_parameters(self) -> None:
        for lin in self.lins:
            lanegroup.glorot(lin.weight)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def forward(self, x, edge_index, edge_weight=None, batch=None, lambda_max=None):
        return _run_convs([[self]], x, edge_index, [edge_weight], batch, lambda_max)


def _lambda_given(batch, lambda_max):
    if lambda_max is None:
        return None
    if torch.is_tensor(lambda_max) and lambda_max.numel() > 1:
        raise ValueError("ChebConv: a per-graph lambda_max" + (" with batch" if batch is not None else "") + " is not supported; "
                         "pass one scalar or None (the maximum of the whole call)")
    return float(lambda_max)


class WrappedMultiConv(nn.Module):
    """/root/reference/networks.py:737-754: ``num_convs`` ChebConvs on one input whose outputs are summed, conv i on
    ``edge_index_list[i]`` / ``edge_weights_list[i]``.  Every entry of ``edge_index_list`` must be the same structure."""

    def __init__(self, num_convs, in_channels, out_channels, K, **kwargs):
        super().__init__()
        lanegroup.check_width("WrappedMultiConv", "num_convs", num_convs, MAX_CONVS)
        self.num_convs = num_convs
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.convs = nn.ModuleList()
        for i in range(num_convs):
            self.convs.append(ChebConv(in_channels, out_channels, K, normalization=None, **kwargs))

    def forward(self, x, edge_index_list, edge_weights_list):
        if len(edge_index_list) != self.num_convs or len(edge_weights_list) != self.num_convs:
            raise ValueError(f"WrappedMultiConv: {self.num_convs} convs need as many edge_index and edge_weights entries")
        ei = edge_index_list[0]
        for other in edge_index_list[1:]:
            if other is not ei and not (other.shape == ei.shape and other.data_ptr() == ei.data_ptr()):
                raise ValueError("WrappedMultiConv: the kernels run every conv on ONE structure; pass the same edge_index to each")
        return _run_convs([list(self.convs)], x, ei, list(edge_weights_list), None, None)


class MultiConvNet(nn.Module):
    """/root/reference/networks.py:756-835.  ``forward(data)`` reads data.x ([N, 4 + dim_featn + dim_featn]: node type, features,
    mask), data.edge_index and data.edge_attr ([E, >= 2]; only the first two columns are used)."""

    def __init__(self, dim_featn, dim_feate, dim_out, dim_hid, n_gnn_layers, K, dropout_rate):
        super().__init__()
        self.dim_featn = dim_featn
        assert dim_feate == 5
        dim_feate = dim_feate - 3      # only these two are meaningful
        self.dim_feate = dim_feate
        self.dim_out = dim_out
        self.dim_hid = dim_hid
        self.n_gnn_layers = n_gnn_layers
        self.K = K
        self.dropout_rate = dropout_rate
        if n_gnn_layers == 1 and dim_out != dim_hid:
            raise ValueError(f"MultiConvNet: n_gnn_layers = 1 builds the layers {dim_featn} -> {dim_out} and {dim_hid} -> {dim_out} "
                             "(as the reference does), which chain only with dim_out == dim_hid")
        self.edge_trans = nn.Sequential(nn.Linear(dim_feate, dim_hid), nn.ReLU(), nn.Linear(dim_hid, dim_feate))
        self.convs = nn.ModuleList()
        if n_gnn_layers == 1:
            self.convs.append(WrappedMultiConv(dim_feate, dim_featn, dim_out, K=K))
        else:
            self.convs.append(WrappedMultiConv(dim_feate, dim_featn, dim_hid, K=K))
        for l in range(n_gnn_layers - 2):
            self.convs.append(WrappedMultiConv(dim_feate, dim_hid, dim_hid, K=K))
        self.convs.append(WrappedMultiConv(dim_feate, dim_hid, dim_out, K=K))

    def is_directed(self, edge_index):
        """determine if a graph is directed by reading only one edge"""
        return reference_is_directed(edge_index)

    def undirect_graph(self, edge_index, edge_attr):
        if self.is_directed(edge_index):
            return torch.cat([edge_index, edge_index.flip(0)], dim=1), torch.cat([edge_attr, edge_attr], dim=0)
        return edge_index, edge_attr

    def forward(self, data):
        assert data.x.shape[-1] == self.dim_featn * 2 + 4      # features and their mask + one-hot node type embedding
        x = data.x[:, 4:4 + self.dim_featn]
        ea, ei = data.edge_attr, data.edge_index
        ops._require_gpu(x, ea, ei, *self.parameters())
        if ea.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("the DSS2 HIP path does not differentiate with respect to edge_attr (edge features are inputs "
                                      "of the reference's training loop, dss2_run.py:138); detach() it")
        if ea.dim() != 2 or ea.size(1) < 2 or ea.size(0) != ei.size(1):
            raise ValueError("edge_attr must be [E, >= 2]")
        if ei.size(1) == 0:
            raise ValueError("MultiConvNet: a batch without edges (the reference's is_directed reads the first edge)")
        lanegroup.check_x(x, ei, int64=True)
        topo = get_topology(ei, x.size(0), double=None, flip=False)      # doubled by the reference's first-edge rule
        topo.stats()       # (cached per structure) raises on node ids outside [0, N) before a kernel reads them
        layers = [list(w.convs) for w in self.convs]
        spec = _Spec(layers, x.size(0), mlp=self.edge_trans, ea=ea.detach(), p=float(self.dropout_rate))
        lanegroup.check_columns(x, spec)
        if any(spec.drops):
            spec.snapshot = ops.dropout_snapshot(self, x.device)
        self.__dict__["_last_snapshot"] = spec.snapshot      # (the masks of this call: ops.dropout_mask(snapshot, p, l + 1, N, width) for layer l)
        ps = [self.edge_trans[0].weight, self.edge_trans[0].bias, self.edge_trans[2].weight, self.edge_trans[2].bias]
        return _ChebFn.apply(x, None, topo, spec, *ps, *_conv_params(layers))


# ------------------------------------------------------------------------------------------
# the fused route
# ------------------------------------------------------------------------------------------
def _conv_params(layers):
    return [t for convs in layers for cv in convs for t in [cv.bias] + [lin.weight for lin in cv.lins]]


class _Spec(lanegroup.Spec):
    """Widths, K, the parallel convs, the slab layout and the launch geometry of a stack of layers (each a list of F ChebConvs)."""

    def __init__(self, layers, n_nodes, mlp=None, ea=None, p=0.0, lam=None):
        F, K = len(layers[0]), layers[0][0].K
        cins, couts = [cvs[0].in_channels for cvs in layers], [cvs[0].out_channels for cvs in layers]
        for cvs, ci, co in zip(layers, cins, couts):
            if len(cvs) != F or any(cv.K != K or cv.in_channels != ci or cv.out_channels != co for cv in cvs):
                raise ValueError("ChebConv stack: every conv of a layer has the layer's widths, every layer the same K and conv count")
        if any(co != ci for co, ci in zip(couts[:-1], cins[1:])):
            raise ValueError("ChebConv stack: a layer's input width is not the output width of the layer before it")
        self.F, self.K, self.cins, self.couts = F, K, cins, couts
        self.mlp, self.ea, self.lam, self.p = mlp, ea, lam, p
        self.hid = mlp[0].out_features if mlp is not None else 0
        if self.hid > 64:
            raise ValueError(f"edge_trans: {self.hid} hidden units above the limit 64")
        n = len(layers)
        self.drops = [l + 1 if (p > 0 and l < n - 1) else 0 for l in range(n)]      # the Philox mask id of layer l's dropout
        self.relus = [int(l < n - 1) for l in range(n)]
        self.snapshot = None
        self.fwd_hops = tuple(range(1, K)) or (0,)
        self.bwd_hops = tuple(range(K - 1, 0, -1)) or (0,)
        # slab columns of layer l: per conv f and term k, lins.k.weight[cout][cin] and a copy of the bias gradient[cout]
        self.blocks = [co * ci + co for ci, co in zip(cins, couts)]
        super().__init__("ChebConv", layers, None, "none", n_nodes, cins + couts, [F * K * b for b in self.blocks])
        self.mlp_off = self.total
        if mlp is not None:
            self.total += 5 * self.hid + 2
        self.n_ps = 4 if mlp is not None else 0      # parameters in front of the convs'


def _run_convs(layers, x, edge_index, weights, batch, lambda_max):
    lam = _lambda_given(batch, lambda_max)
    ps = _conv_params(layers)
    ops._require_gpu(x, edge_index, *[w for w in weights if w is not None], *[t for t in ps if t is not None])
    lanegroup.check_x(x, edge_index, int64=True)
    N, E = x.size(0), edge_index.size(1)
    if N == 0:
        raise ValueError("ChebConv: empty batch")
    if E == 0:
        topo = lanegroup.NoEdges(N, x.device)
    else:
        topo = get_topology(edge_index, N, double=False)
        topo.stats()       # (cached per structure) raises on node ids outside [0, N) before a kernel reads them
    cols = []
    for w in weights:
        if w is None:
            w = torch.ones(E, dtype=_F32, device=x.device)
        if w.dim() != 1 or w.numel() != E:
            raise ValueError("edge_weight must be [E]")
        cols.append(w)
    w = cols[0].unsqueeze(1) if len(cols) == 1 else torch.stack(cols, dim=1)
    spec = _Spec(layers, N, lam=lam)
    lanegroup.check_columns(x, spec)
    return _ChebFn.apply(x, w, topo, spec, *ps)


def _edge_wgs(N, E):
    return max(1, min(256, -(-max(N, E) // 256)))


def _graph(topo, spec, N, eb, slab=None):
    g = _lib.ChebGraph()
    lanegroup.fill_csr(g, topo)
    if topo.E:
        g.perm, g.permT, g.efrom, g.eto = topo.perm.data_ptr(), topo.permT.data_ptr(), topo.efrom.data_ptr(), topo.eto.data_ptr()
    g.n_nodes, g.n_edges, g.n_rows, g.n_convs = N, (topo.E2 if topo.E else 0), topo.E, spec.F
    g.w, g.what, g.dn, g.lam, g.arg = (eb[k].data_ptr() for k in ("w", "what", "dn", "lam", "arg"))
    g.slab, g.n_slabs, g.slab_len = _ptr(slab), spec.n_slabs, spec.total
    return g


def _edge_args(g, topo, spec, N, eb, w, mps):
    e = _lib.ChebEdgeArgs()
    e.g = g
    if spec.mlp is not None:
        ea, ldea = _rows(spec.ea)
        eb["ea"] = ea
        e.ea, e.ldea, e.has_mlp, e.hid = ea.data_ptr(), ldea, 1, spec.hid
        e.W1, e.b1, e.W2, e.b2 = (t.data_ptr() for t in mps)
    else:
        e.w_in, e.ldw = w.data_ptr(), (w.stride(0) if w.size(0) > 1 else w.size(1))
    if spec.lam is not None:
        e.lambda_given, e.lambda_ = 1, spec.lam
    e.n_wg = _edge_wgs(N, topo.E)
    e.pmax, e.parg, e.psum = eb["pmax"].data_ptr(), eb["parg"].data_ptr(), eb["psum"].data_ptr()
    return e


class _ChebFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, topo, spec, *ps):
        N, dev, F, K, n = x.size(0), x.device, spec.F, spec.K, len(spec.convs)
        x, ldx = _rows(x)
        if w is not None:
            w, _ = _rows(w)
        E, E2 = topo.E, (topo.E2 if topo.E else 0)
        mps, cps = ps[:spec.n_ps], ps[spec.n_ps:]
        nwg = _edge_wgs(N, E)
        eb = {"w": torch.empty(F, max(E, 1), dtype=_F32, device=dev), "what": torch.empty(F, max(E, 1), dtype=_F32, device=dev),
              "dn": torch.empty(F, N, dtype=_F32, device=dev), "lam": torch.empty(F, dtype=_F32, device=dev),
              "arg": torch.empty(F, dtype=torch.int64, device=dev), "pmax": torch.empty(F, nwg, dtype=_F32, device=dev),
              "parg": torch.empty(F, nwg, dtype=torch.int64, device=dev), "psum": torch.empty(F, nwg, dtype=_F32, device=dev)}
        g = _graph(topo, spec, N, eb)
        e = _edge_args(g, topo, spec, N, eb, w, mps)
        _lib.check(_lib.lib().dss2_cheb_edge_forward(C.byref(e), _lib.stream_ptr(dev)), "dss2_cheb_edge_forward")

        def extra(l):
            return {"T": torch.empty(F, K - 1, N, spec.cins[l], dtype=_F32, device=dev)} if K > 1 else {}

        states, hs = lanegroup.state_chain(x, ldx, spec.couts, extra)
        thr, scale = ops._dropout_params(spec.p) if spec.snapshot is not None else (0, 0.0)

        def conv_into(d, l, bufs=None):
            d.cin, d.cout, d.K, d.relu, d.drop_id = spec.cins[l], spec.couts[l], K, spec.relus[l], spec.drops[l]
            per = K + 1
            for f in range(F):
                cw = cps[(l * F + f) * per:(l * F + f + 1) * per]
                d.bias[f] = _ptr(cw[0])
                for k in range(K):
                    d.W[f][k] = cw[1 + k].data_ptr()
            d.h, d.ldh = hs[l][0].data_ptr(), hs[l][1]
            d.y, d.T = states[l]["y"].data_ptr(), _ptr(states[l].get("T"))
            if bufs is not None:
                d.dv = bufs["dv"][l].data_ptr()
                if K > 1:
                    d.r[0], d.r[1] = (t.data_ptr() for t in bufs["r"][l % 2])

        def hook(a, l, hop):
            a.hop = hop
            a.drop_state, a.drop_thr, a.drop_scale = _ptr(spec.snapshot), thr, scale

        lanegroup.forward(spec, g, _lib.ChebArgs, "dss2_cheb_forward", conv_into, x, ldx, [], hook)
        ctx.save_for_backward(x, w)
        ctx.st = (topo, spec, ldx, states, hs, eb, conv_into, hook, mps)
        return states[-1]["y"]

    @staticmethod
    def backward(ctx, gout):
        x, w = ctx.saved_tensors
        topo, spec, ldx, states, hs, eb, conv_fwd, hook_fwd, mps = ctx.st
        N, dev, F, K, n = x.size(0), gout.device, spec.F, spec.K, len(spec.convs)
        E, E2 = topo.E, (topo.E2 if topo.E else 0)
        gout, ldgo = _rows(gout)
        slab = torch.empty(spec.n_slabs * spec.total, dtype=_F32, device=dev)
        flat = torch.empty(spec.total, dtype=_F32, device=dev)
        dx = torch.empty(N, x.size(1), dtype=_F32, device=dev) if ctx.needs_input_grad[0] else None
        cmax = max(spec.cins)
        bufs = {"dv": [torch.empty(N, co, dtype=_F32, device=dev) for co in spec.couts],
                "r": [[torch.empty(F, N, cmax, dtype=_F32, device=dev) for _ in range(2)] for _ in range(min(n, 2))] if K > 1 else None}
        dwh = torch.empty(F, max(E2, 1), dtype=_F32, device=dev) if K > 1 else None
        ddn = torch.empty(F, N, dtype=_F32, device=dev) if K > 1 else None

        def conv_into(d, l):
            conv_fwd(d, l, bufs)

        def hook(a, l, hop):
            hook_fwd(a, l, hop)
            a.dwh, a.ddn = _ptr(dwh), _ptr(ddn)
            a.acc_first = int(l == n - 1 and hop == K - 1)      # the first adjoint hop of the step stores, every later one adds

        g = _graph(topo, spec, N, eb, slab)
        lanegroup.backward(spec, g, _lib.ChebArgs, "dss2_cheb_backward", conv_into, gout, ldgo, [], {}, dx, hook)
        # the edge weights: d what, d dn -> d w (through lambda's arg-max entry), and the edge MLP's dz1
        need_w = E > 0 and (spec.mlp is not None or ctx.needs_input_grad[1])
        dw = None
        if need_w:
            e = _edge_args(g, topo, spec, N, eb, w, mps)
            dw = torch.empty(E, F, dtype=_F32, device=dev)
            e.dwh, e.ddn, e.zero_in, e.dw = _ptr(dwh), _ptr(ddn), int(K == 1), dw.data_ptr()
            if spec.mlp is not None:
                dz1, a1 = (torch.empty(E, spec.hid, dtype=_F32, device=dev) for _ in range(2))
                e.dz1, e.a1 = dz1.data_ptr(), a1.data_ptr()
            _lib.check(_lib.lib().dss2_cheb_edge_backward(C.byref(e), _lib.stream_ptr(dev)), "dss2_cheb_edge_backward")
            if spec.mlp is not None:
                h, m = spec.hid, spec.mlp_off
                lanegroup.wgrad([(dz1, h, eb["ea"], e.ldea, h, 2, m), (dw, F, a1, h, 2, h, m + 3 * h)], slab, spec, E, dev)
        # the lins: outer products of dv and T_k over the nodes; then ONE fixed-order reduction
        jobs = []
        for l in range(n):
            ci, co, blk = spec.cins[l], spec.couts[l], spec.blocks[l]
            for f in range(F):
                for k in range(K):
                    Tk, ldt = hs[l] if k == 0 else (states[l]["T"][f, k - 1], ci)
                    jobs.append((bufs["dv"][l], co, Tk, ldt, co, ci, spec.offs[l] + (f * K + k) * blk))
        lanegroup.wgrad(jobs, slab, spec, N, dev)
        lanegroup.reduce_slabs([(slab, flat, spec.total, spec.total, spec.n_slabs)], dev)
        grads = []
        if spec.mlp is not None:
            h, m = spec.hid, spec.mlp_off
            grads += [flat[m:m + 2 * h].view(h, 2), flat[m + 2 * h:m + 3 * h], flat[m + 3 * h:m + 5 * h].view(2, h), flat[m + 5 * h:m + 5 * h + 2]]
        for l in range(n):
            ci, co, blk = spec.cins[l], spec.couts[l], spec.blocks[l]
            for f in range(F):
                o = spec.offs[l] + f * K * blk
                grads.append(flat[o + co * ci:o + blk] if spec.convs[l][f].bias is not None else None)
                grads += [flat[o + k * blk:o + k * blk + co * ci].view(co, ci) for k in range(K)]
        return lanegroup.backward_result(ctx, dx, grads, dw if (spec.mlp is None and ctx.needs_input_grad[1]) else None)
