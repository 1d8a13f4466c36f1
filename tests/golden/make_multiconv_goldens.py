#!/usr/bin/env python3
"""Generate tests/golden/case_multiconv_*.npz by running the REFERENCE's MultiConvNet (networks.py:737-835) and the backward of a
seeded output gradient.

Runs only where the reference checkout exists (REF below).  torch_geometric is not installed, so the reference's imports come from
the stand-in in tests/golden/_pyg_standin; its ChebConv is a placeholder, and THIS process installs a restatement of PyG 2.3-2.6's
into the stand-in's module object before importing the reference's unmodified networks.py:
    ChebConv   lins = K x Linear(in, out, bias=False), bias; __norm__: remove_self_loops, get_laplacian(normalization=None) (the
               stand-in's: deg over the SOURCE, entries -w_e and deg_i), lambda_max = 2 * max over all entries when not given,
               (2 w) / lambda_max, +inf -> 0, -1 on the diagonal; Tx_0 = x, Tx_1 = A x, Tx_k = 2 A Tx_{k-1} - Tx_{k-2};
               out = sum lins[k](Tx_k) + bias
Everything runs in float64 (default dtype); dropout_rate is 0.  Outputs are data only.

    python tests/golden/make_multiconv_goldens.py

Cases (seeded weights, conv biases non-zero since PyG zeros them; dim_featn 8, dim_out 2):
    case_multiconv_real64       the 64 real CIGRE-14 graphs, dim_hid 32, 3 layers, K = 2
    case_multiconv_k3 / _k4     K = 3 / 4 on a small synthetic batch (dim_hid 16)
    case_multiconv_k1           K = 1 (no hop: the edge weights do not reach the output)
    case_multiconv_h8 / _h16    dim_hid 8 / 16 (lane groups of 8 and 16)
    case_multiconv_undirected   an input that already holds both directions (no doubling)
    case_multiconv_mixed        a mixed cigre14 + ober_sub batch (dim_hid 16)
    case_multiconv_l1           n_gnn_layers = 1 (the reference's two layers; dim_out = dim_hid = 8)
Arrays: x ([N, 4 + 8 + 8]: node type one-hot, features, mask; for the real batch `node_type` [N] instead, the features and the
edges come from the fixture `batch` names, edge_attr = its edge_attr[:, ea_cols] with ea_jitter added to [:, :2]), edge_index, edge_attr [E, 5], param/<key> (float32) and gout (float16: the values the
fp64 run used), out, grad/<key>, dx (gradient with respect to x[:, 4:12]; not in the real batch's case, which would exceed 100 KB), keys (the state_dict key list, in order) and the constructor arguments.

The generator ASSERTS, for every case and feature, in fp64: the largest Laplacian entry exceeds the second largest by at least 1e-3
relative (no tie at the arg-max, where torch splits the gradient and the kernels do not), and lambda_max > 0.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as tnn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
# The model reads edge_attr[:, :2].  In the grids' edge features those two columns are flow measurements, zero on every edge that is
# not measured, and the columns that are populated everywhere are line parameters, the same in every graph of a grid: either way
# the largest Laplacian entry is tied (between the two ends of a measured edge, or between the same bus of different graphs)
# whatever the weights are.  The fixtures therefore put two populated columns in front and add a seeded per-edge jitter to them:
# edge_attr = the grid's edge_attr[:, EA_COLS], then [:, :2] += ea_jitter (uniform in +-0.25, float16 values).
EA_COLS = [4, 5, 0, 1, 2]
PKG = os.path.join(ROOT, "deep-statistical-solver-for-distribution-system-state-estimation_amd")

sys.path.insert(0, os.path.join(HERE, "_pyg_standin"))
import torch_geometric.nn.conv as pyg_conv                 # noqa: E402  (stand-in)
from torch_geometric.utils import get_laplacian            # noqa: E402  (stand-in)

LAMBDAS = []      # (entries, lambda_max) of every ChebConv call of the case being generated


class ChebConv(pyg_conv.MessagePassing):
    def __init__(self, in_channels, out_channels, K, normalization="sym", bias=True, **kwargs):
        super().__init__(aggr="add")
        assert K > 0 and normalization is None
        self.in_channels, self.out_channels, self.normalization = in_channels, out_channels, normalization
        self.lins = tnn.ModuleList([tnn.Linear(in_channels, out_channels, bias=False) for _ in range(K)])
        self.bias = tnn.Parameter(torch.zeros(out_channels)) if bias else None

    def __norm__(self, edge_index, num_nodes, edge_weight, lambda_max=None):
        keep = edge_index[0] != edge_index[1]                       # remove_self_loops
        edge_index, edge_weight = edge_index[:, keep], (None if edge_weight is None else edge_weight[keep])
        edge_index, edge_weight = get_laplacian(edge_index, edge_weight, None, torch.get_default_dtype(), num_nodes)
        if lambda_max is None:
            lambda_max = 2.0 * edge_weight.max()
        LAMBDAS.append((edge_weight.detach().clone(), float(lambda_max)))
        edge_weight = (2.0 * edge_weight) / lambda_max
        edge_weight = edge_weight.masked_fill(edge_weight == float("inf"), 0)
        loop_mask = edge_index[0] == edge_index[1]
        edge_weight = edge_weight - loop_mask.to(edge_weight.dtype)
        return edge_index, edge_weight

    def forward(self, x, edge_index, edge_weight=None, batch=None, lambda_max=None):
        edge_index, norm = self.__norm__(edge_index, x.size(0), edge_weight, lambda_max)
        Tx_0 = Tx_1 = x
        out = self.lins[0](Tx_0)
        if len(self.lins) > 1:
            Tx_1 = self.propagate(edge_index, x=x, norm=norm)
            out = out + self.lins[1](Tx_1)
        for lin in self.lins[2:]:
            Tx_2 = 2.0 * self.propagate(edge_index, x=Tx_1, norm=norm) - Tx_0
            out = out + lin(Tx_2)
            Tx_0, Tx_1 = Tx_1, Tx_2
        return out if self.bias is None else out + self.bias

    def message(self, x_j, norm):
        return norm.view(-1, 1) * x_j


pyg_conv.ChebConv = ChebConv
torch.set_default_dtype(torch.float64)
sys.path.insert(0, REF)
import networks as ref_networks  # noqa: E402  (the reference's file, unmodified)

sys.path.insert(0, PKG)
import synthetic  # noqa: E402


def masked_x(feats, seed):
    g = torch.Generator().manual_seed(seed)
    node_type = torch.randint(0, 4, (feats.shape[0],), generator=g)
    return node_type, torch.cat([torch.nn.functional.one_hot(node_type, 4).to(feats.dtype), feats, (feats != 0).to(feats.dtype)], dim=1)


def conditions_hold():
    """The conditions on the inputs, for every ChebConv call of the case: no tie at the arg-max, a positive lambda_max."""
    for ent, lam in LAMBDAS:
        top = torch.sort(ent, descending=True).values[:2]
        if not (lam > 0 and float(top[0] - top[1]) >= 1e-3 * abs(float(top[0]))):
            return False
    return True


def run(name, feats, ei, ea, seed=0, **kw):
    """The case with the first of seed, seed + 100, ... whose weights meet the conditions (a doubled graph ties the two directions
    of an edge exactly, so the arg-max has to be a degree)."""
    for s in range(seed, seed + 3000, 100):
        if run_seed(name, feats, ei, ea, seed=s, **kw):
            return
    raise AssertionError(f"{name}: no seed meets the conditions")


def f32(t):
    """Values a float32 holds exactly (parameters, jitter, output gradient: the fp32 path then starts from the same numbers)."""
    return t.float().double()


def f16(t):
    """The same with float16 (jitter, output gradient: half the bytes in the fixture)."""
    return t.half().double()


def run_seed(name, feats, ei, ea, dim_hid=32, n_gnn_layers=3, K=2, dim_out=2, seed=0, batch_name="", with_dx=True):
    node_type, x = masked_x(feats, 1000 + seed)
    jitter = f16((torch.rand(ea.shape[0], 2, generator=torch.Generator().manual_seed(3000 + seed)) * 2 - 1) * 0.25)
    ea5 = ea[:, EA_COLS].clone()
    ea5[:, :2] += jitter
    net = ref_networks.MultiConvNet(8, 5, dim_out, dim_hid, n_gnn_layers, K, 0.0)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in net.named_parameters():
            a = 0.2 if k.endswith("bias") else (0.5 if k.startswith("edge_trans") else 0.35)
            p.copy_(f32((torch.rand(p.shape, generator=g) * 2 - 1) * a))
    del LAMBDAS[:]
    xin = x.clone().requires_grad_(True)
    out = net(types.SimpleNamespace(x=xin, edge_index=ei, edge_attr=ea5))
    if not conditions_hold():
        return False
    for ent, lam in LAMBDAS:
        top = torch.sort(ent, descending=True).values[:2]
        assert lam > 0, (name, lam)
        assert float(top[0] - top[1]) >= 1e-3 * abs(float(top[0])), (name, top)
    gout = f16(torch.randn(out.shape, generator=torch.Generator().manual_seed(2000 + seed)))
    out.backward(gout)
    arrays = {f"param/{k}": v.clone() for k, v in net.state_dict().items()}
    # (K = 1: the edge weights do not reach the output and autograd leaves edge_trans without a gradient: stored as zeros)
    arrays.update({f"grad/{k}": (p.grad.clone() if p.grad is not None else torch.zeros_like(p)) for k, p in net.named_parameters()})
    arrays.update(out=out.detach().clone(), gout=gout.half())
    arrays.update({k: v.float() for k, v in arrays.items() if k.startswith("param/")})
    if with_dx:
        arrays["dx"] = xin.grad[:, 4:12].clone()
    assert float(xin.grad[:, :4].abs().max()) == 0 and float(xin.grad[:, 12:].abs().max()) == 0
    if batch_name:
        arrays.update(node_type=node_type.to(torch.int8), ea_cols=torch.tensor(EA_COLS), ea_jitter=jitter.half())
    else:
        arrays.update(x=x, edge_index=ei, edge_attr=ea5)
    path = os.path.join(HERE, f"case_{name}.npz")
    np.savez_compressed(path, seed=np.int64(seed), keys=np.array(list(net.state_dict())), batch=np.array(batch_name), dim_featn=np.int64(8), dim_feate=np.int64(5),
                        dim_out=np.int64(dim_out), dim_hid=np.int64(dim_hid), n_gnn_layers=np.int64(n_gnn_layers), K=np.int64(K),
                        **{k: v.detach().numpy() for k, v in arrays.items()})
    kb = os.path.getsize(path) / 1024
    assert kb < 100, (name, kb)
    print(f"wrote case_{name}.npz: seed {seed}, {kb:.1f} KiB, lambda_max {sorted({round(l, 6) for _, l in LAMBDAS})}")
    return True


def syn(grids, B, seed):
    b = synthetic.make_batch(grids, B, seed=seed)
    return b["x"][:, :8].double(), b["edge_index"], b["edge_attr"].double()


def main():
    z = np.load(os.path.join(HERE, "cigre14_real64.npz"))
    run("multiconv_real64", torch.from_numpy(z["x"])[:, :8].double(), torch.from_numpy(z["edge_index"]), torch.from_numpy(z["edge_attr"]).double(),
        seed=71, batch_name="cigre14_real64.npz", with_dx=False)
    small = syn(["cigre14"], 3, 61)
    run("multiconv_k3", *small, dim_hid=16, K=3, seed=72)
    run("multiconv_k4", *small, dim_hid=16, K=4, seed=73)
    run("multiconv_k1", *small, K=1, seed=74)
    run("multiconv_h8", *small, dim_hid=8, seed=75)
    run("multiconv_h16", *small, dim_hid=16, seed=76)
    f, ei, ea = small
    run("multiconv_undirected", f, torch.cat([ei, ei.flip(0)], dim=1), torch.cat([ea, ea], dim=0), seed=77)
    run("multiconv_mixed", *syn(["cigre14", "ober_sub"], 2, 62), dim_hid=16, seed=78)
    run("multiconv_l1", *small, dim_hid=8, dim_out=8, n_gnn_layers=1, K=3, seed=79)


if __name__ == "__main__":
    main()
