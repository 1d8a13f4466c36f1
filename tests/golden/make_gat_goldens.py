#!/usr/bin/env python3
"""Generate tests/golden/case_gat_*.npz by running the REFERENCE's GAT_DSSE (networks.py:113-156), gsp_wls_edge and backward.

Runs only where the reference checkout exists (REF below).  torch_geometric is not installed, so the reference's imports come
from the stand-in in tests/golden/_pyg_standin; its GATv2Conv and Sequential are placeholders there, and THIS process installs
restatements of PyG 2.3-2.6's ``GATv2Conv`` (heads = 1: remove_self_loops -> add_self_loops(fill_value='mean') -> lin_l / lin_r /
lin_edge -> leaky_relu -> att -> softmax(max-subtracted, / (sum + 1e-16)) -> sum of alpha * x_l[j] -> + bias) and ``Sequential``
(children ``module_{i}``, conv entries called with (x, edge_index, edge_attr), the others with x) into the stand-in's module
objects before importing the reference's unmodified networks.py / data.py.  Everything runs in float64 (default dtype), so the
fixtures are the reference's arithmetic without fp32 rounding.  Outputs are data only.

    python tests/golden/make_gat_goldens.py

Cases (explicit seeded weights, WLS loss of dss2_run.py:104-112):
    case_gat_real64.npz       the 64 real CIGRE-14 graphs of cigre14_real64.npz, the driver's GAT_DSSE(8, 32, 2, 8, 6)
    case_gat_reswitched.npz   a reswitched CIGRE batch (its graphs have a cycle)
    case_gat_ober.npz         an ober_sub batch
    case_gat_mixed.npz        CIGRE and reswitched graphs in one batch
    case_gat_tanh_l2.npz      nonlin='tanh', num_layers=2 on the real batch
Arrays: x, edge_index, edge_attr, x_mean, x_std, edge_mean, edge_std, param/<key>, out (before the loss's in-place slack mask),
loss, grad/<key>, keys (the reference's state_dict key list, in order), num_layers, nonlin.
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
PKG = os.path.join(ROOT, "deep-statistical-solver-for-distribution-system-state-estimation_amd")
REG = {"mu_v": 1e-1, "mu_theta": 1e-1, "lam_v": 1e-4, "lam_p": 1e-8, "lam_pf": 1e-6, "lam_reg": 1e2}

sys.path.insert(0, os.path.join(HERE, "_pyg_standin"))
import torch_geometric.nn as pyg_nn          # noqa: E402  (stand-in)
import torch_geometric.nn.conv as pyg_conv   # noqa: E402  (stand-in)


class GATv2Conv(nn.Module):
    """PyG 2.3-2.6 GATv2Conv, heads = 1, concat = True, dropout = 0, fill_value = 'mean' (what GAT_DSSE builds)."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0, add_self_loops=True,
                 edge_dim=None, fill_value="mean", bias=True, share_weights=False, **kwargs):
        super().__init__()
        assert heads == 1 and dropout == 0.0 and fill_value == "mean" and not share_weights
        self.negative_slope, self.add_self_loops = negative_slope, add_self_loops
        self.lin_l = nn.Linear(in_channels, out_channels, bias=bias)
        self.lin_r = nn.Linear(in_channels, out_channels, bias=bias)
        self.att = nn.Parameter(torch.empty(1, heads, out_channels))
        self.lin_edge = nn.Linear(edge_dim, out_channels, bias=False) if edge_dim is not None else None
        self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None
        nn.init.uniform_(self.att, -0.5, 0.5)

    def forward(self, x, edge_index, edge_attr=None):
        n = x.size(0)
        x_l, x_r = self.lin_l(x), self.lin_r(x)
        if self.add_self_loops:
            keep = edge_index[0] != edge_index[1]                                 # remove_self_loops
            edge_index = edge_index[:, keep]
            if edge_attr is not None:
                edge_attr = edge_attr[keep]
                s = torch.zeros(n, edge_attr.size(1)).index_add_(0, edge_index[1], edge_attr)
                c = torch.zeros(n).index_add_(0, edge_index[1], torch.ones(edge_index.size(1)))
                fill = s / c.clamp(min=1).unsqueeze(1)                            # scatter(..., reduce='mean'), 0 where empty
                edge_attr = torch.cat([edge_attr, fill], 0)
            loop = torch.arange(n)
            edge_index = torch.cat([edge_index, torch.stack([loop, loop])], 1)   # add_self_loops
        j, i = edge_index[0], edge_index[1]
        z = x_l[j] + x_r[i]
        if edge_attr is not None and self.lin_edge is not None:
            z = z + self.lin_edge(edge_attr)
        e = (F.leaky_relu(z, self.negative_slope) * self.att.view(1, -1)).sum(-1)
        m = torch.full((n,), float("-inf")).scatter_reduce(0, i, e, "amax", include_self=True)     # torch_geometric.utils.softmax
        p = (e - m[i]).exp()
        alpha = p / (torch.zeros(n).index_add_(0, i, p)[i] + 1e-16)
        out = torch.zeros(n, x_l.size(1)).index_add_(0, i, alpha.unsqueeze(1) * x_l[j])
        return out + self.bias if self.bias is not None else out


class Sequential(nn.Module):
    """PyG Sequential('x, edge_index, edge_attr', [...]): (module, 'x, edge_index, edge_attr -> x') tuples and plain modules."""

    def __init__(self, input_args, modules):
        super().__init__()
        self._calls = []
        for k, entry in enumerate(modules):
            mod, graph = (entry[0], True) if isinstance(entry, tuple) else (entry, False)
            setattr(self, f"module_{k}", mod)
            self._calls.append((f"module_{k}", graph))

    def forward(self, x, edge_index, edge_attr):
        for name, graph in self._calls:
            mod = getattr(self, name)
            x = mod(x, edge_index, edge_attr) if graph else mod(x)
        return x


pyg_conv.GATv2Conv = GATv2Conv
pyg_nn.Sequential = Sequential
torch.set_default_dtype(torch.float64)
sys.path.insert(0, REF)
import networks as ref_networks  # noqa: E402  (the reference's file, unmodified)
import data as ref_data          # noqa: E402  (the reference's file, unmodified)

sys.path.insert(0, PKG)
import synthetic  # noqa: E402


def seeded_weights(model, seed):
    g = torch.Generator().manual_seed(seed)
    scale = {"att": 1.5, "bias": 0.2, "lin_l.weight": 0.6, "lin_l.bias": 0.3, "lin_r.weight": 0.6, "lin_r.bias": 0.3,
             "lin_edge.weight": 0.6}
    with torch.no_grad():
        for k, p in model.state_dict().items():
            a = next((v for s, v in scale.items() if k.endswith("." + s)), 0.35 if k.endswith("weight") else 0.2)
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * a)


def batch64(b):
    return {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in b.items()}


def run(name, batch, num_layers=8, nonlin="leaky_relu", seed=0):
    model = ref_networks.GAT_DSSE(dim_feat=8, dim_dense=32, dim_out=2, heads=1, num_layers=num_layers, edge_dim=6, nonlin=nonlin)
    seeded_weights(model, seed)
    x, ei, ea, st = batch["x"], batch["edge_index"], batch["edge_attr"], batch["stats"]
    keys = list(model.state_dict())
    arrays = {f"param/{k}": v.clone() for k, v in model.state_dict().items()}
    arrays.update(x=x, edge_index=ei, edge_attr=ea, x_mean=st[0], x_std=st[1], edge_mean=st[2], edge_std=st[3])
    out = model(x[:, :8], ei, ea[:, :6])
    arrays["out"] = out.detach().clone()
    loss = ref_data.gsp_wls_edge(input=x[:, :8], edge_input=ea[:, :6], output=out, x_mean=st[0], x_std=st[1], edge_mean=st[2],
                                 edge_std=st[3], edge_index=ei, reg_coefs=REG, num_samples=None, node_param=x[:, 8:],
                                 edge_param=ea[:, 6:])
    loss.backward()
    arrays["loss"] = loss.detach().clone()
    for k, p in model.named_parameters():
        arrays[f"grad/{k}"] = p.grad.clone()
    path = os.path.join(HERE, f"case_{name}.npz")
    np.savez_compressed(path, keys=np.array(keys), num_layers=np.int64(num_layers), nonlin=np.array(nonlin),
                        **{k: v.detach().numpy() for k, v in arrays.items()})
    print(f"wrote case_{name}.npz: {os.path.getsize(path) / 1024:.1f} KiB, loss {loss.item():.6g}")


def main():
    z = np.load(os.path.join(HERE, "cigre14_real64.npz"))
    real = {k: torch.from_numpy(z[k]).double() if z[k].dtype.kind == "f" else torch.from_numpy(z[k]) for k in z.files}
    real["stats"] = (real["x_mean"], real["x_std"], real["edge_mean"], real["edge_std"])
    run("gat_real64", real, seed=1)
    run("gat_reswitched", batch64(synthetic.make_batch(["cigre14_reswitched"], 8, seed=41)), seed=2)
    run("gat_ober", batch64(synthetic.make_batch(["ober_sub"], 4, seed=42)), seed=3)
    run("gat_mixed", batch64(synthetic.make_batch(["cigre14", "cigre14_reswitched"], 16, seed=43)), seed=4)
    run("gat_tanh_l2", real, num_layers=2, nonlin="tanh", seed=5)


if __name__ == "__main__":
    main()
