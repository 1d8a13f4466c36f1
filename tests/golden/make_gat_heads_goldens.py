#!/usr/bin/env python3
"""Generate tests/golden/case_gat_heads4_mean.npz by running the REFERENCE's GAT_DSSE (networks.py:113-156) with
heads = 4, concat = False, num_layers = 3, its gsp_wls_edge and backward, in float64, on the 64 real CIGRE-14 graphs.

As tests/golden/make_gat_goldens.py does for one head: torch_geometric is not installed, so the reference's imports come from the
stand-in in tests/golden/_pyg_standin, and THIS process installs restatements of PyG 2.3-2.6's ``GATv2Conv`` (here with several
heads: lin_l / lin_r / lin_edge to H * C columns viewed [., H, C], att [1, H, C], softmax per head, the heads concatenated or, with
concat=False, averaged before the bias) and ``Sequential`` before importing the reference's unmodified networks.py / data.py.
What the fixture pins is the reference's own wiring: how GAT_DSSE hands heads and concat to its convs, its Sequential order, its
Linears and its loss.  Runs only where the reference checkout exists.  Outputs are data only; same arrays as case_gat_real64.npz
plus heads and concat.

    python tests/golden/make_gat_heads_goldens.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
REG = {"mu_v": 1e-1, "mu_theta": 1e-1, "lam_v": 1e-4, "lam_p": 1e-8, "lam_pf": 1e-6, "lam_reg": 1e2}

sys.path.insert(0, os.path.join(HERE, "_pyg_standin"))
import torch_geometric.nn as pyg_nn          # noqa: E402  (stand-in)
import torch_geometric.nn.conv as pyg_conv   # noqa: E402  (stand-in)


class GATv2Conv(nn.Module):
    """PyG 2.3-2.6 GATv2Conv with H heads, dropout = 0, fill_value = 'mean'."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0, add_self_loops=True,
                 edge_dim=None, fill_value="mean", bias=True, share_weights=False, **kwargs):
        super().__init__()
        assert dropout == 0.0 and fill_value == "mean" and not share_weights
        self.heads, self.out_channels, self.concat = heads, out_channels, concat
        self.negative_slope, self.add_self_loops = negative_slope, add_self_loops
        self.lin_l = nn.Linear(in_channels, heads * out_channels, bias=bias)
        self.lin_r = nn.Linear(in_channels, heads * out_channels, bias=bias)
        self.att = nn.Parameter(torch.empty(1, heads, out_channels))
        self.lin_edge = nn.Linear(edge_dim, heads * out_channels, bias=False) if edge_dim is not None else None
        self.bias = nn.Parameter(torch.zeros(heads * out_channels if concat else out_channels)) if bias else None
        nn.init.uniform_(self.att, -0.5, 0.5)

    def forward(self, x, edge_index, edge_attr=None):
        n, H, C = x.size(0), self.heads, self.out_channels
        x_l, x_r = self.lin_l(x).view(n, H, C), self.lin_r(x).view(n, H, C)
        if self.add_self_loops:
            keep = edge_index[0] != edge_index[1]                                 # remove_self_loops
            edge_index = edge_index[:, keep]
            if edge_attr is not None:
                edge_attr = edge_attr[keep]
                s = torch.zeros(n, edge_attr.size(1)).index_add_(0, edge_index[1], edge_attr)
                c = torch.zeros(n).index_add_(0, edge_index[1], torch.ones(edge_index.size(1)))
                edge_attr = torch.cat([edge_attr, s / c.clamp(min=1).unsqueeze(1)], 0)      # fill_value='mean', 0 where empty
            loop = torch.arange(n)
            edge_index = torch.cat([edge_index, torch.stack([loop, loop])], 1)   # add_self_loops
        j, i = edge_index[0], edge_index[1]
        z = x_l[j] + x_r[i]
        if edge_attr is not None and self.lin_edge is not None:
            z = z + self.lin_edge(edge_attr).view(-1, H, C)
        e = (F.leaky_relu(z, self.negative_slope) * self.att).sum(-1)            # [E, H]
        idx = i.unsqueeze(1).expand(-1, H)
        m = torch.full((n, H), float("-inf")).scatter_reduce(0, idx, e, "amax", include_self=True)     # torch_geometric.utils.softmax
        p = (e - m[i]).exp()
        alpha = p / (torch.zeros(n, H).index_add_(0, i, p)[i] + 1e-16)
        out = torch.zeros(n, H, C).index_add_(0, i, alpha.unsqueeze(-1) * x_l[j])
        out = out.view(n, H * C) if self.concat else out.mean(dim=1)
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

HEAD_SCALES = (1.5, 0.4, 2.5, 0.9)      # att magnitude per head


def seeded_weights(model, seed):
    g = torch.Generator().manual_seed(seed)
    scale = {"bias": 0.2, "lin_l.weight": 0.6, "lin_l.bias": 0.3, "lin_r.weight": 0.6, "lin_r.bias": 0.3, "lin_edge.weight": 0.6}
    with torch.no_grad():
        for k, p in model.state_dict().items():
            r = torch.rand(p.shape, generator=g) * 2 - 1
            if k.endswith(".att"):
                p.copy_(r * torch.tensor(HEAD_SCALES[:p.size(1)]).view(1, -1, 1))
            else:
                p.copy_(r * next((v for s, v in scale.items() if k.endswith("." + s)), 0.35 if k.endswith("weight") else 0.2))


def main():
    z = np.load(os.path.join(HERE, "cigre14_real64.npz"))
    b = {k: torch.from_numpy(z[k]).double() if z[k].dtype.kind == "f" else torch.from_numpy(z[k]) for k in z.files}
    heads, num_layers, nonlin = 4, 3, "leaky_relu"
    model = ref_networks.GAT_DSSE(dim_feat=8, dim_dense=32, dim_out=2, heads=heads, concat=False, num_layers=num_layers, edge_dim=6,
                                  nonlin=nonlin)
    seeded_weights(model, 11)
    x, ei, ea = b["x"], b["edge_index"], b["edge_attr"]
    st = (b["x_mean"], b["x_std"], b["edge_mean"], b["edge_std"])
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
    path = os.path.join(HERE, "case_gat_heads4_mean.npz")
    np.savez_compressed(path, keys=np.array(keys), num_layers=np.int64(num_layers), nonlin=np.array(nonlin), heads=np.int64(heads),
                        concat=np.int64(0), **{k: v.detach().numpy() for k, v in arrays.items()})
    print(f"wrote case_gat_heads4_mean.npz: {os.path.getsize(path) / 1024:.1f} KiB, loss {loss.item():.6g}")


if __name__ == "__main__":
    main()
