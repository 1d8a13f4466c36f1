"""Restatement of the reference's MultiConvNet / WrappedMultiConv (/root/reference/networks.py:737-835) and PyG's ChebConv
(2.3 - 2.6, normalization=None) with get_laplacian, in plain torch (differentiable, any float dtype).  Parameters come as a
state_dict with the reference's keys; dropout masks are explicit ([N, C] multipliers per layer, or None)."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDENS = ["multiconv_real64", "multiconv_k3", "multiconv_k4", "multiconv_k1", "multiconv_h8", "multiconv_h16",
           "multiconv_undirected", "multiconv_mixed", "multiconv_l1"]


def load_golden(name):
    """case_<name>.npz (tests/golden/make_multiconv_goldens.py: the reference's MultiConvNet forward and the backward of a seeded
    output gradient, in float64): (arrays with the batch, params, grads, the state_dict keys in order, the constructor arguments)."""
    z = np.load(os.path.join(GOLDEN, f"case_{name}.npz"), allow_pickle=False)
    t = {k: torch.from_numpy(z[k]) for k in z.files if z[k].dtype.kind in "fi" and z[k].ndim > 0}
    t = {k: (v.double() if v.is_floating_point() else v.long()) for k, v in t.items()}      # (float32 arrays hold the fp64 run's values exactly)
    src = str(z["batch"])
    if src:
        g = np.load(os.path.join(GOLDEN, src))
        t["edge_index"], t["edge_attr"] = torch.from_numpy(g["edge_index"]), torch.from_numpy(g["edge_attr"])[:, t["ea_cols"]].double()
        t["edge_attr"][:, :2] += torch.from_numpy(z["ea_jitter"]).double()
        feats = torch.from_numpy(g["x"])[:, :8].double()      # x is rebuilt from the fixture's features and the stored node types
        t["x"] = torch.cat([torch.nn.functional.one_hot(t["node_type"], 4).double(), feats, (feats != 0).double()], dim=1)
    params = {k[len("param/"):]: v for k, v in t.items() if k.startswith("param/")}
    grads = {k[len("grad/"):]: v for k, v in t.items() if k.startswith("grad/")}
    args = tuple(int(z[k]) for k in ("dim_featn", "dim_feate", "dim_out", "dim_hid", "n_gnn_layers", "K")) + (0.0,)
    return t, params, grads, [str(k) for k in z["keys"]], args


def is_directed(edge_index):
    """The reference's rule: is there NO edge (v0 -> u0) among the edges leaving v0, (u0 -> v0) the first edge?"""
    return not bool((edge_index[1, edge_index[0] == edge_index[1, 0]] == edge_index[0, 0]).any())


def laplacian_entries(edge_index, w, n):
    """get_laplacian(normalization=None) without the index bookkeeping: self loops dropped, deg over the SOURCE; returns the kept
    (src, dst) and the entries [-w_e ..., deg_i ...]."""
    keep = edge_index[0] != edge_index[1]
    src, dst, w = edge_index[0][keep], edge_index[1][keep], w[keep]
    deg = torch.zeros(n, dtype=w.dtype).index_add(0, src, w)
    return src, dst, torch.cat([-w, deg])


def cheb_conv(x, edge_index, w, lins, bias=None, lambda_max=None):
    """PyG ChebConv.forward(x, edge_index, edge_weight=w, lambda_max=lambda_max) with weights lins[k] [out, in]."""
    n = x.size(0)
    if w is None:
        w = torch.ones(edge_index.size(1), dtype=x.dtype)
    src, dst, ent = laplacian_entries(edge_index, w, n)
    lam = 2.0 * ent.max() if lambda_max is None else torch.as_tensor(lambda_max, dtype=x.dtype)
    ent = (2.0 * ent) / lam
    ent = torch.where(ent == float("inf"), torch.zeros_like(ent), ent)
    what, d = ent[:src.numel()], ent[src.numel():] - 1.0

    def A(t):
        return d[:, None] * t + torch.zeros_like(t).index_add(0, dst, what[:, None] * t[src])

    t0, out = x, x @ lins[0].T
    if len(lins) > 1:
        t1 = A(x)
        out = out + t1 @ lins[1].T
        for W in lins[2:]:
            t2 = 2.0 * A(t1) - t0
            out = out + t2 @ W.T
            t0, t1 = t1, t2
    return out if bias is None else out + bias


def wrapped(sd, prefix, x, edge_index, weights, lambda_max=None):
    """WrappedMultiConv: the sum of its convs, conv f on weights[f]."""
    out = 0.0
    for f, w in enumerate(weights):
        k = f"{prefix}convs.{f}."
        lins = [sd[f"{k}lins.{m}.weight"] for m in range(sum(1 for q in sd if q.startswith(k + "lins.")))]
        out = out + cheb_conv(x, edge_index, w, lins, sd.get(k + "bias"), lambda_max)
    return out


def multiconv(sd, x, edge_index, edge_attr, masks=None):
    """MultiConvNet.forward on data.x = x ([N, 4 + featn + featn]); masks[l]: the dropout multipliers after layer l, or None."""
    n_layers = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("convs."))
    featn = sd["convs.0.convs.0.lins.0.weight"].shape[1]
    h = x[:, 4:4 + featn]
    ea = edge_attr[:, :2]
    if is_directed(edge_index):
        edge_index, ea = torch.cat([edge_index, edge_index.flip(0)], dim=1), torch.cat([ea, ea], dim=0)
    z = torch.relu(ea @ sd["edge_trans.0.weight"].T + sd["edge_trans.0.bias"])
    feat = ea + z @ sd["edge_trans.2.weight"].T + sd["edge_trans.2.bias"]
    for l in range(n_layers):
        h = wrapped(sd, f"convs.{l}.", h, edge_index, [feat[:, 0], feat[:, 1]])
        if l < n_layers - 1:
            if masks is not None and masks[l] is not None:
                h = h * masks[l]
            h = torch.relu(h)
    return h
