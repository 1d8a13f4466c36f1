"""fp64 restatement of PyG 2.3-2.6's GATv2Conv (heads = 1) and of the reference's GAT_DSSE wiring (networks.py:113-156).

Plain torch, no PyG and no reference import: remove_self_loops -> add_self_loops(fill_value='mean') -> lin_l / lin_r ->
e = att . leaky_relu(x_r[i] + x_l[j] + lin_edge(ea)) -> PyG softmax (subtract the group max, exp, / (sum + 1e-16)) ->
sum of alpha * x_l[j] per target -> + bias.  Autograd through it gives the reference gradients.
"""
import torch
import torch.nn.functional as F

NONLINS = {"leaky_relu": lambda v: F.leaky_relu(v, 0.01), "relu": torch.relu, "tanh": torch.tanh}


def self_loops(edge_index, edge_attr, n, add_self_loops=True):
    """(src, tgt, ea) after PyG's remove_self_loops + add_self_loops(fill_value='mean'); unchanged without add_self_loops."""
    src, tgt = edge_index[0], edge_index[1]
    if not add_self_loops:
        return src, tgt, edge_attr
    keep = src != tgt
    src, tgt = src[keep], tgt[keep]
    loop = torch.arange(n, dtype=src.dtype)
    ea = None
    if edge_attr is not None:
        ea = edge_attr[keep]
        s = torch.zeros(n, ea.size(1), dtype=ea.dtype).index_add(0, tgt, ea)
        cnt = torch.zeros(n, dtype=ea.dtype).index_add(0, tgt, torch.ones_like(tgt, dtype=ea.dtype))
        fill = s / cnt.clamp(min=1).unsqueeze(1)
        ea = torch.cat([ea, fill], 0)
    return torch.cat([src, loop]), torch.cat([tgt, loop]), ea


def pyg_softmax(e, index, n):
    m = torch.full((n,), float("-inf"), dtype=e.dtype).scatter_reduce(0, index, e, "amax", include_self=True)
    p = (e - m[index]).exp()
    s = torch.zeros(n, dtype=e.dtype).index_add(0, index, p)
    return p / (s[index] + 1e-16)


def gatv2(x, edge_index, edge_attr, p, slope=0.2, add_self_loops=True, return_alpha=False):
    """p: dict with att [1,1,C] (or [C]), bias [C] or None, Wl, bl, Wr, br, We [C, ed] or None."""
    n = x.size(0)
    src, tgt, ea = self_loops(edge_index, edge_attr, n, add_self_loops)
    xl = x @ p["Wl"].t() + (p["bl"] if p.get("bl") is not None else 0.0)
    xr = x @ p["Wr"].t() + (p["br"] if p.get("br") is not None else 0.0)
    z = xr[tgt] + xl[src]
    if p.get("We") is not None:
        z = z + ea @ p["We"].t()
    e = (F.leaky_relu(z, slope) * p["att"].reshape(-1)).sum(-1)
    alpha = pyg_softmax(e, tgt, n)
    out = torch.zeros(n, xl.size(1), dtype=x.dtype).index_add(0, tgt, alpha.unsqueeze(1) * xl[src])
    if p.get("bias") is not None:
        out = out + p["bias"]
    return (out, alpha) if return_alpha else out


def conv_params(sd, prefix):
    g = lambda k: sd.get(prefix + k)  # noqa: E731
    return {"att": g("att"), "bias": g("bias"), "Wl": g("lin_l.weight"), "bl": g("lin_l.bias"), "Wr": g("lin_r.weight"),
            "br": g("lin_r.bias"), "We": g("lin_edge.weight")}


def gat_dsse(x, edge_index, edge_attr, sd, num_layers, nonlin="leaky_relu", slope=0.2, add_self_loops=True):
    """The reference's GAT_DSSE forward from a state_dict with its keys (model.module_{i}.*)."""
    h = x
    act = NONLINS[nonlin]
    for k in range(num_layers - 1):
        h = act(gatv2(h, edge_index, edge_attr, conv_params(sd, f"model.module_{2 * k}."), slope, add_self_loops))
    i = 2 * (num_layers - 1)
    h = h @ sd[f"model.module_{i}.weight"].t() + sd[f"model.module_{i}.bias"]
    return h @ sd[f"model.module_{i + 1}.weight"].t() + sd[f"model.module_{i + 1}.bias"]


def state_dict_keys(num_layers, edge_dim=True):
    keys = []
    for k in range(num_layers - 1):
        keys += [f"model.module_{2 * k}.{s}" for s in ("att", "bias", "lin_l.weight", "lin_l.bias", "lin_r.weight", "lin_r.bias")]
        if edge_dim:
            keys.append(f"model.module_{2 * k}.lin_edge.weight")
    i = 2 * (num_layers - 1)
    keys += [f"model.module_{i}.weight", f"model.module_{i}.bias", f"model.module_{i + 1}.weight", f"model.module_{i + 1}.bias"]
    return keys


def random_state_dict(num_layers, c=8, dense=32, out=2, ed=6, seed=0, scale=1.0):
    """Seeded explicit weights (att large enough that the attention is far from uniform)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, a=1.0: ((torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) * a * scale)  # noqa: E731
    sd = {}
    for k in range(num_layers - 1):
        p = f"model.module_{2 * k}."
        sd[p + "att"] = r(1, 1, c, a=1.5)
        sd[p + "bias"] = r(c, a=0.2)
        sd[p + "lin_l.weight"] = r(c, c, a=0.6)
        sd[p + "lin_l.bias"] = r(c, a=0.3)
        sd[p + "lin_r.weight"] = r(c, c, a=0.6)
        sd[p + "lin_r.bias"] = r(c, a=0.3)
        if ed:
            sd[p + "lin_edge.weight"] = r(c, ed, a=0.6)
    i = 2 * (num_layers - 1)
    sd[f"model.module_{i}.weight"] = r(dense, c, a=0.35)
    sd[f"model.module_{i}.bias"] = r(dense, a=0.2)
    sd[f"model.module_{i + 1}.weight"] = r(out, dense, a=0.18)
    sd[f"model.module_{i + 1}.bias"] = r(out, a=0.1)
    return sd
