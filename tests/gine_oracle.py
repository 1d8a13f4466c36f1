"""fp64 restatement of PyG 2.3-2.6's GINEConv (nn = one Linear) and of the reference's GINE_DSSE wiring (networks.py:71-111).

Plain torch, no PyG and no reference import.  One layer, j = edge_index[0] the source, i = edge_index[1] the target, edges as given:
    out_i = nn( sum_{e: j->i} relu(x_j + lin(ea_e)) + (1 + eps) x_i )       (without lin: relu(x_j + ea_e))
GINE_DSSE shares ONE nn Linear between all its convs: gine_dsse reads it once (``nn.weight`` / ``nn.bias``), so autograd through it
gives the summed gradient that ``named_parameters()`` reports.
"""
import torch
import torch.nn.functional as F

NONLINS = {"leaky_relu": lambda v: F.leaky_relu(v, 0.01), "relu": torch.relu, "tanh": torch.tanh}


def gine(x, edge_index, edge_attr, Wn, bn, eps, We=None, be=None):
    src, tgt = edge_index[0], edge_index[1]
    e = edge_attr if We is None else edge_attr @ We.t() + be
    msg = (x[src] + e).relu()
    agg = torch.zeros(x.size(0), x.size(1), dtype=x.dtype).index_add(0, tgt, msg)
    return (agg + (1 + eps) * x) @ Wn.t() + bn


def gine_dsse(x, edge_index, edge_attr, sd, num_layers, nonlin="leaky_relu"):
    """The reference's GINE_DSSE forward from a state_dict with its keys (nn.*, model.module_{i}.*)."""
    h = x
    act = NONLINS[nonlin]
    for k in range(num_layers - 1):
        p = f"model.module_{2 * k}."
        h = act(gine(h, edge_index, edge_attr, sd["nn.weight"], sd["nn.bias"], sd[p + "eps"], sd.get(p + "lin.weight"),
                     sd.get(p + "lin.bias")))
    i = 2 * (num_layers - 1)
    h = h @ sd[f"model.module_{i}.weight"].t() + sd[f"model.module_{i}.bias"]
    return h @ sd[f"model.module_{i + 1}.weight"].t() + sd[f"model.module_{i + 1}.bias"]


def state_dict_keys(num_layers, edge_dim=True):
    keys = ["nn.weight", "nn.bias"]
    for k in range(num_layers - 1):
        keys += [f"model.module_{2 * k}.{s}" for s in ("eps", "nn.weight", "nn.bias")]
        if edge_dim:
            keys += [f"model.module_{2 * k}.lin.weight", f"model.module_{2 * k}.lin.bias"]
    i = 2 * (num_layers - 1)
    keys += [f"model.module_{i}.weight", f"model.module_{i}.bias", f"model.module_{i + 1}.weight", f"model.module_{i + 1}.bias"]
    return keys


def parameter_names(num_layers, train_eps=False, edge_dim=True):
    """named_parameters() of GINE_DSSE: the shared nn once, under its first owner's name."""
    names = ["nn.weight", "nn.bias"]
    for k in range(num_layers - 1):
        if train_eps:
            names.append(f"model.module_{2 * k}.eps")
        if edge_dim:
            names += [f"model.module_{2 * k}.lin.weight", f"model.module_{2 * k}.lin.bias"]
    i = 2 * (num_layers - 1)
    return names + [f"model.module_{i}.weight", f"model.module_{i}.bias", f"model.module_{i + 1}.weight", f"model.module_{i + 1}.bias"]


def unique_params(sd):
    """A state_dict with the shared nn's copies (model.module_{2k}.nn.*) dropped: one tensor per parameter."""
    return {k: v for k, v in sd.items() if ".nn." not in k}


def random_state_dict(num_layers, c=8, dense=32, out=2, ed=6, eps=0.0, seed=0):
    """Seeded explicit weights with the reference's keys; the shared nn appears under every owner (the same tensor)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, a=1.0: (torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) * a  # noqa: E731
    sd = {"nn.weight": r(c, c, a=0.6), "nn.bias": r(c, a=0.2)}
    for k in range(num_layers - 1):
        p = f"model.module_{2 * k}."
        sd[p + "eps"] = torch.full((1,), float(eps), dtype=torch.float64)
        sd[p + "nn.weight"], sd[p + "nn.bias"] = sd["nn.weight"], sd["nn.bias"]
        if ed:
            sd[p + "lin.weight"] = r(c, ed, a=0.5)
            sd[p + "lin.bias"] = r(c, a=0.3)
    i = 2 * (num_layers - 1)
    sd[f"model.module_{i}.weight"] = r(dense, c, a=0.35)
    sd[f"model.module_{i}.bias"] = r(dense, a=0.2)
    sd[f"model.module_{i + 1}.weight"] = r(out, dense, a=0.18)
    sd[f"model.module_{i + 1}.bias"] = r(out, a=0.1)
    return {k: sd[k] for k in state_dict_keys(num_layers, bool(ed))}
