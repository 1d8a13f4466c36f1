"""fp64 restatement of PyG 2.3-2.6's GATv2Conv with several heads and of GAT_DSSE built on its head mean (concat=False), in the
style of tests/gat_oracle.py, whose ``self_loops`` and ``pyg_softmax`` it uses.

With H heads of C channels: lin_l / lin_r / lin_edge map to H * C columns, rows h * C .. h * C + C - 1 are head h's, att is
[1, H, C].  Per head: e = att[h] . leaky_relu(x_r[i] + x_l[j] + lin_edge(ea)), PyG softmax over a target's incoming edges,
out = sum of alpha * x_l[j].  concat=True: the heads side by side [N, H * C] + bias [H * C]; concat=False: their mean [N, C]
+ bias [C].  At H = 1 this is ``gat_oracle.gatv2``.  Plain torch; autograd through it gives the reference gradients.
"""
import torch
import torch.nn.functional as F

from gat_oracle import NONLINS, conv_params, pyg_softmax, self_loops


def gatv2_heads(x, edge_index, edge_attr, p, heads, concat=True, slope=0.2, add_self_loops=True):
    """p: dict with att [1, H, C], bias [H * C] / [C] (concat=False) or None, Wl, Wr [H * C, cin], bl, br [H * C] or None,
    We [H * C, ed] or None."""
    n, H = x.size(0), heads
    C = p["Wl"].size(0) // H
    src, tgt, ea = self_loops(edge_index, edge_attr, n, add_self_loops)
    xl = (x @ p["Wl"].t() + (p["bl"] if p.get("bl") is not None else 0.0)).view(n, H, C)
    xr = (x @ p["Wr"].t() + (p["br"] if p.get("br") is not None else 0.0)).view(n, H, C)
    z = xr[tgt] + xl[src]
    if p.get("We") is not None:
        z = z + (ea @ p["We"].t()).view(-1, H, C)
    e = (F.leaky_relu(z, slope) * p["att"].reshape(1, H, C)).sum(-1)                     # [E, H]
    alpha = torch.stack([pyg_softmax(e[:, h], tgt, n) for h in range(H)], 1)             # softmax per head
    out = torch.zeros(n, H, C, dtype=x.dtype).index_add(0, tgt, alpha.unsqueeze(-1) * xl[src])
    out = out.reshape(n, H * C) if concat else out.mean(1)
    if p.get("bias") is not None:
        out = out + p["bias"]
    return out


def head_params(p, h, heads, concat):
    """The single-head conv made of head h's row blocks (its bias: the block of a concatenated bias, none for a head mean)."""
    C = p["Wl"].size(0) // heads
    rows = slice(h * C, h * C + C)
    g = lambda k: None if p.get(k) is None else p[k][rows]  # noqa: E731
    return {"att": p["att"].reshape(heads, C)[h], "bias": g("bias") if concat else None, "Wl": g("Wl"), "bl": g("bl"), "Wr": g("Wr"),
            "br": g("br"), "We": g("We")}


def gat_dsse_heads(x, edge_index, edge_attr, sd, num_layers, heads, nonlin="leaky_relu", slope=0.2, add_self_loops=True):
    """GAT_DSSE(heads=H, concat=False) from a state_dict with the reference's keys (model.module_{i}.*)."""
    h = x
    act = NONLINS[nonlin]
    for k in range(num_layers - 1):
        h = act(gatv2_heads(h, edge_index, edge_attr, conv_params(sd, f"model.module_{2 * k}."), heads, False, slope, add_self_loops))
    i = 2 * (num_layers - 1)
    h = h @ sd[f"model.module_{i}.weight"].t() + sd[f"model.module_{i}.bias"]
    return h @ sd[f"model.module_{i + 1}.weight"].t() + sd[f"model.module_{i + 1}.bias"]


HEAD_SCALES = (1.5, 0.4, 2.5, 0.9)      # att magnitude per head: the heads' softmax maxima and sums differ


def random_conv_params(cin, c, heads, concat=True, ed=6, bias=True, seed=0):
    """Seeded explicit weights of one conv (att drawn per head with its own magnitude)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, a=1.0: (torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) * a  # noqa: E731
    w = heads * c
    att = torch.stack([r(c, a=HEAD_SCALES[h % len(HEAD_SCALES)]) for h in range(heads)]).view(1, heads, c)
    p = {"att": att, "bias": r(w if concat else c, a=0.2) if bias else None, "Wl": r(w, cin, a=0.6), "bl": r(w, a=0.3) if bias else None,
         "Wr": r(w, cin, a=0.6), "br": r(w, a=0.3) if bias else None, "We": r(w, ed, a=0.6) if ed else None}
    return p


def random_state_dict(num_layers, heads, c=8, dense=32, out=2, ed=6, seed=0, gain=1.0):
    """Seeded weights of GAT_DSSE(c, dense, out, num_layers, ed, heads=heads, concat=False) under the reference's keys.
    ``gain`` scales lin_l.weight and lin_r.weight of every conv."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, a=1.0: (torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) * a  # noqa: E731
    sd = {}
    for k in range(num_layers - 1):
        p, cp = f"model.module_{2 * k}.", random_conv_params(c, c, heads, concat=False, ed=ed, seed=1000 * seed + k)
        for key, name in (("att", "att"), ("bias", "bias"), ("lin_l.weight", "Wl"), ("lin_l.bias", "bl"), ("lin_r.weight", "Wr"),
                          ("lin_r.bias", "br"), ("lin_edge.weight", "We")):
            if cp[name] is not None:
                sd[p + key] = cp[name] * gain if name in ("Wl", "Wr") else cp[name]
    i = 2 * (num_layers - 1)
    sd[f"model.module_{i}.weight"] = r(dense, c, a=0.35)
    sd[f"model.module_{i}.bias"] = r(dense, a=0.2)
    sd[f"model.module_{i + 1}.weight"] = r(out, dense, a=0.18)
    sd[f"model.module_{i + 1}.bias"] = r(out, a=0.1)
    return sd
