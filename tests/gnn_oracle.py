"""fp64 restatement of the reference's gnn_dsse (/root/reference/networks.py:11-69) and PyG's gcn_norm, GCN2Conv, FAConv and
TAGConv, in plain torch (differentiable).  Parameters come as a state_dict with the reference's keys."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDENS = ["gnn_gcn2_real64", "gnn_fagcn_real64", "gnn_tagcn_real64", "gnn_gcn2_reswitched", "gnn_gcn2_ober", "gnn_gcn2_mixed",
           "gnn_gcn2_unshared", "gnn_gcn2_noloops", "gnn_tagcn_k3_nobias", "gnn_fagcn_eps0", "gnn_gcn2_tanh_l2"]


def load_golden(name):
    """case_<name>.npz (tests/golden/make_gnn_goldens.py: the reference's gnn_dsse + gsp_wls_edge + backward, in float64):
    (arrays with the batch, params, grads, the reference's state_dict keys in order, gnn_dsse's constructor kwargs)."""
    z = np.load(os.path.join(GOLDEN, f"case_{name}.npz"), allow_pickle=False)
    t = {k: torch.from_numpy(z[k]) for k in z.files if z[k].dtype.kind in "fi" and (z[k].ndim > 0 or k == "loss")}
    src = str(z["batch"])
    if src:
        g = np.load(os.path.join(GOLDEN, src))
        t.update({k: torch.from_numpy(g[k]) for k in ("x", "edge_index", "edge_attr", "x_mean", "x_std", "edge_mean", "edge_std")})
    params = {k[len("param/"):]: v for k, v in t.items() if k.startswith("param/")}
    grads = {k[len("grad/"):]: v for k, v in t.items() if k.startswith("grad/")}
    kw = dict(model=str(z["model"]), num_layers=int(z["num_layers"]), K=int(z["K"]), main_param=float(z["main_param"]),
              nonlin=str(z["nonlin"]), shared_weights=bool(z["shared_weights"]), add_self_loops=bool(z["add_self_loops"]),
              bias=bool(z["bias"]))
    return t, params, grads, [str(k) for k in z["keys"]], kw


def gcn_norm(edge_index, n, add_self_loops=True):
    """PyG gcn_norm(edge_index, None, n, improved=False, add_self_loops): with self loops, add_remaining_self_loops drops every
    loop entry and appends one loop of weight 1 per node; deg over the target; w = deg^-1/2[src] * deg^-1/2[dst]."""
    src, dst = edge_index[0], edge_index[1]
    if add_self_loops:
        keep = src != dst
        loop = torch.arange(n, dtype=edge_index.dtype)
        src, dst = torch.cat([src[keep], loop]), torch.cat([dst[keep], loop])
    w = torch.ones(src.numel(), dtype=torch.float64)
    deg = torch.zeros(n, dtype=torch.float64).index_add_(0, dst, w)
    dis = deg.pow(-0.5)
    dis[torch.isinf(dis)] = 0.0
    return src, dst, dis[src] * w * dis[dst]


def propagate(h, src, dst, w):
    out = torch.zeros_like(h)
    return out.index_add(0, dst, h[src] * w.to(h.dtype)[:, None])


class Structure:
    """The normalised structure one conv uses (what PyG caches with cached=True)."""

    def __init__(self, edge_index, n, normalize=True, add_self_loops=True):
        if normalize:
            self.src, self.dst, self.w = gcn_norm(edge_index, n, add_self_loops)
        else:
            self.src, self.dst = edge_index[0], edge_index[1]
            self.w = torch.ones(edge_index.size(1), dtype=torch.float64)

    def P(self, h):
        return propagate(h, self.src, self.dst, self.w)


def gcn2(h, x0, st, alpha, W1, W2=None):
    a = (1 - alpha) * st.P(h)
    if W2 is None:
        return (a + alpha * x0) @ W1
    return a @ W1 + (alpha * x0) @ W2


def fa(h, x0, st, eps, att_l, att_r):
    al, ar = h @ att_l.reshape(-1), h @ att_r.reshape(-1)
    t = torch.tanh(al[st.src] + ar[st.dst])
    out = propagate(h, st.src, st.dst, t * st.w.to(h.dtype))
    if eps != 0.0:
        out = out + eps * x0
    return out


def tag(h, st, lins, bias=None):
    out = h @ lins[0].T
    for W in lins[1:]:
        h = st.P(h)
        out = out + h @ W.T
    return out if bias is None else out + bias


_NONLIN = {"leaky_relu": F.leaky_relu, "relu": F.relu, "tanh": torch.tanh}


class GnnDSSE:
    """gnn_dsse with PyG's cache: cached convs keep the structure of the first call (extra nodes: no edges, no loop)."""

    def __init__(self, sd, num_layers, model="gcn2", main_param=0.1, K=3, nonlin="leaky_relu", cached=True, add_self_loops=True,
                 normalize=True, shared_weights=True):
        self.sd, self.L, self.model, self.p, self.K = sd, num_layers, model, main_param, K
        self.act, self.cached, self.loops, self.normalize = _NONLIN[nonlin], cached, add_self_loops, normalize
        self.shared = shared_weights
        self.cache = [None] * (num_layers - 1)

    def structure(self, l, edge_index, n):
        if self.model == "tagcn":
            return Structure(edge_index, n, self.normalize, False)
        if not (self.cached and self.normalize):
            return Structure(edge_index, n, self.normalize, self.loops)
        if self.cache[l] is None:
            self.cache[l] = Structure(edge_index, n, True, self.loops)
        st = self.cache[l]
        if max(int(st.src.max()) if st.src.numel() else -1, int(st.dst.max()) if st.dst.numel() else -1) >= n:
            raise IndexError("cached structure references nodes beyond the batch")
        return st

    def __call__(self, x, edge_index):
        sd, h, x0, n = self.sd, x, x, x.size(0)
        for l in range(self.L - 1):
            k = f"model.module_{2 * l}."
            st = self.structure(l, edge_index, n)
            if self.model == "gcn2":
                h = gcn2(h, x0, st, self.p, sd[k + "weight1"], sd.get(k + "weight2"))
            elif self.model == "fagcn":
                h = fa(h, x0, st, self.p, sd[k + "att_l.weight"], sd[k + "att_r.weight"])
            else:
                h = tag(h, st, [sd[k + f"lins.{m}.weight"] for m in range(self.K + 1)], sd.get(k + "bias"))
            h = self.act(h)
        k1, k2 = f"model.module_{2 * (self.L - 1)}.", f"model.module_{2 * (self.L - 1) + 1}."
        h = h @ sd[k1 + "weight"].T + sd[k1 + "bias"]
        return h @ sd[k2 + "weight"].T + sd[k2 + "bias"]
