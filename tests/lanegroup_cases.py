"""The case table of the lane-group models (GAT_DSSE, GINE_DSSE, gnn_dsse with GCN2 / FA / TAG), shared by
tests/test_lanegroup_cases_cpu.py (conditioning, kink margin and launch geometry of every case, no GPU) and
tests/test_gpu_lanegroup_shapes.py (the kernels against the fp64 restatement of every case).

A case is a family, the widths (C, dense, out), edge_dim, num_layers, the nonlinearity, the family's options, a structure and a
seed.  Inputs are x = randn(N, C) and edge_attr = randn(E, edge_dim) on the edges of a ``synthetic.make_batch`` structure, the
weights are seeded explicit state_dicts with the reference's keys, and the loss is the quadratic of the existing parity tests.
``restate`` is the model in plain torch on top of gat_oracle / gine_oracle / gnn_oracle, at any dtype; it also hands back the
inputs of the model's nonlinearity, so that a case can be held away from the kinks of ReLU / LeakyReLU.

Three groups of cases:
    width    the eight (C, dense, out) of WIDTHS on a small mixed batch: every lane group (8 / 16 / 32) with a partial and a full
             group, head widths below, at and above the group, dense = 1, and the families' options spread over them
    cap      N = 16 500 (1100 CIGRE graphs): the grid is capped at 256 workgroups, so each one makes several trips of the grid-
             stride loop (unequal numbers of them), sums its partials over several nodes per lane group, and the slab reduction
             and the chunked weight-gradient kernel see all 256 rows
    small    N = 1 (no edges), 3, 33 and 2049: one partial row, a nearly empty second slab, one node in a second trip
"""
import dataclasses
import functools
import importlib
import math

import torch

import gat_oracle
import gine_oracle
import gnn_oracle
from conftest import PKG_NAME

FAMILIES = ["gat", "gine", "gcn2", "fagcn", "tagcn"]
GNN_KINDS = ("gcn2", "fagcn", "tagcn")
NONLINS = ["leaky_relu", "relu", "tanh"]
OUT_FLOOR = 1e-5
MAX_SLABS, NT = 256, 256       # lanegroup._MAX_SLABS (checked in test_lanegroup_cases_cpu.py) and the kernels' workgroup size
KINK_MARGIN = 1e-5
# (C, dense, out): G = 8 with c < G; G = 16 with c < G; G = 16 full; the first width on G = 32; G = 32 with a narrow head; every
# limit at once; G = 32 with dense = 1; G = 8 with nout > G
WIDTHS = [(5, 9, 1), (12, 20, 3), (16, 16, 16), (17, 32, 2), (20, 7, 1), (32, 32, 32), (32, 1, 32), (8, 5, 20)]


def grad_floor(n):
    return max(1e-4, 8.0 / n)


def grad_bound(case, n):
    """The bound on a case's gradients: the suite's floor max(1e-4, 8 / N), whose 8 / N allows for a gate that falls the other
    way on one of N nodes.  At the small ends that term would let any gradient pass (8 at N = 1), so they are held to 1e-4."""
    return 1e-4 if case.group_name == "small" else grad_floor(n)


@dataclasses.dataclass(frozen=True)
class Case:
    group_name: str            # "width", "cap" or "small"
    family: str
    dims: tuple                # (C, dense, out)
    edge_dim: object           # None or a width (gat, gine)
    num_layers: int
    nonlin: str
    struct: str                # see structure()
    seed: int
    opts: tuple = ()           # the family's options, as sorted (key, value) pairs
    chain: tuple = ()          # gat only: the convs' widths where they change (C_0, ..., C_n); dims[0] is C_n

    @property
    def opt(self):
        return dict(self.opts)

    @property
    def id(self):
        o = ",".join(f"{k}={v}" for k, v in self.opts)
        c, d, out = self.dims
        w = "-".join(map(str, self.chain)) + f">{d}>{out}" if self.chain else f"{c}-{d}-{out}"
        return f"{self.group_name}:{self.family}:{w}:L{self.num_layers}:ed{self.edge_dim}:{self.nonlin}:{self.struct}" + (f":{o}" if o else "")

    @property
    def widths(self):
        return self.chain or (self.dims[0],)

    @property
    def group(self):
        m = max(self.widths + (self.dims[0],))
        return 8 if m <= 8 else (16 if m <= 16 else 32)

    @property
    def in_width(self):
        return self.widths[0]


def _case(group_name, family, dims, struct, num_layers=2, nonlin="tanh", edge_dim=None, seed=0, chain=(), **opts):
    return Case(group_name, family, tuple(dims), edge_dim, num_layers, nonlin, struct, seed, tuple(sorted(opts.items())), tuple(chain))


# ------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------
def _width_cases():
    gat_ed = [None, 3, 6, 16, None, 16, 6, 3]
    gine_ed = [None, 6, 16, None, 6, 16, 6, None]
    layers = {"gat": [3, 2, 5, 2, 3, 3, 2, 2], "gine": [3, 2, 5, 2, 3, 3, 1, 2], "gcn2": [3, 2, 2, 2, 3, 3, 1, 5],
              "fagcn": [3, 2, 5, 2, 1, 3, 2, 2], "tagcn": [3, 2, 3, 2, 3, 2, 2, 2]}
    tag_k = [2, 3, 1, 2, 3, 4, 0, 2]
    cases = []
    for fi, fam in enumerate(FAMILIES):
        for wi, dims in enumerate(WIDTHS):
            kw = dict(num_layers=layers[fam][wi], nonlin=NONLINS[(wi + fi) % 3])
            if fam == "fagcn" and dims[0] == 17:
                kw["nonlin"] = "tanh"       # without loops and eps a node without in-edges gets exactly 0: no kink margin to keep
            if fam == "gat":
                kw.update(edge_dim=gat_ed[wi], self_loops=wi != 4)
            elif fam == "gine":
                kw.update(edge_dim=gine_ed[wi], eps=0.3 if wi % 2 else 0.0, train_eps=bool(wi % 2))
            elif fam == "gcn2":
                kw.update(shared_weights=dims[0] != 32, add_self_loops=wi != 2, normalize=wi != 0, main_param=0.3 if wi % 2 else 0.1)
            elif fam == "fagcn":
                kw.update(main_param=0.0 if dims[0] == 17 else 0.1, add_self_loops=dims[0] != 17)
            else:
                kw.update(K=tag_k[wi], bias=dims[0] != 12, normalize=wi != 4)
            cases.append(_case("width", fam, dims, "mixed16", **kw))
    return cases


def _cap_cases():
    cases = []
    nl8 = {"gat": "leaky_relu", "gine": "relu", "gcn2": "leaky_relu", "fagcn": "tanh", "tagcn": "tanh"}
    ed = {"gat": 6, "gine": 6}
    for fam in FAMILIES:
        cases.append(_case("cap", fam, (8, 32, 2), "cap", num_layers=2 if fam == "gcn2" else 3, nonlin=nl8[fam], edge_dim=ed.get(fam),
                           **({"K": 2} if fam == "tagcn" else {})))
    for fam in ("gcn2", "tagcn", "gat", "gine"):
        kw = {"K": 2} if fam == "tagcn" else {}
        cases.append(_case("cap", fam, (12, 20, 3), "cap", num_layers=2, nonlin="leaky_relu" if fam == "gcn2" else "tanh",
                           edge_dim=3 if fam == "gat" else (16 if fam == "gine" else None), **kw))
        cases.append(_case("cap", fam, (32, 32, 32), "cap", num_layers=3 if fam in ("gcn2", "gine") else 2, nonlin="tanh",
                           edge_dim=16 if fam == "gat" else None, **kw))
    cases.append(_case("cap", "fagcn", (32, 32, 32), "cap", num_layers=3, nonlin="tanh"))
    # the hub (320 in-edges on node 5) on the capped batch, one family per lane group
    cases.append(_case("cap", "fagcn", (8, 32, 2), "cap_hub", num_layers=2, nonlin="tanh"))
    cases.append(_case("cap", "gine", (12, 20, 3), "cap_hub", num_layers=2, nonlin="tanh", edge_dim=6))
    cases.append(_case("cap", "gat", (32, 32, 32), "cap_hub", num_layers=2, nonlin="tanh", edge_dim=6))
    return cases


def _small_cases():
    cases = []
    for fam in FAMILIES:
        kw = {"K": 2} if fam == "tagcn" else {}
        ed = 6 if fam in ("gat", "gine") else None
        cases.append(_case("small", fam, (8, 32, 2), "n1", nonlin="tanh", edge_dim=ed, **kw))
        cases.append(_case("small", fam, (12, 20, 3), "n3", nonlin="tanh", edge_dim=ed, **kw))
        cases.append(_case("small", fam, (8, 32, 2), "n33", num_layers=3, nonlin="leaky_relu", edge_dim=ed, **kw))
        cases.append(_case("small", fam, (32, 32, 32), "n2049", num_layers=2, nonlin="relu" if fam == "gcn2" else "tanh", edge_dim=ed, **kw))
    return cases


def _chain_cases():
    # GATv2Conv(5, 12), (12, 20), (20, 7), then the head 7 -> 9 -> 4: per-conv widths, which only gat._Spec supports
    return [_case("width", "gat", (7, 9, 4), "mixed16", num_layers=4, nonlin="leaky_relu", edge_dim=3, chain=(5, 12, 20, 7), self_loops=True)]


# seeds that meet the conditions of tests/test_lanegroup_cases_cpu.py (no pre-activation within KINK_MARGIN of a kink, 4 x the
# fp32 error under every bound), by (group, family, (C, dense, out), structure); a case not listed keeps seed 0
SEEDS = {
    ("width", "gine", (16, 16, 16), "mixed16"): 1,
    ("width", "gine", (32, 32, 32), "mixed16"): 1,
    ("width", "fagcn", (32, 1, 32), "mixed16"): 2,
    ("cap", "gat", (8, 32, 2), "cap"): 7,
    ("cap", "gine", (8, 32, 2), "cap"): 7,
    ("cap", "gcn2", (8, 32, 2), "cap"): 6,
    ("small", "gcn2", (32, 32, 32), "n2049"): 1,
}


def _key(c):
    return (c.group_name, c.family, c.dims, c.struct)


def _with_seeds(cases):
    assert len({_key(c) for c in cases}) == len(cases) and set(SEEDS) <= {_key(c) for c in cases}
    return [dataclasses.replace(c, seed=SEEDS.get(_key(c), c.seed)) for c in cases]


CASES = _with_seeds(_width_cases() + _chain_cases() + _cap_cases() + _small_cases())
WIDTH_CASES = [c for c in CASES if c.group_name == "width"]
CAP_CASES = [c for c in CASES if c.group_name == "cap"]
SMALL_CASES = [c for c in CASES if c.group_name == "small"]
assert len({c.id for c in CASES}) == len(CASES)


def pkg():
    return importlib.import_module(PKG_NAME)


# ------------------------------------------------------------------------------------------
# structures and inputs
# ------------------------------------------------------------------------------------------
def _truncated(ei, n):
    return ei[:, (ei < n).all(0)].contiguous()


@functools.lru_cache(maxsize=None)
def structure(name):
    """(edge_index [2, E] int64, N)."""
    mk = pkg().synthetic.make_batch
    if name == "mixed16":
        b = mk(["cigre14", "ober_sub"], 16, seed=3)
        return b["edge_index"], b["x"].size(0)
    if name in ("cap", "cap_hub"):
        b = mk(["cigre14"], 1100, seed=1)
        ei, n = b["edge_index"], b["x"].size(0)
        assert n == 16500
        if name == "cap_hub":
            src = torch.arange(100, 420)
            ei = torch.cat([ei, torch.stack([src, torch.full_like(src, 5)])], 1)
        return ei, n
    if name == "n1":
        return torch.zeros(2, 0, dtype=torch.int64), 1
    if name == "n3":
        return torch.tensor([[0, 1, 2], [1, 2, 1]]), 3
    if name == "n33":
        return _truncated(mk(["cigre14"], 3, seed=2)["edge_index"], 33), 33
    if name == "n2049":
        return _truncated(mk(["cigre14"], 137, seed=2)["edge_index"], 2049), 2049
    raise KeyError(name)


def inputs(case):
    """(x [N, C_in], edge_index, edge_attr or None) in float64."""
    ei, n = structure(case.struct)
    g = torch.Generator().manual_seed(1000 + case.seed)
    x = torch.randn(n, case.in_width, generator=g, dtype=torch.float64)
    ea = None
    if case.family == "gine":
        ea = torch.randn(ei.size(1), case.edge_dim or case.in_width, generator=g, dtype=torch.float64)
    elif case.family == "gat" and case.edge_dim:
        ea = torch.randn(ei.size(1), case.edge_dim, generator=g, dtype=torch.float64)
    return x, ei, ea


# ------------------------------------------------------------------------------------------
# weights (the reference's state_dict keys)
# ------------------------------------------------------------------------------------------
def _uniform(g):
    return lambda *s, a=1.0: (torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) * a


def _head_into(sd, r, i, c, dense, out):
    sd[f"model.module_{i}.weight"] = r(dense, c, a=1.2 / math.sqrt(c))
    sd[f"model.module_{i}.bias"] = r(dense, a=0.2)
    sd[f"model.module_{i + 1}.weight"] = r(out, dense, a=1.0 / math.sqrt(dense))
    sd[f"model.module_{i + 1}.bias"] = r(out, a=0.1)


def _gat_chain_state_dict(case):
    r = _uniform(torch.Generator().manual_seed(case.seed))
    sd, ed = {}, case.edge_dim
    for k, (ci, co) in enumerate(zip(case.chain[:-1], case.chain[1:])):
        p = f"model.module_{2 * k}."
        sd[p + "att"] = r(1, 1, co, a=1.5)
        sd[p + "bias"] = r(co, a=0.2)
        sd[p + "lin_l.weight"] = r(co, ci, a=1.5 / math.sqrt(ci))
        sd[p + "lin_l.bias"] = r(co, a=0.3)
        sd[p + "lin_r.weight"] = r(co, ci, a=1.5 / math.sqrt(ci))
        sd[p + "lin_r.bias"] = r(co, a=0.3)
        if ed:
            sd[p + "lin_edge.weight"] = r(co, ed, a=0.6)
    _head_into(sd, r, 2 * (len(case.chain) - 1), case.dims[0], case.dims[1], case.dims[2])
    return sd


def _gnn_state_dict(case):
    r = _uniform(torch.Generator().manual_seed(case.seed))
    (c, dense, out), o, sd = case.dims, case.opt, {}
    for l in range(case.num_layers - 1):
        p = f"model.module_{2 * l}."
        if case.family == "gcn2":
            sd[p + "weight1"] = r(c, c, a=1.5 / math.sqrt(c))
            if not o.get("shared_weights", True):
                sd[p + "weight2"] = r(c, c, a=1.5 / math.sqrt(c))
        elif case.family == "fagcn":
            sd[p + "att_l.weight"] = r(1, c, a=1.0 / math.sqrt(c))
            sd[p + "att_r.weight"] = r(1, c, a=1.0 / math.sqrt(c))
        else:
            K = o["K"]
            if o.get("bias", True):
                sd[p + "bias"] = r(c, a=0.3)
            for m in range(K + 1):
                sd[p + f"lins.{m}.weight"] = r(c, c, a=1.5 / math.sqrt(c * (K + 1)))
    _head_into(sd, r, 2 * (case.num_layers - 1), c, dense, out)
    return sd


def state_dict(case):
    """float64 weights with the model's state_dict keys (GINE: the shared nn under every owner, the same tensor)."""
    c, dense, out = case.dims
    if case.chain:
        return _gat_chain_state_dict(case)
    if case.family == "gat":
        return _fan_in_scaled(gat_oracle.random_state_dict(case.num_layers, c, dense, out, case.edge_dim or 0, seed=case.seed))
    if case.family == "gine":
        return _fan_in_scaled(gine_oracle.random_state_dict(case.num_layers, c, dense, out, case.edge_dim or 0,
                                                            eps=case.opt.get("eps", 0.0), seed=case.seed))
    return _gnn_state_dict(case)


def _fan_in_scaled(sd):
    """The oracles' random weights are sized for 8 inputs: a matrix of more columns is scaled by sqrt(8 / columns), so that the
    activations keep their size at every width (a tensor that appears under several keys stays one tensor)."""
    done = {}
    for k, v in sd.items():
        if id(v) not in done:
            done[id(v)] = v * math.sqrt(8.0 / v.size(1)) if v.dim() == 2 and v.size(1) > 8 else v
    return {k: done[id(v)] for k, v in sd.items()}


def leaves(case, sd, dtype):
    """One differentiable tensor per parameter, under named_parameters()'s names."""
    if case.family == "gine":
        sd = gine_oracle.unique_params(sd)
        if not case.opt.get("train_eps", False):
            fixed = {k: v.to(dtype) for k, v in sd.items() if k.endswith(".eps")}
            return {**{k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items() if k not in fixed}, **fixed}
    return {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}


# ------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------
def restate(case, ref, x, ei, ea, pre=None):
    """The model on the oracles' convs; ``ref``: the parameters by name.  Appends every input of the model's nonlinearity to pre."""
    act = gat_oracle.NONLINS[case.nonlin]
    o, n, h = case.opt, x.size(0), x
    n_convs = len(case.chain) - 1 if case.chain else case.num_layers - 1
    for k in range(n_convs):
        p = f"model.module_{2 * k}."
        if case.family == "gat":
            z = gat_oracle.gatv2(h, ei, ea, gat_oracle.conv_params(ref, p), 0.2, o.get("self_loops", True))
        elif case.family == "gine":
            z = gine_oracle.gine(h, ei, ea, ref["nn.weight"], ref["nn.bias"], ref[p + "eps"], ref.get(p + "lin.weight"), ref.get(p + "lin.bias"))
        elif case.family == "gcn2":
            st = gnn_oracle.Structure(ei, n, o.get("normalize", True), o.get("add_self_loops", True))
            z = gnn_oracle.gcn2(h, x, st, o.get("main_param", 0.1), ref[p + "weight1"], ref.get(p + "weight2"))
        elif case.family == "fagcn":
            st = gnn_oracle.Structure(ei, n, True, o.get("add_self_loops", True))
            z = gnn_oracle.fa(h, x, st, o.get("main_param", 0.1), ref[p + "att_l.weight"], ref[p + "att_r.weight"])
        else:
            st = gnn_oracle.Structure(ei, n, o.get("normalize", True), False)
            z = gnn_oracle.tag(h, st, [ref[p + f"lins.{m}.weight"] for m in range(o["K"] + 1)], ref.get(p + "bias"))
        if pre is not None:
            pre.append(z.detach())
        h = act(z)
    i = 2 * n_convs
    h = h @ ref[f"model.module_{i}.weight"].t() + ref[f"model.module_{i}.bias"]
    return h @ ref[f"model.module_{i + 1}.weight"].t() + ref[f"model.module_{i + 1}.bias"]


def existing_oracle(case, sd, x, ei, ea):
    """The same model through the oracle modules' own wiring (gat_dsse / gine_dsse / GnnDSSE): restate() must equal it."""
    if case.chain:
        return None
    if case.family == "gat":
        return gat_oracle.gat_dsse(x, ei, ea, sd, case.num_layers, case.nonlin, 0.2, case.opt.get("self_loops", True))
    if case.family == "gine":
        return gine_oracle.gine_dsse(x, ei, ea, sd, case.num_layers, case.nonlin)
    o = case.opt
    return gnn_oracle.GnnDSSE(sd, case.num_layers, case.family, o.get("main_param", 0.1), o.get("K", 3), case.nonlin, False,
                              o.get("add_self_loops", True), o.get("normalize", True))(x, ei)


def quad(out):
    w = torch.linspace(-1.0, 1.0, out.numel(), dtype=out.dtype, device=out.device).view_as(out)
    return (out * w).sum() + 0.5 * (out ** 2).sum()


def oracle_run(case, dtype, with_pre=False):
    """The restatement at dtype on the CPU: dict(out, grads {name: tensor or None}, dx, pre)."""
    x, ei, ea = inputs(case)
    ref = leaves(case, state_dict(case), dtype)
    xr = x.to(dtype).requires_grad_(True)
    pre = [] if with_pre else None
    out = restate(case, ref, xr, ei, None if ea is None else ea.to(dtype), pre)
    quad(out).backward()
    return dict(out=out.detach(), grads={k: v.grad for k, v in ref.items() if v.requires_grad}, dx=xr.grad, pre=pre)


# ------------------------------------------------------------------------------------------
# the package's model of a case
# ------------------------------------------------------------------------------------------
class _Holder(torch.nn.Module):
    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, x, edge_index, edge_attr):
        return self.model(x, edge_index, edge_attr)


def build_model(case):
    """The package's model with the case's weights (float32, on the CPU)."""
    P = pkg()
    (c, dense, out), o = case.dims, case.opt
    if case.chain:
        convs = [P.GATv2Conv(ci, co, edge_dim=case.edge_dim, add_self_loops=o.get("self_loops", True))
                 for ci, co in zip(case.chain[:-1], case.chain[1:])]
        act = P.lanegroup.nonlin_module(case.nonlin)
        head = [torch.nn.Linear(c, dense), torch.nn.Linear(dense, out)]
        m = _Holder(P.lanegroup.Sequential([l for cv in convs for l in (cv, act)] + head, convs, head, case.nonlin, P.gat.run_gat))
    elif case.family == "gat":
        m = P.GAT_DSSE(c, dense, out, case.num_layers, case.edge_dim, nonlin=case.nonlin, self_loops=o.get("self_loops", True))
    elif case.family == "gine":
        m = P.GINE_DSSE(c, dense, out, case.num_layers, case.edge_dim, nonlin=case.nonlin, eps=o.get("eps", 0.0), train_eps=o.get("train_eps", False))
    else:
        kw = {k: o[k] for k in ("main_param", "K", "bias", "shared_weights", "add_self_loops", "normalize") if k in o}
        m = P.gnn_dsse(c, dense, out, case.num_layers, nonlin=case.nonlin, model=case.family, cached=False, **kw)
    m.load_state_dict({k: v.float() for k, v in state_dict(case).items()}, strict=True)
    return m


def call_model(case, m, x, ei, ea):
    return m(x, ei) if case.family in GNN_KINDS else m(x, ei, ea)


def spec_of(case, m):
    """The family's launch spec (lane group, slab count) for the case's node count."""
    P = pkg()
    seq = m.model
    mod = {"gat": P.gat, "gine": P.gine}.get(case.family, P.gnn)
    return mod._Spec(seq._convs, seq._head, case.nonlin, structure(case.struct)[1])


def trips(n, group, n_slabs):
    """The trips of the grid-stride loop that workgroup b's first lane group makes, for every b."""
    per, stride = NT // group, n_slabs * (NT // group)
    return [len(range(b * per, n, stride)) for b in range(n_slabs)]
