"""The case table of the MPN path (MPN, SkipMPN, PFN, SkipPFN) on graphs that ``synthetic.make_batch`` never produces, shared by
tests/test_mpn_shape_cases_cpu.py (structure, route, conditioning and placement of every case, no GPU) and
tests/test_gpu_mpn_shapes.py (the kernels against the fp64 oracle model of every case).

The four grids give ELL widths 3 and 4, tiles of 64 / 96 / 192 rows that are never full, and no node without a branch.  The kernels
dispatch on the ELL width (1 .. 8, CSR staging beyond), the tile height (32 .. 192 rows) and the rows a tile really holds, so the
cases here move exactly those.

A case is a list of node counts, a degree cap, a model with its constructor arguments and a seed.  ``batch`` builds one connected
graph per count, stored one direction per branch like the reference's data (the model doubles them): a random tree under the cap,
a few loop-closing chords under the same cap, and ONE node per graph driven to exactly the cap (a graph too small for that: to
all its other nodes).  In the graphs listed in ``tail`` that node is the graph's LAST row and has the graph's row 0 among its
neighbours: where the graph fills a tile these are the tile's last and first rows, so a kernel that drops the last ELL slot, the last
tile row or row 0 of the tile cannot pass.  In every other graph the capped node sits mid-graph.  Features are x = randn(N, 8) and
edge_attr = randn(E, 6), drawn in fp64 and rounded to fp32 (so the fp64 referee and the kernels read the same numbers); the
weights are the oracle model's own initialisation under the case's seed.

STRUCTURE and ROUTE pin what every case is there for as literals.  They were read off the library BEFORE these tests existed (the
topology oracle for the structure; route.block_route, the whole-stack query, the weight-gradient plan and the edge plan on a stand-in
topology for the route), not produced by a run of changed code: a case that drifts fails loudly.

tests/mpn_width_cases.py builds cases of its own on the graphs of these (other hidden widths, heads, K and depths): ``batch``, ``reference``,
``topology_oracle``, ``stub_topology`` and ``structure`` take a case object as well as a name of this table, and cases with the same graph
fields share graphs, features and topology oracle."""
import dataclasses
import functools
import importlib
import types

import torch

import dss2_oracle
from conftest import PKG_NAME
from dss2_topology_oracle import TopologyOracle

OUT_BOUND, GRAD_BOUND = 1e-5, 1e-4      # the MPN path's flat bounds (test_gpu_large_graphs.py); no 8 / N term: it would pass anything here
CUS = 256                               # compute units of an MI355X (stack.tiles_of takes 32-row tiles while 64-row ones leave CUs idle)
C2 = (8, 6, 2, 128, 4, 2, 0.0)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    counts: tuple          # nodes per graph
    cap: int               # degree cap on the stored (undoubled) branches, before ``dup3``
    cls: str
    args: tuple            # constructor arguments, as in conftest.CASES
    purpose: str
    tail: tuple = ()       # graphs whose capped node is their last row, with their row 0 among its neighbours
    full: bool = False     # some graph of ``tail`` fills a tile on its own: its capped node is the tile's last row
    dup3: bool = False     # every third branch listed twice (two ELL entries for one neighbour)
    seed: int = 0


CASES = [
    Case("full64_ell5", (64,) * 3, 5, "MPN", C2, "the full fused C2 route on tiles with no padding row", tail=(0, 2), full=True),
    Case("c2_ell8_head_edge", (15,) * 90, 8, "MPN", C2, "forward without, backward with the fused edge phase", tail=tuple(range(3, 90, 4))),
    Case("n65_ell6", (65,) * 3, 6, "MPN", C2, "one row over a 64-row tile: 96-row tiles holding 65", tail=(1,)),
    Case("ragged_ell7", (32, 32, 31, 2, 64, 1, 17, 63), 7, "MPN", (8, 6, 2, 64, 3, 2, 0.0),
         "greedy packing, a one-node graph, max_tile_rows = 0", tail=(2, 4)),
    Case("full96_ell8", (96, 96, 95), 8, "MPN", C2, "tall chain, full and one-short tiles, widest ELL", tail=(0, 2), full=True),
    Case("full128_ell6", (128,) * 2, 6, "MPN", (8, 6, 2, 128, 3, 3, 0.0), "nrb 4 primary, K = 3, matrix-sequential layers", tail=(1,), full=True),
    Case("full192_ell8", (192, 191), 8, "MPN", C2, "192-row chain at the limit of the LDS tile", tail=(0,), full=True),
    Case("nrb1_ell8", (15,) * 9, 8, "MPN", C2, "32-row primary tiling, wgrad16h", tail=(1, 8)),
    Case("pairs_ell1", (2,) * 40, 1, "MPN", (8, 6, 2, 32, 3, 2, 0.0), "ELL width 1, narrow hidden layer"),
    Case("csr9", (20,) * 7, 9, "SkipMPN", (8, 6, 8, 32, 3, 2, 0.0),
         "one over the ELL limit: CSR staging inside tile kernels, on a non-star graph", tail=(2, 6)),
    Case("parallel_ell8", (64,) * 3, 4, "MPN", C2, "two ELL entries for one neighbour, with total width kept <= 8", tail=(1,), full=True, dup3=True),
    Case("stack_full64_ell4", (64, 64, 32, 31, 1), 4, "SkipPFN", (8, 6, 2, 32, 3, 2, 0.0, 2),
         "whole-stack kernels on full tiles and an isolated node", tail=(0, 3), full=True),
    Case("stack_ell5", (15,) * 9, 5, "SkipPFN", (8, 6, 2, 32, 3, 2, 0.0, 2),
         "one over S_MAX_ELL: the stack route must decline and the per-block route must be right", tail=(1, 8)),
    Case("pfn_ell8_96", (96, 95), 8, "PFN", (8, 6, 2, 32, 2, 2, 0.0, 2),
         "per-block route inside a stack node (in_stack=True) on tall tiles", tail=(0,), full=True),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# name -> (nrb, ntiles, ell, ellT, max_segment, min degree on the doubled list), from oracle/dss2_topology_oracle.py
STRUCTURE = {
    "full64_ell5": (2, 3, 5, 5, 64, 1),
    "c2_ell8_head_edge": (2, 23, 8, 8, 15, 1),
    "n65_ell6": (3, 3, 6, 6, 65, 1),
    "ragged_ell7": (3, 3, 7, 7, 64, 0),             # [32 32 31 | 2 64 1 17 | 63]: 96-row tiles beat 64-row ones (0.84 against 0.76)
    "full96_ell8": (3, 3, 8, 8, 96, 1),
    "full128_ell6": (4, 2, 6, 6, 128, 1),
    "full192_ell8": (6, 2, 8, 8, 192, 1),
    "nrb1_ell8": (1, 5, 8, 8, 15, 1),
    "pairs_ell1": (3, 1, 1, 1, 2, 1),
    "csr9": (2, 3, 0, 0, 20, 1),
    "parallel_ell8": (2, 3, 7, 7, 64, 1),           # a node with three of its four branches listed twice
    "stack_full64_ell4": (2, 3, 4, 4, 64, 0),
    "stack_ell5": (1, 5, 5, 5, 15, 1),
    "pfn_ell8_96": (3, 2, 8, 8, 96, 1),
}

# the fields of route.BlockRoute that name a case's purpose
ROUTE_FIELDS = ("f16", "n_chain", "use16", "gw", "head", "edge", "bwd_chain", "bwd_head", "bwd_head_wgrad", "bwd_edge", "glob")

# block routes that several cases share, in the order of ROUTE_FIELDS
_C2_FUSED = (True, 3, True, 128, True, True, True, True, True, True, False)          # f16x3 chains, head, edge and bwd_edge
_C2_DX = (True, 3, True, 128, True, False, True, True, True, False, False)           # ... with an input gradient: the edge launches of their own
_C2_BWD_EDGE_ONLY = (True, 3, True, 128, True, False, True, True, True, True, False)  # the forward refuses the edge phase, the backward takes it
_TALL_256 = (True, 3, True, 256, False, False, True, True, True, False, False)       # 96-row chains: head only in the data-gradient chain
_TALL_384 = (True, 3, True, 384, False, False, True, True, True, False, False)       # 192-row chains
_BF16X6_3 = (False, 3, True, 0, False, False, True, False, False, False, False)      # 32-row tiles: bf16x6 chains, no f16, no gate words
_BF16X6_2 = (False, 2, True, 0, False, False, True, False, False, False, False)      # hid 32 / 64 below the f16 forms
_LAYERS = (False, 0, False, 0, False, False, False, False, False, False, False)      # no chain at all: layer by layer
WG_FP32, WG_BF16_64, WG_F16_32, WG_F16_TALL, WG_F16_TALL_PAIR = 3, 4, 7, 8, 9        # dss2_wgrad_kernel
E_CSR, E_VALU, E_VALU_HALF, E_BF16X6 = 1, 2, 3, 5                                    # dss2_edge_family (0: no such pass)

# name -> need_dx (does x require a gradient) -> (whole-stack kernels take the model, ROUTE_FIELDS of every block, (tile rows,
# dss2_wgrad_kernel) of the hid -> hid weight gradients, (forward, backward by target, backward by source) dss2_edge_family of the first
# block's edge MLP).  The block routes and the two plans are pinned for the whole-stack cases too: what the blocks run with the stack
# kernels switched off.
ROUTE = {
    "full64_ell5": {False: (False, (_C2_FUSED,), (64, WG_BF16_64), (E_BF16X6, E_BF16X6, 0)),
                    True: (False, (_C2_DX,), (64, WG_BF16_64), (E_BF16X6, E_BF16X6, E_VALU))},
    "c2_ell8_head_edge": {False: (False, (_C2_BWD_EDGE_ONLY,), (32, WG_F16_32), (E_BF16X6, E_BF16X6, 0)),
                          True: (False, (_C2_DX,), (32, WG_F16_32), (E_BF16X6, E_BF16X6, E_VALU))},
    "n65_ell6": {False: (False, (_TALL_256,), (96, WG_F16_TALL), (E_BF16X6, E_BF16X6, 0)),
                 True: (False, (_TALL_256,), (96, WG_F16_TALL), (E_VALU, E_VALU, E_VALU))},
    "ragged_ell7": {False: (False, ((True, 2, True, 128, False, False, True, True, True, False, False),), (96, WG_F16_TALL), (E_BF16X6, E_BF16X6, 0)),
                    True: (False, ((True, 2, True, 128, False, False, True, True, True, False, False),), (96, WG_F16_TALL), (E_VALU, E_VALU, E_VALU))},
    "full96_ell8": {False: (False, (_TALL_256,), (96, WG_F16_TALL), (E_BF16X6, E_BF16X6, 0)),
                    True: (False, (_TALL_256,), (96, WG_F16_TALL), (E_VALU, E_VALU, E_VALU))},
    "full128_ell6": {False: (False, (_LAYERS,), (128, WG_FP32), (E_BF16X6, E_BF16X6, 0)),
                     True: (False, (_LAYERS,), (128, WG_FP32), (E_VALU, E_VALU, E_VALU))},
    "full192_ell8": {False: (False, (_TALL_384,), (192, WG_F16_TALL), (E_BF16X6, E_BF16X6, 0)),
                     True: (False, (_TALL_384,), (192, WG_F16_TALL), (E_VALU, E_VALU, E_VALU))},
    "nrb1_ell8": {False: (False, (_BF16X6_3,), (32, WG_F16_32), (E_BF16X6, E_BF16X6, 0)),
                  True: (False, (_BF16X6_3,), (32, WG_F16_32), (E_BF16X6, E_BF16X6, E_VALU))},
    "pairs_ell1": {False: (True, (_BF16X6_2,), (96, WG_F16_TALL_PAIR), (E_BF16X6, E_BF16X6, 0)),
                   True: (True, (_BF16X6_2,), (96, WG_F16_TALL_PAIR), (E_VALU_HALF, E_VALU_HALF, E_VALU_HALF))},
    "csr9": {False: (False, (_LAYERS,), (64, WG_FP32), (E_CSR, E_CSR, 0)),
             True: (False, (_LAYERS,), (64, WG_FP32), (E_CSR, E_CSR, E_CSR))},
    "parallel_ell8": {False: (False, (_C2_FUSED,), (64, WG_BF16_64), (E_BF16X6, E_BF16X6, 0)),
                      True: (False, (_C2_DX,), (64, WG_BF16_64), (E_BF16X6, E_BF16X6, E_VALU))},
    "stack_full64_ell4": {False: (True, (_BF16X6_2,) * 2, (64, WG_FP32), (E_BF16X6, E_BF16X6, 0)),
                          True: (True, (_BF16X6_2,) * 2, (64, WG_FP32), (E_BF16X6, E_BF16X6, E_VALU_HALF))},
    "stack_ell5": {False: (False, (_BF16X6_2,) * 2, (32, WG_FP32), (E_BF16X6, E_BF16X6, 0)),
                   True: (False, (_BF16X6_2,) * 2, (32, WG_FP32), (E_BF16X6, E_BF16X6, E_VALU_HALF))},
    "pfn_ell8_96": {False: (False, (_LAYERS,) * 2, (96, WG_F16_TALL), (E_BF16X6, E_BF16X6, 0)),
                    True: (False, (_LAYERS,) * 2, (96, WG_F16_TALL), (E_VALU_HALF, E_VALU_HALF, E_VALU_HALF))},
}


def pkg():
    return importlib.import_module(PKG_NAME)


# ------------------------------------------------------------------------------------------
# the generator
# ------------------------------------------------------------------------------------------
def _graph(n, cap, hub, tail, g):
    """One connected graph of n nodes: (branches as [(a, b)], the capped node).  ``hub`` is driven to min(cap, n - 1) branches."""
    if n == 1:
        return [], 0
    deg, adj, edges = [0] * n, [set() for _ in range(n)], []

    def add(a, b):
        if torch.rand((), generator=g).item() < 0.5:      # either orientation: the doubled list flips the sign of the stored reverse
            a, b = b, a
        edges.append((a, b))
        adj[a].add(b)
        adj[b].add(a)
        deg[a] += 1
        deg[b] += 1

    rest = [i for i in torch.randperm(n, generator=g).tolist() if i != 0 and not (tail and i == hub)]
    placed = [0]
    if tail:
        add(0, hub)
        placed.append(hub)
    for i in rest:                                          # a random tree under the cap
        ok = [p for p in placed if deg[p] < cap]
        add(ok[int(torch.randint(len(ok), (), generator=g))], i)
        placed.append(i)
    for _ in range(n // 8):                                 # loop-closing chords under the same cap, none at the capped node
        a, b = torch.randint(n, (2,), generator=g).tolist()
        if a != b and hub not in (a, b) and b not in adj[a] and deg[a] < cap and deg[b] < cap:
            add(a, b)
    want = min(cap, n - 1)
    for v in torch.randperm(n, generator=g).tolist():      # the capped node, to exactly the cap
        if deg[hub] == want:
            break
        if v != hub and v not in adj[hub] and deg[v] < cap:
            add(hub, v)
    assert deg[hub] == want and max(deg) <= cap, (n, cap, deg[hub])
    return edges, hub


def case_of(key):
    """A case given as itself or by its name in BY_NAME (tests/mpn_width_cases.py builds cases of its own on the graphs of these)."""
    return key if isinstance(key, Case) else BY_NAME[key]


def graph_key(key):
    """What of a case decides its graphs: two cases with the same key share edge list, x and edge_attr (and the topology oracle)."""
    case = case_of(key)
    return (case.counts, case.cap, case.tail, case.dup3, case.seed)


@functools.lru_cache(maxsize=None)
def _graphs(gkey):
    """(edge_index, x, edge_attr, hubs, start, the generator's state behind them) of a graph key."""
    counts, cap, tails, dup3, seed = gkey
    g = torch.Generator().manual_seed(7000 + seed)
    src, dst, hubs, starts, base = [], [], [], [], 0
    for k, n in enumerate(counts):
        tail = k in tails
        edges, hub = _graph(n, cap, n - 1 if tail else n // 2, tail, g)
        if dup3:
            edges = [e for j, e in enumerate(edges) for _ in range(2 if j % 3 == 0 else 1)]
        src += [a + base for a, _ in edges]
        dst += [b + base for _, b in edges]
        hubs.append(hub + base)
        starts.append(base)
        base += n
    ei = torch.tensor([src, dst], dtype=torch.int64)
    x, ea = _draw(g, base, 8), _draw(g, ei.size(1), 6)
    return ei, x, ea, tuple(hubs), tuple(starts), g.get_state()


def _draw(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64).float().double()      # (fp32 values, held in fp64)


@functools.lru_cache(maxsize=None)
def _batch(gkey, dim_out):
    ei, x, ea, hubs, starts, state = _graphs(gkey)
    g = torch.Generator()
    g.set_state(state)                      # gout comes behind x and edge_attr, whatever its width
    return dict(x=x, edge_index=ei, edge_attr=ea, gout=_draw(g, x.size(0), dim_out), hubs=hubs, start=starts)


def batch(key):
    """dict(x [N, 8] fp64, edge_index [2, E], edge_attr [E, 6] fp64, gout [N, dim_out] fp64, hubs (global row per graph), start (first row
    per graph)) of a case (or the name of one).  Built once and shared: nobody writes to it."""
    return _batch(graph_key(key), case_of(key).args[2])


def degrees(name):
    """Branches per node on the doubled list (a branch listed twice counts twice)."""
    b = batch(name)
    return torch.bincount(b["edge_index"].flatten(), minlength=b["x"].size(0))


# ------------------------------------------------------------------------------------------
# the oracle model
# ------------------------------------------------------------------------------------------
def oracle_model(case, dtype=torch.float64):
    """The oracle's model under the case's seed (its own initialisation), at dtype."""
    torch.manual_seed(100 + case.seed)
    return getattr(dss2_oracle, case.cls)(*case.args).to(dtype)


def oracle_run(case, dtype):
    """The oracle model at dtype on the CPU: dict(out, dx, grads {name: tensor})."""
    b = batch(case)
    m = oracle_model(case, dtype)
    x = b["x"].to(dtype).clone().requires_grad_(True)
    out = m(x, b["edge_index"], b["edge_attr"].to(dtype))
    out.backward(b["gout"].to(dtype))
    return dict(out=out.detach(), dx=x.grad, grads={k: p.grad for k, p in m.named_parameters()})


@functools.lru_cache(maxsize=None)
def reference(key):
    """The fp64 run of a case (or the name of one), computed once."""
    return oracle_run(case_of(key), torch.float64)


# ------------------------------------------------------------------------------------------
# structure and route without a device
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _topology_oracle(gkey, nrb):
    ei, x = _graphs(gkey)[:2]
    o = TopologyOracle(ei, x.size(0), nrb=nrb)
    return o if o.tiled else None


def topology_oracle(key, nrb=None):
    return _topology_oracle(graph_key(key), nrb)


def structure(name):
    o = topology_oracle(name)
    return (o.nrb, o.ntiles, o.ell, o.ellT, o.max_segment, int(degrees(name).min()))


def _tiling(o):
    """topology.Tiling with the oracle's arrays (on the CPU), filled as Topology._launch_tiles fills it."""
    if o is None:
        return None
    tm, seg = 32 * o.nrb, [b - a for a, b in zip(o.bounds[:-1], o.bounds[1:])]
    ell_staged = o.ell > 0 and o.ellT > 0
    return pkg().topology.Tiling(
        global_only=False, nrb=o.nrb, ntiles=o.ntiles, tile_start=o.tile_start, utilisation=o.utilisation, max_segment=o.max_segment,
        max_tile_rows=(tm // o.max_segment) * o.max_segment if min(seg) == o.max_segment else 0,
        max_nnz=o.max_deg * tm if ell_staged else o.max_nnz, max_nnzT=o.max_degT * tm if ell_staged else o.max_nnzT,
        ell=o.ell, ellT=o.ellT, ell_tiles=o.ell_tiles, ellT_tiles=o.ellT_tiles, ell_ent_tiles=o.ell_ent_tiles, ellT_ent_tiles=o.ellT_ent_tiles)


@functools.lru_cache(maxsize=None)
def _stub_topology(gkey):
    prim = _topology_oracle(gkey, None)
    return types.SimpleNamespace(tiling=_tiling(prim), N=prim.N, hint=None, device=None,
                                 tiles_for=functools.lru_cache(maxsize=None)(lambda nrb: _tiling(_topology_oracle(gkey, nrb))))


def stub_topology(key):
    """What the route predicates, stack.tiles_of and the weight-gradient geometry read of a Topology, from the oracle's numbers."""
    return _stub_topology(graph_key(key))


def blocks_of(case):
    """Stand-ins for the model's MPN blocks (the dimensions the route and the stack query read)."""
    fn, fe, nout, hid, L, K = case.args[:6]
    n = case.args[7] if case.cls in ("PFN", "SkipPFN") else 1
    skip_inner = case.cls in ("SkipMPN", "SkipPFN")
    return [types.SimpleNamespace(dim_hid=hid, n_gnn_layers=L, K=K, dim_featn=fn, dim_feate=fe, dropout_rate=0.0,
                                  dim_out=nout if b == n - 1 else fn, skip=skip_inner and (b < n - 1 or case.cls == "SkipMPN"))
            for b in range(n)]


def stack_supported(case):
    """stack.supported on the stand-in topology, for a chip of CUS compute units."""
    st = importlib.import_module(PKG_NAME + ".stack")
    keep = st._cu_count
    st._cu_count = lambda dev: CUS
    try:
        return st.supported(blocks_of(case), stub_topology(case)) is not None
    finally:
        st._cu_count = keep


def route_literal(case, need_dx, block_routes=None, topo=None):
    """The ROUTE entry of one run.  ``block_routes``: the BlockRoutes a forward stored (else route.block_route on the stand-in topology);
    ``topo``: the device Topology (else the stand-in)."""
    P = pkg()
    blocks = blocks_of(case)
    stub = stub_topology(case) if topo is None else topo
    ts = stub.tiling
    in_stack = len(blocks) > 1
    if block_routes is None:
        block_routes = [P.route.block_route(m, ts, bool(bi > 0 or need_dx), in_stack) for bi, m in enumerate(blocks)]
    rows = tuple(tuple(getattr(r, f) for f in ROUTE_FIELDS) for r in block_routes)
    hid, L, nmat = case.args[3], case.args[4], case.args[5] + 1
    b16 = int(P.flags.WGRAD_BF16)      # (as ops.wgrad_batched asks)
    wts = P.ops._wgrad_tiles(stub, nmat, hid, hid, b16)
    keep = torch.cuda.is_current_stream_capturing
    if topo is None:      # (no device to ask: nothing is being captured)
        torch.cuda.is_current_stream_capturing = lambda: False
    try:
        mode = P.ops._wgrad_mode(wts, nmat, b16)
    finally:
        torch.cuda.is_current_stream_capturing = keep
    wp = P.ops._wgrad_shape_plan(wts, nmat, hid, hid, mode, L - 1 if L - 1 >= 2 else 0)
    tiled = P.networks._edge_tiled(ts)[0]
    ep = P.ops.edge_plan(hid, ts.nrb, ts.ell if tiled else 0, ts.ellT if tiled else 0, need_dx)
    return (stack_supported(case) if topo is None else None, rows, (32 * wts.nrb, wp.kernel), (ep.fwd.family, ep.bwd.family, ep.bwd_src.family))


# ------------------------------------------------------------------------------------------
# the package's model of a case
# ------------------------------------------------------------------------------------------
def build_model(case):
    """The package's model with the oracle model's weights (float32, on the CPU)."""
    m = getattr(pkg(), case.cls)(*case.args)
    m.load_state_dict({k: v.float() for k, v in oracle_model(case).state_dict().items()}, strict=True)
    return m
